"""als_explain on the GPU: each rating's share of a fold-in row's score for a target, against the fp64 numpy
restatement tests/explain_cases.py:expected, by the rule tests/explain_cases.py:check_pair (TOL = 1e-10).

Measured on an MI355X over the fold-in ladder (new items from ~700 unit-row user factors, degrees 1..513, 10
targets per row, m = 10; modes varying / mixed / stars_signed), the worst |value - reference| / scale over the
modes per rank (the totals' |total - reference| / sum|e| are the same or smaller):

  rank    1        50       64       65       128      129      200      256
  worst   3.2e-16  2.1e-13  1.2e-14  1.0e-13  2.8e-13  1.8e-14  8.2e-13  3.9e-12

and in the new-users direction (7,000 pairs against 52 source rows) 8.0e-14 at rank 50 and 1.5e-13 at rank 128;
the tile, batch and list edges 8.4e-15, the contract case 5.8e-15.  The largest, 3.9e-12 (stars_signed, rank
256), is below 1e-10 / 16; on that case the reference's own two fp64 routes part by 5.6e-12
(tests/test_explain_cases.py).  The total against the fold-in's fp32 row uses at most 0.35 of its bound, against
the F2J score of als_recommend_vectors at most 0.07.  The run prints each figure (EXPLAIN ... worst value ...).
The independence, tie and read-only tests compare bits.
"""
import ctypes as C

import numpy as np
import pytest

from tests import explain_cases as XC
from tests import foldin_cases as FC
from tests import ladder as LD
from tests.test_gpu_audit import Ctx
from tests.test_gpu_foldin import _fp, _model_state, _src_ctx, fold

pytestmark = pytest.mark.gpu

TOL = XC.TOL
TB = XC.EXPLAIN_TB


def explain_rc(lib, h, side, row, src, r, pr, pt, m, fp=None, n=None, n_pairs=None):
    """The raw call: (rc, total, ids, contributions)."""
    from albedo_amd import _lib as L
    row, src = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(src, np.int32)
    r = np.ascontiguousarray(r, np.float32)
    pr, pt = np.ascontiguousarray(pr, np.int32), np.ascontiguousarray(pt, np.int32)
    n = row.size if n is None else n
    n_pairs = pr.size if n_pairs is None else n_pairs
    mm = max(int(m), 1)
    total = np.full(max(pr.size, 1), 7.0)
    ids = np.full((max(pr.size, 1), mm), 123456789, np.int32)
    val = np.full((max(pr.size, 1), mm), 7.0)
    rc = lib.als_explain(h, side, C.byref(fp) if fp is not None else None, n, L.ptr(row, C.c_int32),
                         L.ptr(src, C.c_int32), L.ptr(r, C.c_float), n_pairs, L.ptr(pr, C.c_int32), L.ptr(pt, C.c_int32),
                         int(m), L.ptr(total, C.c_double), L.ptr(ids, C.c_int32), L.ptr(val, C.c_double))
    return rc, total[:pr.size], ids[:pr.size], val[:pr.size]


def explain(lib, h, side, t, pairs, m, fp=None):
    from albedo_amd import _lib as L
    rc, total, ids, val = explain_rc(lib, h, side, *t, *pairs, m, fp)
    L.check(rc)
    return total, ids, val


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(a, b))


def take(got, idx):
    return tuple(a[idx] for a in got)


def _edge_ctx(lib, k=128):
    c, B, src_ids = _src_ctx(lib, "varying", k, 1)
    return c, src_ids, FC.src_factors(k, len(src_ids), seed=1), dict(reg=0.5, alpha=10.0, implicit=True)


def counted_pairs(t, src_ids, counts, seed=17):
    """Row j of the triples (ascending id) gets counts[j mod len(counts)] targets: one of its own sources, the
    rest drawn from src_ids."""
    rng = np.random.default_rng(seed)
    ids = np.unique(t[0])
    pr, pt = [], []
    for j, rid in enumerate(ids):
        n = counts[j % len(counts)]
        own = t[1][(t[0] == rid) & np.isin(t[1], src_ids)]
        tg = rng.choice(src_ids, n, replace=False)
        if own.size:
            tg[0] = own[0]
        pr.append(np.full(n, rid, np.int32))
        pt.append(tg.astype(np.int32))
    return np.concatenate(pr), np.concatenate(pt)


# ---- 1. ladder parity ---------------------------------------------------------------------------------

def _ladder(lib, monkeypatch, mode, k, side):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, B, _ = _src_ctx(lib, mode, k, side)
    src_ids, Y, t, pairs, kw = XC.ladder_case(mode, k, side)
    ref = XC.ladder_expected(mode, k, side)
    got = explain(lib, c.h, side, t, pairs, 10)
    what = f"{'items' if side == 1 else 'users'} {mode} k{k}"
    wv, wt = XC.check_all(got, ref, 10, TOL, what)
    print(f"EXPLAIN {what}: {pairs[0].size} pairs, worst value {wv:.3e} total {wt:.3e}")
    if mode == "varying" and k >= 50:  # tests/test_explain_cases.py: no gap below 1e-8·scale among the first 11
        assert np.array_equal(got[1], ref.ids), what
    return got, ref


@pytest.mark.parametrize("k", XC.RANKS)
@pytest.mark.parametrize("mode", XC.MODES)
def test_ladder_items_match_the_reference(gpu_lib, monkeypatch, mode, k):
    _ladder(gpu_lib, monkeypatch, mode, k, 1)


@pytest.mark.parametrize("k", [50, 128])
@pytest.mark.parametrize("mode", XC.MODES)
def test_ladder_users_match_the_reference(gpu_lib, monkeypatch, mode, k):
    _ladder(gpu_lib, monkeypatch, mode, k, 0)


# ---- 2. edges -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 63, 64])
def test_tile_batch_and_list_edges(gpu_lib, monkeypatch, m):
    """Degrees at the tile edges and 1; 1, TB - 1, TB, TB + 1 and 2 TB + 1 targets per row; m at its ends (64 is
    above the degrees 1, 31, 32 and 33)."""
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib)
    t = FC.degree_rows(FC.tile_degrees(128) + [1, 1, 33], src_ids)
    pairs = counted_pairs(t, src_ids, [1, TB - 1, TB, TB + 1, 2 * TB + 1])
    ref = XC.expected(Y, src_ids, *t, *pairs, m, **kw)
    got = explain(gpu_lib, c.h, 1, t, pairs, m)
    wv, wt = XC.check_all(got, ref, m, TOL, f"edges m{m}")
    print(f"EXPLAIN edges m{m}: {pairs[0].size} pairs, worst value {wv:.3e} total {wt:.3e}")
    assert np.array_equal(got[1], ref.ids)  # ratings of the `varying` kind
    if m == 64:
        assert np.isnan(got[2]).any() and not np.isnan(got[2][:, 0]).any()


def test_input_contract(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib)
    t = FC.contract_case(src_ids)
    pairs = XC.contract_pairs(src_ids)
    ref = XC.expected(Y, src_ids, *t, *pairs, 10, **kw)
    got = explain(gpu_lib, c.h, 1, t, pairs, 10)
    wv, wt = XC.check_all(got, ref, 10, TOL, "contract")
    print(f"EXPLAIN contract: {pairs[0].size} pairs, worst value {wv:.3e} total {wt:.3e}")
    total, ids, val = got
    p77 = pairs[0] == 77  # no surviving triple: +0.0 and padding
    assert p77.sum() >= 3 and np.all(total[p77].view(np.uint64) == 0) and np.all(ids[p77] == -1)
    cannot = np.array([f is None for f in ref.full])  # an unknown target, an unknown row
    assert cannot.sum() == 3 and np.isnan(total[cannot]).all() and np.all(ids[cannot] == -1)
    assert np.isnan(val[cannot]).all()
    p102 = (pairs[0] == 102) & (pairs[1] == src_ids[7])  # 64 copies of the target itself: entries of their own
    assert np.all(ids[p102] == src_ids[7]) and np.all(val[p102] == val[p102][:, :1])
    assert same_bits(take(got, [0]), take(got, [pairs[0].size - 1]))  # the same pair given twice
    # shuffled pairs: the same answers, each at its pair's slot
    p = np.random.default_rng(5).permutation(pairs[0].size)
    assert same_bits(explain(gpu_lib, c.h, 1, t, (pairs[0][p], pairs[1][p]), 10), take(got, p))
    # no triples: no pair can be explained; no pairs: nothing to do
    e, ef = np.zeros(0, np.int32), np.zeros(0, np.float32)
    rc, t0, i0, v0 = explain_rc(gpu_lib, c.h, 1, e, e, ef, *pairs, 10)
    assert rc == L.ALS_OK and np.isnan(t0).all() and np.all(i0 == -1) and np.isnan(v0).all()
    assert explain_rc(gpu_lib, c.h, 1, *t, e, e, 10)[0] == L.ALS_OK
    assert gpu_lib.als_explain(c.h, 1, None, 0, None, None, None, 0, None, None, 10, None, None, None) == L.ALS_OK


# ---- 3. independence, bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("k", [50, 128, 200])
def test_a_pair_does_not_depend_on_its_company(gpu_lib, monkeypatch, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib, k)
    t = FC.degree_rows([5, 40, 33, 1, 129, 64, 2, 70], src_ids, seed=6)
    pr, pt = counted_pairs(t, src_ids, [2 * TB + 1, 3, TB, 1, TB + 1])
    m = 12
    got = explain(gpu_lib, c.h, 1, t, (pr, pt), m)
    XC.check_all(got, XC.expected(Y, src_ids, *t, pr, pt, m, **kw), m, TOL, f"independence k{k}")
    assert same_bits(got, explain(gpu_lib, c.h, 1, t, (pr, pt), m)), "two calls"
    for rid in np.unique(pr):  # each row's pairs alone
        s = np.nonzero(pr == rid)[0]
        assert same_bits(explain(gpu_lib, c.h, 1, t, (pr[s], pt[s]), m), take(got, s)), f"row {rid} alone"
    for p in range(0, pr.size, 3):  # a pair alone: a batch of one, whatever its place in the full call's batches
        assert same_bits(explain(gpu_lib, c.h, 1, t, (pr[p:p + 1], pt[p:p + 1]), m), take(got, [p])), f"pair {p} alone"
    monkeypatch.setenv("ALBEDO_FOLD_WGS", "1")
    assert same_bits(explain(gpu_lib, c.h, 1, t, (pr, pt), m), got), "one workgroup"
    monkeypatch.delenv("ALBEDO_FOLD_WGS")
    o = np.random.default_rng(8).permutation(t[0].size)
    assert same_bits(explain(gpu_lib, c.h, 1, tuple(a[o] for a in t), (pr, pt), m), got), "shuffled triples"


# ---- 4. ties ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [50, 128, 256])
def test_equal_ratings_of_equal_rows_tie_to_the_bit(gpu_lib, monkeypatch, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib, k)
    Y = XC.tie_factors(Y)
    c.inject(0, src_ids, Y)
    t, pairs = XC.tie_case(src_ids)
    total, ids, val = got = explain(gpu_lib, c.h, 1, t, pairs, 20)
    XC.check_all(got, XC.expected(Y, src_ids, *t, *pairs, 20, **kw), 20, TOL, f"tie k{k}")
    a, b = src_ids[3], src_ids[11]
    for p in range(total.size):
        ia, ib = int(np.nonzero(ids[p] == a)[0][0]), int(np.nonzero(ids[p] == b)[0][0])
        assert ib == ia + 1 and val[p, ia].view(np.uint64) == val[p, ib].view(np.uint64) and val[p, ia] != 0.0


def test_zero_contributions_are_ordered_by_id(gpu_lib, monkeypatch):
    """stars_signed: a rating of 0 has w = 0 and contributes ±0.0, whichever sign the sum had; they tie."""
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "stars_signed", 50
    c, B, _ = _src_ctx(gpu_lib, mode, k, 1)
    src_ids, Y, t, (pr, pt), kw = XC.ladder_case(mode, k, 1)
    deg = dict(zip(*np.unique(t[0], return_counts=True)))
    s = np.nonzero([16 <= deg[r] <= 64 for r in pr.tolist()])[0]
    got = explain(gpu_lib, c.h, 1, t, (pr[s], pt[s]), 64)
    XC.check_all(got, XC.expected(Y, src_ids, *t, pr[s], pt[s], 64, **kw), 64, TOL, "zeros")
    total, ids, val = got
    seen = signs = 0
    for p in range(s.size):
        z = np.nonzero(val[p] == 0.0)[0]
        if z.size > 1:
            seen += 1
            signs += int(np.unique(np.signbit(val[p, z])).size == 2)
            assert np.all(np.diff(z) == 1) and np.all(np.diff(ids[p, z].astype(np.int64)) > 0)
    assert seen > 0
    print(f"EXPLAIN zeros: {seen} lists with tied zeros, {signs} of them with both signs")


# ---- 5. identities on the device ----------------------------------------------------------------------

@pytest.mark.parametrize("k", [50, 128])
def test_total_is_the_score_of_the_folded_in_row(gpu_lib, monkeypatch, k):
    """New users against the 52 items: the total against the fp64 dot of als_fold_in's fp32 row, and against
    the F2J score als_recommend_vectors lists for that row (every item is listed: 52 <= 64)."""
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode = "varying"
    c, B, _ = _src_ctx(gpu_lib, mode, k, 0)
    src_ids, Y, t, _, kw = XC.ladder_case(mode, k, 0)
    users = np.unique(t[0])[:40]
    keep = np.isin(t[0], users)
    t = tuple(a[keep] for a in t)
    ids, deg, X = fold(gpu_lib, c.h, 0, *t)
    assert np.array_equal(ids, users)
    dst, sc = L.recommend_vectors(c.h, L.ALS_ITEM, X, len(src_ids), k)
    assert not np.isnan(sc).any()
    pr, pt = np.repeat(users, len(src_ids)), dst.reshape(-1)
    total, _, _ = explain(gpu_lib, c.h, 0, t, (pr, pt), 1)
    ref = XC.expected(Y, src_ids, *t, pr, pt, 1, **kw)
    sum_e = np.array([np.sum(np.abs(f[1])) for f in ref.full])
    prod = np.repeat(X.astype(np.float64), len(src_ids), axis=0) * Y.astype(np.float64)[np.searchsorted(src_ids, pt)]
    dot, mag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    b1 = 2.0 ** -24 * mag + 1e-10 * sum_e
    b2 = (k + 1) * 2.0 ** -24 * mag + 1e-10 * sum_e
    d1, d2 = np.abs(total - dot), np.abs(total - sc.reshape(-1).astype(np.float64))
    print(f"EXPLAIN identity k{k}: worst ratio to the fold-in bound {np.max(d1 / b1):.3f}, to the F2J bound "
          f"{np.max(d2 / b2):.3f}")
    assert np.all(d1 <= b1) and np.all(d2 <= b2)


# ---- 6. read-only -------------------------------------------------------------------------------------

def test_model_is_untouched_and_the_gram_cache_follows_the_factors(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    implicit, alpha, reg = LD.MODES[mode]
    kw = dict(reg=reg, alpha=alpha, implicit=implicit)
    user, item, r, B = FC.data(mode)

    def start():
        c = Ctx(gpu_lib, k, mode)
        c.ratings(user, item, r)
        c.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids), seed=1))
        c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
        c.half(1)
        c.half(0)
        return c

    def counters(c):
        st = np.zeros(4, np.int64)
        L.check(gpu_lib.als_topk_stats(c.h, L.ptr(st, C.c_int64)))
        return _model_state(gpu_lib, c, k) + [L.fold_in_timing(c.h), L.fold_in_stats(c.h), st]

    c = start()
    keep = np.isin(user, np.unique(user)[:60])
    t = ((user[keep].astype(np.int64) + FC.ID_SHIFT).astype(np.int32), item[keep], r[keep])
    pairs = XC.pairs_for(t[0], t[1], B.item_ids, 6, 2)
    fold(gpu_lib, c.h, 0, *t)  # the fold-in's own timing and stats are then not all zero
    before = counters(c)
    assert before[-3][3] > 0.0
    got = explain(gpu_lib, c.h, 0, t, pairs, 10)
    tm = L.explain_timing(c.h)
    assert tm[1] == 0.0 and tm[0] > 0.0 and tm[2] > 0.0 and tm[3] >= tm[0] + tm[2]  # the fold-in formed the Gram
    assert all(np.array_equal(a, b) for a, b in zip(before, counters(c)))
    V1 = c.factors(1)
    XC.check_all(got, XC.expected(V1, B.item_ids, *t, *pairs, 10, **kw), 10, TOL, "after a sweep")
    # the item factors move: a stale Gram fails here, and this call forms the new one itself
    c.half(1)
    V2 = c.factors(1)
    assert not np.allclose(V1, V2, rtol=1e-3, atol=0)
    got2 = explain(gpu_lib, c.h, 0, t, pairs, 10)
    assert L.explain_timing(c.h)[1] > 0.0
    XC.check_all(got2, XC.expected(V2, B.item_ids, *t, *pairs, 10, **kw), 10, TOL, "after the next half")
    # an explanation between two halves leaves the fit bit-identical
    c2 = start()
    c2.half(1)
    assert np.array_equal(c2.factors(1), V2) and np.array_equal(c2.factors(0), c.factors(0))
    c.half(0)
    c2.half(0)
    assert np.array_equal(c2.factors(0), c.factors(0))


# ---- 7. model-only contexts and errors ----------------------------------------------------------------

def test_model_only_context_needs_its_parameters(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    implicit, alpha, reg = LD.MODES[mode]
    src_ids, Y, t, pairs, kw = XC.ladder_case(mode, k, 1)
    B = FC.data(mode)[3]
    V = FC.src_factors(k, len(B.item_ids), seed=0)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(k, len(B.user_ids), L.ptr(B.user_ids, C.c_int32), L.ptr(Y, C.c_float),
                                     len(B.item_ids), L.ptr(B.item_ids, C.c_int32), L.ptr(V, C.c_float), -1, C.byref(h)))
    try:
        got = explain(gpu_lib, h, 1, t, pairs, 10, fp=_fp(reg, alpha, implicit))
        XC.check_all(got, XC.ladder_expected(mode, k, 1), 10, TOL, "model-only context")
        assert explain_rc(gpu_lib, h, 1, *t, *pairs, 10)[0] == L.ALS_E_INVALID_ARGUMENT  # fp = NULL
        explain(gpu_lib, h, 1, t, pairs, 10, fp=_fp(reg, alpha, implicit))
        assert L.explain_timing(h)[1] == 0.0  # the Gram is formed once per context
    finally:
        gpu_lib.als_destroy(h)


def test_fork_explains_like_its_parent(gpu_lib, monkeypatch):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    c, B, src_ids = _src_ctx(gpu_lib, mode, k, 1)
    f = Ctx(gpu_lib, k, mode, parent=c)
    f.inject(0, src_ids, FC.src_factors(k, len(src_ids), seed=1))
    _, _, t, pairs, _ = XC.ladder_case(mode, k, 1)
    assert same_bits(explain(gpu_lib, c.h, 1, t, pairs, 10), explain(gpu_lib, f.h, 1, t, pairs, 10))
    del f


def test_error_codes(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 8
    user, item, r, B = FC.data(mode)
    t = FC.degree_rows([3, 4], B.user_ids)
    pairs = XC.pairs_for(t[0], t[1], B.user_ids, 2, 1)
    nn = Ctx(gpu_lib, k, mode, nonneg=True)
    nn.ratings(user, item, r)
    nn.inject(0, B.user_ids, np.abs(FC.src_factors(k, len(B.user_ids))))
    assert explain_rc(gpu_lib, nn.h, 1, *t, *pairs, 5)[0] == L.ALS_E_UNSUPPORTED  # fp = NULL, an NNLS context
    assert "not linear" in gpu_lib.als_last_error().decode()
    c = Ctx(gpu_lib, k, mode)
    c.ratings(user, item, r)
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 5)[0] == L.ALS_E_STATE  # no factors
    c.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids)))
    assert explain_rc(gpu_lib, c.h, 0, *t, *pairs, 5)[0] == L.ALS_E_STATE  # the item side still has none
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 5)[0] == L.ALS_OK
    nonneg = L.als_fold_params(0.5, 10.0, 1, 1)
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 5, fp=nonneg)[0] == L.ALS_E_UNSUPPORTED
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 65)[0] == L.ALS_E_UNSUPPORTED
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 64)[0] == L.ALS_OK
    for m in (0, -1):
        assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, m)[0] == L.ALS_E_INVALID_ARGUMENT
    for side in (2, -1):
        assert explain_rc(gpu_lib, c.h, side, *t, *pairs, 5)[0] == L.ALS_E_INVALID_ARGUMENT
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 5, n=-1)[0] == L.ALS_E_INVALID_ARGUMENT
    assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 5, n_pairs=-1)[0] == L.ALS_E_INVALID_ARGUMENT
    for fp in (_fp(float("nan"), 1.0, True), _fp(-0.5, 1.0, True), _fp(0.5, -1.0, True), _fp(0.5, float("nan"), True)):
        assert explain_rc(gpu_lib, c.h, 1, *t, *pairs, 5, fp=fp)[0] == L.ALS_E_INVALID_ARGUMENT
    row, src, rr = (np.ascontiguousarray(a) for a in t)
    pr, pt = (np.ascontiguousarray(a) for a in pairs)
    tot, ids, val = np.zeros(pr.size), np.zeros((pr.size, 5), np.int32), np.zeros((pr.size, 5))
    P = L.ptr
    full = [c.h, 1, None, row.size, P(row, C.c_int32), P(src, C.c_int32), P(rr, C.c_float), pr.size, P(pr, C.c_int32),
            P(pt, C.c_int32), 5, P(tot, C.c_double), P(ids, C.c_int32), P(val, C.c_double)]
    assert gpu_lib.als_explain(*full) == L.ALS_OK
    for null in (4, 5, 6, 8, 9, 11, 12, 13):  # each array in turn
        a = list(full)
        a[null] = None
        assert gpu_lib.als_explain(*a) == L.ALS_E_INVALID_ARGUMENT, null
    assert gpu_lib.als_explain_timing(c.h, None) == L.ALS_E_INVALID_ARGUMENT


@pytest.mark.parametrize("implicit", [True, False])
def test_singular_row_fails_only_when_a_pair_names_it(gpu_lib, monkeypatch, implicit):
    """regParam = 0 on a rank-deficient source side: the kernel's flag word, not a fault."""
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    src_ids, Y, row, src, r = FC.singular_case()
    k = Y.shape[1]
    item_ids = np.array([1, 2], np.int32)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(k, 3, L.ptr(src_ids, C.c_int32), L.ptr(Y, C.c_float), 2, L.ptr(item_ids, C.c_int32),
                                     L.ptr(np.zeros((2, k), np.float32), C.c_float), -1, C.byref(h)))
    try:
        # a second failing row with a higher id and a degree-0 row with a lower one: the lowest failing id is named
        rows = np.concatenate([row, row + 1, [5]]).astype(np.int32)
        srcs = np.concatenate([src, src, [99999]]).astype(np.int32)
        rs = np.concatenate([r, r, [1.0]]).astype(np.float32)
        pr = np.array([row[0] + 1, row[0], 5], np.int32)
        pt = np.array([10, 20, 30], np.int32)
        rc = explain_rc(gpu_lib, h, 1, rows, srcs, rs, pr, pt, 3, fp=_fp(0.0, 1.0, implicit))[0]
        assert rc == L.ALS_E_NOT_POSITIVE_DEFINITE
        msg = gpu_lib.als_last_error().decode()
        assert str(int(row[0])) in msg and str(int(row[0]) + 1) not in msg
        # the same triples with no pair on a singular row
        rc, total, ids, val = explain_rc(gpu_lib, h, 1, rows, srcs, rs, pr[2:], pt[2:], 3, fp=_fp(0.0, 1.0, implicit))
        assert rc == L.ALS_OK and total[0] == 0.0 and np.all(ids == -1)
        kw = dict(reg=0.5, alpha=1.0, implicit=implicit)  # the context still serves
        got = explain(gpu_lib, h, 1, (rows, srcs, rs), (pr, pt), 3, fp=_fp(0.5, 1.0, implicit))
        XC.check_all(got, XC.expected(Y, src_ids, rows, srcs, rs, pr, pt, 3, **kw), 3, TOL, "regularised")
    finally:
        gpu_lib.als_destroy(h)


# ---- 8. Python ----------------------------------------------------------------------------------------

def test_facade_explain_and_recommend_for_new_users(gpu_lib, monkeypatch):
    from albedo_amd import ALS
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    user, item, r, B = FC.data("varying")
    k, reg, alpha = 16, 0.5, 10.0
    kw = dict(reg=reg, alpha=alpha, implicit=True)
    model = ALS(rank=k, maxIter=1, regParam=reg, alpha=alpha, implicitPrefs=True, seed=3, userCol="u", itemCol="i",
                ratingCol="r").fit({"u": user, "i": item, "r": r})
    iid, V = model.item_factors_np()
    new = np.unique(user)[:40]
    keep = np.isin(user, new)
    nu, ni, nr = (user[keep].astype(np.int64) + FC.ID_SHIFT).astype(np.int32), item[keep], r[keep]
    ds = {"u": nu, "i": ni, "r": nr}
    pr, pt = XC.pairs_for(nu, ni, iid, 3, 1)
    ref = XC.expected(V, iid, nu, ni, nr, pr, pt, 4, **kw)
    frame = model.explain({"u": pr, "i": pt}, ds, num=4)
    assert list(frame.columns) == ["u", "i", "score", "explanation"] and len(frame) == pr.size
    assert np.array_equal(frame["u"].to_numpy(), pr) and np.array_equal(frame["i"].to_numpy(), pt)
    got_np = model.explain_np(nu, ni, nr, pr, pt, 4)
    XC.check_all(got_np, ref, 4, TOL, "explain_np")
    assert np.array_equal(frame["score"].to_numpy(), got_np[0])
    for p, lst in enumerate(frame["explanation"]):
        n = int(np.sum(~np.isnan(got_np[2][p])))
        assert lst == [(int(i), float(v)) for i, v in zip(got_np[1][p][:n], got_np[2][p][:n])] and 0 < len(lst) <= 4
    assert set(model.explain_timing()) == {"csr", "gram", "solve", "total"}
    # dataset=None: the model's own ratings of the rows it was fitted on
    known = np.unique(user)[:5]
    kp = (np.repeat(known, 2), np.tile(iid[:2], known.size))
    own = model.explain({"u": kp[0], "i": kp[1]}, num=4)
    m = np.isin(user, known)
    want = XC.expected(V, iid, user[m], item[m], r[m], *kp, 4, **kw)
    XC.check_all((own["score"].to_numpy(), *model.explain_np(user[m], item[m], r[m], *kp, 4)[1:]), want, 4, TOL, "own")
    # recommendForNewUsers(explain=5): the default frame and, per listed item, its total and explanation
    plain = model.recommendForNewUsers(ds, 7)
    recs = model.recommendForNewUsers(ds, 7, explain=5)
    assert list(plain.columns) == ["u", "recommendations"] and list(recs.columns) == ["u", "recommendations", "explanation"]
    assert plain.equals(recs[["u", "recommendations"]])
    users = recs["u"].to_numpy()
    lp = np.repeat(users, 7)
    lt = np.array([i for lst in recs["recommendations"] for i, _ in lst], np.int32)
    total, eids, ev = model.explain_np(nu, ni, nr, lp, lt, 5)
    full = XC.expected(V, iid, nu, ni, nr, lp, lt, 5, **kw)
    XC.check_all((total, eids, ev), full, 5, TOL, "listed items")
    ids_f, _, X = model.fold_in_np(nu, ni, nr)
    at = 0
    for j, (lst, ex) in enumerate(zip(recs["recommendations"], recs["explanation"])):
        assert [d["i"] for d in ex] == [i for i, _ in lst]
        x = X[np.searchsorted(ids_f, users[j])].astype(np.float64)
        for (i, s), d in zip(lst, ex):
            assert d["score"] == total[at]
            mag = float(np.sum(np.abs(x * V[np.searchsorted(iid, i)].astype(np.float64))))
            assert abs(d["score"] - s) <= (k + 1) * 2.0 ** -24 * mag + 1e-10 * float(np.sum(np.abs(full.full[at][1])))
            n = int(np.sum(~np.isnan(ev[at])))
            assert d["explanation"] == [(int(a), float(b)) for a, b in zip(eids[at][:n], ev[at][:n])]
            at += 1
