"""als_similar / als_similar_vectors on the GPU: cosine top-k of one side against itself.

Every expected value is tests/similar_cases.py:expected: the unit image in numpy float32, the rows without a
direction and the row itself dropped, oracle.cbind.recommend over the rest.  Ids and score bits are compared
for equality, in both tiers (ALBEDO_SIMILAR_TIER = scan, passes) unless a test says otherwise.  The contexts
are model-only with a few hundred rows unless a test says otherwise, and ALBEDO_QUERY_SLICE_ROWS = 256 makes
257 rows and more cross scan slices.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import spark_als as O
from tests import foldin_cases as FC
from tests import query_cases as QC
from tests import similar_cases as SC
from tests.test_gpu_audit import Ctx
from tests.test_gpu_foldin import _fp, fold, timing as fold_timing
from tests.test_gpu_query_topk import rv

pytestmark = pytest.mark.gpu

TIERS = ("scan", "passes")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("ALBEDO_QUERY_SLICE_ROWS", str(SC.SLICE_ROWS))
    monkeypatch.delenv("ALBEDO_SIMILAR_TIER", raising=False)
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)


class Model:
    """A model-only context holding the case's rows on `side` and `n_other` zero rows on the other side."""

    def __init__(self, lib, ids, F, side=1, n_other=1):
        from albedo_amd import _lib as L
        self.lib, self.L, self.side = lib, L, side
        ids = np.ascontiguousarray(ids, np.int32)
        F = np.ascontiguousarray(F, np.float32)
        self.k = k = F.shape[1]
        oi, of = np.arange(n_other, dtype=np.int32), np.zeros((n_other, k), np.float32)
        u, i = ((oi, of), (ids, F)) if side == 1 else ((ids, F), (oi, of))
        self.h = C.c_void_p()
        L.check(lib.als_model_create(k, u[0].size, L.ptr(u[0], C.c_int32) if u[0].size else None,
                                     L.ptr(u[1], C.c_float) if u[0].size else None, i[0].size,
                                     L.ptr(i[0], C.c_int32) if i[0].size else None,
                                     L.ptr(i[1], C.c_float) if i[0].size else None, -1, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.als_destroy(self.h)


def sim_rc(lib, h, side, k, subset=None, n=None, null=()):
    """The raw call: (rc, src ids, ids, scores)."""
    from albedo_amd import _lib as L
    if subset is not None:
        sub = np.ascontiguousarray(subset, np.int32)
        n = sub.size if n is None else n
    else:
        sub, n = None, int(lib.als_num_rows(h, side))
    m, kk = max(sub.size if sub is not None else n, 1), max(k, 1)  # an overridden n is never served: the arrays stay small
    src = np.full(m, 123456789, np.int32)
    ids = np.full((m, kk), 123456789, np.int32)
    sc = np.full((m, kk), 7.0, np.float32)
    rc = lib.als_similar(h, side, k, L.ptr(sub, C.c_int32) if sub is not None and sub.size else
                         (None if sub is None else L.ptr(np.zeros(1, np.int32), C.c_int32)), n,
                         None if "src" in null else L.ptr(src, C.c_int32), None if "ids" in null else L.ptr(ids, C.c_int32),
                         None if "sc" in null else L.ptr(sc, C.c_float))
    n = min(max(n, 0), m)
    return rc, src[:n], ids[:n], sc[:n]


def sim(lib, h, side, k, subset=None, null=()):
    from albedo_amd import _lib as L
    rc, src, ids, sc = sim_rc(lib, h, side, k, subset, null=null)
    L.check(rc)
    return src, ids, sc


def sv_rc(lib, h, side, q, k, excl=None, n_q=None, ptr=None, eids=None, null=()):
    from albedo_amd import _lib as L
    q = np.ascontiguousarray(q, np.float32)
    n_q = q.shape[0] if n_q is None else n_q
    if excl is not None and ptr is None:
        ptr, eids = QC.excl_csr(excl)
    if ptr is not None:
        ptr = np.ascontiguousarray(ptr, np.int64)
    if eids is not None:
        eids = np.ascontiguousarray(eids, np.int32)
    m = max(q.shape[0], 1)  # an overridden n_q is never served: the arrays stay small
    ids = np.full((m, max(k, 1)), 123456789, np.int32)
    sc = np.full((m, max(k, 1)), 7.0, np.float32)
    rc = lib.als_similar_vectors(h, side, k, n_q, None if "q" in null else L.ptr(q, C.c_float),
                                 L.ptr(ptr, C.c_int64) if ptr is not None else None,
                                 L.ptr(eids, C.c_int32) if eids is not None and eids.size and "eids" not in null else None,
                                 None if "ids" in null else L.ptr(ids, C.c_int32),
                                 None if "sc" in null else L.ptr(sc, C.c_float))
    return rc, ids[:min(max(n_q, 0), m)], sc[:min(max(n_q, 0), m)]


def sv(lib, h, side, q, k, excl=None):
    from albedo_amd import _lib as L
    rc, ids, sc = sv_rc(lib, h, side, q, k, excl)
    L.check(rc)
    return ids, sc


def stats(h):
    from albedo_amd import _lib as L
    return L.similar_stats(h).tolist()


@functools.lru_cache(maxsize=None)
def _want_random(n, k, rank):
    return SC.expected(SC.random_case(n, k, rank))


def compare(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: the src ids are not echoed"
    bad = [i for i in range(len(want[1])) if not SC.same((got[1][i], got[2][i]), (want[1][i], want[2][i]))]
    if bad:
        i = bad[0]
        print(f"SIMILAR {what}: row {i} (id {want[0][i]}) differs\n got  {got[1][i]}\n      {got[2][i]}\n"
              f" want {want[1][i]}\n      {want[2][i]}")
    assert not bad, f"{what}: {len(bad)} of {len(want[1])} lists differ, first row {bad[0]}"


def check_case(lib, monkeypatch, case, what, want=None, side=1, tiers=TIERS):
    """The case in each tier on one model; returns the model and the last result."""
    want = SC.expected(case) if want is None else want
    m = Model(lib, case["ids"], case["F"], side)
    got = None
    for t, tier in enumerate(TIERS):
        if tier not in tiers:
            continue
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        got = sim(lib, m.h, side, case["k"], case["subset"])
        compare(got, want, f"{what}, {tier} tier")
        st = stats(m.h)
        _, ok = SC.unit_image(case["F"])
        known = int(np.isin(want[0], case["ids"]).sum())
        assert st[:3] == [known, int((~ok).sum()), t], f"{what}, {tier} tier: stats {st}"
    return m, got


# ---- 1. sizes, ranks, k --------------------------------------------------------------------------------

@pytest.mark.parametrize("k", SC.KS)
@pytest.mark.parametrize("n", SC.SIZES)
def test_sizes(gpu_lib, monkeypatch, n, k):
    n = SC.size(n, k)
    check_case(gpu_lib, monkeypatch, SC.random_case(n, k, 6), f"n {n} k {k}", _want_random(n, k, 6))


@pytest.mark.parametrize("rank", SC.RANKS)
def test_ranks(gpu_lib, monkeypatch, rank):
    check_case(gpu_lib, monkeypatch, SC.random_case(300, 30, rank), f"rank {rank}", _want_random(300, 30, rank))


def test_user_side(gpu_lib, monkeypatch):
    check_case(gpu_lib, monkeypatch, SC.random_case(300, 30, 6), "user side", _want_random(300, 30, 6), side=0)


# ---- 2. self at the slice edges, ties, rows without a direction -----------------------------------------

def test_self_at_slice_edges(gpu_lib, monkeypatch):
    case = SC.edge_copy_case()
    _, got = check_case(gpu_lib, monkeypatch, case, "edge rows and their copies")
    for j, c in enumerate(case["pairs"].values()):
        assert got[1][j][0] == case["ids"][c] and got[0][j] not in got[1][j]


def test_ties_of_scaled_and_exact_copies(gpu_lib, monkeypatch):
    case = SC.tie_case()
    _, got = check_case(gpu_lib, monkeypatch, case, "ties")
    bid = case["ids"][case["block"]]
    assert got[1][0].tolist() == bid[:case["k"]].tolist()
    assert got[0][2] not in got[1][2] and np.isin(got[1][2], bid).all()
    assert all(np.unique(SC.bits(row)).size == 1 for row in got[2])  # one score a list, whatever f2j_sdot(u, u) is


@pytest.mark.parametrize("name", ["no_direction_case", "all_without_direction_case", "k_plus_one_directions_case"])
def test_rows_without_a_direction(gpu_lib, monkeypatch, name):
    case = getattr(SC, name)()
    _, ok = SC.unit_image(case["F"])
    m, got = check_case(gpu_lib, monkeypatch, case, name)
    assert not np.isin(got[1], case["ids"][~ok]).any()                   # never listed
    assert (got[1][~ok] == -1).all() and np.isnan(got[2][~ok]).all()      # their own lists: padding
    assert np.array_equal(got[0], case["ids"])                            # the id echoed
    assert stats(m.h)[1] == int((~ok).sum())


# ---- 3. the subset contract ----------------------------------------------------------------------------

def test_subset_contract(gpu_lib, monkeypatch):
    case = SC.subset_case()
    m, got = check_case(gpu_lib, monkeypatch, case, "subset")
    everything = SC.expected(dict(case, subset=None))
    for tier in TIERS:
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        compare(sim(gpu_lib, m.h, 1, case["k"]), everything, f"subset == NULL, {tier}")
        compare(sim(gpu_lib, m.h, 1, case["k"], case["ids"]), everything, f"the explicit ascending list, {tier}")
        src, ids, sc = sim(gpu_lib, m.h, 1, case["k"], case["subset"], null=("src",))
        assert SC.same((ids, sc), (got[1], got[2])) and (src == 123456789).all()   # src_ids_out == NULL
        rc, src, ids, sc = sim_rc(gpu_lib, m.h, 1, case["k"], np.zeros(0, np.int32))
        assert rc == 0 and ids.shape[0] == 0                                          # n_subset = 0
        only_unknown = sim(gpu_lib, m.h, 1, case["k"], case["unknown"])
        assert (only_unknown[1] == -1).all() and np.isnan(only_unknown[2]).all()
        assert stats(m.h)[0] == 0


# ---- 4. every kind of context, both sides --------------------------------------------------------------

def _fitted(lib, k=16, nonneg=False):
    """A context after two half-sweeps on the synthetic problem of smoke(): 600 users, 150 items."""
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(600, 150, 6000, seed=3))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(2)
    c = Ctx(lib, k, "varying", nonneg)
    c.ratings(d["user"], d["item"], d["rating"])
    init = (lambda n: np.abs(rng.standard_normal((n, k))).astype(np.float32)) if nonneg else \
        (lambda n: rng.standard_normal((n, k)).astype(np.float32))
    c.inject(0, B.user_ids, init(len(B.user_ids)))
    c.inject(1, B.item_ids, init(len(B.item_ids)))
    c.half(1)
    c.half(0)
    return c, B


def _check_ctx(lib, monkeypatch, h, side, ids, F, k, what, subset=None):
    want = SC.expected(dict(ids=ids, F=F, k=k, subset=subset))
    for tier in TIERS:
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        compare(sim(lib, h, side, k, subset), want, f"{what}, side {side}, {tier} tier")
    return want


@pytest.mark.parametrize("nonneg", [False, True])
def test_fitted_context_fork_and_model_only(gpu_lib, monkeypatch, nonneg):
    from albedo_amd import _lib as L
    c, B = _fitted(gpu_lib, nonneg=nonneg)
    U, V = c.factors(0), c.factors(1)
    if nonneg:
        assert (V >= 0).all() and (U >= 0).all()  # NNLS leaves exact zeros, which is what this fit is here for
        print(f"SIMILAR nonnegative fit: {np.mean(V == 0):.3f} of the item components and {np.mean(U == 0):.3f} of the "
              f"user components are exactly zero, {int((~V.any(axis=1)).sum())} + {int((~U.any(axis=1)).sum())} zero rows")
    _check_ctx(gpu_lib, monkeypatch, c.h, 1, B.item_ids, V, 30, "fitted")
    _check_ctx(gpu_lib, monkeypatch, c.h, 0, B.user_ids, U, 10, "fitted", B.user_ids[::7][::-1].copy())
    f = Ctx(gpu_lib, c.k, "varying", nonneg, parent=c)
    f.inject(0, B.user_ids, U)
    f.inject(1, B.item_ids, V)
    _check_ctx(gpu_lib, monkeypatch, f.h, 1, B.item_ids, V, 30, "fork")
    del f
    m = Model(gpu_lib, B.item_ids, V, 1, n_other=0)  # created with zero users
    assert gpu_lib.als_num_rows(m.h, 0) == 0
    _check_ctx(gpu_lib, monkeypatch, m.h, 1, B.item_ids, V, 30, "model-only, no users")
    rc, _, ids, sc = sim_rc(gpu_lib, m.h, 0, 5, np.array([1, 2], np.int32))  # the empty side: unknown ids
    assert rc == L.ALS_OK and (ids == -1).all() and np.isnan(sc).all()


# ---- 5. als_similar_vectors ----------------------------------------------------------------------------

def test_similar_vectors(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    case = SC.random_case(300, 30, 6)
    ids, F, k = case["ids"], case["F"], 30
    m = Model(gpu_lib, ids, F)
    rows = np.array([0, 17, 255, 256, 299])
    monkeypatch.setenv("ALBEDO_SIMILAR_TIER", "scan")
    by_row = sim(gpu_lib, m.h, 1, k, ids[rows])
    own = [ids[r:r + 1] for r in rows]
    got = sv(gpu_lib, m.h, 1, F[rows], k, own)
    assert SC.same(got, by_row[1:])                                   # the row's factor, its id excluded
    assert SC.same(got, SC.expected_vectors(ids, F, F[rows], k, own))
    assert SC.same(sv(gpu_lib, m.h, 1, 8 * F[rows], k, own), got)     # q and 8 q: identical bits
    st = stats(m.h)
    assert st[0] == rows.size and st[2] == 0
    # without the exclusion the row itself is listed, first
    plain = sv(gpu_lib, m.h, 1, F[rows], k)
    assert np.array_equal(plain[0][:, 0], ids[rows]) and SC.same(plain, SC.expected_vectors(ids, F, F[rows], k))
    # a zero or NaN q: all padding
    q = F[rows].copy()
    q[1] = 0
    q[3, 2] = np.nan
    q[4] = np.float32(2.0 ** 64)
    got = sv(gpu_lib, m.h, 1, q, k)
    assert (got[0][[1, 3, 4]] == -1).all() and np.isnan(got[1][[1, 3, 4]]).all() and (got[0][[0, 2]] != -1).all()
    assert SC.same(got, SC.expected_vectors(ids, F, q, k))
    # exclusion lists with copies and unknown ids
    top = plain[0]
    excl = [np.concatenate([top[j][:4], top[j][:4], [7777, -7777], top[j][10:12]]).astype(np.int32) for j in range(rows.size)]
    got = sv(gpu_lib, m.h, 1, F[rows], k, excl)
    assert SC.same(got, SC.expected_vectors(ids, F, F[rows], k, excl))
    assert not any(np.isin(got[0][j], excl[j]).any() for j in range(rows.size))
    # by hand: als_recommend_vectors on a model created from the unit image
    U, ok = SC.unit_image(F)
    assert ok.all()
    hand = Model(gpu_lib, ids, U)
    uq, _ = SC.unit_image(F[rows])
    assert SC.same(rv(gpu_lib, hand.h, 1, uq, k, excl), got)
    assert L.similar_timing(m.h)[3] > 0


# ---- 6. the tiers agree, repeatability -----------------------------------------------------------------

@pytest.mark.parametrize("rank,k", [(6, 30), (64, 64)])
def test_tiers_agree_on_1000_rows(gpu_lib, monkeypatch, rank, k):
    case = SC.random_case(1000, k, rank)
    m = Model(gpu_lib, case["ids"], case["F"])
    out = {}
    for t, tier in enumerate(TIERS):
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        out[tier] = sim(gpu_lib, m.h, 1, k)
        assert stats(m.h)[2] == t
        assert SC.same(sim(gpu_lib, m.h, 1, k)[1:], out[tier][1:])  # two calls, identical bits
    assert SC.same(out["scan"][1:], out["passes"][1:])
    compare(out["scan"], _want_random(1000, k, rank), "1000 rows")
    sub = case["ids"][::3][::-1].copy()
    for tier in TIERS:
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        out[tier] = sim(gpu_lib, m.h, 1, k, sub)
    assert SC.same(out["scan"][1:], out["passes"][1:])


def test_default_tier_follows_the_row_count(gpu_lib):
    case = SC.random_case(300, 30, 6)
    m = Model(gpu_lib, case["ids"], case["F"])
    sim(gpu_lib, m.h, 1, 30, case["ids"][:3])
    assert stats(m.h)[2] == 0  # a few rows: the scan


# ---- 7. read-only --------------------------------------------------------------------------------------

def _state(lib, c):
    from albedo_amd import _lib as L
    out = []
    for side in (0, 1):
        out.append(c.factors(side))
        g = np.zeros((c.k, c.k), np.float64)
        L.check(lib.als_get_gram(c.h, side, L.ptr(g, C.c_double)))
        b = np.zeros((c.k, c.k), np.float64)
        L.check(lib.als_get_basis(c.h, side, L.ptr(b, C.c_double)))
        t = np.zeros(L.ALS_T_COUNT, np.float64)
        L.check(lib.als_last_timings(c.h, side, L.ptr(t, C.c_double), L.ALS_T_COUNT))
        s = np.zeros(4, np.int64)
        L.check(lib.als_path_stats(c.h, side, L.ptr(s, C.c_int64)))
        out += [g, b, t, s]
    st = np.zeros(4, np.int64)
    L.check(lib.als_topk_stats(c.h, L.ptr(st, C.c_int64)))
    tm = np.zeros(5, np.float64)
    L.check(lib.als_topk_timing(c.h, L.ptr(tm, C.c_double)))
    us = np.zeros(4, np.int64)
    L.check(lib.als_recommend_unseen_stats(c.h, L.ptr(us, C.c_int64)))
    ut = np.zeros(5, np.float64)
    L.check(lib.als_recommend_unseen_timing(c.h, L.ptr(ut, C.c_double)))
    n = C.c_int64(-1)
    L.check(lib.als_topk_last_rescan(c.h, None, 0, C.byref(n)))
    return out + [st, tm, us, ut, L.recommend_vectors_timing(c.h), L.fold_in_timing(c.h), np.array([n.value])]


def test_model_is_untouched(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    c, B = _fitted(gpu_lib)
    # every counter the call must leave alone holds something first
    sub = np.ascontiguousarray(B.user_ids[:50])
    src, ids, sc = (np.empty(50, np.int32), np.empty((50, 10), np.int32), np.empty((50, 10), np.float32))
    L.check(gpu_lib.als_recommend(c.h, 0, 10, L.ptr(sub, C.c_int32), 50, L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32),
                                  L.ptr(sc, C.c_float)))
    L.check(gpu_lib.als_recommend_unseen(c.h, 0, 10, L.ptr(sub, C.c_int32), 50, L.ALS_EXCLUDE_RATINGS, 0, None, None,
                                         L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32), L.ptr(sc, C.c_float)))
    rv(gpu_lib, c.h, 1, c.factors(0)[:5], 10, [B.item_ids[:3]] * 5)
    row = np.repeat(np.array([900001, 900002], np.int32), 3)
    srcs = np.ascontiguousarray(B.item_ids[[1, 5, 9, 2, 5, 70]])
    fp = _fp(0.5, 10.0, True)
    first = fold(gpu_lib, c.h, 0, row, srcs, np.ones(6, np.float32), fp)
    assert fold_timing(gpu_lib, c.h)[1] > 0                 # the fold-in formed its Gram cache
    before = _state(gpu_lib, c)
    assert before[-7][0] > 0 and before[-5][0] > 0 and before[-3][3] > 0
    for tier in TIERS:
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        sim(gpu_lib, c.h, 1, 10)
        sim(gpu_lib, c.h, 0, 10, B.user_ids[:40])
        sv(gpu_lib, c.h, 1, c.factors(1)[:4], 10)
        after = _state(gpu_lib, c)
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), tier
    again = fold(gpu_lib, c.h, 0, row, srcs, np.ones(6, np.float32), fp)
    assert fold_timing(gpu_lib, c.h)[1] == 0.0              # the cache is still the factors' Gram
    assert np.array_equal(SC.bits(again[2]), SC.bits(first[2]))
    # a call between two half-sweeps leaves the fit bit-identical
    c2, _ = _fitted(gpu_lib)
    c.half(1)
    c2.half(1)
    assert np.array_equal(c.factors(1), c2.factors(1)) and np.array_equal(c.factors(0), c2.factors(0))
    # and the next call sees the new factors
    _check_ctx(gpu_lib, monkeypatch, c.h, 1, B.item_ids, c.factors(1), 10, "after the next half-sweep")


# ---- 8. errors -----------------------------------------------------------------------------------------

def test_error_codes(gpu_lib):
    from albedo_amd import _lib as L
    case = SC.random_case(300, 30, 6)
    m = Model(gpu_lib, case["ids"], case["F"])
    sub = case["ids"][:5]
    call = lambda **kw: sim_rc(gpu_lib, m.h, kw.pop("side", 1), kw.pop("k", 30), kw.pop("subset", sub), **kw)[0]
    assert call() == L.ALS_OK
    assert call(side=2) == L.ALS_E_INVALID_ARGUMENT and call(side=-1) == L.ALS_E_INVALID_ARGUMENT
    assert call(k=0) == L.ALS_E_INVALID_ARGUMENT and call(k=-3) == L.ALS_E_INVALID_ARGUMENT
    assert call(n=-1) == L.ALS_E_INVALID_ARGUMENT
    assert call(null=("ids",)) == L.ALS_E_INVALID_ARGUMENT and call(null=("sc",)) == L.ALS_E_INVALID_ARGUMENT
    assert call(null=("src",)) == L.ALS_OK
    assert gpu_lib.als_similar(None, 1, 30, None, 0, None, None, None) == L.ALS_E_INVALID_ARGUMENT
    assert call(k=65) == L.ALS_E_UNSUPPORTED and call(k=64) == L.ALS_OK
    assert call(n=2 ** 31) == L.ALS_E_UNSUPPORTED
    with pytest.raises(L.ALSError):
        L.check(call(k=65))
    q = case["F"][:3]
    vcall = lambda **kw: sv_rc(gpu_lib, m.h, kw.pop("side", 1), q, kw.pop("k", 30), **kw)[0]
    assert vcall() == L.ALS_OK
    assert vcall(side=2) == L.ALS_E_INVALID_ARGUMENT and vcall(k=0) == L.ALS_E_INVALID_ARGUMENT
    assert vcall(n_q=-1) == L.ALS_E_INVALID_ARGUMENT
    for name in ("q", "ids", "sc"):
        assert vcall(null=(name,)) == L.ALS_E_INVALID_ARGUMENT
    ptr, eids = QC.excl_csr([sub[:2], sub[:0], sub[1:4]])
    assert vcall(ptr=ptr, eids=eids) == L.ALS_OK
    assert vcall(ptr=ptr[::-1].copy(), eids=eids) == L.ALS_E_INVALID_ARGUMENT
    assert vcall(ptr=ptr - 1, eids=eids) == L.ALS_E_INVALID_ARGUMENT
    assert vcall(ptr=ptr, eids=eids, null=("eids",)) == L.ALS_E_INVALID_ARGUMENT
    assert vcall(ptr=np.array([0, 0, 0, 2 ** 31], np.int64), eids=eids) == L.ALS_E_UNSUPPORTED
    assert vcall(k=65) == L.ALS_E_UNSUPPORTED and vcall(n_q=2 ** 31) == L.ALS_E_UNSUPPORTED
    assert gpu_lib.als_similar_vectors(m.h, 1, 30, 0, None, None, None, None, None) == L.ALS_OK
    out4, i4 = np.zeros(4), np.zeros(4, np.int64)
    assert gpu_lib.als_similar_timing(m.h, None) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_similar_timing(None, L.ptr(out4, C.c_double)) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_similar_stats(m.h, None) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_similar_stats(None, L.ptr(i4, C.c_int64)) == L.ALS_E_INVALID_ARGUMENT
    # no factors on the side
    c = Ctx(gpu_lib, 6, "varying")
    assert sim_rc(gpu_lib, c.h, 1, 30, sub)[0] == L.ALS_E_STATE
    user, item, r, B = FC.data("varying")
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, FC.src_factors(6, len(B.user_ids)))
    assert sim_rc(gpu_lib, c.h, 1, 30, sub)[0] == L.ALS_E_STATE and sv_rc(gpu_lib, c.h, 1, q, 30)[0] == L.ALS_E_STATE
    assert sim_rc(gpu_lib, c.h, 0, 30, B.user_ids[:4])[0] == L.ALS_OK  # the users have factors: only that side is needed
    with pytest.raises(L.IllegalStateException):
        L.check(sim_rc(gpu_lib, c.h, 1, 30, sub)[0])


def test_sharded_context_is_unsupported(gpu_lib):
    from albedo_amd import _lib as L
    ar = L.ALLREDUCE_FN(lambda u, buf, n: 1)
    ag = L.ALLGATHER_FN(lambda u, buf, n: 1)
    c = Ctx(gpu_lib, 6, "varying")
    L.check(gpu_lib.als_comm_init_host(c.h, 0, 2, ar, ag, None))
    assert sim_rc(gpu_lib, c.h, 1, 5, np.array([1], np.int32))[0] == L.ALS_E_UNSUPPORTED
    assert "world" in gpu_lib.als_last_error().decode()
    assert sv_rc(gpu_lib, c.h, 1, np.zeros((2, 6), np.float32), 5)[0] == L.ALS_E_UNSUPPORTED
    del c


# ---- 9. Python -----------------------------------------------------------------------------------------

def test_python_surface(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import ALSModel
    from albedo_amd import persistence
    case = SC.no_direction_case()
    ids, F = case["ids"], case["F"]
    k = F.shape[1]
    path = str(tmp_path / "model")
    uid, U = np.arange(3, dtype=np.int32), np.eye(3, k, dtype=np.float32)
    persistence.save_als_model(path, "als_test", {"userCol": "u", "itemCol": "i", "predictionCol": "prediction",
                                                  "coldStartStrategy": "nan"}, k, (uid, U), (ids, F), False, 1 << 20)
    model = ALSModel.load(path)
    want = SC.expected(case)
    _, ok = SC.unit_image(F)
    for tier in TIERS:
        monkeypatch.setenv("ALBEDO_SIMILAR_TIER", tier)
        compare(model.similar_np(case["k"]), want, f"similar_np, {tier}")
        frame = model.similarItems(None, case["k"])                       # the catalogue, rows with a list
        assert list(frame.columns) == ["i", "similarities"]
        assert np.array_equal(frame["i"].to_numpy(), ids[ok])
        for j, lst in zip(np.flatnonzero(ok), frame["similarities"]):
            assert [i for i, _ in lst] == want[1][j].tolist()
            assert np.array_equal(SC.bits(np.array([s for _, s in lst], np.float32)), SC.bits(want[2][j]))
    sub = {"i": np.array([ids[7], ids[7], 4999999, ids[3], ids[1]], np.int64)}  # a copy, an unknown id, no direction
    frame = model.similarItems(sub, 4)
    assert np.array_equal(frame["i"].to_numpy(), np.sort(ids[[1, 7]]))
    users = model.similarUsers(None, 2)
    assert list(users.columns) == ["u", "similarities"] and len(users) == 3
    assert all(len(lst) == 2 and all(s == 0 for _, s in lst) for lst in users["similarities"])  # orthogonal users
    src, sid, ssc = model.similar_np(3, subset=[ids[9], 4999999, ids[9]], side="item")
    assert src.tolist() == [ids[9], 4999999, ids[9]] and (sid[1] == -1).all() and SC.same((sid[0], ssc[0]), (sid[2], ssc[2]))
    vi, vs = model.similar_vectors_np(F[[9]], 3, exclude=[[ids[9]]])
    assert SC.same((vi[0], vs[0]), (sid[0], ssc[0]))
    assert set(model.similar_timing()) == {"unit_image", "lists", "merge", "total"}
    assert set(model.similar_stats()) == {"rows", "no_direction", "tier", "rows_exact"}
    assert model.similar_stats()["no_direction"] == int((~ok).sum())
    with pytest.raises(ValueError):
        model.similar_vectors_np(F[:2, :-1], 3)
    with pytest.raises(ValueError):
        model.similar_np(3, side="repo")
