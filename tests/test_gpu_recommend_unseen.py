"""als_recommend_unseen on the GPU: bulk top-k that leaves out each src row's known pairs.

Every expected value is tests/unseen_cases.py:expected, the C oracle over the dst rows left (through
tests/query_cases.expected); ids and score bits are compared for equality.  Every context holds the case's known
pairs as its ratings and the case's factors, injected: there is no fit.  ALBEDO_UNSEEN_DEPTH is 64, the depth
the cases are designed at (tests/unseen_cases.py DEPTH), unless a test sets it: the designed tier-2 counts are
those of that depth.  The depth test also runs the engine's default.
"""
import ctypes as C

import numpy as np
import pytest

from tests import query_cases as QC
from tests import unseen_cases as UC
from tests.test_gpu_audit import Ctx

pytestmark = pytest.mark.gpu

RATINGS, PAIRS = 0, 1
DEFAULT_DEPTH = 48  # topk_host.cpp unseen_depth


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for name in ("ALBEDO_TOPK_PASS", "ALBEDO_QUERY_SLICE_ROWS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ALBEDO_UNSEEN_DEPTH", str(UC.DEPTH))


def context(lib, case, side=0, ratings=None):
    """A context whose ratings are the case's known pairs (src rows on `side`) and whose factors are the case's."""
    c = Ctx(lib, case["U"].shape[1], "varying")
    c.ratings(*(UC.ratings(case, side) if ratings is None else ratings))
    c.inject(side, case["src_ids"], case["U"])
    c.inject(1 - side, case["dst_ids"], case["V"])
    return c


def model_only(lib, case, side=0):
    from albedo_amd import _lib as L
    u, i = ((case["src_ids"], case["U"]), (case["dst_ids"], case["V"]))[::1 if side == 0 else -1]
    h = C.c_void_p()
    L.check(lib.als_model_create(case["U"].shape[1], u[0].size, L.ptr(u[0], C.c_int32), L.ptr(u[1], C.c_float), i[0].size,
                                 L.ptr(i[0], C.c_int32), L.ptr(i[1], C.c_float), -1, C.byref(h)))
    return h


def unseen_rc(lib, h, side, k, subset=None, pairs=None, n_rows=None, n_subset=None, n_excl=None, mode=None, null=()):
    """The raw call: (rc, src ids, ids, scores).  pairs: (src ids, dst ids) selects the pairs mode."""
    from albedo_amd import _lib as L
    sub = None if subset is None else np.ascontiguousarray(subset, np.int32)
    n = (lib.als_num_rows(h, side) if n_rows is None else n_rows) if sub is None else sub.size
    es = ed = None
    if pairs is not None:
        es, ed = (np.ascontiguousarray(a, np.int32) for a in pairs)
    mode = (RATINGS if pairs is None else PAIRS) if mode is None else mode
    n_excl = (0 if es is None else es.size) if n_excl is None else n_excl
    kk = max(k, 1)
    src = np.full(max(n, 1), 123456789, np.int32)
    ids = np.full((max(n, 1), kk), 123456789, np.int32)
    sc = np.full((max(n, 1), kk), 7.0, np.float32)
    rc = lib.als_recommend_unseen(h, side, k, L.ptr(sub, C.c_int32) if sub is not None else None,
                                  (n if sub is not None else 0) if n_subset is None else n_subset, mode, n_excl,
                                  L.ptr(es, C.c_int32) if es is not None and "es" not in null else None,
                                  L.ptr(ed, C.c_int32) if ed is not None and "ed" not in null else None,
                                  None if "src" in null else L.ptr(src, C.c_int32),
                                  None if "ids" in null else L.ptr(ids, C.c_int32),
                                  None if "sc" in null else L.ptr(sc, C.c_float))
    return rc, src[:n], ids[:n], sc[:n]


def unseen(lib, h, side, k, subset=None, pairs=None):
    from albedo_amd import _lib as L
    rc, src, ids, sc = unseen_rc(lib, h, side, k, subset, pairs)
    L.check(rc)
    return src, ids, sc


def stats(lib, h):
    from albedo_amd import _lib as L
    out = np.zeros(4, np.int64)
    L.check(lib.als_recommend_unseen_stats(h, L.ptr(out, C.c_int64)))
    return out


def timing(lib, h):
    from albedo_amd import _lib as L
    out = np.zeros(5, np.float64)
    L.check(lib.als_recommend_unseen_timing(h, L.ptr(out, C.c_double)))
    return out


def assert_same(got, want, what):
    bad = [i for i in range(len(want[0])) if not QC.same((got[0][i], got[1][i]), (want[0][i], want[1][i]))]
    if bad:
        i = bad[0]
        print(f"UNSEEN {what}: row {i} differs\n got  {got[0][i]}\n      {got[1][i]}\n want {want[0][i]}\n      {want[1][i]}")
    assert not bad, f"{what}: {len(bad)} of {len(want[0])} lists differ, first row {bad[0]}"


def check(lib, c, case, k, what, side=0, tier2=None, pairs=None):
    src, ids, sc = unseen(lib, c.h if isinstance(c, Ctx) else c, side, k, pairs=pairs)
    assert np.array_equal(src, case["src_ids"])
    assert_same((ids, sc), UC.expected(case, k), what)
    st = stats(lib, c.h if isinstance(c, Ctx) else c)
    print(f"UNSEEN {what}: stats {st.tolist()}")
    assert st[0] == len(case["src_ids"])
    if tier2 is not None:
        assert st[1] == tier2, f"{what}: {st[1]} rows through the exact scan, {tier2} designed"
    return (ids, sc), st


# ---- 1. the ladder ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("rank", UC.RANKS)
def test_ladder(gpu_lib, rank, side):
    from albedo_amd import _lib as L
    case = UC.ladder(rank)
    c = context(gpu_lib, case, side)
    excl = [case["dst_ids"][e] for e in case["E"]]
    for k in UC.KS:
        n2 = len(UC.tier2_rows(case, UC.DEPTH, k))
        if k == UC.K:
            assert n2 == len(UC.designed_tier2(case)) and 0 < n2 < len(case["src_ids"])
        got, st = check(gpu_lib, c, case, k, f"ladder rank {rank} side {side} k {k}", side, tier2=n2)
        assert st[2] > 0 and (n2 == 0 or st[3] > 0)
        # the same lists from the only other exact route: each row's factor as a query with its list
        rv = L.recommend_vectors(c.h, 1 - side, c.factors(side), k, rank, excl)
        assert QC.same(got, rv), f"rank {rank} side {side} k {k}: als_recommend_vectors differs"


# ---- 2. sizes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", [(n, k) for k in (1, 30, 64) for n in UC.SIZES if UC.size(n, k) >= 1])  # k - 1 = 0: no catalogue
def test_dst_sizes(gpu_lib, n, k):
    n_dst = UC.size(n, k)
    case = UC.sizes(n_dst, k)
    n2 = len(UC.tier2_rows(case, UC.DEPTH, k))
    assert n_dst > UC.DEPTH or n2 == 0  # every dst row is in the list: certified without tier 2
    check(gpu_lib, context(gpu_lib, case), case, k, f"n_dst {n_dst} k {k}", tier2=n2)


# ---- 3. ties ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tie_groups", "mass_tie", "zeros_and_negatives"])
def test_ties_zeros_negatives(gpu_lib, name):
    case = getattr(UC, name)()
    c = context(gpu_lib, case)
    for k in (UC.K, 64):
        check(gpu_lib, c, case, k, f"{name} k {k}", tier2=len(UC.tier2_rows(case, UC.DEPTH, k)))


# ---- 4. pruning ------------------------------------------------------------------------------------------

def test_exact_scan_prunes(gpu_lib):
    case = UC.pruning()
    n_src, n_dst = len(case["src_ids"]), len(case["dst_ids"])
    _, st = check(gpu_lib, context(gpu_lib, case), case, UC.K, "pruning", tier2=n_src)
    assert 0 < st[3] < st[1] * n_dst, f"the exact scan scored {st[3]} of {st[1] * n_dst} dst rows"


# ---- 5. passes -------------------------------------------------------------------------------------------

def test_two_passes(gpu_lib, monkeypatch):
    monkeypatch.setenv("ALBEDO_TOPK_PASS", "65536")
    case = UC.passes()
    c = context(gpu_lib, case)
    src, ids, sc = unseen(gpu_lib, c.h, 0, UC.K)
    assert np.array_equal(src, case["src_ids"])
    assert_same((ids, sc), UC.expected_fast(case, UC.K), "two passes")
    st = stats(gpu_lib, c.h)
    assert st[0] == len(src) and st[1] == len(UC.tier2_rows(case, UC.DEPTH, UC.K)) > 0


# ---- 6. modes, subsets, ids ------------------------------------------------------------------------------

def test_modes_give_identical_bits(gpu_lib):
    from albedo_amd import _lib as L
    case = UC.ladder(50)
    k, rng = UC.K, np.random.default_rng(5)
    c = context(gpu_lib, case)
    want = UC.expected(case, k)
    base, _ = check(gpu_lib, c, case, k, "ratings mode")
    es, ed = UC.pairs(case)
    pairs_got, _ = check(gpu_lib, c, case, k, "pairs mode", pairs=(es, ed), tier2=len(UC.designed_tier2(case)))
    assert QC.same(pairs_got, base)
    assert timing(gpu_lib, c.h)[0] > 0
    # shuffled, repeated and unknown pairs
    unknown = (np.array([7777777, es[0], 7777777], np.int32), np.array([ed[0], 8888888, 8888888], np.int32))
    assert not np.isin(unknown[0][[0]], case["src_ids"]).any() and not np.isin(unknown[1][[1]], case["dst_ids"]).any()
    p = rng.permutation(2 * es.size + 3)
    messy = (np.concatenate([es, es, unknown[0]])[p], np.concatenate([ed, ed, unknown[1]])[p])
    assert QC.same(unseen(gpu_lib, c.h, 0, k, pairs=messy)[1:], base)
    # a model-only context serves the pairs mode, and refuses the ratings mode
    h = model_only(gpu_lib, case)
    try:
        assert QC.same(unseen(gpu_lib, h, 0, k, pairs=(es, ed))[1:], base)
        assert unseen_rc(gpu_lib, h, 0, k)[0] == L.ALS_E_STATE
    finally:
        gpu_lib.als_destroy(h)
    # ratings with copies of a pair and with ratings <= 0: known pairs all the same
    u, i, r = UC.ratings(case)
    u2, i2 = np.concatenate([u, u[:50]]), np.concatenate([i, i[:50]])
    r2 = np.concatenate([r, r[:50]])
    r2[::3] = 0.0
    r2[1::3] = -r2[1::3]
    c2 = context(gpu_lib, case, ratings=(u2, i2, r2))
    assert QC.same(unseen(gpu_lib, c2.h, 0, k)[1:], base)
    # unsorted subsets with repeated and unknown ids
    ids = case["src_ids"]
    sub = np.concatenate([ids[[40, 3, 3, 69, 0]], [5555555], ids[[17]], [-5555555], ids[[3]]]).astype(np.int32)
    assert not np.isin([5555555, -5555555], ids).any()
    for pairs in (None, (es, ed)):
        src, gi, gs = unseen(gpu_lib, c.h, 0, k, subset=sub, pairs=pairs)
        assert np.array_equal(src, sub)
        for j, s in enumerate(sub):
            row = np.searchsorted(ids, s)
            if row < ids.size and ids[row] == s:
                assert QC.same((gi[j], gs[j]), (want[0][row], want[1][row])), f"subset entry {j}"
            else:
                assert (gi[j] == -1).all() and np.isnan(gs[j]).all()
        assert stats(gpu_lib, c.h)[0] == 7
    # a fork views its parent's ratings
    f = Ctx(gpu_lib, 50, "varying", parent=c)
    f.inject(0, case["src_ids"], case["U"])
    f.inject(1, case["dst_ids"], case["V"])
    assert QC.same(unseen(gpu_lib, f.h, 0, k)[1:], base)
    del f


def test_ids_at_the_int32_edges(gpu_lib):
    case = UC.edge_ids(UC.ladder(3))
    c = context(gpu_lib, case)
    got, _ = check(gpu_lib, c, case, UC.K, "edge ids, ratings")
    assert QC.same(unseen(gpu_lib, c.h, 0, UC.K, pairs=UC.pairs(case))[1:], got)
    assert QC.I32_MIN in got[0] or QC.I32_MAX in got[0]


# ---- 7. the depth knob -----------------------------------------------------------------------------------

def test_depth_cannot_change_a_result(gpu_lib, monkeypatch):
    case = UC.ladder(100)
    c = context(gpu_lib, case)
    k = UC.K
    monkeypatch.delenv("ALBEDO_UNSEEN_DEPTH")
    base, _ = check(gpu_lib, c, case, k, "default depth", tier2=len(UC.designed_tier2(case, DEFAULT_DEPTH, k)))
    seen = []
    for depth in (k, 48, 64, 1, 1000):
        monkeypatch.setenv("ALBEDO_UNSEEN_DEPTH", str(depth))
        used = min(max(depth, k), 64)
        n2 = len(UC.designed_tier2(case, used, k))
        assert n2 == len(UC.tier2_rows(case, used, k))
        got, _ = check(gpu_lib, c, case, k, f"depth {depth}", tier2=n2)
        assert QC.same(got, base)
        seen.append(n2)
    assert seen[0] > seen[1] > seen[2] > 0 and seen[3] == seen[0] and seen[4] == seen[2]


# ---- 8. cross-checks -------------------------------------------------------------------------------------

def test_no_exclusions_equal_als_recommend_and_calls_repeat(gpu_lib):
    from albedo_amd import _lib as L
    case = UC.ladder(50)
    c = context(gpu_lib, case)
    for side in (0, 1):
        n = gpu_lib.als_num_rows(c.h, side)
        for k in (1, UC.K, 64):
            src, ids, sc = (np.empty(n, np.int32), np.empty((n, k), np.int32), np.empty((n, k), np.float32))
            L.check(gpu_lib.als_recommend(c.h, side, k, None, 0, L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32),
                                          L.ptr(sc, C.c_float)))
            empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
            got = unseen(gpu_lib, c.h, side, k, pairs=empty)
            assert np.array_equal(got[0], src) and QC.same(got[1:], (ids, sc)), f"side {side} k {k}"
            assert stats(gpu_lib, c.h)[1:].tolist() == [0, 0, 0] and timing(gpu_lib, c.h)[0] == 0.0
    a = unseen(gpu_lib, c.h, 0, UC.K)
    b = unseen(gpu_lib, c.h, 0, UC.K)
    assert QC.same(a[1:], b[1:])
    t = timing(gpu_lib, c.h)
    assert t[0] == 0.0 and t[1] > 0 and t[2] > 0 and t[3] > 0 and t[4] >= t[1] + t[2] + t[3] - 1e-3


# ---- 9. read-only ----------------------------------------------------------------------------------------

def _state(lib, c):
    from albedo_amd import _lib as L
    out = []
    for side in (0, 1):
        out.append(c.factors(side))
        b = np.zeros((c.k, c.k), np.float64)
        L.check(lib.als_get_basis(c.h, side, L.ptr(b, C.c_double)))
        t = np.zeros(L.ALS_T_COUNT, np.float64)
        L.check(lib.als_last_timings(c.h, side, L.ptr(t, C.c_double), L.ALS_T_COUNT))
        s = np.zeros(4, np.int64)
        L.check(lib.als_path_stats(c.h, side, L.ptr(s, C.c_int64)))
        out += [b, t, s]
    out += [L.fold_in_timing(c.h), L.explain_timing(c.h), L.recommend_vectors_timing(c.h)]
    return out


def _topk_counters(lib, c):
    from albedo_amd import _lib as L
    st, tm = np.zeros(4, np.int64), np.zeros(5, np.float64)
    L.check(lib.als_topk_stats(c.h, L.ptr(st, C.c_int64)))
    L.check(lib.als_topk_timing(c.h, L.ptr(tm, C.c_double)))
    return st, tm


def test_model_is_untouched(gpu_lib):
    case = UC.ladder(50)
    c, c2 = context(gpu_lib, case), context(gpu_lib, case)
    c.half(1)
    c2.half(1)
    before, counters = _state(gpu_lib, c), _topk_counters(gpu_lib, c)
    unseen(gpu_lib, c.h, 0, UC.K)
    unseen(gpu_lib, c.h, 1, 7, pairs=UC.pairs(case)[::-1])
    after, counters2 = _state(gpu_lib, c), _topk_counters(gpu_lib, c)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert counters2[0][0] > counters[0][0] and counters2[1][1] > counters[1][1]  # the call runs the top-k passes
    # a call between two half-sweeps leaves the fit bit-identical
    c.half(0)
    c2.half(0)
    assert np.array_equal(c.factors(0), c2.factors(0)) and np.array_equal(c.factors(1), c2.factors(1))
    # and the next call sees the new factors
    new = dict(case, U=c.factors(0), V=c.factors(1))
    src, ids, sc = unseen(gpu_lib, c.h, 0, UC.K)
    assert_same((ids, sc), UC.expected(new, UC.K), "after a half-sweep")


# ---- 10. errors ------------------------------------------------------------------------------------------

def test_error_codes(gpu_lib):
    from albedo_amd import _lib as L
    case = UC.ladder(3)
    c = context(gpu_lib, case)
    es, ed = UC.pairs(case)
    call = lambda **kw: unseen_rc(gpu_lib, c.h, kw.pop("side", 0), kw.pop("k", 5), **kw)[0]
    assert call() == L.ALS_OK and call(pairs=(es, ed)) == L.ALS_OK
    assert call(side=2) == L.ALS_E_INVALID_ARGUMENT and call(side=-1) == L.ALS_E_INVALID_ARGUMENT
    assert call(mode=2) == L.ALS_E_INVALID_ARGUMENT and call(mode=-1) == L.ALS_E_INVALID_ARGUMENT
    assert call(k=0) == L.ALS_E_INVALID_ARGUMENT and call(k=-3) == L.ALS_E_INVALID_ARGUMENT
    assert call(subset=case["src_ids"][:3], n_subset=-1) == L.ALS_E_INVALID_ARGUMENT
    assert call(pairs=(es, ed), n_excl=-1) == L.ALS_E_INVALID_ARGUMENT
    for name in ("es", "ed"):
        assert call(pairs=(es, ed), null=(name,)) == L.ALS_E_INVALID_ARGUMENT
    assert call(pairs=(es, ed), n_excl=0, null=("es", "ed")) == L.ALS_OK  # null arrays with no pairs
    for name in ("ids", "sc"):
        assert call(null=(name,)) == L.ALS_E_INVALID_ARGUMENT
    assert call(null=("src",)) == L.ALS_OK  # src_ids_out may be NULL
    assert gpu_lib.als_recommend_unseen(None, 0, 5, None, 0, 0, 0, None, None, None, None, None) == L.ALS_E_INVALID_ARGUMENT
    assert call(k=65) == L.ALS_E_UNSUPPORTED and call(k=64) == L.ALS_OK
    assert call(pairs=(es, ed), n_excl=2 ** 31) == L.ALS_E_UNSUPPORTED
    assert call(subset=case["src_ids"][:0]) == L.ALS_OK
    for fn, arr in ((gpu_lib.als_recommend_unseen_stats, np.zeros(4, np.int64)),
                    (gpu_lib.als_recommend_unseen_timing, np.zeros(5, np.float64))):
        ct = C.c_int64 if arr.dtype == np.int64 else C.c_double
        assert fn(c.h, None) == L.ALS_E_INVALID_ARGUMENT and fn(None, L.ptr(arr, ct)) == L.ALS_E_INVALID_ARGUMENT
    # factors missing on either side
    e = Ctx(gpu_lib, 3, "varying")
    assert unseen_rc(gpu_lib, e.h, 0, 5, n_rows=1)[0] == L.ALS_E_STATE
    e.ratings(*UC.ratings(case))
    e.inject(0, case["src_ids"], case["U"])
    for side in (0, 1):
        assert unseen_rc(gpu_lib, e.h, side, 5)[0] == L.ALS_E_STATE
    with pytest.raises(L.IllegalStateException):
        L.check(unseen_rc(gpu_lib, e.h, 0, 5)[0])
    # a sharded context
    ar = L.ALLREDUCE_FN(lambda u, buf, n: 1)
    ag = L.ALLGATHER_FN(lambda u, buf, n: 1)
    w = Ctx(gpu_lib, 3, "varying")
    L.check(gpu_lib.als_comm_init_host(w.h, 0, 2, ar, ag, None))
    assert unseen_rc(gpu_lib, w.h, 0, 5, n_rows=1)[0] == L.ALS_E_UNSUPPORTED
    assert "world" in gpu_lib.als_last_error().decode()
    del w


# ---- 11. Python ------------------------------------------------------------------------------------------

def _lists(frame):
    return [([i for i, _ in lst], np.array([s for _, s in lst], np.float32)) for lst in frame["recommendations"]]


def test_python_interface(gpu_lib, tmp_path):
    from albedo_amd import ALS, ALSModel
    from albedo_amd import _lib as L
    case = UC.ladder(50)
    u, i, r = UC.ratings(case)
    num = UC.K
    model = ALS(rank=8, maxIter=1, regParam=0.5, alpha=10.0, implicitPrefs=True, seed=3, userCol="u", itemCol="i",
                ratingCol="r").fit({"u": u, "i": i, "r": r})
    uid, U = model.user_factors_np()
    iid, V = model.item_factors_np()
    assert np.array_equal(uid, case["src_ids"]) and np.array_equal(iid, case["dst_ids"])
    fit = dict(case, U=U, V=V)
    want = UC.expected(fit, num)

    def frame_equals(frame, src_col, rows, want):
        keep = [j for j in rows if not np.isnan(want[1][j][0])]  # a row left with nothing has no frame row
        assert frame[src_col].tolist() == fit["src_ids"][keep].tolist()
        for (li, ls), j in zip(_lists(frame), keep):
            n = int((~np.isnan(want[1][j])).sum())
            assert li == want[0][j][:n].tolist() and np.array_equal(QC.bits(ls), QC.bits(want[1][j][:n]))

    rows = list(range(len(uid)))
    frame_equals(model.recommendForAllUsers(num, excludeKnown=True), "u", rows, want)
    assert model.unseen_stats()["rows"] == len(uid) and set(model.unseen_timing()) == {"exclusions", "lists", "filter",
                                                                                         "exact", "total"}
    some = [3, 17, 40]
    frame_equals(model.recommendForUserSubset({"u": uid[some]}, num, excludeKnown=True), "u", some, want)
    # the item side: users for an item, without the users who know it
    swapped = dict(src_ids=iid, dst_ids=uid, U=V, V=U,
                   E=[np.nonzero([j in e for e in case["E"]])[0] for j in range(len(iid))])
    fit, all_items = swapped, list(range(len(iid)))
    want_items = UC.expected(swapped, 7)
    frame_equals(model.recommendForAllItems(7, excludeKnown=True), "i", all_items, want_items)
    frame_equals(model.recommendForItemSubset({"i": iid[[5, 9]]}, 7, excludeKnown=True), "i", [5, 9], want_items)
    # numpy interface: the pairs mode equals the ratings mode
    a = model.recommend_unseen_np(num)
    b = model.recommend_unseen_np(num, exclude=UC.pairs(case))
    assert np.array_equal(a[0], uid) and QC.same(a[1:], want) and QC.same(b[1:], want)
    # the defaults stay what they were
    plain = model.recommend_np(num)
    assert QC.same(model.recommend_unseen_np(num, exclude=(np.zeros(0, np.int32), np.zeros(0, np.int32)))[1:], plain[1:])
    assert len(model.recommendForAllUsers(num)) == len(uid)
    with pytest.raises(ValueError):
        model.recommendForUserSubset({"u": uid[:2]}, num, exclude={"u": uid[:1], "i": iid[:1]}, excludeKnown=True)
    # a loaded model holds no ratings
    path = str(tmp_path / "model")
    model.save(path)
    loaded = ALSModel.load(path)
    with pytest.raises(L.IllegalStateException, match="no ratings"):
        loaded.recommendForAllUsers(num, excludeKnown=True)
    assert QC.same(loaded.recommend_unseen_np(num, exclude=UC.pairs(case))[1:], want)
