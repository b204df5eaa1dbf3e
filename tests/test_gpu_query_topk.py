"""als_recommend_vectors on the GPU: exact top-k of caller-supplied vectors with per-query exclusion lists.

Every expected value is tests/query_cases.py:expected: oracle.cbind.recommend over the dst rows left after
removing query i's excluded (and NaN-scoring) rows.  Ids and score bits are compared for equality: the
score is fp32, left to right, without a fused product, so there is nothing to tolerate.  The contexts are
model-only (als_model_create) with a few hundred rows unless a test says otherwise, and
ALBEDO_QUERY_SLICE_ROWS = 256 makes 257 rows and more cross scan slices.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import foldin_cases as FC
from tests import query_cases as QC
from tests.test_gpu_audit import Ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _slices(monkeypatch):
    monkeypatch.setenv("ALBEDO_QUERY_SLICE_ROWS", str(QC.SLICE_ROWS))
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)


class Model:
    """A model-only context holding the case's dst rows on `dst_side` and one zero row on the other."""

    def __init__(self, lib, dst_ids, F, dst_side=1):
        from albedo_amd import _lib as L
        self.lib, self.L, self.side = lib, L, dst_side
        ids = np.ascontiguousarray(dst_ids, np.int32)
        F = np.ascontiguousarray(F, np.float32)
        k = F.shape[1]
        one, z = np.zeros(1, np.int32), np.zeros((1, k), np.float32)
        u, i = ((one, z), (ids, F)) if dst_side == 1 else ((ids, F), (one, z))
        self.h = C.c_void_p()
        L.check(lib.als_model_create(k, u[0].size, L.ptr(u[0], C.c_int32), L.ptr(u[1], C.c_float), i[0].size,
                                     L.ptr(i[0], C.c_int32), L.ptr(i[1], C.c_float), -1, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.als_destroy(self.h)


def rv_rc(lib, h, side, q, k, excl=None, n_q=None, ptr=None, eids=None, null=()):
    """The raw call: (rc, ids, scores).  excl: one id array per query; ptr / eids override the CSR arrays."""
    from albedo_amd import _lib as L
    q = np.ascontiguousarray(q, np.float32)
    n_q = q.shape[0] if n_q is None else n_q
    if excl is not None and ptr is None:
        ptr, eids = QC.excl_csr(excl)
    if ptr is not None:
        ptr = np.ascontiguousarray(ptr, np.int64)
    if eids is not None:
        eids = np.ascontiguousarray(eids, np.int32)
    kk = max(k, 1)
    ids = np.full((max(n_q, 1), kk), 123456789, np.int32)
    sc = np.full((max(n_q, 1), kk), 7.0, np.float32)
    rc = lib.als_recommend_vectors(h, side, k, n_q, None if "q" in null else L.ptr(q, C.c_float),
                                   L.ptr(ptr, C.c_int64) if ptr is not None else None,
                                   L.ptr(eids, C.c_int32) if eids is not None and "eids" not in null else None,
                                   None if "ids" in null else L.ptr(ids, C.c_int32),
                                   None if "sc" in null else L.ptr(sc, C.c_float))
    return rc, ids[:max(n_q, 0)], sc[:max(n_q, 0)]


def rv(lib, h, side, q, k, excl=None):
    from albedo_amd import _lib as L
    rc, ids, sc = rv_rc(lib, h, side, q, k, excl)
    L.check(rc)
    return ids, sc


def run_case(lib, case, dst_side=1):
    m = Model(lib, case["dst_ids"], case["F"], dst_side)
    return m, rv(lib, m.h, dst_side, case["q"], case["k"], case["excl"])


def check_case(lib, case, what, dst_side=1):
    want = QC.expected(case)
    m, got = run_case(lib, case, dst_side)
    bad = [i for i in range(len(want[0])) if not QC.same((got[0][i], got[1][i]), (want[0][i], want[1][i]))]
    if bad:
        i = bad[0]
        print(f"QUERY {what}: query {i} differs\n got  {got[0][i]}\n      {got[1][i]}\n want {want[0][i]}\n      {want[1][i]}")
    assert not bad, f"{what}: {len(bad)} of {len(want[0])} lists differ, first query {bad[0]}"
    return m, got


# ---- 1. sizes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", QC.KS)
@pytest.mark.parametrize("n", QC.SIZES)
def test_dst_sizes(gpu_lib, n, k):
    case = QC.random_case(QC.size(n, k), 17, k, 6)
    check_case(gpu_lib, case, f"n_dst {n} k {k}")
    check_case(gpu_lib, dict(case, excl=None), f"n_dst {n} k {k}, no exclusions")


@pytest.mark.parametrize("n_q", QC.N_Q)
def test_query_counts(gpu_lib, n_q):
    check_case(gpu_lib, QC.random_case(257, n_q, 30, 6), f"n_q {n_q}")


@pytest.mark.parametrize("rank", QC.RANKS)
def test_ranks(gpu_lib, rank):
    check_case(gpu_lib, QC.random_case(300, 17, 30, rank), f"rank {rank}")


def test_user_side_and_unsorted_ids(gpu_lib):
    case = QC.random_case(300, 5, 30, 6)
    p = np.random.default_rng(1).permutation(300)
    check_case(gpu_lib, dict(case, dst_ids=case["dst_ids"][p], F=case["F"][p]), "users as dst, ids shuffled", dst_side=0)


# ---- 2. ties, signs, non-finite ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["boundary_tie_case", "zero_and_sign_case", "nonfinite_case"])
def test_ties_signs_nonfinite(gpu_lib, name):
    check_case(gpu_lib, getattr(QC, name)(), name)


# ---- 3. exclusions, repeatability ----------------------------------------------------------------------

def test_exclusion_contract_and_repeatability(gpu_lib):
    case = QC.exclusion_case()
    m, got = check_case(gpu_lib, case, "exclusion contract")
    assert QC.same((got[0][7], got[1][7]), (got[0][5], got[1][5]))  # one list in two orders
    again = rv(gpu_lib, m.h, 1, case["q"], case["k"], case["excl"])
    assert QC.same(again, got)                                       # two calls, same bits
    sh = QC.shuffled(case)
    assert QC.same(rv(gpu_lib, m.h, 1, sh["q"], sh["k"], sh["excl"]), got)
    # excl_ptr that does not start at 0: the ranges are what counts
    ptr, eids = QC.excl_csr(case["excl"])
    from albedo_amd import _lib as L
    rc, ids, sc = rv_rc(gpu_lib, m.h, 1, case["q"], case["k"], ptr=ptr + 5, eids=np.concatenate([[1, 2, 3, 4, 5], eids]))
    assert rc == L.ALS_OK and QC.same((ids, sc), got)
    t = L.recommend_vectors_timing(m.h)
    assert t[0] > 0 and t[1] > 0 and t[2] > 0 and t[3] >= t[0] + t[1] + t[2] - 1e-3
    rv(gpu_lib, m.h, 1, case["q"], case["k"], None)
    assert L.recommend_vectors_timing(m.h)[0] == 0.0


# ---- 4. against the tuned path -------------------------------------------------------------------------

def _fitted(lib, k=16):
    """A context after two half-sweeps on the synthetic problem of smoke(): 600 users, 150 items."""
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(600, 150, 6000, seed=3))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(2)
    c = Ctx(lib, k, "varying")
    c.ratings(d["user"], d["item"], d["rating"])
    c.inject(0, B.user_ids, rng.standard_normal((len(B.user_ids), k)).astype(np.float32))
    c.inject(1, B.item_ids, rng.standard_normal((len(B.item_ids), k)).astype(np.float32))
    c.half(1)
    c.half(0)
    return c, B


def _tuned(lib, h, side, k, subset):
    from albedo_amd import _lib as L
    sub = np.ascontiguousarray(subset, np.int32)
    src = np.empty(sub.size, np.int32)
    ids = np.empty((sub.size, k), np.int32)
    sc = np.empty((sub.size, k), np.float32)
    L.check(lib.als_recommend(h, side, k, L.ptr(sub, C.c_int32), sub.size, L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32),
                              L.ptr(sc, C.c_float)))
    return src, ids, sc


def test_equals_als_recommend_on_fitted_and_model_only_contexts(gpu_lib):
    from albedo_amd import _lib as L
    c, B = _fitted(gpu_lib)
    k, num = c.k, 30
    U, V = c.factors(0), c.factors(1)
    users = np.sort(np.random.default_rng(4).choice(B.user_ids, 300, replace=False)).astype(np.int32)
    rows = np.searchsorted(B.user_ids, users)
    h2 = C.c_void_p()
    L.check(gpu_lib.als_model_create(k, len(B.user_ids), L.ptr(B.user_ids, C.c_int32), L.ptr(U, C.c_float),
                                     len(B.item_ids), L.ptr(B.item_ids, C.c_int32), L.ptr(V, C.c_float), -1, C.byref(h2)))
    try:
        for what, h in (("fitted", c.h), ("model-only", h2)):
            src, ids, sc = _tuned(gpu_lib, h, 0, num, users)
            assert np.array_equal(src, users)
            assert QC.same(rv(gpu_lib, h, 1, U[rows], num), (ids, sc)), what
            # the mirror: every item's best users, 600 dst rows over three slices
            src, ids, sc = _tuned(gpu_lib, h, 1, num, B.item_ids)
            assert QC.same(rv(gpu_lib, h, 0, V, num), (ids, sc)), what + " (items to users)"
    finally:
        gpu_lib.als_destroy(h2)


# ---- 5. read-only --------------------------------------------------------------------------------------

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
    n = C.c_int64(-1)
    L.check(lib.als_topk_last_rescan(c.h, None, 0, C.byref(n)))
    return out + [st, tm, np.array([n.value])]


def test_model_is_untouched(gpu_lib):
    c, B = _fitted(gpu_lib)
    _tuned(gpu_lib, c.h, 0, 10, B.user_ids[:50])  # the top-k counters hold something
    U = c.factors(0)
    excl = [B.item_ids[:20]] * 40
    before = _state(gpu_lib, c)
    assert before[-3][0] > 0
    got = rv(gpu_lib, c.h, 1, U[:40], 10, excl)
    rv(gpu_lib, c.h, 0, c.factors(1)[:5], 10)
    after = _state(gpu_lib, c)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert not np.isin(got[0], B.item_ids[:20]).any()
    # a call between two half-sweeps leaves the fit bit-identical
    c2, _ = _fitted(gpu_lib)
    c.half(1)
    c2.half(1)
    assert np.array_equal(c.factors(1), c2.factors(1)) and np.array_equal(c.factors(0), c2.factors(0))
    # and the next call sees the new factors
    V = c.factors(1)
    want = QC.expected(dict(dst_ids=B.item_ids, F=V, q=U[:40], k=10, excl=excl))
    assert QC.same(rv(gpu_lib, c.h, 1, U[:40], 10, excl), want)


def test_fork_answers_like_its_parent(gpu_lib):
    c, B = _fitted(gpu_lib)
    f = Ctx(gpu_lib, c.k, "varying", parent=c)
    f.inject(0, B.user_ids, c.factors(0))
    f.inject(1, B.item_ids, c.factors(1))
    q = c.factors(0)[:20]
    assert QC.same(rv(gpu_lib, f.h, 1, q, 7), rv(gpu_lib, c.h, 1, q, 7))
    del f


# ---- 6. errors -----------------------------------------------------------------------------------------

def test_error_codes(gpu_lib):
    from albedo_amd import _lib as L
    case = QC.random_case(300, 3, 30, 6)
    m = Model(gpu_lib, case["dst_ids"], case["F"])
    q, ex = case["q"], case["excl"]
    ptr, eids = QC.excl_csr(ex)
    call = lambda **kw: rv_rc(gpu_lib, m.h, kw.pop("side", 1), q, kw.pop("k", 30), **kw)[0]
    assert call(excl=ex) == L.ALS_OK
    assert call(side=2) == L.ALS_E_INVALID_ARGUMENT and call(side=-1) == L.ALS_E_INVALID_ARGUMENT
    assert call(k=0) == L.ALS_E_INVALID_ARGUMENT and call(k=-3) == L.ALS_E_INVALID_ARGUMENT
    assert call(n_q=-1) == L.ALS_E_INVALID_ARGUMENT
    for name in ("q", "ids", "sc"):
        assert call(null=(name,)) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_recommend_vectors(None, 1, 30, 0, None, None, None, None, None) == L.ALS_E_INVALID_ARGUMENT
    bad = ptr.copy()
    bad[1], bad[2] = ptr[2], ptr[1]
    assert bad[2] < bad[1] and call(ptr=bad, eids=eids) == L.ALS_E_INVALID_ARGUMENT          # not monotone
    assert call(ptr=ptr - 1, eids=eids) == L.ALS_E_INVALID_ARGUMENT                           # negative
    assert call(ptr=ptr, eids=eids, null=("eids",)) == L.ALS_E_INVALID_ARGUMENT              # null ids, ranges not empty
    assert call(ptr=np.zeros(4, np.int64), eids=eids, null=("eids",)) == L.ALS_OK             # null ids, empty ranges
    assert call(ptr=np.array([0, 0, 0, 2 ** 31], np.int64), eids=eids) == L.ALS_E_INVALID_ARGUMENT  # too many
    assert call(k=65) == L.ALS_E_UNSUPPORTED and call(k=64) == L.ALS_OK
    with pytest.raises(L.ALSError):
        L.check(call(k=65))
    rc, ids, sc = rv_rc(gpu_lib, m.h, 1, q, 30, n_q=0)
    assert rc == L.ALS_OK
    assert gpu_lib.als_recommend_vectors(m.h, 1, 30, 0, None, None, None, None, None) == L.ALS_OK  # nulls with n_q = 0
    assert gpu_lib.als_recommend_vectors_timing(m.h, None) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_recommend_vectors_timing(None, L.ptr(np.zeros(4), C.c_double)) == L.ALS_E_INVALID_ARGUMENT
    # no factors on the dst side
    c = Ctx(gpu_lib, 6, "varying")
    assert rv_rc(gpu_lib, c.h, 1, q, 30)[0] == L.ALS_E_STATE
    user, item, r, B = FC.data("varying")
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, FC.src_factors(6, len(B.user_ids)))
    assert rv_rc(gpu_lib, c.h, 1, q, 30)[0] == L.ALS_E_STATE      # the users have factors, the items none
    assert rv_rc(gpu_lib, c.h, 0, q, 30)[0] == L.ALS_OK
    with pytest.raises(L.IllegalStateException):
        L.check(rv_rc(gpu_lib, c.h, 1, q, 30)[0])


def test_sharded_context_is_unsupported(gpu_lib):
    """world = 2 through the host transport (tests/mp_worker.py); the call returns before any exchange."""
    from albedo_amd import _lib as L
    ar = L.ALLREDUCE_FN(lambda u, buf, n: 1)
    ag = L.ALLGATHER_FN(lambda u, buf, n: 1)
    c = Ctx(gpu_lib, 6, "varying")
    L.check(gpu_lib.als_comm_init_host(c.h, 0, 2, ar, ag, None))
    assert rv_rc(gpu_lib, c.h, 1, np.zeros((2, 6), np.float32), 5)[0] == L.ALS_E_UNSUPPORTED
    assert "world" in gpu_lib.als_last_error().decode()
    del c


# ---- 7. Python -----------------------------------------------------------------------------------------

def _lists(frame):
    return [([i for i, _ in lst], np.array([s for _, s in lst], np.float32)) for lst in frame["recommendations"]]


def test_recommend_for_new_users_without_their_items(gpu_lib):
    from albedo_amd import ALS
    user, item, r, B = FC.data("varying")
    k, reg, alpha, num = 16, 0.5, 10.0, 7
    model = ALS(rank=k, maxIter=1, regParam=reg, alpha=alpha, implicitPrefs=True, seed=3, userCol="u", itemCol="i",
                ratingCol="r").fit({"u": user, "i": item, "r": r})
    new = np.unique(user)[:40]
    m = np.isin(user, new)
    nu, ni, nr = (user[m].astype(np.int64) + FC.ID_SHIFT).astype(np.int32), item[m], r[m]
    ds = {"u": nu, "i": ni, "r": nr}
    ids, _, X = model.fold_in_np(nu, ni, nr)
    iid, V = model.item_factors_np()
    excl = [ni[nu == u] for u in ids]
    assert all(len(e) for e in excl)
    want = QC.expected(dict(dst_ids=iid, F=V, q=X, k=num, excl=excl))
    recs = model.recommendForNewUsers(ds, num, excludeKnown=True)
    assert list(recs.columns) == ["u", "recommendations"] and np.array_equal(recs["u"].to_numpy(), ids)
    hit = 0
    for j, (li, ls) in enumerate(_lists(recs)):
        n = int((want[0][j] != -1).sum())
        assert li == want[0][j][:n].tolist() and np.array_equal(QC.bits(ls), QC.bits(want[1][j][:n]))
        assert not np.isin(li, excl[j]).any()
        hit += int(np.isin(QC.expected(dict(dst_ids=iid, F=V, q=X[j:j + 1], k=num, excl=None))[0][0], excl[j]).any())
    assert hit > 20  # without the exclusion most users get their own items back
    # the default stays what it was: the oracle over all items
    plain = model.recommendForNewUsers(ds, num)
    w_ids, w_sc = O.recommend_for_all(ids, X, iid, V, num)
    for j, (li, ls) in enumerate(_lists(plain)):
        assert li == w_ids[j].tolist() and np.array_equal(QC.bits(ls), QC.bits(w_sc[j]))
    # numpy interface, both forms of the exclusion argument
    a = model.recommend_vectors_np(X, num, excl)
    b = model.recommend_vectors_np(X, num, QC.excl_csr(excl))
    assert QC.same(a, want) and QC.same(b, want)
    assert set(model.recommend_vectors_timing()) == {"exclusions", "scan", "merge", "total"}
    # known users with an exclusion frame
    known = np.unique(user)[:25]
    mk = np.isin(user, known)
    sub = model.recommendForUserSubset({"u": known}, num, exclude={"u": user[mk], "i": item[mk]})
    uid, U = model.user_factors_np()
    ke = [item[user == u] for u in known]
    wk = QC.expected(dict(dst_ids=iid, F=V, q=U[np.searchsorted(uid, known)], k=num, excl=ke))
    assert np.array_equal(sub["u"].to_numpy(), known)
    for j, (li, ls) in enumerate(_lists(sub)):
        n = int((wk[0][j] != -1).sum())
        assert li == wk[0][j][:n].tolist() and np.array_equal(QC.bits(ls), QC.bits(wk[1][j][:n]))


def test_recommend_for_vectors_puts_a_dominant_item_first(gpu_lib, tmp_path):
    from albedo_amd import ALSModel
    from albedo_amd import persistence
    case = QC.own_factor_case()
    ids, F = case["dst_ids"], case["F"]
    k = F.shape[1]
    path = str(tmp_path / "model")
    uid, U = np.arange(3, dtype=np.int32), np.zeros((3, k), np.float32)
    persistence.save_als_model(path, "als_test", {"userCol": "u", "itemCol": "i", "predictionCol": "prediction",
                                                  "coldStartStrategy": "nan"}, k, (uid, U), (ids, F), False, 1 << 20)
    model = ALSModel.load(path)
    lead = int(ids[case["lead"]])
    frame = model.recommendForVectors([lead], case["q"], case["k"], side="item")
    assert list(frame.columns) == ["u", "recommendations"] and frame["u"].tolist() == [lead]
    want = QC.expected(case)
    (li, ls), = _lists(frame)
    assert li[0] == lead and li == want[0][0].tolist() and np.array_equal(QC.bits(ls), QC.bits(want[1][0]))
    # "repos like this one" without the repo itself; users recommended for a vector label the item column
    (li2, _), = _lists(model.recommendForVectors([lead], case["q"], case["k"], exclude=[[lead]]))
    assert lead not in li2 and li2[:4] == li[1:]
    assert list(model.recommendForVectors([lead], case["q"], 2, side="user").columns) == ["i", "recommendations"]
    with pytest.raises(ValueError):
        model.recommend_vectors_np(case["q"][:, :-1], 5)
