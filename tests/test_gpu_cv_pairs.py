"""Held-out pair ranking on the device (albedo_amd/csrc/eval_pairs.hip behind als_rank_pairs,
als_evaluate_pairs and als_evaluate_ranking) through the raw C ABI, on the cases of tests/cv_cases.py
(their preconditions are asserted on the CPU by tests/test_cv_cases.py).

No tolerance anywhere.  For every case and every user: the users, list lengths and item ids equal the
oracle route's, the scores are bit-identical to O.f2j_sdot, the per-user metric values are
bit-identical (np.array_equal) to O.ndcg_at and to the restatement of mllib's precisionAt /
meanAveragePrecision, the mean equals the left-to-right sum over ascending user ids divided by the
count, and n_users_out is exact.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import cv_cases as CC
from tests import eval_cases as EC

pytestmark = pytest.mark.gpu

METRIC_CODE = {"NDCG@k": 0, "Precision@k": 1, "MAP": 2}


class _Model:
    """A model-only context of (uid, uf, iid, itf), destroyed on exit."""

    def __init__(self, lib, m):
        from albedo_amd import _lib as L
        self.lib, self.L = lib, L
        uid, uf, iid, itf = (np.ascontiguousarray(a) for a in m)
        assert uf.dtype == itf.dtype == np.float32 and uid.dtype == iid.dtype == np.int32
        self.h = C.c_void_p()
        L.check(lib.als_model_create(uf.shape[1], uid.size, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), iid.size,
                                     L.ptr(iid, C.c_int32), L.ptr(itf, C.c_float), -1, C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.als_destroy(self.h)

    def rank_rc(self, top_k, width, users, items, cap=None):
        L = self.L
        u, it = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(items, np.int32)
        cap = max(int(np.unique(u).size), 1) if cap is None else cap
        w = max(width, 1)
        nu = C.c_int64(-1)
        uo, ln = np.full(max(cap, 1), 12345, np.int32), np.full(max(cap, 1), -7, np.int32)
        io, so = np.full((max(cap, 1), w), 777, np.int32), np.full((max(cap, 1), w), -5.0, np.float32)
        rc = self.lib.als_rank_pairs(self.h, top_k, width, u.size, L.ptr(u, C.c_int32), L.ptr(it, C.c_int32),
                                     C.byref(nu), L.ptr(uo, C.c_int32), L.ptr(ln, C.c_int32), L.ptr(io, C.c_int32),
                                     L.ptr(so, C.c_float), cap)
        n = max(int(nu.value), 0)
        return rc, nu.value, uo[:n], ln[:n], io[:n], so[:n]

    def pairs_rc(self, metric, top_k, k, pairs, actual, cap=None):
        L = self.L
        u, it = (np.ascontiguousarray(a, np.int32) for a in pairs)
        au, ai = (np.ascontiguousarray(a, np.int32) for a in actual[:2])
        ak = np.ascontiguousarray(actual[2], np.int64)
        cap = max(int(np.unique(u).size), 1) if cap is None else cap
        mean, nu = C.c_double(-1.0), C.c_int64(-1)
        uo, vo = np.full(max(cap, 1), 12345, np.int32), np.full(max(cap, 1), -1.0, np.float64)
        rc = self.lib.als_evaluate_pairs(self.h, metric, top_k, k, u.size, L.ptr(u, C.c_int32), L.ptr(it, C.c_int32),
                                         au.size, L.ptr(au, C.c_int32), L.ptr(ai, C.c_int32), L.ptr(ak, C.c_int64),
                                         C.byref(mean), C.byref(nu), L.ptr(uo, C.c_int32), L.ptr(vo, C.c_double), cap)
        n = max(int(nu.value), 0)
        return rc, mean.value, nu.value, uo[:n], vo[:n]

    def ranking_rc(self, metric, k, users, items, keys):
        L = self.L
        u, it = np.ascontiguousarray(users, np.int32), np.ascontiguousarray(items, np.int32)
        ky = np.ascontiguousarray(keys, np.int64)
        cap = max(int(np.unique(u).size), 1)
        mean, nu = C.c_double(-1.0), C.c_int64(-1)
        uo, vo = np.full(cap, 12345, np.int32), np.full(cap, -1.0, np.float64)
        if metric is None:
            rc = self.lib.als_evaluate_ndcg(self.h, k, u.size, L.ptr(u, C.c_int32), L.ptr(it, C.c_int32),
                                            L.ptr(ky, C.c_int64), C.byref(mean), C.byref(nu), L.ptr(uo, C.c_int32),
                                            L.ptr(vo, C.c_double), cap)
        else:
            rc = self.lib.als_evaluate_ranking(self.h, metric, k, u.size, L.ptr(u, C.c_int32), L.ptr(it, C.c_int32),
                                               L.ptr(ky, C.c_int64), C.byref(mean), C.byref(nu), L.ptr(uo, C.c_int32),
                                               L.ptr(vo, C.c_double), cap)
        n = max(int(nu.value), 0)
        return rc, mean.value, uo[:n], vo[:n]


def _assert_lists(what, got, ref):
    rc, nu, uo, ln, io, so = got
    users, rln, items, scores = ref
    assert rc == 0, f"{what}: rc {rc}"
    assert nu == users.size, f"{what}: n_users_out {nu}, want {users.size}"
    assert np.array_equal(uo, users), f"{what}: users differ"
    if not np.array_equal(ln, rln):
        j = int(np.nonzero(ln != rln)[0][0])
        raise AssertionError(f"{what}: user {int(users[j])}: length {int(ln[j])}, want {int(rln[j])}")
    if not np.array_equal(io, items):
        j = int(np.nonzero(np.any(io != items, axis=1))[0][0])
        raise AssertionError(f"{what}: user {int(users[j])} (length {int(rln[j])}): items {io[j].tolist()}, want "
                             f"{items[j].tolist()}")
    if not np.array_equal(so.view(np.uint32)[~np.isnan(scores)], scores.view(np.uint32)[~np.isnan(scores)]):
        j = int(np.nonzero(np.any((so.view(np.uint32) != scores.view(np.uint32)) & ~np.isnan(scores), axis=1))[0][0])
        raise AssertionError(f"{what}: user {int(users[j])}: scores {so[j].tolist()}, want {scores[j].tolist()}")
    assert np.all(np.isnan(so[np.isnan(scores)])), f"{what}: score padding is not NaN"


def _assert_metric(what, got, ref):
    rc, mean, nu, uo, vo = got
    users, vals, ref_mean = ref
    assert rc == 0, f"{what}: rc {rc}"
    assert nu == users.size, f"{what}: n_users_out {nu}, want {users.size}"
    assert np.array_equal(uo, users), f"{what}: evaluated users differ"
    if not np.array_equal(vo, vals):
        bad = np.nonzero(vo != vals)[0]
        j = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {vals.size} per-user values differ; first user {int(users[j])}: "
                             f"got {float(vo[j])!r}, want {float(vals[j])!r}")
    if users.size == 0:
        assert np.isnan(mean)
    else:
        assert mean == ref_mean, f"{what}: mean {mean!r}, want the sequential {ref_mean!r}"


def _check_case(lib, name, args, combos):
    c = CC.case(name, *args)
    with _Model(lib, c.model) as M:
        for top_k, k in combos:
            what = f"{CC.case_id((name, args))} top_k={top_k} k={k}"
            _assert_lists(what, M.rank_rc(top_k, k, *c.pairs), CC.rank_reference(name, args, top_k, k))
            for metric in CC.METRICS:
                _assert_metric(f"{what} {metric}", M.pairs_rc(METRIC_CODE[metric], top_k, k, c.pairs, c.actual),
                               CC.metric_reference(name, args, metric, top_k, k))


@pytest.mark.parametrize("case", CC.SMALL_CASES, ids=CC.case_id)
def test_pairs_match_oracle(gpu_lib, case):
    """Every small case at the job's (top_k 15, k 30): lists and the three metrics, every user."""
    _check_case(gpu_lib, case[0], case[1], [(15, 30)])


@pytest.mark.parametrize("name", ["lengths", "ties", "drop"])
def test_pairs_top_k_and_k_edges(gpu_lib, name):
    """(top_k, k) = (30,30), (30,15), (1,1), (64,64), (1,64), (64,1)."""
    _check_case(gpu_lib, name, (), CC.TOPK_K[1:])


def test_pairs_width_differs_from_top_k(gpu_lib):
    """als_rank_pairs at widths below, at and above what the ties leave: the 70-way tie at width 64."""
    c = CC.case("ties")
    with _Model(gpu_lib, c.model) as M:
        for top_k, width in ((15, 15), (15, 64), (15, 1), (6, 40)):
            _assert_lists(f"ties top_k={top_k} width={width}", M.rank_rc(top_k, width, *c.pairs),
                          CC.rank_reference("ties", (), top_k, width))


@pytest.mark.parametrize("case", CC.SIZE_CASES, ids=CC.case_id)
def test_pairs_size_cases(gpu_lib, case):
    """One user with 100,000 pairs (cut into segments, merged) beside 2,000 one-pair users; an input
    longer than one pass of the map kernel's grid."""
    _check_case(gpu_lib, case[0], case[1], [(15, 30)])


def test_pairs_outputs_wait_for_cap(gpu_lib):
    """n_users_out is exact whatever cap is; the arrays are filled only when it fits."""
    c = CC.case("drop")
    users = CC.rank_reference("drop", (), 15, 30)[0]
    with _Model(gpu_lib, c.model) as M:
        rc, nu, uo, ln, io, so = M.rank_rc(15, 30, *c.pairs, cap=users.size - 1)
        assert rc == 0 and nu == users.size
        assert np.all(uo[:users.size - 1] == 12345)
        eu = CC.metric_reference("drop", (), "MAP", 15, 30)[0]
        rc, mean, nu, uo, vo = M.pairs_rc(2, 15, 30, c.pairs, c.actual, cap=eu.size - 1)
        assert rc == 0 and nu == eu.size and mean == CC.metric_reference("drop", (), "MAP", 15, 30)[2]
        assert np.all(vo[:eu.size - 1] == -1.0)
        # nobody left: only unknown users
        unknown = ~np.isin(c.pairs[0], c.model[0])
        rc, mean, nu, uo, vo = M.pairs_rc(0, 15, 30, (c.pairs[0][unknown], c.pairs[1][unknown]), c.actual)
        assert rc == 0 and nu == 0 and np.isnan(mean)
        rc, nu, *_ = M.rank_rc(15, 30, c.pairs[0][unknown], c.pairs[1][unknown])
        assert rc == 0 and nu == 0
        rc, nu, *_ = M.rank_rc(15, 30, c.pairs[0][:0], c.pairs[1][:0])
        assert rc == 0 and nu == 0


def test_pairs_on_a_fitted_context(gpu_lib):
    """The calls work on a fitted context as on a model-only one holding the same factors."""
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(300, 120, 4000, seed=5))
    model = ALS(rank=6, maxIter=2, regParam=0.1, alpha=10.0, implicitPrefs=True, seed=3).fit(d)
    uid, uf = model.user_factors_np()
    iid, itf = model.item_factors_np()
    rng = np.random.default_rng(1)
    users = rng.choice(np.r_[uid, [-5, 10 ** 6]], 3000).astype(np.int32)
    items = rng.choice(iid, 3000).astype(np.int32)
    got = model.rank_pairs(users, items, topK=15, width=30)
    with _Model(gpu_lib, (uid, uf, iid, itf)) as M:
        rc, nu, uo, ln, io, so = M.rank_rc(15, 30, users, items)
    assert rc == 0 and np.array_equal(got[0], uo) and np.array_equal(got[1], ln) and np.array_equal(got[2], io)
    assert np.array_equal(got[3].view(np.uint32), so.view(np.uint32))
    known = np.isin(users, uid)
    sc = O.f2j_sdot(uf[np.searchsorted(uid, users[known])], itf[np.searchsorted(iid, items[known])])
    lists = O.into_user_items(users[known], items[known], sc, 15)
    assert uo.tolist() == sorted(lists)
    for r, u in enumerate(uo):
        assert io[r, :ln[r]].tolist() == lists[int(u)][:30]


@pytest.mark.parametrize("case", [("lengths", ("random",)), ("bag", ("twentynine",))], ids=EC.case_id)
def test_evaluate_ranking_ndcg_is_evaluate_ndcg(gpu_lib, case):
    """als_evaluate_ranking(ALS_METRIC_NDCG) returns als_evaluate_ndcg's users, values and mean bit for bit."""
    m, ev = EC.case(case[0], *case[1])
    with _Model(gpu_lib, m) as M:
        for k in (30, 5):
            a = M.ranking_rc(None, k, *ev)
            b = M.ranking_rc(0, k, *ev)
            assert a[0] == b[0] == 0
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[1] == b[1] and a[2].size > 0


@pytest.mark.parametrize("case", [("lengths", ("random",)), ("bag", ("twentynine",)), ("bag", ("five",))],
                         ids=EC.case_id)
def test_evaluate_ranking_precision_and_map(gpu_lib, case):
    """Precision@k and MAP of the model's own top-k lists against the restatement on
    O.recommend_for_all lists and O.into_user_items actual lists, every user, bit for bit."""
    m, (users, items, keys) = EC.case(case[0], *case[1])
    with _Model(gpu_lib, m) as M:
        for k in (30, 7):
            known, pred = EC.predicted_lists(m, users, k)
            actual = O.into_user_items(users, items, keys, k)
            for metric in ("Precision@k", "MAP"):
                vals = np.array([CC.metric_value(metric, pred[int(u)][:k], actual[int(u)][:k], k) for u in known])
                rc, mean, uo, vo = M.ranking_rc(METRIC_CODE[metric], k, users, items, keys)
                assert rc == 0 and np.array_equal(uo, known)
                assert np.array_equal(vo, vals), f"{EC.case_id(case)} {metric} k={k}"
                assert mean == CC.sequential_mean(vals)


def test_argument_errors(gpu_lib):
    from albedo_amd import _lib as L
    c = CC.case("drop")
    with _Model(gpu_lib, c.model) as M:
        for top_k, width, want in ((0, 30, L.ALS_E_INVALID_ARGUMENT), (-1, 30, L.ALS_E_INVALID_ARGUMENT),
                                   (15, 0, L.ALS_E_INVALID_ARGUMENT), (65, 30, L.ALS_E_UNSUPPORTED),
                                   (15, 65, L.ALS_E_UNSUPPORTED)):
            assert M.rank_rc(top_k, width, *c.pairs)[0] == want, (top_k, width)
            assert M.pairs_rc(0, top_k, width, c.pairs, c.actual)[0] == want, (top_k, width)
            assert len(gpu_lib.als_last_error()) > 0
        for metric in (-1, 3):
            assert M.pairs_rc(metric, 15, 30, c.pairs, c.actual)[0] == L.ALS_E_INVALID_ARGUMENT
            assert M.ranking_rc(metric, 30, *c.actual)[0] == L.ALS_E_INVALID_ARGUMENT
        assert M.ranking_rc(0, 65, *c.actual)[0] == L.ALS_E_UNSUPPORTED
        assert M.ranking_rc(1, 0, *c.actual)[0] == L.ALS_E_INVALID_ARGUMENT
        nu, mean = C.c_int64(), C.c_double()
        one = np.zeros(1, np.int32)
        assert gpu_lib.als_rank_pairs(M.h, 15, 30, 5, None, L.ptr(one, C.c_int32), C.byref(nu), None, None, None, None,
                                      0) == L.ALS_E_INVALID_ARGUMENT
        assert gpu_lib.als_rank_pairs(M.h, 15, 30, 0, None, None, None, None, None, None, None,
                                      0) == L.ALS_E_INVALID_ARGUMENT
        assert gpu_lib.als_evaluate_pairs(M.h, 0, 15, 30, 1, L.ptr(one, C.c_int32), L.ptr(one, C.c_int32), 3, None, None,
                                          None, C.byref(mean), C.byref(nu), None, None, 0) == L.ALS_E_INVALID_ARGUMENT
        # the context still works after the refusals
        _assert_lists("drop after the refusals", M.rank_rc(15, 30, *c.pairs), CC.rank_reference("drop", (), 15, 30))
