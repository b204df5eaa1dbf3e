"""GPU parity: the HIP path through the C ABI against the CPU oracle and the golden fixtures.

Tolerances (stated per SURVEY.md §8(c)):
  * one half-sweep from identical inputs: max_row |x_gpu - x_oracle|_inf / |x_oracle|_inf <= 1e-4
    (fp32 build + fp32 solve vs Spark's fp64; measured on trained factors at ~2e-5 worst);
  * after a multi-sweep fit: factors within 1e-3 relative, RMSE within 1e-3 relative, NDCG@k
    within 1e-3;
  * top-k: ids and F2J scores bit-exact after the (score desc, id asc) tie-break;
  * transform: bit-exact F2J sdot.
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import spark_als as O
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _row_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    num = np.max(np.abs(a - b), axis=1)
    den = np.maximum(np.max(np.abs(b), axis=1), 1e-30)
    return float(np.max(num / den))


class Ctx:
    """Thin test helper around the raw C ABI (parity tests call through the C ABI)."""

    def __init__(self, lib, rank, implicit=True, reg=0.5, alpha=40.0, light=-1, max_iter=1):
        from albedo_amd import _lib as L
        self.L, self.lib = L, lib
        p = L.als_params()
        L.check(lib.als_params_default(C.byref(p)))
        p.rank, p.implicit_prefs, p.reg_param, p.alpha = rank, int(implicit), reg, alpha
        p.light_max_degree, p.max_iter = light, max_iter
        self.h = C.c_void_p()
        L.check(lib.als_create(C.byref(p), C.byref(self.h)))
        self.rank, self.light = rank, light

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.als_destroy(self.h)

    def ratings(self, user, item, rating):
        L = self.L
        u = np.ascontiguousarray(user, np.int32)
        i = np.ascontiguousarray(item, np.int32)
        r = np.ascontiguousarray(rating, np.float32)
        L.check(self.lib.als_set_ratings(self.h, u.size, L.ptr(u, C.c_int32), L.ptr(i, C.c_int32),
                                         L.ptr(r, C.c_float)))

    def inject(self, side, ids, f):
        L = self.L
        ids = np.ascontiguousarray(ids, np.int32)
        f = np.ascontiguousarray(f, np.float32)
        L.check(self.lib.als_set_initial_factors(self.h, side, ids.size, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float)))

    def factors(self, side):
        L = self.L
        n = self.lib.als_num_rows(self.h, side)
        ids = np.empty(n, np.int32)
        f = np.empty((n, self.rank), np.float32)
        L.check(self.lib.als_get_factors(self.h, side, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float)))
        return ids, f

    def half(self, side):
        self.L.check(self.lib.als_half_sweep(self.h, side))

    def stats(self, side):
        out = np.zeros(4, np.int64)
        self.L.check(self.lib.als_path_stats(self.h, side, self.L.ptr(out, C.c_int64)))
        return out


# ---- ingest + Gram ---------------------------------------------------------------------------

def test_ingest_remap_matches_oracle(gpu_lib):
    f = _g("f1_half_sweep.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    c = Ctx(gpu_lib, 8)
    rng = np.random.default_rng(0)
    perm = rng.permutation(f["user"].size)  # arbitrary input order
    c.ratings(f["user"][perm], f["item"][perm], f["rating"][perm])
    assert gpu_lib.als_num_rows(c.h, 0) == len(B.user_ids)
    assert gpu_lib.als_num_rows(c.h, 1) == len(B.item_ids)
    ids = np.empty(len(B.user_ids), np.int32)
    c.L.check(gpu_lib.als_get_ids(c.h, 0, c.L.ptr(ids, C.c_int32)))
    assert np.array_equal(ids, B.user_ids)


@pytest.mark.parametrize("k", [8, 16])
def test_golden_f1_half_sweep_and_gram(gpu_lib, k):
    f = _g("f1_half_sweep.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    for light in (-1, 0):  # engine default (push-through for light rows) and all-explicit
        c = Ctx(gpu_lib, k, light=light)
        c.ratings(f["user"], f["item"], f["rating"])
        c.inject(0, B.user_ids, f[f"U0_k{k}"])
        c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
        c.half(1)
        ids, V = c.factors(1)
        assert np.array_equal(ids, B.item_ids)
        assert _row_rel(V, f[f"V_k{k}"]) < 1e-4
        G = np.empty((k, k))
        c.L.check(gpu_lib.als_get_gram(c.h, 0, c.L.ptr(G, C.c_double)))
        assert _rel(G, f[f"G_k{k}"]) < 1e-6
        st = c.stats(1)
        assert st[0] + st[2] == len(B.item_ids)
        if light == 0:
            assert st[0] == 0


@pytest.mark.parametrize("k,light", [(50, -1), (50, 0), (64, -1), (100, -1), (128, 0), (128, -1), (128, 96), (200, -1),
                                     (256, 0), (256, -1)])
def test_half_sweep_ranks_and_paths(gpu_lib, k, light):
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(1500, 600, 30000, seed=20 + k))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(k)
    U0 = rng.standard_normal((len(B.user_ids), k)).astype(np.float32)
    U0 /= np.linalg.norm(U0, axis=1, keepdims=True)
    c = Ctx(gpu_lib, k, light=light)
    c.ratings(d["user"], d["item"], d["rating"])
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    V_ref = O.half_sweep(U0, B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0)
    _, V = c.factors(1)
    assert _row_rel(V, V_ref) < 1e-4
    # rows of degree 65..128 named explicitly (the push-through bucket at light = 96, the wave kernel
    # otherwise): 73-77 items and 38-52 users of these sets
    mid = lambda ptr: (np.diff(ptr) > 64) & (np.diff(ptr) <= 128)
    assert mid(B.i_ptr).sum() > 0 and _row_rel(V[mid(B.i_ptr)], V_ref[mid(B.i_ptr)]) < 1e-4
    c.half(0)  # and back: user half-sweep from the GPU's item factors (exercises the basis chain)
    U_ref = O.half_sweep(V, B.u_ptr, B.u_col, B.u_val, reg=0.5, alpha=40.0)
    _, U = c.factors(0)
    assert _row_rel(U, U_ref) < 1e-4
    assert mid(B.u_ptr).sum() > 0 and _row_rel(U[mid(B.u_ptr)], U_ref[mid(B.u_ptr)]) < 1e-4


@pytest.mark.parametrize("k", [64, 128, 256])
def test_heavy_build_column_scaling(gpu_lib, k):
    """The heavy build splits √c·z into fp16 hi + lo with a per-column power-of-two scale: factor
    columns spanning 6 decades of magnitude (and one all-zero column) keep the 1e-4 tolerance."""
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(900, 120, 24000, seed=70 + k))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(k + 1)
    U0 = rng.standard_normal((len(B.user_ids), k)) * np.logspace(-3, 3, k)[None, :]
    U0[:, k // 3] = 0.0
    U0 = U0.astype(np.float32)
    c = Ctx(gpu_lib, k, light=0)  # every row on the heavy (explicit A') path
    c.ratings(d["user"], d["item"], d["rating"])
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    V_ref = O.half_sweep(U0, B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0)
    _, V = c.factors(1)
    assert _row_rel(V, V_ref) < 1e-4


def test_golden_f2_three_sweeps_fit(gpu_lib):
    f = _g("f2_three_sweeps.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    c = Ctx(gpu_lib, 16, max_iter=3)
    c.ratings(f["user"], f["item"], f["rating"])
    c.inject(0, B.user_ids, f["U0"])
    c.inject(1, B.item_ids, f["V0"])
    c.L.check(gpu_lib.als_fit(c.h))
    _, U = c.factors(0)
    _, V = c.factors(1)
    assert _rel(U, f["U"]) < 1e-3 and _rel(V, f["V"]) < 1e-3
    # RMSE of the implicit preference on observed pairs
    def rmse(Uf, Vf):
        p = O.f2j_sdot(Uf[B.u_ptr.searchsorted(np.arange(B.u_col.size), side="right") - 1], Vf[B.u_col])
        return float(np.sqrt(np.mean((p - 1.0) ** 2)))
    assert abs(rmse(U, V) - rmse(f["U"], f["V"])) <= 1e-3 * rmse(f["U"], f["V"])


def test_golden_f3_explicit(gpu_lib):
    f = _g("f3_explicit.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    c = Ctx(gpu_lib, 10, implicit=False, reg=0.1, alpha=1.0, max_iter=2)
    c.ratings(f["user"], f["item"], f["rating"])
    c.inject(0, B.user_ids, f["U0"])
    c.inject(1, B.item_ids, f["V0"])
    c.L.check(gpu_lib.als_fit(c.h))
    assert _rel(c.factors(0)[1], f["U"]) < 1e-3 and _rel(c.factors(1)[1], f["V"]) < 1e-3


@pytest.mark.parametrize("light", [-1, 0])
def test_golden_f6_zero_and_negative_ratings(gpu_lib, light):
    f = _g("f6_zero_negative.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    c = Ctx(gpu_lib, 8, light=light)
    c.ratings(f["user"], f["item"], f["rating"])
    c.inject(1, B.item_ids, f["V0"])
    c.inject(0, B.user_ids, np.zeros((len(B.user_ids), 8), np.float32))
    c.half(0)
    assert _row_rel(c.factors(0)[1], f["U"]) < 1e-4


def test_golden_f7_heavy_row(gpu_lib):
    f = _g("f7_heavy_row.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    assert np.max(np.diff(B.u_ptr)) >= 10000
    c = Ctx(gpu_lib, 16)
    c.ratings(f["user"], f["item"], f["rating"])
    c.inject(1, B.item_ids, f["V0"])
    c.inject(0, B.user_ids, np.zeros((len(B.user_ids), 16), np.float32))
    c.half(0)
    assert _row_rel(c.factors(0)[1], f["U"]) < 1e-4


def test_not_positive_definite_raises(gpu_lib):
    from albedo_amd import IllegalArgumentException
    # explicit, regParam 0, every item rated by one user only: A = y yᵀ is singular for rank 4
    user = np.array([1, 1, 2, 2], np.int32)
    item = np.array([10, 11, 10, 11], np.int32)
    c = Ctx(gpu_lib, 4, implicit=False, reg=0.0, alpha=1.0)
    c.ratings(user, item, np.ones(4, np.float32))
    c.inject(0, [1, 2], np.ones((2, 4), np.float32))
    c.inject(1, [10, 11], np.ones((2, 4), np.float32))
    with pytest.raises(IllegalArgumentException, match="not positive definite"):
        c.half(1)


# ---- Spark-style init, fit through the facade -----------------------------------------------

def test_spark_init_on_device_matches_oracle(gpu_lib):
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(300, 100, 2000, seed=31))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    model = ALS(rank=7, maxIter=0, implicitPrefs=True, seed=42).fit(d)
    su, si = O.spark_side_seeds(42)
    assert np.array_equal(model.user_factors_np()[1], O.spark_initialize(B.user_ids, 7, su))
    assert np.array_equal(model.item_factors_np()[1], O.spark_initialize(B.item_ids, 7, si))


def test_param_grid_fit_shares_ingest(gpu_lib):
    """Estimator.fit(dataset, paramMaps) (the ALSRecommenderCV.scala:67-90 grid): one ingest, the
    rank-dependent layout rebuilt per map (rank 8 -> 70 -> 8 crosses padded ranks 64/128, and the
    light-row limit with them).  Each model equals its own standalone fit bit for bit, and the
    first matches the fp64 oracle."""
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(900, 250, 12000, seed=36))
    base = ALS(implicitPrefs=True, seed=42, maxIter=2)
    grid = [dict(rank=8, regParam=0.5, alpha=40.0), dict(rank=70, regParam=0.1, alpha=10.0),
            dict(rank=8, regParam=0.01, alpha=1.0, maxIter=3, seed=7), dict(rank=16, nonnegative=True)]
    models = base.fit(d, grid)
    assert len(models) == 4
    assert (models[3].user_factors_np()[1] >= 0).all() and (models[3].item_factors_np()[1] >= 0).all()
    for pm, m in zip(grid, models):
        solo = ALS(**{**dict(implicitPrefs=True, seed=42, maxIter=2), **pm}).fit(d)
        assert m.rank == pm["rank"] and m.getRegParam() == pm.get("regParam", base.getRegParam())
        for a, b in ((m.user_factors_np(), solo.user_factors_np()), (m.item_factors_np(), solo.item_factors_np())):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        u = np.array([d["user"][0]], dtype=np.int32)
        assert np.array_equal(m.recommend_np(5, subset=u)[1], solo.recommend_np(5, subset=u)[1])
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    su, si = O.spark_side_seeds(42)
    U, V = O.fit(B, rank=8, max_iter=2, reg=0.5, alpha=40.0, init_user=O.spark_initialize(B.user_ids, 8, su),
                 init_item=O.spark_initialize(B.item_ids, 8, si))
    assert _rel(models[0].user_factors_np()[1], U) < 1e-3
    assert _rel(models[0].item_factors_np()[1], V) < 1e-3
    # a single ParamMap overrides like Estimator.fit(dataset, paramMap)
    one = base.fit(d, dict(rank=8, regParam=0.5, alpha=40.0))
    assert np.array_equal(one.user_factors_np()[1], models[0].user_factors_np()[1])


def test_cv_grid_concurrent_forks(gpu_lib):
    """ALSRecommenderCV.scala:67-72's grid shape (rank {50, 70} x regParam {0.1, 0.5} x alpha {0.1, 40}):
    the four maps of each rank run at once on als_fork contexts from four host threads; every model is
    bit-identical to its standalone fit.  A fork keeps its parent's rank, and the parent's layout is
    frozen while forks view it."""
    import ctypes as C
    from albedo_amd import ALS
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(1500, 300, 20000, seed=44))
    grid = [dict(rank=r, regParam=g, alpha=a) for r in (50, 70) for g in (0.1, 0.5) for a in (0.1, 40.0)]
    base = ALS(implicitPrefs=True, seed=42, maxIter=2)
    models = base.fit(d, grid)
    for pm, m in zip(grid, models):
        solo = ALS(**{**dict(implicitPrefs=True, seed=42, maxIter=2), **pm}).fit(d)
        for a, b in ((m.user_factors_np(), solo.user_factors_np()), (m.item_factors_np(), solo.item_factors_np())):
            assert np.array_equal(a[1], b[1]), pm
    c = Ctx(gpu_lib, 16)
    c.ratings(d["user"], d["item"], d["rating"])
    p = L.als_params()
    L.check(gpu_lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs = 24, 1
    f = C.c_void_p()
    with pytest.raises(L.IllegalArgumentException, match="rank"):
        L.check(gpu_lib.als_fork(c.h, C.byref(p), C.byref(f)))
    p.rank = 16
    L.check(gpu_lib.als_fork(c.h, C.byref(p), C.byref(f)))
    with pytest.raises(L.IllegalStateException):
        L.check(gpu_lib.als_set_params(c.h, C.byref(p)))
    # neither the fork (its ingest is a view) nor the forked parent (viewed) may re-ingest
    u = np.ascontiguousarray(d["user"][:100], np.int32)
    i = np.ascontiguousarray(d["item"][:100], np.int32)
    r = np.ones(100, np.float32)
    for h in (f, c.h):
        with pytest.raises(L.IllegalStateException, match="fork"):
            L.check(gpu_lib.als_set_ratings(h, u.size, L.ptr(u, C.c_int32), L.ptr(i, C.c_int32), L.ptr(r, C.c_float)))
    gpu_lib.als_destroy(c.h)  # the parent outlives it: freed with the fork below
    c.h = None
    L.check(gpu_lib.als_fit(f))
    gpu_lib.als_destroy(f)


def test_cv_grid_light_limit_and_parallelism(gpu_lib):
    """A grid that varies lightMaxDegree (each value its own layout on the parent) fitted with one map
    at a time (parallelism = 1: the sequential path) and with all at once; every model bit-identical
    to its standalone fit."""
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(1200, 250, 16000, seed=45))
    grid = [dict(rank=20, regParam=g, lightMaxDegree=lm) for lm in (0, 16, -1) for g in (0.1, 0.5)]
    base = ALS(implicitPrefs=True, seed=42, maxIter=2, alpha=40.0)
    seq = base.fit(d, grid, parallelism=1)
    par = base.fit(d, grid)
    for pm, a, b in zip(grid, seq, par):
        solo = ALS(**{**dict(implicitPrefs=True, seed=42, maxIter=2, alpha=40.0), **pm}).fit(d)
        for m in (a, b):
            assert np.array_equal(m.user_factors_np()[1], solo.user_factors_np()[1]), pm
            assert np.array_equal(m.item_factors_np()[1], solo.item_factors_np()[1]), pm


def test_facade_fit_matches_oracle_and_ndcg(gpu_lib):
    from albedo_amd import ALS
    from albedo_amd import evaluation as E
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(1200, 300, 14000, seed=32), with_timestamps=True)
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    su, si = O.spark_side_seeds(42)
    U0 = O.spark_initialize(B.user_ids, 12, su)
    V0 = O.spark_initialize(B.item_ids, 12, si)
    U, V = O.fit(B, rank=12, max_iter=4, reg=0.5, alpha=40.0, init_user=U0, init_item=V0)
    als = (ALS().setImplicitPrefs(True).setRank(12).setRegParam(0.5).setAlpha(40).setMaxIter(4).setSeed(42)
           .setColdStartStrategy("drop").setUserCol("user_id").setItemCol("repo_id").setRatingCol("starring"))
    model = als.fit({"user_id": d["user"], "repo_id": d["item"], "starring": d["rating"]})
    assert _rel(model.user_factors_np()[1], U) < 1e-3
    assert _rel(model.item_factors_np()[1], V) < 1e-3
    # albedo protocol: actual = 30 latest stars, predicted = top-30 by score
    actual = E.into_user_items(d["user"], d["item"], d["ts"], 30)
    sample = B.user_ids[::5]
    src, ids, sc = model.recommend_np(30, subset=sample)
    pred_gpu = {int(u): [int(x) for x in ids[r] if x >= 0] for r, u in enumerate(src)}
    oid, _ = O.recommend_for_all(sample, U[np.searchsorted(B.user_ids, sample)], B.item_ids, V, 30)
    pred_ref = {int(u): [int(x) for x in oid[r] if x >= 0] for r, u in enumerate(sample)}
    n_gpu = E.RankingEvaluator(actual, "NDCG@k", 30).evaluate(pred_gpu)
    n_ref = O.evaluate_ndcg(pred_ref, actual, 30)
    assert abs(n_gpu - n_ref) <= 1e-3


# ---- top-k and transform ---------------------------------------------------------------------

@pytest.mark.parametrize("num", [30, 60])
def test_golden_f4_topk_bit_exact_with_ties(gpu_lib, num):
    from albedo_amd import _lib as L
    f = _g("f4_topk_ties.npz")
    h = C.c_void_p()
    uid, uf = np.ascontiguousarray(f["uid"]), np.ascontiguousarray(f["uf"])
    iid, itf = np.ascontiguousarray(f["iid"]), np.ascontiguousarray(f["itf"])
    L.check(gpu_lib.als_model_create(12, uid.size, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), iid.size,
                                     L.ptr(iid, C.c_int32), L.ptr(itf, C.c_float), -1, C.byref(h)))
    try:
        nq = uid.size
        src = np.empty(nq, np.int32)
        ids = np.empty((nq, num), np.int32)
        sc = np.empty((nq, num), np.float32)
        L.check(gpu_lib.als_recommend(h, 0, num, None, nq, L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32),
                                      L.ptr(sc, C.c_float)))
        order = np.argsort(uid)
        assert np.array_equal(src, uid[order])
        assert np.array_equal(ids, f[f"ids{num}"][order])
        assert np.array_equal(sc.view(np.uint32), f[f"sc{num}"][order].view(np.uint32))
    finally:
        gpu_lib.als_destroy(h)


@pytest.mark.parametrize("rank,num", [(50, 30), (100, 64), (200, 30)])
def test_topk_large_catalogue_bit_exact(gpu_lib, rank, num):
    """Top-k over a catalogue of hundreds of LDS chunks (every padded rank: 64, 128, 256), a src count
    that is not a multiple of the 64-row workgroup tile, and exact score ties (duplicated dst
    factor rows, tie-break by id) against the F2J-order oracle, ids and score bits."""
    from albedo_amd import _lib as L
    rng = np.random.default_rng(rank)
    n_u, n_i = 333, 30011
    uid = (np.arange(n_u, dtype=np.int32) * 7 + 11)
    iid = rng.permutation(np.arange(n_i, dtype=np.int32) * 3 + 5).astype(np.int32)
    uf = rng.standard_normal((n_u, rank)).astype(np.float32)
    itf = (rng.standard_normal((n_i, rank)) * rng.uniform(0.2, 1.5, (n_i, 1))).astype(np.float32)
    itf[n_i // 2: n_i // 2 + 200] = itf[:200]  # exact duplicates: equal scores, different ids
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(rank, n_u, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), n_i,
                                     L.ptr(iid, C.c_int32), L.ptr(itf, C.c_float), -1, C.byref(h)))
    try:
        src = np.empty(n_u, np.int32)
        ids = np.empty((n_u, num), np.int32)
        sc = np.empty((n_u, num), np.float32)
        L.check(gpu_lib.als_recommend(h, 0, num, None, n_u, L.ptr(src, C.c_int32), L.ptr(ids, C.c_int32),
                                      L.ptr(sc, C.c_float)))
        ref_ids, ref_sc = O.recommend_for_all(uid, uf, iid, itf, num)
        order = np.argsort(uid)
        assert np.array_equal(src, uid[order])
        assert np.array_equal(ids, ref_ids[order])
        assert np.array_equal(sc.view(np.uint32), ref_sc[order].view(np.uint32))
    finally:
        gpu_lib.als_destroy(h)


@pytest.mark.parametrize("rank,n_u", [(50, 300000), (100, 300000), (200, 140000)])
def test_topk_register_blocking_and_norm_pruning(gpu_lib, rank, n_u):
    """Src counts large enough for the 512- and 256-row scan workgroups (4 waves x 8 / 4 groups of 16
    rows), a catalogue with the skewed norms of trained implicit-ALS factors (so the descending-norm
    scan ends early), ids and score bits of a sample of rows against the F2J-order oracle; the scan
    counters show the early exit and the certification misses stay rare."""
    from albedo_amd import _lib as L
    rng = np.random.default_rng(rank + 1)
    n_i, num = 20000, 30
    uid = np.arange(n_u, dtype=np.int32) * 3 + 1
    iid = rng.permutation(np.arange(n_i, dtype=np.int32) * 2 + 7).astype(np.int32)
    uf = (rng.standard_normal((n_u, rank)) * rng.lognormal(0.0, 0.5, (n_u, 1))).astype(np.float32)
    itf = (rng.standard_normal((n_i, rank)) * rng.lognormal(0.0, 1.0, (n_i, 1))).astype(np.float32)
    itf[n_i - 300:] = itf[:300]  # exact ties across the norm order
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(rank, n_u, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), n_i,
                                     L.ptr(iid, C.c_int32), L.ptr(itf, C.c_float), -1, C.byref(h)))
    try:
        ids = np.empty((n_u, num), np.int32)
        sc = np.empty((n_u, num), np.float32)
        L.check(gpu_lib.als_recommend(h, 0, num, None, n_u, None, L.ptr(ids, C.c_int32), L.ptr(sc, C.c_float)))
        st = np.zeros(4, np.int64)
        L.check(gpu_lib.als_topk_stats(h, L.ptr(st, C.c_int64)))
        assert st[0] == n_u
        assert st[1] <= n_u // 100, f"certification misses {st[1]} of {n_u}"
        assert 0 < st[2] < st[3], f"scan chunks {st[2]} of {st[3]}: no early exit"
        samp = np.sort(rng.choice(n_u, 600, replace=False))
        samp[:4] = [0, 1, n_u - 2, n_u - 1]
        ref_ids, ref_sc = O.recommend_for_all(uid[samp], uf[samp], iid, itf, num)
        assert np.array_equal(ids[samp], ref_ids)
        assert np.array_equal(sc[samp].view(np.uint32), ref_sc.view(np.uint32))
    finally:
        gpu_lib.als_destroy(h)


@pytest.mark.parametrize("num", [100, 300])
def test_topk_above_64_exact_scan(gpu_lib, num):
    """k > 64 (Spark's recommendForAllUsers takes any k): exact full-scan path, ids and F2J score
    bits against the oracle, ties included; k above the engine's 512 raises."""
    from albedo_amd import _lib as L
    rng = np.random.default_rng(num)
    n_u, n_i, rank = 70, 5003, 40
    uid = np.arange(n_u, dtype=np.int32) * 5 + 1
    iid = rng.permutation(np.arange(n_i, dtype=np.int32) * 3 + 2).astype(np.int32)
    uf = rng.standard_normal((n_u, rank)).astype(np.float32)
    itf = rng.standard_normal((n_i, rank)).astype(np.float32)
    itf[2500:2600] = itf[:100]  # exact ties
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(rank, n_u, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), n_i,
                                     L.ptr(iid, C.c_int32), L.ptr(itf, C.c_float), -1, C.byref(h)))
    try:
        ids = np.empty((n_u, num), np.int32)
        sc = np.empty((n_u, num), np.float32)
        L.check(gpu_lib.als_recommend(h, 0, num, None, n_u, None, L.ptr(ids, C.c_int32), L.ptr(sc, C.c_float)))
        ref_ids, ref_sc = O.recommend_for_all(uid, uf, iid, itf, num)
        assert np.array_equal(ids, ref_ids)
        assert np.array_equal(sc.view(np.uint32), ref_sc.view(np.uint32))
        big = np.empty((n_u, 513), np.int32)
        with pytest.raises(L.ALSError, match="not supported"):
            L.check(gpu_lib.als_recommend(h, 0, 513, None, n_u, None, L.ptr(big, C.c_int32),
                                          L.ptr(np.empty((n_u, 513), np.float32), C.c_float)))
    finally:
        gpu_lib.als_destroy(h)


def test_topk_subset_unknown_ids_and_small_catalogue(gpu_lib):
    from albedo_amd import _lib as L
    rng = np.random.default_rng(7)
    uid = np.arange(50, dtype=np.int32) * 3
    iid = np.arange(20, dtype=np.int32) * 5 - 40  # fewer items than k
    uf = rng.standard_normal((50, 9)).astype(np.float32)
    itf = rng.standard_normal((20, 9)).astype(np.float32)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(9, 50, L.ptr(uid, C.c_int32), L.ptr(uf, C.c_float), 20, L.ptr(iid, C.c_int32),
                                     L.ptr(itf, C.c_float), -1, C.byref(h)))
    try:
        sub = np.array([3, 4, 147], np.int32)  # 4 is unknown
        ids = np.empty((3, 30), np.int32)
        sc = np.empty((3, 30), np.float32)
        L.check(gpu_lib.als_recommend(h, 0, 30, L.ptr(sub, C.c_int32), 3, None, L.ptr(ids, C.c_int32),
                                      L.ptr(sc, C.c_float)))
        ref, rs = O.recommend_for_all(np.array([3, 147]), uf[[1, 49]], iid, itf, 30)
        assert np.array_equal(ids[[0, 2]], ref)
        assert np.all(ids[1] == -1) and np.all(np.isnan(sc[1]))
        assert np.all(ids[0, 20:] == -1)
    finally:
        gpu_lib.als_destroy(h)


@pytest.mark.parametrize("k", [30, 10])
def test_device_ndcg_matches_oracle(gpu_lib, k):
    """RankingEvaluator on the device (als_evaluate_ndcg): actual lists = rank() over starred_at desc
    (engineered timestamp ties, users with fewer and more than k stars, duplicated (user, item) rows
    whose label SET is smaller than the list), predicted = the top-k lists; ndcgAt per user
    bit-identical to the oracle's (oracle/spark_als.py ndcg_at / into_user_items, which restate
    RankingEvaluator.scala:83-139 and mllib RankingMetrics.ndcgAt), the mean within 1e-12 of
    O.evaluate_ndcg; users unknown to the model are dropped by the join."""
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(2500, 600, 40000, seed=19), with_timestamps=True)
    model = ALS(rank=24, maxIter=3, regParam=0.5, alpha=40.0, implicitPrefs=True).fit(d)
    rng = np.random.default_rng(k)
    ts = d["ts"] // 1_000_000  # coarse: many equal timestamps within a user (rank() ties)
    dup = rng.choice(d["user"].size, 400, replace=False)  # the same (user, item) again, a later star
    users = np.r_[d["user"], d["user"][dup], np.full(5, 123456789, np.int32)]  # + an unknown id
    items = np.r_[d["item"], d["item"][dup], d["item"][:5]]
    keys = np.r_[ts, ts[dup] + 1 + rng.integers(0, 3, dup.size), ts[:5]]
    perm = rng.permutation(users.size)  # any input order
    mean, uids, vals = model.evaluate_ndcg(users[perm], items[perm], keys[perm], k=k, per_user=True)
    actual = O.into_user_items(users, items, keys, k)
    assert any(len(set(actual[int(u)][:k])) < len(actual[int(u)][:k]) for u in d["user"][dup])
    src, ids, _ = model.recommend_np(k, subset=uids)
    assert np.array_equal(src, uids)
    pred = {int(u): [int(x) for x in ids[r] if x >= 0] for r, u in enumerate(src)}
    assert 123456789 not in set(uids.tolist()) and uids.size == np.unique(d["user"]).size
    ref = [O.ndcg_at([(pred[int(u)][:k], actual[int(u)][:k])], k) for u in uids]
    assert np.array_equal(vals, np.asarray(ref))
    host = O.evaluate_ndcg(pred, actual, k)
    assert abs(mean - host) <= 1e-12 * max(1.0, abs(host))


def test_recommend_for_all_items_and_item_subset(gpu_lib):
    """recommendForAllItems / recommendForItemSubset (Spark ALSModel, side = item): every item's top-k
    users, ids and F2J score bits against the oracle scorer with the roles swapped; a subset with an
    unknown item id gets an empty row."""
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(3000, 400, 30000, seed=27))
    model = ALS(rank=20, maxIter=3, regParam=0.5, alpha=40.0, implicitPrefs=True).fit(d)
    uids, uf = model.user_factors_np()
    iids, itf = model.item_factors_np()
    for num in (30, 100):
        src, ids, sc = model.recommend_np(num, side=1)
        assert np.array_equal(src, iids)
        ref_ids, ref_sc = O.recommend_for_all(iids, itf, uids, uf, num)
        assert np.array_equal(ids, ref_ids)
        assert np.array_equal(sc.view(np.uint32), ref_sc.view(np.uint32))
    sub = np.array([iids[5], 2_000_000_000, iids[-1]], np.int64)
    df = model.recommendForItemSubset({"item": sub}, 10)
    assert sorted(df["item"].tolist()) == sorted([int(iids[5]), int(iids[-1])])
    full = model.recommendForAllItems(10)
    assert len(full) == iids.size
    row = full[full["item"] == iids[5]]["recommendations"].iloc[0]
    ref_ids, _ = O.recommend_for_all(iids[5:6], itf[5:6], uids, uf, 10)
    assert [u for u, _ in row] == ref_ids[0].tolist()


def test_transform_bit_exact_and_cold_start(gpu_lib):
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(400, 150, 4000, seed=33))
    model = ALS(rank=11, maxIter=2, implicitPrefs=True, regParam=0.5, alpha=40.0,
                coldStartStrategy="drop").fit(d)
    uids, uf = model.user_factors_np()
    iids, itf = model.item_factors_np()
    q = {"user": np.r_[d["user"][:500], np.int32(-999)], "item": np.r_[d["item"][:500], d["item"][0]]}
    out = model.transform(q)
    assert len(out) == 500  # the unknown user is dropped
    ref = O.f2j_sdot(uf[np.searchsorted(uids, q["user"][:500])], itf[np.searchsorted(iids, q["item"][:500])])
    assert np.array_equal(out["prediction"].to_numpy().view(np.uint32), ref.view(np.uint32))
    model.setColdStartStrategy("nan")
    out2 = model.transform(q)
    assert len(out2) == 501 and np.isnan(out2["prediction"].to_numpy()[-1])


def test_model_save_load_roundtrip(gpu_lib, tmp_path):
    from albedo_amd import ALS, ALSModel
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(300, 120, 3000, seed=34))
    model = ALS(rank=6, maxIter=2, implicitPrefs=True).fit(d)
    path = str(tmp_path / "alsModel.parquet")
    model.write().overwrite().save(path)
    m2 = ALSModel.load(path)
    assert m2.rank == 6
    assert np.array_equal(m2.user_factors_np()[1], model.user_factors_np()[1])
    a = model.recommend_np(10)
    b = m2.recommend_np(10)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- generator twin, scale properties ---------------------------------------------------------

def test_device_synthetic_generator_matches_numpy(gpu_lib):
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import SynthSpec, generate, popularity_table, user_degrees
    spec = SynthSpec(3000, 500, 60000, seed=35)
    ref = generate(spec)
    deg = user_degrees(spec)
    prefix = np.ascontiguousarray(np.r_[0, np.cumsum(deg)].astype(np.int64))
    cw, perm = popularity_table(spec)
    cw = np.ascontiguousarray(cw)
    perm = np.ascontiguousarray(perm)
    n = int(prefix[-1])
    u = np.empty(n, np.int32)
    i = np.empty(n, np.int32)
    r = np.empty(n, np.float32)
    nout = C.c_int64()
    L.check(gpu_lib.als_synth_generate(-1, spec.seed, spec.rounds, spec.n_users, spec.n_items,
                                       L.ptr(prefix, C.c_int64), L.ptr(cw, C.c_double), L.ptr(perm, C.c_int32),
                                       L.ptr(u, C.c_int32), L.ptr(i, C.c_int32), L.ptr(r, C.c_float), C.byref(nout)))
    m = nout.value
    assert m == ref["user"].size
    assert np.array_equal(u[:m], ref["user"]) and np.array_equal(i[:m], ref["item"])


def _gram_fp64(Y, chunk=1 << 20):
    """YᵀY in fp64, accumulated over row chunks (no fp64 copy of a 20M-row factor matrix)."""
    G = np.zeros((Y.shape[1], Y.shape[1]))
    for r0 in range(0, Y.shape[0], chunk):
        Yc = Y[r0:r0 + chunk].astype(np.float64)
        G += Yc.T @ Yc
    return G


def _check_rows_fp64(gpu_lib, c, side, rows_ids, X_ids, X, Y_ids, Y, k, gram=None):
    """Rows `rows_ids` of `side` (solved into X) equal the fp64 solve of Spark's implicit normal
    equation from the src factors Y, built from the engine's own CSR; returns the worst error."""
    from albedo_amd import _lib as L
    from tests.ladder import padded_rank, path_of, split_chunk
    G = _gram_fp64(Y) if gram is None else gram
    n_row = np.empty(1, np.int64)
    worst = 0.0
    for rid in rows_ids:
        L.check(gpu_lib.als_get_row_ratings(c.h, side, int(rid), 0, None, None, L.ptr(n_row, C.c_int64)))
        cap = int(n_row[0])
        src = np.empty(max(cap, 1), np.int32)
        rat = np.empty(max(cap, 1), np.float32)
        L.check(gpu_lib.als_get_row_ratings(c.h, side, int(rid), cap, L.ptr(src, C.c_int32), L.ptr(rat, C.c_float),
                                            L.ptr(n_row, C.c_int64)))
        n = int(n_row[0])
        Yr = Y[np.searchsorted(Y_ids, src[:n])].astype(np.float64)
        cvec = 40.0 * np.abs(rat[:n].astype(np.float64))
        A = G + (Yr.T * cvec) @ Yr + 0.5 * np.sum(rat[:n] > 0) * np.eye(k)
        b = Yr.T @ np.where(rat[:n] > 0, 1.0 + cvec, 0.0)
        x = np.linalg.solve(A, b)
        err = np.max(np.abs(X[np.searchsorted(X_ids, rid)] - x)) / np.max(np.abs(x))
        assert err < 1e-4, (f"side {side} id {rid} ({n} ratings, path "
                            f"{path_of(n, padded_rank(c.rank), c.light, split_chunk())}): rel err {err:.3e}")
        worst = max(worst, float(err))
    return worst


# ---- NNLS (nonnegative = true) --------------------------------------------------------------

def test_golden_f5_nnls_half_sweep_and_fit(gpu_lib):
    from albedo_amd import _lib as L
    f = _g("f5_nnls.npz")
    B = O.make_blocks(f["user"], f["item"], f["rating"])
    c = Ctx(gpu_lib, 16)
    # nonnegative context
    p = L.als_params()
    L.check(gpu_lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative, p.max_iter = 16, 1, 0.5, 40.0, 1, 2
    h = C.c_void_p()
    L.check(gpu_lib.als_create(C.byref(p), C.byref(h)))
    c.h = h
    c.ratings(f["user"], f["item"], f["rating"])
    c.inject(0, B.user_ids, f["U0"])
    c.inject(1, B.item_ids, f["V0"])
    c.half(1)
    V1 = c.factors(1)[1]
    assert np.all(V1 >= 0)
    assert _rel(V1, f["V1"]) < 1e-3
    zeros_ref = f["V1"] == 0
    assert np.mean((V1 == 0) == zeros_ref) > 0.995  # same active set up to fp32 ties
    c.inject(1, B.item_ids, f["V0"])
    c.L.check(gpu_lib.als_fit(c.h))
    assert _rel(c.factors(0)[1], f["U"]) < 1e-3 and _rel(c.factors(1)[1], f["V"]) < 1e-3


def test_nnls_facade_rank50(gpu_lib):
    from albedo_amd import ALS
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(500, 160, 6000, seed=36))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(9)
    U0 = np.abs(rng.standard_normal((len(B.user_ids), 50))).astype(np.float32)
    V0 = np.abs(rng.standard_normal((len(B.item_ids), 50))).astype(np.float32)
    model = ALS(rank=50, maxIter=1, implicitPrefs=True, regParam=0.5, alpha=40.0, nonnegative=True).fit(
        d, initialUserFactors=(B.user_ids, U0), initialItemFactors=(B.item_ids, V0))
    U, V = O.fit(B, rank=50, max_iter=1, reg=0.5, alpha=40.0, nonnegative=True, init_user=U0, init_item=V0)
    assert np.all(model.user_factors_np()[1] >= 0)
    assert _rel(model.item_factors_np()[1], V) < 1e-3
    assert _rel(model.user_factors_np()[1], U) < 1e-3


def test_nnls_rank256(gpu_lib):
    """nonnegative=true at rank 256 (BASELINE config 5's solver and rank), one half-sweep each way."""
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(160, 60, 2400, seed=41))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    k = 256
    rng = np.random.default_rng(5)
    U0 = np.abs(rng.standard_normal((len(B.user_ids), k))).astype(np.float32)
    U0 /= np.linalg.norm(U0, axis=1, keepdims=True)
    p = L.als_params()
    L.check(gpu_lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative = k, 1, 0.5, 40.0, 1
    c = Ctx(gpu_lib, 8)
    h = C.c_void_p()
    L.check(gpu_lib.als_create(C.byref(p), C.byref(h)))
    gpu_lib.als_destroy(c.h)
    c.h, c.rank = h, k
    c.ratings(d["user"], d["item"], d["rating"])
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    V_ref = O.half_sweep(U0, B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0, nonnegative=True)
    _, V = c.factors(1)
    assert np.all(V >= 0)
    assert _rel(V, V_ref) < 1e-3


@pytest.mark.parametrize("kernel", ["512", "1024"])
def test_nnls_rank256_per_row_kernels(gpu_lib, monkeypatch, kernel):
    """The rank-256 per-row NNLS kernels (nnls_row.hip: 512 threads, two rows per CU, upper tiles in
    registers; als_kernels.hip: 1024 threads, all of A in registers; ALBEDO_NNLS_ROW picks) on rows of
    degree 100-900, against the fp64 oracle: factors within 1e-3, every row stopped by Spark's rule
    before the iteration cap (a wrong A·v or vᵀAv still converges through the residual refreshes but
    runs to the cap), and the same iteration count as the other kernel to within 15 %."""
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(1200, 40, 14000, seed=47))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    k = 256
    rng = np.random.default_rng(9)
    U0 = np.abs(rng.standard_normal((len(B.user_ids), k))).astype(np.float32)
    U0 /= np.linalg.norm(U0, axis=1, keepdims=True)
    U0[:, ::5] *= -1.0  # some coordinates end on the wall
    V_ref = O.half_sweep(U0, B.i_ptr, B.i_col, B.i_val, reg=0.5, alpha=40.0, nonnegative=True)
    its = {}
    for kern in (kernel, "1024" if kernel == "512" else "512"):
        monkeypatch.setenv("ALBEDO_NNLS_ROW", kern)
        p = L.als_params()
        L.check(gpu_lib.als_params_default(C.byref(p)))
        p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative = k, 1, 0.5, 40.0, 1
        c = Ctx(gpu_lib, 8)
        h = C.c_void_p()
        L.check(gpu_lib.als_create(C.byref(p), C.byref(h)))
        gpu_lib.als_destroy(c.h)
        c.h, c.rank = h, k
        c.ratings(d["user"], d["item"], d["rating"])
        c.inject(0, B.user_ids, U0)
        c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
        c.half(1)
        st = np.zeros(4, np.int64)
        L.check(gpu_lib.als_path_stats(c.h, 1, L.ptr(st, C.c_int64)))
        assert st[2] >= 30  # the per-row kernel's rows
        sv = np.zeros(4, np.int64)
        L.check(gpu_lib.als_solver_stats(c.h, 1, L.ptr(sv, C.c_int64)))
        assert sv[1] < 20 * k, f"a row ran to the iteration cap ({sv[1]})"
        its[kern] = (sv[0] - sv[3]) / max(1, st[2])
        _, V = c.factors(1)
        if kern == kernel:
            assert np.all(V >= 0)
            assert _rel(V, V_ref) < 1e-3
    assert abs(its["512"] - its["1024"]) <= 0.15 * its["1024"], its


@pytest.mark.parametrize("k,wgs", [(50, 0), (50, 3), (100, 2), (256, 1)])
def test_nnls_lockstep_light_rows(gpu_lib, monkeypatch, k, wgs):
    """Light NNLS rows run in lockstep (nnls_batch.hip), 16/8/4/2/1 rows per workgroup by degree
    (KP = 256: degree <= 6 / 12 / 24 / 48 / 96): the user half of a set whose users mostly have 1-6
    stars and reach ~40, row count not a multiple of 16, against the fp64 oracle.  wgs > 0 caps the
    persistent grid so that every workgroup refills its slots many times.  The path split is checked
    through als_path_stats (light = lockstep rows)."""
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import SynthSpec, generate
    if wgs:
        monkeypatch.setenv("ALBEDO_NNLS_BATCH_WGS", str(wgs))
    n_users = 330 if k == 256 else 613
    d = generate(SynthSpec(n_users, 90, n_users * 4 + 150, seed=43 + k))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(k)
    V0 = np.abs(rng.standard_normal((len(B.item_ids), k))).astype(np.float32)
    V0 /= np.linalg.norm(V0, axis=1, keepdims=True)
    V0[:, ::3] *= -1.0  # mixed signs: some coordinates end on the wall, others inside
    p = L.als_params()
    L.check(gpu_lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative = k, 1, 0.5, 40.0, 1
    c = Ctx(gpu_lib, 8)
    h = C.c_void_p()
    L.check(gpu_lib.als_create(C.byref(p), C.byref(h)))
    gpu_lib.als_destroy(c.h)
    c.h, c.rank = h, k
    c.ratings(d["user"], d["item"], d["rating"])
    c.inject(1, B.item_ids, V0)
    c.inject(0, B.user_ids, np.zeros((len(B.user_ids), k), np.float32))
    c.half(0)
    st = np.zeros(4, np.int64)
    L.check(gpu_lib.als_path_stats(c.h, 0, L.ptr(st, C.c_int64)))
    kp = 64 if k <= 64 else (128 if k <= 128 else 256)
    # light rows (degree <= the light limit) up to the 8-slot variant's limit run in lockstep
    lim = min(32 if k <= 64 else 64, 24576 // (8 * kp))
    deg = np.diff(B.u_ptr)
    assert st[0] == int(np.sum(deg <= lim)) and st[0] > 250
    if k == 50:
        assert st[2] > 0  # and the rest on the per-row kernel
    U_ref = O.half_sweep(V0, B.u_ptr, B.u_col, B.u_val, reg=0.5, alpha=40.0, nonnegative=True)
    _, U = c.factors(0)
    assert np.all(U >= 0)
    assert _rel(U, U_ref) < 1e-3
    assert np.mean((U == 0) == (U_ref == 0)) > 0.995


@pytest.mark.parametrize("k", [50, 128])
def test_bases_stay_orthogonal_over_many_sweeps(gpu_lib, k):
    """The warm-started device eigensolver chains the bases (W = B_sᵀB_t, B_t <- B_s·W·J): both must
    stay orthogonal to rounding over a long fit (their errors were once coupled and grew ~2.5x per
    half-sweep), and the last half must still match the fp64 solve from the device's own factors."""
    from albedo_amd.synthetic import SynthSpec, generate
    d = generate(SynthSpec(3000, 800, 40000, seed=90 + k))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    c = Ctx(gpu_lib, k)
    c.ratings(d["user"], d["item"], d["rating"])
    rng = np.random.default_rng(k)
    c.inject(0, B.user_ids, (rng.standard_normal((len(B.user_ids), k)) * 0.1).astype(np.float32))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    for h in range(60):
        c.half(1 - (h % 2))
    for side in (0, 1):
        b = np.zeros((k, k))
        c.L.check(gpu_lib.als_get_basis(c.h, side, c.L.ptr(b, C.c_double)))
        assert np.abs(b.T @ b - np.eye(k)).max() < 1e-13, side
    _, V = c.factors(1)
    c.half(0)
    U_ref = O.half_sweep(V, B.u_ptr, B.u_col, B.u_val, reg=0.5, alpha=40.0)
    _, U = c.factors(0)
    assert _row_rel(U, U_ref) < 1e-4


@pytest.mark.parametrize("k", [50, 128, 200])
def test_device_eigensolver(gpu_lib, k):
    """The half-sweep's device eigensolver (eig.hip, warm-started cyclic Jacobi in fp64) on Grams of
    factor-like rows whose columns span 3.5 decades (eigenvalues over 7): eigenvalues equal LAPACK's,
    V orthogonal, VᵀGV diagonal to fp64 precision, cold and warm-started from the eigenvectors of a
    nearby Gram (the next sweep's situation), with the warm start taking few sweeps."""
    from albedo_amd import _lib as L
    rng = np.random.default_rng(k)
    X = rng.standard_normal((20000, k)) * np.logspace(0, 3.5, k)
    G = X.T @ X
    X2 = X + 0.01 * rng.standard_normal(X.shape) * np.logspace(0, 3.5, k)
    G2 = X2.T @ X2
    ref = np.linalg.eigvalsh(G)
    out = {}
    for name, g, w0 in (("cold", G, None), ("warm", G2, "cold")):
        w = np.empty(k)
        V = np.empty((k, k))
        sw = np.zeros(1, np.int32)
        W0 = None if w0 is None else np.ascontiguousarray(out[w0][1])
        L.check(gpu_lib.als_device_eigh(0, k, L.ptr(np.ascontiguousarray(g), C.c_double),
                                        None if W0 is None else L.ptr(W0, C.c_double), L.ptr(w, C.c_double),
                                        L.ptr(V, C.c_double), L.ptr(sw, C.c_int32)))
        out[name] = (w, V, int(sw[0]))
        # the solver stops once the off-diagonal norm is below 1e-14 of the diagonal's (Frobenius,
        # eig.hip JAC_TOL) or at the rounding floor: a backward error of the order of Householder + QL
        gn = np.linalg.norm(g)
        assert np.abs(V.T @ V - np.eye(k)).max() < 1e-12, name
        assert np.linalg.norm(V.T @ g @ V - np.diag(w)) < 1e-12 * gn, name
        assert np.abs(np.sort(w) - np.linalg.eigvalsh(g)).max() < 1e-12 * gn, name
    assert np.abs(np.sort(out["cold"][0]) - ref).max() < 1e-12 * np.linalg.norm(G)
    assert out["cold"][2] <= 12 and out["warm"][2] <= out["cold"][2], (out["cold"][2], out["warm"][2])


@pytest.mark.parametrize("k", [50, 200])
def test_eigensolver_budget_exhausted_raises(gpu_lib, monkeypatch, k):
    """A Jacobi run that spends its sweep budget without converging is an error, as the host
    eigensolver's "did not converge" was: als_device_eigh and a half-sweep both fail with
    ALS_E_NOT_POSITIVE_DEFINITE instead of solving in a basis that does not diagonalise the Gram.
    ALBEDO_JAC_MAX_SWEEPS=1 (test knob) forces it; the default budget then solves the same inputs."""
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import SynthSpec, generate
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4000, k)) * np.logspace(0, 2, k)
    G = np.ascontiguousarray(X.T @ X)
    w = np.empty(k)
    V = np.empty((k, k))
    sw = np.zeros(1, np.int32)
    args = (0, k, L.ptr(G, C.c_double), None, L.ptr(w, C.c_double), L.ptr(V, C.c_double), L.ptr(sw, C.c_int32))
    monkeypatch.setenv("ALBEDO_JAC_MAX_SWEEPS", "1")
    assert gpu_lib.als_device_eigh(*args) == 2
    assert "did not converge" in gpu_lib.als_last_error().decode()
    d = generate(SynthSpec(800, 300, 12000, seed=k))
    B = O.make_blocks(d["user"], d["item"], d["rating"])
    c = Ctx(gpu_lib, k)
    c.ratings(d["user"], d["item"], d["rating"])
    c.inject(0, B.user_ids, rng.standard_normal((len(B.user_ids), k)).astype(np.float32))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    assert gpu_lib.als_half_sweep(c.h, 1) == 2
    assert "did not converge" in gpu_lib.als_last_error().decode()
    monkeypatch.delenv("ALBEDO_JAC_MAX_SWEEPS")
    L.check(gpu_lib.als_device_eigh(*args))
    assert 1 < sw[0] <= 12
    c.half(1)
