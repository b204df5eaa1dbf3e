"""GPU parity with explicit and non-unit ratings on every solve path.

The synthetic generator's ratings are all 1.0, so the other parity tests reach the rank-128 / 256
kernels in implicit mode with one confidence only (the pre-split wave build).  Here the degree ladder
of tests/ladder.py (item rows on both sides of every degree at which the engine changes kernel, user
rows of degree 1..~18) is solved in five rating modes:

  varying         implicit, alpha 10, r in {0.25, 0.5, 1, 2, 4}: per-rating confidence (in-kernel split)
  signed_uniform  implicit, alpha 20, r = +-2: one |r|, so the pre-split build, with w = 0 entries
  mixed           implicit, alpha 10, `varying` with zeros, negatives and item rows without a positive
                  rating (lambda·n = 0, b = 0: the solution is exactly 0)
  stars           explicit, reg 0.1, r in 1..5
  stars_signed    explicit, reg 0.1, r in -5..5 with exact zeros (which still add y yT and count in n)

Tolerances (those of tests/test_gpu_parity.py): every Cholesky row max|x - x64| / max|x64| < 1e-4
against the fp64 oracle (the systems' fp64 condition numbers are below 150 on the item half and
below 3e3 on the user half, so an fp32 solve has two decades of room); NNLS factors >= 0, within 1e-3 of the oracle and the same zero pattern on
more than 99.5 % of the entries; a fit within 1e-3.  Every row carries its path label (restated by
tests/ladder.py:path_of and pinned to the engine through als_path_stats), and a failure names the
failing rows.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cbind
from oracle import spark_als as O
from tests import ladder as LD
from tests import nnls_cases as NC
from tests.test_gpu_parity import Ctx, _rel, _row_rel

pytestmark = pytest.mark.gpu

TOL = 1e-4


@functools.lru_cache(maxsize=None)
def _data(mode):
    user, item, ideg = LD.ladder_coo()
    r = LD.ladder_ratings(mode, user, ideg)
    return user, item, r, O.make_blocks(user, item, r)


@functools.lru_cache(maxsize=None)
def _src(k, n, kind):
    """The user factors the item half starts from: unit-norm Gaussian rows; "wide": columns scaled over
    six decades with one zero column (test_heavy_build_column_scaling's recipe); "nonneg": the NNLS
    tests' |Gaussian| rows with every 5th column negated."""
    F = LD.unit_rows(np.random.default_rng(k), n, k, nonneg=kind == "nonneg")
    if kind == "wide":
        F = F.astype(np.float64) * np.logspace(-3, 3, k)[None, :]
        F[:, k // 3] = 0.0
        F = F.astype(np.float32)
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def _item_ref(mode, k, kind):
    """The oracle's item half, shared by the configurations of one (mode, rank)."""
    implicit, alpha, reg = LD.MODES[mode]
    B = _data(mode)[3]
    V = O.half_sweep(_src(k, len(B.user_ids), kind), B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit)
    V.setflags(write=False)
    return V


def _set_chunk(monkeypatch, chunk):
    """ALBEDO_SPLIT_CHUNK is read at ingest: set it before als_set_ratings.  Returns the chunk length."""
    if chunk:
        monkeypatch.setenv("ALBEDO_SPLIT_CHUNK", chunk)
    else:
        monkeypatch.delenv("ALBEDO_SPLIT_CHUNK", raising=False)
    return LD.split_chunk(chunk or str(LD.DEFAULT_SPLIT_CHUNK))


def _check_paths(c, side, deg, paths, KP, light, chunk):
    """The test-side labels agree with the engine's own split (als_path_stats: light rows, their
    ratings, the other rows, their ratings), and every path this configuration is meant to reach
    holds at least 2 rows."""
    is_light = np.array([p.startswith("light") for p in paths])
    want = [int(is_light.sum()), int(deg[is_light].sum()), int((~is_light).sum()), int(deg[~is_light].sum())]
    assert c.stats(side).tolist() == want, (side, c.stats(side).tolist(), want)
    for p in LD.expected_paths(KP, light, chunk, int(deg.max())):
        assert np.sum(paths == p) >= 2, (side, p)


def _cholesky_case(gpu_lib, monkeypatch, tmp_path, mode, cfg, kind="unit", both_halves=True):
    k, light, chunk = cfg
    implicit, alpha, reg = LD.MODES[mode]
    ch = _set_chunk(monkeypatch, chunk)
    KP = LD.padded_rank(k)
    user, item, r, B = _data(mode)
    U0 = _src(k, len(B.user_ids), kind)
    c = Ctx(gpu_lib, k, implicit=implicit, reg=reg, alpha=alpha, light=light)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    tag = f"{mode}-{LD.config_id(cfg)}" + ("" if kind == "unit" else f"-{kind}")
    for side, ids_ref, ptr in ((1, B.item_ids, B.i_ptr), (0, B.user_ids, B.u_ptr)):
        c.half(side)
        ids, X = c.factors(side)
        assert np.array_equal(ids, ids_ref)
        deg = np.diff(ptr)
        paths = np.array([LD.path_of(d, KP, light, ch) for d in deg])
        _check_paths(c, side, deg, paths, KP, light, ch)
        if side == 1:
            X_ref = _item_ref(mode, k, kind)
            V = X
        else:  # from the device's own item factors (implicit: through the basis chain)
            X_ref = O.half_sweep(V, B.u_ptr, B.u_col, B.u_val, reg=reg, alpha=alpha, implicit=implicit)
        zero = ~X_ref.any(axis=1)
        if mode == "mixed" and side == 1:
            assert zero.sum() >= 4  # rows without a positive rating: exactly 0 on the device (assert_rows)
        name = "item" if side else "user"
        err = LD.row_errors(X, X_ref)
        by_path = ", ".join(f"{p} {err[paths == p].max():.2e}" for p in sorted(set(paths.tolist())))
        print(f"RATING_MODES {tag} KP {KP} {name} half: worst row {_row_rel(X[~zero], X_ref[~zero]):.3e}, "
              f"zero rows {int(zero.sum())}, by path {by_path}")
        LD.assert_rows(X, X_ref, ids, deg, paths, TOL, f"{name} half [{tag}]", tmp_path)
        if not both_halves:
            break


@pytest.mark.parametrize("cfg", LD.CONFIGS, ids=LD.config_id)
@pytest.mark.parametrize("mode", list(LD.MODES))
def test_half_sweeps_rating_modes(gpu_lib, monkeypatch, tmp_path, mode, cfg):
    """Item half from injected unit-norm user factors, then the user half from the device's own item
    factors, every row against the fp64 oracle at 1e-4, rows without a positive rating exactly 0."""
    _cholesky_case(gpu_lib, monkeypatch, tmp_path, mode, cfg)


def test_wide_columns_with_varying_confidence(gpu_lib, monkeypatch, tmp_path):
    """Rank 128 with every row on the wave kernel, per-rating confidence (so the fp16 hi + lo split of
    √c·z runs inside the kernel) and src columns spanning six decades with one zero column."""
    _cholesky_case(gpu_lib, monkeypatch, tmp_path, "varying", (128, 0, None), kind="wide", both_halves=False)


# ---- NNLS ----------------------------------------------------------------------------------------

def _nnls_ctx(gpu_lib, k, implicit, reg, alpha):
    from albedo_amd import _lib as L
    c = Ctx(gpu_lib, 8)
    p = L.als_params()
    L.check(gpu_lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative = k, int(implicit), reg, alpha, 1
    h = C.c_void_p()
    L.check(gpu_lib.als_create(C.byref(p), C.byref(h)))
    gpu_lib.als_destroy(c.h)
    c.h, c.rank = h, k
    return c


def _nnls_path_of(d, KP, chunk):
    """Lockstep rows (nnls_batch.hip) up to the 8-slot variant's degree limit, the per-row kernel above
    it, split-K partials + the per-row kernel on the reduced record above the chunk length."""
    lim = min(LD.light_limit(KP, -1), 24576 // (8 * KP))
    return "nnls-lockstep" if d <= lim else ("nnls-split" if 0 < chunk < d else "nnls-row")


@pytest.mark.parametrize("k,chunk", [(50, None), (100, None), (128, None), (256, None), (256, "256")],
                         ids=["k50-chunkdefault", "k100-chunkdefault", "k128-chunkdefault", "k256-chunkdefault", "k256-chunk256"])
@pytest.mark.parametrize("mode", ["mixed", "stars", "stars_signed"])
def test_nnls_rating_modes(gpu_lib, monkeypatch, tmp_path, mode, k, chunk):
    """nonnegative = true on the ladder: the item half runs the per-row kernels (and split-K + the
    prebuilt NNLS at a chunk of 256), the user half the lockstep kernel, against the C restatement of
    Spark's NNLSSolver (pinned to the numpy oracle in these modes by tests/test_oracle.py): the
    whole-matrix checks, and every row through the per-row check of tests/nnls_cases.py (sign, exact zero
    rows, KKT residual, the row's own distance, the row's zero pattern)."""
    implicit, alpha, reg = LD.MODES[mode]
    ch = _set_chunk(monkeypatch, chunk)
    KP = LD.padded_rank(k)
    user, item, r, B = _data(mode)
    U0 = _src(k, len(B.user_ids), "nonneg")
    c = _nnls_ctx(gpu_lib, k, implicit, reg, alpha)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    tag = f"nnls-{mode}-k{k}-chunk{chunk or 'default'}"
    src = U0
    for side, ptr, col, val in ((1, B.i_ptr, B.i_col, B.i_val), (0, B.u_ptr, B.u_col, B.u_val)):
        c.half(side)
        ids, X = c.factors(side)
        deg = np.diff(ptr)
        paths = np.array([_nnls_path_of(d, KP, ch) for d in deg])
        st = c.stats(side)
        lock = paths == "nnls-lockstep"
        assert st.tolist() == [int(lock.sum()), int(deg[lock].sum()), int((~lock).sum()), int(deg[~lock].sum())]
        if side == 0:
            assert st[0] > 250  # the user half is the lockstep kernel's
        else:
            assert np.sum(paths == "nnls-row") >= 2 and (chunk is None or np.sum(paths == "nnls-split") >= 2)
        X_ref, _ = cbind.solve_rows_nnls(src, O.gram(src), ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
        ref = NC.reference(src, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
        name = "item" if side else "user"
        same = float(np.mean((X == 0) == (X_ref == 0)))
        print(f"RATING_MODES {tag} KP {KP} {name} half: rel {_rel(X, X_ref):.3e}, equal zero pattern {same:.5f}")
        assert np.all(X >= 0)
        # max over the rows of max|x - ref| / max|ref of all rows| is _rel(X, X_ref)
        LD.assert_rows(X, X_ref, ids, deg, paths, 1e-3, f"{name} half [{tag}]", tmp_path, global_scale=True)
        assert same > 0.995
        rows = np.array([NC.nnls_path_of(d, KP, ch) for d in deg])
        assert NC.is_lockstep(rows).tolist() == lock.tolist()
        NC.check_rows(X, ref, ids, deg, rows, f"{name} half per row [{tag}]", tmp_path, NC.KKT_MARGIN)
        src = X


# ---- facade ----------------------------------------------------------------------------------------

def test_facade_explicit_default_fit(gpu_lib):
    """ALS with the facade's (and Spark's) default implicitPrefs = False on the `stars` ladder."""
    from albedo_amd import ALS
    user, item, r, B = _data("stars")
    als = ALS(rank=50, maxIter=2, regParam=0.1, seed=42)
    assert als.getImplicitPrefs() is False
    model = als.fit({"user": user, "item": item, "rating": r})
    su, si = O.spark_side_seeds(42)
    U, V = O.fit(B, rank=50, max_iter=2, reg=0.1, alpha=1.0, implicit=False,
                 init_user=O.spark_initialize(B.user_ids, 50, su), init_item=O.spark_initialize(B.item_ids, 50, si))
    assert np.array_equal(model.user_factors_np()[0], B.user_ids)
    assert _rel(model.user_factors_np()[1], U) < 1e-3
    assert _rel(model.item_factors_np()[1], V) < 1e-3
