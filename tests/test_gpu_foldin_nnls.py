"""als_fold_in with als_fold_params.nonnegative = 1 on the GPU: Spark's NNLS per new row, against the C oracle.

Every expected value is tests/foldin_nnls_cases.py:expected_nnls, oracle.cbind.solve_rows_nnls over the CSR of the
new rows.  The device rows are judged by tests/nnls_cases.py:check_rows under the single path label "fold-nnls":
finite and >= 0, exactly zero where the reference row is, the KKT bound (NC.KKT_MARGIN), the per-row distance
max|x - x_ref| / max|x_ref| < FC.TOL = 1e-4 (the project's bar for every solve path) and zero-pattern differences
only on components below FC.TOL of the row's maximum, at most NC.flip_cap(k) a row.  als_fold_in_stats is held to
the oracle's iteration sum within NC.ITER_BOUND, no row at the limit.

Measured on an MI355X, the worst device row (max|x - x_ref| / max|x_ref|) per rank and case family:

  new items, signed unit-row sources, modes varying / mixed / stars_signed
    rank    1    8    50   64   65   128  129  200  256
    worst   0    0    0    0    0    0    0    0    0      (every fp32 component equal to the oracle's,
                                                            every iteration sum equal to the oracle's)
  new users (700 rows, 52 source rows)      rank 50: 2.8e-7 (mixed)   rank 128: 6.5e-7 (mixed)
  source kinds at regParam 0.5              rank 50: 1.0e-7 (pos)     rank 128: 1.1e-6 (aniso)
  nonneg / pos at regParam 0                rank 50: 6.3e-8           rank 128: 3.1e-7
  tile edges, contract case, singular case  0;  60 rows on 1 / 3 / all workgroups: 0 (rank 128), 1.9e-9 (rank 200)
  users of a nonnegative fit recomputed     rank 50: 2.0e-7           rank 128: 4.5e-7 against the oracle,
                                            7.0e-6 and 8.2e-6 against the context's own fp32 NNLS rows (bar 1e-3)

No zero-pattern difference in any case.  Iteration sums: equal to the oracle's on the new-items ladder and the
edges, within 0.03 % on the new-users cases and within 1.3 % on the source kinds (aniso rank 128: 6890 to the
oracle's 6807, the longest row 559 to 506: the long rows are where the order of a sum decides which stop clause
fires first); `large` and `neg` sources: 0 iterations, all zeros.

The two restatements of Spark's loop part by up to 6.5e-7 on these cases (tests/test_foldin_nnls_cases.py); the
bar stays at 1e-4 and is not to be tightened below 16 x the larger of 6e-8 (one fp32 rounding) and that figure,
1e-5.  The run prints each figure (FOLDIN-NNLS ...).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import foldin_cases as FC
from tests import foldin_nnls_cases as FN
from tests import ladder as LD
from tests import nnls_cases as NC
from tests.test_gpu_audit import Ctx
from tests.test_gpu_foldin import _model_state, fold, fold_rc, timing

pytestmark = pytest.mark.gpu

TOL = FC.TOL


def _fp(reg, alpha, implicit, nonneg=1):
    from albedo_amd import _lib as L
    return L.als_fold_params(float(reg), float(alpha), int(bool(implicit)), int(nonneg))


def _case_fp(c, nonneg=1):
    return _fp(c.reg, c.alpha, c.implicit, nonneg)


def _stats(h):
    from albedo_amd import _lib as L
    return [int(v) for v in L.fold_in_stats(h)]


def _src_ctx(lib, c, mode="varying"):
    """A context on the ladder holding the case's source factors (its own parameters do not matter: fp decides)."""
    user, item, r, B = FC.data(mode)
    ctx = Ctx(lib, c.Y.shape[1], mode)
    ctx.ratings(user, item, r)
    ctx.inject(1 - c.side, c.src_ids, c.Y)
    return ctx


def _check(h, name, got, ref3, tmp_path):
    """check_rows, the stricter zero-pattern rule and the iteration counters; prints the case's figures."""
    ids_e, deg_e, ref = ref3
    ids, deg, X = got
    assert np.array_equal(ids, ids_e), name
    assert np.array_equal(deg, deg_e), name
    k = X.shape[1]
    st = NC.check_rows(X, ref, ids, deg, np.full(ids.size, FN.PATH), name, tmp_path, NC.KKT_MARGIN, tol=TOL)[FN.PATH]
    Xd, Rd = X.astype(np.float64), ref.X.astype(np.float64)
    differ = (Xd == 0) != (Rd == 0)
    rmax = np.max(np.abs(Rd), axis=1, keepdims=True)
    assert (np.maximum(np.abs(Xd), np.abs(Rd))[differ] < (TOL * np.broadcast_to(rmax, Xd.shape))[differ]).all(), name
    sol = _stats(h)
    want = int(ref.it.sum())
    print(f"FOLDIN-NNLS {name}: {ids.size} rows, worst row {st['err']:.3e}, kkt {st['kkt']:.3e} (oracle {st['kkt_ref']:.3e}), "
          f"flips {st['flips']}, iterations {sol[0]} (oracle {want}), most {sol[1]} (oracle {int(ref.it.max(initial=0))})")
    assert abs(sol[0] - want) <= NC.ITER_BOUND * want, (name, sol, want)
    assert sol[1] <= NC.iteration_cap(k)
    assert sol[2] == int((deg > 0).sum())
    assert sol[3] == 0
    return st


def _run(lib, name, tmp_path, mode="varying"):
    c = FN.case(name)
    ctx = _src_ctx(lib, c, mode)
    got = fold(lib, ctx.h, c.side, c.row, c.src, c.r, fp=_case_fp(c))
    _check(ctx.h, name, got, FN.reference(name), tmp_path)
    return ctx, c, got


# ---- 1, 2. ladder parity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", FN.LADDER_RANKS)
@pytest.mark.parametrize("mode", FC.MODES)
def test_ladder_items_match_the_oracle(gpu_lib, monkeypatch, tmp_path, mode, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    ctx, c, got = _run(gpu_lib, f"items-{mode}-k{k}", tmp_path, mode)
    if mode == "mixed":  # the rows without a positive rating: b = 0
        assert (~got[2].any(axis=1)).sum() >= 4


@pytest.mark.parametrize("k", FN.USER_RANKS)
@pytest.mark.parametrize("mode", FC.MODES)
def test_ladder_users_match_the_oracle(gpu_lib, monkeypatch, tmp_path, mode, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    _run(gpu_lib, f"users-{mode}-k{k}", tmp_path, mode)


# ---- 3. source kinds: the zero-iteration exits, the short rows and the long ones ---------------------------

@pytest.mark.parametrize("name", FN.KIND_CASES)
def test_source_kinds_match_the_oracle(gpu_lib, monkeypatch, tmp_path, name):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    ctx, c, got = _run(gpu_lib, name, tmp_path)
    if "-large-" in name or "-neg-" in name:
        assert not got[2].any() and _stats(ctx.h)[:2] == [0, 0]
    if name == "kind-aniso-k128":
        assert _stats(ctx.h)[1] >= 400


# ---- 4. the counters after a Cholesky call -----------------------------------------------------------------

def test_stats_are_zero_after_a_cholesky_call(gpu_lib, monkeypatch, tmp_path):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    ctx, c, got = _run(gpu_lib, "tile-k50", tmp_path)
    assert _stats(ctx.h)[2] == got[0].size
    fold(gpu_lib, ctx.h, c.side, c.row, c.src, c.r, fp=_case_fp(c, 0))
    assert _stats(ctx.h) == [0, 0, 0, 0]
    fold(gpu_lib, ctx.h, c.side, c.row, c.src, c.r)  # fp = NULL: the context's own parameters, Cholesky
    assert _stats(ctx.h) == [0, 0, 0, 0]


# ---- 5. edges ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", FN.KIND_RANKS)
def test_tile_edge_degrees(gpu_lib, monkeypatch, tmp_path, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    ctx, c, got = _run(gpu_lib, f"tile-k{k}", tmp_path)
    assert got[1].tolist() == FC.tile_degrees(k)


def test_input_contract(gpu_lib, monkeypatch, tmp_path):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    ctx, c, got = _run(gpu_lib, "contract-k128", tmp_path)
    ids, deg, X = got
    assert ids[0] == FC.I32_MIN and ids[-1] == FC.I32_MAX and -1 in ids and np.all(np.diff(ids) > 0)
    by_id = dict(zip(ids.tolist(), deg.tolist()))
    assert by_id[77] == 0 and not X[ids == 77].any()          # unknown sources only: degree 0, zeros
    assert by_id[78] == 6                                      # unknown sources mixed in are ignored
    assert [by_id[i] for i in (100, 101, 102)] == [6, 7, 68]  # a pair counts once per copy
    assert _stats(ctx.h)[2] == ids.size - 1                    # the degree-0 row is not solved
    # copies count: without them the rows of the repeated pair move
    r1, s1, v1 = FC.without_duplicates(c.row, c.src, c.r)
    once = fold(gpu_lib, ctx.h, c.side, r1, s1, v1, fp=_case_fp(c))
    ref1 = FN.expected_nnls(c.Y, c.src_ids, r1, s1, v1, reg=c.reg, alpha=c.alpha, implicit=c.implicit)
    _check(ctx.h, "contract case without copies", once, ref1, tmp_path)
    for rid in (100, 101, 102):
        assert not np.array_equal(once[2][once[0] == rid], X[ids == rid])


@pytest.mark.parametrize("implicit", [True, False])
def test_singular_system_is_ok_and_e1(gpu_lib, monkeypatch, tmp_path, implicit):
    """regParam = 0 on a rank-deficient source side: NNLS has no "not positive definite" outcome."""
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    name = f"singular-{'implicit' if implicit else 'explicit'}"
    c = FN.case(name)
    k = c.Y.shape[1]
    item_ids = np.array([1, 2], np.int32)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(k, 3, L.ptr(c.src_ids, C.c_int32), L.ptr(np.ascontiguousarray(c.Y), C.c_float), 2,
                                     L.ptr(item_ids, C.c_int32), L.ptr(np.zeros((2, k), np.float32), C.c_float), -1,
                                     C.byref(h)))
    try:
        rc, ids, deg, X, nr = fold_rc(gpu_lib, h, 1, c.row, c.src, c.r, fp=_case_fp(c))
        assert rc == L.ALS_OK and nr == 1
        want = np.zeros(k, np.float32)
        want[1] = 1.0
        assert np.array_equal(X[0], want) and np.array_equal(FN.reference(name)[2].X[0], want)
        _check(h, name, (ids, deg, X), FN.reference(name), tmp_path)
        assert fold_rc(gpu_lib, h, 1, c.row, c.src, c.r, fp=_case_fp(c, 0))[0] == L.ALS_E_NOT_POSITIVE_DEFINITE
    finally:
        gpu_lib.als_destroy(h)


# ---- 6. determinism ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [128, 200])
def test_bits_do_not_depend_on_the_call_the_order_or_the_grid(gpu_lib, monkeypatch, tmp_path, k):
    """60 rows: with ALBEDO_FOLD_WGS = 1 and 3 every workgroup solves many rows in turn, at rank 200 on one slab of
    global scratch after the other."""
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    ctx, c, got = _run(gpu_lib, f"refill-k{k}", tmp_path)
    fp = _case_fp(c)
    again = fold(gpu_lib, ctx.h, c.side, c.row, c.src, c.r, fp=fp)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    p = np.random.default_rng(3).permutation(c.row.size)
    o = np.lexsort((c.src, c.row))
    for order in (p, o):
        other = fold(gpu_lib, ctx.h, c.side, c.row[order], c.src[order], c.r[order], fp=fp)
        assert all(np.array_equal(a, b) for a, b in zip(got, other))
    sol = _stats(ctx.h)
    for wgs in ("1", "3"):
        monkeypatch.setenv("ALBEDO_FOLD_WGS", wgs)
        other = fold(gpu_lib, ctx.h, c.side, c.row, c.src, c.r, fp=fp)
        assert all(np.array_equal(a, b) for a, b in zip(got, other)), wgs
        assert _stats(ctx.h) == sol


# ---- 7. isolation ----------------------------------------------------------------------------------------------

def _swept(lib, mode, k):
    user, item, r, B = FC.data(mode)
    c = Ctx(lib, k, mode)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids), seed=1))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    c.half(0)
    return c, B


def _grams(lib, c, k):
    from albedo_amd import _lib as L
    out = []
    for side in (0, 1):
        g = np.zeros((k, k), np.float64)
        L.check(lib.als_get_gram(c.h, side, L.ptr(g, C.c_double)))
        out.append(g)
    return out


def test_model_is_untouched_and_the_gram_cache_is_shared(gpu_lib, monkeypatch, tmp_path):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    implicit, alpha, reg = LD.MODES[mode]
    c, B = _swept(gpu_lib, mode, k)
    t = FC.ladder_users(mode)
    nn, ch = _fp(reg, alpha, implicit, 1), _fp(reg, alpha, implicit, 0)
    before = _model_state(gpu_lib, c, k) + _grams(gpu_lib, c, k)
    chol = fold(gpu_lib, c.h, 0, *t, fp=ch)
    assert timing(gpu_lib, c.h)[1] > 0.0  # the first call of either kind forms the Gram
    got = fold(gpu_lib, c.h, 0, *t, fp=nn)
    tm = timing(gpu_lib, c.h)
    assert tm[1] == 0.0 and tm[0] > 0.0 and tm[2] > 0.0 and tm[3] >= tm[0] + tm[2]
    chol2 = fold(gpu_lib, c.h, 0, *t, fp=ch)
    assert timing(gpu_lib, c.h)[1] == 0.0
    assert all(np.array_equal(a, b) for a, b in zip(chol, chol2))  # the same Cholesky bits before and after
    after = _model_state(gpu_lib, c, k) + _grams(gpu_lib, c, k)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    V1 = before[4]
    ref = FN.expected_nnls(V1, B.item_ids, *t, reg=reg, alpha=alpha, implicit=implicit)
    _check(c.h, "fold-in after a sweep", fold(gpu_lib, c.h, 0, *t, fp=nn), ref, tmp_path)
    assert np.array_equal(got[2], fold(gpu_lib, c.h, 0, *t, fp=nn)[2])
    # the other order: NNLS first forms the Gram, the Cholesky call finds it
    c.half(1)
    fold(gpu_lib, c.h, 0, *t, fp=nn)
    assert timing(gpu_lib, c.h)[1] > 0.0
    fold(gpu_lib, c.h, 0, *t, fp=ch)
    assert timing(gpu_lib, c.h)[1] == 0.0
    # and an NNLS fold-in between two halves leaves the fit bit-identical
    c.half(0)
    c2, _ = _swept(gpu_lib, mode, k)
    c2.half(1)
    c2.half(0)
    assert np.array_equal(c2.factors(1), c.factors(1)) and np.array_equal(c2.factors(0), c.factors(0))


# ---- 8. a fitted nonnegative context ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [50, 128])
def test_recomputed_users_of_a_nonnegative_fit(gpu_lib, monkeypatch, tmp_path, k):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode = "varying"
    implicit, alpha, reg = LD.MODES[mode]
    user, item, r, B = FC.data(mode)
    c = Ctx(gpu_lib, k, mode, nonneg=True)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, np.abs(FC.src_factors(k, len(B.user_ids), seed=1)))
    c.inject(1, B.item_ids, np.abs(FC.src_factors(k, len(B.item_ids), seed=0)))
    c.half(1)
    c.half(0)
    U, V = c.factors(0), c.factors(1)
    assert fold_rc(gpu_lib, c.h, 0, user, item, r)[0] == L.ALS_E_UNSUPPORTED  # fp = NULL: ABI version 1
    assert "nonnegative = 1" in gpu_lib.als_last_error().decode()
    got = fold(gpu_lib, c.h, 0, user, item, r, fp=_fp(reg, alpha, implicit, 1))
    assert np.array_equal(got[0], B.user_ids)
    err = LD.row_errors(got[2], U)
    print(f"FOLDIN-NNLS recomputed users k{k}: worst row against the context's own {err.max():.3e}")
    assert err.max() < NC.TOL
    ref = FN.expected_nnls(V, B.item_ids, user, item, r, reg=reg, alpha=alpha, implicit=implicit)
    _check(c.h, f"recomputed users k{k}", got, ref, tmp_path)


# ---- 9. model-only context -------------------------------------------------------------------------------------

def test_model_only_context_gives_the_same_bits(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    name = f"items-{mode}-k{k}"
    ctx, c, got = _run(gpu_lib, name, tmp_path, mode)
    B = FC.data(mode)[3]
    U = np.ascontiguousarray(c.Y)
    V = FC.src_factors(k, len(B.item_ids), seed=0)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(k, len(B.user_ids), L.ptr(B.user_ids, C.c_int32), L.ptr(U, C.c_float),
                                     len(B.item_ids), L.ptr(B.item_ids, C.c_int32), L.ptr(V, C.c_float), -1, C.byref(h)))
    try:
        other = fold(gpu_lib, h, 1, c.row, c.src, c.r, fp=_case_fp(c))
        assert all(np.array_equal(a, b) for a, b in zip(got, other))
        assert _stats(h) == _stats(ctx.h)
        assert fold_rc(gpu_lib, h, 1, c.row, c.src, c.r)[0] == L.ALS_E_INVALID_ARGUMENT  # fp = NULL
    finally:
        gpu_lib.als_destroy(h)


# ---- 10. Python --------------------------------------------------------------------------------------------------

def test_facade_folds_in_by_nnls(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import ALS, ALSModel
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    user, item, r, B = FC.data("varying")
    k, reg, alpha = 16, 0.5, 10.0
    model = ALS(rank=k, maxIter=1, regParam=reg, alpha=alpha, implicitPrefs=True, nonnegative=True, seed=3, userCol="u",
                itemCol="i", ratingCol="r").fit({"u": user, "i": item, "r": r})
    new = np.unique(user)[:40]
    m = np.isin(user, new)
    nu, ni, nr = (user[m].astype(np.int64) + FC.ID_SHIFT).astype(np.int32), item[m], r[m]
    ds = {"u": nu, "i": ni, "r": nr}
    iid, V = model.item_factors_np()
    kw = dict(reg=reg, alpha=alpha, implicit=True)
    ref = FN.expected_nnls(V, iid, nu, ni, nr, **kw)
    frame = model.foldIn(ds)  # the model's own nonnegative = True
    st = model.fold_in_stats()
    assert st["rows"] == int((ref[1] > 0).sum()) > 0 and st["rows_at_limit"] == 0 and st["iterations"] >= st["max_iterations"] > 0
    X = np.stack(frame["features"].to_numpy())
    ids2, deg2, X2 = model.fold_in_np(nu, ni, nr)
    assert np.array_equal(frame["id"].to_numpy(), ids2) and np.array_equal(X2, X)
    _check(model._h, "facade foldIn", (ids2, deg2, X2), ref, tmp_path)
    # nonnegative=False on the same model: the Cholesky rows
    ids_c, deg_c, X_c = FC.expected(V, iid, nu, ni, nr, **kw)
    Xc = np.stack(model.foldIn(ds, nonnegative=False)["features"].to_numpy())
    assert LD.row_errors(Xc, X_c).max() < TOL and not np.array_equal(Xc, X)
    assert model.fold_in_stats() == dict(iterations=0, max_iterations=0, rows=0, rows_at_limit=0)
    # the lists: the oracle's top-k over (the folded factors as returned, the model's item factors)
    num = 10
    recs = model.recommendForNewUsers(ds, num, nonnegative=True)
    assert np.array_equal(recs["u"].to_numpy(), ids2)
    want_ids, want_sc = O.recommend_for_all(ids2, X, iid, V, num)
    for j, lst in enumerate(recs["recommendations"]):
        assert [i for i, _ in lst] == want_ids[j].tolist()
        assert np.array_equal(np.array([s for _, s in lst], np.float32).view(np.uint32), want_sc[j].view(np.uint32))
    # a loaded model does not know how it was fitted: Cholesky unless told
    path = str(tmp_path / "model")
    model.save(path)
    loaded = ALSModel.load(path).setRatingCol("r")
    p3 = dict(regParam=reg, alpha=alpha, implicitPrefs=True)
    assert np.array_equal(np.stack(loaded.foldIn(ds, **p3)["features"].to_numpy()), Xc)
    assert np.array_equal(np.stack(loaded.foldIn(ds, nonnegative=True, **p3)["features"].to_numpy()), X)
    assert loaded.fold_in_stats()["rows"] == st["rows"]
