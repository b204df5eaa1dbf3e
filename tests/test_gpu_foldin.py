"""als_fold_in on the GPU: factors of rows the model has not seen, against the fp64 oracle.

Every expected value is tests/foldin_cases.py:expected, the oracle's half-sweep over the CSR of the new
rows.  The bar is the project's for every solve path, max|x - x64| / max|x64| < 1e-4 per row
(tests/test_gpu_rating_modes.py), rows whose reference is zero exactly zero.  The fold-in solves in fp64
and rounds once, so it sits at fp32 rounding or below.  Measured on an MI355X, new items from ~700 unit-row
user factors, over the modes varying / mixed / stars_signed, the worst row per rank:

  rank    1    50   64   65   128  129  200  256
  worst   0    0    0    0    0    0    0    0      (every fp32 component equal to the oracle's)

and the same in the new-users direction (52 source rows, ranks 50 and 128), on the tile-edge rows and on the
contract case; the audit of 700 recomputed users measures a worst eta of 6.2e-9 (rank 50) and 4.5e-9 (rank
128).  Two fp64 solves that differ in the order of their sums round to different fp32 values only when the
result lies within ~1e-16 relative of a rounding boundary, so a differing last bit (6e-8) can appear on other
data; the assertion stays at 1e-4 and is not to be tightened below 16 x 6e-8 = 1e-6.  The run prints each
figure (FOLDIN ... worst row ...).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import foldin_cases as FC
from tests import ladder as LD
from tests.test_gpu_audit import Ctx

pytestmark = pytest.mark.gpu

TOL = FC.TOL
AUDIT_TOL = 2e-6  # include/albedo_als.h: the recommended working tolerance of als_audit_rows


def _fp(reg, alpha, implicit):
    from albedo_amd import _lib as L
    return L.als_fold_params(float(reg), float(alpha), int(bool(implicit)), 0)


def fold_rc(lib, h, side, row, src, r, fp=None, cap=None, n=None):
    """The raw call: (rc, ids, degrees, factors, n_rows); the arrays are cut to n_rows when they were filled."""
    from albedo_amd import _lib as L
    row, src = np.ascontiguousarray(row, np.int32), np.ascontiguousarray(src, np.int32)
    r = np.ascontiguousarray(r, np.float32)
    n = row.size if n is None else n
    cap = max(row.size, 1) if cap is None else cap
    k = lib.als_rank(h)
    ids = np.full(max(cap, 1), 123456789, np.int32)
    deg = np.full(max(cap, 1), -7, np.int64)
    X = np.full((max(cap, 1), k), np.nan, np.float32)
    nr = C.c_int64(-1)
    rc = lib.als_fold_in(h, side, C.byref(fp) if fp is not None else None, n, L.ptr(row, C.c_int32),
                         L.ptr(src, C.c_int32), L.ptr(r, C.c_float), cap, C.byref(nr), L.ptr(ids, C.c_int32),
                         L.ptr(deg, C.c_int64), L.ptr(X, C.c_float))
    m = nr.value if 0 <= nr.value <= cap else 0
    return rc, ids[:m], deg[:m], X[:m], nr.value


def fold(lib, h, side, row, src, r, fp=None):
    from albedo_amd import _lib as L
    rc, ids, deg, X, nr = fold_rc(lib, h, side, row, src, r, fp)
    L.check(rc)
    assert nr == ids.size
    return ids, deg, X


def timing(lib, h):
    from albedo_amd import _lib as L
    return L.fold_in_timing(h)


def _src_ctx(lib, mode, k, side):
    """A context on the ladder holding unit-row factors on the source side of a fold-in of `side`."""
    user, item, r, B = FC.data(mode)
    c = Ctx(lib, k, mode)
    c.ratings(user, item, r)
    src_ids = B.user_ids if side == 1 else B.item_ids
    c.inject(1 - side, src_ids, FC.src_factors(k, len(src_ids), seed=side))
    return c, B, src_ids


def _check(got, want, tol, what, tmp_path):
    (ids, deg, X), (ids_e, deg_e, X_e) = got, want
    assert np.array_equal(ids, ids_e), what
    assert np.array_equal(deg, deg_e), what
    worst = LD.assert_rows(X, X_e, ids, deg, np.full(ids.size, "fold"), tol, what, tmp_path)
    print(f"FOLDIN {what}: {ids.size} rows, worst row {worst:.3e}")
    return worst


# ---- 1. ladder parity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", FC.RANKS)
@pytest.mark.parametrize("mode", FC.MODES)
def test_ladder_items_match_the_oracle(gpu_lib, monkeypatch, tmp_path, mode, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, B, src_ids = _src_ctx(gpu_lib, mode, k, 1)
    got = fold(gpu_lib, c.h, 1, *FC.ladder_items(mode))
    _check(got, FC.ladder_expected(mode, k, 1), TOL, f"items {mode} k{k}", tmp_path)
    if mode == "mixed":
        assert (~got[2].any(axis=1)).sum() >= 4


@pytest.mark.parametrize("k", [50, 128])
@pytest.mark.parametrize("mode", FC.MODES)
def test_ladder_users_match_the_oracle(gpu_lib, monkeypatch, tmp_path, mode, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, B, src_ids = _src_ctx(gpu_lib, mode, k, 0)
    got = fold(gpu_lib, c.h, 0, *FC.ladder_users(mode))
    _check(got, FC.ladder_expected(mode, k, 0), TOL, f"users {mode} k{k}", tmp_path)


# ---- 2. tile and size edges ---------------------------------------------------------------------------

def _edge_ctx(lib, k=128):
    c, B, src_ids = _src_ctx(lib, "varying", k, 1)
    return c, src_ids, FC.src_factors(k, len(src_ids), seed=1), dict(reg=0.5, alpha=10.0, implicit=True)


def test_tile_edge_degrees(gpu_lib, monkeypatch, tmp_path):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib)
    t = FC.degree_rows(FC.tile_degrees(128), src_ids)
    got = fold(gpu_lib, c.h, 1, *t)
    assert got[1].tolist() == FC.tile_degrees(128)
    _check(got, FC.expected(Y, src_ids, *t, **kw), TOL, "tile edges k128", tmp_path)


def test_every_workgroup_refills(gpu_lib, monkeypatch, tmp_path):
    monkeypatch.setenv("ALBEDO_FOLD_WGS", "3")
    c, src_ids, Y, kw = _edge_ctx(gpu_lib)
    t = FC.degree_rows([5, 40, 33, 1, 129, 64, 2, 70, 31, 12], src_ids, seed=6)
    _check(fold(gpu_lib, c.h, 1, *t), FC.expected(Y, src_ids, *t, **kw), TOL, "10 rows on 3 workgroups", tmp_path)


def test_single_row_and_no_rows(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib)
    t = FC.degree_rows([17], src_ids, seed=8)
    _check(fold(gpu_lib, c.h, 1, *t), FC.expected(Y, src_ids, *t, **kw), TOL, "one row", tmp_path)
    e = np.zeros(0, np.int32)
    rc, ids, deg, X, nr = fold_rc(gpu_lib, c.h, 1, e, e, np.zeros(0, np.float32))
    assert rc == L.ALS_OK and nr == 0
    nr = C.c_int64(-1)  # null arrays are fine with n = 0
    assert gpu_lib.als_fold_in(c.h, 1, None, 0, None, None, None, 0, C.byref(nr), None, None, None) == L.ALS_OK
    assert nr.value == 0


# ---- 3. input contract --------------------------------------------------------------------------------

def test_input_contract(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    c, src_ids, Y, kw = _edge_ctx(gpu_lib)
    row, src, r = FC.contract_case(src_ids)
    want = FC.expected(Y, src_ids, row, src, r, **kw)
    got = fold(gpu_lib, c.h, 1, row, src, r)
    _check(got, want, TOL, "contract case", tmp_path)
    ids, deg, X = got
    assert ids[0] == FC.I32_MIN and ids[-1] == FC.I32_MAX and -1 in ids and np.all(np.diff(ids) > 0)
    by_id = dict(zip(ids.tolist(), deg.tolist()))
    assert by_id[77] == 0 and not X[ids == 77].any()          # unknown sources only: degree 0, zeros
    assert by_id[78] == 6                                      # unknown sources mixed in are ignored
    assert [by_id[i] for i in (100, 101, 102)] == [6, 7, 68]  # a pair counts once per copy
    # two calls: identical bits
    again = fold(gpu_lib, c.h, 1, row, src, r)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    # without copies the order of the input does not matter
    r1, s1, v1 = FC.without_duplicates(row, src, r)
    o = np.lexsort((s1, r1))
    p = np.random.default_rng(3).permutation(r1.size)
    a = fold(gpu_lib, c.h, 1, r1[o], s1[o], v1[o])
    b = fold(gpu_lib, c.h, 1, r1[p], s1[p], v1[p])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _check(a, FC.expected(Y, src_ids, r1, s1, v1, **kw), TOL, "contract case without copies", tmp_path)
    # a cap below the row count fills nothing and reports the count
    rc, i2, d2, X2, nr = fold_rc(gpu_lib, c.h, 1, row, src, r, cap=ids.size - 1)
    assert rc == L.ALS_OK and nr == ids.size and i2.size == 0


# ---- 4. recompute equals solve ------------------------------------------------------------------------

@pytest.mark.parametrize("k", [50, 128])
def test_recomputed_users_pass_the_audit(gpu_lib, monkeypatch, tmp_path, k):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    monkeypatch.delenv("ALBEDO_AUDIT_CHUNK", raising=False)
    mode = "varying"
    implicit, alpha, reg = LD.MODES[mode]
    user, item, r, B = FC.data(mode)
    c = Ctx(gpu_lib, k, mode)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids), seed=1))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    V = c.factors(1)
    ids, deg, X = fold(gpu_lib, c.h, 0, user, item, r)  # ids the model has: recomputed, nothing stored
    _check((ids, deg, X), FC.expected(V, B.item_ids, user, item, r, reg=reg, alpha=alpha, implicit=implicit), TOL,
           f"recomputed users k{k}", tmp_path)
    assert np.array_equal(ids, B.user_ids)
    c.inject(0, ids, X)
    eta, a = c.audit(0, AUDIT_TOL)
    print(f"FOLDIN audit of the recomputed users k{k}: worst eta {eta.max():.3e}")
    assert a.rows_over == 0 and a.non_finite == 0 and eta.max() <= AUDIT_TOL


# ---- 5. model untouched, cache honest -----------------------------------------------------------------

def _model_state(lib, c, k):
    from albedo_amd import _lib as L
    out = []
    for side in (0, 1):
        out.append(c.factors(side))
        b = np.zeros((k, k), np.float64)
        L.check(lib.als_get_basis(c.h, side, L.ptr(b, C.c_double)))
        t = np.zeros(L.ALS_T_COUNT, np.float64)
        L.check(lib.als_last_timings(c.h, side, L.ptr(t, C.c_double), L.ALS_T_COUNT))
        s = np.zeros(4, np.int64)
        L.check(lib.als_path_stats(c.h, side, L.ptr(s, C.c_int64)))
        out += [b, t, s]
    return out


def test_model_is_untouched_and_the_gram_cache_follows_the_factors(gpu_lib, monkeypatch, tmp_path):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    implicit, alpha, reg = LD.MODES[mode]
    kw = dict(reg=reg, alpha=alpha, implicit=implicit)
    user, item, r, B = FC.data(mode)
    c = Ctx(gpu_lib, k, mode)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids), seed=1))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    c.half(0)
    t = FC.ladder_users(mode)
    before = _model_state(gpu_lib, c, k)
    got = fold(gpu_lib, c.h, 0, *t)
    assert timing(gpu_lib, c.h)[1] > 0.0  # the first call forms the Gram
    again = fold(gpu_lib, c.h, 0, *t)
    tm = timing(gpu_lib, c.h)
    assert tm[1] == 0.0 and tm[0] > 0.0 and tm[2] > 0.0 and tm[3] >= tm[0] + tm[2]
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    after = _model_state(gpu_lib, c, k)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    V1 = before[4]
    _check(got, FC.expected(V1, B.item_ids, *t, **kw), TOL, "fold-in after a sweep", tmp_path)
    # the item factors move (their source, the users, moved in the half above): a stale Gram fails here
    c.half(1)
    V2 = c.factors(1)
    assert not np.allclose(V1, V2, rtol=1e-3, atol=0)
    got2 = fold(gpu_lib, c.h, 0, *t)
    assert timing(gpu_lib, c.h)[1] > 0.0
    _check(got2, FC.expected(V2, B.item_ids, *t, **kw), TOL, "fold-in after the next half", tmp_path)
    # and a fold-in between two halves leaves the fit bit-identical
    c2 = Ctx(gpu_lib, k, mode)
    c2.ratings(user, item, r)
    c2.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids), seed=1))
    c2.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    for side in (1, 0, 1):
        c2.half(side)
    assert np.array_equal(c2.factors(1), V2) and np.array_equal(c2.factors(0), c.factors(0))


# ---- 6. model-only context ----------------------------------------------------------------------------

def test_model_only_context_needs_its_parameters(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    implicit, alpha, reg = LD.MODES[mode]
    B = FC.data(mode)[3]
    U = FC.src_factors(k, len(B.user_ids), seed=1)
    V = FC.src_factors(k, len(B.item_ids), seed=0)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(k, len(B.user_ids), L.ptr(B.user_ids, C.c_int32), L.ptr(U, C.c_float),
                                     len(B.item_ids), L.ptr(B.item_ids, C.c_int32), L.ptr(V, C.c_float), -1, C.byref(h)))
    try:
        t = FC.ladder_items(mode)
        got = fold(gpu_lib, h, 1, *t, fp=_fp(reg, alpha, implicit))
        _check(got, FC.ladder_expected(mode, k, 1), TOL, "model-only context", tmp_path)
        assert fold_rc(gpu_lib, h, 1, *t)[0] == L.ALS_E_INVALID_ARGUMENT  # fp = NULL
        fold(gpu_lib, h, 1, *t, fp=_fp(reg, alpha, implicit))
        assert timing(gpu_lib, h)[1] == 0.0  # the Gram is formed once per context
    finally:
        gpu_lib.als_destroy(h)


# ---- 7. errors ----------------------------------------------------------------------------------------

def test_error_codes(gpu_lib, monkeypatch):
    from albedo_amd import _lib as L
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 8
    user, item, r, B = FC.data(mode)
    t = FC.degree_rows([3, 4], B.user_ids)
    nn = Ctx(gpu_lib, k, mode, nonneg=True)
    nn.ratings(user, item, r)
    nn.inject(0, B.user_ids, np.abs(FC.src_factors(k, len(B.user_ids))))
    assert fold_rc(gpu_lib, nn.h, 1, *t)[0] == L.ALS_E_UNSUPPORTED
    c = Ctx(gpu_lib, k, mode)
    c.ratings(user, item, r)
    assert fold_rc(gpu_lib, c.h, 1, *t)[0] == L.ALS_E_STATE  # no factors
    c.inject(0, B.user_ids, FC.src_factors(k, len(B.user_ids)))
    assert fold_rc(gpu_lib, c.h, 0, *t)[0] == L.ALS_E_STATE  # the item side still has none
    assert fold_rc(gpu_lib, c.h, 1, *t)[0] == L.ALS_OK
    assert fold_rc(gpu_lib, c.h, 2, *t)[0] == L.ALS_E_INVALID_ARGUMENT
    assert fold_rc(gpu_lib, c.h, -1, *t)[0] == L.ALS_E_INVALID_ARGUMENT
    assert fold_rc(gpu_lib, c.h, 1, *t, n=-1)[0] == L.ALS_E_INVALID_ARGUMENT
    assert fold_rc(gpu_lib, c.h, 1, *t, fp=_fp(float("nan"), 1.0, True))[0] == L.ALS_E_INVALID_ARGUMENT
    assert fold_rc(gpu_lib, c.h, 1, *t, fp=_fp(-0.5, 1.0, True))[0] == L.ALS_E_INVALID_ARGUMENT
    assert fold_rc(gpu_lib, c.h, 1, *t, fp=_fp(0.5, -1.0, True))[0] == L.ALS_E_INVALID_ARGUMENT
    row, src, rr = (np.ascontiguousarray(a) for a in t)
    nr = C.c_int64(0)
    assert gpu_lib.als_fold_in(c.h, 1, None, row.size, None, L.ptr(src, C.c_int32), L.ptr(rr, C.c_float), row.size,
                               C.byref(nr), None, None, None) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_fold_in(c.h, 1, None, row.size, L.ptr(row, C.c_int32), L.ptr(src, C.c_int32),
                               L.ptr(rr, C.c_float), row.size, None, None, None, None) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_fold_in_timing(c.h, None) == L.ALS_E_INVALID_ARGUMENT


@pytest.mark.parametrize("implicit", [True, False])
def test_singular_system_is_an_error_return(gpu_lib, monkeypatch, implicit):
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
        rc = fold_rc(gpu_lib, h, 1, rows, srcs, rs, fp=_fp(0.0, 1.0, implicit))[0]
        assert rc == L.ALS_E_NOT_POSITIVE_DEFINITE
        msg = gpu_lib.als_last_error().decode()
        assert str(int(row[0])) in msg and str(int(row[0]) + 1) not in msg
        with pytest.raises(L.IllegalArgumentException):
            L.check(rc)
        want = FC.expected(Y, src_ids, row, src, r, reg=0.5, alpha=1.0, implicit=implicit)
        ids, deg, X = fold(gpu_lib, h, 1, row, src, r, fp=_fp(0.5, 1.0, implicit))  # the context still serves
        assert np.array_equal(ids, want[0]) and LD.row_errors(X, want[2]).max() < TOL
    finally:
        gpu_lib.als_destroy(h)


def test_fork_folds_in_like_its_parent(gpu_lib, monkeypatch):
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    mode, k = "varying", 50
    c, B, src_ids = _src_ctx(gpu_lib, mode, k, 1)
    f = Ctx(gpu_lib, k, mode, parent=c)
    f.inject(0, src_ids, FC.src_factors(k, len(src_ids), seed=1))
    t = FC.ladder_items(mode)
    a, b = fold(gpu_lib, c.h, 1, *t), fold(gpu_lib, f.h, 1, *t)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    del f


# ---- 8. Python ----------------------------------------------------------------------------------------

def test_facade_fold_in_and_recommend_for_new_users(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import ALS, ALSModel
    monkeypatch.delenv("ALBEDO_FOLD_WGS", raising=False)
    user, item, r, B = FC.data("varying")
    k, reg, alpha = 16, 0.5, 10.0
    model = ALS(rank=k, maxIter=1, regParam=reg, alpha=alpha, implicitPrefs=True, seed=3, userCol="u", itemCol="i",
                ratingCol="r").fit({"u": user, "i": item, "r": r})
    new = np.unique(user)[:40]
    m = np.isin(user, new)
    nu, ni, nr = (user[m].astype(np.int64) + FC.ID_SHIFT).astype(np.int32), item[m], r[m]
    ds = {"u": nu, "i": ni, "r": nr}
    iid, V = model.item_factors_np()
    ids_e, deg_e, X_e = FC.expected(V, iid, nu, ni, nr, reg=reg, alpha=alpha, implicit=True)
    frame = model.foldIn(ds)
    assert list(frame.columns) == list(model.userFactors.columns) == ["id", "features"]
    assert np.array_equal(frame["id"].to_numpy(), ids_e) and len(frame["features"][0]) == k
    X = np.stack(frame["features"].to_numpy())
    assert X.dtype == np.float32 and LD.row_errors(X, X_e).max() < TOL
    ids2, deg2, X2 = model.fold_in_np(nu, ni, nr)
    assert np.array_equal(ids2, ids_e) and np.array_equal(deg2, deg_e) and np.array_equal(X2, X)
    items_frame = model.foldIn({"u": user[:50], "i": (item[:50].astype(np.int64) + 5).astype(np.int32), "r": r[:50]},
                               side="item")
    assert list(items_frame.columns) == ["id", "features"] and len(items_frame) == np.unique(item[:50]).size
    # the lists: the oracle's top-k over (the folded factors as returned, the model's item factors)
    num = 7
    recs = model.recommendForNewUsers(ds, num)
    assert list(recs.columns) == list(model.recommendForUserSubset({"u": user[:5]}, num).columns) == ["u", "recommendations"]
    assert np.array_equal(recs["u"].to_numpy(), ids_e)
    want_ids, want_sc = O.recommend_for_all(ids_e, X, iid, V, num)
    for j, lst in enumerate(recs["recommendations"]):
        assert [i for i, _ in lst] == want_ids[j].tolist()
        assert np.array_equal(np.array([s for _, s in lst], np.float32).view(np.uint32), want_sc[j].view(np.uint32))
    # a loaded model carries no regParam
    path = str(tmp_path / "model")
    model.save(path)
    loaded = ALSModel.load(path).setRatingCol("r")  # the saved model carries userCol and itemCol only
    with pytest.raises(ValueError, match="regParam"):
        loaded.foldIn(ds)
    with pytest.raises(ValueError, match="alpha"):
        loaded.foldIn(ds, regParam=reg, implicitPrefs=True)
    X3 = np.stack(loaded.foldIn(ds, regParam=reg, alpha=alpha, implicitPrefs=True)["features"].to_numpy())
    assert np.array_equal(X3, X)
