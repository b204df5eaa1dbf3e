"""GPU parity of the front end of every implicit half-sweep at rank, row-count and spectrum edges:
the source side's Gram (launch_gram), its eigenbasis (eig.hip: warm-started parallel Jacobi), the
rotation into that basis and the column scales derived from the eigenvalues.  The per-row solves take
G = diag(Λ) in that basis and B_t = B_s·P orthogonal for granted, so a front end that is slightly
wrong makes every row of the sweep wrong at once.

Inputs come from tests/spectrum_cases.py; what they promise is asserted on the CPU in
tests/test_oracle.py (ranks, multiplicities, cluster widths, exact zeros; every half-sweep case is
solved by a plain fp32 Cholesky within 2e-5 of fp64, a fifth of the tolerance used here, which is why
the generated cases run at alpha = 2: see spectrum_cases.ALPHA).

The eigensolver alone (als_device_eigh) against LAPACK in fp64, the bounds of
test_gpu_parity.test_device_eigensolver: max|VᵀV - I| < 1e-12, ‖VᵀGV - diag(w)‖_F < 1e-12 ‖G‖_F,
sorted w within 1e-12 ‖G‖_F of eigvalsh.  Sweep counts are compared with those of the numpy
restatement tools/jacobi_ref.py on the same matrix (at most 2 more: its 2 x 2 products round
differently in the last bits) and with the budget.

The front end inside a half-sweep against the fp64 oracle: als_get_gram within 1e-6 of O.gram
(relative to max|G|), destination rows within 1e-4 of O.half_sweep, als_get_basis orthogonal to 1e-13,
B_tᵀ G B_t diagonal to 1e-12 ‖G‖_F, the source factors untouched.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import spark_als as O
from tests import ladder as LD
from tests import spectrum_cases as SC
from tests.test_gpu_parity import Ctx, _rel
from tests.test_gpu_rating_modes import _check_paths, _data
from tools import jacobi_ref as JR

pytestmark = pytest.mark.gpu

TOL_ROWS = 1e-4
TOL_GRAM = 1e-6
TOL_EIG = 1e-12
TOL_BASIS = 1e-13
ALS_OK, ALS_E_NOT_POSITIVE_DEFINITE = 0, 2


# ---- the eigensolver alone ---------------------------------------------------------------------

def _eigh(lib, G, W0=None):
    """als_device_eigh on G (warm start W0 or the identity) -> (status, w, V, sweeps)."""
    from albedo_amd import _lib as L
    k = G.shape[0]
    G = np.ascontiguousarray(G, np.float64)
    w = np.full(k, np.nan)
    V = np.full((k, k), np.nan)
    sw = np.full(1, -7, np.int32)
    W0 = None if W0 is None else np.ascontiguousarray(W0, np.float64)
    rc = lib.als_device_eigh(0, k, L.ptr(G, C.c_double), None if W0 is None else L.ptr(W0, C.c_double),
                             L.ptr(w, C.c_double), L.ptr(V, C.c_double), L.ptr(sw, C.c_int32))
    return rc, w, V, int(sw[0])


def _below(x, bound):
    """x < bound, and for the zero matrix (bound 0) x == 0."""
    return x < bound or (bound == 0.0 and x == 0.0)


def _check_eig(G, w, V, what):
    """The three bounds of test_device_eigensolver; returns (orthogonality, residual / ‖G‖, eigenvalue
    error / ‖G‖) for the record."""
    k = G.shape[0]
    gn = float(np.linalg.norm(G))
    assert np.isfinite(w).all() and np.isfinite(V).all(), what
    orth = float(np.abs(V.T @ V - np.eye(k)).max())
    res = float(np.linalg.norm(V.T @ G @ V - np.diag(w)))
    dw = float(np.abs(np.sort(w) - np.linalg.eigvalsh(G)).max())
    assert orth < TOL_EIG, (what, orth)
    assert _below(res, TOL_EIG * gn), (what, res, gn)
    assert _below(dw, TOL_EIG * gn), (what, dw, gn)
    s = gn if gn > 0 else 1.0
    return orth, res / s, dw / s


@functools.lru_cache(maxsize=None)
def _cold(lib, kind, k):
    G = SC.spectrum(kind, k)
    rc, w, V, sw = _eigh(lib, G)
    for a in (w, V):
        a.setflags(write=False)
    return rc, w, V, sw


EIG_CASES = [(kind, k) for k in SC.EIG_KS for kind in SC.spectrum_kinds(k)]


@pytest.mark.parametrize("kind,k", EIG_CASES, ids=[f"{kind}-k{k}" for kind, k in EIG_CASES])
def test_eigensolver_spectra(gpu_lib, kind, k):
    """Every spectrum from the identity warm start, on both Jacobi kernels (k <= 128 in LDS, above in
    global memory), at even and odd k (the round-robin's dummy player) and at k = 1, 2, 3."""
    G = SC.spectrum(kind, k)
    rc, w, V, sw = _cold(gpu_lib, kind, k)
    assert rc == ALS_OK, (rc, gpu_lib.als_last_error().decode())
    orth, res, dw = _check_eig(G, w, V, f"{kind} k={k}")
    ref = SC.reference_sweeps(kind, k)
    print(f"EIG_SWEEPS {kind} k {k}: device {sw} restatement {ref} | orth {orth:.2e} resid {res:.2e} eigenvalues {dw:.2e}")
    assert ref is not None
    assert 0 <= sw <= JR.JAC_MAX_SWEEPS
    assert sw <= ref + 2, (sw, ref)
    if kind in ("zero", "diag", "identity"):
        assert sw == 0
        assert np.array_equal(w.view(np.uint64), np.diag(G).copy().view(np.uint64))
    if kind == "identity":
        assert np.array_equal(V.view(np.uint64), np.eye(k).view(np.uint64))


@pytest.mark.parametrize("k", [50, 65, 129, 256])
@pytest.mark.parametrize("kind", ["graded", "pairs", "deficient"])
def test_eigensolver_power_of_two_scaling(gpu_lib, kind, k):
    """Every quantity of the kernels is scale-free: G·2^100 and G·2^-100 take the sweeps of G, return
    its V bit for bit and its w scaled exactly.  A difference means an absolute threshold crept in."""
    G = SC.spectrum(kind, k)
    rc, w, V, sw = _cold(gpu_lib, kind, k)
    assert rc == ALS_OK
    for e in (100, -100):
        s = 2.0 ** e
        rc2, w2, V2, sw2 = _eigh(gpu_lib, G * s)
        assert rc2 == ALS_OK, (e, gpu_lib.als_last_error().decode())
        assert sw2 == sw, (e, sw2, sw)
        assert np.array_equal(V2.view(np.uint64), V.view(np.uint64)), e
        assert np.array_equal(w2.view(np.uint64), (w * s).view(np.uint64)), e
        _check_eig(G * s, w2, V2, f"{kind} k={k} 2^{e}")


@pytest.mark.parametrize("start", SC.WARM_STARTS)
@pytest.mark.parametrize("k", [50, 65, 128, 200])
@pytest.mark.parametrize("kind", ["graded", "pairs"])
def test_eigensolver_warm_starts(gpu_lib, kind, k, start):
    """Warm starts that a fit does not produce: the exact eigenvectors (at most 1 sweep), their columns
    permuted or one of them negated (determinant -1; no more sweeps than from the identity), and a start
    1e-8 off orthogonal (the Newton-Schulz step in front of the Jacobi has to repair it)."""
    G = SC.spectrum(kind, k)
    cold = _cold(gpu_lib, kind, k)
    assert cold[0] == ALS_OK
    W0 = SC.warm_starts(G)[start]
    rc, w, V, sw = _eigh(gpu_lib, G, W0)
    assert rc == ALS_OK, gpu_lib.als_last_error().decode()
    orth, res, dw = _check_eig(G, w, V, f"{kind} k={k} {start}")
    print(f"EIG_WARM {kind} k {k} {start}: sweeps {sw} (cold {cold[3]}) | orth {orth:.2e} resid {res:.2e} eigenvalues {dw:.2e}")
    if start == "exact":
        assert sw <= 1
    if start in ("permuted", "reflected"):
        assert sw <= cold[3]


@pytest.mark.parametrize("k", [50, 200])
@pytest.mark.parametrize("what", ["nan", "inf"])
def test_eigensolver_refuses_non_finite(gpu_lib, what, k):
    """One NaN or one +Inf in the matrix: a non-zero status with a message, as als_host_eigh gives
    (test_host_eigh_refuses_a_non_finite_matrix), and at once.  `!(off > tol·dia)` is true for a NaN
    mass, so both Jacobi kernels used to report convergence in 0 sweeps with ALS_OK."""
    G = np.array(SC.spectrum("sparkinit", k))
    if what == "nan":
        G[1, k - 1] = G[k - 1, 1] = np.nan
    else:
        G[k // 2, k // 2] = np.inf
    rc, w, V, sw = _eigh(gpu_lib, G)
    msg = gpu_lib.als_last_error().decode()
    assert rc == ALS_E_NOT_POSITIVE_DEFINITE, (rc, sw)
    assert "not finite" in msg and "did not converge" in msg, msg
    assert sw == 0  # it ended at the first check, it did not spend the budget
    rc, w, V, sw = _eigh(gpu_lib, np.array(SC.spectrum("sparkinit", k)))  # and the next call is unharmed
    assert rc == ALS_OK and sw > 0


# ---- the front end inside a half-sweep ------------------------------------------------------------

def _gram(c, side):
    k = c.rank
    G = np.empty((k, k))
    c.L.check(c.lib.als_get_gram(c.h, side, c.L.ptr(G, C.c_double)))
    return G


def _basis(c, side):
    k = c.rank
    B = np.empty((k, k))
    c.L.check(c.lib.als_get_basis(c.h, side, c.L.ptr(B, C.c_double)))
    return B


def _half(c, dst, Ysrc, ptr, col, val, tag, tmp_path, reg=SC.REG, alpha=SC.ALPHA, rows=True):
    """One half-sweep towards side `dst` from the source factors Ysrc (what was injected, or what the
    device returned for that side), then the checks of the module docstring.  Returns the new factors."""
    src = 1 - dst
    k = c.rank
    KP = LD.padded_rank(k)
    c.half(dst)
    G = _gram(c, src)
    G_ref = O.gram(Ysrc)
    gerr = _rel(G, G_ref)
    ids, X = c.factors(dst)
    deg = np.diff(ptr)
    light = 0 if getattr(c, "all_heavy", False) else c.light
    paths = np.array([LD.path_of(d, KP, light, LD.split_chunk()) for d in deg])
    B = _basis(c, dst)
    orth = float(np.abs(B.T @ B - np.eye(k)).max())
    D = B.T @ G @ B
    off = float(np.linalg.norm(D - np.diag(np.diag(D))))
    gn = float(np.linalg.norm(G))
    rerr = -1.0
    if rows:
        X_ref = O.half_sweep(Ysrc, ptr, col, val, reg=reg, alpha=alpha)
        rerr = float(LD.row_errors(X, X_ref).max())
    print(f"FRONT_END {tag} KP {KP} side {dst}: gram {gerr:.2e} rows {rerr:.2e} basis {orth:.2e} "
          f"offdiag {off / (gn if gn > 0 else 1.0):.2e} sweeps {_sweeps(c, dst)}")
    assert gerr < TOL_GRAM, (tag, gerr)
    if rows:
        LD.assert_rows(X, X_ref, ids, deg, paths, TOL_ROWS, f"side {dst} [{tag}]", tmp_path)
    assert orth < TOL_BASIS, (tag, orth)
    assert _below(off, TOL_EIG * gn), (tag, off, gn)
    assert np.array_equal(c.factors(src)[1].view(np.uint32), np.ascontiguousarray(Ysrc, np.float32).view(np.uint32)), tag
    return X, paths


def _sweeps(c, side):
    sv = np.zeros(4, np.int64)
    c.L.check(c.lib.als_solver_stats(c.h, side, c.L.ptr(sv, C.c_int64)))
    return int(sv[0])


def _start(gpu_lib, B, F, k, light, reg=SC.REG, alpha=SC.ALPHA, data=None):
    c = Ctx(gpu_lib, k, reg=reg, alpha=alpha, light=light)
    c.ratings(*data)
    c.inject(0, B.user_ids, F)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    return c


@pytest.mark.parametrize("case", SC.ROW_COUNT_CASES, ids=SC.case_id)
def test_gram_row_counts(gpu_lib, tmp_path, case):
    """Source sides of 1 .. 1025 rows on each Gram kernel: on both sides of the 16-row MFMA trips, the
    32-row stages of the bf16 kernel (two in flight), the 64-row fp32 partials, the rounding of a
    block's rows to 4 or 64 and the slab count ceil(n / 256), with a last block of one row."""
    n, k, kind, light = case
    B = SC.blocks(n)
    F = SC.factors(n, k, kind)
    c = _start(gpu_lib, B, F, k, light, data=SC.coo(n, SC.DEGREES))
    assert len(B.user_ids) == n
    _half(c, 1, F, B.i_ptr, B.i_col, B.i_val, SC.case_id(case), tmp_path)


@pytest.mark.parametrize("k,light", SC.LADDER_CASES, ids=[f"k{k}-light{'default' if l < 0 else l}" for k, l in SC.LADDER_CASES])
def test_rank_ladder(gpu_lib, tmp_path, k, light):
    """Ranks with the fewest and nearly the most padding columns of each padded rank (1, 2, 3, Spark's
    default 10, 63 / 65, 127 / 129, 255) on the degree ladder with per-rating confidences: the item
    half from injected unit rows, then the user half from the device's own item factors."""
    implicit, alpha, reg = LD.MODES["varying"]
    user, item, r, B = _data("varying")
    KP = LD.padded_rank(k)
    F = SC.rank_ladder_factors(k, len(B.user_ids))
    c = _start(gpu_lib, B, F, k, light, reg=reg, alpha=alpha, data=(user, item, r))
    tag = f"ladder-k{k}-light{light}"
    V, paths = _half(c, 1, F, B.i_ptr, B.i_col, B.i_val, tag, tmp_path, reg=reg, alpha=alpha)
    _check_paths(c, 1, np.diff(B.i_ptr), paths, KP, light, LD.split_chunk())
    U, paths = _half(c, 0, V, B.u_ptr, B.u_col, B.u_val, tag, tmp_path, reg=reg, alpha=alpha)
    _check_paths(c, 0, np.diff(B.u_ptr), paths, KP, light, LD.split_chunk())


@pytest.mark.parametrize("case", SC.DEGENERATE_CASES, ids=SC.case_id)
def test_degenerate_grams(gpu_lib, tmp_path, case):
    """Rank-deficient and clustered Grams: fewer source rows than the rank (k - n exact zero
    eigenvalues, a zero column-scale bound), one row repeated (rank 1), exact zero columns, G = cI.
    Four halves, there and back twice: the warm start W = B_sᵀ B_t then runs between two
    rank-deficient sides; each half against the oracle from the device's current source factors."""
    n, k, kind, light = case
    B = SC.blocks(n)
    F = SC.factors(n, k, kind)
    c = _start(gpu_lib, B, F, k, light, data=SC.coo(n, SC.DEGREES))
    src = F
    for h in range(4):
        dst = 1 - h % 2
        ptr, col, val = (B.i_ptr, B.i_col, B.i_val) if dst == 1 else (B.u_ptr, B.u_col, B.u_val)
        src, _ = _half(c, dst, src, ptr, col, val, f"{SC.case_id(case)}-half{h}", tmp_path)


@pytest.mark.parametrize("case", SC.ZERO_CASES, ids=SC.case_id)
def test_zero_source_side(gpu_lib, tmp_path, case):
    """An all-zero source side (G = 0, every eigenvalue and every column-scale bound 0): the half
    succeeds and every destination factor is exactly 0.0, Spark's x = 0 from b = 0 with lambda·n > 0;
    so does the half back from those zeros."""
    n, k, kind, light = case
    B = SC.blocks(n)
    F = SC.factors(n, k, kind)
    c = _start(gpu_lib, B, F, k, light, data=SC.coo(n, SC.DEGREES))
    X, _ = _half(c, 1, F, B.i_ptr, B.i_col, B.i_val, SC.case_id(case), tmp_path)
    assert np.isfinite(X).all() and not X.any()
    X, _ = _half(c, 0, X, B.u_ptr, B.u_col, B.u_val, SC.case_id(case) + "-back", tmp_path)
    assert np.isfinite(X).all() and not X.any()


@pytest.mark.parametrize("variant", ["full", "tiny"])
@pytest.mark.parametrize("k", SC.REG0_RANKS)
def test_implicit_reg_zero(gpu_lib, tmp_path, k, variant):
    """regParam = 0, implicit: the half reads {min Λ, max Λ} back and sends every row to the explicit
    path when min <= 1e-12 max (the push-through light solve needs Λ + lambda·n > 0).  full: a Gram of
    full rank keeps the light rows light; tiny: one column scaled by 2^-22 puts an eigenvalue ratio
    of 2^-44 below the switch.  Rows against the oracle either way."""
    n = 4 * k
    B = SC.blocks(n)
    F = SC.reg0_factors(k, variant)
    c = _start(gpu_lib, B, F, k, -1, reg=0.0, data=SC.coo(n, SC.DEGREES))
    c.all_heavy = variant == "tiny"
    _, paths = _half(c, 1, F, B.i_ptr, B.i_col, B.i_val, f"reg0-{variant}-k{k}", tmp_path, reg=0.0)
    deg = np.diff(B.i_ptr)
    st = c.stats(1).tolist()
    if variant == "tiny":
        assert st == [0, 0, deg.size, int(deg.sum())], st
    else:
        is_light = np.array([p.startswith("light") for p in paths])
        assert is_light.sum() >= 4 and (~is_light).sum() >= 2
        assert st == [int(is_light.sum()), int(deg[is_light].sum()), int((~is_light).sum()), int(deg[~is_light].sum())], st


@pytest.mark.parametrize("k", SC.REG0_RANKS)
def test_implicit_reg_zero_singular_gram_raises(gpu_lib, k):
    """regParam = 0 with one source column exactly zero: that pivot is exactly zero in every row's
    system, as in Spark's dppsv, so the half fails with its message."""
    from albedo_amd import IllegalArgumentException
    n = 4 * k
    B = SC.blocks(n)
    c = _start(gpu_lib, B, SC.reg0_factors(k, "zerocol"), k, -1, reg=0.0, data=SC.coo(n, SC.DEGREES))
    with pytest.raises(IllegalArgumentException, match="not positive definite"):
        c.half(1)
