"""CPU preconditions of the nonnegative fold-in tests (tests/foldin_nnls_cases.py): what keeps the GPU module
(tests/test_gpu_foldin_nnls.py) honest.

1. The two restatements of Spark's NNLS.solve, oracle/spark_als.py:nnls and oracle/c/als_cpu.c:nnls_solve, agree
   on every case the GPU module uses: per row to better than 1e-6 of the row's maximum, with no zero-pattern
   difference and no row at the iteration limit.  The reference is therefore determined to ~1e-6 where the
   device is held to 1e-4.  Cases on which Spark's own loop is not well determined (the `aniso` and `small`
   sources with regParam = 0, where the two restatements part by 0.08 to 0.75 and rows run into the limit) are
   not among them.
2. The bounds are active (signed unit-row sources: at least 30 % of the reference components are exactly 0),
   and at ranks >= 50 every nonzero reference row is more than 0.1 away from the Cholesky fold-in of the same
   row: a build that ignores als_fold_params.nonnegative fails every row.
3. The stop rules and the long rows are there: `large` sources stop at iteration 0 with all-zero rows, `aniso`
   with regParam = 0.5 at rank 128 has a row of at least 400 iterations.
4. The struct keeps its size with the field renamed, and ALSModel._fold_params defaults nonnegative as the
   header says.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import foldin_cases as FC
from tests import foldin_nnls_cases as FN
from tests import ladder as LD
from tests import nnls_cases as NC

ORACLE_AGREEMENT = 1e-6


def _python_oracle(c):
    ids, ptr, col, val, deg = FC.fold_csr(c.row, c.src, c.r, c.src_ids)
    X = np.zeros((ids.size, c.Y.shape[1]), np.float32)
    live = deg > 0
    lptr = np.concatenate([[0], np.cumsum(deg[live])]).astype(np.int64)
    X[live] = O.half_sweep(c.Y, lptr, col, val, reg=c.reg, alpha=c.alpha, implicit=c.implicit, nonnegative=True)
    return X


@pytest.mark.parametrize("name", list(FN.CASES))
def test_the_two_oracles_agree_on_every_gpu_case(name):
    c = FN.case(name)
    ids, deg, ref = FN.reference(name)
    X = _python_oracle(c)
    err = LD.row_errors(X, ref.X)
    flips = int(((X == 0) != (ref.X == 0)).sum())
    print(f"FOLDIN-NNLS oracles {name}: {ids.size} rows, worst row {err.max():.3e}, zero-pattern differences {flips}, "
          f"most iterations {int(ref.it.max())}")
    assert err.max() < ORACLE_AGREEMENT
    assert flips == 0
    assert int(ref.it.max()) < NC.iteration_cap(c.Y.shape[1])
    assert not ref.X[deg == 0].any() and not ref.it[deg == 0].any()
    assert (ref.X >= 0).all() and np.isfinite(ref.X).all()


def test_the_bounds_are_active_on_the_signed_sources():
    for name in FN.LADDER_CASES:
        ids, deg, ref = FN.reference(name)
        k = ref.X.shape[1]
        if k < 8:
            continue
        live = ref.X[ref.X.any(axis=1)]
        frac = float((live == 0).mean())
        assert frac >= 0.30, (name, frac)


def test_nnls_rows_are_far_from_the_cholesky_rows():
    worst = np.inf
    for name in FN.LADDER_CASES:
        mode, k = name.split("-")[1], FN.rank_of(name)
        if k < 50:
            continue
        side = 1 if name.startswith("items-") else 0
        ids, deg, ref = FN.reference(name)
        ids_c, deg_c, X_c = FC.ladder_expected(mode, k, side)
        assert np.array_equal(ids, ids_c) and np.array_equal(deg, deg_c)
        nz = ref.X.any(axis=1)
        d = LD.row_errors(X_c[nz], ref.X[nz])
        worst = min(worst, float(d.min()))
        assert d.min() > 0.1, (name, float(d.min()))
    print(f"FOLDIN-NNLS least distance of an NNLS row from its Cholesky row: {worst:.3f}")


@pytest.mark.parametrize("k", FN.KIND_RANKS)
def test_large_sources_stop_at_iteration_zero(k):
    ids, deg, ref = FN.reference(f"kind-large-k{k}")
    assert not ref.X.any() and not ref.it.any()


def test_aniso_has_a_long_row():
    ids, deg, ref = FN.reference("kind-aniso-k128")
    print(f"FOLDIN-NNLS aniso k128: most iterations {int(ref.it.max())}")
    assert 400 <= int(ref.it.max()) < NC.iteration_cap(128)


def test_the_short_rows_are_there():
    """pos / neg sources: rows that end after a few iterations, and all-zero rows."""
    its = np.concatenate([FN.reference(f"kind-{kind}-k{k}")[2].it for kind in ("pos", "neg") for k in FN.KIND_RANKS])
    assert (its <= 2).any()


@pytest.mark.parametrize("implicit", [True, False])
def test_singular_case_is_e1(implicit):
    ids, deg, ref = FN.reference(f"singular-{'implicit' if implicit else 'explicit'}")
    want = np.zeros(ref.X.shape[1], np.float32)
    want[1] = 1.0
    assert ref.X.shape[0] == 1 and np.array_equal(ref.X[0], want)


def test_struct_keeps_its_layout():
    from albedo_amd import _lib as L
    assert C.sizeof(L.als_fold_params) == 24
    assert [n for n, _ in L.als_fold_params._fields_] == ["reg_param", "alpha", "implicit_prefs", "nonnegative"]
    assert L.als_fold_params.nonnegative.offset == 20 and L.als_fold_params.nonnegative.size == 4
    p = L.als_fold_params(0.5, 10.0, 1, 0)  # four positional values, as before the rename
    assert (p.reg_param, p.alpha, p.implicit_prefs, p.nonnegative) == (0.5, 10.0, 1, 0)
    assert any(name == "als_fold_in_stats" for name, _, _ in L.SIGNATURES)


def _model(loaded, **params):
    from albedo_amd import ALS, ALSModel
    m = ALSModel.__new__(ALSModel)
    m._p = dict(ALS(**params)._p)
    m._loaded = loaded
    return m


def test_fold_params_default_nonnegative_to_the_models_own():
    fitted = _model(False, regParam=0.5, alpha=10.0, implicitPrefs=True, nonnegative=True)
    assert fitted._fold_params(None, None, None) == (0.5, 10.0, True, True)
    assert fitted._fold_params(None, None, None, False) == (0.5, 10.0, True, False)
    plain = _model(False, regParam=0.5, alpha=10.0, implicitPrefs=True)
    assert plain._fold_params(None, None, None) == (0.5, 10.0, True, False)
    assert plain._fold_params(0.1, 1.0, False, True) == (0.1, 1.0, False, True)
    loaded = _model(True, nonnegative=True)  # whatever the dict holds, a loaded model does not know its fit
    assert loaded._fold_params(0.5, 10.0, True) == (0.5, 10.0, True, False)
    assert loaded._fold_params(0.5, 10.0, True, True) == (0.5, 10.0, True, True)
    with pytest.raises(ValueError, match="regParam"):
        loaded._fold_params(None, 10.0, True, True)
