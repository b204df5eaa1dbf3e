"""The preconditions tests/test_gpu_objective.py leans on, checked on the CPU with the fp64 restatement of
tests/objective_cases.py and the oracle:

1. The restatement's total is the same from either side within 1e-12·abs_terms (a reordered sum).
2. The oracle's objective drops by at least 1e-3 relative in each of 12 half-sweeps of every trajectory case,
   so "strictly below" on the GPU is seven decades above the fp64 evaluation noise.
3. The stopping rule: with d_s the oracle's relative decrease of sweep s, d_1..d_3 exceed tol = sqrt(d_3·d_4)
   and d_3 / d_4 >= 1.2, so the tracked fit must stop after sweep 4.
4. Every perturbed row's loss rises by at least 1000 x 1e-10 x that row's own absolute-term scale.
5. The library exports the three entry points and refuses a null context.
"""
import ctypes as C

import numpy as np
import pytest

from tests import audit_cases as AC
from tests import objective_cases as OC


@pytest.mark.parametrize("case", OC.PARITY_CASES, ids=lambda c: f"{c[0]}-k{c[1]}")
def test_two_sides_agree(case):
    mode, k = case
    u, i = OC.reference(mode, k)
    d = abs(u["total"] - i["total"])
    print(f"OBJECTIVE sides {mode} k{k}: |d total| / total {d / abs(u['total']):.2e}, "
          f"abs_terms / total {u['abs_terms'] / abs(u['total']):.1f}")
    assert d <= 1e-12 * u["abs_terms"]
    assert abs(u["abs_terms"] - i["abs_terms"]) <= 1e-12 * u["abs_terms"]
    assert abs(u["sse"] - i["sse"]) <= 1e-12 * u["abs_terms"]
    assert abs(u["reg_side"] - i["reg_other"]) <= 1e-12 * u["abs_terms"]
    assert u["n_ratings"] == i["n_ratings"] == len(AC.data(mode)[0])


@pytest.mark.parametrize("case", OC.TRAJECTORY_CASES, ids=lambda c: f"{c[0]}-k{c[1]}" + ("-nonneg" if c[2] else ""))
def test_oracle_trajectory_drops(case):
    mode, k, nonneg = case
    t = np.asarray(OC.oracle_trajectory(mode, k, nonneg))
    assert t.size == OC.HALF_SWEEPS + 1 and np.all(np.isfinite(t))
    drop = (t[:-1] - t[1:]) / np.abs(t[:-1])
    print(f"OBJECTIVE oracle trajectory {mode} k{k} nonneg {int(nonneg)}: " + " ".join(f"{v:.6e}" for v in t) +
          f"; least relative drop {drop.min():.2e}")
    assert np.all(drop >= OC.ORACLE_MIN_DROP)
    if nonneg:
        U, V = OC.start(mode, k, True)
        assert U.min() >= 0 and V.min() >= 0  # a feasible start: NNLS can only go down from it


@pytest.mark.parametrize("case", OC.STOP_CASES, ids=lambda c: f"{c[0]}-k{c[1]}")
def test_stopping_rule_has_a_margin(case):
    mode, k = case
    d = OC.sweep_decreases(OC.oracle_trajectory(mode, k))
    tol = OC.stop_tol(mode, k)
    s = OC.STOP_SWEEP
    print(f"OBJECTIVE stop {mode} k{k}: d_1..d_{s} " + " ".join(f"{v:.3e}" for v in d[:s]) +
          f", tol {tol:.3e}, d_{s - 1}/d_{s} {d[s - 2] / d[s - 1]:.2f}")
    assert np.all(d[:s - 1] > tol) and d[s - 1] < tol
    assert d[s - 2] / d[s - 1] >= OC.STOP_MARGIN


@pytest.mark.parametrize("case", OC.PERTURB_CASES, ids=lambda c: f"{c[0]}-k{c[1]}")
def test_perturbation_shows(case):
    mode, k = case
    rows = AC.perturbed_rows(AC.data(mode)[3])
    base, pert = OC.reference(mode, k)[1], OC.reference(mode, k, perturbed=True)[1]
    rise = pert["loss"][rows] - base["loss"][rows]
    scale = pert["abs_row"][rows]
    print(f"OBJECTIVE perturbation {mode} k{k}: least rise / row scale {np.min(rise / scale):.2e}")
    assert np.all(rise >= OC.PERTURB_FACTOR * OC.PARITY_TOL * scale)
    others = np.setdiff1d(np.arange(base["loss"].size), rows)
    assert np.array_equal(pert["loss"][others], base["loss"][others])


def test_library_exports_the_objective_symbols():
    from albedo_amd import _lib as L
    lib = L.load()
    for name in ("als_objective", "als_objective_timing", "als_fit_tracked"):
        assert hasattr(lib, name), f"libalbedo_als.so does not export {name}"
    o = L.als_objective_t()
    assert lib.als_objective(None, 0, None, C.byref(o)) == L.ALS_E_INVALID_ARGUMENT
    out = np.zeros(3)
    assert lib.als_objective_timing(None, L.ptr(out, C.c_double)) == L.ALS_E_INVALID_ARGUMENT
    n, ran = C.c_int32(0), C.c_int32(0)
    assert lib.als_fit_tracked(None, 0.0, 0, None, C.byref(n), C.byref(ran)) == L.ALS_E_INVALID_ARGUMENT
