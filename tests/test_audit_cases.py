"""The preconditions of the row-audit GPU tests (tests/test_gpu_audit.py), on the CPU: in every state
those tests inject, the numpy restatement of tests/audit_cases.py puts the item side below 1e-7, and in
every perturbed state each perturbed row above 1e-5 with every other row still below 1e-7, so that
tol = 1e-6 separates a solved row from one whose largest component is 1 % off."""
import numpy as np
import pytest

from tests import audit_cases as AC


def _id(case):
    mode, k, nonneg = case
    return f"{mode}-k{k}" + ("-nonneg" if nonneg else "")


@pytest.mark.parametrize("case", AC.PARITY_CASES, ids=_id)
def test_injected_state_is_solved(case):
    mode, k, nonneg = case
    (eta_u, neg_u), (eta_i, neg_i) = AC.reference(mode, k, nonneg)
    print(f"AUDIT_CASES {_id(case)}: item max eta {eta_i.max():.3e}, user median eta {np.median(eta_u):.3e}")
    assert np.all(np.isfinite(eta_i)) and np.all(np.isfinite(eta_u))
    assert eta_i.max() < AC.INJECTED_MAX
    assert AC.INJECTED_MAX < AC.TOL < AC.PERTURBED_MIN
    assert not neg_i.any()
    assert neg_u.all() == nonneg  # the NNLS tests' user rows carry negated columns
    if mode == "mixed":  # rows without a positive rating: x = 0 and b = 0, eta exactly 0
        B = AC.data(mode)[3]
        zero = ~AC.injected(mode, k)[1].any(axis=1)
        assert zero.sum() == 8 and np.all(eta_i[zero] == 0.0)
        assert set(np.diff(B.i_ptr)[zero].tolist()) == {2, 17, 65, 257}


@pytest.mark.parametrize("case", AC.DETECTION_CASES, ids=_id)
def test_perturbed_rows_stand_out(case):
    mode, k, nonneg = case
    B = AC.data(mode)[3]
    rows = AC.perturbed_rows(B)
    assert np.diff(B.i_ptr)[rows].tolist() == list(AC.PERTURB_DEGREES)
    eta = AC.reference(mode, k, nonneg, perturbed=True)[1][0]
    rest = np.setdiff1d(np.arange(eta.size), rows)
    print(f"AUDIT_CASES {_id(case)}: perturbed min eta {eta[rows].min():.3e}, other rows max {eta[rest].max():.3e}")
    assert eta[rows].min() > AC.PERTURBED_MIN
    assert eta[rest].max() < AC.INJECTED_MAX
    # one row at a time (the rank-128 tier cases perturb a single row)
    for d in (33, 65):
        j = AC.perturbed_rows(B, (d,))
        U, V = AC.injected(mode, k, nonneg)
        e1 = AC.audit_side(B, 1, U, AC.perturb(V, j), mode, nonneg)[0]
        assert e1[j[0]] > AC.PERTURBED_MIN and np.delete(e1, j[0]).max() < AC.INJECTED_MAX
