"""Shared pieces of the objective tests (tests/test_objective_cases.py on the CPU, tests/test_gpu_objective.py
on the GPU): a numpy fp64 restatement of als_objective's definition, row by row, and the cases, built on
the degree ladder of tests/ladder.py and the injected states of tests/audit_cases.py.

Definition (include/albedo_als.h), for dst row j with factors x, ratings r on src rows y, s = x·y:

    implicit:  c = alpha·|r|,  w = 1 + c where r > 0 else 0,  t = c·s² − 2·w·s + w,  n = #(r > 0),  G = YᵀY
    explicit:  t = (r − s)²,                                                          n = degree,    G = 0
    loss_j = xᵀ G x + Σ t + reg·n·‖x‖²
    total  = Σ_j loss_j + reg·Σ_i n_i·‖y_i‖²            (n_i from the other side's own rows)
    abs_j  = |xᵀ G x| + Σ (|c s²| + |2 w s| + |w|)  (explicit: Σ t) + reg·n·‖x‖²
    abs_terms = Σ_j abs_j + the other side's reg term:  the scale of the rounding error

Cases.  Parity and perturbation run on the injected states of tests/audit_cases.py (U unit-norm rows, V the
oracle's item half-sweep from U; the perturbed state has one component of nine item rows 1 % off: each of
those rows was at the minimum of its own loss, so its loss rises).  Trajectories start from unit-norm rows
on both sides (their absolute values with nonnegative, a feasible start) and alternate item and user
half-sweeps, the order of als_run_sweeps.
"""
import functools

import numpy as np

from oracle import spark_als as O
from tests import audit_cases as AC
from tests import ladder as LD

FIELDS = ("total", "all_pairs", "ratings", "reg_side", "reg_other", "sse", "abs_terms")

PARITY_RANKS = (1, 5, 50, 64, 65, 128, 129, 256)
PARITY_MODES = ("varying", "mixed", "stars_signed")
PARITY_CASES = [(m, k) for m in PARITY_MODES for k in PARITY_RANKS]
PARITY_TOL = 1e-10        # the project's bar for fp64 restatements (audit, explain), times the absolute terms

# (mode, rank, nonnegative).  `mixed` is left out above rank 5: its all-non-positive item rows go to zero and
# the user systems turn singular at rank 50 (the oracle raises NotPositiveDefinite)
TRAJECTORY_CASES = ([(m, k, False) for m in ("varying", "signed_uniform", "stars", "stars_signed") for k in (5, 50)] +
                    [("varying", 8, True)])
HALF_SWEEPS = 12
ORACLE_MIN_DROP = 1e-3    # the oracle's relative decrease per half-sweep is at least this (measured: 2.5e-3)

# (mode, rank): the tracked fit stops after sweep 4 with tol = sqrt(d_3·d_4), d_s = the relative decrease of sweep s
STOP_CASES = [("varying", 50), ("stars", 50), ("varying", 5), ("stars_signed", 50)]
STOP_SWEEP = 4
STOP_MARGIN = 1.2         # d_3 / d_4 is at least this

# (mode, rank): the states and rows of audit_cases.perturb.  The audit's fifth state, (stars_signed, 256), is
# left out: a 1 % change of one of 256 components lifts a row's loss by 4.9e-8 of its scale there, below the
# 1e-7 asked of every case (the rise is second order in the perturbation; the others measure 1.5e-7 to 4.6e-7)
PERTURB_CASES = [("varying", 50), ("varying", 256), ("stars_signed", 50), ("varying", 128)]
PERTURB_FACTOR = 1000.0   # a perturbed row's loss rises by this many parity tolerances of its own scale


def objective_rows(Y, X, ptr, col, val, o_ptr, o_val, *, reg, alpha, implicit):
    """The objective through the dst CSR (ptr, col, val) with dst factors X and src factors Y, in fp64 from the
    fp32 factors and ratings; (o_ptr, o_val) is the src side's own CSR, for n_i.  Returns a dict of the
    struct's fields and the per-row arrays `loss` and `abs_row`."""
    Y = np.asarray(Y, np.float64)
    X = np.asarray(X, np.float64)
    val = np.asarray(val, np.float64)
    k = Y.shape[1]
    G = Y.T @ Y if implicit else np.zeros((k, k))
    n_dst = len(ptr) - 1
    loss, abs_row = np.zeros(n_dst), np.zeros(n_dst)
    all_pairs = ratings = reg_side = sse = 0.0
    for j in range(n_dst):
        p0, p1 = int(ptr[j]), int(ptr[j + 1])
        r, x = val[p0:p1], X[j]
        s = Y[col[p0:p1]] @ x
        if implicit:
            c = alpha * np.abs(r)
            w = np.where(r > 0, 1.0 + c, 0.0)
            t = c * s * s - 2.0 * w * s + w
            a = np.abs(c * s * s) + np.abs(2.0 * w * s) + np.abs(w)
            n = float(np.sum(r > 0))
        else:
            t = (r - s) ** 2
            a = t
            n = float(p1 - p0)
        xgx = float(x @ G @ x)
        rg = reg * n * float(x @ x)
        tj = float(np.sum(t))
        loss[j] = xgx + tj + rg
        abs_row[j] = abs(xgx) + float(np.sum(a)) + rg
        all_pairs += xgx
        ratings += tj
        reg_side += rg
        sse += float(np.sum((r - s) ** 2))
    o_val = np.asarray(o_val, np.float64)
    if implicit:
        pos = np.concatenate([[0], np.cumsum(o_val > 0)])
        n_o = (pos[np.asarray(o_ptr[1:])] - pos[np.asarray(o_ptr[:-1])]).astype(np.float64)
    else:
        n_o = np.diff(o_ptr).astype(np.float64)
    reg_other = reg * float(np.sum(n_o * np.sum(Y * Y, axis=1)))
    return {"total": all_pairs + ratings + reg_side + reg_other, "all_pairs": all_pairs, "ratings": ratings,
            "reg_side": reg_side, "reg_other": reg_other, "sse": sse,
            "abs_terms": float(np.sum(abs_row)) + reg_other, "n_ratings": int(ptr[-1]), "rows": n_dst,
            "loss": loss, "abs_row": abs_row}


def objective_side(B, side, U, V, mode):
    """objective_rows through the CSR of `side` (0 = users, 1 = items) of the blocks B in rating mode `mode`."""
    implicit, alpha, reg = LD.MODES[mode]
    kw = dict(reg=reg, alpha=alpha, implicit=implicit)
    if side == 1:
        return objective_rows(U, V, B.i_ptr, B.i_col, B.i_val, B.u_ptr, B.u_val, **kw)
    return objective_rows(V, U, B.u_ptr, B.u_col, B.u_val, B.i_ptr, B.i_val, **kw)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(mode, k, perturbed=False):
    """(user side, item side) of the injected (or perturbed) state of tests/audit_cases.py."""
    B = AC.data(mode)[3]
    U, V = AC.injected(mode, k)
    if perturbed:
        V = AC.perturb(V, AC.perturbed_rows(B))
    return tuple(_freeze(objective_side(B, side, U, V, mode)) for side in (0, 1))


@functools.lru_cache(maxsize=None)
def start(mode, k, nonnegative=False):
    """(U, V): the trajectories' start, unit-norm Gaussian rows in fp32 (absolute values when nonnegative)."""
    B = AC.data(mode)[3]
    U = LD.unit_rows(np.random.default_rng(k), len(B.user_ids), k)
    V = LD.unit_rows(np.random.default_rng(1000 + k), len(B.item_ids), k)
    if nonnegative:
        U, V = np.abs(U), np.abs(V)
    U.setflags(write=False)
    V.setflags(write=False)
    return U, V


@functools.lru_cache(maxsize=None)
def oracle_trajectory(mode, k, nonnegative=False, halves=HALF_SWEEPS):
    """The objective (user side) at the start and after each of `halves` alternating oracle half-sweeps, item
    first: halves + 1 totals."""
    implicit, alpha, reg = LD.MODES[mode]
    B = AC.data(mode)[3]
    U, V = start(mode, k, nonnegative)
    kw = dict(reg=reg, alpha=alpha, implicit=implicit, nonnegative=nonnegative)
    out = [objective_side(B, 0, U, V, mode)["total"]]
    for h in range(halves):
        if h % 2 == 0:
            V = O.half_sweep(U, B.i_ptr, B.i_col, B.i_val, **kw)
        else:
            U = O.half_sweep(V, B.u_ptr, B.u_col, B.u_val, **kw)
        out.append(objective_side(B, 0, U, V, mode)["total"])
    return tuple(out)


def sweep_decreases(traj):
    """d_s, s = 1..: the relative decrease of full sweep s from a trajectory of half-sweep totals."""
    full = np.asarray(traj[::2], np.float64)
    return (full[:-1] - full[1:]) / np.abs(full[:-1])


@functools.lru_cache(maxsize=None)
def stop_tol(mode, k):
    """tol = sqrt(d_3·d_4) of the oracle's trajectory: the tracked fit's rule first holds at sweep 4."""
    d = sweep_decreases(oracle_trajectory(mode, k))
    return float(np.sqrt(d[STOP_SWEEP - 2] * d[STOP_SWEEP - 1]))
