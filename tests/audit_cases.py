"""Shared pieces of the row-audit tests (tests/test_audit_cases.py on the CPU, tests/test_gpu_audit.py
and tests/audit_worker.py on the GPU): a numpy fp64 restatement of als_audit_rows' definition, row by
row, and the states the tests audit, built on the degree ladder of tests/ladder.py.

Definition (include/albedo_als.h), for dst row j with factors x, ratings r_i on src rows y_i:

    implicit:  c_i = alpha·|r_i|,  w_i = 1 + c_i where r_i > 0 else 0,  n = #(r_i > 0),  G = YᵀY (all src rows)
    explicit:  c_i = 1,            w_i = r_i,                            n = degree,      G = 0
    b = Σ w_i y_i,   r = G x + Σ c_i (y_i·x) y_i + reg·n·x − b
    nonnegative:  r_m <- r_m where x_m > 0, else min(r_m, 0)             (the KKT residual)
    eta = ‖r‖₂ / ((‖G‖_F + Σ c_i ‖y_i‖² + reg·n)·‖x‖₂ + ‖b‖₂),  0 when the denominator is 0

States.  Injected: U = unit-norm Gaussian rows, V = the oracle's item half-sweep from U, rounded to
fp32, so every item row solves its equation to fp32 rounding (eta below 1e-7) while the user rows solve
nothing (eta of order 1e-2).  Perturbed: the first item row of each degree in PERTURB_DEGREES has its
largest-magnitude component multiplied by 1 + 1e-2, which lifts its eta above 1e-5; tol = 1e-6 separates
the two.  tests/test_audit_cases.py asserts both bounds for every case listed here.

The detection cases leave out mode `mixed`: its item rows of degree 2, 17, 65 and 257 hold no positive
rating, their factors are exactly zero, and a multiplicative perturbation cannot move a zero row.
"""
import functools

import numpy as np

from oracle import spark_als as O
from tests import ladder as LD

PERTURB_DEGREES = (2, 9, 17, 33, 65, 97, 129, 257, 513)
PERTURB = 1.0 + 1e-2
TOL = 1e-6
INJECTED_MAX = 1e-7   # the injected item side's largest eta stays below this
PERTURBED_MIN = 1e-5  # every perturbed row's eta is above this

PARITY_RANKS = (1, 5, 50, 64, 65, 128, 129, 256)
PARITY_MODES = ("varying", "mixed", "stars_signed")
NONNEG_RANKS = (50, 256)
# (mode, rank, nonnegative): the states whose item side the GPU tests hold to TOL
DETECTION_CASES = [(m, k, False) for m in ("varying", "stars_signed") for k in (50, 256)] + [("varying", 128, False)]
PARITY_CASES = ([(m, k, False) for m in PARITY_MODES for k in PARITY_RANKS] +
                [("varying", k, True) for k in NONNEG_RANKS])


def audit_rows(Y, X, ptr, col, val, *, reg, alpha, implicit, nonnegative=False):
    """(eta, negative) per dst row in fp64 from the fp32 factors and ratings; negative[j]: nonnegative
    and a component of X[j] below zero."""
    Y = np.asarray(Y, np.float64)
    X = np.asarray(X, np.float64)
    val = np.asarray(val, np.float64)
    k = Y.shape[1]
    G = Y.T @ Y if implicit else np.zeros((k, k))
    gnorm = np.sqrt(np.sum(G * G))
    n_dst = len(ptr) - 1
    eta = np.zeros(n_dst)
    negative = np.zeros(n_dst, bool)
    for j in range(n_dst):
        p0, p1 = int(ptr[j]), int(ptr[j + 1])
        Yj, r, x = Y[col[p0:p1]], val[p0:p1], X[j]
        if implicit:
            c = alpha * np.abs(r)
            w = np.where(r > 0, 1.0 + c, 0.0)
            n = float(np.sum(r > 0))
        else:
            c = np.ones(p1 - p0)
            w = r
            n = float(p1 - p0)
        b = Yj.T @ w
        res = G @ x + Yj.T @ (c * (Yj @ x)) + reg * n * x - b
        if nonnegative:
            res = np.where(x > 0, res, np.minimum(res, 0.0))
            negative[j] = bool(np.any(x < 0))
        s = (gnorm + np.sum(c * np.sum(Yj * Yj, axis=1)) + reg * n) * np.linalg.norm(x) + np.linalg.norm(b)
        eta[j] = 0.0 if s == 0 else np.linalg.norm(res) / s
    return eta, negative


def audit_side(B, side, U, V, mode, nonnegative=False):
    """audit_rows of dst side (0 = users, 1 = items) of the blocks B in rating mode `mode`."""
    implicit, alpha, reg = LD.MODES[mode]
    if side == 1:
        return audit_rows(U, V, B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit, nonnegative=nonnegative)
    return audit_rows(V, U, B.u_ptr, B.u_col, B.u_val, reg=reg, alpha=alpha, implicit=implicit, nonnegative=nonnegative)


@functools.lru_cache(maxsize=None)
def data(mode, seed=7):
    user, item, ideg = LD.ladder_coo(seed)
    r = LD.ladder_ratings(mode, user, ideg)
    return user, item, r, O.make_blocks(user, item, r)


@functools.lru_cache(maxsize=None)
def injected(mode, k, nonnegative=False, seed=7):
    """(U, V): unit-norm user rows (the NNLS tests' sign pattern when nonnegative) and the oracle's item
    half-sweep from them in fp32."""
    implicit, alpha, reg = LD.MODES[mode]
    B = data(mode, seed)[3]
    U = LD.unit_rows(np.random.default_rng(k), len(B.user_ids), k, nonneg=nonnegative)
    V = O.half_sweep(U, B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit, nonnegative=nonnegative)
    V = np.ascontiguousarray(V, np.float32)
    U.setflags(write=False)
    V.setflags(write=False)
    return U, V


def perturbed_rows(B, degrees=PERTURB_DEGREES):
    """The first item row (ascending id) of each degree."""
    deg = np.diff(B.i_ptr)
    return np.array([int(np.nonzero(deg == d)[0][0]) for d in degrees])


def perturb(V, rows):
    """V with the largest-magnitude component of each of `rows` multiplied by PERTURB (fp32)."""
    W = np.array(V, np.float32)
    for j in rows:
        m = int(np.argmax(np.abs(W[j])))
        W[j, m] = np.float32(np.float64(W[j, m]) * PERTURB)
    return W


@functools.lru_cache(maxsize=None)
def reference(mode, k, nonnegative=False, perturbed=False):
    """((eta_user, negative_user), (eta_item, negative_item)) of the injected (or perturbed) state."""
    B = data(mode)[3]
    U, V = injected(mode, k, nonnegative)
    if perturbed:
        V = perturb(V, perturbed_rows(B))
    out = tuple(audit_side(B, side, U, V, mode, nonnegative) for side in (0, 1))
    for e, n in out:
        e.setflags(write=False)
        n.setflags(write=False)
    return out
