"""Inputs of the front-end parity tests (tests/test_gpu_gram_eig_edges.py on the GPU, their
preconditions in tests/test_oracle.py on the CPU): what every implicit half-sweep does before its
per-row solves -- the source side's Gram, its eigenbasis by the warm-started Jacobi of eig.hip, the
rotation into that basis and the column scales.

  spectrum(kind, k)        symmetric fp64 matrices for als_device_eigh (SPECTRA; spectrum_kinds(k)
                           leaves out the kinds that mean nothing at a tiny k)
  warm_starts(G)           warm starts for a matrix: exact / permuted / reflected / noisy eigenvectors
  factors(n_src, k, kind)  fp32 source factor matrices (FACTOR_KINDS)
  coo(n_src, degrees)      a tiny rating set: n_src source ids, destination rows of chosen degrees
  ROW_COUNT_CASES, ...     the half-sweep cases of the GPU file, one record each
  ref_sweeps(G)            sweeps of the numpy restatement of the Jacobi (tools/jacobi_ref.py)
  REF_SWEEPS               that count at k > 65 (the restatement takes up to 10 s per matrix there)

numpy (and scipy's LAPACK for the fp32 check) only, every draw seeded by the case's own name.
"""
import functools
import zlib

import numpy as np
import scipy.linalg

from oracle import spark_als as O
from tests import ladder as LD
from tools import jacobi_ref as JR

# ---- symmetric matrices for the eigensolver ------------------------------------------------------

SPECTRA = ("identity", "zero", "diag", "allones", "rank1", "deficient", "pairs", "twoclusters", "graded", "zerocols",
           "sparkinit")
# the smallest k at which a kind is not one of the others (allones at k = 1 is identity, pairs at
# k = 2 is identity, a cluster needs two members, every third column zero needs three columns)
MIN_K = {"identity": 1, "zero": 1, "diag": 1, "allones": 2, "rank1": 2, "deficient": 2, "pairs": 4, "twoclusters": 4,
         "graded": 2, "zerocols": 3, "sparkinit": 2}
EIG_KS = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256)
IDENTITY_C = 3.0
CLUSTER_WIDTH = 1e-15
SPARKINIT_ROWS = 20000


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _orthogonal(rng, k):
    Q, R = np.linalg.qr(rng.standard_normal((k, k)))
    return Q * np.sign(np.diag(R))


def _sym(A):
    return (A + A.T) * 0.5


def spectrum_kinds(k):
    return [s for s in SPECTRA if k >= MIN_K[s]]


def deficient_rows(k):
    return max(1, k // 10)


def pairs_eigenvalues(k):
    """Every eigenvalue twice over 3 decades (odd k: the largest once more)."""
    return np.repeat(np.logspace(0, 3, (k + 1) // 2), 2)[:k]


def twoclusters_eigenvalues(k, rng):
    w = np.r_[np.full(k // 2, 1.0), np.full(k - k // 2, 2.0)]
    return w * (1.0 + CLUSTER_WIDTH * rng.uniform(-1, 1, k))


@functools.lru_cache(maxsize=None)
def spectrum(kind, k):
    """The k x k matrix of `kind`: fp64, exactly symmetric, read-only."""
    rng = _rng("spectrum", kind, k)
    if kind == "identity":
        G = IDENTITY_C * np.eye(k)
    elif kind == "zero":
        G = np.zeros((k, k))
    elif kind == "diag":  # already diagonal, distinct entries over 2 decades, in no order
        G = np.diag(rng.permutation(np.logspace(0, 2, k)))
    elif kind == "allones":
        G = np.ones((k, k))
    elif kind == "rank1":
        x = rng.standard_normal(k)
        G = np.outer(x, x)
    elif kind == "deficient":
        X = rng.standard_normal((deficient_rows(k), k))
        G = X.T @ X
    elif kind == "pairs":
        Q = _orthogonal(rng, k)
        G = (Q * pairs_eigenvalues(k)) @ Q.T
    elif kind == "twoclusters":
        Q = _orthogonal(rng, k)
        G = (Q * twoclusters_eigenvalues(k, rng)) @ Q.T
    elif kind == "graded":
        X = rng.standard_normal((4 * k, k)) * np.logspace(-4, 4, k)
        G = X.T @ X
    elif kind == "zerocols":
        X = rng.standard_normal((4 * k, k))
        X[:, ::3] = 0.0
        G = X.T @ X
    elif kind == "sparkinit":
        G = O.gram(LD.unit_rows(rng, SPARKINIT_ROWS, k))
    else:
        raise ValueError(kind)
    G = _sym(G)
    G.setflags(write=False)
    return G


WARM_STARTS = ("exact", "permuted", "reflected", "noisy")
WARM_NOISE = 1e-8


def warm_starts(G):
    """name -> W0 (columns: the start's basis vectors) for the symmetric matrix G."""
    k = G.shape[0]
    rng = _rng("warm", k, float(G[0, 0]))
    V = np.linalg.eigh(G)[1]
    refl = V.copy()
    refl[:, k // 2] *= -1.0
    return {"exact": V, "permuted": np.ascontiguousarray(V[:, rng.permutation(k)]), "reflected": refl,
            "noisy": V + WARM_NOISE * rng.standard_normal((k, k))}


def ref_sweeps(G, tol=JR.JAC_TOL):
    """(w, VT, sweeps) of the numpy restatement on G with the device's budget rule: the device checks
    before each sweep, and when sweep JAC_MAX_SWEEPS + 1 would be needed it accepts the run if the mass
    is at most JAC_ACCEPT of the diagonal's and fails it otherwise (sweeps is None then)."""
    trace = []
    w, VT, s = JR.jacobi(G, tol=tol, max_sweeps=JR.JAC_MAX_SWEEPS + 1, trace=trace)
    if s == JR.JAC_MAX_SWEEPS and trace[s] > JR.JAC_ACCEPT:
        s = None
    return w, VT, s


# Sweeps of tools/jacobi_ref.py on spectrum(kind, k) from the identity at k > 65, where the restatement
# (dense k x k products per round) takes up to 10 s per matrix: produced once by
# `python -m tests.spectrum_cases` with single-threaded BLAS; tests/test_oracle.py re-runs two entries.
REF_SWEEPS = {
    ("identity", 127): 0, ("zero", 127): 0, ("diag", 127): 0, ("allones", 127): 1, ("rank1", 127): 1,
    ("deficient", 127): 8, ("pairs", 127): 12, ("twoclusters", 127): 20, ("graded", 127): 4, ("zerocols", 127): 9,
    ("sparkinit", 127): 8,
    ("identity", 128): 0, ("zero", 128): 0, ("diag", 128): 0, ("allones", 128): 1, ("rank1", 128): 1,
    ("deficient", 128): 9, ("pairs", 128): 12, ("twoclusters", 128): 20, ("graded", 128): 5, ("zerocols", 128): 9,
    ("sparkinit", 128): 9,
    ("identity", 129): 0, ("zero", 129): 0, ("diag", 129): 0, ("allones", 129): 1, ("rank1", 129): 1,
    ("deficient", 129): 7, ("pairs", 129): 12, ("twoclusters", 129): 20, ("graded", 129): 4, ("zerocols", 129): 9,
    ("sparkinit", 129): 8,
    ("identity", 255): 0, ("zero", 255): 0, ("diag", 255): 0, ("allones", 255): 1, ("rank1", 255): 1,
    ("deficient", 255): 8, ("pairs", 255): 12, ("twoclusters", 255): 22, ("graded", 255): 4, ("zerocols", 255): 9,
    ("sparkinit", 255): 10,
    ("identity", 256): 0, ("zero", 256): 0, ("diag", 256): 0, ("allones", 256): 1, ("rank1", 256): 1,
    ("deficient", 256): 10, ("pairs", 256): 12, ("twoclusters", 256): 22, ("graded", 256): 5, ("zerocols", 256): 9,
    ("sparkinit", 256): 9,
}


def reference_sweeps(kind, k):
    return REF_SWEEPS[kind, k] if k > 65 else ref_sweeps(spectrum(kind, k))[2]


# ---- source factor matrices ----------------------------------------------------------------------

FACTOR_KINDS = ("unit", "same", "zerocols", "ortho", "zero")
SAME_ROWS = 10
ZEROCOLS_ROWS = 300


def ortho_rows(k):
    """Row count of the `ortho` kind at rank k: whole copies of a k x k matrix, about 512 rows."""
    return k * max(2, round(512 / k))


@functools.lru_cache(maxsize=None)
def factors(n_src, k, kind):
    """(n_src, k) fp32, read-only.  unit: unit-norm Gaussian rows; same: one such row n_src times
    (rank 1); zerocols: unit rows with every third column exactly zero; ortho: the rows of 0.5·Q,
    Q orthogonal, repeated n_src / k times (G = 0.25 (n_src / k) I up to the fp32 rounding of Q);
    zero: all zeros."""
    rng = _rng("factors", n_src, k, kind)
    if kind == "unit":
        F = LD.unit_rows(rng, n_src, k)
    elif kind == "same":
        F = np.repeat(LD.unit_rows(rng, 1, k), n_src, axis=0)
    elif kind == "zerocols":
        F = LD.unit_rows(rng, n_src, k)
        F[:, ::3] = 0.0
    elif kind == "ortho":
        assert n_src % k == 0, (n_src, k)
        F = np.tile((0.5 * _orthogonal(rng, k)).astype(np.float32), (n_src // k, 1))
    elif kind == "zero":
        F = np.zeros((n_src, k), np.float32)
    else:
        raise ValueError(kind)
    F = np.ascontiguousarray(F, np.float32)
    F.setflags(write=False)
    return F


# ---- rating sets ---------------------------------------------------------------------------------

RATINGS = (0.25, 0.5, 1.0, 2.0, 4.0)  # the `varying` set of tests/ladder.py: all positive
COVER_DEGREE = 32


@functools.lru_cache(maxsize=None)
def coo(n_src, degrees, seed=0):
    """(user, item, rating): n_src source ("user") ids, one destination ("item") row of degree
    min(n_src, d) for each d of `degrees` (distinct sources per row), then rows of up to COVER_DEGREE
    sources over the source ids no row has rated yet, so that the ingest keeps every source id.
    Sparse raw ids on both sides, shuffled, ratings from RATINGS."""
    rng = _rng("coo", n_src, degrees, seed)
    uid = np.sort(rng.choice(np.arange(-50000, 50000, dtype=np.int64), n_src, replace=False)).astype(np.int32)
    rows = [rng.choice(n_src, min(n_src, d), replace=False) for d in degrees]
    left = np.setdiff1d(np.arange(n_src), np.concatenate(rows))
    rows += [left[i:i + COVER_DEGREE] for i in range(0, left.size, COVER_DEGREE)]
    user = np.concatenate([uid[r] for r in rows])
    item = np.concatenate([np.full(len(r), 500 + 13 * t, np.int32) for t, r in enumerate(rows)])
    rating = rng.choice(RATINGS, user.size).astype(np.float32)
    perm = rng.permutation(user.size)
    out = user[perm], item[perm], rating[perm]
    for a in out:
        a.setflags(write=False)
    return out


# ---- the half-sweep cases ------------------------------------------------------------------------

# alpha: a destination row of degree 1 has cond(A) >= (‖G‖ + alpha·r) / reg whatever the row count or the
# degrees, and on the way back the few destination rows are the (rank-deficient) source side of rows of
# degree 1-3.  With alpha = 40 a plain fp32 Cholesky of these systems is 1e-5 .. 3e-3 from fp64, with 10
# up to 3e-4, with 5 up to 9e-5, with 3 up to 3e-5; with alpha = 2 (confidences 0.5 .. 8), 10 identical
# rows in `same` and cover rows of 32 it stays below 1.8e-5 on every half
# (test_front_end_half_sweep_inputs_are_well_conditioned holds it below 2e-5).
REG, ALPHA = 0.5, 2.0
DEGREES = (1, 8, 9, 17, 70, 150)
ROW_COUNTS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025)
ROW_COUNT_RANKS = (64, 100, 256)  # one per Gram kernel: fp32 MFMA at KP 64, bf16 at KP 128, fp32 at KP 256
LADDER_RANKS = (1, 2, 3, 10, 63, 65, 127, 129, 255)
LADDER_RANKS_HEAVY = (3, 10, 65, 129)
DEGENERATE_RANKS = (50, 128, 200)
DEFICIENT_ROWS = (1, 2, 5, 40)
REG0_RANKS = (50, 128)
REG0_SCALE = 2.0 ** -22  # one column scaled by this: an eigenvalue ratio of 2^-44 < 1e-12


def degenerate_cases(k):
    """(n_src, kind) of the degenerate Grams at rank k."""
    return ([(n, "unit") for n in DEFICIENT_ROWS]
            + [(SAME_ROWS, "same"), (ZEROCOLS_ROWS, "zerocols"), (ortho_rows(k), "ortho")])


def case_id(c):
    return "-".join(str(x) for x in c)


# (n_src, k, kind, light): light -1 is the engine's default limit, 0 sends every row to the explicit path
ROW_COUNT_CASES = [(n, k, "unit", -1) for k in ROW_COUNT_RANKS for n in ROW_COUNTS]
DEGENERATE_CASES = [(n, k, kind, light) for k in DEGENERATE_RANKS for n, kind in degenerate_cases(k) for light in (-1, 0)]
ZERO_CASES = [(64, k, "zero", light) for k in (50, 128) for light in (-1, 0)]
LADDER_CASES = [(k, -1) for k in LADDER_RANKS] + [(k, 0) for k in LADDER_RANKS_HEAVY]


def reg0_factors(k, variant):
    """4k unit rows; "full": as they are, "tiny": column 1 scaled by 2^-22, "zerocol": column 1 zero."""
    F = np.array(factors(4 * k, k, "unit"))
    if variant == "tiny":
        F[:, 1] *= np.float32(REG0_SCALE)
    elif variant == "zerocol":
        F[:, 1] = 0.0
    else:
        assert variant == "full"
    return F


@functools.lru_cache(maxsize=None)
def blocks(n_src, degrees=DEGREES):
    user, item, r = coo(n_src, degrees)
    return O.make_blocks(user, item, r)


# ---- fp64 row systems, solved in fp64 and in plain fp32 -----------------------------------------

def row_solutions(Y, ptr, col, val, reg=REG, alpha=ALPHA, dtype=np.float64, gram=None):
    """The implicit normal equations of every destination row, built in fp64 as
    oracle.spark_als.normal_equation builds them (A = G + Σ c y yᵀ + reg·n·I, b = Σ (1 + c) y over the
    positive ratings), then cast to `dtype` and solved there by LAPACK's Cholesky of that precision.
    gram: G to use instead of YᵀY."""
    Y = np.asarray(Y)
    k = Y.shape[1]
    G = O.gram(Y) if gram is None else gram
    X = np.zeros((len(ptr) - 1, k))
    for j in range(len(ptr) - 1):
        A, b, n = O.normal_equation(Y, ptr, col, val, j, True, alpha, G)
        A = (A + reg * n * np.eye(k)).astype(dtype)
        X[j] = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A), b.astype(dtype))  # potrf / potrs of `dtype`
    return X


def rhs_cancellation(Y, ptr, col, val, alpha=ALPHA):
    """The worst row's Σ_e |(1 + c_e) y_e| / |Σ_e (1 + c_e) y_e| (largest component of each, positive
    ratings): how much of b = Σ (1 + c) y cancels.  Any fp32 accumulation of b is off by about 2^-24
    times this, whatever the solve; at rank 1 that is the row's whole error."""
    Y = np.asarray(Y, np.float64)
    worst = 1.0
    for j in range(len(ptr) - 1):
        e = slice(int(ptr[j]), int(ptr[j + 1]))
        r = np.asarray(val[e], np.float64)
        t = Y[col[e]][r > 0] * (1.0 + alpha * r[r > 0])[:, None]
        b = np.abs(t.sum(axis=0)).max() if t.size else 0.0
        if b > 0:
            worst = max(worst, float(np.abs(t).sum(axis=0).max() / b))
    return worst


LADDER_SEED = {1: 1002}  # rank -> seed of the ladder's unit rows when it is not the rank (rank_ladder_factors)


def rank_ladder_factors(k, n):
    """The unit rows the rank ladder starts from: ladder.unit_rows seeded by the rank, as
    test_half_sweep_ranks_and_paths seeds them.  At rank 1 unit rows are +-1 and that draw leaves a
    user row of degree 10 whose b cancels 3551-fold (2e-4 in fp32 before any solve; the device
    measured 3.5e-4 on it): the seed there is the first of 1001, 1002, .. whose two halves keep
    rhs_cancellation below 2e-5 · 2^24 = 335, the fp32 condition of tests/test_oracle.py on every rank."""
    F = LD.unit_rows(np.random.default_rng(LADDER_SEED.get(k, k)), n, k)
    F.setflags(write=False)
    return F


if __name__ == "__main__":  # the REF_SWEEPS table
    import sys
    for k in [int(a) for a in sys.argv[1:]] or [k for k in EIG_KS if k > 65]:
        for kind in spectrum_kinds(k):
            print(f'    ("{kind}", {k}): {ref_sweeps(spectrum(kind, k))[2]},', flush=True)
