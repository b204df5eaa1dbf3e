"""Shared pieces of the NNLS edge suite (tests/test_gpu_nnls_edges.py on the GPU, tests/test_oracle.py
on the CPU): the NNLS degree ladder, the src-factor generators, a test-side restatement of the engine's
NNLS path choice (sweep_host.cpp rank_layout / nnls_batch_rows_limit, als_kernels.hip
launch_solve_nnls), and the per-row check against the fp64 restatement of Spark's NNLS.solve.

The per-row check (check_rows) asks of every dst row, with A = G + sum c y yT + lambda n I and b built in
fp64 (oracle.spark_als.normal_equation) and x_ref, iterations from oracle.cbind.solve_rows_nnls:

  a  x finite and >= 0;
  b  a row whose x_ref is all zero is exactly zero;
  c  kkt = max|pg| / max|b| with g = A x - b, pg_i = 0 where (x_i == 0 and g_i > 0) else g_i, at most
     margin * max(worst oracle kkt of the row's path, worst fp32-x floor of the row's path), the floor
     being 2^-24 max(|A| |x_ref|) / max|b|: both terms come from the reference;
  d  max|x - x_ref| / max|x_ref of that row| < 1e-3;
  e  the zero patterns of x and x_ref differ in at most max(1, k // 64) entries, and a differing entry is
     below 1e-3 of the row's largest on the side where it is not zero.
"""
import functools
import os
from collections import namedtuple

import numpy as np

from oracle import cbind
from oracle import spark_als as O
from tests import ladder as LD

# one item row on each side of every lockstep variant's degree limit at every padded rank (KP 64:
# 24 | 32, KP 128: 12 | 24 | 48 | 64, KP 256: 6 | 12 | 24 | 48 | 64), of the per-row kernels' 96, and of
# a split-K chunk of 256
NNLS_LADDER = [1, 2, 5, 6, 7, 11, 12, 13, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 129, 257, 513]

YBUDGET = 24576  # nnls_batch.hip: floats of Y~ per workgroup
BATCH_SLOTS = (16, 8, 4, 2, 1)
DEFAULT_MIN_SLOTS = 8
TOL = 1e-3  # the project's NNLS tolerance, here per row
KKT_MARGIN = 64.0  # the single margin of criterion c: measured, see tests/test_gpu_nnls_edges.py
ITER_BOUND = 0.15  # between two correct implementations of this loop (tests/test_gpu_parity.py)
# Cases whose device iteration sums exceed the oracle's by more than ITER_BOUND while every row passes the
# KKT criterion: (lockstep bound, per-row bound), each the measured ratio plus 5 points (None: ITER_BOUND).
# Measured, not derived; see tests/test_gpu_nnls_edges.py for the ratios and the reason.
ITER_MEASURED = {
    "aniso-k50": (0.26, None),
    "rows-k50-sv16-n1-wgsdefault": (0.22, None), "rows-k50-sv16-n1-wgs1": (0.22, None),
}


def iteration_bounds(case):
    lo, ro = ITER_MEASURED.get(case, (None, None))
    return (ITER_BOUND if lo is None else lo, ITER_BOUND if ro is None else ro)


def iteration_cap(k):
    return max(400, 20 * k)


def flip_cap(k):
    return max(1, k // 64)


def nnls_ladder_coo(seed=22, degrees=None):
    """ladder.ladder_coo over NNLS_LADDER (its own draws: the rating-mode ladder's stay as they are):
    (user, item, degree of the entry's item row), shuffled, ~700 users with sparse raw ids."""
    degrees = NNLS_LADDER if degrees is None else list(degrees)
    rng = np.random.default_rng(seed)
    n_users = 700
    uid = np.sort(rng.choice(np.arange(3, 90000, dtype=np.int64), n_users, replace=False)).astype(np.int32)
    users, items, degs = [], [], []
    for t, d in enumerate(degrees + degrees):
        users.append(uid[rng.choice(n_users, d, replace=False)])
        items.append(np.full(d, 1000 + 37 * t, np.int32))
        degs.append(np.full(d, d, np.int64))
    user, item, deg = np.concatenate(users), np.concatenate(items), np.concatenate(degs)
    perm = rng.permutation(user.size)
    return user[perm], item[perm], deg[perm]


def uniform_degree_coo(n, d, seed=23):
    """n item rows of degree d each over a pool of d + 12 users (row-count edges of one lockstep launch)."""
    rng = np.random.default_rng(seed + 1000 * n + d)
    uid = np.sort(rng.choice(np.arange(5, 5000, dtype=np.int64), d + 12, replace=False)).astype(np.int32)
    user = np.concatenate([uid[rng.choice(uid.size, d, replace=False)] for _ in range(n)])
    item = np.repeat((700 + 11 * np.arange(n)).astype(np.int32), d)
    perm = rng.permutation(user.size)
    return user[perm], item[perm]


SRC_KINDS = ("nonneg", "neg", "pos", "small", "large", "aniso")


def src_factors(kind, n, k, seed=None):
    """fp32 src factors [n, k].  nonneg: unit-norm |Gaussian| rows with the columns c % 5 == 2 negated
    (k = 1, 2 keep only positive columns); neg / pos: every entry negative / positive; small / large:
    nonneg at row norm 2^-10 / 2^10; aniso: nonneg with the columns scaled by logspace(-1, 1, k)."""
    rng = np.random.default_rng(1000 + k if seed is None else seed)
    F = np.abs(rng.standard_normal((n, k)))
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    if kind == "neg":
        F = -F
    elif kind != "pos":
        F[:, np.arange(k) % 5 == 2] *= -1.0
    if kind == "small":
        F *= 2.0 ** -10
    elif kind == "large":
        F *= 2.0 ** 10
    elif kind == "aniso":
        F *= np.logspace(-1, 1, k)[None, :]
    elif kind not in ("nonneg", "neg", "pos"):
        raise ValueError(kind)
    F = F.astype(np.float32)
    F.setflags(write=False)
    return F


# name -> (implicit, alpha, reg, ranks): the parameter edges, on the `varying` ratings
PARAM_CASES = {
    "reg0": (True, 10.0, 0.0, (50, 128, 256)),      # A = G + sum c y yT alone; the many-refresh case
    "alpha0": (True, 0.0, 0.5, (50, 128, 256)),     # Y~ all zero: A = G + lambda n I
    "stiff": (True, 200.0, 1e-3, (50, 128)),        # rank 256 takes 14 s of CPU oracle: left out
}


@functools.lru_cache(maxsize=None)
def ladder_data(mode):
    """(user, item, rating, blocks) of the NNLS ladder in a rating mode of tests/ladder.py."""
    user, item, ideg = nnls_ladder_coo()
    r = LD.ladder_ratings(mode, user, ideg)
    return user, item, r, O.make_blocks(user, item, r)


def case_params(mode, params=None):
    """(implicit, alpha, reg) of a rating mode, or of a PARAM_CASES entry."""
    return PARAM_CASES[params][:3] if params else LD.MODES[mode]


@functools.lru_cache(maxsize=None)
def item_reference(mode, k, kind="nonneg", params=None):
    """The oracle's item half of the NNLS ladder from src_factors(kind), shared by every configuration."""
    implicit, alpha, reg = case_params(mode, params)
    B = ladder_data(mode)[3]
    return reference(src_factors(kind, len(B.user_ids), k), B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit)


def fit_reference(B, U0, *, max_iter, reg, alpha, implicit):
    """oracle.spark_als.fit with nonnegative = true through the C restatement of NNLS.solve (the item half
    never reads the initial item factors)."""
    U = np.ascontiguousarray(U0, np.float32)
    k = U.shape[1]
    V = None
    for _ in range(max_iter):
        V, _ = cbind.solve_rows_nnls(U, cbind.gram(U) if implicit else np.zeros((k, k)), B.i_ptr, B.i_col, B.i_val,
                                     reg=reg, alpha=alpha, implicit=implicit)
        U, _ = cbind.solve_rows_nnls(V, cbind.gram(V) if implicit else np.zeros((k, k)), B.u_ptr, B.u_col, B.u_val,
                                     reg=reg, alpha=alpha, implicit=implicit)
    return U, V


# ---- the engine's NNLS path choice, restated -----------------------------------------------------

def batch_limits(KP, min_slots=DEFAULT_MIN_SLOTS):
    """[(slots, degree limit)] of the lockstep variants in launch order; a closed variant (fewer slots
    than ALBEDO_NNLS_MIN_SLOTS allows) has limit 0.  sweep_host.cpp nnls_batch_rows_limit."""
    if min_slots not in BATCH_SLOTS:
        min_slots = DEFAULT_MIN_SLOTS
    light = LD.light_limit(KP, -1)
    return [(sv, 0 if sv < min_slots else min(YBUDGET // (sv * KP), light)) for sv in BATCH_SLOTS]


def variant_ranges(KP, min_slots=DEFAULT_MIN_SLOTS):
    """{slots: (lowest degree, highest degree)} of the variants that can hold a row."""
    out, prev = {}, 0
    for sv, lim in batch_limits(KP, min_slots):
        if lim > prev:
            out[sv] = (prev + 1, lim)
            prev = lim
    return out


def nnls_path_of(degree, KP, chunk, min_slots=DEFAULT_MIN_SLOTS, row_kernel=None):
    """lockstep-<slots>, else row-<KP> (row-256-1024 with ALBEDO_NNLS_ROW=1024), with -split above a
    split-K chunk of `chunk` ratings (0: no split)."""
    d = int(degree)
    for sv, lim in batch_limits(KP, min_slots):
        if d <= lim:
            return f"lockstep-{sv}"
    name = f"row-{KP}" + ("-1024" if KP == 256 and str(row_kernel) == "1024" else "")
    return name + ("-split" if 0 < chunk < d else "")


def expected_nnls_paths(KP, chunk, min_slots, max_degree, row_kernel=None):
    """The labels a configuration is meant to reach with row degrees 1..max_degree."""
    out = [f"lockstep-{sv}" for sv, (lo, _) in variant_ranges(KP, min_slots).items() if lo <= max_degree]
    if max_degree > max(lim for _, lim in batch_limits(KP, min_slots)):
        out.append(nnls_path_of(max(lim for _, lim in batch_limits(KP, min_slots)) + 1, KP, 0, min_slots, row_kernel))
    if 0 < chunk < max_degree:
        out.append(nnls_path_of(chunk + 1, KP, chunk, min_slots, row_kernel))
    return out


def path_stats(deg, paths):
    """What als_path_stats reports after an NNLS half: lockstep rows, their ratings, the other rows,
    their ratings."""
    deg = np.asarray(deg)
    lock = is_lockstep(paths)
    return [int(lock.sum()), int(deg[lock].sum()), int((~lock).sum()), int(deg[~lock].sum())]


def is_lockstep(paths):
    return np.array([str(p).startswith("lockstep") for p in paths], bool)


def boundary_rows(deg, paths, KP, min_slots):
    """{slots: (rows of the variant at its limit, rows one above the limit on another path)}."""
    deg, paths = np.asarray(deg), np.asarray(paths)
    return {sv: (int(np.sum((deg == hi) & (paths == f"lockstep-{sv}"))),
                 int(np.sum((deg == hi + 1) & (paths != f"lockstep-{sv}"))))
            for sv, (_, hi) in variant_ranges(KP, min_slots).items()}


# ---- the per-row reference and check -----------------------------------------------------------------

Ref = namedtuple("Ref", "src G ptr col val reg alpha implicit X it kkt floor")


def row_kkt(ref, X, want_floor=False):
    """Per row kkt = max|pg| / max|b| of the rows of X against ref's systems (0 / inf when b = 0), and
    with want_floor the fp32-x floor 2^-24 max(|A| |x|) / max|b|."""
    n, k = X.shape
    kkt, floor = np.zeros(n), np.zeros(n)
    for j in range(n):
        A, b, ne = O.normal_equation(ref.src, ref.ptr, ref.col, ref.val, j, ref.implicit, ref.alpha, ref.G)
        A = A.copy()
        A[np.diag_indices(k)] += ref.reg * ne
        x = np.asarray(X[j], np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            g = A @ x - b
        pg = np.where((x == 0) & (g > 0), 0.0, g)
        bmax = float(np.max(np.abs(b)))
        num = float(np.max(np.abs(pg))) if np.isfinite(pg).all() else np.inf
        kkt[j] = num / bmax if bmax > 0 else (0.0 if num == 0 else np.inf)
        if want_floor and bmax > 0:
            floor[j] = 2.0 ** -24 * float(np.max(np.abs(A) @ np.abs(x))) / bmax
    return (kkt, floor) if want_floor else kkt


def reference(src, ptr, col, val, *, reg, alpha, implicit):
    """The oracle's rows, iteration counts, kkt and fp32-x floor for one half-sweep from `src`."""
    src = np.ascontiguousarray(src, np.float32)
    k = src.shape[1]
    G = cbind.gram(src) if implicit else np.zeros((k, k))
    X, it = cbind.solve_rows_nnls(src, G, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
    r = Ref(src, G, ptr, col, val, reg, alpha, implicit, X, it, None, None)
    kkt, floor = row_kkt(r, X, want_floor=True)
    for a in (X, it, kkt, floor):
        a.setflags(write=False)
    return r._replace(kkt=kkt, floor=floor)


def kkt_bounds(ref, paths, margin):
    """{path: margin * max(worst oracle kkt, worst fp32-x floor) over the path's rows}."""
    paths = np.asarray(paths)
    return {p: margin * max(float(ref.kkt[paths == p].max()), float(ref.floor[paths == p].max()))
            for p in sorted(set(paths.tolist()))}


def check_rows(X, ref, ids, deg, paths, what, tmp_path, margin, tol=TOL, tol_by_path=None, cap=None):
    """Criteria a-e of the module docstring for every row of X (the device's [n, k] factors of ref's
    half-sweep).  A failure names the failing rows' count by path and by criterion and, for the 5 worst,
    raw id, degree, path label and the figures; got / ref / ids / degrees of the failing rows are saved
    under tmp_path.  Returns {path: dict(kkt, kkt_ref, floor, bound, err, flips, rows)}."""
    ids, deg, paths = np.asarray(ids), np.asarray(deg), np.asarray(paths)
    X = np.asarray(X)
    n, k = X.shape
    assert ref.X.shape == (n, k) and ids.shape == deg.shape == paths.shape == (n,)
    cap = flip_cap(k) if cap is None else cap
    Xd, Rd = X.astype(np.float64), ref.X.astype(np.float64)
    finite = np.isfinite(Xd).all(axis=1)
    valid = finite & (np.where(np.isfinite(Xd), Xd, 0.0) >= 0).all(axis=1)
    zero_ref = ~ref.X.any(axis=1)
    zero_ok = ~zero_ref | ~X.any(axis=1)
    kkt = row_kkt(ref, np.where(np.isfinite(Xd), Xd, 0.0))
    kkt = np.where(finite, kkt, np.inf)
    bound = kkt_bounds(ref, paths, margin)
    kkt_ok = kkt <= np.array([bound[p] for p in paths])
    err = np.where(finite, LD.row_errors(np.where(np.isfinite(Xd), Xd, 0.0), Rd), np.inf)
    tols = np.array([(tol_by_path or {}).get(p, tol) for p in paths])
    err_ok = err < tols
    rmax = np.max(np.abs(Rd), axis=1, keepdims=True)
    differ = (Xd == 0) != (Rd == 0)
    flips = differ.sum(axis=1)
    small = np.where(differ, np.maximum(np.abs(Xd), np.abs(Rd)) < TOL * rmax, True).all(axis=1)
    flips_ok = (flips <= cap) & (small | zero_ref)
    crit = {"a:sign/finite": valid, "b:zero row": zero_ok, "c:kkt": kkt_ok, "d:distance": err_ok, "e:zero pattern": flips_ok}
    ok = np.ones(n, bool)
    for m in crit.values():
        ok &= m
    bad = np.nonzero(~ok)[0]
    if bad.size:
        score = np.where(np.isfinite(err), err, 1e300) + np.where(np.isfinite(kkt), kkt, 1e300)
        worst = bad[np.argsort(-score[bad], kind="stable")[:5]]
        name = "".join(ch if ch.isalnum() else "_" for ch in what)
        out = os.path.join(str(tmp_path), f"failing_rows_{name}.npz")
        np.savez(out, got=X[bad], ref=ref.X[bad], ids=ids[bad], deg=deg[bad], paths=paths[bad], err=err[bad],
                 kkt=kkt[bad], kkt_ref=ref.kkt[bad], it_ref=ref.it[bad])
        by_path = {p: int(np.sum(paths[bad] == p)) for p in sorted(set(paths[bad].tolist()))}
        by_crit = {c: int(np.sum(~m)) for c, m in crit.items() if not m.all()}
        lines = [f"  id {int(ids[r])} degree {int(deg[r])} path {paths[r]} fails "
                 f"{'+'.join(c[0] for c, m in crit.items() if not m[r])}: err {err[r]:.3e} (tol {tols[r]:g}), kkt {kkt[r]:.3e} "
                 f"(bound {bound[paths[r]]:.3e}, oracle {ref.kkt[r]:.3e}), zero-pattern flips {int(flips[r])} (cap {cap}), "
                 f"oracle iterations {int(ref.it[r])}" for r in worst]
        raise AssertionError(f"{what}: {bad.size} of {n} rows fail (by path {by_path}; by criterion {by_crit}); worst:\n"
                             + "\n".join(lines) + f"\n  failing rows saved to {out}")
    stats = {}
    for p in sorted(set(paths.tolist())):
        m = paths == p
        stats[p] = dict(rows=int(m.sum()), kkt=float(kkt[m].max()), kkt_ref=float(ref.kkt[m].max()),
                        floor=float(ref.floor[m].max()), bound=bound[p], err=float(err[m].max()), flips=int(flips[m].max()))
    return stats


def iteration_sums(it, paths):
    """(oracle iterations of the lockstep rows, of the other rows)."""
    lock = is_lockstep(paths)
    it = np.asarray(it, np.int64)
    return int(it[lock].sum()), int(it[~lock].sum())


def check_iterations(solver, ref, paths, k, what, bounds=(ITER_BOUND, ITER_BOUND)):
    """als_solver_stats [sum, max, rows, lockstep sum] against the oracle's per-row counts: every row
    counted, no row at the cap, the lockstep rows' sum and the other rows' sum each within their bound
    (`bounds`: lockstep, per-row) of the oracle's sums over the same rows.  Returns the two ratios (None where the oracle's sum is 0)."""
    solver = [int(v) for v in solver]
    want_lock, want_rest = iteration_sums(ref.it, paths)
    assert solver[2] == len(paths), (what, solver, len(paths))
    assert solver[1] < iteration_cap(k), f"{what}: a row ran to the iteration cap ({solver[1]})"
    assert int(ref.it.max(initial=0)) < iteration_cap(k), f"{what}: the oracle ran to the cap"
    ratios = []
    for name, got, want, bound in (("lockstep", solver[3], want_lock, bounds[0]),
                                   ("per-row", solver[0] - solver[3], want_rest, bounds[1])):
        assert abs(got - want) <= bound * want, f"{what}: {name} iterations {got} against the oracle's {want} (bound {bound:.0%})"
        ratios.append(got / want if want else None)
    return ratios
