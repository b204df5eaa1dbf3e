"""Time of als_fold_in against the half-sweep of the same rows, at a bench shape (default c2: the synthetic
ingest and the seeded factors of bench.py, two warm-up sweeps).  Every user is folded in with their own
ratings against the fitted item factors, which is the work of als_half_sweep(ALS_USER) from the same
context; the tool prints rows/s and the four stage times of als_fold_in_timing beside ALS_T_HALF_TOTAL,
the distance of the fold-in's rows from the half-sweep's, and the latency of a one-row call with the src
Gram cached and not.  One warm-up call, then `--repeats` timed ones; medians.  Prints one JSON line and
writes profiles/foldin_<config>.json; DESIGN.md ("Fold-in") records the c2 figures.

With --nonnegative the context is fitted with nonnegative = true, so its factors are nonnegative and its
half-sweep is the NNLS one; every user is folded in twice, by NNLS (als_fold_params.nonnegative = 1) and by
Cholesky on the same build and rows, with the iteration counters of als_fold_in_stats, and the one-row latency is
taken for both.  Writes profiles/foldin_nnls_<config>.json.

    python tools/foldin_time.py [--config c2|c4|c1p] [--repeats 5] [--nonnegative]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG_RANK = {"c2": 64, "c4": 128, "c1p": 50}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIG_RANK))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nonnegative", action="store_true")
    args = ap.parse_args()
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import CONFIGS, popularity_table, user_degrees
    lib = L.load()
    spec, k = CONFIGS[args.config], CONFIG_RANK[args.config]
    p = L.als_params()
    L.check(lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.seed = k, 1, 0.5, 40.0, 42
    p.nonnegative = int(args.nonnegative)
    h = C.c_void_p()
    L.check(lib.als_create(C.byref(p), C.byref(h)))
    prefix = np.ascontiguousarray(np.r_[0, np.cumsum(user_degrees(spec))].astype(np.int64))
    cw, perm = popularity_table(spec)
    cw, perm = np.ascontiguousarray(cw), np.ascontiguousarray(perm)
    L.check(lib.als_set_ratings_synthetic(h, spec.seed, spec.rounds, spec.n_users, spec.n_items, L.ptr(prefix, C.c_int64),
                                          L.ptr(cw, C.c_double), L.ptr(perm, C.c_int32)))
    n = int(prefix[-1])
    user, item, rating = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    nout = C.c_int64()
    L.check(lib.als_synth_generate(-1, spec.seed, spec.rounds, spec.n_users, spec.n_items, L.ptr(prefix, C.c_int64),
                                   L.ptr(cw, C.c_double), L.ptr(perm, C.c_int32), L.ptr(user, C.c_int32),
                                   L.ptr(item, C.c_int32), L.ptr(rating, C.c_float), C.byref(nout)))
    n = nout.value
    user, item, rating = user[:n], item[:n], rating[:n]
    assert n == lib.als_num_ratings(h)
    L.check(lib.als_init_factors_random(h, 42))
    L.check(lib.als_run_sweeps(h, 2))

    half = []
    for _ in range(args.repeats + 1):  # the same half again: the items do not move
        L.check(lib.als_half_sweep(h, L.ALS_USER))
        tt = np.zeros(L.ALS_T_COUNT)
        L.check(lib.als_last_timings(h, L.ALS_USER, L.ptr(tt, C.c_double), L.ALS_T_COUNT))
        half.append(float(tt[6]))
    half_ms = statistics.median(half[1:])
    n_users = int(lib.als_num_rows(h, L.ALS_USER))
    U = np.empty((n_users, k), np.float32)
    L.check(lib.als_get_factors(h, L.ALS_USER, None, L.ptr(U, C.c_float)))
    if args.nonnegative:
        return nonnegative_run(args, L, lib, h, spec, k, user, item, rating, n, n_users, U, half_ms)

    stages, wall = [], []
    for _ in range(args.repeats + 1):
        L.check(lib.als_synchronize(h))
        t0 = time.perf_counter()
        ids, deg, X = L.fold_in(h, L.ALS_USER, user, item, rating, k, cap=n_users)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(L.fold_in_timing(h))
    st = np.median(np.array(stages[1:]), axis=0)
    assert ids.size == n_users and int(deg.sum()) == n
    num = np.max(np.abs(X.astype(np.float64) - U), axis=1)
    den = np.maximum(np.max(np.abs(U), axis=1), 1e-30)

    # one row: a user of the median degree
    target = int(np.sort(deg)[deg.size // 2])
    uid = int(ids[np.nonzero(deg == target)[0][0]])
    m = user == uid
    one = (np.ascontiguousarray(user[m]), np.ascontiguousarray(item[m]), np.ascontiguousarray(rating[m]))
    n_items = int(lib.als_num_rows(h, L.ALS_ITEM))
    iid, V = np.empty(n_items, np.int32), np.empty((n_items, k), np.float32)
    L.check(lib.als_get_factors(h, L.ALS_ITEM, L.ptr(iid, C.c_int32), L.ptr(V, C.c_float)))

    def one_row():
        L.check(lib.als_synchronize(h))
        t0 = time.perf_counter()
        L.fold_in(h, L.ALS_USER, *one, k, cap=1)
        return (time.perf_counter() - t0) * 1e3, L.fold_in_timing(h)

    one_row()
    cached = [one_row() for _ in range(4 * args.repeats)]
    uncached = []
    for _ in range(args.repeats):  # the same item factors injected again: the cached Gram is dropped
        L.check(lib.als_set_initial_factors(h, L.ALS_ITEM, n_items, L.ptr(iid, C.c_int32), L.ptr(V, C.c_float)))
        uncached.append(one_row())
    lib.als_destroy(h)

    def lat(runs):
        return {"wall_ms": round(statistics.median(w for w, _ in runs), 3),
                "device_ms": round(statistics.median(float(t[3]) for _, t in runs), 3),
                "gram_ms": round(statistics.median(float(t[1]) for _, t in runs), 3)}

    res = {"config": args.config, "rank": k, "ratings": n, "users": n_users, "items": n_items,
           "repeats": args.repeats, "gpu": "one MI355X (gfx950)",
           "half_sweep_user_total_ms": round(half_ms, 2),
           "fold_in_ms": {"csr": round(float(st[0]), 2), "gram": round(float(st[1]), 2), "solve": round(float(st[2]), 2),
                          "total": round(float(st[3]), 2), "wall": round(statistics.median(wall[1:]), 2),
                          "gram_first_call": round(float(stages[0][1]), 2)},
           "fold_in_rows_per_s": round(n_users / (float(st[3]) * 1e-3)),
           "solve_over_half_sweep": round(float(st[2]) / half_ms, 2),
           "total_over_half_sweep": round(float(st[3]) / half_ms, 2),
           "worst_row_vs_half_sweep": float(np.max(num / den)),
           "one_row": {"degree": target, "gram_cached": lat(cached), "gram_uncached": lat(uncached)}}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"foldin_{args.config}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def nonnegative_run(args, L, lib, h, spec, k, user, item, rating, n, n_users, U, half_ms):
    """The NNLS fold-in beside the Cholesky fold-in of the same rows and the NNLS half-sweep of the context."""
    kw = dict(reg_param=0.5, alpha=40.0, implicit_prefs=True)

    def rel(X):
        num = np.max(np.abs(X.astype(np.float64) - U), axis=1)
        return float(np.max(num / np.maximum(np.max(np.abs(U), axis=1), 1e-30)))

    def bulk(nonneg):
        stages, wall = [], []
        for _ in range(args.repeats + 1):
            L.check(lib.als_synchronize(h))
            t0 = time.perf_counter()
            ids, deg, X = L.fold_in(h, L.ALS_USER, user, item, rating, k, cap=n_users, nonnegative=nonneg, **kw)
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(L.fold_in_timing(h))
        st = np.median(np.array(stages[1:]), axis=0)
        assert ids.size == n_users and int(deg.sum()) == n
        its = [int(v) for v in L.fold_in_stats(h)]
        out = {"csr": round(float(st[0]), 2), "solve": round(float(st[2]), 2), "total": round(float(st[3]), 2),
               "wall": round(statistics.median(wall[1:]), 2), "rows_per_s": round(n_users / (float(st[3]) * 1e-3)),
               "solve_over_half_sweep": round(float(st[2]) / half_ms, 2), "worst_row_vs_half_sweep": rel(X)}
        if nonneg:
            out.update(iterations=its[0], most_iterations=its[1], rows_solved=its[2], rows_at_limit=its[3],
                       negative_components=int((X < 0).sum()))
        return out, ids, deg

    nn, ids, deg = bulk(True)
    ch, _, _ = bulk(False)
    target = int(np.sort(deg)[deg.size // 2])
    uid = int(ids[np.nonzero(deg == target)[0][0]])
    m = user == uid
    one = (np.ascontiguousarray(user[m]), np.ascontiguousarray(item[m]), np.ascontiguousarray(rating[m]))

    def one_row(nonneg):
        runs = []
        for _ in range(4 * args.repeats + 1):
            L.check(lib.als_synchronize(h))
            t0 = time.perf_counter()
            L.fold_in(h, L.ALS_USER, *one, k, cap=1, nonnegative=nonneg, **kw)
            runs.append(((time.perf_counter() - t0) * 1e3, L.fold_in_timing(h), int(L.fold_in_stats(h)[0])))
        runs = runs[1:]
        return {"wall_ms": round(statistics.median(w for w, _, _ in runs), 3),
                "device_ms": round(statistics.median(float(t[3]) for _, t, _ in runs), 3),
                "solve_ms": round(statistics.median(float(t[2]) for _, t, _ in runs), 3), "iterations": runs[-1][2]}

    one_nn, one_ch = one_row(True), one_row(False)
    n_items = int(lib.als_num_rows(h, L.ALS_ITEM))
    lib.als_destroy(h)
    res = {"config": args.config, "rank": k, "nonnegative": True, "ratings": n, "users": n_users, "items": n_items,
           "repeats": args.repeats, "gpu": "one MI355X (gfx950)",
           "half_sweep_user_total_ms": round(half_ms, 2),
           "fold_in_nnls_ms": nn, "fold_in_cholesky_ms": ch,
           "one_row": {"degree": target, "nnls": one_nn, "cholesky": one_ch}}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"foldin_nnls_{args.config}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
