"""Time of one audited half (als_audit_rows) against ALS_T_HALF_TOTAL of the same context, at a bench
shape (default c2: the synthetic ingest and the seeded factors of bench.py, one warm-up sweep, one timed
sweep).  The first audit after a half-sweep also brings both sides into the original basis (materialize);
the second one finds them there.  Prints one JSON line; DESIGN.md ("Row audit") records the c2 figures.

    python tools/audit_time.py [--config c2|c4|c1p|c5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG_RANK = {"c2": 64, "c4": 128, "c1p": 50, "c5": 256}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIG_RANK))
    args = ap.parse_args()
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import CONFIGS, popularity_table, user_degrees
    lib = L.load()
    spec, k = CONFIGS[args.config], CONFIG_RANK[args.config]
    p = L.als_params()
    L.check(lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.seed = k, 1, 0.5, 40.0, 42
    p.nonnegative = 1 if args.config == "c5" else 0
    h = C.c_void_p()
    L.check(lib.als_create(C.byref(p), C.byref(h)))
    prefix = np.ascontiguousarray(np.r_[0, np.cumsum(user_degrees(spec))].astype(np.int64))
    cw, perm = popularity_table(spec)
    L.check(lib.als_set_ratings_synthetic(h, spec.seed, spec.rounds, spec.n_users, spec.n_items,
                                          L.ptr(prefix, C.c_int64), L.ptr(np.ascontiguousarray(cw), C.c_double),
                                          L.ptr(np.ascontiguousarray(perm), C.c_int32)))
    L.check(lib.als_init_factors_random(h, 42))
    L.check(lib.als_run_sweeps(h, 1))
    half_ms = {}
    for side in (1, 0):
        L.check(lib.als_half_sweep(h, side))
        tt = np.zeros(L.ALS_T_COUNT)
        L.check(lib.als_last_timings(h, side, L.ptr(tt, C.c_double), L.ALS_T_COUNT))
        half_ms[side] = float(tt[6])
    tol = 1e-4 * np.sqrt(k)
    res = {"config": args.config, "rank": k, "ratings": int(lib.als_num_ratings(h)),
           "users": int(lib.als_num_rows(h, 0)), "items": int(lib.als_num_rows(h, 1)), "tol": tol}
    for label, side in (("user_first", 0), ("item", 1), ("user", 0)):
        a = L.als_audit()
        L.check(lib.als_synchronize(h))
        t0 = time.perf_counter()
        L.check(lib.als_audit_rows(h, side, tol, None, C.byref(a)))
        ms = (time.perf_counter() - t0) * 1e3
        res[label] = {"audit_ms": round(ms, 2), "half_total_ms": round(half_ms[side], 2),
                      "ratio": round(ms / half_ms[side], 2), "rows": a.rows, "rows_over": a.rows_over,
                      "non_finite": a.non_finite, "worst_eta": a.worst_eta, "worst_degree": a.worst_degree,
                      "worst_path": L.PATH_NAMES[a.worst_path], "mean_eta": a.sum_eta / max(a.rows, 1)}
    lib.als_destroy(h)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
