"""Time of als_objective beside als_audit_rows of the same side, one als_run_sweeps(1) and the per-sweep
overhead of als_fit_tracked over als_fit, in one process at a bench shape (default c2: the synthetic ingest
and the seeded factors of bench.py, two sweeps fitted, one warm-up call, median of 5).  Every call ends
synchronised, so the host clock around it is the call's time; the objective's own device time
(als_objective_timing, HIP events) is recorded beside it.  Prints one JSON line and writes it to --out;
DESIGN.md ("Objective") records the c2 figures.

    python tools/objective_time.py [--config c2|c4|c1p|c5] [--out profiles/objective_c2.json]
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
REPEATS = 5
FIT_SWEEPS = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIG_RANK))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"objective_{args.config}.json")
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import CONFIGS, popularity_table, user_degrees
    lib = L.load()
    spec, k = CONFIGS[args.config], CONFIG_RANK[args.config]
    p = L.als_params()
    L.check(lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.seed, p.max_iter = k, 1, 0.5, 40.0, 42, FIT_SWEEPS
    p.nonnegative = 1 if args.config == "c5" else 0
    h = C.c_void_p()
    L.check(lib.als_create(C.byref(p), C.byref(h)))
    prefix = np.ascontiguousarray(np.r_[0, np.cumsum(user_degrees(spec))].astype(np.int64))
    cw, perm = popularity_table(spec)
    L.check(lib.als_set_ratings_synthetic(h, spec.seed, spec.rounds, spec.n_users, spec.n_items,
                                          L.ptr(prefix, C.c_int64), L.ptr(np.ascontiguousarray(cw), C.c_double),
                                          L.ptr(np.ascontiguousarray(perm), C.c_int32)))

    def timed(fn):
        L.check(lib.als_synchronize(h))
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def median(fn, setup=None):
        ms = []
        for i in range(REPEATS + 1):  # the first call warms up
            if setup:
                setup()
            ms.append(timed(fn))
        return float(np.median(ms[1:])), [round(v, 3) for v in ms[1:]]

    L.check(lib.als_init_factors_random(h, 42))
    L.check(lib.als_run_sweeps(h, FIT_SWEEPS))
    res = {"config": args.config, "rank": k, "ratings": int(lib.als_num_ratings(h)),
           "users": int(lib.als_num_rows(h, 0)), "items": int(lib.als_num_rows(h, 1)), "sweeps_fitted": FIT_SWEEPS,
           "repeats": REPEATS, "what": "host clock around synchronised calls, ms, median of the repeats"}
    tol = 1e-4 * np.sqrt(k)
    o, a = L.als_objective_t(), L.als_audit()
    for name, side in (("user", 0), ("item", 1)):
        dev = []

        def objective():
            L.check(lib.als_objective(h, side, None, C.byref(o)))
            t = np.zeros(3)
            L.check(lib.als_objective_timing(h, L.ptr(t, C.c_double)))
            dev.append(t)

        obj_ms, obj_all = median(objective)
        aud_ms, aud_all = median(lambda: L.check(lib.als_audit_rows(h, side, tol, None, C.byref(a))))
        d = np.median(np.array(dev[1:]), axis=0)
        res[name] = {"objective_ms": round(obj_ms, 3), "objective_runs": obj_all,
                     "objective_device_ms": {"gram": round(float(d[0]), 3), "rows_and_sums": round(float(d[1]), 3),
                                             "total": round(float(d[2]), 3)},
                     "audit_ms": round(aud_ms, 3), "audit_runs": aud_all,
                     "objective_over_audit": round(obj_ms / aud_ms, 3),
                     "total": o.total, "abs_terms": o.abs_terms, "rmse": float(np.sqrt(o.sse / max(o.n_ratings, 1)))}
    sweep_ms, sweep_all = median(lambda: L.check(lib.als_run_sweeps(h, 1)))
    res["run_sweeps_1_ms"] = round(sweep_ms, 3)
    res["run_sweeps_1_runs"] = sweep_all

    # als_fit_tracked against als_fit, both from the same seeded start (als_fit keeps factors that are there)
    def restart():
        L.check(lib.als_init_factors_random(h, 42))

    hist = np.zeros(FIT_SWEEPS + 1)
    n, ran = C.c_int32(0), C.c_int32(0)
    fit_ms, fit_all = median(lambda: L.check(lib.als_fit(h)), restart)
    trk_ms, trk_all = median(lambda: L.check(lib.als_fit_tracked(h, 0.0, FIT_SWEEPS + 1, L.ptr(hist, C.c_double),
                                                                 C.byref(n), C.byref(ran))), restart)
    res["fit"] = {"max_iter": FIT_SWEEPS, "als_fit_ms": round(fit_ms, 3), "als_fit_runs": fit_all,
                  "als_fit_tracked_ms": round(trk_ms, 3), "als_fit_tracked_runs": trk_all,
                  "evaluations": int(n.value),
                  "overhead_ms_per_evaluation": round((trk_ms - fit_ms) / max(n.value, 1), 3),
                  "overhead_ms_per_sweep": round((trk_ms - fit_ms) / FIT_SWEEPS, 3),
                  "history": hist[:n.value].tolist()}
    lib.als_destroy(h)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
