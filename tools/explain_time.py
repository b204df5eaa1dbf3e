"""Time of als_explain beside als_fold_in of the same rows, at a bench shape (default c2: the synthetic ingest
and the seeded factors of bench.py, two sweeps fitted).  Three shapes, 30 random item targets per user:
  one_user     one user of the median degree (7 ratings at c2), the src Gram cached
  long_row     one new row of 1,000 ratings of distinct items
  users_1024   the first 1,024 users, each with their own ratings
One warm-up call, then `--repeats` timed ones; medians of the wall time and of the device stages
(als_explain_timing, als_fold_in_timing).  The fold-in's code path is untouched by the explanation, so its
one-row figures should reproduce profiles/foldin_<config>.json; the tool records both and says whether they
agree within 25 %.  Prints one JSON line and writes profiles/explain_<config>.json; DESIGN.md ("Explain")
records the c2 figures.

    python tools/explain_time.py [--config c2|c4|c1p] [--repeats 5] [--targets 30]
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
    ap.add_argument("--targets", type=int, default=30)
    args = ap.parse_args()
    from albedo_amd import _lib as L
    from albedo_amd.synthetic import CONFIGS, popularity_table, user_degrees
    lib = L.load()
    spec, k = CONFIGS[args.config], CONFIG_RANK[args.config]
    p = L.als_params()
    L.check(lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.seed = k, 1, 0.5, 40.0, 42
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
    L.check(lib.als_init_factors_random(h, 42))
    L.check(lib.als_run_sweeps(h, 2))
    n_items = int(lib.als_num_rows(h, L.ALS_ITEM))
    iid = np.empty(n_items, np.int32)
    L.check(lib.als_get_ids(h, L.ALS_ITEM, L.ptr(iid, C.c_int32)))
    rng = np.random.default_rng(7)

    uids, deg = np.unique(user, return_counts=True)
    median = int(np.sort(deg)[deg.size // 2])

    def rows_of(ids):
        m = np.isin(user, ids)
        return tuple(np.ascontiguousarray(a[m]) for a in (user, item, rating))

    def targets_for(ids):
        return (np.repeat(ids, args.targets).astype(np.int32),
                np.concatenate([rng.choice(iid, args.targets, replace=False) for _ in ids]).astype(np.int32))

    one_id = uids[np.nonzero(deg == median)[0][:1]]
    long_items = rng.choice(iid, 1000, replace=False).astype(np.int32)
    long_id = np.array([int(uids.max()) + 1 if uids.max() < 2 ** 31 - 1 else -7], np.int32)
    shapes = {
        "one_user": (rows_of(one_id), targets_for(one_id)),
        "long_row": ((np.full(1000, long_id[0], np.int32), long_items, np.ones(1000, np.float32)), targets_for(long_id)),
        "users_1024": (rows_of(uids[:1024]), targets_for(uids[:1024])),
    }

    def timed(call, timing):
        wall, stages = [], []
        for _ in range(args.repeats + 1):
            L.check(lib.als_synchronize(h))
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(timing(h))
        st = np.median(np.array(stages[1:]), axis=0)
        return {"wall_ms": round(statistics.median(wall[1:]), 3), "csr_ms": round(float(st[0]), 3),
                "gram_ms": round(float(st[1]), 3), "solve_ms": round(float(st[2]), 3), "device_ms": round(float(st[3]), 3)}

    res = {"config": args.config, "rank": k, "ratings": int(n), "users": int(uids.size), "items": n_items,
           "repeats": args.repeats, "targets_per_row": args.targets, "m": 10, "gpu": "one MI355X (gfx950)", "shapes": {}}
    for name, (t, pairs) in shapes.items():
        rows = int(np.unique(t[0]).size)
        fold = timed(lambda: L.fold_in(h, L.ALS_USER, *t, k, cap=rows), L.fold_in_timing)
        ex = timed(lambda: L.explain(h, L.ALS_USER, *t, *pairs, 10), L.explain_timing)
        res["shapes"][name] = {"rows": rows, "ratings": int(t[0].size), "pairs": int(pairs[0].size), "explain": ex,
                               "fold_in": fold}
    lib.als_destroy(h)
    recorded = os.path.join(ROOT, "profiles", f"foldin_{args.config}.json")
    if os.path.exists(recorded):
        with open(recorded) as f:
            was = json.load(f)["one_row"]
        now = res["shapes"]["one_user"]["fold_in"]
        res["fold_in_one_row_recorded"] = {"degree": was["degree"], **was["gram_cached"]}
        res["fold_in_one_row_reproduces"] = bool(
            was["degree"] == res["shapes"]["one_user"]["ratings"]
            and abs(now["device_ms"] - was["gram_cached"]["device_ms"]) <= 0.25 * was["gram_cached"]["device_ms"]
            and abs(now["wall_ms"] - was["gram_cached"]["wall_ms"]) <= 0.25 * was["gram_cached"]["wall_ms"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"explain_{args.config}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
