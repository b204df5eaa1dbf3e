"""Time of als_recommend_vectors at a bench shape (default c2: the synthetic ingest and the seeded factors of
bench.py, two sweeps).  One warm-up call, then `--repeats` timed ones; medians.  Three measurements:

  1. one new user end to end: ALSModel.recommendForNewUsers of 7 ratings, k = 30, wall time.  With
     --parent-root DIR the same call is timed on another checkout of the project (the parent commit, built),
     in a fresh child process running this file against that tree, before this process touches the GPU.
  2. device time of als_recommend_vectors (its four timers) for n_q = 1, 16, 1024 known users as queries, with
     the scan against the time to read the dst factors once at 8 TB/s (n_q = 1) and against the fp32 vector
     rate at 2 x rank unfused operations per pair (n_q = 1024: a multiply and an add are two instructions, so
     the bound is half the 157.3 TFLOPS the FMA rate is quoted at).
  3. the same queries through als_recommend over the same user subset, device time from als_topk_timing on the
     same context, for n_q = 1, 16, 64, 256, 1024: where the tuned path takes over.

Prints one JSON line and writes profiles/query_topk_<config>.json; DESIGN.md records the c2 figures.

    python tools/query_topk_time.py [--config c2|c4|c1p] [--repeats 5] [--parent-root DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG_RANK = {"c2": 64, "c4": 128, "c1p": 50}
HBM_BYTES_PER_S = 8e12
FP32_UNFUSED_OPS_PER_S = 157.3e12 / 2


def build_model(config):
    """(ALSModel over a context fitted with two sweeps, the lib, the _lib module)."""
    from albedo_amd import _lib as L
    from albedo_amd.als import ALSModel
    from albedo_amd.synthetic import CONFIGS, popularity_table, user_degrees
    lib = L.load()
    spec, k = CONFIGS[config], CONFIG_RANK[config]
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
    L.check(lib.als_init_factors_random(h, 42))
    L.check(lib.als_run_sweeps(h, 2))
    model = ALSModel(h, dict(rank=k, regParam=0.5, alpha=40.0, implicitPrefs=True))
    return model, lib, L


def new_user_wall(model, lib, repeats):
    """Wall ms of recommendForNewUsers for one unseen user with 7 ratings, k = 30: (median, all runs)."""
    n_items = int(lib.als_num_rows(model._h, 1))
    iid = np.empty(n_items, np.int32)
    from albedo_amd import _lib as L
    L.check(lib.als_get_ids(model._h, 1, L.ptr(iid, C.c_int32)))
    items = iid[np.linspace(0, n_items - 1, 7).astype(np.int64)]
    ds = {"user": np.full(7, 2 ** 31 - 5, np.int32), "item": items, "rating": np.ones(7, np.float32)}
    runs = []
    for _ in range(repeats + 1):
        L.check(lib.als_synchronize(model._h))
        t0 = time.perf_counter()
        recs = model.recommendForNewUsers(ds, 30)
        runs.append((time.perf_counter() - t0) * 1e3)
        assert len(recs) == 1 and len(recs["recommendations"][0]) == 30
    return statistics.median(runs[1:]), runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIG_RANK))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit to time measurement 1 on")
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--new-user-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    if args.new_user_only:
        model, lib, L = build_model(args.config)
        med, runs = new_user_wall(model, lib, args.repeats)
        print(json.dumps({"wall_ms": round(med, 3), "runs_ms": [round(r, 3) for r in runs]}))
        return

    parent = None
    if args.parent_root:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", args.config, "--repeats",
                              str(args.repeats), "--root", os.path.abspath(args.parent_root), "--new-user-only"],
                             check=True, capture_output=True, text=True, timeout=900).stdout
        parent = json.loads(out.strip().splitlines()[-1])

    model, lib, L = build_model(args.config)
    k, h = model.rank, model._h
    n_users, n_items = int(lib.als_num_rows(h, 0)), int(lib.als_num_rows(h, 1))
    KP = 64 if k <= 64 else 128 if k <= 128 else 256
    med, runs = new_user_wall(model, lib, args.repeats)
    one = {"wall_ms": round(med, 3), "runs_ms": [round(r, 3) for r in runs], "fold_in_device_ms": model.fold_in_timing(),
           "recommend_vectors_device_ms": model.recommend_vectors_timing()}
    if parent:
        one["parent_wall_ms"] = parent["wall_ms"]
        one["parent_runs_ms"] = parent["runs_ms"]
        one["parent_over_this"] = round(parent["wall_ms"] / med, 2)

    uid, U = model.user_factors_np()
    rng = np.random.default_rng(7)
    num = 30
    names = ("exclusions", "scan", "merge", "total")
    vec, tuned = {}, {}
    for n_q in (1, 16, 64, 256, 1024):
        rows = np.sort(rng.choice(n_users, n_q, replace=False))
        q, sub = np.ascontiguousarray(U[rows]), np.ascontiguousarray(uid[rows])
        stages, wall = [], []
        for _ in range(args.repeats + 1):
            L.check(lib.als_synchronize(h))
            t0 = time.perf_counter()
            ids, sc = L.recommend_vectors(h, L.ALS_ITEM, q, num, k)
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(L.recommend_vectors_timing(h))
        st = np.median(np.array(stages[1:]), axis=0)
        vec[n_q] = dict(zip(names, (round(float(x), 4) for x in st)))
        vec[n_q]["wall"] = round(statistics.median(wall[1:]), 3)
        dev = []
        for _ in range(args.repeats + 1):
            t0 = np.zeros(5)
            L.check(lib.als_topk_timing(h, L.ptr(t0, C.c_double)))
            src, tid, tsc = model.recommend_np(num, sub, L.ALS_USER)
            t1 = np.zeros(5)
            L.check(lib.als_topk_timing(h, L.ptr(t1, C.c_double)))
            dev.append(float((t1 - t0)[:4].sum()))
        tuned[n_q] = round(statistics.median(dev[1:]), 4)
        assert np.array_equal(src, sub) and np.array_equal(tid, ids) and np.array_equal(tsc.view(np.uint32), sc.view(np.uint32))

    read_ms = n_items * KP * 4 / HBM_BYTES_PER_S * 1e3
    ops = 2.0 * k * 1024 * n_items
    res = {"config": args.config, "rank": k, "users": n_users, "items": n_items, "k": num, "repeats": args.repeats,
           "gpu": "one MI355X (gfx950)", "new_user": one,
           "recommend_vectors_ms": {str(n): v for n, v in vec.items()},
           "als_recommend_subset_device_ms": {str(n): v for n, v in tuned.items()},
           "vectors_over_tuned": {str(n): round(vec[n]["total"] / tuned[n], 2) for n in vec},
           "n_q_1": {"dst_read_once_at_8TBs_ms": round(read_ms, 5),
                     "read_time_over_scan": round(read_ms / vec[1]["scan"], 4)},
           "n_q_1024": {"unfused_ops": ops, "scan_ops_per_s": round(ops / (vec[1024]["scan"] * 1e-3)),
                        "fraction_of_unfused_fp32_vector_rate":
                            round(ops / (vec[1024]["scan"] * 1e-3) / FP32_UNFUSED_OPS_PER_S, 4)}}
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", f"query_topk_{args.config}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
