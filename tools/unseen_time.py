"""Time of als_recommend_unseen at a bench shape (default c2: the synthetic ingest and the seeded factors of
bench.py, two sweeps, as tools/query_topk_time.py fits it), k = 30, every user, ratings mode.  One warm-up call
per variant, then `--repeats` timed ones with the variants alternating; medians.  Recorded:

  1. als_recommend_unseen at ALBEDO_UNSEEN_DEPTH = 48 and 64: wall time (a host clock around the call, which
     ends synchronised), its five device timers and four counters; from them the share of rows in tier 2, the
     tier-2 time per row and the fraction of the dst rows the exact scan scored.
  2. als_recommend at k = 30 on the same context: the unfiltered call, the cost floor.
  3. the only other exact route to the same lists: als_recommend_vectors with the factors and the rating lists
     of `--sample` uniformly sampled users, wall time of the call alone (the lists are gathered before the
     clock starts), scaled to all users.  Its lists are compared with those of (1) for the sampled users.

Prints one JSON line and writes profiles/unseen_<config>.json; DESIGN.md records the c2 figures.

    python tools/unseen_time.py [--config c2|c4|c1p] [--repeats 5] [--sample 16384]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

STAGES = ("exclusions", "lists", "filter", "exact", "total")
COUNTERS = ("rows", "rows_exact", "entries_removed", "dst_rows_scored")


def rating_lists(model, lib, L, users):
    """(ptr, item ids): the items of each user's ratings in the context, as als_recommend_vectors takes them."""
    h, n = model._h, C.c_int64(0)
    lists = []
    for u in users:
        L.check(lib.als_get_row_ratings(h, L.ALS_USER, int(u), 0, None, None, C.byref(n)))
        src, r = np.empty(n.value, np.int32), np.empty(n.value, np.float32)
        L.check(lib.als_get_row_ratings(h, L.ALS_USER, int(u), n.value, L.ptr(src, C.c_int32), L.ptr(r, C.c_float), C.byref(n)))
        lists.append(src)
    return L.exclusion_csr(lists, len(lists))


def main():
    from query_topk_time import CONFIG_RANK, build_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIG_RANK))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16384)
    args = ap.parse_args()
    model, lib, L = build_model(args.config)
    h, k, num = model._h, model.rank, 30
    n_users, n_items = int(lib.als_num_rows(h, 0)), int(lib.als_num_rows(h, 1))

    def timed(fn):
        L.check(lib.als_synchronize(h))
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    # 1 and 2, alternating: depth 48, depth 64, als_recommend
    runs = {"48": [], "64": [], "recommend": []}
    lists = {}
    for rep in range(args.repeats + 1):
        for depth in ("48", "64"):
            os.environ["ALBEDO_UNSEEN_DEPTH"] = depth
            wall, (src, ids, sc) = timed(lambda: model.recommend_unseen_np(num))
            runs[depth].append((wall, list(model.unseen_timing().values()), list(model.unseen_stats().values())))
            if depth in lists:
                assert np.array_equal(lists[depth][0], ids) and np.array_equal(lists[depth][1].view(np.uint32), sc.view(np.uint32))
            lists[depth] = (ids, sc)
        t0 = np.zeros(5)
        L.check(lib.als_topk_timing(h, L.ptr(t0, C.c_double)))
        wall, _ = timed(lambda: model.recommend_np(num))
        t1 = np.zeros(5)
        L.check(lib.als_topk_timing(h, L.ptr(t1, C.c_double)))
        runs["recommend"].append((wall, float((t1 - t0)[:4].sum())))
    del os.environ["ALBEDO_UNSEEN_DEPTH"]
    assert np.array_equal(lists["48"][0], lists["64"][0])
    assert np.array_equal(lists["48"][1].view(np.uint32), lists["64"][1].view(np.uint32))

    unseen = {}
    for depth in ("48", "64"):
        timed_runs = runs[depth][1:]
        ms = np.median(np.array([r[1] for r in timed_runs]), axis=0)
        st = dict(zip(COUNTERS, timed_runs[-1][2]))
        unseen[depth] = {
            "wall_ms": round(statistics.median(r[0] for r in timed_runs), 3),
            "wall_runs_ms": [round(r[0], 3) for r in runs[depth]],
            "device_ms": dict(zip(STAGES, (round(float(x), 4) for x in ms))),
            "counters": st,
            "tier2_share_of_rows": round(st["rows_exact"] / max(st["rows"], 1), 5),
            "tier2_us_per_row": round(float(ms[3]) * 1e3 / max(st["rows_exact"], 1), 4),
            "tier2_fraction_of_dst_rows_scored": round(st["dst_rows_scored"] / max(st["rows_exact"] * n_items, 1), 5),
        }
    rec = runs["recommend"][1:]
    floor = {"wall_ms": round(statistics.median(r[0] for r in rec), 3), "wall_runs_ms": [round(r[0], 3) for r in runs["recommend"]],
             "device_ms": round(statistics.median(r[1] for r in rec), 4)}

    # 3. the query route on a sample, scaled
    uid, U = model.user_factors_np()
    rows = np.sort(np.random.default_rng(7).choice(n_users, min(args.sample, n_users), replace=False))
    q = np.ascontiguousarray(U[rows])
    excl = rating_lists(model, lib, L, uid[rows])
    vec_runs, vec_dev = [], []
    for _ in range(args.repeats + 1):
        wall, (vi, vs) = timed(lambda: L.recommend_vectors(h, L.ALS_ITEM, q, num, k, excl))
        vec_runs.append(wall)
        vec_dev.append(float(L.recommend_vectors_timing(h)[3]))
    same = bool(np.array_equal(vi, lists["64"][0][rows]) and np.array_equal(vs.view(np.uint32), lists["64"][1][rows].view(np.uint32)))
    scale = n_users / rows.size
    vec_wall = statistics.median(vec_runs[1:])
    best = min(unseen, key=lambda d: unseen[d]["wall_ms"])
    res = {"config": args.config, "rank": k, "users": n_users, "items": n_items, "k": num, "repeats": args.repeats,
           "gpu": "one MI355X (gfx950)", "mode": "ratings", "unseen": unseen, "faster_depth": int(best),
           "als_recommend": floor,
           "unseen_over_als_recommend_wall": {d: round(unseen[d]["wall_ms"] / floor["wall_ms"], 3) for d in unseen},
           "recommend_vectors": {"sample_users": int(rows.size), "exclusions": int(excl[1].size),
                                 "wall_ms": round(vec_wall, 3), "wall_runs_ms": [round(r, 3) for r in vec_runs],
                                 "device_total_ms": round(statistics.median(vec_dev[1:]), 4),
                                 "us_per_row": round(vec_wall * 1e3 / rows.size, 4),
                                 "scaled_to_all_users_wall_ms": round(vec_wall * scale, 1),
                                 "lists_equal_unseen": same},
           "vectors_scaled_over_unseen_wall": {d: round(vec_wall * scale / unseen[d]["wall_ms"], 2) for d in unseen}}
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", f"unseen_{args.config}.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    assert same, "als_recommend_vectors and als_recommend_unseen disagree on the sampled users"


if __name__ == "__main__":
    main()
