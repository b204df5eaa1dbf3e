"""Time of als_similar at a bench shape (default c2: the synthetic ingest and the seeded factors of bench.py,
two sweeps).  One warm-up call, then `--repeats` timed ones; medians.  Measurements:

  1. als_similar on the item side for 1, 16, 1,024, 16,384 and all items in each forced tier
     (ALBEDO_SIMILAR_TIER): device time by stage (als_similar_timing) and wall time; where the tiers' wall
     times cross.  The user side for 1,024 and all users in both tiers.
  2. what the passes tier rebuilds per call, from one traced call (ALBEDO_SIMILAR_TRACE): the unit image, the
     transient context, and the transient context's own counters: how far its passes prune on unit rows and
     how many rows fail certification.
  3. the caller-side route through calls the project had before als_similar: als_get_factors, numpy
     normalise, als_model_create with the image as both sides, als_recommend at k + 1, drop self; for one
     item and for all of them, in this process.

Prints one JSON line and writes profiles/similar_<config>.json (or --out); DESIGN.md records the c2 figures.

    python tools/similar_time.py [--config c2|c4|c1p] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

NAMES = ("unit_image", "lists", "merge", "total")


def timed(model, L, lib, num, subset, side, tier, repeats):
    if tier:
        os.environ["ALBEDO_SIMILAR_TIER"] = tier
    else:
        os.environ.pop("ALBEDO_SIMILAR_TIER", None)  # the default tier, by the row count
    stages, wall, st = [], [], None
    for _ in range(repeats + 1):
        L.check(lib.als_synchronize(model._h))
        t0 = time.perf_counter()
        out = model.similar_np(num, subset, side)
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(L.similar_timing(model._h))
        st = model.similar_stats()
    os.environ.pop("ALBEDO_SIMILAR_TIER", None)
    med = np.median(np.array(stages[1:]), axis=0)
    rec = dict(zip(NAMES, (round(float(x), 4) for x in med)))
    rec["wall"] = round(statistics.median(wall[1:]), 3)
    rec["stats"] = st
    return rec, out


def traced(model, num, subset, side):
    """One passes-tier call with the trace line of the transient context caught from stderr."""
    os.environ["ALBEDO_SIMILAR_TIER"] = "passes"
    os.environ["ALBEDO_SIMILAR_TRACE"] = "1"
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            model.similar_np(num, subset, side)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            os.environ.pop("ALBEDO_SIMILAR_TRACE", None)
            os.environ.pop("ALBEDO_SIMILAR_TIER", None)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"rows (\d+) of (\d+) with a direction, context ([\d.]+) ms \(wall\), unit image ([\d.]+) ms, compaction "
                  r"([\d.]+) ms; unseen ms ([\d. ]+); unseen stats ([\d ]+); topk stats ([\d ]+)", text)
    if not m:
        return {"trace": text.strip()}
    ums = [float(x) for x in m.group(6).split()]
    ust = [int(x) for x in m.group(7).split()]
    tst = [int(x) for x in m.group(8).split()]
    return {"rows_with_direction": int(m.group(1)), "rows": int(m.group(2)),
            "transient_context_wall_ms": float(m.group(3)), "unit_image_ms": float(m.group(4)),
            "compaction_ms": float(m.group(5)),
            "unseen_ms": dict(zip(("exclusions", "plan_and_lists", "filter", "exact", "total"), ums)),
            "unseen_stats": dict(zip(("rows", "rows_exact", "entries_removed", "dst_rows_scored"), ust)),
            "topk_stats": dict(zip(("rows_mfma", "rows_rescored", "chunks_scanned", "chunks_full_scan"), tst)),
            "chunks_scanned_over_full": round(tst[2] / tst[3], 4) if tst[3] else None,
            "rows_failing_certification_fraction": round((tst[1] + ust[1]) / max(ust[0], 1), 5)}


def unit_image_np(F):
    s = np.zeros(F.shape[0], np.float32)
    for c in range(F.shape[1]):
        s = s + F[:, c] * F[:, c]
    with np.errstate(all="ignore"):
        return (F / np.sqrt(s)[:, None]).astype(np.float32)


def baseline(model, L, lib, num, subset, repeats):
    """The caller-side route, wall ms by step (medians), and its lists."""
    h = model._h
    steps, out = [], None
    for _ in range(repeats + 1):
        L.check(lib.als_synchronize(h))
        t0 = time.perf_counter()
        ids, F = model.item_factors_np()
        t1 = time.perf_counter()
        U = np.ascontiguousarray(unit_image_np(F))
        t2 = time.perf_counter()
        h2 = C.c_void_p()
        L.check(lib.als_model_create(model.rank, ids.size, L.ptr(ids, C.c_int32), L.ptr(U, C.c_float), ids.size,
                                     L.ptr(ids, C.c_int32), L.ptr(U, C.c_float), -1, C.byref(h2)))
        t3 = time.perf_counter()
        sub = ids if subset is None else np.ascontiguousarray(subset, np.int32)
        src = np.empty(sub.size, np.int32)
        rid = np.empty((sub.size, num + 1), np.int32)
        rsc = np.empty((sub.size, num + 1), np.float32)
        L.check(lib.als_recommend(h2, 0, num + 1, L.ptr(sub, C.c_int32) if subset is not None else None, sub.size,
                                  L.ptr(src, C.c_int32), L.ptr(rid, C.c_int32), L.ptr(rsc, C.c_float)))
        t4 = time.perf_counter()
        own = rid == src[:, None]
        own[~own.any(axis=1), -1] = True                     # self not listed: the last entry goes
        first = np.argmax(own, axis=1)
        keep = np.ones_like(own)
        keep[np.arange(sub.size), first] = False
        out = (rid[keep].reshape(sub.size, num), rsc[keep].reshape(sub.size, num))
        t5 = time.perf_counter()
        lib.als_destroy(h2)
        steps.append([(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t4, t5), (t0, t5))])
    med = np.median(np.array(steps[1:]), axis=0)
    names = ("get_factors", "numpy_normalise", "model_create", "recommend_k_plus_1", "drop_self", "wall")
    return dict(zip(names, (round(float(x), 3) for x in med))), out


def main():
    from query_topk_time import CONFIG_RANK, build_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIG_RANK))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    model, lib, L = build_model(args.config)
    h, num = model._h, 30
    n_users, n_items = int(lib.als_num_rows(h, 0)), int(lib.als_num_rows(h, 1))
    iid, _ = model.item_factors_np()
    uid, _ = model.user_factors_np()
    rng = np.random.default_rng(7)

    item, agree = {}, {}
    counts = [n for n in (1, 16, 1024, 16384) if n < n_items] + [n_items]
    subsets = {n: (None if n == n_items else np.ascontiguousarray(iid[np.sort(rng.choice(n_items, n, replace=False))]))
               for n in counts}
    for n in counts:
        item[n] = {}
        outs = {}
        for tier in ("scan", "passes"):
            item[n][tier], outs[tier] = timed(model, L, lib, num, subsets[n], "item", tier, args.repeats)
        agree[n] = bool(np.array_equal(outs["scan"][1], outs["passes"][1]) and
                        np.array_equal(outs["scan"][2].view(np.uint32), outs["passes"][2].view(np.uint32)))
    cross = None
    for a, b in zip(counts, counts[1:]):
        if item[a]["scan"]["wall"] <= item[a]["passes"]["wall"] and item[b]["scan"]["wall"] > item[b]["passes"]["wall"]:
            cross = [a, b]
    user = {}
    for n in (1024, n_users):
        sub = None if n == n_users else np.ascontiguousarray(uid[np.sort(rng.choice(n_users, n, replace=False))])
        user[n] = {tier: timed(model, L, lib, num, sub, "user", tier, args.repeats)[0] for tier in ("scan", "passes")}

    rebuild = {"item_all": traced(model, num, None, "item"), "item_1024": traced(model, num, subsets[1024], "item"),
               "user_all": traced(model, num, None, "user")}

    base = {}
    for n in (1, n_items):
        b, lists = baseline(model, L, lib, num, subsets[n], args.repeats)
        mine, mine_out = timed(model, L, lib, num, subsets[n], "item", None, args.repeats)
        same_ids = float(np.mean(np.all(lists[0] == mine_out[1], axis=1)))
        base[n] = {"caller_side_ms": b, "als_similar_default_tier": mine,
                   "caller_side_wall_over_als_similar_wall": round(b["wall"] / mine["wall"], 2),
                   "fraction_of_lists_with_equal_ids": round(same_ids, 5)}

    res = {"config": args.config, "rank": model.rank, "users": n_users, "items": n_items, "k": num,
           "repeats": args.repeats, "gpu": "one MI355X (gfx950)",
           "item_side_ms": {str(n): v for n, v in item.items()},
           "tiers_bit_identical": {str(n): v for n, v in agree.items()},
           "item_side_wall_crossover_between_rows": cross,
           "user_side_ms": {str(n): v for n, v in user.items()},
           "passes_tier_rebuild": rebuild,
           "caller_side_baseline": {str(n): v for n, v in base.items()}}
    path = args.out or os.path.join(HERE, "profiles", f"similar_{args.config}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
