"""Worker of tests/test_gpu_shard_edges.py: one process = one rank on device 0; the ranks exchange through
gloo by the engine's host transport (als_comm_init_host), like tests/mp_worker.py and tests/audit_worker.py.
EVERY rank saves what it saw to <out>.rank<r>.npz.

    shard_worker.py <case> <rank k> <mode: cholesky | nnls | explicit> <light_max_degree> <out>

ALBEDO_SPLIT_CHUNK comes from the environment.  The script, in order (tests/shard_cases.py builds every
input): ingest bookkeeping (degrees, rows' ratings at the layout-chunk boundaries, the refusal for another
rank's row); one sweep from injected factors with factors, path stats, audit and Gram after each half; the
same sweep again from the same injected factors (bit-identical?); top-k on both sides at k = 1 .. 200 and on
id subsets, evaluation and prediction (not for NNLS); the calls a sharded context refuses; als_set_params
with another regParam, re-injection and one item half.
"""
import ctypes as C
import datetime
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    case, k, mode, light, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5]
    # a rank whose peer died ends by itself
    dist.init_process_group("gloo", init_method="env://", timeout=datetime.timedelta(seconds=60))
    rank, world = dist.get_rank(), dist.get_world_size()
    from albedo_amd import _lib as L
    from tests import shard_cases as SC
    lib = L.load()
    user, item, r, B, (implicit, alpha, reg) = SC.problem(case, mode)
    U0, V0 = SC.injected(case, k, mode)
    res = {}
    t_start = time.perf_counter()

    def allreduce(_u, buf, n):
        dist.all_reduce(torch.from_numpy(np.ctypeslib.as_array(buf, shape=(n,))))
        return 0

    def allgather(_u, buf, n):
        a = np.ctypeslib.as_array(buf, shape=(world * n,))
        parts = [torch.empty(n, dtype=torch.float32) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(a[rank * n:(rank + 1) * n].copy()))
        for q in range(world):
            a[q * n:(q + 1) * n] = parts[q].numpy()
        return 0

    ar, ag = L.ALLREDUCE_FN(allreduce), L.ALLGATHER_FN(allgather)
    p = L.als_params()
    L.check(lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha = k, int(implicit), reg, alpha
    p.nonnegative, p.light_max_degree = int(mode == "nnls"), light
    h = C.c_void_p()
    L.check(lib.als_create(C.byref(p), C.byref(h)))
    L.check(lib.als_comm_init_host(h, rank, world, ar, ag, None))
    u, i, rr = (np.ascontiguousarray(a) for a in (user, item, r))
    L.check(lib.als_set_ratings(h, u.size, L.ptr(u, C.c_int32), L.ptr(i, C.c_int32), L.ptr(rr, C.c_float)))
    n_side = [int(lib.als_num_rows(h, s)) for s in (0, 1)]
    ids_side = [B.user_ids, B.item_ids]

    def inject():
        for side, f in ((0, U0), (1, V0)):
            ids, f = np.ascontiguousarray(ids_side[side]), np.ascontiguousarray(f)
            L.check(lib.als_set_initial_factors(h, side, ids.size, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float)))

    def factors(side):
        f = np.empty((n_side[side], k), np.float32)
        L.check(lib.als_get_factors(h, side, None, L.ptr(f, C.c_float)))
        return f

    # 1. ingest bookkeeping
    for side in (0, 1):
        deg = np.full(n_side[side], -7, np.int64)
        L.check(lib.als_get_degrees(h, side, L.ptr(deg, C.c_int64)))
        res[f"deg{side}"] = deg
        lay = SC.layout(case, side, world, mode)
        rows = lay.probe_rows(rank)
        res[f"rr{side}_rows"] = np.array(rows, np.int64)
        for row in rows:
            cap = int(SC.side_csr(B, side)[1][-1])
            sid, val, n = np.full(cap, -1, np.int32), np.full(cap, np.nan, np.float32), C.c_int64(-1)
            L.check(lib.als_get_row_ratings(h, side, int(ids_side[side][row]), cap, L.ptr(sid, C.c_int32),
                                            L.ptr(val, C.c_float), C.byref(n)))
            res[f"rr{side}_{row}_ids"], res[f"rr{side}_{row}_val"] = sid[:n.value].copy(), val[:n.value].copy()
        f = lay.foreign_row(rank)
        res[f"rr{side}_foreign"] = np.int64(-1 if f is None else f)
        if f is not None:
            n = C.c_int64(-1)
            res[f"rr{side}_foreign_rc"] = np.int64(lib.als_get_row_ratings(h, side, int(ids_side[side][f]), 0, None, None,
                                                                           C.byref(n)))

    # 2. the first sweep, 3. the same sweep again
    def sweep(tag):
        inject()
        for side, name in ((1, "V"), (0, "U")):
            L.check(lib.als_half_sweep(h, side))
            res[f"{tag}{name}"] = factors(side)
            if tag:
                continue
            st = np.zeros(4, np.int64)
            L.check(lib.als_path_stats(h, side, L.ptr(st, C.c_int64)))
            res[f"stats{side}"] = st
            eta = np.full(n_side[side], -1.0)
            a = L.als_audit()
            L.check(lib.als_audit_rows(h, side, 2e-6, L.ptr(eta, C.c_double), C.byref(a)))
            res[f"eta{side}"], res[f"audit_rows{side}"] = eta, np.int64(a.rows)
            res[f"audit_over{side}"] = np.int64(a.rows_over)
            G = np.full((k, k), np.nan)
            res[f"gram_rc{side}"] = np.int64(lib.als_get_gram(h, 1 - side, L.ptr(G, C.c_double)))
            res[f"gram{side}"] = G  # the Gram of the src side the half of `side` solved from

    sweep("")
    res["t_sweep"] = time.perf_counter() - t_start
    sweep("again_")
    res["same_V"] = np.bool_(np.array_equal(res["V"].view(np.uint32), res["again_V"].view(np.uint32)))
    res["same_U"] = np.bool_(np.array_equal(res["U"].view(np.uint32), res["again_U"].view(np.uint32)))

    # 4. top-k, evaluation, prediction
    if mode != "nnls":
        def topk_delta():
            st = np.zeros(4, np.int64)
            L.check(lib.als_topk_stats(h, L.ptr(st, C.c_int64)))
            d = st[0] - topk_delta.last
            topk_delta.last = st[0]
            return np.int64(d)
        topk_delta.last = 0

        for side in (0, 1):
            n = n_side[side]
            for kk in SC.TOPK_KS:
                ids, sc = np.full((n, kk), -5, np.int32), np.full((n, kk), -5.0, np.float32)
                L.check(lib.als_recommend(h, side, kk, None, n, None, L.ptr(ids, C.c_int32), L.ptr(sc, C.c_float)))
                res[f"tk{side}_{kk}_ids"], res[f"tk{side}_{kk}_sc"] = ids, sc
                res[f"tk{side}_{kk}_scanned"] = topk_delta()  # rows through the MFMA scan: 0 for k > 64
            for name in SC.SUBSETS:
                sub = SC.subset(name, ids_side[side], world)
                for kk in (10, 65):
                    ids, sc = np.full((sub.size, kk), -5, np.int32), np.full((sub.size, kk), -5.0, np.float32)
                    src = np.full(sub.size, -5, np.int32)
                    L.check(lib.als_recommend(h, side, kk, L.ptr(sub, C.c_int32), sub.size, L.ptr(src, C.c_int32),
                                              L.ptr(ids, C.c_int32), L.ptr(sc, C.c_float)))
                    res[f"ts{side}_{name}_{kk}_ids"], res[f"ts{side}_{name}_{kk}_sc"] = ids, sc
                    res[f"ts{side}_{name}_{kk}_src"] = src
                    res[f"ts{side}_{name}_{kk}_scanned"] = topk_delta()
        for table in SC.EVAL_TABLES:
            eu, ei, ek = SC.eval_table(table, B, world)
            cap = int(np.unique(eu).size)
            for kk in SC.EVAL_KS:
                for metric in (-1, L.ALS_METRIC_NDCG, L.ALS_METRIC_PRECISION, L.ALS_METRIC_MAP):
                    mean, nu = C.c_double(-1.0), C.c_int64(-1)
                    uo, vo = np.full(cap, 12345, np.int32), np.full(cap, -1.0, np.float64)
                    args = (eu.size, L.ptr(eu, C.c_int32), L.ptr(ei, C.c_int32), L.ptr(ek, C.c_int64), C.byref(mean),
                            C.byref(nu), L.ptr(uo, C.c_int32), L.ptr(vo, C.c_double), cap)
                    if metric < 0:  # als_evaluate_ndcg itself
                        L.check(lib.als_evaluate_ndcg(h, kk, *args))
                    else:
                        L.check(lib.als_evaluate_ranking(h, metric, kk, *args))
                    tag = f"ev_{table}_{kk}_{'ndcg' if metric < 0 else metric}"
                    res[tag + "_mean"], res[tag + "_users"] = np.float64(mean.value), uo[:nu.value].copy()
                    res[tag + "_vals"] = vo[:nu.value].copy()
        pu, pi = SC.predict_pairs(B)
        pred = np.full(pu.size, -5.0, np.float32)
        L.check(lib.als_predict(h, pu.size, L.ptr(pu, C.c_int32), L.ptr(pi, C.c_int32), L.ptr(pred, C.c_float)))
        res["pred"] = pred

    # 5. calls a sharded context refuses (no exchange: a rank that started one would leave the others waiting)
    one_u, one_i = np.ascontiguousarray(B.user_ids[:1]), np.ascontiguousarray(B.item_ids[:1])
    one_r, one_key = np.ones(1, np.float32), np.zeros(1, np.int64)
    nu, fh, mean = C.c_int64(-1), C.c_void_p(), C.c_double(-1.0)
    res["refused"] = np.array([
        lib.als_fork(h, C.byref(p), C.byref(fh)),
        lib.als_rank_pairs(h, 5, 5, 1, L.ptr(one_u, C.c_int32), L.ptr(one_i, C.c_int32), C.byref(nu), None, None, None,
                           None, 0),
        lib.als_evaluate_pairs(h, L.ALS_METRIC_NDCG, 5, 5, 1, L.ptr(one_u, C.c_int32), L.ptr(one_i, C.c_int32), 1,
                               L.ptr(one_u, C.c_int32), L.ptr(one_i, C.c_int32), L.ptr(one_key, C.c_int64), C.byref(mean),
                               C.byref(nu), None, None, 0),
        lib.als_fold_in(h, 0, None, 1, L.ptr(one_u, C.c_int32), L.ptr(one_i, C.c_int32), L.ptr(one_r, C.c_float), 1,
                        C.byref(nu), None, None, None)], np.int64)

    # 6. als_set_params rebuilds the row layout of the sharded context
    p.reg_param = SC.NEW_REG
    L.check(lib.als_set_params(h, C.byref(p)))
    inject()
    L.check(lib.als_half_sweep(h, 1))
    res["newreg_V"] = factors(1)
    res["t_total"] = time.perf_counter() - t_start
    np.savez(f"{out}.rank{rank}.npz", **res)
    lib.als_destroy(h)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
