"""Worker of tests/test_gpu_audit.py::test_two_ranks_match_single_process: one process = one rank, the
ranks share device 0 and exchange through gloo by the engine's host transport (als_comm_init_host), like
tests/mp_worker.py.  Every rank audits both sides of the injected ladder state, then runs one sweep, audits
again and fetches the factors; it saves its per-row values, row counts and the factors to <out>.rank<r>.npz.

    audit_worker.py <mode> <rank k> <out>
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    mode, k, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo", init_method="env://")
    rank, world = dist.get_rank(), dist.get_world_size()
    from albedo_amd import _lib as L
    from tests import audit_cases as AC
    from tests import ladder as LD
    lib = L.load()
    user, item, r, B = AC.data(mode)
    U, V = AC.injected(mode, k)
    implicit, alpha, reg = LD.MODES[mode]

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
    h = C.c_void_p()
    L.check(lib.als_create(C.byref(p), C.byref(h)))
    L.check(lib.als_comm_init_host(h, rank, world, ar, ag, None))
    u, i, rr = (np.ascontiguousarray(a) for a in (user, item, r))
    L.check(lib.als_set_ratings(h, u.size, L.ptr(u, C.c_int32), L.ptr(i, C.c_int32), L.ptr(rr, C.c_float)))
    for side, ids, f in ((0, B.user_ids, U), (1, B.item_ids, V)):
        ids, f = np.ascontiguousarray(ids), np.ascontiguousarray(f)
        L.check(lib.als_set_initial_factors(h, side, ids.size, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float)))

    res = {}

    def audit(prefix):
        for side in (0, 1):
            eta = np.full(lib.als_num_rows(h, side), -1.0)
            a = L.als_audit()
            L.check(lib.als_audit_rows(h, side, AC.TOL, L.ptr(eta, C.c_double), C.byref(a)))
            res[f"{prefix}eta{side}"] = eta
            res[f"rows{side}"] = np.int64(a.rows)

    audit("")
    L.check(lib.als_half_sweep(h, 1))
    L.check(lib.als_half_sweep(h, 0))
    audit("swept_")
    for side, name in ((0, "U"), (1, "V")):
        f = np.empty((lib.als_num_rows(h, side), k), np.float32)
        L.check(lib.als_get_factors(h, side, None, L.ptr(f, C.c_float)))
        res[name] = f
    np.savez(f"{out}.rank{rank}.npz", **res)
    lib.als_destroy(h)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
