"""The sharded (world > 1) path at the edges of its layout: an empty shard, chpad = 1 with fewer rows than
gather chunks, chunks that are all padding for one rank while the others fill them, chunk tails, and the
sharded top-k / evaluation / prediction calls, against the fp64 oracle and against a single-process
context.  One process per rank on device 0 (tests/shard_worker.py), the cases and the restated layout in
tests/shard_cases.py, their CPU preconditions in tests/test_shard_cases.py.

Every rank saves what it computed, and every check runs on every rank's copy: a stale or misplaced
gathered row shows as one rank's row differing from the others'.

Launches are shared by the tests of one configuration: each runs once and _launch keeps its result.  The
longest launch (ladder, rank 256, world 3) measured MEASURED_LAUNCH_S = 5.4 s of wall time on an MI355X
shared by its ranks, the others 2.7 .. 3.7 s (start of the interpreters and the import of torch included);
LAUNCH_LIMIT_S is about ten times that.  A worker that ends by a signal or reports a GPU fault, or a launch
that runs into its limit, stops every later launch of the module: the remaining tests then fail without
touching the GPU.
"""
import ctypes as C
import functools
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from oracle import cbind
from oracle import spark_als as O
from tests import ladder as LD
from tests import shard_cases as SC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

MEASURED_LAUNCH_S = 5.4   # ladder, rank 256, world 3; the other launches took 2.7 .. 3.7 s
LAUNCH_LIMIT_S = 60.0
TOL_ROWS = 1e-4      # tests/test_gpu_rating_modes.py; the condition cap it rests on: tests/test_shard_cases.py
TOL_NNLS = 1e-3      # tests/test_gpu_nnls_edges.py, tests/test_gpu_rating_modes.py
TOL_GRAM = 1e-6      # tests/test_gpu_gram_eig_edges.py
TOL_ETA = 2e-6       # include/albedo_als.h, als_audit_rows: the recommended working tolerance
ALS_E_STATE, ALS_E_UNSUPPORTED = 3, 8
# a worker that reports one of these met a GPU fault, whatever its exit status
FAULT_MARKS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")

CHOLESKY = [c for c in SC.LAUNCHES if c[4] != "nnls"]
_stopped = []  # why no further launch is started


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_launched = {}  # configuration -> (every rank's arrays, wall seconds), or the message of its failed launch


def _launch(cfg):
    """(every rank's saved arrays, wall seconds) of a configuration, launched once: a failed launch fails
    every test that reads it, with the same message."""
    if cfg not in _launched:
        try:
            _launched[cfg] = _run_workers(cfg)
        except AssertionError as e:
            _launched[cfg] = str(e)
    if isinstance(_launched[cfg], str):
        raise AssertionError(_launched[cfg])
    return _launched[cfg]


def _run_workers(cfg):
    """Starts the `world` workers and polls them: the first non-zero exit kills the rest and fails with that
    rank's output."""
    if _stopped:
        raise AssertionError(f"{SC.launch_id(cfg)}: no launch after {_stopped[0]}")
    case, k, world, chunk, mode = cfg
    tmp = tempfile.mkdtemp(prefix="shard_edges_")
    out = os.path.join(tmp, "w")
    env0 = {key: v for key, v in os.environ.items() if key != "ALBEDO_SPLIT_CHUNK"}
    if chunk:
        env0["ALBEDO_SPLIT_CHUNK"] = chunk
    port = _free_port()
    procs, logs = [], []
    t0 = time.perf_counter()
    try:
        for r in range(world):
            env = dict(env0, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port))
            logs.append(open(os.path.join(tmp, f"log{r}.txt"), "w+b"))
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "shard_worker.py"), case, str(k),
                                           mode, "-1", out], env=env, stdout=logs[-1], stderr=subprocess.STDOUT))

        def tail(r):
            logs[r].flush()
            logs[r].seek(0)
            return logs[r].read().decode(errors="replace")[-3000:]

        failed = None
        while failed is None and any(p.poll() is None for p in procs):
            if time.perf_counter() - t0 > LAUNCH_LIMIT_S:
                _stopped.append(f"{SC.launch_id(cfg)} ran into its limit of {LAUNCH_LIMIT_S:.0f} s")
                failed = ("limit", [r for r, p in enumerate(procs) if p.poll() is None][0])
                break
            failed = next((("exit", r) for r, p in enumerate(procs) if p.poll() not in (None, 0)), None)
            running = [p for p in procs if p.poll() is None]
            if failed is None and running:
                try:
                    running[0].wait(timeout=0.05)
                except subprocess.TimeoutExpired:
                    pass
        if failed is None:
            failed = next((("exit", r) for r, p in enumerate(procs) if p.returncode != 0), None)
        if failed is not None:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            for p in procs:
                p.wait()
            why, r = failed
            rc = procs[r].returncode
            text = tail(r)
            if why == "exit" and (rc in (134, 139, -6, -11) or any(m in text for m in FAULT_MARKS)):
                _stopped.append(f"rank {r} of {SC.launch_id(cfg)} ended with {rc}")
            raise AssertionError(f"{SC.launch_id(cfg)}: rank {r} " +
                                 (f"exited with {rc}" if why == "exit" else "was still running at the limit") +
                                 f":\n{text}")
        wall = time.perf_counter() - t0
        res = []
        for r in range(world):
            with np.load(f"{out}.rank{r}.npz") as f:
                res.append({key: f[key] for key in f.files})
        print(f"SHARD_EDGES launch {SC.launch_id(cfg)}: {wall:.1f} s wall, worker {float(res[0]['t_total']):.1f} s")
        return res, wall
    finally:
        for f in logs:
            f.close()
        shutil.rmtree(tmp, ignore_errors=True)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _refs(cfg):
    """(V_ref, U_ref, V_ref at the new regParam): the oracle's item half from the injected user factors, its
    user half from the ENGINE's item factors, and the item half after als_set_params."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    B, (implicit, alpha, reg) = SC.problem(case, mode)[3:]
    U0 = SC.injected(case, k, mode)[0]
    out = []
    for src, side, rg in ((U0, 1, reg), (res[0]["V"], 0, reg), (U0, 1, SC.NEW_REG)):
        _, ptr, col, val, _ = SC.side_csr(B, side)
        if mode == "nnls":
            X = cbind.solve_rows_nnls(src, O.gram(src), ptr, col, val, reg=rg, alpha=alpha, implicit=implicit)[0]
        else:
            X = cbind.half_sweep(src, ptr, col, val, reg=rg, alpha=alpha, implicit=implicit)
        X.setflags(write=False)
        out.append(X)
    return tuple(out)


def _side_rows(cfg, side):
    """(ids, degrees, labels `path / owner rank / layout chunk`, layout) of a side."""
    case, k, world, chunk, mode = cfg
    B = SC.problem(case, mode)[3]
    ids, ptr = SC.side_csr(B, side)[:2]
    deg = np.diff(ptr)
    lay = SC.layout(case, side, world, mode)
    return ids, deg, SC.row_labels(SC.row_paths(deg, k, mode, chunk), lay), lay


# ---- the solve ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", SC.LAUNCHES, ids=SC.launch_id)
def test_rows_match_the_oracle(gpu_lib, tmp_path, cfg):
    """Every row of both halves, on every rank's copy of the factors, against the fp64 oracle: Cholesky rows
    within 1e-4 (a reference row that is all zero exactly zero), NNLS factors >= 0, within 1e-3 and with
    the same zero pattern on more than 99.5 % of the entries; then the item half after als_set_params
    changed regParam on the sharded context."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    V_ref, U_ref, V_new = _refs(cfg)
    for side, name, key, ref in ((1, "item", "V", V_ref), (0, "user", "U", U_ref), (1, "item-newreg", "newreg_V", V_new)):
        ids, deg, labels, lay = _side_rows(cfg, side)
        X = res[0][key]
        err = LD.row_errors(X, ref, global_scale=mode == "nnls")
        paths = np.array([lb.split("/")[0] for lb in labels])
        owner = np.array([lay.owner(j) for j in range(lay.n)])
        by_path = ", ".join(f"{p} {err[paths == p].max():.2e}" for p in sorted(set(paths.tolist())))
        by_rank = ", ".join(f"r{r} {err[owner == r].max():.2e}" if np.any(owner == r) else f"r{r} -" for r in range(world))
        print(f"SHARD_EDGES {case} k{k} w{world} {mode} chunk {chunk or 'default'} {name}: worst row {err.max():.3e}, "
              f"by path {by_path}, by rank {by_rank}")
        for r in range(world):
            what = f"{name} half on rank {r} [{SC.launch_id(cfg)}]"
            if mode == "nnls":
                Xr = res[r][key]
                assert np.all(Xr >= 0), what
                LD.assert_rows(Xr, ref, ids, deg, labels, TOL_NNLS, what, tmp_path, global_scale=True)
                assert float(np.mean((Xr == 0) == (ref == 0))) > 0.995, what
            else:
                LD.assert_rows(res[r][key], ref, ids, deg, labels, TOL_ROWS, what, tmp_path)


@pytest.mark.parametrize("cfg", SC.LAUNCHES, ids=SC.launch_id)
def test_every_rank_agrees(gpu_lib, cfg):
    """als_get_factors of both sides after each half, every top-k list, every metric and every prediction are
    bit-identical on all ranks (an empty rank included: it joins every gather)."""
    res = _launch(cfg)[0]
    shared = [key for key in res[0] if key.split("_")[0] in ("U", "V", "again", "newreg", "ev", "pred", "refused")
              or (key.startswith(("tk", "ts")) and not key.endswith("_scanned"))]
    assert {"U", "V", "again_U", "again_V", "newreg_V"} <= set(shared)
    if cfg[4] != "nnls":
        assert "pred" in shared and sum(key.startswith("ev_") for key in shared) == 2 * 3 * 4 * 3
        assert sum(key.startswith("tk") for key in shared) == 2 * 5 * 2 and sum(key.startswith("ts") for key in shared) == 2 * 4 * 2 * 3
    for r in range(1, len(res)):
        assert set(shared) <= set(res[r])
        for key in shared:
            assert _same(res[0][key], res[r][key]), f"{SC.launch_id(cfg)}: {key} differs between rank 0 and rank {r}"


@pytest.mark.parametrize("cfg", SC.LAUNCHES, ids=SC.launch_id)
def test_second_sweep_is_bit_identical(gpu_lib, cfg):
    """The same two halves from the same re-injected factors, inside the same processes, give the same bits
    on every rank."""
    for r, f in enumerate(_launch(cfg)[0]):
        assert bool(f["same_V"]) and bool(f["same_U"]), (SC.launch_id(cfg), r, bool(f["same_V"]), bool(f["same_U"]))


# ---- bookkeeping and audit ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", SC.LAUNCHES, ids=SC.launch_id)
def test_bookkeeping(gpu_lib, cfg):
    """als_get_degrees: the true degree on the rows the restated plan gives a rank, -1 elsewhere (all -1 on an
    empty rank); als_path_stats summed over the ranks equals the restated routing of all rows;
    als_get_row_ratings returns the oracle CSR's row at the first / last own row and on the chunk
    boundaries (the inverse of the chunk-major src position) and ALS_E_STATE for another rank's row;
    als_get_gram is the fp64 Gram of the src factors."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    B, (implicit, _, _) = SC.problem(case, mode)[3:]
    U0 = SC.injected(case, k, mode)[0]
    for side in (0, 1):
        ids, ptr, col, val, src_ids = SC.side_csr(B, side)
        deg = np.diff(ptr)
        lay = SC.layout(case, side, world, mode)
        stats = np.zeros(4, np.int64)
        for r in range(world):
            lo, hi = lay.own(r)
            want = np.full(lay.n, -1, np.int64)
            want[lo:hi] = deg[lo:hi]
            assert np.array_equal(res[r][f"deg{side}"], want), (SC.launch_id(cfg), side, r)
            stats += res[r][f"stats{side}"]
            assert res[r][f"rr{side}_rows"].tolist() == lay.probe_rows(r)
            for row in lay.probe_rows(r):
                e0, e1 = ptr[row], ptr[row + 1]
                assert np.array_equal(res[r][f"rr{side}_{row}_ids"], src_ids[col[e0:e1]]), (side, r, row)
                assert np.array_equal(res[r][f"rr{side}_{row}_val"], val[e0:e1]), (side, r, row)
            f = lay.foreign_row(r)
            assert f is not None and int(res[r][f"rr{side}_foreign"]) == f
            assert int(res[r][f"rr{side}_foreign_rc"]) == ALS_E_STATE, (side, r, f)
            if hi == lo:
                assert not np.any(res[r][f"deg{side}"] >= 0) and res[r][f"rr{side}_rows"].size == 0
        assert stats.tolist() == SC.path_stats(deg, SC.row_paths(deg, k, mode, chunk), mode), (SC.launch_id(cfg), side)
        src = U0 if side == 1 else res[0]["V"]
        for r in range(world):
            if not implicit:  # no Gram term: als_get_gram has nothing to return
                assert int(res[r][f"gram_rc{side}"]) == ALS_E_STATE
                continue
            assert int(res[r][f"gram_rc{side}"]) == 0
            G = O.gram(src)
            assert np.max(np.abs(res[r][f"gram{side}"] - G)) <= TOL_GRAM * np.max(np.abs(G)), (SC.launch_id(cfg), side, r)


@pytest.mark.parametrize("cfg", SC.LAUNCHES, ids=SC.launch_id)
def test_audit(gpu_lib, cfg):
    """als_audit_rows right after each half: every own row's eta finite and at most 2e-6, rows of other ranks
    NaN, the `rows` fields adding up to the side's row count (0 on an empty rank)."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    for side in (0, 1):
        ids, deg, labels, lay = _side_rows(cfg, side)
        total = 0
        for r in range(world):
            lo, hi = lay.own(r)
            eta = res[r][f"eta{side}"]
            own = np.zeros(lay.n, bool)
            own[lo:hi] = True
            assert np.all(np.isnan(eta[~own])), (SC.launch_id(cfg), side, r)
            assert int(res[r][f"audit_rows{side}"]) == hi - lo
            total += hi - lo
            if hi > lo:
                w = lo + int(np.argmax(np.where(np.isfinite(eta[lo:hi]), eta[lo:hi], np.inf)))
                print(f"SHARD_EDGES audit {SC.launch_id(cfg)} side {side} rank {r}: worst eta {eta[w]:.3e} ({labels[w]})")
                assert np.all(np.isfinite(eta[own])) and eta[w] <= TOL_ETA, (
                    f"{SC.launch_id(cfg)} side {side} rank {r}: row id {int(ids[w])} degree {int(deg[w])} {labels[w]} "
                    f"eta {eta[w]:.3e}")
                assert int(res[r][f"audit_over{side}"]) == 0
        assert total == lay.n


@pytest.mark.parametrize("cfg", SC.LAUNCHES, ids=SC.launch_id)
def test_refusals(gpu_lib, cfg):
    """als_fork, als_rank_pairs, als_evaluate_pairs and als_fold_in return ALS_E_UNSUPPORTED on every rank."""
    for r, f in enumerate(_launch(cfg)[0]):
        assert f["refused"].tolist() == [ALS_E_UNSUPPORTED] * 4, (SC.launch_id(cfg), r, f["refused"].tolist())


# ---- top-k --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lists(cfg, side, num):
    """O.recommend_for_all of every src row of `side` on the factors the ranks returned."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    B = SC.problem(case, mode)[3]
    f = [res[0]["again_U"], res[0]["again_V"]]
    ids = [B.user_ids, B.item_ids]
    return O.recommend_for_all(ids[side], f[side], ids[1 - side], f[1 - side], num)


def _assert_lists(what, ids, sc, ref_ids, ref_sc):
    real = ~np.isnan(ref_sc)  # -1 is a valid raw id: the NaN score marks the padding
    assert np.array_equal(ids, ref_ids), what
    assert np.array_equal(sc.view(np.uint32)[real], ref_sc.view(np.uint32)[real]), what
    assert np.all(np.isnan(sc[~real])) and np.all(ids[~real] == -1), what


@pytest.mark.parametrize("cfg", CHOLESKY, ids=SC.launch_id)
def test_topk_lists_and_counters(gpu_lib, cfg):
    """als_recommend on both sides with the src rows dealt to the ranks: every list at k = 1, 10, 64, 65
    (the exact scan) and 200 (past n_dst where the side is small) equals O.recommend_for_all in ids and
    score bits, padding is id -1 / score NaN; id subsets (shuffled with repeats and unknown ids: the
    out_pos scatter through the all-gather; one id; fewer known ids than ranks; unknown ids only) give the
    full call's rows, unknown ids an all-padding row, src_ids_out the subset as given.  For k <= 64 each
    rank scanned exactly its rank_slice of the known rows."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    B = SC.problem(case, mode)[3]
    for side in (0, 1):
        ids_side = [B.user_ids, B.item_ids][side]
        n, n_dst = len(ids_side), len([B.item_ids, B.user_ids][side])
        for kk in SC.TOPK_KS:
            ref_ids, ref_sc = _lists(cfg, side, kk)
            assert (kk > n_dst) == bool(np.any(ref_ids[:, -1] == -1) and np.isnan(ref_sc[0, -1]))
            what = f"{SC.launch_id(cfg)} side {side} k {kk}"
            _assert_lists(what, res[0][f"tk{side}_{kk}_ids"], res[0][f"tk{side}_{kk}_sc"], ref_ids, ref_sc)
            if kk <= 64:
                got = [int(res[r][f"tk{side}_{kk}_scanned"]) for r in range(world)]
                want = [SC.rank_slice(n, r, world) for r in range(world)]
                assert got == [hi - lo for _, lo, hi in want] and sum(got) == n, (what, got)
        for name in SC.SUBSETS:
            sub = SC.subset(name, ids_side, world)
            row = np.searchsorted(ids_side, sub)
            known = (row < n) & (ids_side[np.minimum(row, n - 1)] == sub)
            assert {"shuffled": 0 < known.sum() < sub.size, "single": known.all() and sub.size == 1,
                    "few": 0 < known.sum() < world, "unknown": not known.any()}[name], (name, sub)
            for kk in (10, 65):
                what = f"{SC.launch_id(cfg)} side {side} subset {name} k {kk}"
                full_ids, full_sc = _lists(cfg, side, kk)
                ref_ids = np.full((sub.size, kk), -1, np.int32)
                ref_sc = np.full((sub.size, kk), np.nan, np.float32)
                ref_ids[known], ref_sc[known] = full_ids[row[known]], full_sc[row[known]]
                _assert_lists(what, res[0][f"ts{side}_{name}_{kk}_ids"], res[0][f"ts{side}_{name}_{kk}_sc"], ref_ids, ref_sc)
                assert np.array_equal(res[0][f"ts{side}_{name}_{kk}_src"], sub), what
                if kk <= 64:
                    got = [int(res[r][f"ts{side}_{name}_{kk}_scanned"]) for r in range(world)]
                    want = [SC.rank_slice(int(known.sum()), r, world) for r in range(world)]
                    assert got == [hi - lo for _, lo, hi in want], (what, got)


# ---- metrics and predictions ------------------------------------------------------------------------------

class _Model:
    """A single-process model-only context of the factors the ranks returned."""

    def __init__(self, lib, B, U, V):
        from albedo_amd import _lib as L
        self.lib, self.L = lib, L
        uid, iid, U, V = (np.ascontiguousarray(a) for a in (B.user_ids, B.item_ids, U, V))
        self.h = C.c_void_p()
        L.check(lib.als_model_create(U.shape[1], uid.size, L.ptr(uid, C.c_int32), L.ptr(U, C.c_float), iid.size,
                                     L.ptr(iid, C.c_int32), L.ptr(V, C.c_float), -1, C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.als_destroy(self.h)

    def evaluate(self, metric, k, eu, ei, ek):
        L = self.L
        cap = int(np.unique(eu).size)
        mean, nu = C.c_double(-1.0), C.c_int64(-1)
        uo, vo = np.full(cap, 12345, np.int32), np.full(cap, -1.0, np.float64)
        args = (eu.size, L.ptr(eu, C.c_int32), L.ptr(ei, C.c_int32), L.ptr(ek, C.c_int64), C.byref(mean), C.byref(nu),
                L.ptr(uo, C.c_int32), L.ptr(vo, C.c_double), cap)
        L.check(self.lib.als_evaluate_ndcg(self.h, k, *args) if metric < 0
                else self.lib.als_evaluate_ranking(self.h, metric, k, *args))
        return np.float64(mean.value), uo[:nu.value].copy(), vo[:nu.value].copy()

    def predict(self, pu, pi):
        out = np.full(pu.size, -5.0, np.float32)
        self.L.check(self.lib.als_predict(self.h, pu.size, self.L.ptr(pu, C.c_int32), self.L.ptr(pi, C.c_int32),
                                          self.L.ptr(out, C.c_float)))
        return out


@pytest.mark.parametrize("cfg", CHOLESKY, ids=SC.launch_id)
def test_metrics_and_predictions(gpu_lib, cfg):
    """als_evaluate_ndcg / als_evaluate_ranking (NDCG, Precision, MAP) at k = 1, 10, 64, each rank scoring a
    slice of the users and the fp64 values travelling through the float all-gather: user list, per-user
    values and mean bit-identical to a single-process context built from the ranks' factors (also with
    fewer known users than ranks), NDCG per user bit-identical to the oracle's and its mean within 1e-12;
    als_predict bit-identical to O.f2j_sdot, NaN for unknown ids."""
    case, k, world, chunk, mode = cfg
    res = _launch(cfg)[0]
    B = SC.problem(case, mode)[3]
    U, V = res[0]["again_U"], res[0]["again_V"]
    with _Model(gpu_lib, B, U, V) as M:
        for table in SC.EVAL_TABLES:
            eu, ei, ek = SC.eval_table(table, B, world)
            known = np.intersect1d(np.unique(eu), B.user_ids)
            assert (0 < known.size < world) if table == "few" else known.size >= min(40, len(B.user_ids))
            actual = O.into_user_items(eu, ei, ek, 64)
            for kk in SC.EVAL_KS:
                for metric in (-1, 0, 1, 2):
                    tag = f"ev_{table}_{kk}_{'ndcg' if metric < 0 else metric}"
                    what = f"{SC.launch_id(cfg)} {tag}"
                    mean, users, vals = M.evaluate(metric, kk, eu, ei, ek)
                    assert np.array_equal(res[0][tag + "_users"], users) and np.array_equal(users, known), what
                    assert _same(res[0][tag + "_vals"], vals), (what, res[0][tag + "_vals"], vals)
                    assert _same(res[0][tag + "_mean"], mean), (what, float(res[0][tag + "_mean"]), float(mean))
                    if metric > 0:
                        continue
                    pred_ids = _lists(cfg, 0, kk)[0][np.searchsorted(B.user_ids, known)]
                    n = min(kk, len(B.item_ids))
                    pred = {int(u): [int(x) for x in pred_ids[j, :n]] for j, u in enumerate(known)}
                    ref = np.array([O.ndcg_at([(pred[int(u)][:kk], actual[int(u)][:kk])], kk) for u in known])
                    assert np.array_equal(res[0][tag + "_vals"], ref), what
                    ref_mean = O.evaluate_ndcg(pred, {u: a[:kk] for u, a in actual.items()}, kk)
                    assert abs(float(res[0][tag + "_mean"]) - ref_mean) <= 1e-12 * max(1.0, abs(ref_mean)), what
        pu, pi = SC.predict_pairs(B)
        ru, ri = np.searchsorted(B.user_ids, pu), np.searchsorted(B.item_ids, pi)
        ok = (ru < len(B.user_ids)) & (ri < len(B.item_ids))
        ok[ok] = (B.user_ids[ru[ok]] == pu[ok]) & (B.item_ids[ri[ok]] == pi[ok])
        assert ok[:50].all() and not ok[50:].any()
        ref = O.f2j_sdot(U[ru[ok]], V[ri[ok]])
        got = res[0]["pred"]
        assert np.array_equal(got[ok].view(np.uint32), ref.view(np.uint32)), SC.launch_id(cfg)
        assert np.all(np.isnan(got[~ok])), SC.launch_id(cfg)
        assert _same(M.predict(pu, pi)[ok], got[ok])


def test_launches_stay_within_their_limit(gpu_lib):
    """Every launch of the module, its wall time against the limit (the launches are shared with the tests
    above; run alone, this test starts them all)."""
    for cfg in SC.LAUNCHES:
        wall = _launch(cfg)[1]
        print(f"SHARD_EDGES wall {SC.launch_id(cfg)}: {wall:.1f} s")
        assert wall < LAUNCH_LIMIT_S
