"""als_audit_rows on the GPU: every row's normal-equation residual against the numpy fp64 restatement of
tests/audit_cases.py.

1. Kernel parity with no solve kernel involved: injected factors on the degree ladder, both sides, every
   padded rank and its edges, three rating modes, the KKT form, with the default chunk and a chunk of 256
   (degrees 255 / 256 / 257 and 511 / 512 / 513 on both sides of one and two chunk edges).  Both sides are
   fp64 and differ in summation order only: |Δeta| <= 1e-10 on the item side (eta < 1e-7), <= 1e-9·eta on
   the user side, where the injected factors solve nothing.
2. Detection: nine item rows with one component 1 % off are exactly the rows above tol = 1e-6, and the
   summary names the worst of them with its degree and solve path.
3. After real half-sweeps: the values agree with the restatement on als_get_factors' own output, a
   freshly solved side has no row above 1e-4·sqrt(rank), a stale side has its median above it.
4. Two ranks sharing the GPU through the host transport agree with the single-process audit.
5. Error codes, and a fork audits like its parent.

Engine backward error: the largest eta of a freshly solved side per solve path, measured by
test_after_half_sweeps on the ladder (mode `varying`, printed per path; the table is in DESIGN.md, "Row
audit"): light16 pairs 9.9e-8, light16 1.2e-7, light32 5.0e-8, light64 3.4e-8, wave / heavy 6.8e-8 (every
row on the wave kernel at rank 128, else 3.5e-8), split-K 2.5e-8, lockstep NNLS 5.5e-8, per-row NNLS
3.4e-8.  The largest is 1.2e-7, so the working tolerance the header recommends is 16 x that, 2e-6; the
1e-4·sqrt(rank) asserted here is the guarantee.  A stale side's median is 2e-2 to 5e-2.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import audit_cases as AC
from tests import ladder as LD
from tests.conftest import ROOT
from tests.test_multi_rank import _free_port

pytestmark = pytest.mark.gpu

PATH_CODE = {"light16-pair": 0, "light16": 1, "light32": 2, "light48": 3, "light64": 4, "light96": 5, "tier80": 6,
             "wave": 7, "heavy": 7, "split": 8}


class Ctx:
    def __init__(self, lib, k, mode, nonneg=False, light=-1, parent=None):
        from albedo_amd import _lib as L
        self.L, self.lib, self.k = L, lib, k
        implicit, alpha, reg = LD.MODES[mode]
        p = L.als_params()
        L.check(lib.als_params_default(C.byref(p)))
        p.rank, p.implicit_prefs, p.reg_param, p.alpha = k, int(implicit), reg, alpha
        p.nonnegative, p.light_max_degree = int(nonneg), light
        self.h = C.c_void_p()
        if parent is None:
            L.check(lib.als_create(C.byref(p), C.byref(self.h)))
        else:
            L.check(lib.als_fork(parent.h, C.byref(p), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.als_destroy(self.h)

    def ratings(self, user, item, r):
        L = self.L
        u, i, r = (np.ascontiguousarray(a, t) for a, t in ((user, np.int32), (item, np.int32), (r, np.float32)))
        L.check(self.lib.als_set_ratings(self.h, u.size, L.ptr(u, C.c_int32), L.ptr(i, C.c_int32), L.ptr(r, C.c_float)))

    def inject(self, side, ids, f):
        L = self.L
        ids, f = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(f, np.float32)
        L.check(self.lib.als_set_initial_factors(self.h, side, ids.size, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float)))

    def half(self, side):
        self.L.check(self.lib.als_half_sweep(self.h, side))

    def factors(self, side):
        L = self.L
        f = np.empty((self.lib.als_num_rows(self.h, side), self.k), np.float32)
        L.check(self.lib.als_get_factors(self.h, side, None, L.ptr(f, C.c_float)))
        return f

    def audit(self, side, tol=AC.TOL):
        L = self.L
        eta = np.full(self.lib.als_num_rows(self.h, side), -1.0)
        a = L.als_audit()
        L.check(self.lib.als_audit_rows(self.h, side, tol, L.ptr(eta, C.c_double), C.byref(a)))
        return eta, a


def _state(lib, mode, k, nonneg=False, light=-1, V=None):
    """A context on the ladder in `mode` holding the injected state (or the given item factors)."""
    user, item, r, B = AC.data(mode)
    U, V0 = AC.injected(mode, k, nonneg)
    c = Ctx(lib, k, mode, nonneg, light)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, U)
    c.inject(1, B.item_ids, V0 if V is None else V)
    return c, B


def _set_audit_chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("ALBEDO_AUDIT_CHUNK", chunk)
    else:
        monkeypatch.delenv("ALBEDO_AUDIT_CHUNK", raising=False)


def _check_summary(a, eta, neg, ids, deg, tol):
    """The summary against the per-row array it was reduced from."""
    assert a.rows == eta.size
    assert a.rows_over == int(np.sum(~(eta <= tol)))
    assert a.non_finite == int(np.sum(~np.isfinite(eta)))
    assert a.negative == int(np.sum(neg))
    w = int(np.argmax(eta))  # the first of equal maxima: the lowest id
    assert a.worst_id == int(ids[w]) and a.worst_degree == int(deg[w]) and a.worst_eta == eta[w]
    assert abs(a.sum_eta - float(np.sum(eta))) <= 1e-12 * float(np.sum(eta))


# ---- 1. kernel parity ----------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [None, "256"], ids=["chunkdefault", "chunk256"])
@pytest.mark.parametrize("case", AC.PARITY_CASES, ids=lambda c: f"{c[0]}-k{c[1]}" + ("-nonneg" if c[2] else ""))
def test_kernel_parity_injected(gpu_lib, monkeypatch, case, chunk):
    mode, k, nonneg = case
    _set_audit_chunk(monkeypatch, chunk)
    c, B = _state(gpu_lib, mode, k, nonneg)
    ref = AC.reference(mode, k, nonneg)
    for side, ids, ptr in ((1, B.item_ids, B.i_ptr), (0, B.user_ids, B.u_ptr)):
        eta, a = c.audit(side)
        want, neg = ref[side]
        d = np.abs(eta - want)
        print(f"AUDIT parity {mode} k{k} nonneg {int(nonneg)} chunk {chunk} side {side}: max |d eta| {d.max():.3e}, "
              f"max eta {eta.max():.3e}")
        assert np.all(np.isfinite(eta))
        if side == 1:
            assert d.max() <= 1e-10
        else:
            assert np.all(d <= 1e-9 * want)
        _check_summary(a, eta, neg, ids, np.diff(ptr), AC.TOL)
        if side == 1:
            assert a.rows_over == 0
    if mode == "mixed":  # the eight item rows without a positive rating: x = 0 and b = 0
        zero = ~AC.injected(mode, k)[1].any(axis=1)
        assert zero.sum() == 8 and np.all(c.audit(1)[0][zero] == 0.0)


# ---- 2. detection ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [x for x in AC.DETECTION_CASES if x[1] != 128], ids=lambda c: f"{c[0]}-k{c[1]}")
def test_detects_perturbed_rows(gpu_lib, monkeypatch, case):
    mode, k, nonneg = case
    _set_audit_chunk(monkeypatch, None)
    B = AC.data(mode)[3]
    rows = AC.perturbed_rows(B)
    c, _ = _state(gpu_lib, mode, k, nonneg, V=AC.perturb(AC.injected(mode, k, nonneg)[1], rows))
    eta, a = c.audit(1)
    want = AC.reference(mode, k, nonneg, perturbed=True)[1][0]
    deg = np.diff(B.i_ptr)
    assert a.rows_over == len(rows)
    assert np.array_equal(np.nonzero(eta > AC.TOL)[0], np.sort(rows))
    w = int(np.argmax(want))
    assert w in rows and a.worst_id == int(B.item_ids[w]) and a.worst_degree == int(deg[w])
    assert abs(a.worst_eta - want[w]) <= 1e-10
    assert a.worst_path == PATH_CODE[LD.path_of(deg[w], LD.padded_rank(k), -1, LD.split_chunk())]


@pytest.mark.parametrize("degree,path", [(33, 3), (65, 6)], ids=["d33-light48", "d65-tier80"])
def test_worst_path_names_the_degree_tiers(gpu_lib, monkeypatch, degree, path):
    """Rank 128 with the default routing has the degree tiers on: D = 48 and D = 80."""
    monkeypatch.delenv("ALBEDO_DEGREE_TIERS", raising=False)
    _set_audit_chunk(monkeypatch, None)
    mode, k = "varying", 128
    B = AC.data(mode)[3]
    row = AC.perturbed_rows(B, (degree,))
    c, _ = _state(gpu_lib, mode, k, V=AC.perturb(AC.injected(mode, k)[1], row))
    eta, a = c.audit(1)
    assert a.rows_over == 1 and np.nonzero(eta > AC.TOL)[0].tolist() == row.tolist()
    assert (a.worst_id, a.worst_degree, a.worst_path) == (int(B.item_ids[row[0]]), degree, path)
    from albedo_amd import _lib as L
    assert (L.ALS_PATH_LIGHT48, L.ALS_PATH_TIER80) == (3, 6)


def test_non_finite_rows_rank_above_all(gpu_lib, monkeypatch):
    """Item rows holding a NaN or an Inf: their eta is not finite, they count in non_finite and in rows_over
    whatever tol is, and the one of lowest id is the worst row, above the perturbed rows' finite values."""
    _set_audit_chunk(monkeypatch, None)
    mode, k = "varying", 50
    B = AC.data(mode)[3]
    V = AC.perturb(AC.injected(mode, k)[1], AC.perturbed_rows(B))
    bad = [40, 11, 29]  # degrees 95 (second copy), 63 and 8 (second copy): none of the perturbed rows
    V[bad[0], 3] = np.nan
    V[bad[1], 0] = np.inf
    V[bad[2], k - 1] = -np.inf
    c, _ = _state(gpu_lib, mode, k, V=V)
    eta, a = c.audit(1, tol=1e300)
    assert np.nonzero(~np.isfinite(eta))[0].tolist() == sorted(bad)
    assert a.non_finite == 3 and a.rows_over == 3
    assert a.worst_id == int(B.item_ids[min(bad)]) and a.worst_degree == int(np.diff(B.i_ptr)[min(bad)])
    assert not np.isfinite(a.worst_eta) and not np.isfinite(a.sum_eta)
    assert c.audit(1)[1].rows_over == 3 + len(AC.PERTURB_DEGREES)


# ---- 3. after real half-sweeps ---------------------------------------------------------------------------

SWEEP_CASES = [(50, -1, None, False), (128, -1, None, False), (128, 0, None, False), (256, -1, "256", False),
               (50, -1, None, True), (256, -1, None, True)]


def _path_names(a_paths):
    from albedo_amd import _lib as L
    return [L.PATH_NAMES[p] for p in a_paths]


@pytest.mark.parametrize("cfg", SWEEP_CASES,
                         ids=lambda c: LD.config_id(c[:3]) + ("-nonneg" if c[3] else ""))
def test_after_half_sweeps(gpu_lib, monkeypatch, cfg):
    k, light, split, nonneg = cfg
    mode = "varying"
    if split:
        monkeypatch.setenv("ALBEDO_SPLIT_CHUNK", split)
    else:
        monkeypatch.delenv("ALBEDO_SPLIT_CHUNK", raising=False)
    _set_audit_chunk(monkeypatch, None)
    user, item, r, B = AC.data(mode)
    U0 = AC.injected(mode, k, nonneg)[0]
    c = Ctx(gpu_lib, k, mode, nonneg, light)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    tol = 1e-4 * np.sqrt(k)
    sides = {0: (B.user_ids, B.u_ptr), 1: (B.item_ids, B.i_ptr)}

    def audit(side, fresh):
        eta, a = c.audit(side, tol)
        want, neg = AC.audit_side(B, side, c.factors(0), c.factors(1), mode, nonneg)
        ids, ptr = sides[side]
        assert np.max(np.abs(eta - want)) <= 1e-10
        _check_summary(a, eta, neg, ids, np.diff(ptr), tol)
        if fresh:
            assert a.rows_over == 0 and a.negative == 0
            # the worst row per solve path: the engine's backward error ("Row audit")
            if not nonneg:
                paths = np.array([LD.path_of(d, LD.padded_rank(k), light, LD.split_chunk(split)) for d in np.diff(ptr)])
                print(f"AUDIT backward error {LD.config_id(cfg[:3])} side {side}: " +
                      ", ".join(f"{p} {eta[paths == p].max():.2e}" for p in sorted(set(paths.tolist()))))
            else:
                print(f"AUDIT backward error nnls k{k} side {side}: max {eta.max():.2e} (path of the worst row "
                      f"{_path_names([a.worst_path])[0]})")
        else:
            print(f"AUDIT stale side {side} k{k}: median eta {np.median(eta):.2e} against tol {tol:.2e}")
            assert np.median(eta) > tol
        return eta

    c.half(1)
    audit(1, True)
    c.half(0)
    audit(0, True)
    audit(1, False)


# ---- 4. two ranks sharing the GPU ------------------------------------------------------------------------

def test_two_ranks_match_single_process(gpu_lib, monkeypatch, tmp_path):
    """Ladder, rank 50, host transport: each rank's values on its own rows equal the single-process audit,
    the other rank's rows are NaN, the row counts add up; then one sweep, and each rank's values against
    the restatement on the gathered factors (the rotation of the own rows and the factor gather with a
    basis that is not the identity)."""
    _set_audit_chunk(monkeypatch, None)
    mode, k, world = "varying", 50, 2
    out = str(tmp_path / "audit")
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "audit_worker.py"), mode, str(k), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    res = [np.load(f"{out}.rank{r}.npz") for r in range(world)]
    c, B = _state(gpu_lib, mode, k)
    for side in (0, 1):
        single = c.audit(side)[0]
        own = [~np.isnan(res[r][f"eta{side}"]) for r in range(world)]
        assert np.all(own[0] ^ own[1])  # every row on exactly one rank
        assert sum(int(res[r][f"rows{side}"]) for r in range(world)) == single.size
        for r in range(world):
            assert int(res[r][f"rows{side}"]) == int(own[r].sum()) > 0
            assert np.max(np.abs(res[r][f"eta{side}"][own[r]] - single[own[r]])) <= 1e-10
    # after a sweep on the ranks: against the restatement on the factors the ranks returned
    U, V = res[0]["U"], res[0]["V"]
    assert np.array_equal(U, res[1]["U"]) and np.array_equal(V, res[1]["V"])
    for side in (0, 1):
        want = AC.audit_side(B, side, U, V, mode)[0]
        for r in range(world):
            got = res[r][f"swept_eta{side}"]
            own = ~np.isnan(got)
            assert own.sum() == int(res[r][f"rows{side}"])
            assert np.max(np.abs(got[own] - want[own])) <= 1e-10


# ---- 5. errors and forks -----------------------------------------------------------------------------------

def _rc(lib, h, side, tol=AC.TOL, out=True):
    from albedo_amd import _lib as L
    a = L.als_audit()
    return lib.als_audit_rows(h, side, tol, None, C.byref(a) if out else None)


def test_model_only_context_is_a_state_error(gpu_lib):
    from albedo_amd import _lib as L
    ids = np.arange(4, dtype=np.int32)
    f = np.ones((4, 3), np.float32)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(3, 4, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float), 4, L.ptr(ids, C.c_int32),
                                     L.ptr(f, C.c_float), -1, C.byref(h)))
    try:
        assert _rc(gpu_lib, h, 0) == L.ALS_E_STATE
    finally:
        gpu_lib.als_destroy(h)


def test_context_without_factors_is_a_state_error(gpu_lib):
    from albedo_amd import _lib as L
    user, item, r, B = AC.data("varying")
    c = Ctx(gpu_lib, 5, "varying")
    assert _rc(gpu_lib, c.h, 1) == L.ALS_E_STATE  # no ratings either
    c.ratings(user, item, r)
    assert _rc(gpu_lib, c.h, 1) == L.ALS_E_STATE
    c.inject(0, B.user_ids, AC.injected("varying", 5)[0])
    assert _rc(gpu_lib, c.h, 1) == L.ALS_E_STATE  # the item side still has none
    with pytest.raises(L.IllegalStateException):
        L.check(_rc(gpu_lib, c.h, 0))


def test_bad_side_and_nan_tol_are_invalid_arguments(gpu_lib):
    from albedo_amd import _lib as L
    c, _ = _state(gpu_lib, "varying", 5)
    assert _rc(gpu_lib, c.h, 2) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, c.h, -1) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, c.h, 1, tol=float("nan")) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, c.h, 1) == L.ALS_OK


def test_null_out_is_an_invalid_argument(gpu_lib):
    from albedo_amd import _lib as L
    c, _ = _state(gpu_lib, "varying", 5)
    assert _rc(gpu_lib, c.h, 1, out=False) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, None, 1) == L.ALS_E_INVALID_ARGUMENT


def test_fork_audits_like_its_parent(gpu_lib, monkeypatch):
    _set_audit_chunk(monkeypatch, None)
    mode, k = "varying", 50
    c, B = _state(gpu_lib, mode, k)
    f = Ctx(gpu_lib, k, mode, parent=c)
    U, V = AC.injected(mode, k)
    f.inject(0, B.user_ids, U)
    f.inject(1, B.item_ids, V)
    for side in (0, 1):
        (e0, a0), (e1, a1) = c.audit(side), f.audit(side)
        assert np.array_equal(e0, e1)
        assert all(getattr(a0, n) == getattr(a1, n) for n, _ in a0._fields_)
    del f


def test_facade_audit(gpu_lib):
    """ALSModel.audit on a fitted model: the dict and the per-row array."""
    from albedo_amd import ALS
    user, item, r, B = AC.data("varying")
    k = 50
    model = ALS(rank=k, maxIter=1, regParam=0.5, alpha=10.0, implicitPrefs=True, seed=3).fit(
        {"user": user, "item": item, "rating": r})
    tol = 1e-4 * np.sqrt(k)
    summary, eta = model.audit(0, tol, per_row=True)  # the user half ran last
    assert summary["rows"] == eta.size == len(B.user_ids) and summary["rows_over"] == 0
    from albedo_amd import _lib as L
    assert summary["worst_path"] in L.PATH_NAMES and summary["worst_id"] in B.user_ids
    assert model.audit(1, tol)["rows_over"] > 0  # the item side is one half behind
