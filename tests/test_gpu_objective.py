"""als_objective and als_fit_tracked on the GPU, against the numpy fp64 restatement of tests/objective_cases.py.
Every case runs on the degree ladder (about 700 users, 52 item rows, degrees 1..513).

1. Kernel parity on injected factors, no solve kernel involved: three rating modes, both sides of every padded
   rank, both sides of the ratings, with the default chunk (no long rows) and a chunk of 256 on the item side
   (rows of 256 ratings in one piece, 257 as 256 + 1, 511 / 512 in two chunks, 513 in three).  Both sides are
   fp64 and differ in summation order only: every field within 1e-10·abs_terms, every row's loss within 1e-10
   of the row's own absolute terms.
2. Side consistency: the totals through the user and the item CSR agree; a perturbed row's loss is strictly
   larger and every other row's is bit-identical.
3. Monotone: the objective falls after each of 12 alternating half-sweeps, on the push-through, explicit,
   split-K and NNLS paths.
4. Read-only and reproducible.
5. als_fit_tracked: the history is als_objective's total sweep by sweep, the stopping rule, the edges.
6. Error codes.
7. The Python facade.

tests/test_objective_cases.py checks on the CPU what these tests take for granted (the oracle's trajectory
drops by at least 1e-3 per half-sweep, the stopping rule's margin, the size of the perturbed rows' rise).
"""
import ctypes as C

import numpy as np
import pytest

from tests import audit_cases as AC
from tests import ladder as LD
from tests import objective_cases as OC

pytestmark = pytest.mark.gpu

USER, ITEM = 0, 1


class Ctx:
    def __init__(self, lib, k, mode, nonneg=False, light=-1, max_iter=10, parent=None):
        from albedo_amd import _lib as L
        self.L, self.lib, self.k = L, lib, k
        implicit, alpha, reg = LD.MODES[mode]
        p = L.als_params()
        L.check(lib.als_params_default(C.byref(p)))
        p.rank, p.implicit_prefs, p.reg_param, p.alpha = k, int(implicit), reg, alpha
        p.nonnegative, p.light_max_degree, p.max_iter = int(nonneg), light, max_iter
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

    def sweeps(self, n):
        self.L.check(self.lib.als_run_sweeps(self.h, n))

    def fit(self):
        self.L.check(self.lib.als_fit(self.h))

    def factors(self, side):
        L = self.L
        f = np.empty((self.lib.als_num_rows(self.h, side), self.k), np.float32)
        L.check(self.lib.als_get_factors(self.h, side, None, L.ptr(f, C.c_float)))
        return f

    def objective(self, side):
        """(dict of the struct's fields, per-row losses)"""
        L = self.L
        loss = np.full(self.lib.als_num_rows(self.h, side), -1.0)
        o = L.als_objective_t()
        L.check(self.lib.als_objective(self.h, side, L.ptr(loss, C.c_double), C.byref(o)))
        return {n: getattr(o, n) for n, _ in o._fields_}, loss

    def total(self):
        L = self.L
        o = L.als_objective_t()
        L.check(self.lib.als_objective(self.h, USER, None, C.byref(o)))
        return o.total

    def fit_tracked(self, tol, cap):
        """(history buffer of `cap` entries prefilled with -7, n_history, sweeps_run)"""
        L = self.L
        hist = np.full(max(cap, 1), -7.0)
        n, ran = C.c_int32(-1), C.c_int32(-1)
        L.check(self.lib.als_fit_tracked(self.h, tol, cap, L.ptr(hist, C.c_double), C.byref(n), C.byref(ran)))
        return hist, n.value, ran.value


def _ctx(lib, mode, k, U, V, **kw):
    """A context on the ladder in `mode` holding the factors (U, V)."""
    user, item, r, B = AC.data(mode)
    c = Ctx(lib, k, mode, **kw)
    c.ratings(user, item, r)
    c.inject(USER, B.user_ids, U)
    c.inject(ITEM, B.item_ids, V)
    return c, B


def _set_env(monkeypatch, name, value):
    if value:
        monkeypatch.setenv(name, value)
    else:
        monkeypatch.delenv(name, raising=False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _check_against(got, loss, want, what):
    """Every field and every row's loss against the restatement; returns the worst ratio to the 1e-10 bars."""
    bar = OC.PARITY_TOL * want["abs_terms"]  # for abs_terms itself this is 1e-10 relative
    worst = 0.0
    for f in OC.FIELDS:
        d = abs(got[f] - want[f])
        worst = max(worst, d / bar)
        assert d <= bar, f"{what}: {f} {got[f]!r} against {want[f]!r}"
    assert got["n_ratings"] == want["n_ratings"] and got["rows"] == want["rows"]
    assert np.all(np.isfinite(loss))
    d = np.abs(loss - want["loss"])
    bar = OC.PARITY_TOL * want["abs_row"]
    assert np.all(d <= bar), f"{what}: {int(np.sum(d > bar))} rows' losses are off, worst {np.max(d / want['abs_row']):.3e}"
    nz = want["abs_row"] > 0
    if nz.any():
        worst = max(worst, float(np.max(d[nz] / bar[nz])))
    return worst


# ---- 1. kernel parity ----------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [None, "256"], ids=["chunkdefault", "chunk256"])
@pytest.mark.parametrize("case", OC.PARITY_CASES, ids=lambda c: f"{c[0]}-k{c[1]}")
def test_kernel_parity_injected(gpu_lib, monkeypatch, case, chunk):
    mode, k = case
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", chunk)
    U, V = AC.injected(mode, k)
    c, B = _ctx(gpu_lib, mode, k, U, V)
    ref = OC.reference(mode, k)
    for side in ((ITEM,) if chunk else (ITEM, USER)):  # the long rows are item rows
        got, loss = c.objective(side)
        worst = _check_against(got, loss, ref[side], f"{mode} k{k} chunk {chunk} side {side}")
        print(f"OBJECTIVE parity {mode} k{k} chunk {chunk} side {side}: worst difference {worst:.3e} of the 1e-10 bar, "
              f"total {got['total']:.9e}, abs_terms / total {got['abs_terms'] / abs(got['total']):.2f}")
    if chunk:  # the chunk moves the result by rounding only, and the rows it does not cut not at all
        monkeypatch.delenv("ALBEDO_OBJECTIVE_CHUNK")
        whole, loss0 = c.objective(ITEM)
        assert abs(whole["total"] - got["total"]) <= OC.PARITY_TOL * got["abs_terms"]
        deg = np.diff(B.i_ptr)
        assert np.array_equal(loss[deg <= 256], loss0[deg <= 256])


# ---- 2. side consistency -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", OC.PARITY_CASES[::3], ids=lambda c: f"{c[0]}-k{c[1]}")
def test_sides_agree(gpu_lib, monkeypatch, case):
    mode, k = case
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    c, _ = _ctx(gpu_lib, mode, k, *AC.injected(mode, k))
    u, i = c.objective(USER)[0], c.objective(ITEM)[0]
    bar = OC.PARITY_TOL * u["abs_terms"]
    assert abs(u["total"] - i["total"]) <= bar
    assert abs(u["sse"] - i["sse"]) <= bar and abs(u["ratings"] - i["ratings"]) <= bar
    assert abs(u["reg_side"] - i["reg_other"]) <= bar and abs(u["reg_other"] - i["reg_side"]) <= bar
    assert u["n_ratings"] == i["n_ratings"]


@pytest.mark.parametrize("case", OC.PERTURB_CASES, ids=lambda c: f"{c[0]}-k{c[1]}")
def test_perturbed_rows_cost_more(gpu_lib, monkeypatch, case):
    mode, k = case
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    U, V = AC.injected(mode, k)
    B = AC.data(mode)[3]
    rows = AC.perturbed_rows(B)
    c0, _ = _ctx(gpu_lib, mode, k, U, V)
    c1, _ = _ctx(gpu_lib, mode, k, U, AC.perturb(V, rows))
    (o0, l0), (o1, l1) = c0.objective(ITEM), c1.objective(ITEM)
    assert np.all(l1[rows] > l0[rows])
    others = np.setdiff1d(np.arange(l0.size), rows)
    assert np.array_equal(l1[others], l0[others])
    assert o1["total"] > o0["total"]
    _check_against(o1, l1, OC.reference(mode, k, perturbed=True)[ITEM], f"perturbed {mode} k{k}")


# ---- 3. monotone -----------------------------------------------------------------------------------------

# (mode, rank, nonnegative, light_max_degree, ALBEDO_SPLIT_CHUNK)
MONOTONE = ([(m, k, n, -1, None) for m, k, n in OC.TRAJECTORY_CASES] +
            [(m, k, n, light, split) for m, k, n in OC.TRAJECTORY_CASES if k == 50
             for light, split in ((0, None), (-1, "256"))])


@pytest.mark.parametrize("cfg", MONOTONE, ids=lambda c: f"{c[0]}-" + LD.config_id(c[1:2] + c[3:]) + ("-nonneg" if c[2] else ""))
def test_objective_falls_every_half_sweep(gpu_lib, monkeypatch, cfg):
    mode, k, nonneg, light, split = cfg
    _set_env(monkeypatch, "ALBEDO_SPLIT_CHUNK", split)
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    c, _ = _ctx(gpu_lib, mode, k, *OC.start(mode, k, nonneg), nonneg=nonneg, light=light)
    traj = [c.total()]
    for h in range(OC.HALF_SWEEPS):
        c.half(ITEM if h % 2 == 0 else USER)
        traj.append(c.total())
    want = OC.oracle_trajectory(mode, k, nonneg)
    rel = [abs(a - b) / abs(b) for a, b in zip(traj, want)]
    print(f"OBJECTIVE trajectory {mode} k{k} nonneg {int(nonneg)} light {light} split {split}: engine " +
          " ".join(f"{v:.9e}" for v in traj) + f"; largest relative distance from the oracle's {max(rel):.2e}")
    assert np.all(np.isfinite(traj))
    for h in range(OC.HALF_SWEEPS):
        assert traj[h + 1] < traj[h], f"half-sweep {h + 1}: {traj[h]!r} -> {traj[h + 1]!r}"


# ---- 4. read-only and reproducible -------------------------------------------------------------------------

def _observables(c):
    L, lib = c.L, c.lib
    out = [_bits(c.factors(USER)), _bits(c.factors(ITEM))]
    for side in (USER, ITEM):
        g = np.zeros((c.k, c.k))
        L.check(lib.als_get_gram(c.h, side, L.ptr(g, C.c_double)))
        t = np.zeros(L.ALS_T_COUNT)
        L.check(lib.als_last_timings(c.h, side, L.ptr(t, C.c_double), t.size))
        s = np.zeros(4, np.int64)
        L.check(lib.als_path_stats(c.h, side, L.ptr(s, C.c_int64)))
        out += [_bits(g), _bits(t), _bits(s)]
    s = np.zeros(4, np.int64)
    L.check(lib.als_topk_stats(c.h, L.ptr(s, C.c_int64)))
    return out + [_bits(s)]


@pytest.mark.parametrize("chunk", [None, "256"], ids=["chunkdefault", "chunk256"])
def test_read_only_and_reproducible(gpu_lib, monkeypatch, chunk):
    mode, k = "varying", 50
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", chunk)
    U, V = OC.start(mode, k)
    a, _ = _ctx(gpu_lib, mode, k, U, V)
    b, _ = _ctx(gpu_lib, mode, k, U, V)
    for c in (a, b):
        c.half(ITEM)
        c.half(USER)
    before = _observables(a)
    first = [a.objective(side) for side in (USER, ITEM)]
    again = [a.objective(side) for side in (USER, ITEM)]
    for (o0, l0), (o1, l1) in zip(first, again):
        assert o0 == o1 and _bits(l0) == _bits(l1)
    assert _observables(a) == before
    # a call between two half-sweeps leaves the fit bit-identical
    for side in (ITEM, USER):
        a.objective(USER)
        a.objective(ITEM)
        a.half(side)
        b.half(side)
        assert _bits(a.factors(side)) == _bits(b.factors(side))


def test_non_finite_factors_are_not_an_error(gpu_lib, monkeypatch):
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    mode, k = "varying", 5
    U, V = AC.injected(mode, k)
    W = np.array(V)
    W[3, 1] = np.nan
    c, B = _ctx(gpu_lib, mode, k, U, W)
    o, loss = c.objective(ITEM)
    assert not np.isfinite(o["total"]) and not np.isfinite(loss[3])
    assert np.all(np.isfinite(np.delete(loss, 3)))
    assert o["n_ratings"] == int(B.i_ptr[-1])


# ---- 5. tracked fit ------------------------------------------------------------------------------------------

def test_history_is_the_objective_sweep_by_sweep(gpu_lib, monkeypatch):
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    mode, k, iters = "varying", 50, 4
    U, V = OC.start(mode, k)
    a, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=iters)
    hist, n, ran = a.fit_tracked(0.0, iters + 1)
    assert (n, ran) == (iters + 1, iters)
    b, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=iters)
    want = [b.total()]
    for _ in range(iters):
        b.sweeps(1)
        want.append(b.total())
    assert _bits(hist[:n]) == _bits(np.array(want))
    assert np.all(np.diff(hist[:n]) < 0)
    f, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=iters)
    f.fit()
    for side in (USER, ITEM):
        assert _bits(a.factors(side)) == _bits(f.factors(side)) == _bits(b.factors(side))
    # a NaN tol runs every sweep too
    d, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=iters)
    hist2, n2, ran2 = d.fit_tracked(float("nan"), iters + 1)
    assert (n2, ran2) == (n, ran) and _bits(hist2) == _bits(hist)


@pytest.mark.parametrize("case", OC.STOP_CASES, ids=lambda c: f"{c[0]}-k{c[1]}")
def test_tolerance_stops_the_fit(gpu_lib, monkeypatch, case):
    mode, k = case
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    U, V = OC.start(mode, k)
    tol = OC.stop_tol(mode, k)
    a, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=8)
    hist, n, ran = a.fit_tracked(tol, 9)
    print(f"OBJECTIVE stop {mode} k{k}: tol {tol:.3e}, engine decreases " + " ".join(f"{v:.3e}" for v in
          (hist[:n - 1] - hist[1:n]) / np.abs(hist[:n - 1])))
    assert ran == OC.STOP_SWEEP and n == OC.STOP_SWEEP + 1
    assert np.all(hist[n:] == -7.0)
    f, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=OC.STOP_SWEEP)
    f.fit()
    for side in (USER, ITEM):
        assert _bits(a.factors(side)) == _bits(f.factors(side))


def test_tracked_fit_edges(gpu_lib, monkeypatch):
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    mode, k = "varying", 5
    U, V = OC.start(mode, k)
    # max_iter = 0: the start alone
    a, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=0)
    hist, n, ran = a.fit_tracked(0.0, 1)
    assert (n, ran) == (1, 0) and hist[0] == a.total()
    # cap too small: the counts are set, nothing is written
    b, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=3)
    hist, n, ran = b.fit_tracked(0.0, 3)
    assert (n, ran) == (4, 3) and np.all(hist == -7.0)
    # a null history
    L = b.L
    c, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=3)
    n2, ran2 = C.c_int32(-1), C.c_int32(-1)
    L.check(gpu_lib.als_fit_tracked(c.h, 0.0, 0, None, C.byref(n2), C.byref(ran2)))
    assert (n2.value, ran2.value) == (4, 3)
    assert _bits(c.factors(ITEM)) == _bits(b.factors(ITEM))
    assert gpu_lib.als_fit_tracked(c.h, 0.0, 0, None, None, C.byref(ran2)) == L.ALS_E_INVALID_ARGUMENT
    assert gpu_lib.als_fit_tracked(c.h, 0.0, 0, None, C.byref(n2), None) == L.ALS_E_INVALID_ARGUMENT


def test_fork_tracks_like_its_parent(gpu_lib, monkeypatch):
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    mode, k, iters = "varying", 50, 3
    U, V = OC.start(mode, k)
    p, B = _ctx(gpu_lib, mode, k, U, V, max_iter=iters)
    f = Ctx(gpu_lib, k, mode, max_iter=iters, parent=p)
    f.inject(USER, B.user_ids, U)
    f.inject(ITEM, B.item_ids, V)
    (o0, l0), (o1, l1) = p.objective(ITEM), f.objective(ITEM)
    assert o0 == o1 and _bits(l0) == _bits(l1)
    hf, nf, rf = f.fit_tracked(0.0, iters + 1)
    s, _ = _ctx(gpu_lib, mode, k, U, V, max_iter=iters)  # a context of its own
    hp, np_, rp = s.fit_tracked(0.0, iters + 1)
    assert (nf, rf) == (np_, rp) == (iters + 1, iters) and _bits(hf) == _bits(hp)
    del f


# ---- 6. errors -----------------------------------------------------------------------------------------------

def _rc(lib, h, side, out=True):
    from albedo_amd import _lib as L
    o = L.als_objective_t()
    return lib.als_objective(h, side, None, C.byref(o) if out else None)


def test_model_only_context_is_a_state_error(gpu_lib):
    from albedo_amd import _lib as L
    ids = np.arange(4, dtype=np.int32)
    f = np.ones((4, 3), np.float32)
    h = C.c_void_p()
    L.check(gpu_lib.als_model_create(3, 4, L.ptr(ids, C.c_int32), L.ptr(f, C.c_float), 4, L.ptr(ids, C.c_int32),
                                     L.ptr(f, C.c_float), -1, C.byref(h)))
    try:
        assert _rc(gpu_lib, h, USER) == L.ALS_E_STATE
    finally:
        gpu_lib.als_destroy(h)


def test_context_without_factors_is_a_state_error(gpu_lib):
    from albedo_amd import _lib as L
    user, item, r, B = AC.data("varying")
    c = Ctx(gpu_lib, 5, "varying")
    assert _rc(gpu_lib, c.h, ITEM) == L.ALS_E_STATE  # no ratings either
    c.ratings(user, item, r)
    assert _rc(gpu_lib, c.h, ITEM) == L.ALS_E_STATE
    c.inject(USER, B.user_ids, AC.injected("varying", 5)[0])
    assert _rc(gpu_lib, c.h, ITEM) == L.ALS_E_STATE  # the item side still has none
    with pytest.raises(L.IllegalStateException):
        L.check(_rc(gpu_lib, c.h, USER))


def test_bad_side_and_null_out_are_invalid_arguments(gpu_lib):
    from albedo_amd import _lib as L
    c, _ = _ctx(gpu_lib, "varying", 5, *AC.injected("varying", 5))
    assert _rc(gpu_lib, c.h, 2) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, c.h, -1) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, c.h, ITEM, out=False) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, None, ITEM) == L.ALS_E_INVALID_ARGUMENT
    assert _rc(gpu_lib, c.h, ITEM) == L.ALS_OK
    t = np.full(3, -1.0)
    L.check(gpu_lib.als_objective_timing(c.h, L.ptr(t, C.c_double)))
    assert np.all(t >= 0) and t[2] >= t[1] > 0


# ---- 7. the Python facade ------------------------------------------------------------------------------------

def _als(mode, k, **kw):
    from albedo_amd import ALS
    implicit, alpha, reg = LD.MODES[mode]
    return ALS(rank=k, regParam=reg, alpha=alpha, implicitPrefs=implicit, seed=3, **kw)


def test_facade_objective_and_tracking(gpu_lib, monkeypatch, tmp_path):
    from albedo_amd import ALSModel
    from albedo_amd import _lib as L
    _set_env(monkeypatch, "ALBEDO_OBJECTIVE_CHUNK", None)
    mode, k = "varying", 50
    user, item, r, B = AC.data(mode)
    data = {"user": user, "item": item, "rating": r}
    U, V = OC.start(mode, k)
    init = dict(initialUserFactors=(B.user_ids, U), initialItemFactors=(B.item_ids, V))
    # objective against the restatement on the model's own factors
    model = _als(mode, k, maxIter=3).fit(data, trackObjective=True, **init)
    assert model.sweepsRun == 3 and len(model.objectiveHistory) == 4
    assert all(isinstance(v, float) for v in model.objectiveHistory)
    assert np.all(np.diff(model.objectiveHistory) < 0)
    for side, name in ((USER, "user"), (ITEM, "item")):
        o, loss = model.objective(name, per_row=True)
        want = OC.objective_side(B, side, model.user_factors_np()[1], model.item_factors_np()[1], mode)
        _check_against(o, loss, want, f"facade {name}")
        assert o["rmse"] == np.sqrt(o["sse"] / o["n_ratings"])
    assert model.objective()["total"] == model.objectiveHistory[-1]
    t = model.objective_timing()
    assert set(t) == {"gram", "rows", "total"} and t["total"] > 0
    # tol stops the fit where the oracle says
    stopped = _als(mode, k, maxIter=8).fit(data, tol=OC.stop_tol(mode, k), **init)
    assert stopped.sweepsRun == OC.STOP_SWEEP and len(stopped.objectiveHistory) == OC.STOP_SWEEP + 1
    # an untracked fit is today's
    plain = _als(mode, k, maxIter=3).fit(data, **init)
    assert plain.objectiveHistory is None and plain.sweepsRun is None
    assert np.array_equal(plain.user_factors_np()[1], model.user_factors_np()[1])
    # a grid: every fork is tracked, each history equal to its standalone fit's
    maps = [{"regParam": 0.5}, {"regParam": 0.25}]
    est = _als(mode, 5, maxIter=2)
    grid = est.fit(data, maps, trackObjective=True)
    for m, pm in zip(grid, maps):
        alone = est.fit(data, pm, trackObjective=True)
        assert m.sweepsRun == alone.sweepsRun == 2 and m.objectiveHistory == alone.objectiveHistory
        with pytest.raises(L.IllegalStateException):
            m.objective()  # a snapshot holds no ratings
    assert grid[0].objectiveHistory != grid[1].objectiveHistory
    # a loaded model holds no ratings
    path = str(tmp_path / "model")
    model.save(path)
    with pytest.raises(L.IllegalStateException):
        ALSModel.load(path).objective()
