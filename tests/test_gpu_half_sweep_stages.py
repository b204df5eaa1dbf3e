"""By-products of a half-sweep: als_last_timings, als_path_stats and als_solver_stats after one item
half and one user half, on every route through sweep_host.cpp's prepare / solve / finish steps.

Data: the 400 x 400 ladder of tests/test_gpu_degree_tiers.py (rows in every degree bucket and in both
tier buckets); either half is solved from injected unit-norm src factors.

Cases: implicit at rank 128 (degree tiers on) and rank 64, explicit stars at regParam 0.1 and 0, and
nonnegative at rank 64 with ALBEDO_SPLIT_CHUNK=64 (every row of degree above 64 is a split-K row).  The
regParam = 0 case runs at rank 1: the ladder has rows of degree 1, and A = sum z^2 over a row's +-1 src
entries is positive definite at that rank only.

Timings.  Cholesky path: the six stage times are consecutive intervals between the events that bound
ALS_T_HALF_TOTAL, so their sum is the total up to the rounding of seven separately measured intervals.
The largest |sum - total| seen on the parent of the commit that added this test, over these cases,
both halves and three runs, was PARENT_WORST = 2.11e-7 ms (half an fp32 ulp of a 4 ms total is 2.4e-7);
the test allows ten times that, SUM_TOL = 2.11e-6 ms.  NNLS path: the eigen stage is exactly 0 and the
two solve stages lie inside the total (the Gram read-back's upload and the column scales are in neither:
sum - total was -0.021 .. -0.023 ms on the parent).
"""
import ctypes as C

import numpy as np
import pytest

from tests import ladder as LD
from tests import test_gpu_degree_tiers as DT
from tests.test_gpu_parity import Ctx

pytestmark = pytest.mark.gpu

PARENT_WORST = 2.11e-7  # ms: three runs of every case on the parent (totals of 0.08 .. 4.1 ms)
SUM_TOL = 10 * PARENT_WORST
T_GRAM, T_EIG, T_ROTATE, T_COMM, T_LIGHT, T_HEAVY, T_TOTAL = range(7)

# name -> (data mode, rank, implicit, regParam, nonnegative)
CASES = {
    "implicit-k128": ("unit", 128, True, 0.1, False),
    "implicit-k64": ("unit", 64, True, 0.1, False),
    "explicit-reg0.1": ("stars", 128, False, 0.1, False),
    "explicit-reg0": ("stars", 1, False, 0.0, False),
    "nnls-k64": ("unit", 64, True, 0.1, True),
}
KNOBS = ("ALBEDO_DEGREE_TIERS", "ALBEDO_SPLIT_CHUNK", "ALBEDO_NNLS_MIN_SLOTS", "ALBEDO_NNLS_ROW", "ALBEDO_NNLS_BATCH_WGS")


def _ctx(gpu_lib, rank, implicit, reg, nonnegative):
    c = Ctx(gpu_lib, rank, implicit=implicit, reg=reg, alpha=40.0)
    if nonnegative:  # Ctx has no switch for it: the same context with nonnegative set
        L = c.L
        p = L.als_params()
        L.check(gpu_lib.als_params_default(C.byref(p)))
        p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative, p.max_iter = rank, int(implicit), reg, 40.0, 1, 1
        L.check(gpu_lib.als_set_params(c.h, C.byref(p)))
    return c


def _i64(c, fn, side):
    out = np.zeros(4, np.int64)
    c.L.check(fn(c.h, side, c.L.ptr(out, C.c_int64)))
    return out.tolist()


def _timings(c, side):
    t = np.full(c.L.ALS_T_COUNT, np.nan)
    c.L.check(c.lib.als_last_timings(c.h, side, c.L.ptr(t, C.c_double), c.L.ALS_T_COUNT))
    return t


@pytest.mark.parametrize("case", list(CASES))
def test_half_sweep_by_products(gpu_lib, monkeypatch, case):
    mode, k, implicit, reg, nonneg = CASES[case]
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if nonneg:
        monkeypatch.setenv("ALBEDO_SPLIT_CHUNK", "64")
    user, item, r, B = DT._data(mode)
    c = _ctx(gpu_lib, k, implicit, reg, nonneg)
    c.ratings(user, item, r)
    KP = 64 if k <= 64 else 128
    for side in (1, 0):
        name = "item" if side else "user"
        c.inject(0, B.user_ids, DT._src(k, len(B.user_ids), k))
        c.inject(1, B.item_ids, DT._src(k, len(B.item_ids), k + 1))
        c.half(side)
        deg, _ = DT._degrees(mode, side)
        t, st, sv = _timings(c, side), _i64(c, gpu_lib.als_path_stats, side), _i64(c, gpu_lib.als_solver_stats, side)
        stage_sum = float(t[T_GRAM:T_TOTAL].sum())
        print(f"HALF_STAGES {case} {name} half: t {np.array2string(t, precision=6)} sum - total "
              f"{stage_sum - t[T_TOTAL]:+.3e} ms, path {st}, solver {sv}")
        assert np.isfinite(t).all() and (t >= 0).all(), (name, t)
        assert st[0] + st[2] == deg.size and st[1] + st[3] == int(deg.sum()), (name, st)
        if nonneg:
            assert t[T_EIG] == 0.0, (name, t)
            assert t[T_LIGHT] + t[T_HEAVY] <= t[T_TOTAL], (name, t)
            assert sv[2] == deg.size and sv[0] >= sv[3] and sv[1] >= 1, (name, sv)
            continue
        assert abs(stage_sum - t[T_TOTAL]) <= SUM_TOL, (name, t, stage_sum - t[T_TOTAL])
        if reg == 0.0:  # forced explicit path: no light rows
            assert st[0] == 0 and st[1] == 0, (name, st)
        else:  # light = within the light limit; at rank 128 the tier rows of degree 65..80 count as heavy
            light = deg <= LD.light_limit(KP, -1)
            assert st == [int(light.sum()), int(deg[light].sum()), int((~light).sum()), int(deg[~light].sum())], (name, st)
            assert ((deg >= 65) & (deg <= 80)).sum() >= 6
        if implicit:
            assert sv[0] >= 1 and sv[1:] == [0, 0, 0], (name, sv)
        else:
            assert sv == [0, 0, 0, 0], (name, sv)
