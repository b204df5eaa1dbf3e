"""GPU parity of nonnegative = true, per row, at slot, rank, scale and stopping-rule edges.

Every test solves half-sweeps on the device and puts each dst row through tests/nnls_cases.py:check_rows
(x >= 0 and finite; rows whose reference is all zero exactly zero; the KKT residual of the row's own
fp64 system; the row's own distance to the fp64 restatement of Spark's NNLS.solve below 1e-3; a zero
pattern that differs in at most max(1, k // 64) entries) and compares als_solver_stats with the oracle's
per-row iteration counts (check_iterations: within 15 % for the lockstep rows and for the others).  Every
row carries the label of the kernel that solves it (nnls_cases.nnls_path_of), pinned to the engine
through als_path_stats under every ALBEDO_NNLS_MIN_SLOTS value used.

KKT bound (criterion c): MARGIN * max(oracle's worst kkt over the path's rows, the fp32-x floor of those
rows), both from the reference.  Measured on an MI355X over every case of this module (after the fix below): per path the worst device kkt as a multiple of that baseline, the kkt there, the worst per-row
distance to the oracle and the most zero-pattern flips in a row:

  path                 kkt / baseline   kkt       row error   flips
  lockstep-16               4.6         2.7e-07   2.0e-05     1
  lockstep-8                5.7         3.4e-07   5.0e-05     0
  lockstep-4                3.4         3.1e-07   2.9e-06     0
  lockstep-2                5.0         3.6e-07   3.0e-06     0
  lockstep-1                8.7         5.2e-07   9.2e-06     0
  row-64                    5.5         3.4e-07   3.2e-05     0
  row-64-split             15.0         8.9e-07   6.8e-06     0
  row-128                   4.9         2.9e-07   7.2e-05     0
  row-128-split            12.4         7.4e-07   1.1e-05     0
  row-256                   4.8         2.9e-07   6.3e-05     0
  row-256-split             3.9         2.3e-07   3.3e-06     0
  row-256-1024              1.7         2.5e-07   3.6e-06     0
  row-256-1024-split        3.9         2.3e-07   3.7e-06     0

MARGIN = 64 is the smallest power of two that leaves every path 4x headroom (worst 15.0, the split rows
of degree 257 / 513, whose A is summed in fp32 from chunk partials; no path is 100x another).  No row
needed more than the 1e-3 distance or the max(1, k // 64) flips, so neither has a measured exception.

Iterations (device sum / oracle sum over the same rows): lockstep rows 1.00-1.09 at KP 64, 0.93-1.08 at
KP 128, 1.00-1.11 at KP 256, per-row kernels 1.00-1.12 at KP 64, 1.00-1.06 at KP 128, 1.00-1.03 at KP 256,
all inside the 15 % that two correct implementations of this loop keep -- except the cases of
nnls_cases.ITER_MEASURED, whose bound is the measured ratio plus 5 points (measured, not derived):
  aniso-k50, lockstep rows: 2744 against 2281 (1.20; its per-row kernel 1.12, aniso-k128 1.08 / 1.06);
  one 5-star row at rank 50 alone in a launch: 7 against 6 iterations (1.17).
Every row of both passes the KKT criterion at the margin above.  The device forms A·g in fp32 (the
lockstep kernel from G held to 22 bits against one power-of-two scale), so on a G whose entries span four
decades the products lose the conjugacy of the directions sooner than fp64 does, and a row whose stopping
test sits at the rounding of its step takes one iteration more.

Before this suite the ratios reached 1.48 (aniso-k50), 1.28 (regParam 1e-3, alpha 200), 1.19 (alpha = 0,
rank 128; rank 65) and 1.16 (rank 128, plain ladder): every 64 iterations the kernels replace the carried
residual A·x - b by an fp32 A·x, which moves it by the rounding of x and of the product, and kept the
previous direction with its carried A·lastDir and lastDir·A·lastDir.  That direction is not conjugate to
the new residual; a row that was about to stop then ran on for several refreshes (259 iterations against
the oracle's 72 at rank 65, 451 against 170 at alpha = 0).  All four kernels now restart CG at a refresh
(as after a wall hit): 73 against 72 and 171 against 170.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import spark_als as O
from tests import ladder as LD
from tests import nnls_cases as NC
from tests.test_gpu_parity import Ctx, _rel

pytestmark = pytest.mark.gpu

MARGIN = NC.KKT_MARGIN

KNOBS = ("ALBEDO_SPLIT_CHUNK", "ALBEDO_NNLS_MIN_SLOTS", "ALBEDO_NNLS_ROW", "ALBEDO_NNLS_BATCH_WGS")


def _knobs(monkeypatch, chunk=None, min_slots=None, row_kernel=None, wgs=None):
    """The engine's knobs, set before als_set_ratings (rank_layout reads the chunk and the slot floor)."""
    for name, v in zip(KNOBS, (chunk, min_slots, row_kernel, wgs)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return LD.split_chunk(str(chunk) if chunk else str(LD.DEFAULT_SPLIT_CHUNK))


def _ctx(gpu_lib, k, implicit, reg, alpha, max_iter=1):
    from albedo_amd import _lib as L
    c = Ctx(gpu_lib, 8)
    p = L.als_params()
    L.check(gpu_lib.als_params_default(C.byref(p)))
    p.rank, p.implicit_prefs, p.reg_param, p.alpha, p.nonnegative, p.max_iter = k, int(implicit), reg, alpha, 1, max_iter
    h = C.c_void_p()
    L.check(gpu_lib.als_create(C.byref(p), C.byref(h)))
    gpu_lib.als_destroy(c.h)
    c.h, c.rank = h, k
    return c


def _solver(c, side):
    out = np.zeros(4, np.int64)
    c.L.check(c.lib.als_solver_stats(c.h, side, c.L.ptr(out, C.c_int64)))
    return out


def _fmt(v):
    return "-" if v is None else f"{v:.3f}"


def _check_half(c, side, ref, ids_ref, tag, tmp_path, KP, ch, min_slots, row_kernel, expected=True, case=None):
    """One solved half against its reference: path labels pinned to als_path_stats, the per-row check,
    the iteration parity.  Returns (factors, labels, per-path figures)."""
    k = c.rank
    ids, X = c.factors(side)
    assert np.array_equal(ids, ids_ref)
    deg = np.diff(ref.ptr)
    ms = NC.DEFAULT_MIN_SLOTS if min_slots is None else int(min_slots)
    paths = np.array([NC.nnls_path_of(d, KP, ch, ms, row_kernel) for d in deg])
    assert c.stats(side).tolist() == NC.path_stats(deg, paths), (tag, c.stats(side).tolist(), NC.path_stats(deg, paths))
    if expected:
        for p in NC.expected_nnls_paths(KP, ch, ms, int(deg.max()), row_kernel):
            assert np.sum(paths == p) >= 2, (tag, p)
    solver = _solver(c, side)
    want = NC.iteration_sums(ref.it, paths)
    print(f"NNLS_EDGES {tag} KP {KP}: iterations lockstep {solver[3]} / oracle {want[0]}, per-row "
          f"{solver[0] - solver[3]} / oracle {want[1]}, max {solver[1]} / oracle {int(ref.it.max())}")
    kkt = NC.row_kkt(ref, np.nan_to_num(X.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    err = LD.row_errors(np.nan_to_num(X.astype(np.float64)), ref.X)
    flips = ((X == 0) != (ref.X == 0)).sum(axis=1)
    bounds = NC.kkt_bounds(ref, paths, MARGIN)
    for p in sorted(set(paths.tolist())):
        m = paths == p
        print(f"NNLS_EDGES {tag} KP {KP} path {p}: rows {int(m.sum())}, kkt {kkt[m].max():.3e} (oracle "
              f"{ref.kkt[m].max():.3e}, floor {ref.floor[m].max():.3e}, bound {bounds[p]:.3e}), row err "
              f"{err[m].max():.3e}, flips {int(flips[m].max())}, zero rows {int((~ref.X[m].any(axis=1)).sum())}")
    stats = NC.check_rows(X, ref, ids, deg, paths, tag, tmp_path, MARGIN)
    ratios = NC.check_iterations(solver, ref, paths, k, tag, NC.iteration_bounds(case))
    print(f"NNLS_EDGES {tag} KP {KP}: iteration ratios lockstep {_fmt(ratios[0])}, per-row {_fmt(ratios[1])}")
    return X, paths, stats, solver


def _ladder_case(gpu_lib, monkeypatch, tmp_path, tag, *, mode="varying", k, kind="nonneg", params=None, chunk=None,
                 min_slots=None, row_kernel=None, wgs=None, both_halves=False):
    """The NNLS ladder's item half from nnls_cases.src_factors(kind), then (both_halves) the user half
    from the device's own item factors."""
    ch = _knobs(monkeypatch, chunk, min_slots, row_kernel, wgs)
    implicit, alpha, reg = NC.case_params(mode, params)
    KP = LD.padded_rank(k)
    user, item, r, B = NC.ladder_data(mode)
    ref = NC.item_reference(mode, k, kind, params)
    c = _ctx(gpu_lib, k, implicit, reg, alpha)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, ref.src)
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    V, paths, stats, solver = _check_half(c, 1, ref, B.item_ids, f"{tag} item half", tmp_path, KP, ch, min_slots, row_kernel,
                                           case=tag)
    out = dict(item=(ref, V, paths, stats, solver))
    if both_halves:
        c.half(0)
        uref = NC.reference(V, B.u_ptr, B.u_col, B.u_val, reg=reg, alpha=alpha, implicit=implicit)
        out["user"] = (uref,) + _check_half(c, 0, uref, B.user_ids, f"{tag} user half", tmp_path, KP, ch, min_slots, row_kernel)
    return out


# ---- the degree ladder -----------------------------------------------------------------------------

LADDER_CONFIGS = [(50, None), (100, None), (128, None), (256, None), (50, "256"), (128, "256"), (256, "256")]


@pytest.mark.parametrize("k,chunk", LADDER_CONFIGS, ids=[f"k{k}-chunk{c or 'default'}" for k, c in LADDER_CONFIGS])
@pytest.mark.parametrize("mode", list(LD.MODES))
def test_nnls_ladder(gpu_lib, monkeypatch, tmp_path, mode, k, chunk):
    """Item rows on both sides of every lockstep limit, the per-row kernel above it and its prebuilt
    (split-K) form at a chunk of 256, then the user half on the lockstep kernel, in five rating modes."""
    out = _ladder_case(gpu_lib, monkeypatch, tmp_path, f"ladder-{mode}-k{k}-chunk{chunk or 'default'}", mode=mode, k=k,
                       chunk=chunk, both_halves=True)
    if mode == "mixed":
        assert (~out["item"][0].X.any(axis=1)).sum() >= 4  # rows without a positive rating: exactly 0 (check_rows b)


@pytest.mark.parametrize("chunk", [None, "256"], ids=["chunkdefault", "chunk256"])
@pytest.mark.parametrize("mode", list(LD.MODES))
def test_nnls_ladder_rank256_register_kernel(gpu_lib, monkeypatch, tmp_path, mode, chunk):
    """ALBEDO_NNLS_ROW=1024: the 1024-thread register kernel and its prebuilt form at rank 256."""
    out = _ladder_case(gpu_lib, monkeypatch, tmp_path, f"ladder1024-{mode}-chunk{chunk or 'default'}", mode=mode, k=256,
                       chunk=chunk, row_kernel="1024")
    assert "row-256-1024" in out["item"][3] and (chunk is None or "row-256-1024-split" in out["item"][3])


@pytest.mark.parametrize("k", [50, 128, 256])
@pytest.mark.parametrize("min_slots", [4, 1])
def test_nnls_ladder_few_slot_variants(gpu_lib, monkeypatch, tmp_path, k, min_slots):
    """ALBEDO_NNLS_MIN_SLOTS = 4 and 1 open the 4 / 2 / 1-slot variants: every variant that can hold a
    row at this padded rank has at least 2 rows at its limit and 2 one above it on another path, and
    als_path_stats moves with the knob."""
    KP = LD.padded_rank(k)
    out = _ladder_case(gpu_lib, monkeypatch, tmp_path, f"minslots{min_slots}-k{k}", k=k, min_slots=min_slots)
    ref, _, paths, stats, _ = out["item"]
    for sv, (at, above) in NC.boundary_rows(np.diff(ref.ptr), paths, KP, min_slots).items():
        assert at >= 2 and above >= 2, (sv, at, above)
        assert f"lockstep-{sv}" in stats


# ---- row-count edges of a lockstep launch ------------------------------------------------------------

# (k, slots, ALBEDO_NNLS_MIN_SLOTS, degree inside the variant's range); the 1-slot variant holds rows
# at KP = 256 only (at KP 64 and 128 the light limit closes its range)
_ROW_VARIANTS = [(50, 16, None, 5), (50, 8, None, 30), (256, 16, None, 5), (256, 8, None, 10), (256, 1, 1, 60)]
ROW_COUNT_CASES = [(k, sv, ms, d, n, wgs) for k, sv, ms, d in _ROW_VARIANTS
                   for n in sorted({1, sv - 1, sv, sv + 1, 2 * sv + 3} - {0}) for wgs in (None, 1)]


@pytest.mark.parametrize("k,sv,min_slots,d,n,wgs", ROW_COUNT_CASES,
                         ids=[f"k{k}-sv{sv}-n{n}-wgs{w or 'default'}" for k, sv, _, _, n, w in ROW_COUNT_CASES])
def test_nnls_lockstep_row_counts(gpu_lib, monkeypatch, tmp_path, k, sv, min_slots, d, n, wgs):
    """A launch of n rows of one degree on one lockstep variant, n = 1, slots - 1, slots, slots + 1,
    2 slots + 3: idle slots for the whole launch, and the refill taken on the first pass; wgs = 1: one
    workgroup refills through the whole list."""
    ch = _knobs(monkeypatch, None, min_slots, None, wgs)
    KP = LD.padded_rank(k)
    implicit, alpha, reg = LD.MODES["varying"]
    user, item = NC.uniform_degree_coo(n, d)
    r = np.random.default_rng(n + d).choice([0.25, 0.5, 1.0, 2.0, 4.0], user.size).astype(np.float32)
    B = O.make_blocks(user, item, r)
    src = NC.src_factors("nonneg", len(B.user_ids), k)
    ref = NC.reference(src, B.i_ptr, B.i_col, B.i_val, reg=reg, alpha=alpha, implicit=implicit)
    c = _ctx(gpu_lib, k, implicit, reg, alpha)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, src)
    c.inject(1, B.item_ids, np.zeros((n, k), np.float32))
    c.half(1)
    tag = f"rows-k{k}-sv{sv}-n{n}-wgs{wgs or 'default'}"
    _, paths, _, _ = _check_half(c, 1, ref, B.item_ids, tag, tmp_path, KP, ch, min_slots, None, expected=False, case=tag)
    assert set(paths.tolist()) == {f"lockstep-{sv}"} and len(paths) == n


# ---- rank edges --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256])
def test_nnls_rank_edges(gpu_lib, monkeypatch, tmp_path, k):
    """Ranks at and around every padded rank: the pad coordinates (lambda n -> 1, masked by kreal in four
    kernels) must not reach the k returned columns."""
    _ladder_case(gpu_lib, monkeypatch, tmp_path, f"rank-k{k}", k=k)


# ---- active-set extremes, scale, parameters, anisotropy ---------------------------------------------------

@pytest.mark.parametrize("k", [50, 256])
def test_nnls_all_negative_src(gpu_lib, monkeypatch, tmp_path, k):
    """b <= 0 in every row: x = 0 after 0 iterations."""
    ref, V, _, _, solver = _ladder_case(gpu_lib, monkeypatch, tmp_path, f"neg-k{k}", k=k, kind="neg")["item"]
    assert not ref.X.any() and not ref.it.any() and not V.any()
    assert solver[0] == 0 and solver[1] == 0


@pytest.mark.parametrize("k", [50, 256])
def test_nnls_all_positive_src(gpu_lib, monkeypatch, tmp_path, k):
    _ladder_case(gpu_lib, monkeypatch, tmp_path, f"pos-k{k}", k=k, kind="pos")


@pytest.mark.parametrize("k", [50, 128, 256])
@pytest.mark.parametrize("kind", ["small", "large"])
def test_nnls_src_scale(gpu_lib, monkeypatch, tmp_path, kind, k):
    """Src rows of norm 2^-10 and 2^10: Spark's absolute step threshold 1e-7 decides.  At 2^10 the first
    step of every row is below it, so every row is exactly 0 after 0 iterations; at 2^-10 every row
    iterates.  The only inputs that move the lockstep kernel's power-of-two scales off their unit-norm values."""
    ref, V, _, _, solver = _ladder_case(gpu_lib, monkeypatch, tmp_path, f"scale-{kind}-k{k}", k=k, kind=kind)["item"]
    if kind == "large":
        assert not ref.X.any() and not ref.it.any() and not V.any()
        assert solver[0] == 0 and solver[1] == 0
    else:
        assert ref.it.min() >= 1 and ref.X.any(axis=1).all()


PARAM_IDS = [(name, k) for name, (_, _, _, ranks) in NC.PARAM_CASES.items() for k in ranks]


@pytest.mark.parametrize("params,k", PARAM_IDS, ids=[f"{n}-k{k}" for n, k in PARAM_IDS])
def test_nnls_parameter_edges(gpu_lib, monkeypatch, tmp_path, params, k):
    """regParam = 0 (rows that pass several residual refreshes), alpha = 0, and regParam 1e-3 with alpha 200."""
    _ladder_case(gpu_lib, monkeypatch, tmp_path, f"{params}-k{k}", k=k, params=params)


@pytest.mark.parametrize("k", [50, 128, 256])
def test_nnls_anisotropic_gram(gpu_lib, monkeypatch, tmp_path, k):
    """Src columns scaled over two decades, G over four: the lockstep kernel's fp16 hi + lo split of G
    against one global power-of-two scale, next to the per-row kernels' fp32 G."""
    _ladder_case(gpu_lib, monkeypatch, tmp_path, f"aniso-k{k}", k=k, kind="aniso")


# ---- fit ----------------------------------------------------------------------------------------------

def test_nnls_fit_three_sweeps(gpu_lib, monkeypatch, tmp_path):
    """3 full sweeps at rank 128 on the NNLS ladder, whole-matrix (errors compound over the sweeps),
    against oracle.spark_als.fit in its C restatement (nnls_cases.fit_reference, pinned to O.fit by
    tests/test_oracle.py; the numpy loop takes 30 s at this rank)."""
    _knobs(monkeypatch)
    k = 128
    implicit, alpha, reg = LD.MODES["varying"]
    user, item, r, B = NC.ladder_data("varying")
    U0 = NC.src_factors("nonneg", len(B.user_ids), k)
    V0 = NC.src_factors("nonneg", len(B.item_ids), k, seed=77)
    c = _ctx(gpu_lib, k, implicit, reg, alpha, max_iter=3)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, U0)
    c.inject(1, B.item_ids, V0)
    c.L.check(gpu_lib.als_fit(c.h))
    U, V = NC.fit_reference(B, U0, max_iter=3, reg=reg, alpha=alpha, implicit=implicit)
    Ud, Vd = c.factors(0)[1], c.factors(1)[1]
    print(f"NNLS_EDGES fit-k{k}: rel user {_rel(Ud, U):.3e}, item {_rel(Vd, V):.3e}")
    assert np.all(Ud >= 0) and np.all(Vd >= 0)
    assert _rel(Ud, U) < 1e-3 and _rel(Vd, V) < 1e-3
