"""CPU preconditions of tests/test_gpu_shard_edges.py: the cases of tests/shard_cases.py reach the layout
edges they claim, the test-side restatement of the shard plan and of the gathered layout agrees with the
engine's planner and is self-consistent, every row's normal equation is well enough conditioned for the
1e-4 per-row tolerance, and the C oracle solving each rank's rows through the restated padded layout
reproduces the single-process half-sweep (the `cpu` mode of tests/mp_worker.py, in-process, on the three
cases)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cbind
from oracle import spark_als as O
from tests import ladder as LD
from tests import shard_cases as SC

WORLDS = (2, 3, 4)
# (case, mode) pairs and the (case, rank, mode) of the Cholesky launches
CASE_MODES = sorted({(c, m) for c, _, _, _, m in SC.LAUNCHES})
CHOLESKY_RANKS = sorted({(c, k, m) for c, k, _, _, m in SC.LAUNCHES if m != "nnls"})


@pytest.mark.parametrize("case,mode", CASE_MODES)
def test_restated_plan_is_the_engines(case, mode):
    """plan_shards restated in numpy equals als_host_plan_shards for every case, side and world used."""
    from albedo_amd import _lib as L
    lib = L.load()
    B = SC.problem(case, mode)[3]
    for side in (0, 1):
        ptr = np.ascontiguousarray(SC.side_csr(B, side)[1], np.int64)
        for world in WORLDS:
            starts = np.empty(world + 1, np.int64)
            L.check(lib.als_host_plan_shards(L.ptr(ptr, C.c_int64), len(ptr) - 1, world, L.ptr(starts, C.c_int64)))
            assert SC.plan_shards(ptr, world).tolist() == starts.tolist(), (case, side, world)


def test_launch_matrix_covers_the_plans():
    """Every (case, world) the edge claims below speak of is launched."""
    have = {(c, w) for c, _, w, _, _ in SC.LAUNCHES}
    assert {("ladder", 2), ("ladder", 3), ("ladder", 4), ("skew", 3), ("skew", 4), ("tiny", 2), ("tiny", 3),
            ("tiny", 4)} <= have


def test_ladder_edges():
    """Item side: world 2 even shards; world 3 a last rank of 5 rows in one layout chunk (three all-padding
    chunks beside full ones), holding only wave / split rows; world 4 two ranks of 3 rows.  At a split chunk
    of 256 every path a rank is meant to reach has rows, and at world 2 and 3 every light bucket lies on at
    least two ranks."""
    B = SC.problem("ladder")[3]
    deg = np.diff(B.i_ptr)
    assert len(B.item_ids) == 52 and len(B.user_ids) == 700
    w2, w3, w4 = (SC.layout("ladder", 1, w) for w in WORLDS)
    assert w2.rows.tolist() == [26, 26] and w2.chpad == 7
    assert w3.rows.tolist() == [24, 23, 5] and w3.chpad == 6
    assert [w3.chunks_used(r) for r in range(3)] == [4, 4, 1]
    assert w4.rows.tolist() == [23, 3, 23, 3]
    u3 = SC.layout("ladder", 0, 3)
    assert u3.rows.tolist() == [232, 238, 230] and u3.chpad == 60
    for k in (50, 128, 256):
        KP = LD.padded_rank(k)
        paths = np.array([LD.path_of(d, KP, -1, 256) for d in deg])
        want = LD.expected_paths(KP, -1, 256, int(deg.max()))
        assert set(want) == set(paths.tolist()), (k, want)
        lo, hi = w3.own(2)
        assert set(paths[lo:hi].tolist()) <= {"wave", "heavy", "split"}
        for lay in (w2, w3):
            for p in want:
                if p.startswith("light"):
                    ranks = {lay.owner(i) for i in np.nonzero(paths == p)[0]}
                    assert len(ranks) >= 2, (k, lay.world, p, ranks)


@pytest.mark.parametrize("mode", ["cholesky", "explicit"])
def test_skew_edges(mode):
    """One item holds more than half of the ratings, so rank 1 owns no item row at world 3 and 4, while the
    user side stays balanced; sparse ids with negatives on both sides."""
    user, item, r, B, _ = SC.problem("skew", mode)
    ideg, udeg = np.diff(B.i_ptr), np.diff(B.u_ptr)
    assert len(B.user_ids) == 1500 and len(B.item_ids) == 160 and B.user_ids[0] < 0 and B.item_ids[0] < 0
    assert ideg[0] == 1500 and 1 <= ideg[1:].min() and ideg[1:].max() <= 7 and ideg[1:].sum() < 700
    assert udeg.min() == 1 and udeg.max() == 5
    for world in (3, 4):
        lay = SC.layout("skew", 1, world, mode)
        assert lay.rows[0] == 1 and lay.rows[1] == 0, lay.starts  # rank 1 is empty
        assert lay.chunks_used(1) == 0 and lay.rows.sum() == 160
        ul = SC.layout("skew", 0, world, mode)
        assert ul.rows.min() > 0.8 * ul.rows.max()
    assert SC.layout("skew", 1, 3, mode).starts.tolist() == [0, 1, 1, 160]
    if mode == "explicit":
        assert set(np.unique(r).tolist()) == {1.0, 2.0, 3.0, 4.0, 5.0}
    else:
        assert set(np.unique(r).tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0}


def test_tiny_edges():
    """3 item rows: chpad = 1, 4·world gathered positions, the last rank (world 3) or the last rank of 4
    empty, fewer item rows than ranks at world 4."""
    B = SC.problem("tiny")[3]
    assert np.diff(B.i_ptr).tolist() == [30, 25, 35] and len(B.user_ids) == 40
    want = {2: [0, 2, 3], 3: [0, 1, 3, 3], 4: [0, 1, 2, 3, 3]}
    for world in WORLDS:
        lay = SC.layout("tiny", 1, world)
        assert lay.starts.tolist() == want[world]
        assert lay.chpad == 1 and lay.prows == 4 * world
        assert lay.rows[-1] == 0 or world == 2
    # an item-side top-k deals the 3 src rows one per rank: at world 4 the last rank scores nothing
    assert [SC.rank_slice(3, r, 4)[1:] for r in range(4)] == [(0, 1), (1, 2), (2, 3), (3, 3)]


@pytest.mark.parametrize("case", SC.CASES)
def test_position_map(case):
    """pos is injective into [0, prows), keeps a rank's chunk contiguous, and pos_inv recovers (rank, local
    row): every row of the small sides, and the first / last own row and both sides of every chunk
    boundary of each rank."""
    for side in (0, 1):
        for world in WORLDS:
            lay = SC.layout(case, side, world)
            assert lay.chpad == max(1, -(-lay.maxrows // SC.NCH)) and lay.prows == SC.NCH * world * lay.chpad
            seen = {}
            for r in range(world):
                lo, hi = lay.own(r)
                for row in range(lo, hi):
                    i = row - lo
                    p = lay.pos(r, i)
                    assert 0 <= p < lay.prows, (case, side, world, r, i, p)
                    assert p not in seen, (case, side, world, r, i, seen.get(p))
                    seen[p] = (r, i)
                    assert lay.pos_inv(p) == (r, i)
                    assert lay.owner(row) == r and lay.chunk(row) == i // lay.chpad
                    # chunk q of every rank is one contiguous block of world·chpad positions
                    assert p // (world * lay.chpad) == i // lay.chpad
                for row in lay.probe_rows(r):
                    assert lo <= row < hi and lay.pos_inv(lay.pos(r, row - lo)) == (r, row - lo)
                f = lay.foreign_row(r)
                assert f is None or not lo <= f < hi
            assert len(seen) == lay.n
            # positions no row maps to are padding: their inverse lies past the owner's rows
            for p in set(range(lay.prows)) - set(seen):
                r, i = lay.pos_inv(p)
                assert i >= lay.rows[r]


def test_rank_slice():
    for n in (0, 1, 2, 3, 5, 37, 160):
        for world in WORLDS:
            cuts = [SC.rank_slice(n, r, world) for r in range(world)]
            assert cuts[0][1] == 0 and cuts[-1][2] == n
            assert all(a[2] == b[1] for a, b in zip(cuts, cuts[1:]))
            assert all(hi - lo <= per for per, lo, hi in cuts)


@functools.lru_cache(maxsize=None)
def _max_cond(case, k, mode):
    """Largest fp64 condition number of A + lambda·n·I over the rows of the item half (from the injected
    user factors) and of the user half (from the oracle's item factors)."""
    B, (implicit, alpha, reg) = SC.problem(case, mode)[3:]
    src = SC.injected(case, k, mode)[0]
    out = []
    for side in (1, 0):
        _, ptr, col, val, _ = SC.side_csr(B, side)
        G = O.gram(src) if implicit else None
        worst = 0.0
        for j in range(len(ptr) - 1):
            A, _, n = O.normal_equation(src, ptr, col, val, j, implicit, alpha, G)
            w = np.linalg.eigvalsh(A + reg * n * np.eye(k))
            worst = max(worst, float(w[-1] / w[0]) if w[0] > 0 else np.inf)
        out.append(worst)
        src = cbind.half_sweep(src, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
    return tuple(out)


@pytest.mark.parametrize("case,k,mode", CHOLESKY_RANKS)
def test_condition_cap(case, k, mode):
    """Every row's normal equation, on both halves, has an fp64 condition number below 3e3: the bound under
    which tests/test_gpu_rating_modes.py justifies 1e-4 per row.  A condition of the cases, not a
    measurement: a case that exceeds it is changed, not the cap."""
    item, user = _max_cond(case, k, mode)
    print(f"SHARD_CASES {case} k{k} {mode}: condition item side {item:.3g}, user side {user:.3g}")
    assert item < SC.COND_CAP and user < SC.COND_CAP


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("case,mode", CASE_MODES)
def test_oracle_through_the_layout(case, mode, world):
    """Each rank's rows solved by the C oracle from the src factors as the gathered layout holds them (col
    remapped to padded positions, zero rows in the padding), the result packed into the rank's layout
    chunks, gathered chunk by chunk and unpacked into dense order: equals O.half_sweep of the whole
    problem, item half then user half."""
    B, (implicit, alpha, reg) = SC.problem(case, mode)[3:]
    k = 3 if case == "tiny" else 16
    src = SC.injected(case, k, mode)[0]
    for side in (1, 0):
        _, ptr, col, val, _ = SC.side_csr(B, side)
        dst, sl = SC.layout(case, side, world, mode), SC.layout(case, 1 - side, world, mode)
        # the gathered src: rank r's local row i at pos(r, i)
        Z = np.zeros((sl.prows, k), np.float32)
        where = np.array([sl.pos(sl.owner(j), j - sl.starts[sl.owner(j)]) for j in range(sl.n)], np.int64)
        Z[where] = src
        G = cbind.gram(Z)
        full = np.zeros((dst.prows, k), np.float32)
        for r in range(world):
            lo, hi = dst.own(r)
            own = np.zeros((SC.NCH * dst.chpad, k), np.float32)
            if hi > lo:
                e0, e1 = ptr[lo], ptr[hi]
                own[:hi - lo] = cbind.solve_rows(Z, G, ptr[lo:hi + 1] - e0, where[col[e0:e1]].astype(np.int32), val[e0:e1],
                                                 reg=reg, alpha=alpha, implicit=implicit)
            for q in range(SC.NCH):  # gather_chunks: chunk q of rank r
                p0 = q * world * dst.chpad + r * dst.chpad
                full[p0:p0 + dst.chpad] = own[q * dst.chpad:(q + 1) * dst.chpad]
        X = np.stack([full[dst.pos(dst.owner(j), j - dst.starts[dst.owner(j)])] for j in range(dst.n)])
        ref = O.half_sweep(src, ptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
        assert np.allclose(X, ref, rtol=1e-5, atol=1e-6), (case, side, world, float(np.max(np.abs(X - ref))))
        src = ref
