"""GPU parity at the edges of the per-row gathers of the D = 64 / 96 push-through kernels and of the
one-wave heavy kernel's start-up.

The D >= 64 light kernels gather unconditionally (masked and past-the-end entries gather the zero
row of Z); x' owns its columns per lane in consecutive groups and runs two gather
batches deep.  The wave kernel reads each row's {row, p0, degree} descriptor from the bucket-ordered
descriptor list at the launch's own offset (past the light buckets and past the split-K prefix).  The
cases below put rows on both sides of every size at which those paths change: degrees around the
16-entry blocks and the 8-entry x' batches, the 64-entry boundary of the two-entries-per-lane D = 96
instance, the 32-rating stages of the wave build, masked entries (implicit ratings <= 0) in the first,
a middle and the last entry, a row of zeros only, src row 0 and the last src row, launches whose row
count leaves waves past the end in the last workgroup, and descriptor offsets behind light buckets and
a split-K prefix.

One item half-sweep per case from injected unit-norm user factors over 320 users, every row against
the fp64 oracle (oracle/spark_als.py half_sweep) at the project's per-row bound max|x - x64| /
max|x64| < 1e-4 (tests/test_gpu_parity.py), rows whose reference is zero exactly zero; a second
half-sweep on the same inputs gives the same bits.
"""
import functools

import numpy as np
import pytest

from oracle import spark_als as O
from tests import ladder as LD
from tests.test_gpu_parity import Ctx

pytestmark = pytest.mark.gpu

TOL = 1e-4
N_SRC = 320
FILL = 8  # degree of the filler rows that make every user appear (light16 pairs, or the wave kernel)


def _uids():
    rng = np.random.default_rng(5)
    return np.sort(rng.choice(np.arange(3, 50000, dtype=np.int64), N_SRC, replace=False)).astype(np.int32)


def _row(rng, d, must=()):
    """d distinct src indices, sorted (the CSR order of a row's entries), holding every index of `must`."""
    rest = np.setdiff1d(np.arange(N_SRC), np.asarray(must, np.int64))
    return np.sort(np.r_[np.asarray(must, np.int64), rng.choice(rest, d - len(must), replace=False)])


def _ratings(rng, d, mode):
    if mode == "uniform":  # one confidence: the pre-split build of the wave kernel
        return np.ones(d)
    if mode == "varying":  # per-rating confidence
        return rng.choice([0.5, 1.0, 2.0], d)
    return rng.integers(1, 6, d).astype(np.float64)  # explicit stars


def _mask(r, *where):
    """Zero and negative ratings at the given entries (alternating), as the masked entries of an
    implicit row; explicit rows keep them as ordinary ratings."""
    r = r.copy()
    for t, e in enumerate(where):
        r[e] = 0.0 if t % 2 == 0 else -2.0
    return r


@functools.lru_cache(maxsize=None)
def _case(name, mode):
    """(user, item, rating, blocks, degree of each item row in item-id order) of a named row set."""
    rng = np.random.default_rng(sum(map(ord, name + mode)))
    rows = []  # (src indices, ratings)

    def add(d, must=(), mask=()):
        cols = _row(rng, d, must)
        r = _ratings(rng, d, mode)
        rows.append((cols, _mask(r, *mask) if mask else r))

    if name == "light64":
        for d in (33, 40, 41, 48, 63, 64):
            add(d)
        add(33, must=(0, N_SRC - 1))
        add(64, must=(0, N_SRC - 1), mask=(0, 31, 63))
        add(41, mask=(0, 20, 40))
        add(57, mask=(56,))
        cols = _row(rng, 48)
        rows.append((cols, np.zeros(48)))  # no positive rating: b = 0, the solution is exactly 0
    elif name == "light96":
        for d in (65, 72, 73, 80, 96):
            add(d)
        add(96, must=(0, N_SRC - 1), mask=(0, 63, 64, 95))
        add(81, mask=(64, 80))
    elif name.startswith("heavy"):  # heavy-<degrees joined by _>
        for t, d in enumerate(int(x) for x in name.split("-")[1].split("_")):
            add(d, must=(0, N_SRC - 1) if t == 0 else ())
    elif name == "buckets":  # degrees of every light bucket, all through the wave kernel at light 0
        for d in (12, 20, 31, 40, 64, 70, 96, 130, 97):
            add(d)
    elif name == "split":  # chunk 256: one split row ahead of the unsplit heavy rows
        for d in (300, 65, 129, 256):
            add(d, must=(0, N_SRC - 1) if d == 65 else ())
    else:
        raise ValueError(name)
    for f in range(N_SRC // FILL):  # every user appears
        rows.append((np.arange(FILL * f, FILL * f + FILL), _ratings(rng, FILL, mode)))
    uid = _uids()
    user = np.concatenate([uid[c] for c, _ in rows])
    item = np.concatenate([np.full(len(c), 1000 + 7 * t, np.int32) for t, (c, _) in enumerate(rows)])
    r = np.concatenate([v for _, v in rows]).astype(np.float32)
    perm = rng.permutation(user.size)
    user, item, r = user[perm], item[perm], r[perm]
    B = O.make_blocks(user, item, r)
    assert len(B.user_ids) == N_SRC
    return user, item, r, B, np.diff(B.i_ptr)


@functools.lru_cache(maxsize=None)
def _src(k):
    F = LD.unit_rows(np.random.default_rng(k), N_SRC, k)
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def _ref(name, mode, k):
    """The oracle's item half, computed once per (row set, rating mode, rank)."""
    B = _case(name, mode)[3]
    implicit = mode != "stars"
    V = O.half_sweep(_src(k), B.i_ptr, B.i_col, B.i_val, reg=0.5 if implicit else 0.1, alpha=40.0, implicit=implicit)
    V.setflags(write=False)
    return V


def _run(gpu_lib, tmp_path, name, mode, k, light, chunk=0):
    """One item half-sweep of the case, every row against the oracle, the engine's light / other split
    against the test's labels, and a second half-sweep bit for bit."""
    implicit = mode != "stars"
    user, item, r, B, deg = _case(name, mode)
    KP = LD.padded_rank(k)
    c = Ctx(gpu_lib, k, implicit=implicit, reg=0.5 if implicit else 0.1, alpha=40.0, light=light)
    c.ratings(user, item, r)
    c.inject(0, B.user_ids, _src(k))
    c.inject(1, B.item_ids, np.zeros((len(B.item_ids), k), np.float32))
    c.half(1)
    ids, X = c.factors(1)
    assert np.array_equal(ids, B.item_ids)
    paths = np.array([LD.path_of(d, KP, light, chunk) for d in deg])
    is_light = np.array([p.startswith("light") for p in paths])
    want = [int(is_light.sum()), int(deg[is_light].sum()), int((~is_light).sum()), int(deg[~is_light].sum())]
    assert c.stats(1).tolist() == want, (c.stats(1).tolist(), want)
    X_ref = _ref(name, mode, k)
    err = LD.row_errors(X, X_ref)
    by_path = ", ".join(f"{p} {err[paths == p].max():.2e}" for p in sorted(set(paths.tolist())))
    print(f"ROW_GATHER {name} {mode} k{k} light{light} chunk{chunk}: by path {by_path}")
    LD.assert_rows(X, X_ref, ids, deg, paths, TOL, f"item half [{name}-{mode}-k{k}]", tmp_path)
    c.half(1)
    X2 = c.factors(1)[1]
    assert np.array_equal(X.view(np.uint32), X2.view(np.uint32)), "a second half-sweep on the same inputs differs"
    return paths


@pytest.mark.parametrize("k", [50, 100, 128, 200])
@pytest.mark.parametrize("mode", ["varying", "stars"])
def test_light64_gathers(gpu_lib, tmp_path, mode, k):
    """Degrees 33..64 in one launch of the D = 64 kernel at KP 64 / 128 / 128 / 256 (padded columns at
    every rank but 128): masked first / middle / last entries, a row of zeros, src row 0 and the last
    src row, 11 rows (waves past the end in the last workgroup)."""
    paths = _run(gpu_lib, tmp_path, "light64", mode, k, 64)
    n64 = int(np.sum(paths == "light64"))
    assert n64 == 11 and n64 % 4 != 0
    if mode == "varying":
        X_ref = _ref("light64", mode, k)
        assert (~X_ref.any(axis=1)).sum() == 1  # the row of zeros (checked exactly zero by assert_rows)


@pytest.mark.parametrize("mode", ["varying", "stars"])
def test_light96_gathers(gpu_lib, tmp_path, mode):
    """light_max_degree = 96 at rank 128: the second entry per lane (entries 64..95), x' batches across
    the 64-entry boundary, masked entries 0, 63, 64 and 95."""
    paths = _run(gpu_lib, tmp_path, "light96", mode, 128, 96)
    assert int(np.sum(paths == "light96")) == 7


HEAVY_SETS = ["256", "65_256", "96_97_128", "65_96_97_129_256", "65_96_97_128_129_256"]


@pytest.mark.parametrize("k", [50, 128])
@pytest.mark.parametrize("degs", HEAVY_SETS)
def test_wave_startup_row_counts(gpu_lib, tmp_path, degs, k):
    """1, 2, 3, 5 and 6 heavy rows behind the light buckets (the descriptor offset of the heavy run;
    waves past n_rows in the last workgroup), degrees at the 32-rating stage boundaries; uniform
    confidence (the pre-split build)."""
    paths = _run(gpu_lib, tmp_path, "heavy-" + degs, "uniform", k, -1)
    assert int(np.sum(paths == "wave")) == len(degs.split("_"))


@pytest.mark.parametrize("k", [50, 128])
@pytest.mark.parametrize("mode", ["varying", "stars"])
def test_wave_startup_rating_modes(gpu_lib, tmp_path, mode, k):
    """The six stage-boundary degrees with per-rating confidence (the in-kernel split) and explicit."""
    paths = _run(gpu_lib, tmp_path, "heavy-" + HEAVY_SETS[-1], mode, k, -1)
    assert int(np.sum(paths == "wave")) == 6


@pytest.mark.parametrize("k", [50, 128])
@pytest.mark.parametrize("mode", ["uniform", "varying"])
def test_wave_every_bucket(gpu_lib, tmp_path, mode, k):
    """light_max_degree = 0: rows of every degree from 8 up go through the wave kernel, whose launch
    then starts at the head of the descriptor list."""
    paths = _run(gpu_lib, tmp_path, "buckets", mode, k, 0)
    assert set(paths.tolist()) == {"wave"}


@pytest.mark.parametrize("k", [50, 128])
def test_wave_behind_split_prefix(gpu_lib, tmp_path, monkeypatch, k):
    """A row above the split-K chunk length (256) ahead of three unsplit heavy rows: the unsplit
    launch's descriptors start past the split prefix."""
    monkeypatch.setenv("ALBEDO_SPLIT_CHUNK", "256")
    paths = _run(gpu_lib, tmp_path, "split", "uniform", k, -1, chunk=256)
    assert int(np.sum(paths == "split")) == 1 and int(np.sum(paths == "wave")) == 3
