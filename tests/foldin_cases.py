"""Shared pieces of the fold-in tests (tests/test_gpu_foldin.py on the GPU, tests/test_foldin_cases.py on
the CPU): the triples of each case and `expected`, the fp64 oracle's answer for them.

`expected` is the fold-in's definition: the CSR of the new rows (triples with an unknown source dropped,
duplicates kept, ascending source order) through oracle.spark_als.half_sweep against the source factors,
and zeros for the rows left with no triple.  The data are the degree ladder of tests/ladder.py, whose 52
item rows (degrees 1..513) are folded in as new items against ~700 user factors, and small hand-built
cases for the tile edges and the input contract.
"""
import functools

import numpy as np

from oracle import spark_als as O
from tests import ladder as LD

FOLD_TILE = 32  # kernels.h: ratings per build step of the fold-in kernel
TOL = 1e-4      # the project's bar for every solve path (tests/test_gpu_rating_modes.py)
ID_SHIFT = 1 << 20  # new raw ids: the ladder's, moved off the model's
MODES = ("varying", "mixed", "stars_signed")
RANKS = (1, 50, 64, 65, 128, 129, 200, 256)
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


def fold_csr(row_id, src_id, rating, src_ids):
    """(ids, ptr, col, val, degree): the distinct row ids ascending and their CSR over the rows of the
    ascending table `src_ids`; a row's entries in ascending source row, copies of a pair in input order."""
    row_id = np.asarray(row_id, np.int32)
    src_id = np.asarray(src_id, np.int32)
    rating = np.asarray(rating, np.float32)
    src_ids = np.asarray(src_ids, np.int32)
    ids = np.unique(row_id)
    pos = np.searchsorted(src_ids, src_id)
    known = np.zeros(src_id.size, bool)
    if src_ids.size:
        known = src_ids[np.minimum(pos, src_ids.size - 1)] == src_id
    r = np.searchsorted(ids, row_id[known])
    s = pos[known]
    order = np.lexsort((s, r))  # stable
    deg = np.bincount(r, minlength=ids.size).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return ids, ptr, s[order].astype(np.int32), rating[known][order], deg


def expected(Ysrc, src_ids, row_id, src_id, rating, *, reg, alpha, implicit):
    """(ids, degree, factors fp32) of the fold-in of these triples against Ysrc (rows of src_ids)."""
    ids, ptr, col, val, deg = fold_csr(row_id, src_id, rating, src_ids)
    Ysrc = np.asarray(Ysrc, np.float32)
    X = np.zeros((ids.size, Ysrc.shape[1]), np.float32)
    live = deg > 0
    if live.any():  # the rows without a triple hold no entries: col and val serve as they are
        lptr = np.concatenate([[0], np.cumsum(deg[live])]).astype(np.int64)
        X[live] = O.half_sweep(Ysrc, lptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
    return ids, deg, X


@functools.lru_cache(maxsize=None)
def data(mode):
    user, item, ideg = LD.ladder_coo()
    r = LD.ladder_ratings(mode, user, ideg)
    for a in (user, item, r):
        a.setflags(write=False)
    return user, item, r, O.make_blocks(user, item, r)


@functools.lru_cache(maxsize=None)
def src_factors(k, n, seed=0):
    F = LD.unit_rows(np.random.default_rng(1000 * seed + k), n, k)
    F.setflags(write=False)
    return F


def ladder_items(mode):
    """The ladder's item rows as new items: (row ids shifted off the model's, user ids, ratings)."""
    user, item, r, _ = data(mode)
    return (item.astype(np.int64) + ID_SHIFT).astype(np.int32), user, r


def ladder_users(mode):
    """The mirror: the ladder's ~700 users as new users rating the 52 items."""
    user, item, r, _ = data(mode)
    return (user.astype(np.int64) + ID_SHIFT).astype(np.int32), item, r


@functools.lru_cache(maxsize=None)
def ladder_expected(mode, k, side):
    """side 1: new items against unit-row user factors; side 0: new users against unit-row item factors."""
    implicit, alpha, reg = LD.MODES[mode]
    B = data(mode)[3]
    src_ids = B.user_ids if side == 1 else B.item_ids
    Y = src_factors(k, len(src_ids), seed=side)
    row, src, r = ladder_items(mode) if side == 1 else ladder_users(mode)
    ids, deg, X = expected(Y, src_ids, row, src, r, reg=reg, alpha=alpha, implicit=implicit)
    X.setflags(write=False)
    return ids, deg, X


def degree_rows(degrees, src_ids, seed=5, first_id=-3):
    """One new row per entry of `degrees`, consecutive raw ids from first_id, sources drawn without
    replacement, ratings of the `varying` kind; shuffled."""
    rng = np.random.default_rng(seed)
    rows, srcs = [], []
    for t, d in enumerate(degrees):
        rows.append(np.full(d, first_id + t, np.int32))
        srcs.append(rng.choice(src_ids, d, replace=False))
    row, src = np.concatenate(rows), np.concatenate(srcs).astype(np.int32)
    r = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], row.size).astype(np.float32)
    p = rng.permutation(row.size)
    return row[p], src[p], r[p]


def tile_degrees(k):
    return [FOLD_TILE - 1, FOLD_TILE, FOLD_TILE + 1, 2 * FOLD_TILE + 1, k - 1, k, k + 1]


def unknown_sources(src_ids, n, seed=9):
    """n int32 ids that are not in src_ids."""
    rng = np.random.default_rng(seed)
    out = np.setdiff1d(rng.integers(I32_MIN, I32_MAX, 4 * n + 16, dtype=np.int64), src_ids)[:n]
    assert out.size == n
    return out.astype(np.int32)


def contract_case(src_ids, seed=21):
    """The input-contract triples: row ids at both ends of int32 and -1, a row of unknown sources only,
    unknown sources mixed into a row, and one pair repeated 2, 3 and 64 times (in rows of their own)."""
    rng = np.random.default_rng(seed)
    src_ids = np.asarray(src_ids, np.int32)
    unk = unknown_sources(src_ids, 8)
    rows, srcs = [], []

    def add(rid, s):
        rows.append(np.full(len(s), rid, np.int32))
        srcs.append(np.asarray(s, np.int32))

    add(I32_MIN, rng.choice(src_ids, 5, replace=False))
    add(-1, rng.choice(src_ids, 40, replace=False))
    add(I32_MAX, rng.choice(src_ids, 9, replace=False))
    add(77, unk[:3])                                                   # degree 0
    add(78, np.concatenate([rng.choice(src_ids, 6, replace=False), unk[3:]]))  # 6 live of 11
    for rid, copies in ((100, 2), (101, 3), (102, 64)):
        add(rid, np.concatenate([np.full(copies, src_ids[7]), rng.choice(src_ids[8:], 4, replace=False)]))
    row, src = np.concatenate(rows), np.concatenate(srcs)
    r = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], row.size).astype(np.float32)
    # copies of one pair carry one rating: the result is then free of the input order
    for rid in (100, 101, 102):
        m = (row == rid) & (src == src_ids[7])
        r[m] = r[m][0]
    return row, src, r


def without_duplicates(row, src, r):
    """The triples with the first copy of every (row, src) pair only."""
    key = (row.astype(np.int64) << 32) | (src.astype(np.int64) & 0xFFFFFFFF)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return row[first], src[first], r[first]


def singular_case(k=8):
    """A source side of 3 rows at rank k (unit vectors: every product is exact) and one rating of source 1.
    With regParam = 0 the system is singular whatever the mode: G = diag(1, 1, 1, 0, ...) + c·e1 e1ᵀ meets
    an exact zero at pivot 3, the explicit e1 e1ᵀ at pivot 0.  Returns (src ids, Y, row, src, rating)."""
    src_ids = np.array([10, 20, 30], np.int32)
    Y = np.zeros((3, k), np.float32)
    Y[0, 0] = Y[1, 1] = Y[2, 2] = 1.0
    return src_ids, Y, np.array([4242], np.int32), np.array([20], np.int32), np.array([1.0], np.float32)
