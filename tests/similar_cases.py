"""Shared pieces of the als_similar tests (tests/test_gpu_similar.py on the GPU, tests/test_similar_cases.py on
the CPU): the cases and `expected`, the definition computed with numpy float32 and the C oracle.

The unit image of a side is, per row y (fp32): s = f2j_sdot(y, y), r = sqrt(s), u = y / r, all in float32
(numpy's float32 sqrt and divide are correctly rounded, like the device's).  A row has no direction when
!(s > 0 && s < inf); its unit row is NaN.  For a requested row, the rows without a direction and the row
itself are dropped and oracle.cbind.recommend gives the best k of the rest by f2j_sdot(u_i, u_j) in
(score desc, id asc) order, -1 / NaN padded.  A requested row that is unknown or has no direction gets an
all-padding list.  Everything is compared bit for bit.

A case is a dict: ids (ascending raw ids), F [n, rank], k, subset (None: every row, or raw ids in caller order).
"""
import functools

import numpy as np

from oracle import cbind
from oracle import spark_als as O
from tests.query_cases import bits, same  # noqa: F401  (the GPU tests compare with them)

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
SLICE_ROWS = 256  # ALBEDO_QUERY_SLICE_ROWS of the GPU tests
SIZES = (1, 2, "k", "k+1", "k+2", 255, 256, 257, 258, 1000)
RANKS = (1, 4, 5, 50, 64, 65, 128, 129, 256)
KS = (1, 30, 63, 64)


def size(n, k):
    return {"k": k, "k+1": k + 1, "k+2": k + 2}.get(n, n)


def unit_image(F):
    """(U [n, rank] float32 with NaN rows where there is no direction, has_direction [n] bool)."""
    F = np.ascontiguousarray(F, np.float32)
    with np.errstate(all="ignore"):
        s = O.f2j_sdot(F, F)
        ok = (s > 0) & (s < np.inf)
        r = np.sqrt(s, dtype=np.float32)
        U = (F / r[:, None]).astype(np.float32)
    U[~ok] = np.nan
    return U, ok


def expected(case):
    """(src ids [n], ids [n, k] int32, scores [n, k] float32) of the case."""
    ids = np.asarray(case["ids"], np.int32)
    k = int(case["k"])
    U, ok = unit_image(case["F"])
    src = ids.copy() if case["subset"] is None else np.asarray(case["subset"], np.int32)
    out_i = np.full((src.size, k), -1, np.int32)
    out_s = np.full((src.size, k), np.nan, np.float32)
    for i, sid in enumerate(src):
        r = int(np.searchsorted(ids, sid))
        if r >= ids.size or ids[r] != sid or not ok[r]:
            continue
        keep = ok.copy()
        keep[r] = False
        if keep.any():
            out_i[i], out_s[i] = (a[0] for a in cbind.recommend(U[r:r + 1], ids[keep], U[keep], k))
    return src, out_i, out_s


def expected_vectors(ids, F, q, k, excl=None):
    """als_similar_vectors: the unit rule on q, then tests/query_cases.py:expected on the unit image."""
    from tests import query_cases as QC
    U, _ = unit_image(F)
    uq, _ = unit_image(q)
    return QC.expected(dict(dst_ids=np.asarray(ids, np.int32), F=U, q=uq, k=k, excl=excl))


def _ids(rng, n, lo=-5000, hi=5000):
    return np.sort(rng.choice(np.arange(lo, hi, dtype=np.int64), n, replace=False)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def random_case(n, k, rank, seed=0):
    """Gaussian rows whose norms spread over e^-20 .. e^20 (17 decades); every row is asked."""
    rng = np.random.default_rng([seed, n, k, rank])
    F = rng.standard_normal((n, rank)) * np.exp(rng.uniform(-20.0, 20.0, (n, 1)))
    return dict(ids=_ids(rng, n), F=F.astype(np.float32), k=k, subset=None)


def edge_copy_case(k=5, rank=6):
    """1000 rows in slices of 256.  Rows 0, 255, 256 and 999, the first or last of their slices, each have an
    exact copy in another slice; the eight are positive rows and the rest negative ones (cosine below 0), so
    each one's best match is its copy, ahead of the other three pairs."""
    rng = np.random.default_rng(21)
    n = 1000
    F = -np.abs(rng.standard_normal((n, rank))).astype(np.float32) - np.float32(0.01)
    pairs = {0: 300, 255: 500, 256: 100, 999: 10}
    for q, c in pairs.items():
        F[q] = np.abs(rng.standard_normal(rank)).astype(np.float32) + np.float32(0.5)
        F[c] = F[q]
    ids = _ids(rng, n)
    return dict(ids=ids, F=F, k=k, subset=ids[list(pairs)].copy(), pairs=pairs)


def tie_case(k=10, rank=6):
    """Rows 246..275 of 400 (30 rows straddling row 256) share one direction: 19 are the base row scaled by
    2^-9 .. 2^9, 11 are exact copies, so their unit rows are bit-equal and they tie in every list.  The
    other rows have negative components where the base is positive.  Asked: row 5, a positive row (its
    list is the k lowest ids of the block), the block's first member and one in the middle (each leaves
    itself out and keeps the others)."""
    rng = np.random.default_rng(22)
    n = 400
    F = -np.abs(rng.standard_normal((n, rank))).astype(np.float32) - np.float32(0.01)
    base = np.array([2, 1.5, 1, 0.5, 2.25, 1.25][:rank], np.float32)
    block = np.arange(246, 276)
    scale = np.concatenate([2.0 ** np.arange(-9, 10), np.ones(11)]).astype(np.float32)
    F[block] = base[None, :] * rng.permutation(scale)[:, None]
    F[5] = base + np.array([0.25, -0.125, 0.5, 0, 0.125, -0.25][:rank], np.float32)
    ids = _ids(rng, n)
    return dict(ids=ids, F=F, k=k, subset=ids[[5, 246, 260]].copy(), block=block)


def no_direction_rows(rank):
    """One row of each kind without a direction."""
    z = np.zeros(rank, np.float32)
    rows = [z.copy(), np.full(rank, -0.0, np.float32)]
    for v in (np.nan, np.inf, -np.inf):
        r = np.ones(rank, np.float32)
        r[rank // 2] = v
        rows.append(r)
    rows.append(np.full(rank, 2.0 ** 64, np.float32))   # s overflows to +inf
    rows.append(np.full(rank, 2.0 ** -80, np.float32))  # s underflows to 0
    return np.array(rows, np.float32)


def no_direction_case(k=8, rank=5):
    """300 Gaussian rows, seven of them without a direction, at slice edges among other places."""
    rng = np.random.default_rng(23)
    n = 300
    F = rng.standard_normal((n, rank)).astype(np.float32)
    at = np.array([3, 100, 255, 256, 257, 280, 299])
    F[at] = no_direction_rows(rank)
    return dict(ids=_ids(rng, n), F=F, k=k, subset=None, at=at)


def all_without_direction_case(k=4, rank=5):
    F = np.tile(no_direction_rows(rank), (6, 1))
    rng = np.random.default_rng(24)
    return dict(ids=_ids(rng, F.shape[0]), F=F, k=k, subset=None)


def k_plus_one_directions_case(k=8, rank=5):
    """50 rows of which exactly k + 1 have a direction: their lists are full, only because self is gone."""
    rng = np.random.default_rng(25)
    n = 50
    F = np.tile(no_direction_rows(rank), (8, 1))[:n].copy()
    good = np.sort(rng.choice(n, k + 1, replace=False))
    F[good] = rng.standard_normal((k + 1, rank)).astype(np.float32)
    return dict(ids=_ids(rng, n), F=F, k=k, subset=None, good=good)


def subset_case(k=7, rank=6):
    """The subset contract on 300 rows whose catalogue holds INT32_MIN and INT32_MAX: unknown ids, repeated
    ids, the edge ids, caller order kept."""
    rng = np.random.default_rng(26)
    n = 300
    ids = _ids(rng, n)
    ids[0], ids[-1] = I32_MIN, I32_MAX
    F = (rng.standard_normal((n, rank)) * np.exp(rng.uniform(-5, 5, (n, 1)))).astype(np.float32)
    unknown = np.array([I32_MIN + 1, 4999999, I32_MAX - 1], np.int32)
    assert not np.isin(unknown, ids).any()
    subset = np.concatenate([ids[[200, 3]], unknown[:1], [I32_MAX, I32_MIN], ids[[3, 3, 299, 150]], unknown[1:],
                             ids[[200]]]).astype(np.int32)
    return dict(ids=ids, F=F, k=k, subset=subset, unknown=unknown)


def fp64_cosine(F):
    """[n, n] cosine in fp64 of the rows that have a direction (NaN elsewhere)."""
    F64 = np.asarray(F, np.float64)
    with np.errstate(all="ignore"):
        nr = np.sqrt(np.sum(F64 * F64, axis=1))
        return (F64 / nr[:, None]) @ (F64 / nr[:, None]).T


CASES = ("edge_copy_case", "tie_case", "no_direction_case", "all_without_direction_case", "k_plus_one_directions_case",
         "subset_case")
