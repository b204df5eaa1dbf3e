"""Shared inputs of the top-k edge tests (tests/test_gpu_topk_edges.py on the GPU, the precondition
test of tests/test_oracle.py on the CPU): the role tests/ladder.py has for the solve paths.

Every generator is pure numpy and seeded and returns (uid, uf, iid, itf): raw ids that are sparse,
partly negative and in shuffled order (als_model_create sorts them), fp32 factors.  Each case aims at
one defence of albedo_amd/csrc/topk.hip that isotropic Gaussian factors never reach:

  negative        every top-k score below 0, a last chunk with padding rows (which score 0)
  mass_tie        300 identical dst rows on top: more ties at the k-th place than a candidate list holds
  group_ties      groups of identical dst rows, the k boundary inside a group
  zeros           exactly-zero rows on both sides, scores of exactly +0.0, k-th scores of 0
  dynamic_range   row norms over many decades under one global fp16 scale; the dst side at 2^-60 (the
                  scale's exponent reaches its clamp of +60) and at 2^60 (exponent about -52: the clamp
                  of -60 needs norms of 2^73, more than the dst Gram's fp32 partial sums hold; the src
                  side reaches it in test_topk_dst_norms_past_the_gram_range_raise)
  anisotropic     two dominant directions, half of the src rows on the negative side of the bound's box
  sizes           the size boundaries of the kernels (SIZE_* below)

oracle_lists() computes (and caches) the oracle's lists of a case, so that the tests of one process
share one reference per case.
"""
import functools

import numpy as np

from oracle import spark_als as O
from tests.ladder import padded_rank

LOW_RANKS = [1, 2, 3, 4, 5]          # below and around TOPK_M = 4 directions of the chunk bound
RANKS = [50, 100, 200]               # one per padded rank (64, 128, 256)
DYNAMIC_KINDS = ["dst_spread", "src_spread", "dst_tiny", "dst_huge"]
GROUP_TIES = {30: 4, 64: 7}          # k -> copies: the k boundary falls inside a group of `copies`

TOPK_KC = 64                         # kernels.h: list length / largest certified k
TOPK_CAP = 128                       # kernels.h: candidate list capacity
TINY = np.float32(np.finfo(np.float32).tiny)


def chunk_rows(rank):
    """dst rows per 16-KiB fp16 chunk (topk.hip TkScan::CH)."""
    return {64: 128, 128: 64, 256: 32}[padded_rank(rank)]


def _ids(rng, n):
    """n distinct raw ids from a range 37 times as long, a third of it below 0, in shuffled order."""
    lo = -(n * 37) // 3
    return (rng.choice(n * 37, n, replace=False) + lo).astype(np.int32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _unit(rng, rank):
    d = rng.standard_normal(rank)
    return d / np.linalg.norm(d)


def negative(rank):
    CH = chunk_rows(rank)
    rng = np.random.default_rng(1000 + rank)
    n_src, n_dst = 77, 3 * CH + 5
    itf = np.abs(rng.standard_normal((n_dst, rank)))
    uf = -np.abs(rng.standard_normal((n_src, rank)))
    return _ids(rng, n_src), _f32(uf), _ids(rng, n_dst), _f32(itf)


def mass_tie(rank):
    rng = np.random.default_rng(2000 + rank)
    n_src, n_dst, n_tie = 100, 3000, 300
    itf = _f32(0.3 * rng.standard_normal((n_dst, rank)))
    u = np.abs(rng.standard_normal(rank)) + 0.5
    itf[rng.choice(n_dst, n_tie, replace=False)] = _f32(u * (8.0 / np.linalg.norm(u)))
    uf = np.abs(rng.standard_normal((n_src, rank))) + 0.5
    return _ids(rng, n_src), _f32(uf), _ids(rng, n_dst), itf


def mass_tie_ids(iid, itf):
    """The ids of mass_tie's identical dst rows (the rows equal to the largest-norm row), ascending."""
    top = itf[np.argmax(np.linalg.norm(itf.astype(np.float64), axis=1))]
    return np.sort(iid[np.all(itf == top, axis=1)])


def group_ties(rank, copies):
    rng = np.random.default_rng(3000 + 10 * rank + copies)
    n_src, n_distinct = 90, 1500
    base = _f32(rng.standard_normal((n_distinct, rank)))
    itf = np.repeat(base, copies, axis=0)[rng.permutation(n_distinct * copies)]
    uf = rng.standard_normal((n_src, rank))
    return _ids(rng, n_src), _f32(uf), _ids(rng, n_distinct * copies), _f32(itf)


def zeros(rank):
    rng = np.random.default_rng(4000 + rank)
    n_src, n_dst = 120, 2000
    d = _unit(rng, rank)
    itf = -np.abs(rng.standard_normal((n_dst, 1))) * d + 0.05 * rng.standard_normal((n_dst, rank))
    zero = rng.random(n_dst) < 0.4
    itf[zero] = 0.0
    flip = rng.choice(np.nonzero(~zero)[0], 10, replace=False)
    itf[flip] = -itf[flip]
    uf = np.abs(rng.standard_normal((n_src, 1))) * d + 0.05 * rng.standard_normal((n_src, rank))
    uf[0::7] = 0.0
    uf[1::7] = -uf[1::7]
    return _ids(rng, n_src), _f32(uf) + np.float32(0.0), _ids(rng, n_dst), _f32(itf) + np.float32(0.0)


def dynamic_range(rank, kind):
    rng = np.random.default_rng(5000 + rank)
    n_src, n_dst = 100, 2000
    itf = rng.standard_normal((n_dst, rank))
    uf = rng.standard_normal((n_src, rank))
    if kind == "dst_spread":
        itf *= 10.0 ** rng.uniform(-6.0, 0.0, (n_dst, 1))
        itf[n_dst // 3] *= 1e3 / np.linalg.norm(itf[n_dst // 3])
    elif kind == "src_spread":
        uf *= 10.0 ** rng.uniform(-8.0, 0.0, (n_src, 1))
    elif kind == "dst_tiny":
        itf *= 2.0 ** -60
    elif kind == "dst_huge":
        itf *= 2.0 ** 60
    else:
        raise ValueError(kind)
    return _ids(rng, n_src), _f32(uf), _ids(rng, n_dst), _f32(itf)


def anisotropic(rank, n_dst=8000):
    rng = np.random.default_rng(6000 + rank)
    n_src = 400
    d1 = _unit(rng, rank)
    d2 = _unit(rng, rank)

    def rows(n):
        a = rng.lognormal(0.0, 1.0, (n, 1))
        b = rng.normal(0.0, 0.5, (n, 1))
        return a, b, 0.1 * rng.standard_normal((n, rank))

    a, b, e = rows(n_dst)
    itf = _f32(a * d1 + b * d2 + e)
    itf[n_dst - 100:] = itf[:100]  # equal scores, different ids, anywhere in the norm order
    a, b, e = rows(n_src)
    a[1::2] = -a[1::2]             # the chunk bound takes the lo side of the box in direction 1
    uf = a * d1 + b * d2 + e
    return _ids(rng, n_src), _f32(uf), _ids(rng, n_dst), itf


# ---- the size grid ---------------------------------------------------------------------------------

SIZE_USERS = 129     # users of every size-grid model; fewer are reached through the subset path
SIZE_SRC_DEFAULT = 67
SIZE_KS = [1, 30, 64]
SIZE_N_SRC = [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129]
SIZE_K_AT_1000 = [1, 2, 47, 48, 49, 63, 64, 65, 127, 128, 129, 511, 512]
SIZE_K_AT_100 = [65, 128, 512]


def size_n_dst(rank):
    """n_dst around TOPK_KC, one chunk, TOPK_NPROBE = 512 and one super-chunk of 16 chunks."""
    CH = chunk_rows(rank)
    return [1, 2, 63, 64, 65, CH - 1, CH, CH + 1, 511, 512, 513, 16 * CH - 1, 16 * CH + 1]


def size_grid(rank):
    """{n_dst: [(n_src, k), ...]} of test_topk_size_boundaries, n_dst in ascending order."""
    CH = chunk_rows(rank)
    grid = {}
    for n_dst in size_n_dst(rank):
        grid.setdefault(n_dst, []).extend((SIZE_SRC_DEFAULT, k) for k in SIZE_KS)
    grid.setdefault(16 * CH + 1, []).extend((n, 30) for n in SIZE_N_SRC)
    grid.setdefault(1000, []).extend((SIZE_SRC_DEFAULT, k) for k in SIZE_K_AT_1000)
    grid.setdefault(100, []).extend((SIZE_SRC_DEFAULT, k) for k in SIZE_K_AT_100)
    return {n: list(dict.fromkeys(grid[n])) for n in sorted(grid)}


def sizes(rank, n_dst):
    rng = np.random.default_rng(7000 + 13 * rank + n_dst)
    itf = _f32(rng.standard_normal((n_dst, rank)))
    if n_dst >= 18:
        m = itf[1::9].shape[0]
        itf[1::9] = itf[0::9][:m]
    uf = _f32(rng.standard_normal((SIZE_USERS, rank)))
    return _ids(rng, SIZE_USERS), uf, _ids(rng, n_dst), itf


# ---- the oracle's lists ------------------------------------------------------------------------------

GENERATORS = {"negative": negative, "mass_tie": mass_tie, "group_ties": group_ties, "zeros": zeros,
              "dynamic_range": dynamic_range, "anisotropic": anisotropic, "sizes": sizes}


@functools.lru_cache(maxsize=None)
def case(name, *args):
    """(uid, uf, iid, itf) of GENERATORS[name](*args), read-only and cached."""
    out = GENERATORS[name](*args)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_lists(name, args, k, swap=False):
    """O.recommend_for_all of a case at k, rows in ascending src id order (the engine's order for a
    whole side): (src ids, ids [n_src, k], scores [n_src, k]).  swap: the item side is the src."""
    uid, uf, iid, itf = case(name, *args)
    if swap:
        uid, uf, iid, itf = iid, itf, uid, uf
    order = np.argsort(uid, kind="stable")
    ids, sc = O.recommend_for_all(uid[order], uf[order], iid, itf, k)
    out = (uid[order], ids, sc)
    for a in out:
        a.setflags(write=False)
    return out


def products_are_normal(uf, itf):
    """Every fp32 product uf[i, c] * itf[j, c] is a normal number or exactly 0 (and finite)."""
    for s in uf:
        p = np.abs(s[None, :] * itf)
        if not np.all(np.isfinite(p)) or np.any((p != 0) & (p < TINY)):
            return False
    return True
