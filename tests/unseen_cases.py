"""Shared pieces of the als_recommend_unseen tests (tests/test_gpu_recommend_unseen.py on the GPU,
tests/test_unseen_cases.py on the CPU): the cases and their expectation.

A case is a dict: src_ids / dst_ids (ascending raw ids), U [n_src, rank], V [n_dst, rank] and E, one array of
dst row indices per src row: the row's known pairs.  Every src row knows at least one dst row and every dst
row is known by someone (a filler row knows them all), so the ratings of `ratings(case)` make a context hold
exactly these ids.

The expectation is tests/query_cases.expected, the C oracle over the rows left, on a case dict built from the
factors and each row's exclusion list.  Everything is compared bit for bit: there is no tolerance.

DEPTH and K are the design point of the exclusion ladder: with the top m of a row's unfiltered ranking known,
its certified top-DEPTH list keeps DEPTH - min(m, DEPTH) entries, and m cycles through the values at which
that crosses K, the list empties, or fewer than K dst rows are left at all.
"""
import functools

import numpy as np

from tests import query_cases as QC
from tests import topk_cases as TC

DEPTH, K = 64, 30
KS = (1, 30, 63, 64)
RANKS = (1, 3, 50, 100, 200)
SIZES = (1, "k-1", "k", "k+1", 63, 64, 65, 127, 128, 129, 513)


def _ids(rng, n):
    return np.sort(rng.choice(np.arange(-40 * n, 40 * n, dtype=np.int64), n, replace=False)).astype(np.int32)


def _case(src_ids, U, dst_ids, V, E, **more):
    so, do = np.argsort(src_ids, kind="stable"), np.argsort(dst_ids, kind="stable")
    inv = np.empty(len(do), np.int64)
    inv[do] = np.arange(len(do))
    E = [np.unique(inv[np.asarray(E[i], np.int64)]) if len(E[i]) else np.zeros(0, np.int64) for i in so]
    return dict(src_ids=np.ascontiguousarray(src_ids[so], np.int32), U=np.ascontiguousarray(U[so], np.float32),
                dst_ids=np.ascontiguousarray(dst_ids[do], np.int32), V=np.ascontiguousarray(V[do], np.float32), E=E, **more)


def scores(case):
    key = id(case["U"])
    if key not in _SCORES:
        _SCORES[key] = (case, QC.scores(case["U"], case["V"]))
    return _SCORES[key][1]


_SCORES = {}


def ranking(case):
    """[n_src, n_dst] dst rows of every src row in (score desc, id asc) order, nothing excluded (a stable sort of
    the negated scores: equal scores, -0.0 and +0.0 among them, stay in row order, which is id order)."""
    key = id(case["U"])
    if key not in _RANKING:
        _RANKING[key] = (case, np.argsort(-scores(case), axis=1, kind="stable").astype(np.int32))
    return _RANKING[key][1]


_RANKING = {}


def known(case):
    """[n_src, n_dst] bool: src row i knows dst row j."""
    m = np.zeros((len(case["src_ids"]), len(case["dst_ids"])), bool)
    m[np.repeat(np.arange(len(case["E"])), [len(e) for e in case["E"]]), np.concatenate(case["E"])] = True
    return m


def pairs(case):
    """The known pairs as raw (src ids, dst ids), one entry per pair, grouped by src row."""
    n = [len(e) for e in case["E"]]
    src = np.repeat(case["src_ids"], n)
    dst = case["dst_ids"][np.concatenate(case["E"])] if sum(n) else np.zeros(0, np.int32)
    return np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32)


def ratings(case, side=0, seed=0):
    """(user, item, rating) of the known pairs, shuffled; side = 1: the case's src rows are the items."""
    src, dst = pairs(case)
    rng = np.random.default_rng(seed)
    p = rng.permutation(src.size)
    r = rng.uniform(0.5, 3.0, src.size).astype(np.float32)
    return (src[p], dst[p], r) if side == 0 else (dst[p], src[p], r)


def expected(case, k, rows=None):
    """(ids, scores) [n, k] of the src rows `rows` (default: all) from the C oracle over the dst rows left."""
    rows = np.arange(len(case["src_ids"])) if rows is None else np.asarray(rows)
    q = dict(dst_ids=case["dst_ids"], F=case["V"], q=case["U"][rows], k=k,
             excl=[case["dst_ids"][case["E"][i]] for i in rows])
    return QC.expected(q)


def expected_fast(case, k):
    """The same lists from the full ranking, vectorised (the CPU test holds it equal to `expected` on a sample).
    For finite factors only: no score is NaN."""
    s, order = scores(case), ranking(case)
    keep = ~np.take_along_axis(known(case), order, axis=1)
    place = np.cumsum(keep, axis=1)
    r, c = np.nonzero(keep & (place <= k))
    out_i = np.full((len(order), k), -1, np.int32)
    out_s = np.full((len(order), k), np.nan, np.float32)
    out_i[r, place[r, c] - 1] = case["dst_ids"][order[r, c]]
    out_s[r, place[r, c] - 1] = s[r, order[r, c]]
    return out_i, out_s


def survivors(case, depth):
    """Entries each row's unfiltered top-`depth` list keeps."""
    top = ranking(case)[:, :depth]
    return (~np.take_along_axis(known(case), top, axis=1)).sum(axis=1)


def tier2_rows(case, depth, k):
    """The rows the filter cannot certify: a full list that keeps fewer than k entries."""
    if len(case["dst_ids"]) <= depth:
        return np.zeros(0, np.int64)
    return np.nonzero(survivors(case, depth) < k)[0]


def ladder_m(n_dst, depth=DEPTH, k=K):
    return [int(np.clip(m, 0, n_dst)) for m in (0, 1, depth - k - 1, depth - k, depth - k + 1, depth, depth + 40,
                                                n_dst - k - 1, n_dst - k, n_dst - k + 1)]


def designed_tier2(case, depth=DEPTH, k=K):
    """The rows `with_exclusions` sends to tier 2 by design: m above depth - k (the filler row knows all)."""
    if len(case["dst_ids"]) <= depth:
        return np.zeros(0, np.int64)
    return np.nonzero(np.minimum(case["m"], depth) > depth - k)[0]


def with_exclusions(src_ids, U, dst_ids, V, seed, depth=DEPTH, k=K):
    """Each src row knows the top m of its unfiltered ranking, m cycling through ladder_m, a few random rows
    past rank max(m, depth + 46) and so outside every list it is filtered from, and at least one such row; the
    last src row is the filler and knows every dst row."""
    rng = np.random.default_rng(seed)
    base = _case(src_ids, U, dst_ids, V, [np.zeros(0, np.int64)] * len(src_ids))
    order = ranking(base)
    n_src, n_dst = order.shape
    ms = ladder_m(n_dst, depth, k)
    E, m_of = [], []
    for i in range(n_src):
        m = n_dst if i == n_src - 1 else ms[i % len(ms)]
        tail = order[i][max(m, depth + 46):]
        extra = rng.choice(tail, min(tail.size, 1 + int(rng.integers(0, 4))), replace=False) if tail.size else tail
        e = np.concatenate([order[i][:m], extra])
        if e.size == 0:  # nothing past the lists to know (a small catalogue): the row's last-ranked dst row
            e, m = order[i][-1:], 0
        E.append(e)
        m_of.append(m)
    base["E"] = [np.unique(e) for e in E]
    base["m"] = np.array(m_of)
    return base


@functools.lru_cache(maxsize=None)
def ladder(rank, n_dst=700, n_src=70, seed=0):
    rng = np.random.default_rng([seed, rank, n_dst, n_src])
    U = rng.standard_normal((n_src, rank)).astype(np.float32)
    V = rng.standard_normal((n_dst, rank)).astype(np.float32)
    return with_exclusions(_ids(rng, n_src), U, _ids(rng, n_dst), V, seed + 1)


def size(n, k):
    return {"k-1": k - 1, "k": k, "k+1": k + 1}.get(n, n)


@functools.lru_cache(maxsize=None)
def sizes(n_dst, k=K, rank=6):
    """Eight src rows: exclusions that leave 0 (the filler, last), k - 1, k and k + 1 dst rows, and four rows of
    the ladder's first rungs."""
    rng = np.random.default_rng([7, n_dst, k])
    n_src = 8
    U = rng.standard_normal((n_src, rank)).astype(np.float32)
    V = rng.standard_normal((n_dst, rank)).astype(np.float32)
    case = with_exclusions(_ids(rng, n_src), U, _ids(rng, n_dst), V, 3, k=k)
    for i, left in enumerate((k - 1, k, k + 1)):
        keep = rng.choice(n_dst, min(left, n_dst - 1), replace=False) if n_dst > 1 else np.zeros(0, np.int64)
        case["E"][i] = np.setdiff1d(np.arange(n_dst), keep)
    case.pop("m")
    return case


def _exact(rng, shape, lo=-16, hi=17):
    return (rng.integers(lo, hi, shape) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_groups(k=K, depth=DEPTH, rank=6):
    """Exact small-integer factors.  Every src row is the same vector q.  Twenty dst rows score above a group of
    60 equal scores, which therefore lies across place `depth` of the unfiltered ranking (places 21 .. 80) and,
    once a row knows part of the twenty and part of the group, across place k of the filtered one."""
    rng = np.random.default_rng(21)
    n_dst, n_src = 400, 12
    V = _exact(rng, (n_dst, rank), -4, 5)                     # scores of at most 4.125 against q
    q = np.array([2, -1.5, 1, 0.5, -2, 1.25][:rank], np.float32)
    tie = np.sort(rng.choice(n_dst, 60, replace=False))
    V[tie] = q
    rest = np.setdiff1d(np.arange(n_dst), tie)
    top = rng.choice(rest, 20, replace=False)
    V[top] = 2 * q
    U = np.tile(q, (n_src, 1))
    others = np.setdiff1d(rest, top)
    E = []
    for i in range(n_src - 1):
        e = [top[: (3 * i) % 21], tie[i::3] if i % 2 else tie[:i], others[i:i + 1]]
        E.append(np.concatenate(e))
    E.append(np.arange(n_dst))
    return _case(_ids(rng, n_src), U, _ids(rng, n_dst), V, E, tie=tie, top=top)


@functools.lru_cache(maxsize=None)
def mass_tie(rank=50):
    """topk_cases.mass_tie (300 identical dst rows on top); src row 0 knows 250 of them, row 1 all 300, the
    others one each, the last is the filler."""
    uid, uf, iid, itf = TC.case("mass_tie", rank)
    uid, uf = uid[:24], uf[:24]
    tied = np.nonzero(np.isin(iid, TC.mass_tie_ids(iid, itf)))[0]
    rng = np.random.default_rng(22)
    E = [rng.choice(tied, 250, replace=False), tied] + [tied[i:i + 1] for i in range(21)] + [np.arange(len(iid))]
    return _case(uid, uf, iid, itf, E)


@functools.lru_cache(maxsize=None)
def zeros_and_negatives(rank=5):
    """Src rows 0 .. 3 are all zero (every score +0.0: the lowest ids not known); the others score every dst row
    negative except six rows of exactly zero."""
    rng = np.random.default_rng(23)
    n_dst, n_src = 300, 12
    V = -np.abs(_exact(rng, (n_dst, rank), 1, 17))
    zero = np.array([5, 100, 255, 256, 257, 299])
    V[zero] = 0.0
    V[zero[:3], 0] = np.float32(-0.0)
    U = np.abs(_exact(rng, (n_src, rank), 1, 17))
    U[:4] = 0.0
    E = [np.arange(i, 40 + 10 * i, 1 + i % 3) for i in range(n_src - 1)] + [np.arange(n_dst)]
    E[5], E[6] = zero[:4], np.concatenate([zero, np.arange(90)])
    return _case(_ids(rng, n_src), U, _ids(rng, n_dst), V, E, zero=zero)


PRUNE_KNOWN = 200  # dst rows every row of the pruning case knows: its unfiltered top 200


@functools.lru_cache(maxsize=None)
def pruning(rank=50, n_dst=8000, n_src=48):
    """topk_cases.anisotropic (the generator whose k = 100 case prunes in topk_exact_kernel): each src row knows
    its top PRUNE_KNOWN, so every row goes to tier 2; one more row knows everything."""
    uid, uf, iid, itf = TC.case("anisotropic", rank, n_dst)
    base = _case(uid[:n_src], uf[:n_src], iid, itf, [np.zeros(0, np.int64)] * n_src)
    order = ranking(base)
    base["E"] = [np.sort(order[i][:PRUNE_KNOWN]) for i in range(n_src - 1)] + [np.arange(n_dst)]
    return base


@functools.lru_cache(maxsize=None)
def passes(n_src=70000, n_dst=300, rank=4):
    """Two top-k passes at ALBEDO_TOPK_PASS = 65536.  Row i knows the dst rows (i + 7j) mod n_dst for j below
    1 + i mod 5, and every 97th row its unfiltered top 40 as well (tier 2); the last row knows all."""
    rng = np.random.default_rng(31)
    U = rng.standard_normal((n_src, rank)).astype(np.float32)
    V = rng.standard_normal((n_dst, rank)).astype(np.float32)
    case = _case(np.arange(n_src, dtype=np.int32) * 3 - 100000, U, _ids(rng, n_dst), V, [np.zeros(0, np.int64)] * n_src)
    order = ranking(case)
    E = [np.sort((i + 7 * np.arange(1 + i % 5)) % n_dst) for i in range(n_src)]
    for i in range(0, n_src, 97):
        E[i] = np.unique(np.concatenate([E[i], order[i][:40]]))
    E[-1] = np.arange(n_dst)
    case["E"] = E
    return case


def edge_ids(case):
    """The case with its lowest and highest ids on both sides moved to INT32_MIN / INT32_MAX."""
    out = dict(case)
    for name in ("src_ids", "dst_ids"):
        ids = case[name].copy()
        ids[0], ids[-1] = QC.I32_MIN, QC.I32_MAX
        out[name] = ids
    return out
