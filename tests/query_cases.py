"""Shared pieces of the query top-k tests (tests/test_gpu_query_topk.py on the GPU, tests/test_query_cases.py
on the CPU): the cases of als_recommend_vectors and `expected`, the C oracle's answer for them.

`expected` is the call's definition.  For query i the dst rows named by its exclusion list are removed, then
those whose F2J score is NaN, and oracle.cbind.recommend (oracle/c/topk_cpu.c) gives the best k of the rest
in (score desc, id asc) order, -1 / NaN padded.  Everything is compared bit for bit: the arithmetic is fully
specified (fp32, left to right, no fused product), so there is no tolerance.

A case is a dict: dst_ids (any order), F [n_dst, rank], q [n_q, rank], k, excl (None or one id array per
query).  Factors are small integers over 8 (or 1/64 steps) where a case needs exact ties: their products and
sums are exact in fp32, so equal scores are equal by construction, not by luck.
"""
import functools

import numpy as np

from oracle import cbind
from oracle import spark_als as O

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
SLICE_ROWS = 256  # ALBEDO_QUERY_SLICE_ROWS of the GPU tests: 257 and 1000 rows cross slices
SIZES = (1, "k-1", "k", "k+1", 255, 256, 257, 1000)
N_Q = (1, 15, 16, 17, 33)
KS = (1, 30, 63, 64)
RANKS = (1, 4, 5, 6, 50, 64, 65, 128, 129, 256)


def scores(q, F):
    """[n_q, n_dst] F2J scores (fp32, left to right, multiply and add rounded separately)."""
    with np.errstate(all="ignore"):
        return O.f2j_sdot(np.asarray(q, np.float32)[:, None, :], np.asarray(F, np.float32)[None, :, :])


def kept_rows(case, i):
    """Mask over the dst rows query i lists: not excluded, score not NaN."""
    ids = np.asarray(case["dst_ids"], np.int32)
    keep = np.ones(ids.size, bool)
    if case["excl"] is not None:
        keep &= ~np.isin(ids, np.asarray(case["excl"][i], np.int32))
    keep &= ~np.isnan(scores(case["q"][i:i + 1], case["F"])[0])
    return keep


def expected(case):
    """(ids [n_q, k] int32, scores [n_q, k] float32) of the case, -1 / NaN padded."""
    q, F, k = np.asarray(case["q"], np.float32), np.asarray(case["F"], np.float32), int(case["k"])
    ids = np.asarray(case["dst_ids"], np.int32)
    out_i = np.full((q.shape[0], k), -1, np.int32)
    out_s = np.full((q.shape[0], k), np.nan, np.float32)
    for i in range(q.shape[0]):
        keep = kept_rows(case, i)
        if keep.any():
            out_i[i], out_s[i] = (a[0] for a in cbind.recommend(q[i:i + 1], ids[keep], F[keep], k))
    return out_i, out_s


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """ids equal and scores equal bit for bit (padding NaN included)."""
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def excl_csr(excl):
    ptr = np.zeros(len(excl) + 1, np.int64)
    np.cumsum([len(e) for e in excl], out=ptr[1:])
    ids = np.concatenate([np.asarray(e, np.int32) for e in excl]) if len(excl) else np.zeros(0, np.int32)
    return ptr, np.ascontiguousarray(ids, np.int32)


def _ids(rng, n, lo=-5000, hi=5000):
    return np.sort(rng.choice(np.arange(lo, hi, dtype=np.int64), n, replace=False)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def random_case(n_dst, n_q, k, rank, seed=0, with_excl=True):
    """Gaussian factors and queries; every query excludes a few of its own unexcluded top-k, a few others and
    an unknown id (with_excl)."""
    rng = np.random.default_rng([seed, n_dst, n_q, k, rank])
    ids = _ids(rng, n_dst)
    F = rng.standard_normal((n_dst, rank)).astype(np.float32)
    q = rng.standard_normal((n_q, rank)).astype(np.float32)
    case = dict(dst_ids=ids, F=F, q=q, k=k, excl=None)
    if with_excl:
        top = expected(case)[0]
        excl = []
        for i in range(n_q):
            t = top[i][top[i] != -1] if n_dst > 1 else top[i][:0]
            mine = t[::3]
            other = rng.choice(ids, min(3, n_dst), replace=False) if n_dst > 3 else ids[:0]
            excl.append(np.concatenate([mine, other, [7777]]).astype(np.int32))
        case["excl"] = excl
    return case


def size(n, k):
    return {"k-1": k - 1, "k": k, "k+1": k + 1}.get(n, n)


def _exact(rng, shape, lo=-16, hi=17):
    """Multiples of 1/8 in [-2, 2]: products and short sums are exact in fp32."""
    return (rng.integers(lo, hi, shape) / 8.0).astype(np.float32)


def boundary_tie_case(k=10, rank=6):
    """One dst factor row repeated 3k times, every fourth row from row 240 of 400: four copies in the first
    slice of 256 rows, the others in the second.  Four more rows score twice as much.  Query 0 excludes those
    four: its list is the k lowest ids of the copies, from both slices.  Query 1 lists the four and then the
    k - 4 lowest copies, the tie sitting at the list's end.  Query 2 also excludes one kept member of the tie."""
    rng = np.random.default_rng(11)
    n = 400
    ids = _ids(rng, n)
    F = _exact(rng, (n, rank), -4, 5)  # |component| <= 0.5: such a row scores at most 4.125
    rep = np.arange(240, 240 + 12 * k, 4)
    assert rep.size == 3 * k and np.sum(rep < SLICE_ROWS) == 4 and rep[-1] < n
    F[rep] = np.array([2, -1.5, 1, 0.5, -2, 1.25][:rank], np.float32)  # scores 13.0625 against itself
    better = np.array([3, 150, 301, 390])
    F[better] = 2 * F[rep[0]]
    q = np.tile(F[rep[0]], (3, 1))
    excl = [ids[better], np.zeros(0, np.int32), ids[rep[2:3]]]
    return dict(dst_ids=ids, F=F, q=q, k=k, excl=excl, rep=rep, better=better)


def zero_and_sign_case(k=8, rank=5):
    """Query 0 is all zero: every score is +0.0 (products -0.0 included: the sum starts at +0.0), the list is the
    k lowest ids.  Query 1 scores every row negative except six rows that score exactly zero (orthogonal or
    all-zero rows, some through -0.0 products)."""
    rng = np.random.default_rng(12)
    n = 300
    ids = _ids(rng, n)
    F = -np.abs(_exact(rng, (n, rank), 1, 17))      # all components negative
    zero = np.array([5, 100, 255, 256, 257, 299])
    F[zero] = 0.0
    F[zero[:3], 0] = np.float32(-0.0)
    F[zero[3], 1] = -1.5                              # orthogonal to query 1, which is zero there
    q = np.zeros((2, rank), np.float32)
    q[1] = np.abs(_exact(rng, (rank,), 1, 17))
    q[1, 1] = 0.0
    return dict(dst_ids=ids, F=F, q=q, k=k, excl=None, zero=zero)


def nonfinite_case(k=6, rank=4):
    """Row 10 holds a NaN (never listed), row 20 scores +inf and row 280 -inf for query 0; query 1 is zero in
    the infinite component's column, so rows 20 and 280 score NaN for it (inf * 0) and are dropped too."""
    rng = np.random.default_rng(13)
    n = 290
    ids = _ids(rng, n)
    F = _exact(rng, (n, rank))
    F[:, 2] = np.abs(F[:, 2])
    F[10, 1] = np.nan
    F[20, 2] = np.inf
    F[280, 2] = -np.inf
    q = np.array([[0.5, -1, 1, 2], [1, 0.25, 0, -1]], np.float32)
    # k = 6 of 290 rows: -inf is listed only when few rows are left, which query 2 arranges by exclusion
    q = np.vstack([q, q[0]])
    excl = [np.zeros(0, np.int32), np.zeros(0, np.int32), np.delete(ids, [10, 20, 100, 280])]
    return dict(dst_ids=ids, F=F, q=q, k=k, excl=excl)


def exclusion_case(k=7, rank=6):
    """The exclusion contract, one query each on 300 distinct-score rows:
      0  three rows outside its top-k                        1  an empty range between non-empty ones
      2  its whole unexcluded top-k                          3  every dst row (all padding)
      4  all but k - 1 rows (short list)                     5  copies and unknown ids in the list
      6  ids INT32_MIN / INT32_MAX, which the catalogue holds 7  query 5's list shuffled"""
    rng = np.random.default_rng(14)
    n = 300
    ids = _ids(rng, n)
    ids[0], ids[-1] = I32_MIN, I32_MAX
    F = rng.standard_normal((n, rank)).astype(np.float32)
    F[0] *= 50.0
    F[-1] = 1.5 * F[0]
    q = np.tile(F[0], (8, 1)).astype(np.float32)  # the two edge ids lead every unexcluded list
    base = dict(dst_ids=ids, F=F, q=q, k=k, excl=None)
    top = expected(base)[0]
    unknown = np.array([I32_MIN + 1, 4999999, -4999999], np.int32)
    assert not np.isin(unknown, ids).any()
    e5 = np.concatenate([top[5][:3], top[5][:3], unknown, top[5][1:2], ids[100:110], unknown[:1]]).astype(np.int32)
    excl = [ids[150:153], np.zeros(0, np.int32), top[2].copy(), ids.copy(), rng.permutation(ids)[: n - (k - 1)],
            e5, np.array([I32_MAX, I32_MIN], np.int32), np.random.default_rng(5).permutation(e5)]
    return dict(dst_ids=ids, F=F, q=q, k=k, excl=excl, unexcluded_top=top)


def shuffled(case, seed=3):
    """The same case with every exclusion list shuffled."""
    rng = np.random.default_rng(seed)
    out = dict(case)
    out["excl"] = [rng.permutation(np.asarray(e, np.int32)) for e in case["excl"]]
    return out


def own_factor_case(rank=8, n=300):
    """Item factors of unit norm but one of norm 3: that item's own factor scores itself 9 and any other item
    at most 3 (Cauchy-Schwarz), so it comes first, far above fp32 rounding."""
    rng = np.random.default_rng(15)
    ids = _ids(rng, n)
    F = rng.standard_normal((n, rank)).astype(np.float32)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    lead = 120
    F[lead] *= np.float32(3.0)
    return dict(dst_ids=ids, F=F, q=F[lead:lead + 1].copy(), k=5, excl=None, lead=lead)
