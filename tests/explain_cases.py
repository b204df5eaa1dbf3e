"""Shared pieces of the als_explain tests (tests/test_gpu_explain.py on the GPU, tests/test_explain_cases.py on
the CPU): `expected`, the fp64 numpy restatement of the definition in include/albedo_als.h, the pairs of each
case, and `check_pair`, the rule by which a returned list is compared.

For row j with the surviving triples (y_i, r_i) in CSR order (tests/foldin_cases.py:fold_csr) and a target t:
  A = G + sum_i c_i y_i y_i^T + regParam·n·I      (c, w, n and G as als_audit_rows defines them)
  z = A^-1 y_t                                     (numpy.linalg.cholesky and two triangular solves)
  e_i = w_i · sum_m y_i[m]·z[m]                    (ascending m, each rating from its own (w_i, y_i) and z)
The sum over m is a loop of element-wise operations, so e_i does not depend on where rating i stands in the
row: two ratings with equal factor rows and equal ratings give equal bits.

The arithmetic of the device is not specified to the bit, so the comparison is tolerant: with `scale` the
pair's largest |e_ref|,
  1. the returned list is sorted by its own (value desc, id asc), and the padding (id -1, value NaN) comes last;
  2. every listed value is within TOL·scale of the reference value of that (row, src, copy);
  3. no surviving triple left off the list has a reference value above the list's last value + TOL·scale;
  4. |total - sum e_ref| <= TOL·sum|e_ref|.
TOL = 1e-10 is the bar tests/test_gpu_audit.py holds against its numpy restatement; two fp64 routes of this
reference (Cholesky with two triangular solves, numpy.linalg.solve) differ by at most 5.6e-12·scale over the
ladder cases below (stars_signed at rank 256; 1.9e-13 below rank 256; tests/test_explain_cases.py asserts 1e-11),
where cond(A) is at most 87.
"""
import functools

import numpy as np

from tests import foldin_cases as FC
from tests import ladder as LD

EXPLAIN_TB = 8   # kernels.h: targets a workgroup solves and scores at a time
MAX_M = 64       # kernels.h EXPLAIN_MAX_M
TOL = 1e-10
MODES = FC.MODES
RANKS = FC.RANKS


def weights(val, *, alpha, implicit):
    """(c, w, n) of a row's ratings as als_audit_rows defines them, in fp64."""
    r = np.asarray(val, np.float32).astype(np.float64)
    if implicit:
        c = alpha * np.abs(r)
        return c, np.where(r > 0, 1.0 + c, 0.0), float(np.sum(r > 0))
    return np.ones(r.size), r, float(r.size)


def _forward(L, B):
    """L U = B, column by column."""
    U = B.copy()
    for j in range(L.shape[0]):
        U[j] /= L[j, j]
        U[j + 1:] -= L[j + 1:, j, None] * U[j]
    return U


def _backward(L, U):
    """L^T Z = U."""
    Z = U.copy()
    for j in range(L.shape[0] - 1, -1, -1):
        Z[j] /= L[j, j]
        Z[:j] -= L[j, :j, None] * Z[j]
    return Z


def solve_targets(A, Yt, route="cholesky"):
    """z_t = A^-1 y_t for the columns of Yt [k, T]."""
    if route == "cholesky":
        L = np.linalg.cholesky(A)  # raises LinAlgError when A is not positive definite
        return _backward(L, _forward(L, Yt))
    return np.linalg.solve(A, Yt)


def contributions(Yr, w, Z):
    """e [deg, T]: e[i, t] = w_i · sum_m Yr[i, m]·Z[m, t], summed in ascending m by element-wise operations."""
    acc = np.zeros((Yr.shape[0], Z.shape[1]))
    for m in range(Yr.shape[1]):
        acc += Yr[:, m, None] * Z[None, m, :]
    return w[:, None] * acc


def top_list(src, e, m):
    """The m entries of (src ids, e) with the largest e by (value desc, id asc), -1 / NaN padded.  -0.0 and +0.0
    tie (they compare equal)."""
    o = np.lexsort((src, -(e + 0.0)))[:m]
    ids = np.full(m, -1, np.int32)
    val = np.full(m, np.nan)
    ids[:o.size], val[:o.size] = src[o], e[o]
    return ids, val


class Ref:
    """total [P], ids / val [P, m], and per pair the (src raw ids, e) of every surviving triple of its row in CSR
    order (None for a pair that cannot be explained)."""

    def __init__(self, n_pairs, m):
        self.total = np.full(n_pairs, np.nan)
        self.ids = np.full((n_pairs, m), -1, np.int32)
        self.val = np.full((n_pairs, m), np.nan)
        self.full = [None] * n_pairs


def expected(Ysrc, src_ids, row_id, src_id, rating, pair_row, pair_target, m, *, reg, alpha, implicit,
             route="cholesky"):
    """The definition of als_explain for these triples and pairs against Ysrc (rows of the ascending src_ids)."""
    src_ids = np.asarray(src_ids, np.int32)
    pair_row, pair_target = np.asarray(pair_row, np.int32), np.asarray(pair_target, np.int32)
    Y = np.asarray(Ysrc, np.float32).astype(np.float64)
    out = Ref(pair_row.size, m)
    if np.asarray(row_id).size == 0 or pair_row.size == 0:
        return out
    ids, ptr, col, val, deg = FC.fold_csr(row_id, src_id, rating, src_ids)
    G = Y.T @ Y if implicit else np.zeros((Y.shape[1], Y.shape[1]))
    pj = np.searchsorted(ids, pair_row)
    row_ok = ids[np.minimum(pj, ids.size - 1)] == pair_row
    pt = np.searchsorted(src_ids, pair_target)
    tgt_ok = src_ids[np.minimum(pt, src_ids.size - 1)] == pair_target
    valid = row_ok & tgt_ok
    for j in np.unique(pj[valid]):
        ps = np.nonzero(valid & (pj == j))[0]
        c0, c1 = ptr[j], ptr[j + 1]
        if c1 == c0:  # no surviving triple: a sum of nothing
            for p in ps:
                out.total[p] = 0.0
                out.full[p] = (np.zeros(0, np.int32), np.zeros(0))
            continue
        Yr = Y[col[c0:c1]]
        c, w, n = weights(val[c0:c1], alpha=alpha, implicit=implicit)
        A = G + (Yr.T * c) @ Yr + reg * n * np.eye(Y.shape[1])
        Z = solve_targets(A, np.ascontiguousarray(Y[pt[ps]].T), route)
        E = contributions(Yr, w, Z)
        src = src_ids[col[c0:c1]]
        for q, p in enumerate(ps):
            e = np.ascontiguousarray(E[:, q])
            t = 0.0
            for v in e.tolist():  # CSR order, one fixed order of addition
                t += v
            out.total[p] = t
            out.ids[p], out.val[p] = top_list(src, e, m)
            out.full[p] = (src, e)
    return out


def check_pair(total, ids, val, full, m, tol=TOL, what=""):
    """The comparison rule of the module docstring for one pair; returns (worst |value - reference| / scale,
    |total - reference| / sum|e_ref|), 0 where the scale is 0 and the values are equal."""
    ids, val = np.asarray(ids), np.asarray(val, np.float64)
    assert ids.shape == (m,) and val.shape == (m,), what
    if full is None:  # cannot be explained
        assert np.isnan(total) and np.all(ids == -1) and np.all(np.isnan(val)), what
        return 0.0, 0.0
    src, e = full
    scale = float(np.max(np.abs(e))) if e.size else 0.0
    n = min(m, e.size)
    # 1. its own order, the padding last
    assert not np.isnan(val[:n]).any() and np.all(np.isnan(val[n:])) and np.all(ids[n:] == -1), what
    lv, li = val[:n], ids[:n].astype(np.int64)
    assert _sorted(lv, li), f"{what}: the list is not in (value desc, id asc) order"
    # 2. every listed value against the reference of that (row, src, copy): the copies of a src, best first
    worst = 0.0
    ro = np.lexsort((-e, src))  # the reference by (src asc, value desc); the list likewise
    rs, re = src.astype(np.int64)[ro], e[ro]
    lo = np.lexsort((-lv, li))
    ls, lvs = li[lo], lv[lo]
    at = np.searchsorted(rs, ls, "left") + (np.arange(n) - np.searchsorted(ls, ls, "left"))  # the c-th copy
    assert np.all(at < np.searchsorted(rs, ls, "right")), f"{what}: an id is listed more often than the row has it"
    if n:
        d = float(np.max(np.abs(lvs - re[at])))
        assert d <= tol * scale, f"{what}: a listed value is off by {d:.3e}, scale {scale:.3e}"
        worst = d / scale if scale > 0 else 0.0
    # 3. nothing better was left off
    left = np.ones(e.size, bool)
    left[at] = False
    if left.any():
        assert n == m and re[left].max() <= lv[-1] + tol * scale, f"{what}: {re[left].max()} left off, last {lv[-1]}"
    # 4. the total
    tref, tabs = float(np.sum(e)), float(np.sum(np.abs(e)))
    assert abs(total - tref) <= tol * tabs, f"{what}: total {total} reference {tref}"
    return worst, (abs(total - tref) / tabs if tabs > 0 else 0.0)


def _sorted(v, i):
    """(value desc, id asc), -0.0 and +0.0 tied."""
    return all(v[a] > v[a + 1] or (v[a] == v[a + 1] and i[a] <= i[a + 1]) for a in range(v.size - 1))


def check_all(got, ref, m, tol=TOL, what=""):
    """check_pair over a call's pairs; returns the worst value and total errors."""
    total, ids, val = got
    assert total.shape == ref.total.shape, what
    wv = wt = 0.0
    for p in range(total.size):
        a, b = check_pair(total[p], ids[p], val[p], ref.full[p], m, tol, f"{what} pair {p}")
        wv, wt = max(wv, a), max(wt, b)
    return wv, wt


# ---- the cases ---------------------------------------------------------------------------------------------

def pairs_for(row_id, src_id, src_ids, n_random, n_own, seed=31):
    """Per distinct row: n_random targets drawn from src_ids and n_own of the row's own (known) sources."""
    rng = np.random.default_rng(seed)
    row_id, src_id = np.asarray(row_id, np.int32), np.asarray(src_id, np.int32)
    src_ids = np.asarray(src_ids, np.int32)
    o = np.argsort(row_id, kind="stable")
    rs, ss = row_id[o], src_id[o]
    starts = np.concatenate([[0], np.nonzero(np.diff(rs))[0] + 1, [rs.size]])
    pr, pt = [], []
    for a, b in zip(starts[:-1], starts[1:]):
        own = ss[a:b][np.isin(ss[a:b], src_ids)]
        t = [rng.choice(src_ids, min(n_random, src_ids.size), replace=False)]
        if own.size and n_own:
            t.append(rng.choice(own, min(n_own, own.size), replace=False))
        t = np.concatenate(t).astype(np.int32)
        pr.append(np.full(t.size, rs[a], np.int32))
        pt.append(t)
    return np.concatenate(pr), np.concatenate(pt)


@functools.lru_cache(maxsize=None)
def ladder_case(mode, k, side):
    """The fold-in ladder (side 1: the 52 item rows as new items against ~700 unit-row user factors; side 0: the
    ~700 users against 52 item factors) with 8 random targets and 2 of its own sources per row.  Returns
    (src_ids, Y, triples, pairs, kw)."""
    implicit, alpha, reg = LD.MODES[mode]
    B = FC.data(mode)[3]
    src_ids = B.user_ids if side == 1 else B.item_ids
    Y = FC.src_factors(k, len(src_ids), seed=side)
    t = FC.ladder_items(mode) if side == 1 else FC.ladder_users(mode)
    pr, pt = pairs_for(t[0], t[1], src_ids, 8, 2)
    for a in (pr, pt):
        a.setflags(write=False)
    return src_ids, Y, t, (pr, pt), dict(reg=reg, alpha=alpha, implicit=implicit)


@functools.lru_cache(maxsize=None)
def ladder_expected(mode, k, side, m=10, route="cholesky"):
    src_ids, Y, t, (pr, pt), kw = ladder_case(mode, k, side)
    return expected(Y, src_ids, *t, pr, pt, m, route=route, **kw)


UNKNOWN_ROW = 424242  # occurs in no triple of contract_pairs' case


def contract_pairs(src_ids, seed=33):
    """Pairs over foldin_cases.contract_case: every row (ids at both ends of int32 and -1, the degree-0 row 77,
    the rows with 2, 3 and 64 copies of src_ids[7]) with 3 random targets and, where it has one, one of its own
    sources; the copied source as a target; an unknown target; an unknown row; one pair given twice."""
    src_ids = np.asarray(src_ids, np.int32)
    row, src, r = FC.contract_case(src_ids)
    pr, pt = pairs_for(row, src, src_ids, 3, 1, seed)
    unk = FC.unknown_sources(src_ids, 8)[0]
    extra_r = [100, 101, 102, -1, UNKNOWN_ROW, UNKNOWN_ROW, pr[0]]
    extra_t = [src_ids[7], src_ids[7], src_ids[7], unk, src_ids[0], unk, pt[0]]
    return (np.concatenate([pr, np.array(extra_r, np.int32)]), np.concatenate([pt, np.array(extra_t, np.int32)]))


def tie_factors(Y, a=3, b=11):
    """Y with row b made a copy of row a: two src ids with identical factor rows."""
    Y = np.array(Y, np.float32)
    Y[b] = Y[a]
    return Y


def tie_case(src_ids, a=3, b=11, seed=41):
    """One row (id 555) of 20 ratings that rates the src rows a and b equally (with tie_factors their
    contributions are equal bits), and three targets.  Returns (triples, pairs)."""
    rng = np.random.default_rng(seed)
    src_ids = np.asarray(src_ids, np.int32)
    others = np.setdiff1d(np.arange(src_ids.size), [a, b])
    s = np.concatenate([[b, a], rng.choice(others, 18, replace=False)])
    r = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], s.size).astype(np.float32)
    r[0] = r[1] = 4.0
    p = rng.permutation(s.size)
    row = np.full(s.size, 555, np.int32)
    tg = np.array([src_ids[a], src_ids[others[0]], src_ids[others[5]]], np.int32)
    return (row, src_ids[s[p]], r[p]), (np.full(tg.size, 555, np.int32), tg)
