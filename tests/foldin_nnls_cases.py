"""Shared pieces of the nonnegative fold-in tests (tests/test_gpu_foldin_nnls.py on the GPU,
tests/test_foldin_nnls_cases.py on the CPU): the cases, and `expected_nnls`, the C oracle's answer for them.

`expected_nnls` is the definition of als_fold_in with als_fold_params.nonnegative = 1: the CSR of the new rows
(tests/foldin_cases.py:fold_csr) through oracle.cbind.solve_rows_nnls, Spark 2.2.0's NNLSSolver per row in
fp64 rounded once to fp32, and zeros for the rows left with no triple.  It comes as a tests/nnls_cases.py Ref
over all the rows, so that nnls_cases.check_rows judges the device rows: every row carries the single path
label PATH.

A case is (src factors, src ids, triples, regParam, alpha, implicitPrefs, side).  CASES names every case the
GPU module runs; the CPU module runs both oracles on each of them.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cbind
from tests import foldin_cases as FC
from tests import ladder as LD
from tests import nnls_cases as NC

PATH = "fold-nnls"
LADDER_RANKS = (1, 8, 50, 64, 65, 128, 129, 200, 256)  # every instance on both sides of each padded rank
USER_RANKS = (50, 128)
KIND_RANKS = (50, 128)
KINDS = ("nonneg", "pos", "neg", "large", "small", "aniso")
KINDS_REG0 = ("nonneg", "pos")  # aniso and small with regParam = 0 are left out: Spark's loop is not well determined there
KIND_MODE = "varying"           # implicit, alpha 10, regParam 0.5

Case = namedtuple("Case", "Y src_ids row src r reg alpha implicit side")


def expected_nnls(Ysrc, src_ids, row_id, src_id, rating, *, reg, alpha, implicit):
    """(ids, degree, Ref) of the nonnegative fold-in of these triples against Ysrc (rows of src_ids): Ref.X the
    fp32 factors and Ref.it the NNLS iterations of every row, zeros for the rows without a surviving triple."""
    ids, ptr, col, val, deg = FC.fold_csr(row_id, src_id, rating, src_ids)
    Ysrc = np.ascontiguousarray(Ysrc, np.float32)
    k = Ysrc.shape[1]
    G = cbind.gram(Ysrc) if implicit else np.zeros((k, k))
    X = np.zeros((ids.size, k), np.float32)
    it = np.zeros(ids.size, np.int32)
    live = deg > 0
    if live.any():  # the rows without a triple hold no entries: col and val serve as they are
        lptr = np.concatenate([[0], np.cumsum(deg[live])]).astype(np.int64)
        X[live], it[live] = cbind.solve_rows_nnls(Ysrc, G, lptr, col, val, reg=reg, alpha=alpha, implicit=implicit)
    ref = NC.Ref(Ysrc, G, ptr, col, val, reg, alpha, implicit, X, it, None, None)
    kkt, floor = NC.row_kkt(ref, X, want_floor=True)
    for a in (X, it, kkt, floor):
        a.setflags(write=False)
    return ids, deg, ref._replace(kkt=kkt, floor=floor)


def ladder_case(mode, k, side):
    """side 1: the ladder's 52 item rows as new items against signed unit-row user factors; side 0: its ~700
    users as new users against 52 unit-row item factors (tests/foldin_cases.py:ladder_expected's inputs)."""
    implicit, alpha, reg = LD.MODES[mode]
    B = FC.data(mode)[3]
    src_ids = B.user_ids if side == 1 else B.item_ids
    row, src, r = FC.ladder_items(mode) if side == 1 else FC.ladder_users(mode)
    return Case(FC.src_factors(k, len(src_ids), seed=side), src_ids, row, src, r, reg, alpha, implicit, side)


def kind_case(kind, k, reg=None):
    """The ladder's item rows against the source kinds of tests/nnls_cases.py:src_factors."""
    implicit, alpha, reg0 = LD.MODES[KIND_MODE]
    B = FC.data(KIND_MODE)[3]
    row, src, r = FC.ladder_items(KIND_MODE)
    return Case(NC.src_factors(kind, len(B.user_ids), k), B.user_ids, row, src, r, reg0 if reg is None else reg, alpha,
                implicit, 1)


def _edge(k, triples):
    implicit, alpha, reg = LD.MODES["varying"]
    src_ids = FC.data("varying")[3].user_ids
    return Case(FC.src_factors(k, len(src_ids), seed=1), src_ids, *triples(src_ids), reg, alpha, implicit, 1)


def tile_case(k):
    return _edge(k, lambda src_ids: FC.degree_rows(FC.tile_degrees(k), src_ids))


def contract_case(k=128):
    return _edge(k, FC.contract_case)


def refill_case(k):
    """60 rows of mixed degrees: with ALBEDO_FOLD_WGS = 1 or 3 every workgroup solves many rows in turn."""
    return _edge(k, lambda src_ids: FC.degree_rows([5, 40, 33, 1, 129, 64, 2, 70, 31, 12] * 6, src_ids, seed=6))


def singular_case(implicit):
    src_ids, Y, row, src, r = FC.singular_case()
    return Case(Y, src_ids, row, src, r, 0.0, 1.0, implicit, 1)


def _cases():
    out = {}
    for mode in FC.MODES:
        for k in LADDER_RANKS:
            out[f"items-{mode}-k{k}"] = functools.partial(ladder_case, mode, k, 1)
        for k in USER_RANKS:
            out[f"users-{mode}-k{k}"] = functools.partial(ladder_case, mode, k, 0)
    for k in KIND_RANKS:
        for kind in KINDS:
            out[f"kind-{kind}-k{k}"] = functools.partial(kind_case, kind, k)
        for kind in KINDS_REG0:
            out[f"kind-{kind}-reg0-k{k}"] = functools.partial(kind_case, kind, k, 0.0)
        out[f"tile-k{k}"] = functools.partial(tile_case, k)
    out["contract-k128"] = contract_case
    out["refill-k128"] = functools.partial(refill_case, 128)
    out["refill-k200"] = functools.partial(refill_case, 200)
    out["singular-implicit"] = functools.partial(singular_case, True)
    out["singular-explicit"] = functools.partial(singular_case, False)
    return out


CASES = _cases()
LADDER_CASES = [n for n in CASES if n.startswith(("items-", "users-"))]
KIND_CASES = [n for n in CASES if n.startswith("kind-")]


def rank_of(name):
    return CASES[name]().Y.shape[1]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ids, degree, Ref) of a named case, computed once."""
    c = case(name)
    return expected_nnls(c.Y, c.src_ids, c.row, c.src, c.r, reg=c.reg, alpha=c.alpha, implicit=c.implicit)
