"""ctypes binding of libalbedo_als.so (include/albedo_als.h).

The library is built in-tree (`albedo_amd/libalbedo_als.so`, see `__graft_entry__.build`).  There is
no CPU fallback: when the library or a gfx950 device is missing, engine calls raise.

If the same process uses PyTorch, import torch BEFORE albedo_amd: torch ships its own HIP runtime
(soname libamdhip64.so.7) and loading it after ours would put two HIP runtimes in one process.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALBEDO_ALS_LIB", os.path.join(_HERE, "libalbedo_als.so"))

ALS_OK = 0
ALS_E_INVALID_ARGUMENT = 1
ALS_E_NOT_POSITIVE_DEFINITE = 2
ALS_E_STATE = 3
ALS_E_HIP = 4
ALS_E_RCCL = 5
ALS_E_OUT_OF_MEMORY = 6
ALS_E_NO_DEVICE = 7
ALS_E_UNSUPPORTED = 8
ALS_USER, ALS_ITEM = 0, 1
ALS_METRIC_NDCG, ALS_METRIC_PRECISION, ALS_METRIC_MAP = 0, 1, 2
ALS_EXCLUDE_RATINGS, ALS_EXCLUDE_PAIRS = 0, 1
METRICS = {"NDCG@k": ALS_METRIC_NDCG, "Precision@k": ALS_METRIC_PRECISION, "MAP": ALS_METRIC_MAP}
ALS_T_COUNT = 8
# als_audit.worst_path: the solve path the row layout routes a row to (ALS_PATH_* in order)
PATH_NAMES = ["light16-pair", "light16", "light32", "light48", "light64", "light96", "tier80", "explicit", "split",
              "nnls-lockstep", "nnls-row"]
(ALS_PATH_LIGHT16_PAIR, ALS_PATH_LIGHT16, ALS_PATH_LIGHT32, ALS_PATH_LIGHT48, ALS_PATH_LIGHT64, ALS_PATH_LIGHT96,
 ALS_PATH_TIER80, ALS_PATH_EXPLICIT, ALS_PATH_SPLIT, ALS_PATH_NNLS_LOCKSTEP, ALS_PATH_NNLS_ROW) = range(11)
T_NAMES = ["gram", "eig", "rotate", "comm", "solve_light", "solve_heavy", "half_total", "_"]


class als_params(C.Structure):
    _fields_ = [
        ("rank", C.c_int32),
        ("max_iter", C.c_int32),
        ("implicit_prefs", C.c_int32),
        ("nonnegative", C.c_int32),
        ("num_user_blocks", C.c_int32),
        ("num_item_blocks", C.c_int32),
        ("reg_param", C.c_double),
        ("alpha", C.c_double),
        ("seed", C.c_int64),
        ("device", C.c_int32),
        ("light_max_degree", C.c_int32),
    ]


class als_audit(C.Structure):
    _fields_ = [
        ("rows", C.c_int64),
        ("rows_over", C.c_int64),
        ("non_finite", C.c_int64),
        ("negative", C.c_int64),
        ("worst_degree", C.c_int64),
        ("worst_id", C.c_int32),
        ("worst_path", C.c_int32),
        ("worst_eta", C.c_double),
        ("sum_eta", C.c_double),
    ]


class als_objective_t(C.Structure):
    _fields_ = [
        ("total", C.c_double),
        ("all_pairs", C.c_double),
        ("ratings", C.c_double),
        ("reg_side", C.c_double),
        ("reg_other", C.c_double),
        ("sse", C.c_double),
        ("abs_terms", C.c_double),
        ("n_ratings", C.c_int64),
        ("rows", C.c_int64),
    ]


class als_fold_params(C.Structure):
    _fields_ = [
        ("reg_param", C.c_double),
        ("alpha", C.c_double),
        ("implicit_prefs", C.c_int32),
        ("nonnegative", C.c_int32),
    ]


class ALSError(RuntimeError):
    """Base class; `code` is the ALS_E_* value."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class IllegalArgumentException(ALSError, ValueError):
    """Spark's IllegalArgumentException (ParamValidators, empty ratings, dppsv not-PD)."""


class IllegalStateException(ALSError):
    pass


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int64)

# (name, restype, argtypes) — every entry point of include/albedo_als.h
P = C.c_void_p
I32P = C.POINTER(C.c_int32)
I64P = C.POINTER(C.c_int64)
F32P = C.POINTER(C.c_float)
F64P = C.POINTER(C.c_double)
SIGNATURES = [
    ("als_params_default", C.c_int, [C.POINTER(als_params)]),
    ("als_create", C.c_int, [C.POINTER(als_params), C.POINTER(P)]),
    ("als_destroy", None, [P]),
    ("als_set_params", C.c_int, [P, C.POINTER(als_params)]),
    ("als_fork", C.c_int, [P, C.POINTER(als_params), C.POINTER(P)]),
    ("als_last_error", C.c_char_p, []),
    ("als_abi_version", C.c_int, []),
    ("als_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("als_comm_unique_id", C.c_int, [P]),
    ("als_comm_init", C.c_int, [P, C.c_int32, C.c_int32, P]),
    ("als_set_ratings", C.c_int, [P, C.c_int64, I32P, I32P, F32P]),
    ("als_set_ratings_device", C.c_int, [P, C.c_int64, P, P, P]),
    ("als_num_rows", C.c_int64, [P, C.c_int]),
    ("als_num_ratings", C.c_int64, [P]),
    ("als_rank", C.c_int, [P]),
    ("als_get_ids", C.c_int, [P, C.c_int, I32P]),
    ("als_set_initial_factors", C.c_int, [P, C.c_int, C.c_int64, I32P, F32P]),
    ("als_init_factors", C.c_int, [P]),
    ("als_init_factors_random", C.c_int, [P, C.c_uint64]),
    ("als_get_factors", C.c_int, [P, C.c_int, I32P, F32P]),
    ("als_fit", C.c_int, [P]),
    ("als_run_sweeps", C.c_int, [P, C.c_int32]),
    ("als_half_sweep", C.c_int, [P, C.c_int]),
    ("als_get_gram", C.c_int, [P, C.c_int, F64P]),
    ("als_get_degrees", C.c_int, [P, C.c_int, I64P]),
    ("als_get_row_ratings", C.c_int, [P, C.c_int, C.c_int32, C.c_int64, I32P, F32P, I64P]),
    ("als_model_create", C.c_int, [C.c_int32, C.c_int64, I32P, F32P, C.c_int64, I32P, F32P, C.c_int32, C.POINTER(P)]),
    ("als_recommend", C.c_int, [P, C.c_int, C.c_int32, I32P, C.c_int64, I32P, I32P, F32P]),
    ("als_predict", C.c_int, [P, C.c_int64, I32P, I32P, F32P]),
    ("als_fold_in", C.c_int, [P, C.c_int, C.POINTER(als_fold_params), C.c_int64, I32P, I32P, F32P, C.c_int64, I64P, I32P,
                              I64P, F32P]),
    ("als_fold_in_timing", C.c_int, [P, F64P]),
    ("als_fold_in_stats", C.c_int, [P, I64P]),
    ("als_explain", C.c_int, [P, C.c_int, C.POINTER(als_fold_params), C.c_int64, I32P, I32P, F32P, C.c_int64, I32P, I32P,
                              C.c_int32, F64P, I32P, F64P]),
    ("als_explain_timing", C.c_int, [P, F64P]),
    ("als_recommend_vectors", C.c_int, [P, C.c_int, C.c_int32, C.c_int64, F32P, I64P, I32P, I32P, F32P]),
    ("als_recommend_vectors_timing", C.c_int, [P, F64P]),
    ("als_recommend_unseen", C.c_int, [P, C.c_int, C.c_int32, I32P, C.c_int64, C.c_int32, C.c_int64, I32P, I32P, I32P,
                                       I32P, F32P]),
    ("als_recommend_unseen_stats", C.c_int, [P, I64P]),
    ("als_recommend_unseen_timing", C.c_int, [P, F64P]),
    ("als_similar", C.c_int, [P, C.c_int, C.c_int32, I32P, C.c_int64, I32P, I32P, F32P]),
    ("als_similar_vectors", C.c_int, [P, C.c_int, C.c_int32, C.c_int64, F32P, I64P, I32P, I32P, F32P]),
    ("als_similar_timing", C.c_int, [P, F64P]),
    ("als_similar_stats", C.c_int, [P, I64P]),
    ("als_evaluate_ndcg", C.c_int, [P, C.c_int32, C.c_int64, I32P, I32P, I64P, F64P, I64P, I32P, F64P, C.c_int64]),
    ("als_evaluate_ranking", C.c_int, [P, C.c_int32, C.c_int32, C.c_int64, I32P, I32P, I64P, F64P, I64P, I32P, F64P,
                                       C.c_int64]),
    ("als_rank_pairs", C.c_int, [P, C.c_int32, C.c_int32, C.c_int64, I32P, I32P, I64P, I32P, I32P, I32P, F32P,
                                 C.c_int64]),
    ("als_evaluate_pairs", C.c_int, [P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, I32P, I32P, C.c_int64, I32P, I32P,
                                     I64P, F64P, I64P, I32P, F64P, C.c_int64]),
    ("als_eval_pairs_timing", C.c_int, [P, F64P]),
    ("als_last_timings", C.c_int, [P, C.c_int, F64P, C.c_int]),
    ("als_path_stats", C.c_int, [P, C.c_int, I64P]),
    ("als_solver_stats", C.c_int, [P, C.c_int, I64P]),
    ("als_audit_rows", C.c_int, [P, C.c_int, C.c_double, F64P, C.POINTER(als_audit)]),
    ("als_objective", C.c_int, [P, C.c_int, F64P, C.POINTER(als_objective_t)]),
    ("als_objective_timing", C.c_int, [P, F64P]),
    ("als_fit_tracked", C.c_int, [P, C.c_double, C.c_int32, F64P, I32P, I32P]),
    ("als_topk_stats", C.c_int, [P, I64P]),
    ("als_topk_timing", C.c_int, [P, F64P]),
    ("als_get_basis", C.c_int, [P, C.c_int, F64P]),
    ("als_topk_last_rescan", C.c_int, [P, I32P, C.c_int64, I64P]),
    ("als_synchronize", C.c_int, [P]),
    ("als_synth_generate", C.c_int, [C.c_int32, C.c_uint64, C.c_int32, C.c_int64, C.c_int64, I64P, F64P, I32P,
                                     I32P, I32P, F32P, I64P]),
    ("als_set_ratings_synthetic", C.c_int, [P, C.c_uint64, C.c_int32, C.c_int64, C.c_int64, I64P, F64P, I32P]),
    ("als_comm_init_host", C.c_int, [P, C.c_int32, C.c_int32, ALLREDUCE_FN, ALLGATHER_FN, P]),
    ("als_host_eigh", C.c_int, [C.c_int32, F64P, F64P, F64P]),
    ("als_device_eigh", C.c_int, [C.c_int32, C.c_int32, F64P, F64P, F64P, F64P, I32P]),
    ("als_host_spark_side_seeds", C.c_int, [C.c_int64, I64P, I64P]),
    ("als_host_spark_init", C.c_int, [I32P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, F32P]),
    ("als_host_plan_shards", C.c_int, [I64P, C.c_int64, C.c_int32, I64P]),
]

_lib = None


def load():
    """Load (once) and return the ctypes library; raises ImportError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the ALS engine has no CPU fallback)")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc == ALS_OK:
        return
    msg = load().als_last_error().decode("utf-8", "replace")
    if rc in (ALS_E_INVALID_ARGUMENT, ALS_E_NOT_POSITIVE_DEFINITE):
        raise IllegalArgumentException(rc, msg)
    if rc == ALS_E_STATE:
        raise IllegalStateException(rc, msg)
    raise ALSError(rc, msg)


def ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def device_count() -> int:
    n = C.c_int(0)
    check(load().als_device_count(C.byref(n)))
    return n.value



def fold_in(ctx, side, row_id, src_id, rating, rank, reg_param=None, alpha=None, implicit_prefs=None, cap=None,
            nonnegative=None):
    """als_fold_in on the context handle `ctx`: (ids ascending, degrees, factors [n_rows][rank]) of the distinct
    row ids.  The three parameters go together: all None means the context's own (fp = NULL).  cap: an upper
    bound of the number of distinct row ids the caller knows (default: they are counted here).  nonnegative
    (with the three parameters): solve each row by Spark's NNLS in place of the Cholesky; None is False."""
    import numpy as np

    row_id = np.ascontiguousarray(row_id, dtype=np.int32)
    src_id = np.ascontiguousarray(src_id, dtype=np.int32)
    rating = np.ascontiguousarray(rating, dtype=np.float32)
    n = int(row_id.shape[0])
    if src_id.shape != (n,) or rating.shape != (n,):
        raise ValueError("row_id, src_id and rating should be one-dimensional and of one length")
    given = [v is not None for v in (reg_param, alpha, implicit_prefs)]
    fp = None
    if any(given):
        if not all(given):
            raise ValueError("reg_param, alpha and implicit_prefs are given together or not at all")
        fp = C.byref(als_fold_params(float(reg_param), float(alpha), int(bool(implicit_prefs)), int(bool(nonnegative))))
    elif nonnegative is not None:
        raise ValueError("nonnegative goes with reg_param, alpha and implicit_prefs (als_fold_params)")
    cap = int(np.unique(row_id).size) if cap is None else int(cap)
    ids = np.empty(cap, dtype=np.int32)
    deg = np.empty(cap, dtype=np.int64)
    fac = np.empty((cap, rank), dtype=np.float32)
    nr = C.c_int64(0)
    check(load().als_fold_in(ctx, side, fp, n, ptr(row_id, C.c_int32), ptr(src_id, C.c_int32), ptr(rating, C.c_float),
                             cap, C.byref(nr), ptr(ids, C.c_int32), ptr(deg, C.c_int64), ptr(fac, C.c_float)))
    if nr.value > cap:
        raise ValueError(f"fold_in: {nr.value} distinct row ids, cap {cap}")
    return ids[:nr.value].copy(), deg[:nr.value].copy(), fac[:nr.value].copy()


def fit_tracked(ctx, max_iter, tol=None):
    """als_fit_tracked on the context handle `ctx`: (objective history as a list of floats, entry 0 = after the
    initialisation; sweeps run).  tol None: every sweep runs."""
    import numpy as np

    cap = int(max_iter) + 1
    hist = np.empty(cap, dtype=np.float64)
    n, ran = C.c_int32(0), C.c_int32(0)
    check(load().als_fit_tracked(ctx, 0.0 if tol is None else float(tol), cap, ptr(hist, C.c_double), C.byref(n),
                                 C.byref(ran)))
    return hist[:n.value].tolist(), int(ran.value)


def fold_in_timing(ctx):
    """als_fold_in_timing: device ms of the last call: [map + sort + CSR, src Gram, solve, total]."""
    import numpy as np

    out = np.zeros(4, dtype=np.float64)
    check(load().als_fold_in_timing(ctx, ptr(out, C.c_double)))
    return out


def fold_in_stats(ctx):
    """als_fold_in_stats: NNLS iterations of the last call: [sum over rows, maximum, rows solved by NNLS, rows at
    the iteration limit]; zeros after a Cholesky fold-in."""
    import numpy as np

    out = np.zeros(4, dtype=np.int64)
    check(load().als_fold_in_stats(ctx, ptr(out, C.c_int64)))
    return out


def explain(ctx, side, row_id, src_id, rating, pair_row_id, pair_target_id, m, reg_param=None, alpha=None,
            implicit_prefs=None):
    """als_explain on the context handle `ctx`: (totals [n_pairs], src ids [n_pairs, m], contributions
    [n_pairs, m]) of the pairs (row, target of the src side) over the rows the triples describe, -1 / NaN padded.
    The three parameters go together, as in fold_in: all None means the context's own (fp = NULL)."""
    import numpy as np

    row_id = np.ascontiguousarray(row_id, dtype=np.int32)
    src_id = np.ascontiguousarray(src_id, dtype=np.int32)
    rating = np.ascontiguousarray(rating, dtype=np.float32)
    pair_row_id = np.ascontiguousarray(pair_row_id, dtype=np.int32)
    pair_target_id = np.ascontiguousarray(pair_target_id, dtype=np.int32)
    n, n_pairs, m = int(row_id.shape[0]), int(pair_row_id.shape[0]), int(m)
    if row_id.ndim != 1 or src_id.shape != (n,) or rating.shape != (n,):
        raise ValueError("row_id, src_id and rating should be one-dimensional and of one length")
    if pair_row_id.ndim != 1 or pair_target_id.shape != (n_pairs,):
        raise ValueError("pair_row_id and pair_target_id should be one-dimensional and of one length")
    given = [v is not None for v in (reg_param, alpha, implicit_prefs)]
    fp = None
    if any(given):
        if not all(given):
            raise ValueError("reg_param, alpha and implicit_prefs are given together or not at all")
        fp = C.byref(als_fold_params(float(reg_param), float(alpha), int(bool(implicit_prefs)), 0))
    total = np.empty(n_pairs, dtype=np.float64)
    ids = np.empty((n_pairs, max(m, 0)), dtype=np.int32)
    contrib = np.empty((n_pairs, max(m, 0)), dtype=np.float64)
    check(load().als_explain(ctx, side, fp, n, ptr(row_id, C.c_int32), ptr(src_id, C.c_int32), ptr(rating, C.c_float),
                             n_pairs, ptr(pair_row_id, C.c_int32), ptr(pair_target_id, C.c_int32), m,
                             ptr(total, C.c_double), ptr(ids, C.c_int32), ptr(contrib, C.c_double)))
    return total, ids, contrib


def explain_timing(ctx):
    """als_explain_timing: device ms of the last call: [map + sort + CSR, src Gram, solve + select, total]."""
    import numpy as np

    out = np.zeros(4, dtype=np.float64)
    check(load().als_explain_timing(ctx, ptr(out, C.c_double)))
    return out


def exclusion_csr(exclude, n_q):
    """The (ptr int64 [n_q + 1], ids int32) pair als_recommend_vectors takes, from None, a (ptr, ids) pair or
    a list of n_q id arrays."""
    import numpy as np

    if exclude is None:
        return None, None
    if isinstance(exclude, tuple):  # a tuple is always the pair; id lists come in a list
        if len(exclude) != 2 or len(exclude[0]) != n_q + 1:
            raise ValueError(f"exclude as a tuple should be (ptr [{n_q + 1}], ids)")
        return np.ascontiguousarray(exclude[0], dtype=np.int64), np.ascontiguousarray(exclude[1], dtype=np.int32)
    if len(exclude) != n_q:
        raise ValueError(f"exclude should hold one id list per query: {len(exclude)} lists, {n_q} queries")
    lists = [np.asarray(e, dtype=np.int32).reshape(-1) for e in exclude]
    ptr_ = np.zeros(n_q + 1, dtype=np.int64)
    np.cumsum([e.size for e in lists], out=ptr_[1:])
    ids = np.concatenate(lists) if lists else np.zeros(0, np.int32)
    return ptr_, np.ascontiguousarray(ids, dtype=np.int32)


def recommend_vectors(ctx, side, vectors, k, rank, exclude=None):
    """als_recommend_vectors on the context handle `ctx`: (dst ids [n_q, k], scores [n_q, k]) of the query
    vectors [n_q, rank] against the factors of `side`, -1 / NaN padded."""
    import numpy as np

    q = np.ascontiguousarray(vectors, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] != rank:
        raise ValueError(f"vectors should be [n, {rank}], not {q.shape}")
    n_q = int(q.shape[0])
    ptr_, eids = exclusion_csr(exclude, n_q)
    ids = np.empty((n_q, max(int(k), 0)), dtype=np.int32)
    sc = np.empty((n_q, max(int(k), 0)), dtype=np.float32)
    check(load().als_recommend_vectors(ctx, side, int(k), n_q, ptr(q, C.c_float),
                                       ptr(ptr_, C.c_int64) if ptr_ is not None else None,
                                       ptr(eids, C.c_int32) if eids is not None and eids.size else None,
                                       ptr(ids, C.c_int32), ptr(sc, C.c_float)))
    return ids, sc


def recommend_vectors_timing(ctx):
    """als_recommend_vectors_timing: device ms of the last call: [exclusion map + sort, scan, merge, total]."""
    import numpy as np

    out = np.zeros(4, dtype=np.float64)
    check(load().als_recommend_vectors_timing(ctx, ptr(out, C.c_double)))
    return out


def similar(ctx, side, k, subset=None):
    """als_similar on the context handle `ctx`: (src ids [n], ids [n, k], scores [n, k]) of the cosine top-k of
    the requested rows of `side` (every row when subset is None) among the other rows of that side."""
    import numpy as np

    lib = load()
    if subset is not None:
        sub = np.ascontiguousarray(subset, dtype=np.int32).reshape(-1)
        n = int(sub.size)
    else:
        sub, n = None, int(lib.als_num_rows(ctx, side))
    src = np.empty(n, dtype=np.int32)
    ids = np.empty((n, max(int(k), 0)), dtype=np.int32)
    sc = np.empty((n, max(int(k), 0)), dtype=np.float32)
    check(lib.als_similar(ctx, side, int(k), ptr(sub, C.c_int32) if sub is not None else None, n,
                          ptr(src, C.c_int32), ptr(ids, C.c_int32), ptr(sc, C.c_float)))
    return src, ids, sc


def similar_vectors(ctx, side, vectors, k, rank, exclude=None):
    """als_similar_vectors: recommend_vectors with the cosine of the query and each row of `side` as the score."""
    import numpy as np

    q = np.ascontiguousarray(vectors, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] != rank:
        raise ValueError(f"vectors should be [n, {rank}], not {q.shape}")
    n_q = int(q.shape[0])
    ptr_, eids = exclusion_csr(exclude, n_q)
    ids = np.empty((n_q, max(int(k), 0)), dtype=np.int32)
    sc = np.empty((n_q, max(int(k), 0)), dtype=np.float32)
    check(load().als_similar_vectors(ctx, side, int(k), n_q, ptr(q, C.c_float),
                                     ptr(ptr_, C.c_int64) if ptr_ is not None else None,
                                     ptr(eids, C.c_int32) if eids is not None and eids.size else None,
                                     ptr(ids, C.c_int32), ptr(sc, C.c_float)))
    return ids, sc


def similar_timing(ctx):
    """als_similar_timing: device ms of the last call: [unit image, lists, merge / filter, total]."""
    import numpy as np

    out = np.zeros(4, dtype=np.float64)
    check(load().als_similar_timing(ctx, ptr(out, C.c_double)))
    return out


def similar_stats(ctx):
    """als_similar_stats of the last call: [rows asked and known, rows without a direction, tier, exact-scan rows]."""
    import numpy as np

    out = np.zeros(4, dtype=np.int64)
    check(load().als_similar_stats(ctx, ptr(out, C.c_int64)))
    return out
