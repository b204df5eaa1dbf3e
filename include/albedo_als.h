/*
 * albedo_als.h — C ABI of libalbedo_als.so, the MI355X implicit-ALS engine.
 *
 * Drop-in boundary: this library replaces Spark MLlib 2.2.0's
 * `ml.recommendation.ALS` / `ALSModel` as reached from albedo:
 *   - estimator params + fit  : ALSRecommenderBuilder.scala:46-58  (new ALS().setX(...).fit(ds))
 *                               ALSRecommenderCV.scala:46-52, Playground.scala:54-65,
 *                               src/main/python/train_als.py:55-61
 *   - model factors / rank    : ALSRecommender.scala:16-19,33-36  (alsModel.userFactors/itemFactors/rank)
 *   - top-k recommendation    : ALSRecommender.scala:28-65 (+ BoundedPriorityQueue.scala:30-53),
 *                               Spark ALSModel.recommendForAllUsers / recommendForUserSubset
 *   - per-pair prediction     : Spark ALSModel.transform (LogisticRegressionRanker.scala:167-174,229)
 * A JVM would bind these through JNI / Panama; Python binds them via ctypes
 * (albedo_amd/als.py).  No C++ or torch types cross this boundary: plain pointers and sizes.
 *
 * Conventions
 *   - Every function returning int returns ALS_OK (0) or an ALS_E_* code; the message is in
 *     als_last_error() (thread-local, valid until the next failing call on the same thread).
 *   - Host inputs are caller-owned and copied in.  Outputs go to caller-allocated buffers sized
 *     with als_num_rows()/als_rank().  The context owns all device memory.
 *   - A context is not re-entrant; separate contexts may be used from separate threads.
 *   - side: ALS_USER (0) or ALS_ITEM (1).  Factor rows are returned in ascending raw-id order,
 *     row-major [n][rank] float32, exactly like ALSModel.userFactors sorted by id.
 */
#ifndef ALBEDO_ALS_H
#define ALBEDO_ALS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALBEDO_ALS_ABI_VERSION 1

enum {
  ALS_OK = 0,
  ALS_E_INVALID_ARGUMENT = 1, /* Spark: IllegalArgumentException (ParamValidators, "No ratings available") */
  ALS_E_NOT_POSITIVE_DEFINITE = 2, /* Spark: IllegalArgumentException from CholeskyDecomposition (dppsv info>0) */
  ALS_E_STATE = 3,            /* call out of order (e.g. recommend before fit) -> IllegalStateException */
  ALS_E_HIP = 4,              /* HIP runtime failure                -> SparkException/RuntimeException */
  ALS_E_RCCL = 5,             /* RCCL failure */
  ALS_E_OUT_OF_MEMORY = 6,
  ALS_E_NO_DEVICE = 7,        /* no gfx950 device visible: the engine has no CPU fallback */
  ALS_E_UNSUPPORTED = 8       /* e.g. rank above the compiled maximum */
};

enum { ALS_USER = 0, ALS_ITEM = 1 };

/* Spark ALS params (ml/recommendation/ALS.scala ALSParams), defaults as Spark 2.2.0. */
typedef struct als_params {
  int32_t rank;            /* setRank, default 10, >= 1 */
  int32_t max_iter;        /* setMaxIter, default 10, >= 0 */
  int32_t implicit_prefs;  /* setImplicitPrefs, default 0 */
  int32_t nonnegative;     /* setNonnegative, default 0 */
  int32_t num_user_blocks; /* setNumUserBlocks, default 10, >= 1 (only shapes the Spark-style init) */
  int32_t num_item_blocks; /* setNumItemBlocks, default 10, >= 1 */
  double reg_param;        /* setRegParam, default 0.1, >= 0 */
  double alpha;            /* setAlpha, default 1.0, >= 0 */
  int64_t seed;            /* setSeed, default = hash of the class name in Spark; here 0 if unset */
  int32_t device;          /* HIP device ordinal; -1 = current device */
  int32_t light_max_degree;/* rows with <= this many ratings take the rotated push-through solve (capped at
                              96 at rank 65..128, 64 otherwise);
                              -1 = engine default, 0 = every row takes the explicit Cholesky solve.
                              The default limit is 64 at rank 65..256 and 32 below.  At rank 65..128 the
                              default (-1, not nonnegative) also switches on the degree tiers: rows of
                              33..48 ratings use a 48-wide instance of the push-through kernel, and rows of
                              65..80 ratings, which stay above the limit, are solved by an 80-wide instance
                              instead of the explicit solve.  A value >= 0 gives exactly the routing it
                              names (no tiers); ALBEDO_DEGREE_TIERS=0 in the environment switches the tiers
                              off for the default too. */
} als_params;

typedef struct als_ctx als_ctx;

/* ---- lifecycle ---------------------------------------------------------------------------- */
int als_params_default(als_params* p);
int als_create(const als_params* p, als_ctx** out);
void als_destroy(als_ctx* ctx);
/* Replace the params of a context that already holds ratings (Spark Estimator.fit(dataset, paramMaps),
 * ALSRecommenderCV.scala:67-90): the ingest (remap, both CSRs, shards) is kept, rank-dependent
 * buffers and degree buckets are rebuilt and the factors are dropped, so the next als_fit starts
 * from the new seed's initialisation.  Validated like als_create; the device is kept. */
int als_set_params(als_ctx* ctx, const als_params* p);
/* A context that shares `parent`'s ingest (both CSRs, degree buckets, split-K lists: read-only views)
 * with factors, streams and scratch of its own, for concurrent fits of a CV grid
 * (ALSRecommenderCV.scala:67-90: several ParamMaps of one rank fitted at once from separate host
 * threads).  regParam, alpha, maxIter, implicitPrefs and seed may differ from the parent's; rank,
 * nonnegative and light_max_degree may not.  Single-process contexts only.  The parent's memory stays
 * allocated until its last fork is destroyed; als_set_params is refused on a fork and on a parent with
 * live forks. */
int als_fork(als_ctx* parent, const als_params* p, als_ctx** out);
const char* als_last_error(void);
int als_abi_version(void);
/* number of visible gfx950 devices (0 when no GPU; never initialises a context) */
int als_device_count(int* out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------------------------------------- */
/* 128-byte ncclUniqueId produced on rank 0 and broadcast by the host (e.g. torch.distributed). */
int als_comm_unique_id(void* out128);
/* Must be called before als_set_ratings*; all ranks pass identical ratings. Rows of both sides are
 * sharded by nnz across ranks; each half-sweep all-reduces the partial Gram and all-gathers the
 * rotated factor shard. */
int als_comm_init(als_ctx* ctx, int32_t rank, int32_t world, const void* unique_id128);

/* ---- ingest (DatasetUtils.scala:111-123 input contract: (user Int, item Int, rating Float)) -- */
int als_set_ratings(als_ctx* ctx, int64_t n, const int32_t* user, const int32_t* item, const float* rating);
/* same, inputs already resident in device memory of ctx's device (not modified) */
int als_set_ratings_device(als_ctx* ctx, int64_t n, const int32_t* d_user, const int32_t* d_item,
                           const float* d_rating);
int64_t als_num_rows(const als_ctx* ctx, int side);
int64_t als_num_ratings(const als_ctx* ctx);
int als_rank(const als_ctx* ctx);
int als_get_ids(const als_ctx* ctx, int side, int32_t* ids_out); /* ascending */

/* ---- factors --------------------------------------------------------------------------------- */
/* Parity path: inject initial factors ([n][rank], any id order; every side id must be present). */
int als_set_initial_factors(als_ctx* ctx, int side, int64_t n, const int32_t* ids, const float* factors);
/* Spark-style initialisation (ALS.initialize with XORShiftRandom; best effort). */
int als_init_factors(als_ctx* ctx);
/* Seeded unit-norm Gaussian rows generated on device (large synthetic runs; not Spark's RNG). */
int als_init_factors_random(als_ctx* ctx, uint64_t seed);
int als_get_factors(als_ctx* ctx, int side, int32_t* ids_out, float* factors_out);

/* ---- fit --------------------------------------------------------------------------------------- */
/* Full ALS.train: init (if not injected) + max_iter x (item half-sweep, user half-sweep). Blocking. */
int als_fit(als_ctx* ctx);
/* Run n more full sweeps on the current factors (bench / incremental use). Blocking. */
int als_run_sweeps(als_ctx* ctx, int32_t n);
/* One half-sweep solving `dst_side` from the other side's current factors. Blocking. */
int als_half_sweep(als_ctx* ctx, int dst_side);
/* The ratings of one dst row (by raw id) as (src raw ids, ratings); *n_out = row length, arrays
 * are filled only when n_out <= cap.  Rows of other ranks are not available (ALS_E_STATE). */
int als_get_row_ratings(als_ctx* ctx, int side, int32_t id, int64_t cap, int32_t* src_ids, float* ratings,
                        int64_t* n_out);
/* Ratings per row of `side` in ascending id order (this rank's rows; -1 for rows other ranks own).
 * Observability for the power-law skew (the per-row work of Spark's computeFactors). */
int als_get_degrees(const als_ctx* ctx, int side, int64_t* out);
/* The orthogonal basis B of side's factors (rank x rank, row-major): original factors = X·Bᵀ, X the
 * factors as the engine holds them (als_get_factors returns the original ones).  Implicit fits
 * rotate every half-sweep's solution into the eigenbasis of the src Gram (B_t = B_s·P). */
int als_get_basis(als_ctx* ctx, int side, double* out);
/* Debug/parity: the last Gram matrix YᵀY of `src_side` in the original basis (fp64, [rank][rank];
 * Spark computeYtY of the src factors the last half-sweep solved from). */
int als_get_gram(als_ctx* ctx, int src_side, double* out);

/* ---- model (ALSModel) ------------------------------------------------------------------------ */
/* Build a model-only context from saved factors (ALSModel.load); ids need not be sorted. */
int als_model_create(int32_t rank, int64_t n_users, const int32_t* user_ids, const float* user_factors,
                     int64_t n_items, const int32_t* item_ids, const float* item_factors, int32_t device,
                     als_ctx** out);
/* recommendForAllUsers / recommendForUserSubset (side=ALS_USER) or ...Items (side=ALS_ITEM):
 * for each requested src id (all src rows when subset==NULL, ascending) the top-k dst ids by the
 * F2J-order fp32 dot product (ALSRecommender.scala:51), sorted (score desc, id asc).
 * Outputs [n_src][k]; rows with fewer than k dst entries are padded with id -1 / score NaN.
 * -1 is also a valid raw id (ids are any int32): the NaN score is the padding marker, and a list is
 * dense (its min(k, n_dst) entries come first).
 * Unknown subset ids produce an all-padding row.  src_ids_out may be NULL.
 * k <= 64: MFMA pre-selection + exact rescoring; 64 < k <= 512: exact full scan per src row (slower);
 * k > 512: ALS_E_UNSUPPORTED. */
int als_recommend(als_ctx* ctx, int side, int32_t k, const int32_t* subset, int64_t n_subset,
                  int32_t* src_ids_out, int32_t* dst_ids_out, float* scores_out);
/* als_recommend without each src row's known pairs: for src row u the first k dst rows not in its excluded
 * set E_u, in the total order of als_recommend (F2J score desc, raw id asc).  side, subset, n_subset,
 * src_ids_out and the [n][k] outputs mean what they mean in als_recommend: subset == NULL is every src row in
 * ascending id order, an unknown subset id gives an all-padding row, a repeated id one row each, padding is
 * id -1 / score NaN and a list is dense.
 *   E_u, mode ALS_EXCLUDE_RATINGS  every dst row that occurs in a rating of u in the context's ingest, whatever
 *                 the rating's value (zero and negative ratings are known pairs too); a repeated pair counts
 *                 once.  n_excl, excl_src and excl_dst are ignored.
 *   E_u, mode ALS_EXCLUDE_PAIRS    the dst ids paired with u's raw id in (excl_src, excl_dst) [n_excl], raw ids of
 *                 the src and the dst side.  Any order, repeats allowed, a pair with an id unknown on either side
 *                 is ignored; the result does not depend on the order of the pairs.  n_excl = 0: E is empty
 *                 everywhere.
 *   Result        the score is the F2J sdot of als_recommend / als_recommend_vectors (fp32, left to right, no
 *                 FMA), so a row's list equals, ids and score bits, als_recommend_vectors with u's factor as
 *                 als_get_factors returns it and E_u as the exclusion list, and als_recommend when E_u is empty.
 *                 Fewer than k dst rows left: a shorter, padded list; all excluded: all padding.
 * The contract covers finite factors; non-finite factors are outside it (als_recommend_vectors never lists a
 * NaN score, als_recommend's order kernel has its own rules).
 * Limits: 1 <= k <= 64 and world = 1, ALS_E_UNSUPPORTED beyond either; n_excl >= 2^31 is ALS_E_UNSUPPORTED.
 * ALS_E_STATE when either side has no factors, and for ALS_EXCLUDE_RATINGS on a context without ratings (from
 * als_model_create).  ALS_E_INVALID_ARGUMENT for a bad side or mode, k < 1, a negative count, null pair arrays
 * with n_excl > 0, null outputs.  Forks may call it; they view the parent's ratings.
 * Two calls give identical bits; no floating-point atomics are used.  The model is read-only: factors, bases,
 * Gram caches, sweep timings, path stats and the fold-in / explain / query timings are unchanged, and a call
 * between two half-sweeps leaves the fit bit-identical.  The call runs the top-k passes of als_recommend (as
 * als_evaluate_ndcg does), so als_topk_stats, als_topk_timing and als_topk_last_rescan advance.
 * How: the certified top-`depth` lists (k <= depth <= 64) stay on the device and are filtered there; every dst
 * row outside a list ranks after every row in it, so a list that keeps k entries is the answer.  Only the rows
 * that keep fewer go to an exact scan that knows the row's excluded set.  ALBEDO_UNSEEN_DEPTH in the environment
 * (read per call, clamped to [k, 64]) overrides the default depth of 48; no result depends on it.  ALBEDO_TOPK_PASS and the
 * free-memory cap split the src rows into passes as in als_recommend. */
enum { ALS_EXCLUDE_RATINGS = 0, ALS_EXCLUDE_PAIRS = 1 };
int als_recommend_unseen(als_ctx* ctx, int side, int32_t k,
                         const int32_t* subset, int64_t n_subset,
                         int32_t mode, int64_t n_excl,
                         const int32_t* excl_src, const int32_t* excl_dst /* raw ids, mode ALS_EXCLUDE_PAIRS */,
                         int32_t* src_ids_out, int32_t* dst_ids_out, float* scores_out);
/* Counters of the last als_recommend_unseen call: out[0] = known src rows served, out[1] = rows the filter could
 * not certify, which went to the exact scan, out[2] = list entries the filter removed, out[3] = dst rows the
 * exact scan scored (out[3] < out[1]·n_dst: it pruned). */
int als_recommend_unseen_stats(const als_ctx* ctx, int64_t* out4);
/* Device time of the last als_recommend_unseen call from HIP events on the context's stream (ms): out[0] =
 * exclusion map + sort (0 in ALS_EXCLUDE_RATINGS mode), out[1] = the top-`depth` lists (plan and passes),
 * out[2] = filter, out[3] = exact scan with exclusions, out[4] = total. */
int als_recommend_unseen_timing(const als_ctx* ctx, double* out5);
/* RankingEvaluator (RankingEvaluator.scala:83-139) on the device, the albedo protocol of
 * ALSRecommenderBuilder.scala:92-104: actual lists = intoUserActualItems(user, item, key desc, k) of
 * the given (user, item, key) rows (key = starred_at; rank() <= k, collect_list, slice(0, k) = the
 * first k by (key desc, item asc)), restricted to the model's users (inner join); predicted lists =
 * the users' top-k recommendations (als_recommend, kept on the device); mllib RankingMetrics.ndcgAt(k)
 * per user and the mean over users (*ndcg_out; NaN when no user is left).  users_out (ascending ids)
 * and per_user_out are filled when non-null and *n_users_out <= cap.  1 <= k <= 64. */
int als_evaluate_ndcg(als_ctx* ctx, int32_t k, int64_t n, const int32_t* user, const int32_t* item, const int64_t* key,
                      double* ndcg_out, int64_t* n_users_out, int32_t* users_out, double* per_user_out, int64_t cap);
/* RankingEvaluator's metrics (RankingEvaluator.scala:21, :97-101 -> mllib RankingMetrics.ndcgAt(k),
 * precisionAt(k), meanAveragePrecision). */
enum { ALS_METRIC_NDCG = 0, ALS_METRIC_PRECISION = 1, ALS_METRIC_MAP = 2 };
/* als_evaluate_ndcg with a metric (RankingEvaluator.scala:97-101): the model's own top-k recommendations as
 * the predicted lists, the same actual lists, inner join and rank slicing.  ALS_METRIC_NDCG returns exactly
 * als_evaluate_ndcg's values.  Precision@k = hits in the first min(|pred|, k) / k; MAP = sum over hit
 * positions i of hits_so_far / (i + 1), divided by |labSet| (distinct actual items); fp64, index order. */
int als_evaluate_ranking(als_ctx* ctx, int32_t metric, int32_t k, int64_t n, const int32_t* user, const int32_t* item,
                         const int64_t* key, double* mean_out, int64_t* n_users_out, int32_t* users_out,
                         double* per_user_out, int64_t cap);
/* RankingMetricFormatter("als") (RankingMetricFormatter.scala:59-64, RankingEvaluator.scala:131-139) of
 * ALSModel.transform(pairs) with coldStartStrategy = "drop", the predicted side of the cross-validation
 * job (ALSRecommenderCV.scala:54-90), on the device: every (user, item) pair whose ids the model knows is
 * scored with the F2J sdot; pairs with an unknown id or a NaN score are dropped; per user the pairs with
 * rank() over (score desc) <= top_k stay (ties at the boundary all stay), in (score desc, item asc)
 * order, cut to `width` entries.  +-inf scores order normally, -0.0 and +0.0 tie, a repeated (user, item)
 * pair stays once per copy.  One row per user with at least one surviving pair, ascending user ids:
 * users_out / len_out [cap], items_out / scores_out [cap][width] padded with -1 / NaN; each is filled when
 * non-null and *n_users_out <= cap.  1 <= top_k, width <= 64.  world > 1: ALS_E_UNSUPPORTED (contexts
 * from als_model_create are single-process; a sharded fit is evaluated through its model). */
int als_rank_pairs(als_ctx* ctx, int32_t top_k, int32_t width, int64_t n, const int32_t* user, const int32_t* item,
                   int64_t* n_users_out, int32_t* users_out, int32_t* len_out, int32_t* items_out, float* scores_out,
                   int64_t cap);
/* RankingEvaluator.evaluate (RankingEvaluator.scala:83-103) of those lists with width = k against
 * intoUserActualItems(act_user, act_item, act_key desc, k) (:111-129), as ALSRecommenderCV.scala:72-90 and
 * albedo_toolkit/evaluators.py:42-67 do per fold: the users with at least one surviving predicted pair and
 * at least one actual row (inner join), ascending ids; the mean is their left-to-right sum divided by
 * their count (NaN when nobody is left).  Per-user values are bit-identical to the host evaluator's on the
 * same lists; a predicted item repeated in a list counts as a hit each time, as in mllib.  users_out and
 * per_user_out are filled when non-null and *n_users_out <= cap.  1 <= top_k, k <= 64.  world > 1:
 * ALS_E_UNSUPPORTED. */
int als_evaluate_pairs(als_ctx* ctx, int32_t metric, int32_t top_k, int32_t k, int64_t n_pairs, const int32_t* user,
                       const int32_t* item, int64_t n_act, const int32_t* act_user, const int32_t* act_item,
                       const int64_t* act_key, double* mean_out, int64_t* n_users_out, int32_t* users_out,
                       double* per_user_out, int64_t cap);
/* Device time of the last als_rank_pairs / als_evaluate_pairs call from HIP events on the context's
 * stream (ms): out[0] = id mapping, out[1] = sort + run lengths, out[2] = scoring, out[3] = list
 * selection, out[4] = actual lists + metric (als_evaluate_pairs only). */
int als_eval_pairs_timing(const als_ctx* ctx, double* out5);
/* ALSModel.transform: F2J sdot per (user, item) pair; NaN when either id is unknown. */
int als_predict(als_ctx* ctx, int64_t n, const int32_t* user, const int32_t* item, float* out);

/* ---- fold-in: factors for rows the fit did not see ---------------------------------------------- */
typedef struct als_fold_params {   /* the normal equation's parameters, as als_params */
  double reg_param, alpha;
  int32_t implicit_prefs, nonnegative;   /* nonnegative != 0: solve by NNLS (0, the former reserved field: Cholesky) */
} als_fold_params;
/* The factors of new rows of `side` from their (row_id, src_id, rating) triples, each row solved against
 * the current factors of the other side, which stay frozen ("recalculate user"): side = ALS_USER gives new
 * users from (user, item, rating) triples and the item factors, ALS_ITEM is the mirror.  The factor of row
 * j is what Spark's computeFactors gives that row from these src factors: with G the fp64 Gram of all src
 * rows (implicit prefs; 0 otherwise) and c, w, n as als_audit_rows defines them,
 *   (G + sum_i c_i y_i y_i^T + regParam·n_j·I) x_j = sum_i w_i y_i
 * built and solved by Cholesky in fp64, in the original basis (the src factors are what als_get_factors
 * returns), at the model rank, and rounded to fp32.
 * With fp->nonnegative != 0 the same system, as the full symmetric matrix with regParam·n_j on its diagonal, goes
 * through Spark 2.2.0's NNLSSolver instead (mllib/optimization/NNLS.scala solve, in fp64: x0 = 0, at most
 * max(400, 20·rank) iterations, its stop rules included), and x is rounded once to fp32: the row that
 * ALS.setNonnegative(true) would compute.  NNLS has no "not positive definite" outcome: a singular system is
 * ALS_OK with whatever the loop returns.
 * The model is read-only: the context's factors, bases, Gram state, timings and path stats are unchanged,
 * and a fold-in between two half-sweeps leaves the fit bit-identical.  row_id is any int32; it may
 * coincide with an id the model already has on that side: the call then recomputes that row and stores
 * nothing.  One output row per distinct row_id, in ascending id order; *n_rows_out is their count.
 * ids_out / degree_out [cap] and factors_out [cap][rank] are each filled when non-null and
 * *n_rows_out <= cap; cap = n always suffices.  A triple whose src_id the model does not know is dropped;
 * degree_out is the number of surviving triples of the row, and a row left with none gets an all-zero
 * factor.  A repeated (row, src) pair counts once per copy, as in the ingest.  The triples of a row are
 * summed in ascending src-row order, so the result does not depend on the order of the input arrays
 * (except among copies of one pair with different ratings); no floating-point atomics are used and two
 * calls give identical bits.
 * fp == NULL means the context's own regParam, alpha and implicitPrefs.  A context from als_model_create
 * has none (Spark's saved ALSModel carries only the rank) and requires fp.  When fp is given, fp alone decides
 * the solver, on a context created with nonnegative = true too; fp == NULL does not take the context's
 * nonnegative: in ABI version 1 it stays ALS_E_UNSUPPORTED on such a context (pass fp with nonnegative = 1).
 * Errors: ALS_E_UNSUPPORTED for fp == NULL on a context with nonnegative = true, for
 * world > 1 and for n >= 2^31; ALS_E_STATE when the src side has no factors; ALS_E_INVALID_ARGUMENT for
 * a bad side, a negative n, a NaN or negative reg_param / alpha, null inputs with n > 0, a null
 * n_rows_out, and fp == NULL on a model-only context.  n = 0 is ALS_OK with *n_rows_out = 0.  Forks may
 * call it.  In the Cholesky solve a pivot <= 0 or NaN (regParam·n = 0 on a singular system) fails the call with
 * ALS_E_NOT_POSITIVE_DEFINITE; the message names the lowest failing raw id, and the outputs are then
 * unspecified.  The fp64 src Gram is kept per side until that side's factors change, so further calls
 * (one user at a time on a serving context) skip it; the Cholesky and the NNLS fold-in share it.
 * ALBEDO_FOLD_WGS in the environment caps the persistent grid of the solve (one workgroup per row); the
 * result does not depend on it. */
int als_fold_in(als_ctx* ctx, int side, const als_fold_params* fp,
                int64_t n, const int32_t* row_id, const int32_t* src_id, const float* rating,
                int64_t cap, int64_t* n_rows_out, int32_t* ids_out, int64_t* degree_out,
                float* factors_out /* [cap][rank] */);
/* Device time of the last als_fold_in call from HIP events on the context's stream (ms): out[0] = id
 * mapping + sort + CSR, out[1] = src Gram (0 when taken from the cache), out[2] = solve (whichever solver
 * ran), out[3] = total. */
int als_fold_in_timing(const als_ctx* ctx, double* out4);
/* NNLS iterations of the last als_fold_in call: out[0] = summed over rows, out[1] = the maximum over rows,
 * out[2] = rows solved by NNLS (those with a surviving triple), out[3] = rows that ran into the iteration
 * limit max(400, 20·rank).  All four are 0 after a Cholesky call. */
int als_fold_in_stats(const als_ctx* ctx, int64_t* out4);

/* Which ratings drive a recommendation: for a row of `side` given by its triples, as als_fold_in takes them,
 * and a target of the other side, how much of the row's score for the target each rating contributes.  With
 *   A_j = G + sum_i c_i y_i y_i^T + regParam·n_j·I
 * the system als_fold_in builds for row j (c, w, n and G as als_audit_rows defines them), the score of target t
 * is linear in the row's ratings,
 *   s_jt = y_t^T x_j = y_t^T A_j^-1 sum_i w_i y_i = sum_i e_jti,   e_jti = w_i · y_t^T A_j^-1 y_i,
 * and e_jti is rating i's share of it ("because you starred X").  Everything is fp64, in the original basis, at
 * the model rank: A_j is built and factored exactly as the fold-in does, z = A_j^-1 y_t comes from two
 * triangular solves, and e_i = w_i · sum_m y_i[m]·z[m], summed in ascending m.
 *   Rows      (row_id, src_id, rating) [n], side and fp mean what they mean in als_fold_in: new or known ids, a
 *             triple with an unknown src_id is dropped, a copy of a pair counts once per copy, the triples of a
 *             row are summed in ascending src-row order.
 *   Pairs     pair p asks about row pair_row_id[p] and the target pair_target_id[p], a raw id of the *src* side:
 *             with side = ALS_USER an item ("why this item for this user").  A target among the row's own
 *             sources is ordinary.  Only the rows that a valid pair names are built and factored.
 *   Output    total_out[p] = sum_i e_i over the row's surviving triples in CSR order, one fixed order of
 *             addition.  src_ids_out / contrib_out [n_pairs][m]: the m surviving triples with the largest e_i,
 *             by (value desc, src id asc); -0.0 and +0.0 tie; a copy of a pair is an entry of its own; a shorter
 *             list is padded with id -1 and value NaN (the NaN tells the padding: -1 is a valid raw id).
 *             A pair whose row id occurs in no triple, or whose target the model does not know: total NaN, all
 *             padding.  A row left with no surviving triple: total +0.0, all padding.
 * Two calls give identical bits; no floating-point atomics are used.  A pair's output does not depend on the
 * other pairs of the call, on their order, on ALBEDO_FOLD_WGS (which caps this grid as it caps the fold-in's),
 * or on the order of the triples (except among copies of one pair with different ratings).  e_i depends only on
 * rating i's own (w_i, y_i) and the pair's z: two ratings with equal factor rows and equal ratings give equal
 * bits, and the id decides their order.
 * The total is the fold-in's score before any rounding: als_fold_in rounds x_j to fp32 once, so
 * |total - sum_m x_j[m]·y_t[m]| <= 2^-24 · sum_m |x_j[m]·y_t[m]| beyond the fp64 arithmetic.
 * The model is read-only, as for als_fold_in: the call may form or use the side's fp64 src Gram cache (the
 * fold-in's, with its validity rule); no factor, basis, sweep Gram, timing, path stat or top-k counter changes,
 * als_fold_in_timing / als_fold_in_stats keep their values, and a call between two half-sweeps leaves the fit
 * bit-identical.  Forks and contexts from als_model_create may call it; the latter need fp.
 * Errors: ALS_E_INVALID_ARGUMENT for a bad side, a negative n or n_pairs, m < 1, null arrays with a positive
 * count, null outputs with n_pairs > 0, a NaN or negative reg_param / alpha, fp == NULL on a model-only
 * context.  ALS_E_UNSUPPORTED for m > 64, world > 1, n or n_pairs >= 2^31, and for fp->nonnegative != 0 or
 * fp == NULL on a context with nonnegative = true: an NNLS row is not linear in its ratings, so this
 * decomposition is not its score.  ALS_E_STATE when the src side has no factors.  ALS_E_NOT_POSITIVE_DEFINITE
 * for a pivot <= 0 or NaN in a row that a valid pair names (a singular row that no pair names does not fail the
 * call); the message names the lowest failing raw id, and the outputs are then unspecified.  n_pairs = 0 is
 * ALS_OK. */
int als_explain(als_ctx* ctx, int side, const als_fold_params* fp,
                int64_t n, const int32_t* row_id, const int32_t* src_id, const float* rating,
                int64_t n_pairs, const int32_t* pair_row_id, const int32_t* pair_target_id,
                int32_t m,
                double* total_out   /* [n_pairs] */,
                int32_t* src_ids_out /* [n_pairs][m] */,
                double* contrib_out  /* [n_pairs][m] */);
/* Device time of the last als_explain call from HIP events on the context's stream (ms): out[0] = id mapping,
 * sort and CSR of the triples and the pairs, out[1] = src Gram (0 when taken from the cache), out[2] = build,
 * factor, solves, contributions and selection, out[3] = total. */
int als_explain_timing(const als_ctx* ctx, double* out4);

/* Exact top-k of caller-supplied query vectors against the factors of `dst_side` (ALS_ITEM: score against
 * the items, ALS_USER: against the users), with an optional exclusion list per query: recommendations for a
 * folded-in row without what it already has, for an average of rows, or for an item's own factor against
 * the item side.  q is [n_q][rank], row-major.
 *   Listed rows   for query i, the rows of dst_side whose raw id is not in
 *                 excl_ids[excl_ptr[i] .. excl_ptr[i+1]).  excl_ptr == NULL: no exclusions.  The ids may come
 *                 in any order, may repeat, and may name ids the model does not know (ignored); the result
 *                 does not depend on their order.
 *   Scoring       the F2J sdot of q[i] and the row's factor as als_get_factors returns it: fp32, strictly
 *                 left to right over the rank, multiply and add rounded separately (no FMA), the sum
 *                 starting from +0.0.
 *   Selection     the best k in (score desc, id asc) order, the total order of als_recommend; -0.0 and +0.0
 *                 tie.  A row whose score is NaN is never listed; +inf and -inf order normally.
 *   Output        dst_ids_out / scores_out [n_q][k], dense; a list shorter than k is padded with id -1 and
 *                 score NaN (the NaN tells the padding: -1 is a valid raw id).
 * Two calls give identical bits; no floating-point atomics are used.
 * Limits: 1 <= k <= 64, world = 1, n_q < 2^31: ALS_E_UNSUPPORTED beyond them (als_recommend serves larger k
 * for rows the model holds).  Cosine similarity: als_similar / als_similar_vectors below.
 * Errors: ALS_E_INVALID_ARGUMENT for a bad side, k < 1, a negative n_q, null q or outputs with n_q > 0, an
 * excl_ptr that is negative or does not ascend, a null excl_ids with a non-empty range, more than 2^31 - 1
 * exclusions; ALS_E_STATE when dst_side has no factors.  n_q = 0 is ALS_OK.
 * The model is read-only: factors, bases, Gram caches, als_topk_stats, als_topk_timing,
 * als_topk_last_rescan, sweep timings and path stats are unchanged, and a call between two half-sweeps
 * leaves the fit bit-identical.  Contexts from als_model_create and forks may call it.
 * ALBEDO_QUERY_SLICE_ROWS in the environment overrides the number of dst rows per scan slice (default: from
 * the CU count). */
int als_recommend_vectors(als_ctx* ctx, int dst_side, int32_t k,
                          int64_t n_q, const float* q /* [n_q][rank] */,
                          const int64_t* excl_ptr /* [n_q+1] or NULL */, const int32_t* excl_ids /* raw dst ids */,
                          int32_t* dst_ids_out /* [n_q][k] */, float* scores_out /* [n_q][k] */);
/* Device time of the last als_recommend_vectors call from HIP events on the context's stream (ms):
 * out[0] = exclusion map + sort (0 without exclusions), out[1] = scan, out[2] = merge, out[3] = total. */
int als_recommend_vectors_timing(const als_ctx* ctx, double* out4);

/* Cosine top-k within one side: for each requested row of `side` (every row, ascending id, when subset ==
 * NULL) the best k OTHER rows of the same side ("repos like this one", "users like this user").
 *   Unit image    every row y of the side as als_get_factors returns it (fp32, `rank` columns) gives
 *                 s = F2J sdot(y, y) (fp32, left to right from +0.0, multiply and add rounded separately),
 *                 r = sqrt(s) and u_c = y_c / r, square root and divide correctly rounded in fp32: numpy's
 *                 float32 sqrt and /.  A row has no direction when !(s > 0 && s < inf): all zero, NaN or
 *                 +-inf inside, s overflowed or underflowed to 0.  Its unit row is NaN.
 *   Score         cos(i, j) = F2J sdot(u_i, u_j): als_recommend_vectors' scoring on the unit image.  Scaling a
 *                 row by a power of two (no overflow, no underflow) leaves its unit row, and so every score,
 *                 bit-identical; a row against a copy of itself scores sdot(u, u), which need not be 1.0f.
 *                 To first order the score is within (rank + 4) * 2^-24 of the fp64 cosine.
 *   Listed rows   the row itself is never listed; rows without a direction are never listed and their own
 *                 list is all padding; an id of `subset` the side does not know gives an all-padding row, a
 *                 repeated id one row each, in the caller's order.
 *   Selection     (score desc, id asc), -0.0 and +0.0 tie, a NaN score is never listed; lists are dense,
 *                 padded with id -1 / score NaN: als_recommend's order and padding.
 *   Output        src_ids_out [n] (may be NULL) echoes the requested ids; ids_out / scores_out [n][k] with
 *                 n = n_subset, or the side's row count when subset == NULL.
 * Two tiers give the same bits: the query scan of als_recommend_vectors for few rows, and for many rows the
 * passes of als_recommend_unseen on a transient model whose two sides are both the unit image (rows without
 * a direction left out), built on the device and destroyed with the call.  The tier follows the row count;
 * ALBEDO_SIMILAR_TIER=scan|passes in the environment (read per call) forces one.  The default goes to the passes
 * from 2^18 rows asked; what that rests on, and where it is not backed by a measurement, is in DESIGN.md
 * ("Similar rows within one side").  ALBEDO_SIMILAR_TRACE=1 (diagnostic) makes the passes tier print one line
 * on stderr with the transient model's build time, timers and counters.  The unit image is rebuilt by every
 * call; nothing is cached on the context.
 * Limits: 1 <= k <= 64, world = 1, n_subset < 2^31: ALS_E_UNSUPPORTED beyond them.
 * Errors: ALS_E_INVALID_ARGUMENT for a bad side, k < 1, a negative n_subset, null ids_out or scores_out;
 * ALS_E_STATE when `side` has no factors.  n_subset = 0 is ALS_OK.  Only the one side is needed: a model
 * created with zero users serves als_similar(ALS_ITEM).
 * The model is read-only: factors, bases, Gram caches, sweep timings, path stats and the counters and timings
 * of als_recommend, als_recommend_unseen, als_recommend_vectors, als_fold_in and als_explain are unchanged,
 * and a call between two half-sweeps leaves the fit bit-identical.  Two calls give identical bits; no
 * floating-point atomics are used.  Fitted contexts, forks and contexts from als_model_create may call it. */
int als_similar(als_ctx* ctx, int side, int32_t k,
                const int32_t* subset /* raw ids or NULL */, int64_t n_subset,
                int32_t* src_ids_out /* [n] or NULL */, int32_t* ids_out /* [n][k] */, float* scores_out /* [n][k] */);
/* The same for caller-supplied vectors (a folded-in user, an average of repos): q[i] ([n_q][rank]) goes
 * through the unit rule above (a q[i] without a direction: all padding), then exactly als_recommend_vectors'
 * contract on the unit image of dst_side, exclusion lists included (a query that is a row of dst_side lists
 * that row unless its id is excluded).  Always the scan tier.
 * Limits: 1 <= k <= 64, world = 1, n_q < 2^31, fewer than 2^31 exclusions: ALS_E_UNSUPPORTED beyond them.
 * Errors: ALS_E_INVALID_ARGUMENT for a bad side, k < 1, a negative n_q, null q or outputs with n_q > 0, an
 * excl_ptr that is negative or does not ascend, a null excl_ids with a non-empty range; ALS_E_STATE when
 * dst_side has no factors.  n_q = 0 is ALS_OK.  Read-only like als_similar. */
int als_similar_vectors(als_ctx* ctx, int dst_side, int32_t k,
                        int64_t n_q, const float* q /* [n_q][rank] */,
                        const int64_t* excl_ptr /* [n_q+1] or NULL */, const int32_t* excl_ids /* raw dst ids */,
                        int32_t* ids_out /* [n_q][k] */, float* scores_out /* [n_q][k] */);
/* Device time of the last als_similar / als_similar_vectors call (ms, HIP events): out[0] = unit image (with
 * the queries and their exclusion keys in the scan tier, the compaction in the passes tier), out[1] = the lists
 * (the scan, or the passes' plan, lists and exact scan), out[2] = merge (scan tier) or filter (passes tier),
 * out[3] = total. */
int als_similar_timing(const als_ctx* ctx, double* out4);
/* Counters of the last call: out[0] = rows asked that the side knows (als_similar_vectors: n_q), out[1] = rows
 * of the side without a direction, out[2] = tier used (0 scan, 1 passes), out[3] = rows the passes tier sent
 * to its exact scan. */
int als_similar_stats(const als_ctx* ctx, int64_t* out4);

/* ---- observability ---------------------------------------------------------------------------- */
/* Per-stage device time (ms) of the last half-sweeps: see ALS_T_* indices. n = array length. */
enum {
  ALS_T_GRAM = 0, ALS_T_EIG = 1, ALS_T_ROTATE = 2, ALS_T_COMM = 3, ALS_T_SOLVE_LIGHT = 4,
  ALS_T_SOLVE_HEAVY = 5, ALS_T_HALF_TOTAL = 6, ALS_T_COUNT = 8
};
int als_last_timings(const als_ctx* ctx, int dst_side, double* out, int n);
/* Rows / nnz handled by each solve path in the last half-sweep of dst_side:
 * out[0]=light rows, out[1]=light nnz, out[2]=heavy rows, out[3]=heavy nnz.  "Light" means within
 * the light limit (light_max_degree; 64 by default at rank 65..256) and solved by the push-through
 * path; every row above the limit counts under out[2..3], the degree tier 65..80 included although a
 * push-through instance solves it (its launch is timed with ALS_T_SOLVE_HEAVY).  With nonnegative =
 * true "light" is the lockstep NNLS kernel (16 low-degree rows per workgroup) and "heavy" every
 * other row (one workgroup per row). */
int als_path_stats(const als_ctx* ctx, int dst_side, int64_t* out4);
/* Solver counters of the last half-sweep of dst_side.
 * nonnegative = true (NNLS): out[0] = iterations summed over rows, out[1] = max over rows,
 *   out[2] = rows, out[3] = the part of out[0] spent by the lockstep kernel's rows (als_path_stats out[0]).
 * nonnegative = false (Cholesky path): out[0] = Jacobi sweeps the device eigensolver took on the src
 *   Gram (0 without implicitPrefs), out[1..3] = 0.  A half-sweep whose eigensolver spends its sweep
 *   budget without converging fails with ALS_E_NOT_POSITIVE_DEFINITE. */
int als_solver_stats(const als_ctx* ctx, int dst_side, int64_t* out4);
/* The solve path the context's row layout routes a row to (als_audit.worst_path).  It is the layout's
 * routing (degree, light limit, degree tiers, split-K chunk; nonnegative: lockstep or per-row NNLS kernel,
 * split-K rows counting with the per-row kernel): a half-sweep that sent every row to the explicit path
 * (regParam = 0) is not reflected. */
enum { ALS_PATH_LIGHT16_PAIR = 0, ALS_PATH_LIGHT16, ALS_PATH_LIGHT32, ALS_PATH_LIGHT48, ALS_PATH_LIGHT64,
       ALS_PATH_LIGHT96, ALS_PATH_TIER80, ALS_PATH_EXPLICIT, ALS_PATH_SPLIT, ALS_PATH_NNLS_LOCKSTEP,
       ALS_PATH_NNLS_ROW };
typedef struct als_audit {
  int64_t rows;         /* own dst rows audited */
  int64_t rows_over;    /* rows with !(eta <= tol): a non-finite eta counts */
  int64_t non_finite;   /* rows whose eta is NaN/Inf */
  int64_t negative;     /* nonnegative = true: rows with a component < 0 (else 0) */
  int64_t worst_degree;
  int32_t worst_id;     /* raw id of the row with the largest eta (non-finite ranks above all; ties: lowest id) */
  int32_t worst_path;   /* ALS_PATH_*: the path this context's layout routes that row to */
  double  worst_eta, sum_eta;
} als_audit;
/* Every own row of dst_side checked against its normal equation, in fp64 on the device, from the current
 * factors of both sides in the original basis (what als_get_factors returns).  With G the fp64 Gram of
 * all src rows (implicitPrefs; 0 otherwise), and per rating c = alpha·|r|, w = (r > 0 ? 1 + c : 0),
 * n = the count of r > 0 (implicitPrefs) or c = 1, w = r, n = the degree:
 *   r_j = G·x_j + sum_i c_i (y_i·x_j) y_i + regParam·n_j·x_j - sum_i w_i y_i
 *   eta_j = |r_j|_2 / ((|G|_F + sum_i c_i |y_i|^2 + regParam·n_j)·|x_j|_2 + |sum_i w_i y_i|_2), 0 when
 * the denominator is 0.  nonnegative = true: r is the KKT residual (component m is r_m where x_m > 0,
 * else min(r_m, 0)).  One pass over the ratings, O(nnz·rank); nothing a half-sweep computed is used, so
 * the call is stateless: right after als_half_sweep(t) the audit of t is the solve's backward error, on
 * the other side it measures the distance from that side's fixed point, and it works on injected factors
 * with no sweep at all.  eta_out (or NULL): [als_num_rows] in ascending id order like als_get_degrees,
 * NaN for rows other ranks own; *out summarises the own rows (worst_id = -1, worst_path = -1 when there
 * are none).  world > 1: collective (one Gram all-reduce, one factor gather), every rank calls it and
 * receives the summary of its own rows.  Forks may call it.  ALS_E_STATE without ratings (model-only
 * contexts) or when a side has no factors; ALS_E_INVALID_ARGUMENT for a bad side, a NaN tol, a null out.
 * tol: the engine's solves measure at most 1.2e-7 on the degree ladder of the test suite (the
 * row audit), so 16 times that, 2e-6, is the recommended working tolerance; 1e-4·sqrt(rank) is the
 * guaranteed bound.  Rows longer than ALBEDO_AUDIT_CHUNK ratings (environment; default: a quarter of
 * one wave's share of the ratings, at least 512) are summed in chunks, in chunk order. */
int als_audit_rows(als_ctx* ctx, int dst_side, double tol, double* eta_out /* [als_num_rows] or NULL */,
                   als_audit* out);
/* The loss that ALS minimises, in fp64 on the device, from the current factors of both sides in the original
 * basis (what als_get_factors returns) and the fp32 ratings.  Per rating r of row j of `side` on row i of the
 * other side, s = x_j·y_i; with c, w, n_j and G as als_audit_rows defines them for implicitPrefs (c = alpha·|r|,
 * w = (r > 0 ? 1 + c : 0), n_j = the count of r > 0, G = the fp64 Gram of all rows of the other side), and
 * n_j = the degree, G = 0 otherwise:
 *   implicit:  t_r = c·s^2 - 2·w·s + w          explicit:  t_r = (r - s)^2
 *   loss_j = x_j^T G x_j + sum_{r in row j} t_r + regParam·n_j·|x_j|^2
 *   total  = sum_j loss_j + regParam·sum_i n_i·|y_i|^2,          n_i from the other side's own rows.
 * With implicitPrefs sum_j (x_j^T G x_j + sum t_r) is the sum over ALL pairs (j, i) of conf·(p - x_j·y_i)^2,
 * conf = 1 + c on rated pairs and 1 elsewhere, p = [r > 0]: the cost of Hu, Koren and Volinsky with Spark's
 * weighted regulariser, the function whose gradient per row is the normal equation of als_fold_in and
 * als_audit_rows.  Every half-sweep minimises it over one side, so it falls after each.  A copy of a pair
 * counts once per copy, a zero rating adds nothing to t but is a rated pair, a negative rating adds c·s^2.
 * `side` chooses the CSR that is walked and the rows of row_loss_out ([als_num_rows(side)], ascending ids, or
 * NULL); the total is the same from either side up to rounding.  sse / n_ratings is the squared training RMSE.
 * abs_terms is the sum of the absolute values of everything added and so the scale of the rounding error.
 * Two calls give identical bits; no floating-point atomics are used, rows and chunks are added in a fixed
 * order.  Rows longer than ALBEDO_OBJECTIVE_CHUNK ratings (environment, read per call; default as
 * ALBEDO_AUDIT_CHUNK) are summed in chunks, in chunk order; the value changes the result by rounding only.
 * The model is read-only: factors, bases, Gram caches, sweep timings, path stats, top-k counters and the
 * fold-in / explain timings are unchanged, and a call between two half-sweeps leaves the fit bit-identical.
 * Non-finite factors give non-finite outputs and are not an error.  Forks may call it.  ALS_E_STATE without
 * ratings (contexts from als_model_create) or when a side has no factors; ALS_E_INVALID_ARGUMENT for a bad
 * side or a null out; ALS_E_UNSUPPORTED for world > 1. */
typedef struct als_objective_t {
  double total;       /* all_pairs + ratings + reg_side + reg_other */
  double all_pairs;   /* sum_j x_j^T G x_j   (0 for explicit) */
  double ratings;     /* sum_r t_r */
  double reg_side;    /* regParam·sum_j n_j |x_j|^2 over `side` */
  double reg_other;   /* the same over the other side */
  double sse;         /* sum_r (r - s_r)^2: training RMSE = sqrt(sse / n_ratings); equals `ratings` when explicit */
  double abs_terms;   /* sum of the absolute values of everything added: |x_j^T G x_j| + sum_r (|c s^2| + |2 w s|
                         + |w|) (explicit: t_r) + both reg terms */
  int64_t n_ratings, rows;
} als_objective_t;
int als_objective(als_ctx* ctx, int side, double* row_loss_out /* [als_num_rows(side)] or NULL */,
                  als_objective_t* out);
/* Device time of the last als_objective call from HIP events on the context's stream (ms): out[0] = the fp64
 * Gram (0 for explicit), out[1] = the row pass and the sums, out[2] = total. */
int als_objective_timing(const als_ctx* ctx, double* out3);
/* als_fit with the objective (als_objective through the user-side CSR, `total`) evaluated after the
 * initialisation, history[0], and after every full sweep s, history[s].  tol > 0: the fit stops after the first
 * sweep s >= 1 with history[s-1] - history[s] < tol·|history[s-1]| (an increase stops it; a NaN never satisfies
 * the test, so the fit runs on).  tol <= 0 or NaN: all max_iter sweeps run.  *sweeps_run_out = the sweeps run,
 * *n_history_out = that + 1; history_out is filled when non-null and *n_history_out <= cap (cap = max_iter + 1
 * always suffices).  The factors after s sweeps are bit-identical to als_fit with max_iter = s.  Errors as
 * als_fit, and ALS_E_UNSUPPORTED for world > 1. */
int als_fit_tracked(als_ctx* ctx, double tol, int32_t cap, double* history_out /* [cap] */,
                    int32_t* n_history_out, int32_t* sweeps_run_out);
/* Top-k counters since als_create (als_recommend with k <= 64): out[0] = src rows through the MFMA
 * scan, out[1] = rows whose candidate set failed certification and were re-scored by the exact scan,
 * out[2] = dst rows the scan waves scored (a wave skips a chunk none of its rows can use), out[3] = the same without the chunk
 * early exit. */
int als_topk_stats(const als_ctx* ctx, int64_t* out4);
/* Top-k device time since als_create, from HIP events on the context's stream (ms): out[0] = scan
 * order + chunk masks, out[1] = the MFMA scan, out[2] = select + certification, out[3] = exact
 * rescans; out[4] = the flops the scan's MFMAs performed (2·KP per scored src x dst pair), so
 * out[4] / out[1] is the scan's achieved matrix rate. */
int als_topk_timing(const als_ctx* ctx, double* out5);
/* The src ids whose candidate set failed certification in the last als_recommend call (k <= 64) and
 * were re-scored by the exact scan, in output order; *n_out = their count, ids filled when
 * n_out <= cap.  Parity tests check exactly these rows against the oracle. */
int als_topk_last_rescan(const als_ctx* ctx, int32_t* src_ids_out, int64_t cap, int64_t* n_out);
/* Synchronise the context's streams (bench barrier helper). */
int als_synchronize(als_ctx* ctx);

/* ---- synthetic workloads (BASELINE configs; same algorithm as albedo_amd/synthetic.py) -------- */
/* Run the device twin of synthetic.generate() and copy the COO to host buffers (n_out entries;
 * buffers sized deg_prefix[n_users]).  deg_prefix: per-user degree prefix (n_users+1, host),
 * cw: cumulative popularity weights (n_items, host), perm: popularity rank -> item position. */
int als_synth_generate(int32_t device, uint64_t seed, int32_t rounds, int64_t n_users, int64_t n_items,
                       const int64_t* deg_prefix, const double* cw, const int32_t* perm, int32_t* user_out,
                       int32_t* item_out, float* rating_out, int64_t* n_out);
/* Same, generated straight into the context's device ingest (inputs resident in HBM). */
int als_set_ratings_synthetic(als_ctx* ctx, uint64_t seed, int32_t rounds, int64_t n_users, int64_t n_items,
                              const int64_t* deg_prefix, const double* cw, const int32_t* perm);

/* ---- multi-process exchange through the host (tests: ranks sharing one GPU) -------------------- */
/* allreduce: in-place sum of n doubles over ranks; allgather: buf holds world*n_per_rank floats with
 * this rank's block filled; on return every block is filled.  Return 0 on success. */
int als_comm_init_host(als_ctx* ctx, int32_t rank, int32_t world, int (*allreduce)(void*, double*, int64_t),
                       int (*allgather)(void*, float*, int64_t), void* user);

/* ---- host-only utilities (no GPU; exercised by the CPU test suite) ----------------------------- */
int als_host_eigh(int32_t n, const double* a, double* w, double* v);  /* a = v diag(w) vᵀ, w ascending */
/* The engine's device eigensolver (warm-started cyclic Jacobi, eig.hip) on one k x k symmetric g:
 * a = v diag(w) vᵀ, w unordered; w0 (or NULL = identity) the orthogonal warm start; sweeps: Jacobi
 * sweeps taken.  Test hook, like als_host_eigh. */
int als_device_eigh(int32_t device, int32_t k, const double* g, const double* w0, double* w, double* v,
                    int32_t* sweeps);
int als_host_spark_side_seeds(int64_t seed, int64_t* user_seed, int64_t* item_seed);
int als_host_spark_init(const int32_t* ids_sorted, int64_t n, int32_t rank, int64_t side_seed,
                        int32_t num_blocks, float* out);
int als_host_plan_shards(const int64_t* ptr, int64_t n, int32_t world, int64_t* starts_out);

#ifdef __cplusplus
}
#endif
#endif /* ALBEDO_ALS_H */
