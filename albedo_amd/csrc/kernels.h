// Internal launch interface between the host code (als_engine.cpp, sweep_host.cpp, topk_host.cpp,
// eval_host.cpp, audit_host.cpp and objective_host.cpp with row_plan.h, foldin_host.cpp, explain_host.cpp,
// query_topk_host.cpp, similar_host.cpp) and the HIP kernels.  Not part of the public C ABI (include/albedo_als.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace albedo {

// Padded rank used on device: factor rows are KP floats (zero beyond `rank`).
int padded_rank(int rank);  // 64, 128 or 256 (0 if unsupported)

// *SolveArgs::err bits: 1 = a non-positive diagonal (λn + Λ), 2 = a collapsed pivot / non-finite
// solution; with 2 the path that met it (reported in the not-positive-definite message)
constexpr int ALBEDO_EF_LIGHT16 = 16, ALBEDO_EF_LIGHT_REG = 32, ALBEDO_EF_LIGHT_ACC = 64, ALBEDO_EF_WAVE = 128,
              ALBEDO_EF_HEAVY = 256;

struct SolveArgs {
  const float* Z;          // src factors in the eigenbasis of the src Gram, [*][KP]
  const int64_t* ptr;      // dst CSR row pointer (global dst row index)
  const int32_t* col;      // src row index (into Z)
  const float* val;        // rating
  const int32_t* rows;     // dst rows handled by this launch
  int64_t n_rows;
  const float* lam;        // [KP] eigenvalues of the src Gram (implicit) or zeros (explicit)
  float* X;                // out: dst factors in that eigenbasis, [*][KP]
  int kreal;               // the model rank (<= KP)
  int implicit;
  float alpha;
  float reg;
  int* err;                // device flag: set to 1 when a solve meets a non-positive pivot
  const float* colscale;   // [2*KP] heavy-build fp16 column scales 2^e and their inverses
  const float* prebuilt;   // split rows: reduced A' records [n_rows][split_rec_floats] (else null)
  unsigned long long* iters;  // NNLS: [0] += iterations of every row, [1] = max over rows (or null)
  // uniform confidence (every rating of the side has the same c: binary implicit data, or explicit):
  // the heavy build gathers pre-split rows instead of Z (launch_presplit), null otherwise
  const void* Zhl;         // [*][2·KP] fp16: hi of √c·colscale·z, then lo
  int64_t zero_row;        // an all-zero row of Zhl and of Z (the gather target of ratings past a row's end or masked)
  float wsc;               // power-of-two scale of the rating weights w in the b' MFMA (max|w|·wsc < 2^13)
  float inv_sw;            // 1 / √c
  const int32_t* desc;     // light launches: int4 {row, p0 lo, p0 hi, degree} per entry of `rows` (or null)
  int n_cu;                // compute units (persistent launches)
};

// Split-K of the heavy tail (rows with more ratings than one chunk): every chunk of chunk_len
// ratings is built by its own workgroup into an fp32 partial record (packed A' tiles + b' + the
// positive-rating count), the partials of a row are summed in fp64 in chunk order (deterministic),
// and the row is factored from the reduced record (SolveArgs::prebuilt).
struct SplitArgs {
  const int32_t* chunk_row;  // [n_chunks] dst row (CSR row index) of each chunk
  const int32_t* chunk_idx;  // [n_chunks] chunk number within its row
  int64_t n_chunks;
  int chunk_len;
  const int32_t* slot0;      // [n_split + 1] first chunk of each split row (rows in factor order)
  int64_t n_split;
  float* partial;            // [n_chunks][split_rec_floats]
  float* reduced;            // [n_split][split_rec_floats]
};
int split_rec_floats(int KP);
// partial builds of every chunk (KP <= 128: one wave per chunk, heavy_wave.hip; KP = 256: one
// 16-wave workgroup per chunk), then the fp64 reduction into s.reduced
hipError_t launch_heavy_split(int KP, const SolveArgs& a, const SplitArgs& s, hipStream_t st);
hipError_t launch_wave_partial(int KP, const SolveArgs& a, const SplitArgs& s, hipStream_t st);

// G (fp64 [KP][KP], full symmetric) = Σ_rows Xᵀ X over rows [0, n) of X ([n][KP]).
hipError_t launch_gram(int KP, const float* X, int64_t n, double* slab, int slab_blocks, double* G,
                       hipStream_t s);
int gram_slab_blocks(int KP, int64_t n);
size_t gram_slab_doubles(int KP, int slab_blocks);

// Z = X · M for n rows ([n][KP] · [KP][KP], row-major M); cmax (optional, zeroed by the caller):
// atomicMax of the bits of max |Z[.][c]| per column (launch_colscale(..., have_max = true) reads it)
hipError_t launch_rotate(int KP, const float* X, const float* M, float* Z, int64_t n, hipStream_t s,
                         unsigned* cmax = nullptr);

// Per-row solves. light: rows with degree <= D (D in {16,32,64}); heavy: any degree.
hipError_t launch_solve_light(int KP, int D, const SolveArgs& a, hipStream_t s);
// light rows of degree <= 16 (light16.hip): the push-through solve written for VALU instruction count
hipError_t launch_solve_light16(int KP, const SolveArgs& a, hipStream_t s, bool pair = false);
// desc[4i .. 4i+3] = {rows[i], ptr[rows[i]] lo, hi, degree}: one scalar load per row for light16
hipError_t launch_row_desc(const int32_t* rows, int64_t n, const int64_t* ptr, int32_t* desc, hipStream_t s);
hipError_t launch_solve_heavy(int KP, const SolveArgs& a, hipStream_t s);
// heavy rows, one wave per row (heavy_wave.hip), KP <= 128; rows of any degree (split rows excepted)
hipError_t launch_solve_wave(int KP, const SolveArgs& a, hipStream_t s);
// Rows on the explicit k x k path, whichever kernel that is: split rows (a.prebuilt) and KP = 256 take
// launch_solve_heavy, every other row at KP <= 128 launch_solve_wave
hipError_t launch_solve_explicit(int KP, const SolveArgs& a, hipStream_t s);
// whether launch_solve_explicit's kernels gather the pre-split src rows (SolveArgs::Zhl) when given
bool explicit_reads_presplit(int KP);

// nonnegative = true: Spark NNLS per row; Gt = the src Gram in the NNLS tile layout (fp32).
hipError_t launch_solve_nnls(int KP, const SolveArgs& a, const float* Gt, hipStream_t s);
// KP = 256 per-row NNLS on 512-thread workgroups, two per CU (nnls_row.hip); launch_solve_nnls
// routes KP = 256 here unless ALBEDO_NNLS_ROW=1024 (the register kernel of als_kernels.hip)
hipError_t launch_solve_nnls_row256(const SolveArgs& a, const float* Gt, hipStream_t s);
int nnls_gtile_floats(int KP);
// NNLS rows of low degree, `slots` (16/8/4/2/1) per workgroup in lockstep (nnls_batch.hip); a slot
// holds rows of degree <= nnls_batch_max_degree(KP, slots).  A persistent grid of at most n_cu
// workgroups takes rows from *counter (zeroed by the launch).  Gfrag: KP*KP*4 bytes holding G·gscale
// in MFMA operand order as fp16 hi + lo, filled by launch_nnls_gfrag (gscale a power of two with
// max|G|·gscale < 2^15).
int nnls_batch_max_degree(int KP, int slots);
hipError_t launch_nnls_gfrag(int KP, const float* Gt, float gscale, void* Gfrag, hipStream_t s);
hipError_t launch_nnls_batch(int KP, int slots, const SolveArgs& a, const void* Gfrag, float gscale,
                             unsigned int* counter, int n_cu, hipStream_t s);
// colscale[c] = 2^e_c with max_rows |Z[.][c]|·√cmax < 2^13, colscale[KP+c] = 2^-e_c (tmp: KP uints)
hipError_t launch_colscale(int KP, const float* Z, int64_t n, float cmax, unsigned* tmp, float* colscale,
                           hipStream_t s, bool have_max = false);
// Zhl[r] = fp16 hi and lo of Z[r][c]·(sw·colscale[c]) (the heavy build's operand split, done once per
// src row instead of once per gathered rating); row n (the zero row) is cleared
hipError_t launch_presplit(int KP, const float* Z, int64_t n, const float* colscale, float sw, void* Zhl, hipStream_t s);
// Z = X·P on bf16 MFMA (three-part split of both operands, KP = 128 only); Pf: rotate_bf_pfrag_bytes
// of scratch for P's parts; Zhl (or null): the heavy build's operand split written in the same pass
// (colscale cs and √c sw as launch_presplit, which it replaces), row zrow of Zhl zeroed
hipError_t launch_rotate_bf(int KP, const float* X, const float* P, void* Pf, float* Z, int64_t n, const float* cs, float sw,
                            void* Zhl, int64_t zrow, int n_cu, hipStream_t s);
int rotate_bf_pfrag_bytes(int KP);
// *out = bits of max |v[i]| (non-negative float, compared as unsigned)
hipError_t launch_absmax(const float* v, int64_t n, unsigned* out, hipStream_t s);
// *out = bits of min |v[i]| (0x7f800000 when n = 0)
hipError_t launch_absmin(const float* v, int64_t n, unsigned* out, hipStream_t s);
int nnls_gtile_index(int r, int c);  // block(r) >= block(c): NNLS tile layout, diagonal tiles full

// Eigenbasis of the src Gram on the device (eig.hip): W = B_sᵀ·B_t_in (warm start), M = Wᵀ G W, cyclic
// Jacobi in fp64 -> P (eigenvectors, in scratch), P32 (fp32 [KP][KP]), lam32 = max(Λ, 0), ub = the
// rotation's column-scale bound (float bits), B_t_out = B_s·P.  G, B_s, B_t: fp64 [KP][KP] row-major
// (B_t_in may alias B_t_out: it is read before the last GEMM writes).  scratch: eig_scratch_doubles.
size_t eig_scratch_doubles(int KP);
hipError_t launch_device_eig(int KP, int k, const double* G, const double* Bs, const double* Bt_in, double* Bt_out,
                             double* scratch, float* P32, float* lam32, unsigned* ub, hipStream_t s);
const double* eig_minmax(const double* scratch, int KP);  // device {min Λ, max Λ} of the last call
const int* eig_sweeps(const double* scratch, int KP);     // device Jacobi sweep count of the last call
constexpr int EIG_NOT_FINITE = -(1 << 30);                 // ... its value when the matrix held a NaN or an Inf
hipError_t launch_identity(double* B, int KP, hipStream_t s);
hipError_t launch_basis_t32(const double* B, float* Bt, int KP, hipStream_t s);  // Bt = (float) Bᵀ

// Seeded unit-norm Gaussian rows (global row index row0 + r) for large synthetic runs.
hipError_t launch_init_random(int KP, int kreal, float* X, int64_t n, uint64_t seed, int64_t row0, hipStream_t s);

// ALSModel.transform: out[p] = F2J sdot(U[u[p]], V[v[p]]) (NaN when u[p] < 0 or v[p] < 0).
hipError_t launch_predict(int KP, int kreal, const float* U, const float* V, const int32_t* u,
                          const int32_t* v, float* out, int64_t n, hipStream_t s);

// Top-k (topk.hip): dst rows ordered by descending ‖t_⊥‖ in the dst Gram's eigenbasis and packed as
// fp16 with per-chunk bound boxes (topk_prepare), a probe pass for the starting thresholds and the src
// features (topk_order), per-workgroup chunk masks (launch_topk_mask), an MFMA scan over the masked
// chunks, then exact F2J rescoring of the best TOPK_KC candidates with a certification bound (rows
// that fail it: topk_exact).
constexpr int TOPK_M = 4;       // leading eigen-directions of the dst Gram in the pruning bound
constexpr int TOPK_CF = 12;     // floats per chunk feature record: lo[M], hi[M], R = max ‖t_⊥‖, pad
constexpr int TOPK_SF = 8;      // floats per src feature record: s_P[M], ‖s_⊥‖, margin, ‖s‖, pad
constexpr int TOPK_SUPER = 16;  // chunks per super-chunk (mask pre-pass)
struct TopkArgs {
  const float* S;          // src factors (original basis) [*][KP]
  const float* T;          // dst factors (original basis) [n_dst][KP]
  const int32_t* src_rows; // src rows to score
  int64_t n_src;
  int64_t n_dst;
  const int32_t* dst_ids;  // raw ids of dst rows (ascending with the row index)
  int kreal;
  int k;                   // requested top-k
  int kt;                  // rank of the running threshold in the candidate lists (k <= kt <= TOPK_KC)
  float tmax_norm;         // max_j ||T_j||_2 (for the error bound)
  const void* Th;          // [n_chunks * chunk rows][KP] fp16: T[perm[p]]·tsc, zero rows past n_dst
  const uint32_t* perm;    // [n_dst] dst row of scan position p
  int64_t n_chunks;
  const double* VP;        // [TOPK_M][KP] leading eigenvectors of the dst Gram (fp64)
  const float* cfeat;      // [n_chunks][TOPK_CF] chunk bound boxes (null: no pruning)
  const void* probe;       // [TOPK_NPROBE][KP] fp16 probe rows (the largest norms), ·tsc, zero rows past n_dst
  const float* sfeat;      // [n_src][TOPK_SF] src features by scan position (order kernel output)
  const uint32_t* mask;    // [n_wg][mask_words] needed chunks per scan workgroup (null: every chunk)
  int64_t mask_words;
  float ssc, tsc;          // src / dst fp16 scales (powers of two)
  float unscale;           // 1 / (ssc·tsc): exact rescaling of the MFMA scores
  float scaled;            // ssc·tsc
  uint2* lent;             // [n_src][TOPK_CAP] candidate lists: (approx score bits, scan position) pairs
  int32_t* lcnt;           // [n_src] list lengths
  int32_t* out_ids;        // [n_src][k] raw dst ids
  float* out_scores;       // [n_src][k]
  int32_t* need_exact;     // [n_src] set when the candidate set could not be certified
  float* kth0;             // [n_src] select -> exact rescan: the certification pass's k-th exact score (or null)
  unsigned long long* scanned;  // += dst chunks scanned by each scan workgroup (or null)
  const uint32_t* out_pos;      // select: results of scan position i go to slot out_pos[i] (or i)
  const float* thr0;            // scan: starting threshold of each src position (topk_order; or null)
  // select over output slots slot0 .. slot0 + n_slots - 1 (in_pos != null: slot -> scan position,
  // the inverse of out_pos), so a pass's results can be finished and copied out range by range
  const uint32_t* in_pos;
  int64_t slot0, n_slots;
  int order_dir_bits;           // order: key bits of the direction s_P / ‖s‖ (bytes: u1, u2, u3; 0: depth only)
};
constexpr int TOPK_KC = 64;     // candidates rescored exactly per src row (k <= 64)
#ifndef ALBEDO_TOPK_NPROBE
#define ALBEDO_TOPK_NPROBE 512
#endif
constexpr int TOPK_NPROBE = ALBEDO_TOPK_NPROBE;  // probe rows of the starting thresholds (largest norms)
#ifndef ALBEDO_TOPK_BISECT
#define ALBEDO_TOPK_BISECT 16
#endif
// bisection steps of the probe threshold: the top bits of the order-preserving key; fewer than 32 leave
// a lower bound of the kt-th probe score (valid, coarser by the undecided bits)
constexpr int TOPK_BISECT = ALBEDO_TOPK_BISECT;
#ifndef ALBEDO_TOPK_KT_EXTRA
#define ALBEDO_TOPK_KT_EXTRA 16
#endif
constexpr int TOPK_CAP = 128;   // candidate list capacity per src row (compacted to 64 above TOPK_TRIG)
constexpr int TOPK_TRIG = 112;  // compaction trigger: frequent enough that thresholds follow the running kt-th best
constexpr int TOPK_MAX = 512;   // k above TOPK_KC: exact full scan (topk_exact_kernel)
int topk_chunk_rows(int KP);    // dst rows per scan chunk (Th / cfeat are padded to whole chunks)
size_t topk_sort_temp_bytes(int64_t n_dst);
// VP: [TOPK_M][KP] fp64 (device); keys: 4·n uint32, perm / nperm: 2·n uint32 ([0, n) is the result:
// scan order / descending norm), tp: [n][TOPK_M] fp64 scratch, Th / cfeat / supf (super-chunk boxes)
// as above, probe: [TOPK_NPROBE][KP] fp16
hipError_t topk_prepare(int KP, int kreal, const float* T, int64_t n_dst, float tsc, const double* VP, void* temp,
                        size_t temp_bytes, uint32_t* keys, uint32_t* perm, uint32_t* nperm, double* tp, void* Th,
                        float* cfeat, float* supf, void* probe, hipStream_t s);
hipError_t launch_topk(int KP, const TopkArgs& a, int n_cu, hipStream_t s);
hipError_t launch_topk_select(int KP, const TopkArgs& a, hipStream_t s);  // after launch_topk (the scan)
// starting thresholds + features + scan order of the src rows: keys / order 2·n_src uint32,
// thr_tmp / thr_sorted n_src floats, sf_tmp / sf_sorted n_src·TOPK_SF floats
size_t topk_order_temp_bytes(int64_t n_src);
hipError_t topk_order(int KP, const TopkArgs& a, void* temp, size_t temp_bytes, uint32_t* keys, uint32_t* order,
                      int32_t* src_sorted, float* thr_tmp, float* thr_sorted, float* sf_tmp, float* sf_sorted,
                      hipStream_t s);
// mask[wg][a.mask_words]: the chunks scan workgroup wg (rows_per_wg rows from position wg·rows_per_wg)
// can need against the starting thresholds (a.thr0, a.sfeat in scan order)
hipError_t launch_topk_mask(const TopkArgs& a, int rows_per_wg, const float* supf, int64_t n_super, uint32_t* mask,
                            hipStream_t s);
int topk_rows_per_workgroup(int KP, int64_t n_src, int n_cu);
// exact full scan for the given src-row indices (rows == null: rows 0 .. n_rows-1), any k <= TOPK_MAX
hipError_t launch_topk_exact(int KP, const TopkArgs& a, const int32_t* rows, int64_t n_rows, hipStream_t s);
// inv[perm[i]] = i for i < n
hipError_t launch_invert_perm(const uint32_t* perm, int64_t n, uint32_t* inv, hipStream_t s);
hipError_t launch_iota_i32(int32_t* out, int64_t n, int64_t start, hipStream_t s);  // out[i] = start + i
// the certification rescans without a host round trip: need[0 .. n) compacted into flags (cnt[0]: their
// count, cnt[1]: the persistent grid's work counter, both zero on entry; cnt[2] += the count), then a
// persistent exact scan over them
hipError_t launch_topk_exact_flagged(int KP, const TopkArgs& a, const int32_t* need, int64_t n, int32_t* flags, int* cnt,
                                     int n_cu, hipStream_t s);
// ---- top-k without known pairs (topk.hip, als_recommend_unseen) -------------------------------------
// The dst rows src row u excludes: entries [ptr[u], ptr[u + 1]) of `col` (ratings mode: the side's CSR,
// ascending within a row, copies allowed) or of the low halves of `key` (pairs mode: sorted keys
// src row << 32 | dst row); exactly one of col / key is set
struct UnseenExcl {
  const int64_t* ptr;
  const int32_t* col;
  const uint64_t* key;
};
size_t unseen_sort_temp_bytes(int64_t n_e);
// n_e > 0 raw (src id, dst id) pairs -> key_sorted [n_e] and ptr [n_src + 1]; a pair with an unknown id
// sorts past ptr[n_src]
hipError_t unseen_pair_ranges(const int32_t* esrc, const int32_t* edst, int64_t n_e, const int32_t* src_ids, int64_t n_src,
                              const int32_t* dst_ids, int64_t n_dst, uint64_t* key, uint64_t* key_sorted, void* temp,
                              size_t temp_bytes, int64_t* ptr, hipStream_t s);
// lists [n][depth] (raw ids, NaN-score padded) of the src rows src_rows[0 .. n) -> the first k entries not
// excluded into out [n][k] (-1 / NaN padded); a row it cannot certify: flags[atomicAdd(cnt, 1)] = its
// position.  stat[0] += entries removed, stat[2] += rows flagged
hipError_t launch_unseen_filter(const int32_t* list_ids, const float* list_scores, int depth, int k, int64_t n, int64_t n_dst,
                                const int32_t* src_rows, const int32_t* dst_ids, const UnseenExcl& x, int32_t* out_ids,
                                float* out_scores, int32_t* flags, int* cnt, unsigned long long* stat, hipStream_t s);
// exact scan of the flagged positions flags[0 .. cnt[0]) (cnt[1]: the persistent grid's work counter, zero on
// entry; n: an upper bound of the count) over the dst rows each row does not exclude, into a.out_ids /
// a.out_scores [*][a.k]; *scored += dst rows scored
hipError_t launch_unseen_exact(int KP, const TopkArgs& a, const UnseenExcl& x, const int32_t* flags, int* cnt,
                               unsigned long long* scored, int64_t n, int n_cu, hipStream_t s);
// ---- evaluation (eval.hip): RankingEvaluator.scala:83-139 on the device ----------------------------
size_t eval_sort_temp_bytes(int64_t n);
// user ids -> rows of the ascending `ids`, grouped: runs[r] (row) with counts[r] entries at
// idx_sorted[offsets[r] ..]; *n_runs on the device (host copy synchronised inside); the unknown-id run
// (row 0xFFFFFFFF) is the last one when present
hipError_t eval_group_users(const int32_t* user, int64_t n, const int32_t* ids, int64_t n_ids, void* temp,
                            size_t temp_bytes, uint32_t* row, uint32_t* row_sorted, uint32_t* idx, uint32_t* idx_sorted,
                            uint32_t* runs, int32_t* counts, int64_t* offsets, int64_t* n_runs, hipStream_t s);
// per run: the first min(k, count) items by (key desc, item asc) -> act [n_runs][k] (-1 padded), act_n
hipError_t eval_actual_lists(const uint32_t* idx_sorted, const int64_t* offsets, const int32_t* counts, int64_t n_runs,
                             const int64_t* key, const int32_t* item, int k, int32_t* act, int32_t* act_n,
                             hipStream_t s);
// ndcgAt(k) per user of pred [n][k] (raw ids of any sign; the first min(k, n_dst) entries are the list,
// the rest padding) against act; gain[i] = 1 / ln(i + 2)
hipError_t eval_ndcg(const int32_t* pred, const int32_t* act, const int32_t* act_n, int64_t n_users, int k,
                     int64_t n_dst, const double* gain, double* out, hipStream_t s);
// ---- held-out pair ranking (eval_pairs.hip): RankingMetricFormatter("als") of transform(pairs) ------
constexpr int PAIRS_SEG = 4096;  // entries one wave selects from; a longer user is cut into segments
size_t pairs_sort_temp_bytes(int64_t n, int64_t n_users);
// raw ids -> rows of the ascending tables; urow = n_u and irow = 0 when either id is unknown
hipError_t pairs_map(const int32_t* user, const int32_t* item, int64_t n, const int32_t* uids, int64_t n_u,
                     const int32_t* iids, int64_t n_i, uint32_t* urow, uint32_t* irow, hipStream_t s);
// (urow, irow) sorted by urow (stable), then runs[r] (user row) with counts[r] pairs from offsets[r]; the
// dropped pairs' run (row n_u) is the last one when present; *n_runs_host is valid on return
hipError_t pairs_group(int64_t n, int64_t n_u, void* temp, size_t temp_bytes, const uint32_t* urow,
                       uint32_t* urow_sorted, const uint32_t* irow, uint32_t* irow_sorted, uint32_t* runs,
                       int32_t* counts, int64_t* offsets, int64_t* n_runs, int64_t* n_runs_host, hipStream_t s);
// ent[p] = {bits of F2J sdot(U[urow_sorted[p]], V[irow_sorted[p]]), iids[irow_sorted[p]]} for p < n_live
hipError_t pairs_score(int KP, int kreal, const float* U, const float* V, const uint32_t* urow_sorted,
                       const uint32_t* irow_sorted, const int32_t* iids, int64_t n_live, uint2* ent, hipStream_t s);
// per run of at most PAIRS_SEG entries: the entries with rank() <= top_k in (score desc, item asc) order, cut
// to width -> items / scores [n_runs][width] (-1 / NaN padded), len; NaN scores are dropped; longer runs
// are left to pairs_select_long
hipError_t pairs_select(const uint2* ent, const int64_t* offsets, const int32_t* counts, int64_t n_runs, int top_k,
                        int width, int32_t* items, float* scores, int32_t* len, hipStream_t s);
// the runs longer than PAIRS_SEG: segment g (seg_cnt[g] <= PAIRS_SEG entries from seg_off[g]) leaves its best
// 64 keys in seg_keys[g][64]; long run j merges key_cnt[j] keys from seg_keys + key_off[j] into row run[j]
hipError_t pairs_select_long(const uint2* ent, const int64_t* seg_off, const int32_t* seg_cnt, int64_t n_seg,
                             uint64_t* seg_keys, const int64_t* key_off, const int32_t* key_cnt, const int32_t* run,
                             int64_t n_long, int top_k, int width, int32_t* items, float* scores, int32_t* len,
                             hipStream_t s);
// metric (ALS_METRIC_*) of evaluated user u: predicted list pred[pred_row[u]] ([.][pred_width], its first
// pred_len[.] entries; pred_len null: np_all for every user; pred_row null: u) against actual list
// act[act_row[u]] ([.][k] with act_n; act_row null: u); every list is cut to k
hipError_t eval_metric(int metric, const int32_t* pred, int pred_width, const int32_t* pred_len, int np_all,
                       const int32_t* pred_row, const int32_t* act, const int32_t* act_n, const int32_t* act_row,
                       int64_t n_users, int k, const double* gain, double* out, hipStream_t s);
// *out = bits of max_r ||T[r][0..kreal)||_2 computed in fp64
hipError_t launch_rownorm_max(const float* T, int64_t n, int KP, int kreal, unsigned long long* out, hipStream_t s);

// ---- the fp64 row pass (row_pass.h) under the row audit and the objective ------------------------------
struct RowPassArgs {
  const float* Y;            // src factors in the original basis, [*][KP], indexed by col
  const float* X;            // dst rows in the original basis, [n rows][KP] (local row index, like ptr)
  const int64_t* ptr;        // dst CSR of the own rows
  const int32_t* col;
  const float* val;
  const double* G;           // fp64 src Gram [KP][KP] (implicit), null when explicit
  double* GX;                // scratch [nb][KP]: G·x of the batch's rows; null when explicit
  int64_t row0, nb;          // the batch: rows [row0, row0 + nb)
  int implicit;
  double alpha;
  int64_t chunk;             // rows of more ratings are cut into chunks of this many
  const int32_t* chunk_row;  // [n_chunks] dst row of each chunk, rows ascending, a row's chunks in order
  const int32_t* chunk_idx;  // [n_chunks] chunk number within its row
  int64_t n_chunks;
  const int32_t* long_row;   // [n_long] the rows above `chunk`, ascending
  const int64_t* long_slot0; // [n_long + 1] first chunk of each
  double* partial;           // [n_chunks] chunk records of the pass's size
};
// GX[r] = G·X[row0 + r] for r < nb in fp64 (audit.hip, beside the fp64 Gram)
hipError_t launch_row_gx(int KP, const float* X, const double* G, double* GX, int64_t row0, int64_t nb, hipStream_t s);

// ---- row audit (audit.hip): the fp64 normal-equation residual of every dst row (als_audit_rows) -------
struct AuditArgs : RowPassArgs {  // partial: [n_chunks][2·KP + 2], Σ c (y·x) y, Σ w y, Σ c ‖y‖², n
  double reg;
  int nonneg;
  double gnorm;              // ‖G‖_F (0 when explicit)
  double* eta;               // out [n rows]
  int32_t* neg;              // out [n rows]: nonneg and a component of x below zero
};
struct AuditSummary {
  long long over, non_finite, negative;
  long long worst_row;       // -1: no rows
  double worst_eta, sum;
};
constexpr int AUDIT_SUM_BLOCKS = 1024;  // records of launch_audit_summary's first pass (`part`)
// G = Σ x xᵀ over rows [0, n) of X in fp64 throughout; slab: nblk·KP·KP doubles, nblk = audit_gram_blocks(n)
int audit_gram_blocks(int64_t n);
hipError_t launch_audit_gram(int KP, const float* X, int64_t n, double* slab, int nblk, double* G, hipStream_t s);
// the partial records of every chunk of the long rows (once per call, before the batches)
hipError_t launch_audit_chunks(int KP, const AuditArgs& g, hipStream_t s);
// one batch: G·x, the rows of at most `chunk` ratings, then the long rows [l0, l0 + n_long) of the list,
// which are the batch's
hipError_t launch_audit_rows(int KP, const AuditArgs& g, int64_t l0, int64_t n_long, hipStream_t s);
// rows with !(eta <= tol), non-finite and negative counts, the worst row and Σ eta, added in a fixed order
hipError_t launch_audit_summary(const double* eta, const int32_t* neg, int64_t n, double tol, AuditSummary* part,
                                AuditSummary* out, hipStream_t s);

// ---- objective (objective.hip): the loss ALS minimises, per dst row and summed (als_objective) ---------
// A dst row's record, OBJ_REC doubles: the columns launch_objective_colsum adds
enum { OBJ_ALL_PAIRS = 0, OBJ_RATINGS, OBJ_REG, OBJ_SSE, OBJ_ABS, OBJ_DEGREE, OBJ_LOSS, OBJ_REC = 8 };
constexpr int OBJ_CHUNK_REC = 4;       // a chunk's record: Σ t, Σ (r − s)², Σ |terms|, n
constexpr int OBJ_SUM_BLOCKS = 1024;   // rows of launch_objective_colsum's first pass (`part`)
struct ObjectiveArgs : RowPassArgs {  // partial: [n_chunks][OBJ_CHUNK_REC]
  double reg;
  double* rec;               // out [n rows][OBJ_REC]
};
// the partial records of every chunk of the long rows (once per call, before the batches)
hipError_t launch_objective_chunks(int KP, const ObjectiveArgs& g, hipStream_t s);
// one batch: G·x, the rows of at most `chunk` ratings, then the long rows [l0, l0 + n_long) of the list
hipError_t launch_objective_rows(int KP, const ObjectiveArgs& g, int64_t l0, int64_t n_long, hipStream_t s);
// out[i] = n_i·‖y_i‖² over the n rows of a side from its own CSR: n_i = ratings > 0 (val null: the degree)
hipError_t launch_objective_other(int KP, const float* Y, const int64_t* ptr, const float* val, int64_t n, double* out,
                                  hipStream_t s);
// out[w] = Σ_i in[i][w] over the n rows of in [n][W] (W <= OBJ_REC) in a fixed order; part: OBJ_SUM_BLOCKS·W doubles
hipError_t launch_objective_colsum(const double* in, int64_t n, int W, double* part, double* out, hipStream_t s);

// ---- fold-in (foldin.hip): factors of new rows from the frozen other side (als_fold_in) ----------------
constexpr int FOLD_TILE = 32;  // ratings gathered into LDS per build step
// The triples as a CSR over the distinct row ids.  Sort key: the row id (sign bit flipped) above the src
// row, 0xFFFFFFFF for a src id the model does not know, so a row's dropped triples end its range.
struct FoldCsr {
  uint64_t *key, *key_sorted;  // [n]
  float* val_sorted;           // [n] ratings in key order
  uint32_t *hi, *col;          // [n] the two halves of the sorted keys: row key, src row
  uint32_t* runs;              // [n] distinct row keys, ascending
  int32_t* counts;             // [n + 1] triples per row, dropped ones included
  int64_t* ptr;                // [n + 1] first triple of each row
  int64_t* n_rows;             // device count of distinct rows
  int32_t* ids;                // [n] raw id of each row
  uint32_t *deg, *deg_sorted;  // [n] surviving triples per row
  int32_t *iota, *order;       // [n] order: the rows by descending degree (ties: ascending id)
};
size_t fold_sort_temp_bytes(int64_t n);
// map + sort + run lengths + degrees + solve order of n > 0 triples (id_front.h: find_id, split_keys_kernel,
// group_runs, degree_order); *n_rows_host is valid on return
hipError_t fold_build_csr(const int32_t* row_id, const int32_t* src_id, const float* rating, int64_t n,
                          const int32_t* src_ids, int64_t n_src, void* temp, size_t temp_bytes, const FoldCsr& f,
                          int64_t* n_rows_host, hipStream_t s);
struct FoldArgs {
  const float* Y;         // src factors in the original basis, [n_src][KP]
  const double* G;        // fp64 src Gram [KP][KP] (implicit), null when explicit
  const int64_t* ptr;     // FoldCsr::ptr
  const uint32_t* deg;    // FoldCsr::deg: the first deg[r] triples of row r are the live ones
  const uint32_t* col;
  const float* val;
  const int32_t* order;   // list position -> row
  int64_t n_rows;
  int k;                  // the model rank: the system is k x k
  int implicit;
  double alpha, reg;
  double* scratch;        // KP = 256: fold_scratch_doubles of packed triangles, one per workgroup
  int* bad;               // atomicMin of the rows that met a pivot <= 0 or NaN (caller sets it to INT_MAX)
  float* X;               // out [n_rows][k], row order (degree-0 rows: zeros)
  int nonnegative;        // Spark's NNLS.solve in place of the Cholesky factorisation
  unsigned long long* stats;  // nonnegative: [4] NNLS iterations summed and their maximum, rows solved, rows at
                              // the iteration limit (integer atomics; the caller clears them)
};
int fold_workgroups(int KP, int64_t n_rows, int n_cu);  // the persistent grid (ALBEDO_FOLD_WGS caps it)
size_t fold_scratch_doubles(int KP, int n_wg);
hipError_t launch_fold_solve(int KP, const FoldArgs& a, int n_wg, hipStream_t s);

// ---- explain (explain.hip): each rating's share of a fold-in row's score for a target (als_explain) ----
constexpr int EXPLAIN_TB = 8;       // targets a workgroup solves and scores at a time
constexpr int EXPLAIN_MAX_M = 64;   // entries of a list: one per lane of the wave that keeps it
constexpr uint32_t EXPLAIN_NONE = 0xFFFFFFFFu;  // the row of a pair that cannot be explained
// The pairs over the fold-in's CSR.  Sort key: the CSR row of the pair's row id (EXPLAIN_NONE when no triple has
// that id or the model does not know the target) above the pair's input position, so the sorted order is
// fixed, every row's pairs are a range and the pairs that cannot be explained end the list.
struct ExplainPairs {
  uint64_t *key, *key_sorted;  // [n_pairs]
  uint32_t* target;            // [n_pairs] src row of the target, by input position
  uint32_t *hi, *slot;         // [n_pairs] the two halves of the sorted keys: CSR row, input position
  uint32_t* runs;              // [n_pairs] the distinct CSR rows ascending (the last may be EXPLAIN_NONE)
  int32_t* counts;             // [n_pairs + 1]
  int64_t* ptr;                // [n_pairs + 1] each listed row's range of the sorted pairs
  int64_t* n_runs;             // device scalar
  uint32_t *deg, *deg_sorted;  // [n_pairs] the listed rows' degrees (0 for EXPLAIN_NONE)
  int32_t *iota, *order;       // [n_pairs] order: the listed rows by descending degree
};
size_t explain_sort_temp_bytes(int64_t n_pairs);
// map + sort + run lengths + solve order of n_pairs > 0 pairs over the CSR rows row_ids [n_rows] (FoldCsr::ids,
// ascending) with degrees row_deg, through the same id_front.h pieces as fold_build_csr; *n_runs_host is valid
// on return
hipError_t explain_map_pairs(const int32_t* pair_row_id, const int32_t* pair_target_id, int64_t n_pairs,
                             const int32_t* row_ids, const uint32_t* row_deg, int64_t n_rows, const int32_t* src_ids,
                             int64_t n_src, void* temp, size_t temp_bytes, const ExplainPairs& e, int64_t* n_runs_host,
                             hipStream_t s);
struct ExplainArgs {
  FoldArgs f;              // the fold-in's Y, G, CSR, k, parameters, scratch and bad (order, n_rows, X, stats unused)
  const uint32_t* runs;    // ExplainPairs::runs, ptr, order, slot, target
  const int64_t* pptr;
  const int32_t* order;
  int64_t n_runs;
  const uint32_t* slot;
  const uint32_t* target;
  const int32_t* src_ids;  // raw ids of the src rows, ascending
  int m;                   // 1 .. EXPLAIN_MAX_M
  double* total;           // out [n_pairs], by input position
  int32_t* ids;            // out [n_pairs][m]
  double* contrib;         // out [n_pairs][m]
};
// total = NaN, ids = -1, contrib = NaN: what a pair that cannot be explained, and the padding, keep
hipError_t launch_explain_fill(int64_t n_pairs, int m, double* total, int32_t* ids, double* contrib, hipStream_t s);
// the persistent grid is the fold-in's (fold_workgroups, fold_scratch_doubles)
hipError_t launch_explain(int KP, const ExplainArgs& a, int n_wg, hipStream_t s);

// ---- query top-k (query_topk.hip): exact top-k of caller-supplied vectors (als_recommend_vectors) ------
constexpr int QT_Q = 16;  // queries a workgroup scores at a time
struct QueryPlan {
  int64_t slice_rows, n_slices, n_qtiles;  // grid of the scan: n_slices dst slices x n_qtiles tiles of QT_Q queries
};
// slice size from the CU count (ALBEDO_QUERY_SLICE_ROWS in the environment overrides it)
QueryPlan query_plan(int64_t n_dst, int64_t n_q, int n_cu);
size_t query_sort_temp_bytes(int64_t n_e);
// key_sorted [n_e]: (query << 32 | dst row), ascending; row 0xFFFFFFFF for an id the model does not know.
// excl_ptr [n_q + 1] starts at 0 and ends at n_e (device, like every pointer here)
hipError_t query_map_exclusions(const int64_t* excl_ptr, int64_t n_q, const int32_t* excl_ids, int64_t n_e,
                                const int32_t* dst_ids, int64_t n_dst, uint64_t* key, uint64_t* key_sorted, void* temp,
                                size_t temp_bytes, hipStream_t s);
// part_score / part_row [n_slices][n_q][k]: each slice's best k per query, row 0xFFFFFFFF past its length.
// excl_ptr null: no exclusions
hipError_t launch_query_scan(int KP, int rank, const float* Y, int64_t n_dst, const float* q, int64_t n_q, int k,
                             const int64_t* excl_ptr, const uint64_t* excl_key, const QueryPlan& p, float* part_score,
                             uint32_t* part_row, int n_cu, hipStream_t s);
// ids_out / scores_out [n_q][k]: raw ids and scores in (score desc, row asc) order, -1 / NaN padded
hipError_t launch_query_merge(const float* part_score, const uint32_t* part_row, int64_t n_slices, int64_t n_q, int k,
                              const int32_t* dst_ids, int32_t* ids_out, float* scores_out, hipStream_t s);

// Ingest (ingest.hip): COO -> remap + CSR.
struct DeviceBuf;
hipError_t remap_ids(const int32_t* d_ids, int64_t n, int32_t* d_dense, int32_t** d_unique,
                     int64_t* n_unique, hipStream_t s);
hipError_t build_csr(const int32_t* d_dst, const int32_t* d_src, const float* d_val, int64_t n,
                     int64_t n_dst, int64_t n_src, int64_t* d_ptr, int32_t* d_col, float* d_valout,
                     hipStream_t s);
// Shard row starts of one side (world + 1 entries, world <= 16), passed by value to kernels.
struct ShardStarts {
  int64_t s[17];
  int world;
};
// out[e] = gathered-layout position of dense src row in[e]: local row l of rank r at
// (l / chpad)·world·chpad + r·chpad + l % chpad (chunk-major: one chunk of every rank is contiguous)
hipError_t padded_remap(const int32_t* d_in, int64_t n, const ShardStarts& st, int64_t chpad, int32_t* d_out,
                        hipStream_t s);
// Failure diagnostics (not on the hot path): over n values of p (fp32, or fp16 when f16),
// out[0] += non-finite count, out[1] = min index of a non-finite value (atomicMin; caller sets it to
// ~0), out[2] = max |finite value| as float bits (atomicMax; caller zeroes it)
hipError_t launch_diag_scan(const void* p, int64_t n, bool f16, unsigned long long* out, hipStream_t s);
// Synthetic generator (synth.hip)
hipError_t synth_fill(uint64_t seed, int rounds, int64_t n_users, int64_t n_items,
                      const int64_t* d_deg_prefix, const double* d_cw, const int32_t* d_perm,
                      int32_t* d_user, int32_t* d_item, float* d_rating, int64_t n_slots,
                      int64_t* n_out, hipStream_t s);

// ---- similarity within one side (similar.hip): the unit image behind als_similar / als_similar_vectors ----
// out [n][ld_out]: row i of `in` ([n][ld_in], `rank` columns used) divided by the square root of its F2J
// sdot with itself, columns past `rank` zero; a row without a direction (!(s > 0 && s < inf)) is NaN and
// flag[i] = 0 (flag may be null).  in and out must not overlap
hipError_t launch_similar_unit(const float* in, int64_t ld_in, int64_t n, int rank, float* out, int64_t ld_out,
                               int32_t* flag, hipStream_t s);
// q [n_q][rank]: the unit rows `rows[i]` (null: row i), NaN for a negative row or one without a direction;
// excl_ptr [n_q + 1] and excl_key [n_q]: each query's own row as its one exclusion, sorted as
// launch_query_scan reads them
hipError_t launch_similar_gather(const float* unit, int KP, int rank, const int32_t* flag, const int32_t* rows, int64_t n_q,
                                 float* q, int64_t* excl_ptr, uint64_t* excl_key, hipStream_t s);
// out [n][KP]: rows `rows[j]` of the image, in that order
hipError_t launch_similar_compact(const float* unit, int KP, const int32_t* rows, int64_t n, float* out, hipStream_t s);

}  // namespace albedo
