// What the host translation units share (als_engine.cpp: contexts, ingest, init, the C ABI;
// sweep_host.cpp: the row layout and the half-sweep; topk_host.cpp: top-k and NDCG; eval_host.cpp:
// held-out pair ranking; audit_host.cpp: the row audit; objective_host.cpp: the training loss, both
// over row_plan.h; foldin_host.cpp: the fold-in; explain_host.cpp: the explanation, both over fold_host.h;
// query_topk_host.cpp: top-k of caller-supplied vectors, with the exclusion lists and the scan tier that
// similar_host.cpp (cosine top-k within one side) runs too):
// error reporting, the device buffer, the
// stream guards, the row buckets, the per-side state, the context and the few functions one file calls
// in another.  Not part of the public C ABI (include/albedo_als.h).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <string>
#include <vector>

#include "albedo_als.h"

namespace albedo {

// records the message als_last_error returns on this thread (one thread_local, in als_engine.cpp)
int fail(int code, const std::string& msg);

#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess)                                                                          \
      return fail(e_ == hipErrorOutOfMemory ? ALS_E_OUT_OF_MEMORY : ALS_E_HIP,                     \
                  std::string("HIP error: ") + hipGetErrorString(e_) + " in " #x);                 \
  } while (0)
#define TRYC(x)                    \
  do {                             \
    int rc_ = (x);                 \
    if (rc_ != ALS_OK) return rc_; \
  } while (0)
#define NCCLCHK(x)                                                                                 \
  do {                                                                                             \
    ncclResult_t r_ = (x);                                                                         \
    if (r_ != ncclSuccess) return fail(ALS_E_RCCL, std::string("RCCL error: ") + ncclGetErrorString(r_) + " in " #x); \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;  // false: a view of another context's buffer (als_fork), never freed here
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    owned = true;
  }
  void share(const DevBuf& o) {
    release();
    p = o.p;
    bytes = o.bytes;
    owned = false;
  }
  hipError_t ensure(size_t b) {
    if (!owned) return hipErrorNotSupported;  // a view (als_fork) is never resized or written through
    if (b <= bytes && p) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, b ? b : 16);
    if (e == hipSuccess) bytes = b;
    return e;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// An owned non-blocking stream / event (null until created); destroyed without waiting, so whoever
// holds one synchronises before it goes
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { reset(); }
  bool create() {
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
    return s != nullptr;
  }
  void reset() {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
  }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { reset(); }
  bool create() {
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    return e != nullptr;
  }
  void reset() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
};

// Declared after the buffers a call queues work on, so that it goes first: whatever way the call
// returns, a failed launch included, the stream is drained before a buffer is freed
struct Drain {
  hipStream_t s;
  ~Drain() {
    if (s) (void)hipStreamSynchronize(s);
  }
};

// one stage mark: an event created in the empty slot *e and recorded on s
inline hipError_t mark_event(hipEvent_t* e, hipStream_t s) {
  hipError_t r = hipEventCreate(e);
  if (r != hipSuccess) return r;
  return hipEventRecord(*e, s);
}

template <int N>
struct Marks {  // stage marks on the stream
  hipEvent_t e[N] = {};
  Marks() = default;
  Marks(const Marks&) = delete;
  Marks& operator=(const Marks&) = delete;
  ~Marks() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipError_t mark(int i, hipStream_t s) { return mark_event(&e[i], s); }
};

// Row buckets, one table row each, in list order: the order of Side::d_rows, which fixes the launch
// order and the layout the chunked solve indexes (Side::cb), so it is not degree order.
//   D      the solve_light_kernel<KP, D> instance (degree <= D); 0: B_HEAVY, the explicit k x k path
//   light  counted as light by als_path_stats and timed with ALS_T_SOLVE_LIGHT: the buckets within the
//          light limit.  B_M80 (degree 65..80, above the default limit of 64) runs the push-through
//          kernel too but counts, and is timed, with the rows above the limit
//   tier   exists only with the degree tiers on (als_ctx::tiers), empty otherwise
enum { B_L16 = 0, B_L32, B_L48, B_L64, B_L96, B_M80, B_HEAVY, NBUCKET };
struct Bucket {
  int D;
  bool light, tier;
};
constexpr Bucket BUCKETS[NBUCKET] = {{16, true, false}, {32, true, false}, {48, true, true}, {64, true, false},
                                     {96, true, false}, {80, false, true}, {0, false, false}};
// the light buckets come first: B_LIGHT_END is where the light / heavy timer event goes, and the rows
// from Side::boff[B_LIGHT_END] on are the rows above the light limit
constexpr int light_bucket_end() {
  int b = 0;
  while (b < NBUCKET && BUCKETS[b].light) ++b;
  return b;
}
constexpr int B_LIGHT_END = light_bucket_end();
constexpr bool buckets_well_formed() {
  for (int b = B_LIGHT_END; b < NBUCKET; ++b)
    if (BUCKETS[b].light) return false;
  return BUCKETS[B_L16].D == 16 && BUCKETS[B_HEAVY].D == 0;  // light16.hip takes B_L16, whatever the table says
}
static_assert(buckets_well_formed(), "light buckets first, B_L16 and B_HEAVY in their places");

struct Side {
  int64_t n = 0;                 // rows (unique raw ids)
  std::vector<int32_t> ids;      // ascending
  std::vector<int64_t> starts;   // shard starts over dense rows (world + 1)
  int64_t maxrows = 0;           // max own rows over ranks
  // Gathered (padded) layout, chunk-major so that one chunk of every rank is contiguous: rank r's
  // local row i sits at (i / chpad)·world·chpad + r·chpad + i % chpad.  world = 1: nch = 1 and
  // the position is i.  prows() = nch·world·chpad rows.
  int nch = 1, world = 1;
  int64_t chpad = 0;
  int64_t own0 = 0, own_n = 0;   // this rank's dense row range
  // dst CSR of this side restricted to own rows (local row index; col = padded src position)
  DevBuf d_ptr, d_col, d_val;
  int64_t own_nnz = 0;
  std::vector<int64_t> h_deg;    // degree per own row
  DevBuf d_rows;                 // own local rows grouped by bucket
  DevBuf d_desc;                 // int4 per d_rows entry: {row, p0 lo, p0 hi, degree} (light16 prefetch)
  int64_t boff[NBUCKET + 1] = {0};
  int64_t bnnz[NBUCKET] = {0};
  float vmax = 0.f;              // max |rating| over own dst rows (heavy-build fp16 scaling)
  float vmin = 0.f;              // min |rating| over own dst rows: vmin == vmax -> one confidence c
  DevBuf d_X;                    // [own_n][KP] factors in basis B
  DevBuf d_Z;                    // [prows][KP] rotated factors (src role), gathered layout
  DevBuf d_Xfull;                // world > 1: [prows][KP] every rank's X (basis B), gathered layout
  bool full_valid = false;       // d_Xfull holds the current X (gathered behind the solve on st2)
  int64_t prows() const { return (int64_t)nch * world * chpad; }
  int64_t pos(int r, int64_t i) const { return (i / chpad) * world * chpad + (int64_t)r * chpad + i % chpad; }
  DevBuf d_B;                    // fp64 [KP][KP] orthogonal basis on the device: original = X · Bᵀ
  DevBuf d_Gk;                   // fp64 [KP][KP] last Gram of this side (as src), in basis d_GB
  DevBuf d_GB;                   // fp64 [KP][KP] the side's basis when d_Gk was computed (G_orig = GB G GBᵀ)
  bool has_gram = false;
  bool has_factors = false;
  double t[ALS_T_COUNT] = {0};
  int64_t stats[4] = {0};
  int64_t solver[4] = {0};       // NNLS iterations: sum over rows, max, rows (last half-sweep)
  DevBuf d_orig;                 // [n][KP] original-basis factors, dense order (materialised)
  bool orig_valid = false;
  DevBuf d_foldG;                // fp64 [KP][KP] Gram of d_orig, formed and used by als_fold_in alone
  bool fold_gram_valid = false;  // d_foldG is the Gram of the current factors (cleared with orig_valid)
  // split-K of the heavy tail: the first n_split heavy rows (degree > split chunk), their chunks
  int64_t n_split = 0, n_chunks = 0;
  DevBuf d_chunk_row, d_chunk_idx, d_slot0;
  // nonnegative: the first n_batch rows of the (degree-ascending) light list go to the lockstep
  // NNLS kernel, rows [bat_off[v], bat_off[v+1]) with BATCH_SLOTS[v] slots per workgroup
  int64_t n_batch = 0, n_batch_nnz = 0;
  int64_t bat_off[6] = {0};
  // solve chunks (world > 1, Cholesky path): chunk q's rows of bucket b are the list positions
  // [cb[b][q], cb[b][q + 1]); its split-K rows are the first split_n[q] of its heavy segment, their
  // chunk lists start at ck_off[q] and their (chunk-local) slot0 at sl_off[q]
  int nsolve = 1;
  int64_t cb[NBUCKET][9] = {{0}};
  int64_t c8[8] = {0};           // bucket B_L16, solve chunk q: its first c8[q] rows have degree <= 8 (paired)
  int64_t split_n[8] = {0}, ck_off[9] = {0}, sl_off[8] = {0};
};

}  // namespace albedo

struct als_ctx {
  using DevBuf = albedo::DevBuf;
  using Side = albedo::Side;
  als_params p{};
  int KP = 0;
  int dev = 0;
  hipStream_t st = nullptr;
  int rank = 0, world = 1;
  ncclComm_t comm = nullptr;
  // host transport (tests: several processes sharing one GPU exchange through the host)
  int (*h_allreduce)(void*, double*, int64_t) = nullptr;
  int (*h_allgather)(void*, float*, int64_t) = nullptr;
  void* h_user = nullptr;
  Side s[2];
  int64_t nnz = 0;
  bool has_ratings = false;
  bool model_only = false;
  DevBuf slab, d_G, d_P, d_lam, d_err, d_Gt, d_cs, d_csmax;
  DevBuf d_eig;                  // device eigensolver scratch (eig.hip)
  DevBuf d_partial, d_reduced;   // split-K partial / reduced A' records (shared by both sides)
  DevBuf d_Zhl;                  // pre-split src rows of the uniform-confidence heavy build
  DevBuf d_Pf;                   // P's bf16 parts in MFMA fragment order (rotate_bf)
  DevBuf d_iters;                // NNLS iteration counters (sum, max)
  DevBuf d_gfrag, d_counter;     // lockstep NNLS: G in MFMA operand order, row counter
  int n_cu = 256;
  // top-k counters, cumulative: [0] rows through the MFMA scan, [1] rows re-scored by the exact scan
  // (certification misses), [2] dst chunks scanned, [3] dst chunks a full scan would take
  int64_t topk_stats[4] = {0, 0, 0, 0};
  // top-k device time, cumulative (ms, HIP events on st): [0] order + mask, [1] MFMA scan, [2] select,
  // [3] exact rescans; [4] scan flops (2·KP per src x dst pair the scan's waves scored)
  double topk_ms[5] = {0, 0, 0, 0, 0};
  // device time of the last pair-ranking call (ms): map, sort, score, select, metric (als_eval_pairs_timing)
  double eval_ms[5] = {0, 0, 0, 0, 0};
  // device time of the last als_fold_in call (ms): map + sort + CSR, src Gram, solve, total
  double fold_ms[4] = {0, 0, 0, 0};
  // NNLS iterations of the last als_fold_in call: sum, maximum, rows solved, rows at the limit (0 after Cholesky)
  int64_t fold_stats[4] = {0, 0, 0, 0};
  // device time of the last als_explain call (ms): map + sort + CSR of triples and pairs, src Gram, solve, total
  double explain_ms[4] = {0, 0, 0, 0};
  // device time of the last als_objective call (ms): src Gram, row pass + sums, total
  double objective_ms[3] = {0, 0, 0};
  // device time of the last als_recommend_vectors call (ms): exclusion map + sort, scan, merge, total
  double query_ms[4] = {0, 0, 0, 0};
  // the last als_recommend_unseen call: known src rows served, rows sent to the exact scan, list entries the
  // filter removed, dst rows the exact scan scored; device ms: exclusion map + sort, lists, filter, exact
  // scan, total
  int64_t unseen_stats[4] = {0, 0, 0, 0};
  double unseen_ms[5] = {0, 0, 0, 0, 0};
  // the last als_similar / als_similar_vectors call: device ms of the unit image, the lists (scan or passes),
  // merge / filter, total; rows asked and known, rows of the side without a direction, tier (0 scan,
  // 1 passes), rows the passes tier sent to its exact scan
  double similar_ms[4] = {0, 0, 0, 0};
  int64_t similar_stats[4] = {0, 0, 0, 0};
  hipEvent_t evt[5] = {};
  // src ids the last als_recommend / als_evaluate_ndcg sent to the exact rescan, built on demand
  // (als_topk_last_rescan) from the device flags of that call: position p of the call's rows was
  // rescanned when d_last_need[p] != 0; its src row is p (last_rows_dense) or last_rows[p]
  mutable std::vector<int32_t> last_rescan;
  DevBuf d_last_need;
  double* h_plan = nullptr;      // pinned: the top-k plan's dst Gram [KP][KP] + two max row norms
  int64_t last_need_n = 0;
  std::vector<int32_t> last_rows;
  mutable bool last_rescan_ready = true;
  bool last_rows_dense = false;
  int last_src = 0;
  int split_len = 0;             // ratings per split-K chunk (0: no split)
  bool tiers = false;            // degree tiers D = 48 / D = 80 in the row layout (rank_layout)
  int slab_blocks = 0;
  hipEvent_t ev[8] = {};         // half-sweep stage timers (sweep_host.cpp EV_*)
  hipStream_t st2 = nullptr;     // world > 1: factor-chunk gathers behind the solve
  // als_fork: a fork views its parent's ingest buffers; the parent is freed after its last fork
  als_ctx* parent = nullptr;
  int forks = 0;
  bool doomed = false;
  hipEvent_t evc[9] = {};        // per solve chunk: done on st; [EVC_GATHERED]: gathers done on st2
};

namespace albedo {

// Ordering of a sharded context's two streams (world > 1), kept by sweep_host.cpp half_sweep:
//   1. the previous half's factor gathers (st2) finish before any collective or rotation of the next
//      half is issued: st waits on evc[EVC_GATHERED] first.  Two RCCL operations of one communicator
//      must never overlap;
//   2. solve chunk q's gather (st2) waits on evc[q], recorded on st behind the chunk's last solve;
//   3. evc[EVC_GATHERED], recorded on st2 behind the last gather, closes the half's gathers; whoever
//      reads d_Xfull or issues a collective on st (materialize) waits on it.
constexpr int EVC_GATHERED = 8;

int set_device(als_ctx* c);
// A context of rank `rank` on `device` with its streams and events and nothing else: what als_model_create
// fills from host arrays and als_similar's passes tier from device buffers.  Freed with als_destroy
int bare_context(int32_t rank, int32_t device, als_ctx** out);
// both streams idle: before anything rewrites factor buffers with engine-stream copies, or returns to
// the caller as "done" (world > 1: the last half's gathers run on st2 behind the solve)
int drain(als_ctx* c);
// Copies between the host and the context's buffers go through the engine stream c->st and complete
// before returning (als_engine.cpp)
hipError_t copy_st(const als_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
float event_ms(hipEvent_t a, hipEvent_t b);
// original-basis factors of `side`, dense order, on device: d_orig [n][KP]
int materialize(als_ctx* c, int side);
// world > 1, the first half of materialize: this rank's rows of `side` rotated into the original basis
// (own: [nch·chpad][KP], zero past own_n) and, when `padded` is given, every rank's rows gathered into
// the padded layout ([prows][KP], what the other side's CSR col indexes).  Queued on c->st.
int original_rows(als_ctx* c, int side, DevBuf* own, DevBuf* padded);
int64_t find_row(const Side& S, int32_t id);  // dense row of a raw id, -1 when unknown
// all-gather of host blocks: buf holds world blocks of n floats (this rank's filled)
int allgather_host(als_ctx* c, float* buf, int64_t n);

// ---- objective_host.cpp --------------------------------------------------------------------------
// ALS_E_STATE without ratings, ALS_E_UNSUPPORTED for world > 1; `who` names the caller in the message
int objective_ready(const als_ctx* c, const char* who);
// als_objective behind its argument checks: dst side t, both sides hold factors, the device is set
int objective(als_ctx* c, int t, double* row_loss_out, als_objective_t* out);

// ---- query_topk_host.cpp -------------------------------------------------------------------------
// The exclusion lists of als_recommend_vectors and als_similar_vectors (`who`, named in the messages): checks
// excl_ptr [n_q + 1] and *excl_ids; *ptr0 becomes the ranges shifted to start at 0, empty when the call has
// none, and *excl_ids moves to the first range.  More than 2^31 - 1 exclusions return `too_many`, the one
// code the two calls do not share
int exclusion_ranges(const char* who, int too_many, int64_t n_q, const int64_t* excl_ptr, const int32_t** excl_ids,
                     std::vector<int64_t>* ptr0);
// Those lists on the device, declared before the caller's Drain.  upload queues the copies on c->st (nothing
// when ptr0 is empty); map leaves each query's range of `keys` ascending (query_map_exclusions) against the
// id table d_ids [n_dst]
struct Exclusions {
  DevBuf d_ptr, d_eid, d_key, d_keys, d_tmp;
  int64_t n_e = 0;
  size_t temp_bytes = 0;
  int upload(als_ctx* c, int64_t n_q, const std::vector<int64_t>& ptr0, const int32_t* excl_ids);
  int map(als_ctx* c, int64_t n_q, const int32_t* d_ids, int64_t n_dst);
  const int64_t* ptr() const { return n_e > 0 ? d_ptr.as<int64_t>() : nullptr; }  // null: no exclusions
  const uint64_t* keys() const { return n_e > 0 ? d_keys.as<uint64_t>() : nullptr; }
};
// The slice partials and the lists of the scan tier, declared before the caller's Drain.  The caller chooses
// where ensure's four allocations fall among its stage marks
struct ScanBuffers {
  DevBuf d_ps, d_pr, d_oi, d_os;
  int ensure(const als_ctx* c, int64_t n_dst, int64_t n_q, int k);
};
// The scan tier on device inputs: the k best rows of d_Y [n_dst][KP] for each query of d_q [n_q][rank], less
// its exclusions, as raw ids in ids_out / scores_out on the host; the stream is synchronised on return.  The
// events of scan done and merge done go into the two empty slots: the caller's timing is its own
int scan_lists(als_ctx* c, const ScanBuffers& b, int k, const float* d_Y, int64_t n_dst, const float* d_q, int64_t n_q,
               const int64_t* d_ptr, const uint64_t* d_keys, const int32_t* d_ids, hipEvent_t* scan_done,
               hipEvent_t* merge_done, int32_t* ids_out, float* scores_out);

// ---- sweep_host.cpp ------------------------------------------------------------------------------
// Everything that depends on the rank / light-row limit rather than on the ratings: degree buckets,
// split-K lists, then factor_buffers.  Called after ingest and again by als_set_params.
int rank_layout(als_ctx* c);
// The solve path (ALS_PATH_*) that layout gives own row r of side T (als_audit_rows' worst_path)
int row_path(const als_ctx* c, const Side& T, int64_t r);
// Sum of c->d_G ([KP][KP] fp64) over the ranks, on c->st (nothing to do when world = 1)
int allreduce_G(als_ctx* c);
// Per-fit device state (factor buffers, Gram slabs, scratch); the factors are dropped
int factor_buffers(als_ctx* c);
// Gathers layout chunks [q0, q1) of the own rows `own` ([nch·chpad][KP], zero past own_n) into
// `full` ([prows][KP]) on stream s: chunk q of every rank is one contiguous all-gather.
int gather_chunks(als_ctx* c, const Side& S, const float* own, float* full, int q0, int q1, hipStream_t s);
// One computeFactors call: dst side t solved from the other side's factors
int half_sweep(als_ctx* c, int t);

}  // namespace albedo
