// The half-sweep of libalbedo_als.so (one Spark computeFactors call) and the row layout it solves
// over.  rank_layout() sorts a side's rows into the buckets of engine.h; half_sweep() is
//   prepare_src   the src side made ready: Gram, eigenbasis and rotation (implicit), a copy (explicit),
//                 or the Gram in tile layout and the gather (nonnegative); column scales, operand split
//   solve_rows    every dst row: bucket by bucket per solve chunk (Cholesky), or the lockstep variants
//                 and the per-row kernel (NNLS)
//   finish_half   one read-back, then timings, statistics and the error returns
// with one SolveArgs builder (solve_args) and one table from timer events to ALS_T_* (STAGES).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"

using namespace albedo;

namespace {

hipError_t fill_st(const als_ctx* c, void* dst, int v, size_t bytes) {
  if (bytes == 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(dst, v, bytes, c->st);
  return e != hipSuccess ? e : hipStreamSynchronize(c->st);
}

// ---- row layout -----------------------------------------------------------------------------------
// Rows of degree <= light_limit take the push-through solve (a d x d system).  d <= 64 by default;
// light_max_degree up to 96 (KP = 128) routes rows of degree 65..96 through the d x d path too
// (solve_light_kernel<128, 96>), measured against the explicit k x k wave kernel in DESIGN §4.
// The limit is also what als_path_stats calls "light"; the degree tiers below do not move it.
int64_t light_limit(const als_ctx* c) {
  if (c->p.light_max_degree >= 0) return std::min<int64_t>(c->p.light_max_degree, c->KP == 128 ? 96 : 64);
  return c->KP >= 128 ? 64 : 32;
}

// Degree tiers (KP = 128, the default light limit, Cholesky path): rows of degree 33..48 take
// solve_light_kernel<128, 48> (3 panels, 6 tiles instead of 4 and 10) and rows of degree 65..80, which
// are above the light limit, take solve_light_kernel<128, 80> at three waves per SIMD instead of the
// wave kernel.  An explicit light_max_degree keeps the routing it names.
// ALBEDO_DEGREE_TIERS=0 switches the tiers off (the A/B handle, read when the row layout is built).
bool degree_tiers_on(const als_ctx* c) {
  if (c->KP != 128 || c->p.light_max_degree != -1 || c->p.nonnegative) return false;
  const char* e = std::getenv("ALBEDO_DEGREE_TIERS");
  return !(e && *e && std::atoi(e) == 0);
}

// The bucket of a row of degree d (engine.h BUCKETS): on its side of the light limit, the smallest
// instance D >= d among the buckets that exist; B_HEAVY when there is none
int bucket_of(int64_t d, int64_t lmax, bool tiers) {
  int best = B_HEAVY;
  for (int b = 0; b < B_HEAVY; ++b) {
    const Bucket& k = BUCKETS[b];
    if ((k.tier && !tiers) || k.light != (d <= lmax) || d > k.D) continue;
    if (best == B_HEAVY || k.D < BUCKETS[best].D) best = b;
  }
  return best;
}

// Ratings per split-K chunk.  One workgroup gathering a 10^6-star row is the launch's tail (45.9
// ms for 1.05M stars at rank 128, more than a whole c4 half-sweep at 8 GPUs), and a partial of 8192
// ratings keeps every fp32 MFMA accumulation to 256 steps before the fp64 sum (a 1.05M-star row then
// matches the fp64 solve to 7e-7, tests/test_gpu_heavy_tail.py).  ALBEDO_SPLIT_CHUNK overrides it
// for tuning (0 disables the split): 2048 / 4096 / 16384 measured 338 / 324 / 311 ms per c4 sweep
// against 316 ms.
int split_chunk_len() {
  const char* e = std::getenv("ALBEDO_SPLIT_CHUNK");
  if (e && *e) return std::max(0, std::atoi(e));
  return 8192;
}

// nonnegative = true: light rows run in lockstep (nnls_batch.hip), BATCH_SLOTS[v] rows per workgroup
// for degrees up to nnls_batch_max_degree(KP, slots).  A lockstep iteration costs about the same for
// any slot count, so the variants pay off down to 8 slots (KP = 256 per row-iteration, tools/probe/
// batchtime: 16 slots 1.3 us, 8 slots 2.2 us, 4 slots 4.7 us against 4.5 us for solve_nnls_kernel);
// rows of higher degree take solve_nnls_kernel.
constexpr int BATCH_SLOTS[5] = {16, 8, 4, 2, 1};
constexpr int BATCH_MIN_SLOTS = 8;
int nnls_min_slots() {  // ALBEDO_NNLS_MIN_SLOTS: A/B knob (16, 8, 4, 2 or 1)
  const char* e = std::getenv("ALBEDO_NNLS_MIN_SLOTS");
  const int v = e && *e ? std::atoi(e) : BATCH_MIN_SLOTS;
  return (v == 16 || v == 8 || v == 4 || v == 2 || v == 1) ? v : BATCH_MIN_SLOTS;
}
int64_t nnls_batch_rows_limit(const als_ctx* c, int v) {
  if (BATCH_SLOTS[v] < nnls_min_slots()) return 0;
  return std::min<int64_t>(nnls_batch_max_degree(c->KP, BATCH_SLOTS[v]), light_limit(c));
}

using BucketRows = std::vector<int32_t>[NBUCKET];

// Degree buckets (heavy rows longest first for the tail) and, for nonnegative, the lockstep offsets
void bucket_rows(const als_ctx* c, Side& S, BucketRows& rows) {
  const int64_t lmax = light_limit(c);
  for (int b = 0; b < NBUCKET; ++b) S.bnnz[b] = 0;
  for (int64_t r = 0; r < S.own_n; ++r) {
    const int b = bucket_of(S.h_deg[r], lmax, c->tiers);
    rows[b].push_back((int32_t)r);
    S.bnnz[b] += S.h_deg[r];
  }
  std::stable_sort(rows[B_HEAVY].begin(), rows[B_HEAVY].end(),
                   [&](int32_t a, int32_t b) { return S.h_deg[a] > S.h_deg[b]; });
  S.n_batch = S.n_batch_nnz = 0;
  for (int v = 0; v < 6; ++v) S.bat_off[v] = 0;
  if (!c->p.nonnegative) return;
  // light rows by ascending degree: the lockstep NNLS kernel's rows first
  for (int b = 0; b < B_HEAVY; ++b)
    std::stable_sort(rows[b].begin(), rows[b].end(), [&](int32_t x, int32_t y) { return S.h_deg[x] < S.h_deg[y]; });
  // variant v takes the degrees (limit of v-1, limit of v]; the light list is one ascending run
  int64_t pos = 0;
  std::vector<int32_t> light;
  for (int b = 0; b < B_HEAVY; ++b) light.insert(light.end(), rows[b].begin(), rows[b].end());
  for (int v = 0; v < 5; ++v) {
    const int64_t dl = nnls_batch_rows_limit(c, v);
    while (pos < (int64_t)light.size() && S.h_deg[light[pos]] <= dl) S.n_batch_nnz += S.h_deg[light[pos++]];
    S.bat_off[v + 1] = pos;
  }
  S.n_batch = pos;
}

// world > 1 (Cholesky path): each bucket's rows grouped by solve chunk (= gathered-layout chunk,
// local row / chpad), stably, so a chunk's rows of a bucket are one contiguous run of the list `all`
// (S.cb); B_L16: within a chunk the rows of degree <= 8 first (light16 pairs them), counted in S.c8
void group_by_chunk(const als_ctx* c, Side& S, BucketRows& rows, std::vector<int32_t>& all) {
  const int nsolve = (c->world > 1 && !c->p.nonnegative) ? S.nch : 1;
  S.nsolve = nsolve;
  auto chunk_of = [&](int32_t r) { return nsolve == 1 ? 0 : (int)std::min<int64_t>(r / S.chpad, nsolve - 1); };
  all.reserve(S.own_n);
  for (int b = 0; b < NBUCKET; ++b) {
    S.boff[b] = (int64_t)all.size();
    const bool pairs = b == B_L16;
    std::stable_sort(rows[b].begin(), rows[b].end(), [&](int32_t x, int32_t y) {
      const int cx = chunk_of(x), cy = chunk_of(y);
      if (cx != cy || !pairs) return cx < cy;
      return (S.h_deg[x] <= 8) > (S.h_deg[y] <= 8);
    });
    int64_t p = 0;
    for (int q = 0; q <= nsolve; ++q) {
      while (q < nsolve && p < (int64_t)rows[b].size() && chunk_of(rows[b][p]) < q) ++p;
      S.cb[b][q] = S.boff[b] + (q == nsolve ? (int64_t)rows[b].size() : p);
    }
    if (pairs)
      for (int q = 0; q < nsolve; ++q) {
        int64_t k = 0;
        for (int64_t i = S.cb[b][q] - S.boff[b]; i < S.cb[b][q + 1] - S.boff[b] && S.h_deg[rows[b][i]] <= 8; ++i) ++k;
        S.c8[q] = k;
      }
    all.insert(all.end(), rows[b].begin(), rows[b].end());
  }
  S.boff[NBUCKET] = (int64_t)all.size();
}

// Split-K chunks of each solve chunk's heaviest rows (a prefix of its heavy run: by degree); slot0 is
// chunk-local (starts at 0 for every solve chunk)
int split_lists(als_ctx* c, Side& S, const std::vector<int32_t>& all) {
  const int64_t CH = c->split_len;
  std::vector<int32_t> crow, cidx, slot0;
  S.n_split = 0;
  for (int q = 0; q < S.nsolve; ++q) {
    S.ck_off[q] = (int64_t)crow.size();
    S.sl_off[q] = (int64_t)slot0.size();
    slot0.push_back(0);
    int64_t n = 0;
    for (int64_t p = S.cb[B_HEAVY][q]; p < S.cb[B_HEAVY][q + 1]; ++p) {
      const int32_t r = all[p];
      if (CH <= 0 || S.h_deg[r] <= CH) break;
      const int64_t nch = (S.h_deg[r] + CH - 1) / CH;
      for (int64_t k = 0; k < nch; ++k) {
        crow.push_back(r);
        cidx.push_back((int32_t)k);
      }
      slot0.push_back((int32_t)((int64_t)crow.size() - S.ck_off[q]));
      ++n;
    }
    S.split_n[q] = n;
    S.n_split += n;
  }
  S.ck_off[S.nsolve] = (int64_t)crow.size();
  S.n_chunks = (int64_t)crow.size();
  if (S.n_split > 0) {
    HIPCHK(S.d_chunk_row.ensure(crow.size() * 4));
    HIPCHK(S.d_chunk_idx.ensure(cidx.size() * 4));
    HIPCHK(S.d_slot0.ensure(slot0.size() * 4));
    HIPCHK(copy_st(c, S.d_chunk_row.p, crow.data(), crow.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, S.d_chunk_idx.p, cidx.data(), cidx.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, S.d_slot0.p, slot0.data(), slot0.size() * 4, hipMemcpyHostToDevice));
  }
  return ALS_OK;
}

}  // namespace

// Called after ingest and again by als_set_params, so several fits (a CV grid) share one ingest.
int albedo::rank_layout(als_ctx* c) {
  TRYC(drain(c));
  c->split_len = split_chunk_len();
  c->tiers = degree_tiers_on(c);
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    BucketRows rows;
    std::vector<int32_t> all;
    bucket_rows(c, S, rows);
    group_by_chunk(c, S, rows, all);
    HIPCHK(S.d_rows.ensure(all.size() * 4));
    HIPCHK(copy_st(c, S.d_rows.p, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(S.d_desc.ensure(all.size() * 16));
    HIPCHK(launch_row_desc(S.d_rows.as<int32_t>(), (int64_t)all.size(), S.d_ptr.as<int64_t>(), S.d_desc.as<int32_t>(), c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    TRYC(split_lists(c, S, all));
  }
  return factor_buffers(c);
}

// The ALS_PATH_* of own row r of side T: what bucket_rows, group_by_chunk and split_lists above make of
// its degree.  nonnegative: the lockstep kernel takes the light list's rows up to the largest degree
// limit of its variants (the list is degree-ascending), the per-row kernel every other row, split-K
// rows included.  The layout's routing only: a half that forced the explicit path is not reflected.
int albedo::row_path(const als_ctx* c, const Side& T, int64_t r) {
  const int64_t d = T.h_deg[r];
  if (c->p.nonnegative) {
    int64_t lim = 0;
    for (int v = 0; v < 5; ++v) lim = std::max(lim, nnls_batch_rows_limit(c, v));
    return d <= lim ? ALS_PATH_NNLS_LOCKSTEP : ALS_PATH_NNLS_ROW;
  }
  switch (bucket_of(d, light_limit(c), c->tiers)) {
    case B_L16: return d <= 8 ? ALS_PATH_LIGHT16_PAIR : ALS_PATH_LIGHT16;
    case B_L32: return ALS_PATH_LIGHT32;
    case B_L48: return ALS_PATH_LIGHT48;
    case B_L64: return ALS_PATH_LIGHT64;
    case B_L96: return ALS_PATH_LIGHT96;
    case B_M80: return ALS_PATH_TIER80;
    default: return c->split_len > 0 && d > c->split_len ? ALS_PATH_SPLIT : ALS_PATH_EXPLICIT;
  }
}

// Per-fit device state: split-K records, factor / rotated-factor buffers, Gram slabs and scratch;
// the factors are dropped (the next fit initialises them).
int albedo::factor_buffers(als_ctx* c) {
  {
    const size_t rec = (size_t)split_rec_floats(c->KP) * 4;
    const int64_t mc = std::max(c->s[0].n_chunks, c->s[1].n_chunks);
    const int64_t ms = std::max(c->s[0].n_split, c->s[1].n_split);
    if (mc > 0) {
      HIPCHK(c->d_partial.ensure(mc * rec));
      HIPCHK(c->d_reduced.ensure(ms * rec));
    }
  }
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    // X padded to whole layout chunks (zero rows past own_n: they travel in the chunk gathers)
    HIPCHK(S.d_X.ensure((size_t)std::max<int64_t>(std::max<int64_t>(S.own_n, (int64_t)S.nch * S.chpad), 1) * c->KP * 4));
    // + one zero row at prows(): the gather target of masked light-row entries (never written)
    HIPCHK(S.d_Z.ensure((size_t)(S.prows() + 1) * c->KP * 4));
    HIPCHK(fill_st(c, S.d_X.p, 0, S.d_X.bytes));
    HIPCHK(fill_st(c, S.d_Z.p, 0, S.d_Z.bytes));
    if (c->world > 1) {
      HIPCHK(S.d_Xfull.ensure((size_t)std::max<int64_t>(S.prows(), 1) * c->KP * 4));
      HIPCHK(fill_st(c, S.d_Xfull.p, 0, S.d_Xfull.bytes));
    }
    S.full_valid = false;
    HIPCHK(S.d_B.ensure((size_t)c->KP * c->KP * 8));
    HIPCHK(S.d_Gk.ensure((size_t)c->KP * c->KP * 8));
    HIPCHK(S.d_GB.ensure((size_t)c->KP * c->KP * 8));
    HIPCHK(launch_identity(S.d_B.as<double>(), c->KP, c->st));
    S.has_gram = false;
    S.has_factors = false;
    S.orig_valid = false;
    S.fold_gram_valid = false;
    S.full_valid = false;
  }
  const int64_t maxsrc = std::max(c->s[0].own_n, c->s[1].own_n);
  c->slab_blocks = gram_slab_blocks(c->KP, maxsrc);
  HIPCHK(c->slab.ensure(gram_slab_doubles(c->KP, c->slab_blocks) * 8));
  HIPCHK(c->d_G.ensure((size_t)c->KP * c->KP * 8));
  HIPCHK(c->d_P.ensure((size_t)c->KP * c->KP * 4));
  HIPCHK(c->d_eig.ensure(eig_scratch_doubles(c->KP) * 8));
  HIPCHK(c->d_lam.ensure((size_t)c->KP * 4));
  HIPCHK(c->d_err.ensure(16));
  HIPCHK(c->d_cs.ensure((size_t)2 * c->KP * 4));
  HIPCHK(c->d_csmax.ensure((size_t)c->KP * 4));
  return ALS_OK;
}

// ---- collectives ------------------------------------------------------------------------------
int albedo::allreduce_G(als_ctx* c) {
  const int64_t n = (int64_t)c->KP * c->KP;
  if (c->world == 1) return ALS_OK;
  if (c->comm) {
    NCCLCHK(ncclAllReduce(c->d_G.p, c->d_G.p, n, ncclDouble, ncclSum, c->comm, c->st));
    return ALS_OK;
  }
  std::vector<double> h(n);
  HIPCHK(hipMemcpyAsync(h.data(), c->d_G.p, n * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (c->h_allreduce(c->h_user, h.data(), n) != 0) return fail(ALS_E_RCCL, "host all-reduce callback failed");
  HIPCHK(hipMemcpyAsync(c->d_G.p, h.data(), n * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return ALS_OK;
}

namespace {

// in-place all-gather on stream s: rank r's rows_per_rank rows at buf + r·rows_per_rank·KP
int allgather_rows(als_ctx* c, float* buf, int64_t rows_per_rank, hipStream_t s) {
  if (c->world == 1) return ALS_OK;
  const int64_t per = rows_per_rank * c->KP;
  if (c->comm) {
    NCCLCHK(ncclAllGather(buf + (int64_t)c->rank * per, buf, per, ncclFloat, c->comm, s));
    return ALS_OK;
  }
  std::vector<float> h((size_t)per * c->world);
  HIPCHK(hipMemcpyAsync(h.data() + (size_t)c->rank * per, buf + (int64_t)c->rank * per, per * 4,
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (c->h_allgather(c->h_user, h.data(), per) != 0) return fail(ALS_E_RCCL, "host all-gather callback failed");
  HIPCHK(hipMemcpyAsync(buf, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return ALS_OK;
}

}  // namespace

int albedo::gather_chunks(als_ctx* c, const Side& S, const float* own, float* full, int q0, int q1, hipStream_t s) {
  const int64_t per = S.chpad * c->KP;
  for (int q = q0; q < q1; ++q) {
    float* base = full + (int64_t)q * c->world * per;
    HIPCHK(hipMemcpyAsync(base + (int64_t)c->rank * per, own + (int64_t)q * per, per * 4, hipMemcpyDeviceToDevice, s));
    TRYC(allgather_rows(c, base, S.chpad, s));
  }
  return ALS_OK;
}

// ---- the half-sweep -------------------------------------------------------------------------------
namespace {

// Timer events (als_ctx::ev), in the order a half records them on the engine stream.  A stage of
// als_last_timings is the time between two of them (STAGES); what lies between a pair no stage names
// (NNLS: the upload of the Gram tiles, the column scales) is in ALS_T_HALF_TOTAL only.
enum {
  EV_BEGIN,    // behind the wait for the previous half's gathers
  EV_GRAM,     // Gram + all-reduce done (NNLS: and read back)
  EV_EIG,      // eigenbasis and dst basis done (explicit: lam cleared, basis copied; NNLS: Gram tiles uploaded)
  EV_ROTATE,   // Z written: rotation, or the copy of the src factors
  EV_PREP,     // Cholesky: column scales and operand split done, the solve starts.  NNLS: src gathered
  EV_SCALED,   // NNLS only: column scales done, the solve starts
  EV_LIGHT,    // light buckets done (NNLS: lockstep kernel done; chunked Cholesky: every chunk done)
  EV_END,
  EV_COUNT
};
static_assert(EV_COUNT == sizeof(als_ctx::ev) / sizeof(hipEvent_t), "one timer event per name");

// How a half's rows were solved, as far as the timers care
enum HalfKind {
  HALF_ONE_CHUNK,  // Cholesky, one solve chunk
  HALF_CHUNKED,    // Cholesky, nsolve > 1 (sharded): the whole solve is timed as heavy, light = 0
  HALF_NNLS        // eig = 0, light = the lockstep kernel, heavy = the per-row kernels (split-K included)
};
struct Span {
  int from, to;  // from == to: the path has no such stage, 0 ms
};
// indexed by ALS_T_GRAM .. ALS_T_HALF_TOTAL
constexpr Span STAGES[3][ALS_T_HALF_TOTAL + 1] = {
    {{EV_BEGIN, EV_GRAM}, {EV_GRAM, EV_EIG}, {EV_EIG, EV_ROTATE}, {EV_ROTATE, EV_PREP}, {EV_PREP, EV_LIGHT},
     {EV_LIGHT, EV_END}, {EV_BEGIN, EV_END}},
    {{EV_BEGIN, EV_GRAM}, {EV_GRAM, EV_EIG}, {EV_EIG, EV_ROTATE}, {EV_ROTATE, EV_PREP}, {EV_PREP, EV_PREP},
     {EV_PREP, EV_LIGHT}, {EV_BEGIN, EV_END}},
    {{EV_BEGIN, EV_GRAM}, {EV_EIG, EV_EIG}, {EV_EIG, EV_ROTATE}, {EV_ROTATE, EV_PREP}, {EV_SCALED, EV_LIGHT},
     {EV_LIGHT, EV_END}, {EV_BEGIN, EV_END}}};
static_assert(ALS_T_GRAM == 0 && ALS_T_EIG == 1 && ALS_T_ROTATE == 2 && ALS_T_COMM == 3 && ALS_T_SOLVE_LIGHT == 4 &&
                  ALS_T_SOLVE_HEAVY == 5 && ALS_T_HALF_TOTAL == 6,
              "STAGES is written in this order");

int mark(als_ctx* c, int ev) {
  HIPCHK(hipEventRecord(c->ev[ev], c->st));
  return ALS_OK;
}

// What prepare_src leaves for the solve and for the diagnostics of a failed one
struct Prepared {
  bool force_heavy = false;  // every row takes the explicit k x k path (light_max_degree = 0, or regParam = 0)
  const void* zhl = nullptr;  // pre-split src rows (presplit), or null
  float wsc = 1.f, inv_sw = 1.f;
  int64_t src_rows = 0;  // rows of Z this half wrote (failure_diag)
  float gscale = 1.0f;   // NNLS: the lockstep kernel's power-of-two scale of G
  std::vector<float> gt;  // NNLS: host copy of the Gram tiles; the queued upload reads it until the half's sync
};

// fp16 column scales of the heavy build for dst side T over the gathered src rows Z
// have_max: the rotation left the column maxima of Z in d_csmax (rotate_kernel's epilogue)
int column_scales(als_ctx* c, const Side& S, const Side& T, bool have_max = false) {
  const float cmax = c->p.implicit_prefs ? (float)c->p.alpha * T.vmax : 1.0f;
  HIPCHK(launch_colscale(c->KP, S.d_Z.as<float>(), S.prows(), cmax, c->d_csmax.as<unsigned>(),
                         c->d_cs.as<float>(), c->st, have_max));
  return ALS_OK;
}

// KP = 128: the rotation on bf16 MFMA with the fused operand split (rotate_bf); KP = 64 / 256 keep the
// fp32 MFMA rotation + colmax epilogue + separate presplit pass
bool rotate_bf_on(const als_ctx* c) { return c->KP == 128; }

// One confidence c for every rating of dst side T (explicit: c = 1; implicit: all |r| equal): the
// heavy build's operand split z·√c·colscale -> fp16 hi + lo is then the same for every gather of a
// src row, so it runs once per src row here (launch_presplit) instead of once per gathered rating
// inside the wave kernel.
// presplit_wanted: whether the split applies to this half (and its √c); split_done: the rotation
// already wrote it (rotate_bf)
bool presplit_wanted(const als_ctx* c, const Side& T, float* sw) {
  const bool uniform = !c->p.implicit_prefs || (T.vmin == T.vmax && T.vmax > 0.f);
  // rows above the light limit (from B_LIGHT_END on): the tier bucket among them counts, since a
  // forced-heavy half sends it to the explicit path
  if (!uniform || !explicit_reads_presplit(c->KP) || T.boff[NBUCKET] == T.boff[B_LIGHT_END]) return false;
  const float cw = c->p.implicit_prefs ? (float)c->p.alpha * T.vmax : 1.0f;
  if (!(cw > 0.f)) return false;
  *sw = std::sqrt(cw);
  return true;
}

int presplit(als_ctx* c, const Side& S, const Side& T, Prepared* P, bool split_done) {
  float sw = 1.f;
  if (!presplit_wanted(c, T, &sw)) return ALS_OK;
  const float cw = c->p.implicit_prefs ? (float)c->p.alpha * T.vmax : 1.0f;
  HIPCHK(c->d_Zhl.ensure((size_t)(S.prows() + 1) * c->KP * 4));
  if (!split_done)
    HIPCHK(launch_presplit(c->KP, S.d_Z.as<float>(), S.prows(), c->d_cs.as<float>(), sw, c->d_Zhl.p, c->st));
  // b' weights w = 1 + c (implicit, r > 0) or r (explicit), scaled by a power of two below 2^13
  const double wmax = c->p.implicit_prefs ? 1.0 + (double)cw : (double)T.vmax;
  int e = 0;
  std::frexp(wmax > 0.0 ? wmax : 1.0, &e);  // wmax < 2^e
  P->wsc = (float)std::ldexp(1.0, std::max(-60, std::min(60, 13 - e)));
  P->inv_sw = 1.0f / sw;
  P->zhl = c->d_Zhl.p;
  return ALS_OK;
}

// Where the column scales of a Cholesky half come from
enum Scales {
  SCALES_BY_ROTATION,  // rotate_bf: the scales came first (from the eigenvalue bound) and it wrote the split
  SCALES_FROM_MAXIMA,  // the fp32 rotation left the column maxima of Z in d_csmax
  SCALES_BY_SCAN       // explicit: colscale scans Z
};

// The end of both Cholesky preparations, Z written: column scales, operand split, cleared error flags
int scales_and_split(als_ctx* c, const Side& S, const Side& T, Scales how, Prepared* P) {
  TRYC(mark(c, EV_ROTATE));
  if (how != SCALES_BY_ROTATION) TRYC(column_scales(c, S, T, how == SCALES_FROM_MAXIMA));
  TRYC(presplit(c, S, T, P, how == SCALES_BY_ROTATION));
  TRYC(mark(c, EV_PREP));
  HIPCHK(hipMemsetAsync(c->d_err.p, 0, 4, c->st));
  return ALS_OK;
}

// implicitPrefs: G = Σ y yᵀ [+ all-reduce], G = P Λ Pᵀ on the device, Z = X_src · P
int prepare_implicit(als_ctx* c, Side& S, Side& T, Prepared* P) {
  const int KP = c->KP;
  hipStream_t st = c->st;
  const bool multi = c->world > 1;
  HIPCHK(launch_gram(KP, S.d_X.as<float>(), S.own_n, c->slab.as<double>(), c->slab_blocks, c->d_G.as<double>(), st));
  TRYC(allreduce_G(c));
  TRYC(mark(c, EV_GRAM));
  // eigenbasis of the src Gram on the device (eig.hip): warm-started cyclic Jacobi in fp64, no host
  // round trip; the dst side's new basis B_t = B_s·P is formed there too
  HIPCHK(hipMemcpyAsync(S.d_Gk.p, c->d_G.p, (size_t)KP * KP * 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(S.d_GB.p, S.d_B.p, (size_t)KP * KP * 8, hipMemcpyDeviceToDevice, st));
  S.has_gram = true;
  HIPCHK(launch_device_eig(KP, c->p.rank, c->d_G.as<double>(), S.d_B.as<double>(), T.d_B.as<double>(), T.d_B.as<double>(),
                           c->d_eig.as<double>(), c->d_P.as<float>(), c->d_lam.as<float>(), c->d_csmax.as<unsigned>(), st));
  bool singular = false;  // regParam = 0 and min Λ <= 1e-12 max Λ
  if (c->p.reg_param == 0.0) {
    // the push-through light solve needs Λ + λn > 0 for every row; with λ = 0 a singular Gram sends
    // every row to the explicit path (the only host round trip left, and only at regParam = 0)
    double wmm[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(wmm, eig_minmax(c->d_eig.as<double>(), KP), 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!(wmm[0] > 1e-12 * wmm[1])) P->force_heavy = singular = true;
  }
  TRYC(mark(c, EV_EIG));
  // world > 1: every rank rotates the whole gathered src (no collective on the critical path)
  const float* Xs = multi ? S.d_Xfull.as<float>() : S.d_X.as<float>();
  const int64_t ns = multi ? S.prows() : S.own_n;
  P->src_rows = ns;
  // regParam = 0 on a near-singular Gram: nothing but Σ c z² stands on the diagonal of a small
  // eigen-direction, and that bound's floor of 1e-6 λ_max is decades above its column of Z, whose fp16
  // hi + lo split then keeps too few bits (1.3e-4 on a row at rank 128 with one src column at 2^-22).
  // Such a half takes the fp32 rotation below, whose column scales come from the measured maxima.
  if (rotate_bf_on(c) && !singular) {
    // bf16 MFMA rotation with the heavy build's split in the same pass.  Its column scales come
    // first, from a bound: Σ_i Z_ij² = p_jᵀ G p_j, which is λ_j up to the fp32 rounding of P and of
    // the product (≤ 1e-6 λ_max), so max_i |Z_ij| ≤ √(λ_j + 1e-6 λ_max).  The split's fp16 range
    // needs the scaled maxima below 2^16; the scales put the bound at 2^13 (colscale_kernel).
    // (the bound itself came from the eigensolver: launch_device_eig left it in d_csmax)
    TRYC(column_scales(c, S, T, true));
    float sw = 1.f;
    const bool split = presplit_wanted(c, T, &sw);
    if (split) HIPCHK(c->d_Zhl.ensure((size_t)(S.prows() + 1) * KP * 4));
    HIPCHK(c->d_Pf.ensure((size_t)rotate_bf_pfrag_bytes(KP)));
    HIPCHK(launch_rotate_bf(KP, Xs, c->d_P.as<float>(), c->d_Pf.p, S.d_Z.as<float>(), ns, c->d_cs.as<float>(), sw,
                            split ? c->d_Zhl.p : nullptr, S.prows(), c->n_cu, st));
    return scales_and_split(c, S, T, SCALES_BY_ROTATION, P);
  }
  // the rotation also leaves the column maxima of Z for the heavy build's column scales
  HIPCHK(hipMemsetAsync(c->d_csmax.p, 0, KP * sizeof(unsigned), st));
  HIPCHK(launch_rotate(KP, Xs, c->d_P.as<float>(), S.d_Z.as<float>(), ns, st, c->d_csmax.as<unsigned>()));
  return scales_and_split(c, S, T, SCALES_FROM_MAXIMA, P);
}

// explicit ratings: no Gram term, the solve runs in the src basis as it is (Λ = 0, B_t = B_s, Z = X_src)
int prepare_explicit(als_ctx* c, Side& S, Side& T, Prepared* P) {
  const int KP = c->KP;
  hipStream_t st = c->st;
  TRYC(mark(c, EV_GRAM));
  HIPCHK(hipMemsetAsync(c->d_lam.p, 0, KP * 4, st));
  HIPCHK(hipMemcpyAsync(T.d_B.p, S.d_B.p, (size_t)KP * KP * 8, hipMemcpyDeviceToDevice, st));
  if (c->p.reg_param == 0.0) P->force_heavy = true;
  TRYC(mark(c, EV_EIG));
  if (c->world > 1) HIPCHK(hipMemcpyAsync(S.d_Z.p, S.d_Xfull.p, (size_t)S.prows() * KP * 4, hipMemcpyDeviceToDevice, st));
  else HIPCHK(hipMemcpyAsync(S.d_Z.p, S.d_X.p, (size_t)S.own_n * KP * 4, hipMemcpyDeviceToDevice, st));
  P->src_rows = S.own_n;
  return scales_and_split(c, S, T, SCALES_BY_SCAN, P);
}

// nonnegative = true: Spark's NNLSSolver in the original basis (no rotation; B stays I).  The Gram
// goes back to the host for the tile layout (d_Gt) and the lockstep kernel's scale; Z = the gathered X
int prepare_nnls(als_ctx* c, Side& S, Side& T, Prepared* P) {
  const int KP = c->KP;
  hipStream_t st = c->st;
  const int ngt = nnls_gtile_floats(KP);
  std::vector<float>& gt = P->gt;
  gt.assign(ngt, 0.f);
  if (c->p.implicit_prefs) {
    HIPCHK(launch_gram(KP, S.d_X.as<float>(), S.own_n, c->slab.as<double>(), c->slab_blocks, c->d_G.as<double>(), st));
    TRYC(allreduce_G(c));
    std::vector<double> Gf((size_t)KP * KP);
    HIPCHK(hipMemcpyAsync(Gf.data(), c->d_G.p, Gf.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(S.d_Gk.p, c->d_G.p, (size_t)KP * KP * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(S.d_GB.p, S.d_B.p, (size_t)KP * KP * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    S.has_gram = true;
    for (int i = 0; i < KP; ++i)
      for (int j = 0; j < 16 * ((i >> 4) + 1); ++j) gt[nnls_gtile_index(i, j)] = (float)Gf[(size_t)i * KP + j];
    double gmax = 0.0;
    for (double v : Gf) gmax = std::max(gmax, std::fabs(v));
    if (gmax > 0.0) {  // lockstep kernel's fp16 split of G: max|G|·gscale < 2^15
      int ex = 0;
      (void)std::frexp(gmax, &ex);
      P->gscale = (float)std::ldexp(1.0, std::max(-120, std::min(120, 15 - ex)));
    }
  }
  TRYC(mark(c, EV_GRAM));
  HIPCHK(c->d_Gt.ensure((size_t)ngt * 4));
  HIPCHK(hipMemcpyAsync(c->d_Gt.p, gt.data(), (size_t)ngt * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_lam.p, 0, KP * 4, st));
  TRYC(mark(c, EV_EIG));
  if (c->world == 1) HIPCHK(hipMemcpyAsync(S.d_Z.p, S.d_X.p, (size_t)S.own_n * KP * 4, hipMemcpyDeviceToDevice, st));
  TRYC(mark(c, EV_ROTATE));
  if (c->world > 1) TRYC(gather_chunks(c, S, S.d_X.as<float>(), S.d_Z.as<float>(), 0, S.nch, st));
  TRYC(mark(c, EV_PREP));
  HIPCHK(hipMemsetAsync(c->d_err.p, 0, 4, st));
  TRYC(column_scales(c, S, T));
  return mark(c, EV_SCALED);
}

int prepare_src(als_ctx* c, Side& S, Side& T, Prepared* P) {
  if (c->p.nonnegative) return prepare_nnls(c, S, T, P);
  P->force_heavy = c->p.light_max_degree == 0;
  if (c->world > 1 && !S.full_valid) {  // src factors set outside a half-sweep (init / injection): gather now
    TRYC(gather_chunks(c, S, S.d_X.as<float>(), S.d_Xfull.as<float>(), 0, S.nch, c->st));
    S.full_valid = true;
  }
  return c->p.implicit_prefs ? prepare_implicit(c, S, T, P) : prepare_explicit(c, S, T, P);
}

// The launch arguments every solve of the half shares (rows, n_rows, desc, prebuilt and iters are set
// per launch).  Both halves get every field.  Zhl, wsc and inv_sw are read only by the one-wave
// kernels of heavy_wave.hip, and only when Zhl is set, which presplit alone does (never for NNLS);
// zero_row is read by the light kernels (als_kernels.hip, light16.hip) and by those same pre-split
// builds; n_cu is read by launch_solve_light16 alone, on the host.  The NNLS kernels
// (solve_nnls_kernel, nnls_batch.hip, nnls_row.hip, the split-K partials without Zhl) read none of them.
SolveArgs solve_args(const als_ctx* c, const Side& S, const Side& T, const Prepared& P) {
  SolveArgs a{};
  a.Zhl = P.zhl;
  a.zero_row = S.prows();
  a.wsc = P.wsc;
  a.inv_sw = P.inv_sw;
  a.Z = S.d_Z.as<float>();
  a.ptr = T.d_ptr.as<int64_t>();
  a.col = T.d_col.as<int32_t>();
  a.val = T.d_val.as<float>();
  a.lam = c->d_lam.as<float>();
  a.X = T.d_X.as<float>();
  a.kreal = c->p.rank;
  a.implicit = c->p.implicit_prefs;
  a.alpha = (float)c->p.alpha;
  a.reg = (float)c->p.reg_param;
  a.err = c->d_err.as<int>();
  a.colscale = c->d_cs.as<float>();
  a.n_cu = c->n_cu;
  return a;
}

// Explicit-path launch over rows [h0, h0 + hn) of T's bucket-ordered row list, the first split_n[q] of
// which (when h0 starts solve chunk q's heavy run) are the split-K rows: chunk partials + fp64 reduce,
// then the factor (or NNLS) from the reduced records, then the remaining rows as usual.
int heavy_launches(als_ctx* c, const Side& T, SolveArgs a, int64_t h0, int64_t hn, bool nnls, int q = 0) {
  const int KP = c->KP;
  const int32_t* rows = T.d_rows.as<int32_t>();
  int64_t ns = (h0 == T.cb[B_HEAVY][q]) ? std::min<int64_t>(T.split_n[q], hn) : 0;
  if (ns > 0) {
    SplitArgs sp{};
    sp.chunk_row = T.d_chunk_row.as<int32_t>() + T.ck_off[q];
    sp.chunk_idx = T.d_chunk_idx.as<int32_t>() + T.ck_off[q];
    sp.n_chunks = T.ck_off[q + 1] - T.ck_off[q];
    sp.chunk_len = c->split_len;
    sp.slot0 = T.d_slot0.as<int32_t>() + T.sl_off[q];
    sp.n_split = ns;
    sp.partial = c->d_partial.as<float>();
    sp.reduced = c->d_reduced.as<float>();
    HIPCHK(launch_heavy_split(KP, a, sp, c->st));
    SolveArgs b = a;
    b.rows = rows + h0;
    b.n_rows = ns;
    b.prebuilt = c->d_reduced.as<float>();
    if (nnls) HIPCHK(launch_solve_nnls(KP, b, c->d_Gt.as<float>(), c->st));
    else HIPCHK(launch_solve_explicit(KP, b, c->st));
  }
  a.rows = rows + h0 + ns;
  a.desc = T.d_desc.as<int32_t>() + 4 * (h0 + ns);  // the descriptors follow d_rows entry by entry
  a.n_rows = hn - ns;
  a.prebuilt = nullptr;
  if (nnls) HIPCHK(launch_solve_nnls(KP, a, c->d_Gt.as<float>(), c->st));
  else HIPCHK(launch_solve_explicit(KP, a, c->st));
  return ALS_OK;
}

// Cholesky path.  Solve chunk by chunk (one chunk unless world > 1); world > 1: each finished chunk of
// the new factors is gathered on the second stream while the next chunk solves (the
// ordering rules are in engine.h, beside EVC_GATHERED).  The light / heavy timer event goes in front
// of the first bucket that is not light.
int solve_rows_cholesky(als_ctx* c, const Side& T, const Prepared& P, SolveArgs a) {
  const int KP = c->KP;
  hipStream_t st = c->st;
  const bool multi = c->world > 1;
  const int32_t* rows = T.d_rows.as<int32_t>();
  for (int q = 0; q < T.nsolve; ++q) {
    for (int b = 0; b < NBUCKET; ++b) {
      if (b == B_LIGHT_END && T.nsolve == 1) TRYC(mark(c, EV_LIGHT));
      if (b == B_HEAVY) {
        TRYC(heavy_launches(c, T, a, T.cb[b][q], T.cb[b][q + 1] - T.cb[b][q], false, q));
        continue;
      }
      a.rows = rows + T.cb[b][q];
      a.desc = T.d_desc.as<int32_t>() + 4 * T.cb[b][q];
      a.n_rows = T.cb[b][q + 1] - T.cb[b][q];
      if (P.force_heavy) HIPCHK(launch_solve_explicit(KP, a, st));
      else if (b == B_L16) {  // light16.hip: degree <= 8 two rows per wave unit, then the rest
        SolveArgs p8 = a, p16 = a;
        p8.n_rows = T.c8[q];
        p16.rows += T.c8[q];
        p16.desc += 4 * T.c8[q];
        p16.n_rows -= T.c8[q];
        HIPCHK(launch_solve_light16(KP, p8, st, true));
        HIPCHK(launch_solve_light16(KP, p16, st, false));
      } else HIPCHK(launch_solve_light(KP, BUCKETS[b].D, a, st));
    }
    if (multi) {  // rule 2: chunk q's gather waits on evc[q]
      HIPCHK(hipEventRecord(c->evc[q], st));
      HIPCHK(hipStreamWaitEvent(c->st2, c->evc[q], 0));
      TRYC(gather_chunks(c, T, T.d_X.as<float>(), T.d_Xfull.as<float>(), q, q + 1, c->st2));
    }
  }
  if (T.nsolve > 1) TRYC(mark(c, EV_LIGHT));  // chunked: the whole solve is timed as heavy
  if (multi) {
    if (T.nsolve == 1) TRYC(gather_chunks(c, T, T.d_X.as<float>(), T.d_Xfull.as<float>(), 0, T.nch, c->st2));
    HIPCHK(hipEventRecord(c->evc[EVC_GATHERED], c->st2));  // rule 3
  }
  return ALS_OK;
}

// the lockstep kernel's rows: the first of the (degree-ascending) light list
int64_t lockstep_rows(const Side& T) { return std::min<int64_t>(T.n_batch, T.boff[B_HEAVY]); }

// NNLS path: the lockstep variants over the low-degree rows, then the per-row kernel over the other
// light rows and over the heavy rows (split-K first)
int solve_rows_nnls(als_ctx* c, const Side& T, const Prepared& P, SolveArgs a) {
  const int KP = c->KP;
  hipStream_t st = c->st;
  HIPCHK(c->d_iters.ensure(32));  // [sum, max] of every row, then [sum, max] of the lockstep rows
  HIPCHK(hipMemsetAsync(c->d_iters.p, 0, 32, st));
  a.iters = c->d_iters.as<unsigned long long>();
  const int64_t nb = lockstep_rows(T);
  if (nb > 0) {
    HIPCHK(c->d_gfrag.ensure((size_t)KP * KP * 4));
    HIPCHK(c->d_counter.ensure(64));
    HIPCHK(launch_nnls_gfrag(KP, c->d_Gt.as<float>(), P.gscale, c->d_gfrag.p, st));
    // ALBEDO_NNLS_BATCH_WGS caps the persistent grid (tests: force many slot refills per workgroup)
    const char* ew = std::getenv("ALBEDO_NNLS_BATCH_WGS");
    const int wgs = (ew && std::atoi(ew) > 0) ? std::min(c->n_cu, std::atoi(ew)) : c->n_cu;
    for (int v = 0; v < 5; ++v) {
      SolveArgs b = a;
      b.rows = T.d_rows.as<int32_t>() + T.bat_off[v];
      b.n_rows = T.bat_off[v + 1] - T.bat_off[v];
      b.iters = a.iters + 2;
      HIPCHK(launch_nnls_batch(KP, BATCH_SLOTS[v], b, c->d_gfrag.p, P.gscale, c->d_counter.as<unsigned int>(), wgs, st));
    }
  }
  TRYC(mark(c, EV_LIGHT));
  TRYC(heavy_launches(c, T, a, nb, T.boff[B_HEAVY] - nb, true));
  TRYC(heavy_launches(c, T, a, T.boff[B_HEAVY], T.boff[NBUCKET] - T.boff[B_HEAVY], true));
  return ALS_OK;
}

// the solve paths named by the bits of a not-positive-definite flag word (kernels.h ALBEDO_EF_*)
std::string err_paths(int err) {
  std::string r;
  const std::pair<int, const char*> names[] = {{ALBEDO_EF_LIGHT16, "light16"}, {ALBEDO_EF_LIGHT_REG, "light-d16"},
                                               {ALBEDO_EF_LIGHT_ACC, "light"}, {ALBEDO_EF_WAVE, "wave"},
                                               {ALBEDO_EF_HEAVY, "heavy"}};
  for (const auto& n : names)
    if (err & n.first) r += std::string(r.empty() ? ": " : ",") + n.second;
  return r;
}

// After a failed solve: what the half's inputs and outputs held (non-finite counts, first bad index,
// max |value|), so a failure that does not repeat still names where it started
std::string failure_diag(als_ctx* c, const Side& S, const Side& T, int64_t ns, const void* zhl) {
  const int KP = c->KP;
  struct Item {
    const char* name;
    const void* p;
    int64_t n;
    bool f16;
  } items[] = {{"src X", S.d_X.p, S.own_n * KP, false},
               {"src Z", S.d_Z.p, ns * KP, false},
               {"Z zero row", S.d_Z.as<float>() + S.prows() * KP, KP, false},
               {"Zhl", zhl, zhl ? (S.prows() + 1) * KP * 2 : 0, true},
               {"lam", c->d_lam.p, KP, false},
               {"colscale", c->d_cs.p, KP, false},
               {"dst X", T.d_X.p, T.own_n * KP, false}};
  const int ni = (int)(sizeof(items) / sizeof(items[0]));
  DevBuf out;
  std::vector<unsigned long long> h((size_t)ni * 3, 0ull);
  for (int i = 0; i < ni; ++i) h[(size_t)i * 3 + 1] = ~0ull;
  // an early return drains the stream first: the queued upload reads h and the scans write out
  auto unavailable = [&]() { (void)hipStreamSynchronize(c->st); return std::string(" [diagnostics unavailable]"); };
  if (out.ensure(h.size() * 8) != hipSuccess ||
      hipMemcpyAsync(out.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->st) != hipSuccess)
    return unavailable();
  for (int i = 0; i < ni; ++i)
    if (items[i].p && launch_diag_scan(items[i].p, items[i].n, items[i].f16, out.as<unsigned long long>() + 3 * i, c->st) != hipSuccess)
      return unavailable();
  std::vector<float> lam(KP), cs(KP);
  if (hipMemcpyAsync(h.data(), out.p, h.size() * 8, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
      hipMemcpyAsync(lam.data(), c->d_lam.p, KP * 4, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
      hipMemcpyAsync(cs.data(), c->d_cs.p, KP * 4, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
      hipStreamSynchronize(c->st) != hipSuccess)
    return unavailable();
  std::string r = " [";
  char buf[160];
  for (int i = 0; i < ni; ++i) {
    if (!items[i].p) continue;
    const unsigned mx = (unsigned)h[(size_t)i * 3 + 2];
    float fmx;
    std::memcpy(&fmx, &mx, 4);
    if (h[(size_t)i * 3])
      std::snprintf(buf, sizeof buf, "%s: %llu non-finite (first at %llu, row %llu), max %.3g; ", items[i].name,
                    h[(size_t)i * 3], h[(size_t)i * 3 + 1], h[(size_t)i * 3 + 1] / (items[i].f16 ? 2 * KP : KP), fmx);
    else std::snprintf(buf, sizeof buf, "%s: finite, max %.3g; ", items[i].name, fmx);
    r += buf;
  }
  const auto lm = std::minmax_element(lam.begin(), lam.begin() + c->p.rank);
  const auto cm = std::minmax_element(cs.begin(), cs.begin() + c->p.rank);
  std::snprintf(buf, sizeof buf, "lam %.4g..%.4g, colscale %.4g..%.4g]", *lm.first, *lm.second, *cm.first, *cm.second);
  return r + buf;
}

// als_path_stats.  Cholesky: light = the rows of the light buckets, unless the half forced every row
// onto the explicit path; the tier bucket B_M80 is above the light limit and counts with the heavy
// rows, whichever kernel solves it.  NNLS: the lockstep kernel's rows and stars, then every other row.
void path_stats(const als_ctx* c, Side& T, const Prepared& P) {
  T.stats[0] = T.stats[1] = T.stats[2] = T.stats[3] = 0;
  if (c->p.nonnegative) {
    T.stats[0] = lockstep_rows(T);
    T.stats[1] = T.stats[0] > 0 ? T.n_batch_nnz : 0;
    T.stats[2] = T.boff[NBUCKET] - T.stats[0];
    T.stats[3] = T.own_nnz - T.stats[1];
    return;
  }
  for (int b = 0; b < NBUCKET; ++b) {
    const int o = BUCKETS[b].light && !P.force_heavy ? 0 : 2;
    T.stats[o] += T.boff[b + 1] - T.boff[b];
    T.stats[o + 1] += T.bnnz[b];
  }
}

// The one read-back of a half (error flags; Jacobi sweeps or NNLS iterations), then als_last_timings,
// als_path_stats, als_solver_stats and the error returns
int finish_half(als_ctx* c, int t, const Prepared& P) {
  Side& S = c->s[1 - t];
  Side& T = c->s[t];
  const int KP = c->KP;
  hipStream_t st = c->st;
  const bool nnls = c->p.nonnegative, multi = c->world > 1;
  TRYC(mark(c, EV_END));
  int err = 0, sweeps = 0;
  unsigned long long it[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(&err, c->d_err.p, 4, hipMemcpyDeviceToHost, st));
  if (nnls) HIPCHK(hipMemcpyAsync(it, c->d_iters.p, 32, hipMemcpyDeviceToHost, st));
  else if (c->p.implicit_prefs) HIPCHK(hipMemcpyAsync(&sweeps, eig_sweeps(c->d_eig.as<double>(), KP), 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  path_stats(c, T, P);
  if (nnls) {
    T.solver[0] = (int64_t)(it[0] + it[2]);
    T.solver[1] = (int64_t)std::max(it[1], it[3]);
    T.solver[2] = T.boff[NBUCKET];
    T.solver[3] = (int64_t)it[2];
  } else {
    // Cholesky path: the device eigensolver's Jacobi sweeps (als_solver_stats), decoded like
    // als_device_eigh (eig.hip stores -(sweeps + 1) when the budget ran out)
    T.solver[0] = sweeps == EIG_NOT_FINITE ? 0 : (sweeps < 0 ? -sweeps - 1 : sweeps);
    T.solver[1] = T.solver[2] = T.solver[3] = 0;
  }
  const Span* stages = STAGES[nnls ? HALF_NNLS : (T.nsolve > 1 ? HALF_CHUNKED : HALF_ONE_CHUNK)];
  for (int i = 0; i <= ALS_T_HALF_TOTAL; ++i)
    T.t[i] = stages[i].from == stages[i].to ? 0.0 : event_ms(c->ev[stages[i].from], c->ev[stages[i].to]);
  if (nnls && (err & 4)) return fail(ALS_E_STATE, "lockstep NNLS row above its degree limit (row layout out of date)");
  if (nnls && err) return fail(ALS_E_NOT_POSITIVE_DEFINITE, "NNLS solve produced a non-finite result");
  if (sweeps == EIG_NOT_FINITE)  // eig.hip: a NaN or an Inf in the Gram (non-finite src factors, or norms past fp32)
    return fail(ALS_E_NOT_POSITIVE_DEFINITE,
                std::string("the ") + (t == ALS_USER ? "item" : "user") +
                    " Gram matrix is not finite (NaN or Inf in the source factors, or row norms past fp32): "
                    "the eigensolver did not converge");
  if (sweeps < 0)  // eig.hip: the Jacobi sweep budget ran out (the host eigensolver's "did not converge")
    return fail(ALS_E_NOT_POSITIVE_DEFINITE, "eigensolver did not converge (device Jacobi: " +
                                                 std::to_string(-sweeps - 1) + " sweeps without meeting the tolerance)");
  if (!nnls && (err & 3))
    return fail(ALS_E_NOT_POSITIVE_DEFINITE,
                "LAPACK.dppsv-equivalent Cholesky met a non-positive pivot because A is not positive "
                "definite. Is A derived from a singular matrix (e.g. collinear column values)? (flags " +
                    std::to_string(err) + err_paths(err) + ", " + std::to_string(sweeps) + " eigensolver sweeps, " +
                    (t == ALS_USER ? "user" : "item") + " half)" + failure_diag(c, S, T, P.src_rows, P.zhl));
  if (nnls) HIPCHK(hipMemcpyAsync(T.d_B.p, S.d_B.p, (size_t)KP * KP * 8, hipMemcpyDeviceToDevice, st));  // no rotation
  T.has_factors = true;
  T.orig_valid = false;
  T.fold_gram_valid = false;
  T.full_valid = multi && !nnls;  // Cholesky: gathered behind the solve (st2); the next half waits for it
  return ALS_OK;
}

}  // namespace

int albedo::half_sweep(als_ctx* c, int t) {
  Side& S = c->s[1 - t];
  Side& T = c->s[t];
  if (!S.has_factors) return fail(ALS_E_STATE, "source factors are not initialised");
  // rule 1 (engine.h, EVC_GATHERED): the previous half's gathers finish before this half's collectives
  if (c->world > 1) HIPCHK(hipStreamWaitEvent(c->st, c->evc[EVC_GATHERED], 0));
  TRYC(mark(c, EV_BEGIN));
  Prepared P;
  TRYC(prepare_src(c, S, T, &P));
  const SolveArgs a = solve_args(c, S, T, P);
  if (c->p.nonnegative) TRYC(solve_rows_nnls(c, T, P, a));
  else TRYC(solve_rows_cholesky(c, T, P, a));
  return finish_half(c, t, P);
}
