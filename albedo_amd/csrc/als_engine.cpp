// libalbedo_als.so host engine: contexts, ingest, factor initialisation and the C ABI of
// include/albedo_als.h, except top-k and NDCG (topk_host.cpp) and the held-out pair ranking
// (eval_host.cpp).  The half-sweep and the row layout it runs over are in sweep_host.cpp; engine.h is
// what the files share.
//
// Mirrors Spark MLlib 2.2.0 ALS.train as reached from ALSRecommenderBuilder.scala:46-58:
//   userFactors = initialize(...); itemFactors = initialize(...)
//   for iter in 1..maxIter: itemFactors = computeFactors(userFactors -> items)
//                           userFactors = computeFactors(itemFactors -> users)
// Each computeFactors call is one half-sweep here (sweep_host.cpp half_sweep()):
//   G = Σ y yᵀ over the src rows (MFMA, fp64 partials)    [+ all-reduce across ranks]
//   G = P Λ Pᵀ (device fp64 eigensolver);  Z = X_src · P  (every rank rotates the gathered src)
//   every dst row solved in the eigenbasis (light: push-through, heavy: explicit Cholesky)
// Factors are stored in a per-side basis B (original = X · Bᵀ); solving from src basis B_s with
// rotation P puts the dst solution in basis B_s·P, so only one rotation GEMM runs per half-sweep.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "host_math.h"
#include "kernels.h"

using namespace albedo;

namespace {

thread_local std::string g_err;
std::mutex g_fork_mu;  // parent / fork lifetimes (als_fork: forks may be destroyed from any thread)

}  // namespace

int albedo::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int albedo::set_device(als_ctx* c) {
  HIPCHK(hipSetDevice(c->dev));
  return ALS_OK;
}

// Copies between the host and the context's buffers go through the engine stream c->st and
// complete before returning.  c->st is a non-blocking stream: it does not order itself after the null
// stream, so a plain hipMemcpy / hipMemset could overlap the engine's kernels (a host-to-device
// hipMemcpy from pageable memory may return before its DMA lands, a device-to-device one does not
// wait at all, and neither waits for kernels still running on c->st).
hipError_t albedo::copy_st(const als_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->st);
  return e != hipSuccess ? e : hipStreamSynchronize(c->st);
}

// world > 1: the factor-chunk gathers of the last half-sweep run on st2 behind the solve.  Anything
// that rewrites factor buffers with default-stream copies, or returns to the caller as "done",
// first waits for both streams.
int albedo::drain(als_ctx* c) {
  if (c->st2) HIPCHK(hipStreamSynchronize(c->st2));
  if (c->st) HIPCHK(hipStreamSynchronize(c->st));
  return ALS_OK;
}

namespace {

int validate(const als_params* p) {
  auto bad = [](const char* name, double v) {
    char buf[160];
    snprintf(buf, sizeof buf, "als parameter %s given invalid value %g.", name, v);
    return fail(ALS_E_INVALID_ARGUMENT, buf);
  };
  if (p->rank < 1) return bad("rank", p->rank);
  if (p->max_iter < 0) return bad("maxIter", p->max_iter);
  if (!(p->reg_param >= 0)) return bad("regParam", p->reg_param);
  if (!(p->alpha >= 0)) return bad("alpha", p->alpha);
  if (p->num_user_blocks < 1) return bad("numUserBlocks", p->num_user_blocks);
  if (p->num_item_blocks < 1) return bad("numItemBlocks", p->num_item_blocks);
  if (padded_rank(p->rank) == 0)
    return fail(ALS_E_UNSUPPORTED, "rank " + std::to_string(p->rank) + " exceeds the compiled maximum (256)");
  return ALS_OK;
}

}  // namespace

// all-gather of host blocks: buf holds world blocks of n floats (this rank's filled); bytes are
// moved, never combined (ids travel as float bit patterns)
int albedo::allgather_host(als_ctx* c, float* buf, int64_t n) {
  if (c->world == 1) return ALS_OK;
  if (c->comm) {
    DevBuf d;
    HIPCHK(d.ensure((size_t)n * c->world * 4));
    float* dp = d.as<float>();
    HIPCHK(hipMemcpyAsync(dp + (int64_t)c->rank * n, buf + (int64_t)c->rank * n, n * 4, hipMemcpyHostToDevice, c->st));
    NCCLCHK(ncclAllGather(dp + (int64_t)c->rank * n, dp, n, ncclFloat, c->comm, c->st));
    HIPCHK(hipMemcpyAsync(buf, dp, (size_t)n * c->world * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return ALS_OK;
  }
  if (c->h_allgather(c->h_user, buf, n) != 0) return fail(ALS_E_RCCL, "host all-gather callback failed");
  return ALS_OK;
}

namespace {

// world > 1: the solve runs in this many row chunks, each gathered on a second stream while the
// next one solves
int gather_chunk_count() { return 4; }

// ---- ingest -------------------------------------------------------------------------------------
// A fork views its parent's ingest, and a parent's ingest is viewed by its live forks: neither may
// rebuild it (a re-ingest would write through the views or free buffers the forks still read).
int ingest_allowed(als_ctx* c) {
  std::lock_guard<std::mutex> lk(g_fork_mu);
  if (c->parent) return fail(ALS_E_STATE, "new ratings on a fork (set them on a fresh context instead)");
  if (c->forks > 0) return fail(ALS_E_STATE, "new ratings while forks view this context's ingest");
  return ALS_OK;
}

int ingest_device(als_ctx* c, int64_t n, const int32_t* d_user, const int32_t* d_item, const float* d_rating) {
  TRYC(ingest_allowed(c));
  if (n <= 0)
    return fail(ALS_E_INVALID_ARGUMENT, "No ratings available from the input dataset (empty ratings).");
  TRYC(set_device(c));
  // the previous top-k call's rescan flags index the old id tables: drop them before S.ids changes
  c->last_rescan.clear();
  c->last_need_n = 0;
  c->last_rows.clear();
  c->last_rescan_ready = true;
  hipStream_t st = c->st;
  DevBuf ud, id;
  HIPCHK(ud.ensure(n * 4));
  HIPCHK(id.ensure(n * 4));
  int32_t *uu = nullptr, *ii = nullptr;
  int64_t nu = 0, ni = 0;
  HIPCHK(remap_ids(d_user, n, ud.as<int32_t>(), &uu, &nu, st));
  HIPCHK(remap_ids(d_item, n, id.as<int32_t>(), &ii, &ni, st));
  Side& U = c->s[ALS_USER];
  Side& I = c->s[ALS_ITEM];
  U.n = nu;
  I.n = ni;
  U.ids.resize(nu);
  I.ids.resize(ni);
  HIPCHK(copy_st(c, U.ids.data(), uu, nu * 4, hipMemcpyDeviceToHost));
  HIPCHK(copy_st(c, I.ids.data(), ii, ni * 4, hipMemcpyDeviceToHost));
  (void)hipFree(uu);
  (void)hipFree(ii);
  c->nnz = n;
  // both orientations, full, then sliced to this rank's rows
  struct Full { DevBuf ptr, col, val; std::vector<int64_t> hptr; } full[2];
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    Full& F = full[side];
    HIPCHK(F.ptr.ensure((S.n + 1) * 8));
    HIPCHK(F.col.ensure(n * 4));
    HIPCHK(F.val.ensure(n * 4));
    const int32_t* dst = side == ALS_USER ? ud.as<int32_t>() : id.as<int32_t>();
    const int32_t* src = side == ALS_USER ? id.as<int32_t>() : ud.as<int32_t>();
    HIPCHK(build_csr(dst, src, d_rating, n, S.n, c->s[1 - side].n, F.ptr.as<int64_t>(), F.col.as<int32_t>(),
                     F.val.as<float>(), st));
    F.hptr.resize(S.n + 1);
    HIPCHK(copy_st(c, F.hptr.data(), F.ptr.p, (S.n + 1) * 8, hipMemcpyDeviceToHost));
    S.starts.assign(c->world + 1, 0);
    plan_shards(F.hptr.data(), S.n, c->world, S.starts.data());
    S.maxrows = 0;
    for (int r = 0; r < c->world; ++r) S.maxrows = std::max<int64_t>(S.maxrows, S.starts[r + 1] - S.starts[r]);
    S.own0 = S.starts[c->rank];
    S.own_n = S.starts[c->rank + 1] - S.own0;
    S.world = c->world;
    S.nch = c->world > 1 ? gather_chunk_count() : 1;
    S.chpad = std::max<int64_t>(1, (S.maxrows + S.nch - 1) / S.nch);
  }
  ud.release();
  id.release();
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    Side& Src = c->s[1 - side];
    Full& F = full[side];
    const int64_t e0 = F.hptr[S.own0], e1 = F.hptr[S.own0 + S.own_n];
    S.own_nnz = e1 - e0;
    std::vector<int64_t> lp(S.own_n + 1);
    for (int64_t r = 0; r <= S.own_n; ++r) lp[r] = F.hptr[S.own0 + r] - e0;
    HIPCHK(S.d_ptr.ensure((S.own_n + 1) * 8));
    HIPCHK(copy_st(c, S.d_ptr.p, lp.data(), (S.own_n + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(S.d_col.ensure(S.own_nnz * 4));
    HIPCHK(S.d_val.ensure(S.own_nnz * 4));
    HIPCHK(copy_st(c, S.d_val.p, F.val.as<float>() + e0, S.own_nnz * 4, hipMemcpyDeviceToDevice));
    if (c->world == 1) {
      HIPCHK(copy_st(c, S.d_col.p, F.col.as<int32_t>() + e0, S.own_nnz * 4, hipMemcpyDeviceToDevice));
    } else {  // dense src index -> padded src position, on the device
      ShardStarts ss{};
      ss.world = c->world;
      for (int r = 0; r <= c->world; ++r) ss.s[r] = Src.starts[r];
      HIPCHK(padded_remap(F.col.as<int32_t>() + e0, S.own_nnz, ss, Src.chpad, S.d_col.as<int32_t>(), st));
      HIPCHK(hipStreamSynchronize(st));
    }
    S.h_deg.resize(S.own_n);
    for (int64_t r = 0; r < S.own_n; ++r) S.h_deg[r] = lp[r + 1] - lp[r];
  }
  TRYC(rank_layout(c));
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    unsigned bits[2] = {0, 0};
    HIPCHK(launch_absmax(S.d_val.as<float>(), S.own_nnz, c->d_csmax.as<unsigned>(), st));
    HIPCHK(launch_absmin(S.d_val.as<float>(), S.own_nnz, c->d_csmax.as<unsigned>() + 1, st));
    HIPCHK(hipMemcpyAsync(bits, c->d_csmax.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&S.vmax, &bits[0], 4);
    std::memcpy(&S.vmin, &bits[1], 4);
  }
  c->has_ratings = true;
  return ALS_OK;
}

// upload host factors (dense order, [n][rank]) for this rank's own rows
int upload_factors(als_ctx* c, int side, const float* f, int64_t ld) {
  TRYC(drain(c));
  Side& S = c->s[side];
  std::vector<float> h((size_t)std::max<int64_t>(S.own_n, 1) * c->KP, 0.f);
  for (int64_t r = 0; r < S.own_n; ++r)
    std::memcpy(&h[(size_t)r * c->KP], f + (size_t)(S.own0 + r) * ld, sizeof(float) * c->p.rank);
  HIPCHK(copy_st(c, S.d_X.p, h.data(), (size_t)S.own_n * c->KP * 4, hipMemcpyHostToDevice));
  HIPCHK(launch_identity(S.d_B.as<double>(), c->KP, c->st));
  S.has_factors = true;
  S.orig_valid = false;
  S.fold_gram_valid = false;
  S.full_valid = false;
  return ALS_OK;
}

// Spark's initialize for every side that has no factors yet.  Both side seeds are always drawn
// (seedGen.nextLong twice, user first), so a side initialised here gets the same rows whether or
// not the other side was injected by the caller.
int spark_init(als_ctx* c) {
  int64_t su, si;
  spark_side_seeds(c->p.seed, &su, &si);
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    if (S.has_factors) continue;
    std::vector<float> f((size_t)S.n * c->p.rank);
    spark_initialize(S.ids.data(), S.n, c->p.rank, side == ALS_USER ? su : si,
                     side == ALS_USER ? c->p.num_user_blocks : c->p.num_item_blocks, f.data(), c->p.rank);
    TRYC(upload_factors(c, side, f.data(), c->p.rank));
  }
  return ALS_OK;
}

}  // namespace

float albedo::event_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, a, b);
  return ms;
}

int albedo::original_rows(als_ctx* c, int side, DevBuf* own, DevBuf* padded) {
  Side& S = c->s[side];
  if (!S.has_factors) return fail(ALS_E_STATE, "factors are not available (call fit first)");
  const int KP = c->KP;
  HIPCHK(c->d_P.ensure((size_t)KP * KP * 4));
  HIPCHK(launch_basis_t32(S.d_B.as<double>(), c->d_P.as<float>(), KP, c->st));
  if (c->st2) HIPCHK(hipStreamWaitEvent(c->st, c->evc[EVC_GATHERED], 0));
  const int64_t nown = (int64_t)S.nch * S.chpad;
  HIPCHK(own->ensure((size_t)nown * KP * 4));
  HIPCHK(launch_rotate(KP, S.d_X.as<float>(), c->d_P.as<float>(), own->as<float>(), nown, c->st));
  if (!padded) return ALS_OK;
  HIPCHK(padded->ensure((size_t)std::max<int64_t>(S.prows(), 1) * KP * 4));
  return gather_chunks(c, S, own->as<float>(), padded->as<float>(), 0, S.nch, c->st);
}

// original-basis factors of `side`, dense order, on device: d_orig [n][KP]
int albedo::materialize(als_ctx* c, int side) {
  Side& S = c->s[side];
  if (S.orig_valid) return ALS_OK;
  if (!S.has_factors) return fail(ALS_E_STATE, "factors are not available (call fit first)");
  const int KP = c->KP;
  HIPCHK(S.d_orig.ensure((size_t)std::max<int64_t>(S.n, 1) * KP * 4));
  if (c->world == 1) {
    HIPCHK(c->d_P.ensure((size_t)KP * KP * 4));
    HIPCHK(launch_basis_t32(S.d_B.as<double>(), c->d_P.as<float>(), KP, c->st));
    HIPCHK(launch_rotate(KP, S.d_X.as<float>(), c->d_P.as<float>(), S.d_orig.as<float>(), S.own_n, c->st));
  } else {  // rotate the own chunks, gather them, unpack the chunk-major layout into dense order
    DevBuf own, padded;
    TRYC(original_rows(c, side, &own, &padded));
    for (int r = 0; r < c->world; ++r) {
      const int64_t nr = S.starts[r + 1] - S.starts[r];
      for (int q = 0; q < S.nch && (int64_t)q * S.chpad < nr; ++q) {
        const int64_t l0 = (int64_t)q * S.chpad, cnt = std::min<int64_t>(S.chpad, nr - l0);
        HIPCHK(hipMemcpyAsync(S.d_orig.as<float>() + (size_t)(S.starts[r] + l0) * KP,
                              padded.as<float>() + (size_t)S.pos(r, l0) * KP, (size_t)cnt * KP * 4,
                              hipMemcpyDeviceToDevice, c->st));
      }
    }
    HIPCHK(hipStreamSynchronize(c->st));
  }
  HIPCHK(hipStreamSynchronize(c->st));
  S.orig_valid = true;
  return ALS_OK;
}

int64_t albedo::find_row(const Side& S, int32_t id) {
  auto it = std::lower_bound(S.ids.begin(), S.ids.end(), id);
  if (it == S.ids.end() || *it != id) return -1;
  return it - S.ids.begin();
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* als_last_error(void) { return g_err.c_str(); }
int als_abi_version(void) { return ALBEDO_ALS_ABI_VERSION; }

int als_device_count(int* out) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  int good = 0;
  for (int d = 0; d < n; ++d) {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, d) == hipSuccess && std::strncmp(pr.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  *out = good;
  return ALS_OK;
}

int als_params_default(als_params* p) {
  if (!p) return fail(ALS_E_INVALID_ARGUMENT, "null params");
  p->rank = 10;
  p->max_iter = 10;
  p->implicit_prefs = 0;
  p->nonnegative = 0;
  p->num_user_blocks = 10;
  p->num_item_blocks = 10;
  p->reg_param = 0.1;
  p->alpha = 1.0;
  p->seed = 0;
  p->device = -1;
  p->light_max_degree = -1;
  return ALS_OK;
}

static int ctx_common(const als_params* p, als_ctx** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(ALS_E_NO_DEVICE, "no HIP device visible: the ALS engine runs on MI355X (gfx950) only");
  auto* c = new als_ctx();
  c->p = *p;
  c->KP = padded_rank(p->rank);
  if (p->device >= 0) c->dev = p->device;
  else if (hipGetDevice(&c->dev) != hipSuccess) c->dev = 0;
  if (c->dev >= ndev) {
    delete c;
    return fail(ALS_E_NO_DEVICE, "device ordinal out of range");
  }
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, c->dev) != hipSuccess || std::strncmp(pr.gcnArchName, "gfx950", 6) != 0) {
    delete c;
    return fail(ALS_E_NO_DEVICE, "device is not gfx950 (MI355X)");
  }
  c->n_cu = pr.multiProcessorCount;
  if (hipSetDevice(c->dev) != hipSuccess || hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(ALS_E_HIP, "failed to create a HIP stream");
  }
  for (auto& e : c->ev) (void)hipEventCreate(&e);
  for (auto& e : c->evt) (void)hipEventCreate(&e);
  for (auto& e : c->evc) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  if (hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(ALS_E_HIP, "failed to create a HIP stream");
  }
  *out = c;
  return ALS_OK;
}

}  // extern "C"

int albedo::bare_context(int32_t rank, int32_t device, als_ctx** out) {
  *out = nullptr;
  als_params p;
  als_params_default(&p);
  p.rank = rank;
  p.device = device;
  TRYC(validate(&p));
  return ctx_common(&p, out);
}

extern "C" {

int als_create(const als_params* p, als_ctx** out) {
  if (!p || !out) return fail(ALS_E_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  TRYC(validate(p));
  return ctx_common(p, out);
}

int als_set_params(als_ctx* c, const als_params* p) {
  if (!c || !p) return fail(ALS_E_INVALID_ARGUMENT, "null argument");
  if (c->model_only) return fail(ALS_E_STATE, "als_set_params on a model-only context");
  if (c->parent) return fail(ALS_E_STATE, "als_set_params on a fork (fork the parent again instead)");
  {
    std::lock_guard<std::mutex> lk(g_fork_mu);
    if (c->forks > 0) return fail(ALS_E_STATE, "als_set_params while forks view this context's layout");
  }
  TRYC(validate(p));
  TRYC(set_device(c));
  const int dev = c->dev;
  c->p = *p;
  c->p.device = dev;  // the context stays on its device
  c->KP = padded_rank(p->rank);
  if (c->has_ratings) TRYC(rank_layout(c));  // factors are dropped: the next fit re-initialises
  return ALS_OK;
}

int als_fork(als_ctx* parent, const als_params* p, als_ctx** out) {
  if (!parent || !p || !out) return fail(ALS_E_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (!parent->has_ratings || parent->model_only) return fail(ALS_E_STATE, "als_fork needs a context holding ratings");
  if (parent->world > 1) return fail(ALS_E_UNSUPPORTED, "als_fork of a sharded (multi-rank) context");
  TRYC(validate(p));
  if (p->rank != parent->p.rank || p->nonnegative != parent->p.nonnegative ||
      p->light_max_degree != parent->p.light_max_degree)
    return fail(ALS_E_INVALID_ARGUMENT, "a fork keeps its parent's rank, nonnegative and light_max_degree");
  als_params q = *p;
  q.device = parent->dev;
  als_ctx* c = nullptr;
  TRYC(ctx_common(&q, &c));
  // the ingest and the rank layout are the parent's (read-only during a fit): views, not copies
  c->nnz = parent->nnz;
  c->split_len = parent->split_len;
  c->tiers = parent->tiers;
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    const Side& P = parent->s[side];
    S.n = P.n;
    S.ids = P.ids;
    S.starts = P.starts;
    S.maxrows = P.maxrows;
    S.nch = P.nch;
    S.world = P.world;
    S.chpad = P.chpad;
    S.own0 = P.own0;
    S.own_n = P.own_n;
    S.own_nnz = P.own_nnz;
    S.h_deg = P.h_deg;
    S.vmax = P.vmax;
    S.vmin = P.vmin;
    S.d_ptr.share(P.d_ptr);
    S.d_col.share(P.d_col);
    S.d_val.share(P.d_val);
    S.d_rows.share(P.d_rows);
    S.d_desc.share(P.d_desc);
    S.d_chunk_row.share(P.d_chunk_row);
    S.d_chunk_idx.share(P.d_chunk_idx);
    S.d_slot0.share(P.d_slot0);
    std::memcpy(S.boff, P.boff, sizeof S.boff);
    std::memcpy(S.bnnz, P.bnnz, sizeof S.bnnz);
    S.n_split = P.n_split;
    S.n_chunks = P.n_chunks;
    S.n_batch = P.n_batch;
    S.n_batch_nnz = P.n_batch_nnz;
    std::memcpy(S.bat_off, P.bat_off, sizeof S.bat_off);
    S.nsolve = P.nsolve;
    std::memcpy(S.cb, P.cb, sizeof S.cb);
    std::memcpy(S.c8, P.c8, sizeof S.c8);
    std::memcpy(S.split_n, P.split_n, sizeof S.split_n);
    std::memcpy(S.ck_off, P.ck_off, sizeof S.ck_off);
    std::memcpy(S.sl_off, P.sl_off, sizeof S.sl_off);
  }
  {
    std::lock_guard<std::mutex> lk(g_fork_mu);
    ++parent->forks;
  }
  c->parent = parent;
  c->has_ratings = true;
  if (int rc = set_device(c); rc != ALS_OK || (rc = factor_buffers(c)) != ALS_OK) {
    const std::string msg = g_err;
    als_destroy(c);
    return fail(rc, msg);
  }
  *out = c;
  return ALS_OK;
}

static void destroy_now(als_ctx* c);

void als_destroy(als_ctx* c) {
  if (!c) return;
  als_ctx* parent_to_free = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_fork_mu);
    if (c->forks > 0) {  // forks still view this context's ingest: freed with the last of them
      c->doomed = true;
      return;
    }
    if (c->parent && --c->parent->forks == 0 && c->parent->doomed) parent_to_free = c->parent;
  }
  destroy_now(c);
  if (parent_to_free) destroy_now(parent_to_free);
}

static void destroy_now(als_ctx* c) {
  (void)hipSetDevice(c->dev);
  if (c->st) (void)hipStreamSynchronize(c->st);
  if (c->st2) (void)hipStreamSynchronize(c->st2);  // no RCCL gather may be in flight at the destroy
  if (c->comm) (void)ncclCommDestroy(c->comm);
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->evc)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->evt)
    if (e) (void)hipEventDestroy(e);
  if (c->h_plan) (void)hipHostFree(c->h_plan);
  if (c->st2) (void)hipStreamDestroy(c->st2);
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

int als_comm_unique_id(void* out128) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  std::memcpy(out128, &id, sizeof id);
  return ALS_OK;
}

int als_comm_init(als_ctx* c, int32_t rank, int32_t world, const void* id128) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(ALS_E_INVALID_ARGUMENT, "bad comm args");
  if (world > 16) return fail(ALS_E_UNSUPPORTED, "at most 16 ranks (one node)");
  if (c->has_ratings) return fail(ALS_E_STATE, "als_comm_init must precede als_set_ratings");
  TRYC(set_device(c));
  c->rank = rank;
  c->world = world;
  if (world > 1) {
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof id);
    NCCLCHK(ncclCommInitRank(&c->comm, world, id, rank));
  }
  return ALS_OK;
}

int als_comm_init_host(als_ctx* c, int32_t rank, int32_t world, int (*allreduce)(void*, double*, int64_t),
                       int (*allgather)(void*, float*, int64_t), void* user) {
  if (!c || world < 1 || rank < 0 || rank >= world || !allreduce || !allgather)
    return fail(ALS_E_INVALID_ARGUMENT, "bad comm args");
  if (world > 16) return fail(ALS_E_UNSUPPORTED, "at most 16 ranks (one node)");
  if (c->has_ratings) return fail(ALS_E_STATE, "als_comm_init_host must precede als_set_ratings");
  c->rank = rank;
  c->world = world;
  c->h_allreduce = allreduce;
  c->h_allgather = allgather;
  c->h_user = user;
  return ALS_OK;
}

int als_set_ratings(als_ctx* c, int64_t n, const int32_t* user, const int32_t* item, const float* rating) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  if (n <= 0) return fail(ALS_E_INVALID_ARGUMENT, "No ratings available from the input dataset (empty ratings).");
  if (!user || !item || !rating) return fail(ALS_E_INVALID_ARGUMENT, "null ratings");
  TRYC(ingest_allowed(c));
  TRYC(set_device(c));
  DevBuf du, di, dr;
  HIPCHK(du.ensure(n * 4));
  HIPCHK(di.ensure(n * 4));
  HIPCHK(dr.ensure(n * 4));
  HIPCHK(copy_st(c, du.p, user, n * 4, hipMemcpyHostToDevice));
  HIPCHK(copy_st(c, di.p, item, n * 4, hipMemcpyHostToDevice));
  HIPCHK(copy_st(c, dr.p, rating, n * 4, hipMemcpyHostToDevice));
  return ingest_device(c, n, du.as<int32_t>(), di.as<int32_t>(), dr.as<float>());
}

int als_set_ratings_device(als_ctx* c, int64_t n, const int32_t* du, const int32_t* di, const float* dr) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  return ingest_device(c, n, du, di, dr);
}

int64_t als_num_rows(const als_ctx* c, int side) {
  if (!c || (side != 0 && side != 1)) return -1;
  return c->s[side].n;
}
int64_t als_num_ratings(const als_ctx* c) { return c ? c->nnz : -1; }
int als_rank(const als_ctx* c) { return c ? c->p.rank : -1; }

int als_get_ids(const als_ctx* c, int side, int32_t* out) {
  if (!c || (side != 0 && side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  std::memcpy(out, c->s[side].ids.data(), c->s[side].ids.size() * 4);
  return ALS_OK;
}

int als_set_initial_factors(als_ctx* c, int side, int64_t n, const int32_t* ids, const float* f) {
  if (!c || (side != 0 && side != 1) || !ids || !f) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings before injecting factors");
  TRYC(set_device(c));
  Side& S = c->s[side];
  const int k = c->p.rank;
  std::vector<float> dense((size_t)S.n * k, 0.f);
  std::vector<char> seen(S.n, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = find_row(S, ids[i]);
    if (r < 0) continue;  // ids absent from the ratings are ignored, like Spark's join
    std::memcpy(&dense[(size_t)r * k], f + (size_t)i * k, sizeof(float) * k);
    seen[r] = 1;
  }
  for (int64_t r = 0; r < S.n; ++r)
    if (!seen[r]) return fail(ALS_E_INVALID_ARGUMENT, "initial factors missing for id " + std::to_string(S.ids[r]));
  return upload_factors(c, side, dense.data(), k);
}

int als_init_factors(als_ctx* c) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings first");
  TRYC(set_device(c));
  c->s[0].has_factors = c->s[1].has_factors = false;  // explicit request: both sides
  return spark_init(c);
}

int als_init_factors_random(als_ctx* c, uint64_t seed) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings first");
  TRYC(set_device(c));
  TRYC(drain(c));
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    HIPCHK(launch_init_random(c->KP, c->p.rank, S.d_X.as<float>(), S.own_n, seed + 0x51ED270B27u * (side + 1),
                              S.own0, c->st));
    HIPCHK(launch_identity(S.d_B.as<double>(), c->KP, c->st));
    S.has_factors = true;
    S.orig_valid = false;
    S.fold_gram_valid = false;
    S.full_valid = false;
  }
  HIPCHK(hipStreamSynchronize(c->st));
  return ALS_OK;
}

int als_half_sweep(als_ctx* c, int dst_side) {
  if (!c || (dst_side != 0 && dst_side != 1)) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings first");
  TRYC(set_device(c));
  return half_sweep(c, dst_side);
}

int als_run_sweeps(als_ctx* c, int32_t n) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings first");
  TRYC(set_device(c));
  for (int it = 0; it < n; ++it) {
    TRYC(half_sweep(c, ALS_ITEM));
    TRYC(half_sweep(c, ALS_USER));
  }
  return ALS_OK;
}

int als_fit(als_ctx* c) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  if (!c->has_ratings)
    return fail(ALS_E_INVALID_ARGUMENT, "No ratings available from the input dataset (empty ratings).");
  TRYC(set_device(c));
  TRYC(spark_init(c));  // only the sides the caller did not inject
  return als_run_sweeps(c, c->p.max_iter);
}

int als_fit_tracked(als_ctx* c, double tol, int32_t cap, double* history_out, int32_t* n_history_out,
                    int32_t* sweeps_run_out) {
  if (!c || !n_history_out || !sweeps_run_out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!c->has_ratings)
    return fail(ALS_E_INVALID_ARGUMENT, "No ratings available from the input dataset (empty ratings).");
  TRYC(objective_ready(c, "als_fit_tracked"));
  TRYC(set_device(c));
  TRYC(spark_init(c));  // only the sides the caller did not inject
  std::vector<double> hist;
  als_objective_t o{};
  TRYC(objective(c, ALS_USER, nullptr, &o));
  hist.push_back(o.total);
  for (int s = 1; s <= c->p.max_iter; ++s) {
    TRYC(als_run_sweeps(c, 1));
    TRYC(objective(c, ALS_USER, nullptr, &o));
    hist.push_back(o.total);
    if (tol > 0.0 && hist[s - 1] - hist[s] < tol * std::fabs(hist[s - 1])) break;  // false for a NaN: the fit runs on
  }
  *sweeps_run_out = (int32_t)hist.size() - 1;
  *n_history_out = (int32_t)hist.size();
  if (history_out && (int64_t)hist.size() <= (int64_t)cap) std::copy(hist.begin(), hist.end(), history_out);
  return ALS_OK;
}

int als_get_basis(als_ctx* c, int side, double* out) {
  if (!c || (side != 0 && side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  const Side& S = c->s[side];
  if (!S.d_B.p) return fail(ALS_E_STATE, "no factors yet");
  TRYC(set_device(c));
  const int k = c->p.rank, KP = c->KP;
  std::vector<double> B((size_t)KP * KP);
  HIPCHK(hipMemcpyAsync(B.data(), S.d_B.p, B.size() * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) out[(size_t)i * k + j] = B[(size_t)i * KP + j];
  return ALS_OK;
}

int als_get_gram(als_ctx* c, int src_side, double* out) {
  if (!c || (src_side != 0 && src_side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  const Side& S = c->s[src_side];
  if (!S.has_gram) return fail(ALS_E_STATE, "no Gram computed yet");
  TRYC(set_device(c));
  // G was formed from the factors in the side's basis at that time (original = X·GBᵀ):
  // YᵀY = GB G GBᵀ, restricted to the model rank (GB is the identity on the padding)
  const int k = c->p.rank, KP = c->KP;
  std::vector<double> Gf((size_t)KP * KP), GB((size_t)KP * KP), G((size_t)k * k);
  HIPCHK(hipMemcpyAsync(Gf.data(), S.d_Gk.p, Gf.size() * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(GB.data(), S.d_GB.p, GB.size() * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) G[(size_t)i * k + j] = Gf[(size_t)i * KP + j];
  std::vector<double> T((size_t)k * k, 0.0);  // T = GB_k G
  for (int i = 0; i < k; ++i)
    for (int m = 0; m < k; ++m) {
      const double b = GB[(size_t)i * KP + m];
      if (b == 0.0) continue;
      for (int j = 0; j < k; ++j) T[(size_t)i * k + j] += b * G[(size_t)m * k + j];
    }
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      double acc = 0.0;
      for (int m = 0; m < k; ++m) acc += T[(size_t)i * k + m] * GB[(size_t)j * KP + m];
      out[(size_t)i * k + j] = acc;
    }
  return ALS_OK;
}

int als_get_factors(als_ctx* c, int side, int32_t* ids_out, float* f_out) {
  if (!c || (side != 0 && side != 1)) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  TRYC(set_device(c));
  TRYC(materialize(c, side));
  Side& S = c->s[side];
  if (ids_out) std::memcpy(ids_out, S.ids.data(), S.n * 4);
  if (f_out) {
    const int KP = c->KP, k = c->p.rank;
    std::vector<float> h((size_t)S.n * KP);
    HIPCHK(copy_st(c, h.data(), S.d_orig.p, h.size() * 4, hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < S.n; ++r) std::memcpy(f_out + (size_t)r * k, &h[(size_t)r * KP], sizeof(float) * k);
  }
  return ALS_OK;
}

int als_model_create(int32_t rank, int64_t nu, const int32_t* uids, const float* uf, int64_t ni,
                     const int32_t* iids, const float* ifac, int32_t device, als_ctx** out) {
  if (!out) return fail(ALS_E_INVALID_ARGUMENT, "null out");
  *out = nullptr;
  als_params p;
  als_params_default(&p);
  p.rank = rank;
  p.device = device;
  TRYC(validate(&p));
  if (nu < 0 || ni < 0 || (nu && (!uids || !uf)) || (ni && (!iids || !ifac)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad factor arrays");
  als_ctx* c = nullptr;
  TRYC(ctx_common(&p, &c));
  c->model_only = true;
  const int64_t ns[2] = {nu, ni};
  const int32_t* ids[2] = {uids, iids};
  const float* fs[2] = {uf, ifac};
  for (int side = 0; side < 2; ++side) {
    Side& S = c->s[side];
    std::vector<int64_t> ord(ns[side]);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return ids[side][a] < ids[side][b]; });
    S.n = ns[side];
    S.ids.resize(S.n);
    std::vector<float> h((size_t)std::max<int64_t>(S.n, 1) * c->KP, 0.f);
    for (int64_t r = 0; r < S.n; ++r) {
      S.ids[r] = ids[side][ord[r]];
      if (r > 0 && S.ids[r] == S.ids[r - 1]) {
        als_destroy(c);
        return fail(ALS_E_INVALID_ARGUMENT, "duplicate id in factors");
      }
      std::memcpy(&h[(size_t)r * c->KP], fs[side] + (size_t)ord[r] * rank, sizeof(float) * rank);
    }
    if (S.d_orig.ensure(h.size() * 4) != hipSuccess ||
        copy_st(c, S.d_orig.p, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      als_destroy(c);
      return fail(ALS_E_OUT_OF_MEMORY, "failed to upload factors");
    }
    S.orig_valid = true;
    S.fold_gram_valid = false;
    S.has_factors = true;
    S.starts = {0, S.n};
    S.maxrows = S.n;
    S.chpad = std::max<int64_t>(1, S.n);
  }
  *out = c;
  return ALS_OK;
}

int als_predict(als_ctx* c, int64_t n, const int32_t* user, const int32_t* item, float* out) {
  if (!c || (n > 0 && (!user || !item || !out))) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (n <= 0) return ALS_OK;
  TRYC(set_device(c));
  TRYC(materialize(c, ALS_USER));
  TRYC(materialize(c, ALS_ITEM));
  std::vector<int32_t> u(n), v(n);
  for (int64_t i = 0; i < n; ++i) {
    u[i] = (int32_t)find_row(c->s[ALS_USER], user[i]);
    v[i] = (int32_t)find_row(c->s[ALS_ITEM], item[i]);
  }
  DevBuf du, dv, dout;
  HIPCHK(du.ensure(n * 4));
  HIPCHK(dv.ensure(n * 4));
  HIPCHK(dout.ensure(n * 4));
  HIPCHK(copy_st(c, du.p, u.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(copy_st(c, dv.p, v.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(launch_predict(c->KP, c->p.rank, c->s[ALS_USER].d_orig.as<float>(), c->s[ALS_ITEM].d_orig.as<float>(),
                        du.as<int32_t>(), dv.as<int32_t>(), dout.as<float>(), n, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(copy_st(c, out, dout.p, n * 4, hipMemcpyDeviceToHost));
  return ALS_OK;
}

int als_get_row_ratings(als_ctx* c, int side, int32_t id, int64_t cap, int32_t* src_ids, float* ratings,
                        int64_t* n_out) {
  if (!c || (side != 0 && side != 1) || !n_out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings first");
  TRYC(set_device(c));
  Side& S = c->s[side];
  const Side& Src = c->s[1 - side];
  const int64_t r = find_row(S, id);
  if (r < 0) return fail(ALS_E_INVALID_ARGUMENT, "unknown id " + std::to_string(id));
  if (r < S.own0 || r >= S.own0 + S.own_n) return fail(ALS_E_STATE, "row not owned by this rank");
  int64_t pr[2];
  HIPCHK(copy_st(c, pr, S.d_ptr.as<int64_t>() + (r - S.own0), 16, hipMemcpyDeviceToHost));
  const int64_t n = pr[1] - pr[0];
  *n_out = n;
  if (n > cap) return ALS_OK;
  std::vector<int32_t> col(n);
  if (n) {
    HIPCHK(copy_st(c, col.data(), S.d_col.as<int32_t>() + pr[0], n * 4, hipMemcpyDeviceToHost));
    if (ratings) HIPCHK(copy_st(c, ratings, S.d_val.as<float>() + pr[0], n * 4, hipMemcpyDeviceToHost));
  }
  if (src_ids)
    for (int64_t e = 0; e < n; ++e) {
      const int64_t p = col[e];
      const int64_t span = (int64_t)Src.world * Src.chpad;  // invert the chunk-major gathered layout
      const int64_t q = p / span, rem = p % span, rk = rem / Src.chpad;
      src_ids[e] = Src.ids[Src.starts[rk] + q * Src.chpad + rem % Src.chpad];
    }
  return ALS_OK;
}

int als_get_degrees(const als_ctx* c, int side, int64_t* out) {
  if (!c || (side != 0 && side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!c->has_ratings) return fail(ALS_E_STATE, "set ratings first");
  const Side& S = c->s[side];
  for (int64_t r = 0; r < S.n; ++r) out[r] = -1;
  for (int64_t r = 0; r < S.own_n; ++r) out[S.own0 + r] = S.h_deg[r];
  return ALS_OK;
}

int als_last_timings(const als_ctx* c, int dst_side, double* out, int n) {
  if (!c || (dst_side != 0 && dst_side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < n && i < ALS_T_COUNT; ++i) out[i] = c->s[dst_side].t[i];
  return ALS_OK;
}

int als_path_stats(const als_ctx* c, int dst_side, int64_t* out4) {
  if (!c || (dst_side != 0 && dst_side != 1) || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->s[dst_side].stats[i];
  return ALS_OK;
}

int als_solver_stats(const als_ctx* c, int dst_side, int64_t* out4) {
  if (!c || (dst_side != 0 && dst_side != 1) || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->s[dst_side].solver[i];
  return ALS_OK;
}

int als_synchronize(als_ctx* c) {
  if (!c) return fail(ALS_E_INVALID_ARGUMENT, "null context");
  TRYC(set_device(c));
  return drain(c);  // both streams: the bench barrier covers the trailing factor gathers
}

int als_synth_generate(int32_t device, uint64_t seed, int32_t rounds, int64_t n_users, int64_t n_items,
                       const int64_t* deg_prefix, const double* cw, const int32_t* perm, int32_t* user_out,
                       int32_t* item_out, float* rating_out, int64_t* n_out) {
  if (!deg_prefix || !cw || !perm || !n_out || n_users <= 0 || n_items <= 0)
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(ALS_E_NO_DEVICE, "no HIP device");
  if (device >= 0) HIPCHK(hipSetDevice(device));
  const int64_t n = deg_prefix[n_users];
  DevBuf dp, dcw, dperm, du, di, dr;
  HIPCHK(dp.ensure((n_users + 1) * 8));
  HIPCHK(dcw.ensure(n_items * 8));
  HIPCHK(dperm.ensure(n_items * 4));
  HIPCHK(du.ensure(n * 4));
  HIPCHK(di.ensure(n * 4));
  HIPCHK(dr.ensure(n * 4));
  HIPCHK(hipMemcpy(dp.p, deg_prefix, (n_users + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dcw.p, cw, n_items * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dperm.p, perm, n_items * 4, hipMemcpyHostToDevice));
  hipStream_t st;
  HIPCHK(hipStreamCreate(&st));
  hipError_t e = synth_fill(seed, rounds, n_users, n_items, dp.as<int64_t>(), dcw.as<double>(), dperm.as<int32_t>(),
                            du.as<int32_t>(), di.as<int32_t>(), dr.as<float>(), n, n_out, st);
  (void)hipStreamDestroy(st);
  HIPCHK(e);
  if (user_out) HIPCHK(hipMemcpy(user_out, du.p, *n_out * 4, hipMemcpyDeviceToHost));
  if (item_out) HIPCHK(hipMemcpy(item_out, di.p, *n_out * 4, hipMemcpyDeviceToHost));
  if (rating_out) HIPCHK(hipMemcpy(rating_out, dr.p, *n_out * 4, hipMemcpyDeviceToHost));
  return ALS_OK;
}

int als_set_ratings_synthetic(als_ctx* c, uint64_t seed, int32_t rounds, int64_t n_users, int64_t n_items,
                              const int64_t* deg_prefix, const double* cw, const int32_t* perm) {
  if (!c || !deg_prefix || !cw || !perm || n_users <= 0 || n_items <= 0)
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  TRYC(ingest_allowed(c));
  TRYC(set_device(c));
  const int64_t n = deg_prefix[n_users];
  DevBuf dp, dcw, dperm, du, di, dr;
  HIPCHK(dp.ensure((n_users + 1) * 8));
  HIPCHK(dcw.ensure(n_items * 8));
  HIPCHK(dperm.ensure(n_items * 4));
  HIPCHK(du.ensure(n * 4));
  HIPCHK(di.ensure(n * 4));
  HIPCHK(dr.ensure(n * 4));
  HIPCHK(copy_st(c, dp.p, deg_prefix, (n_users + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(copy_st(c, dcw.p, cw, n_items * 8, hipMemcpyHostToDevice));
  HIPCHK(copy_st(c, dperm.p, perm, n_items * 4, hipMemcpyHostToDevice));
  int64_t nout = 0;
  HIPCHK(synth_fill(seed, rounds, n_users, n_items, dp.as<int64_t>(), dcw.as<double>(), dperm.as<int32_t>(),
                    du.as<int32_t>(), di.as<int32_t>(), dr.as<float>(), n, &nout, c->st));
  dp.release();
  dcw.release();
  dperm.release();
  return ingest_device(c, nout, du.as<int32_t>(), di.as<int32_t>(), dr.as<float>());
}

// ---- host-only utilities (no GPU needed; used by the CPU test suite) ------------------------
int als_host_eigh(int32_t n, const double* a, double* w, double* v) {
  if (n <= 0 || !a || !w || !v) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!sym_eig(n, a, w, v)) return fail(ALS_E_NOT_POSITIVE_DEFINITE, "eigensolver did not converge");
  return ALS_OK;
}

int als_device_eigh(int32_t device, int32_t k, const double* g, const double* w0, double* w, double* v,
                    int32_t* sweeps) {
  if (k <= 0 || k > 256 || !g || !w || !v) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (hipSetDevice(device) != hipSuccess) return fail(ALS_E_NO_DEVICE, "no such device");
  const int KP = padded_rank(k);
  std::vector<double> G((size_t)KP * KP, 0.0), B((size_t)KP * KP, 0.0), W((size_t)KP * KP, 0.0);
  for (int i = 0; i < KP; ++i) B[(size_t)i * KP + i] = W[(size_t)i * KP + i] = 1.0;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      G[(size_t)i * KP + j] = g[(size_t)i * k + j];
      if (w0) W[(size_t)i * KP + j] = w0[(size_t)i * k + j];
    }
  DevBuf dG, dB, dW, dOut, dS, dP, dl, du;
  HIPCHK(dG.ensure(G.size() * 8));
  HIPCHK(dB.ensure(B.size() * 8));
  HIPCHK(dW.ensure(W.size() * 8));
  HIPCHK(dOut.ensure(W.size() * 8));
  HIPCHK(dS.ensure(eig_scratch_doubles(KP) * 8));
  HIPCHK(dP.ensure((size_t)KP * KP * 4));
  HIPCHK(dl.ensure((size_t)KP * 4));
  HIPCHK(du.ensure((size_t)KP * 4));
  HIPCHK(hipMemcpy(dG.p, G.data(), G.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dB.p, B.data(), B.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dW.p, W.data(), W.size() * 8, hipMemcpyHostToDevice));
  // B_s = I, B_t = W0: the warm start is W0 itself; B_t_out = P
  HIPCHK(launch_device_eig(KP, k, dG.as<double>(), dB.as<double>(), dW.as<double>(), dOut.as<double>(), dS.as<double>(),
                           dP.as<float>(), dl.as<float>(), du.as<unsigned>(), nullptr));
  std::vector<double> wk(KP), P(W.size());
  int sw = 0;
  HIPCHK(hipMemcpy(P.data(), dOut.p, P.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(wk.data(), dS.as<double>() + (size_t)3 * KP * KP, KP * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sw, eig_sweeps(dS.as<double>(), KP), 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < k; ++i) {
    w[i] = wk[i];
    for (int j = 0; j < k; ++j) v[(size_t)i * k + j] = P[(size_t)i * KP + j];
  }
  if (sweeps) *sweeps = sw == EIG_NOT_FINITE ? 0 : (sw < 0 ? -sw - 1 : sw);
  if (sw == EIG_NOT_FINITE)
    return fail(ALS_E_NOT_POSITIVE_DEFINITE, "the matrix is not finite (NaN or Inf): eigensolver did not converge");
  if (sw < 0) return fail(ALS_E_NOT_POSITIVE_DEFINITE, "eigensolver did not converge");
  return ALS_OK;
}

int als_host_spark_side_seeds(int64_t seed, int64_t* user_seed, int64_t* item_seed) {
  if (!user_seed || !item_seed) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  spark_side_seeds(seed, user_seed, item_seed);
  return ALS_OK;
}

int als_host_spark_init(const int32_t* ids_sorted, int64_t n, int32_t rank, int64_t side_seed, int32_t num_blocks,
                        float* out) {
  if ((n > 0 && (!ids_sorted || !out)) || rank < 1 || num_blocks < 1) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  spark_initialize(ids_sorted, n, rank, side_seed, num_blocks, out, rank);
  return ALS_OK;
}

int als_host_plan_shards(const int64_t* ptr, int64_t n, int32_t world, int64_t* starts_out) {
  if (!ptr || n < 0 || world < 1 || !starts_out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  plan_shards(ptr, n, world, starts_out);
  return ALS_OK;
}

}  // extern "C"
