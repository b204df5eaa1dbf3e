// als_recommend_vectors: host side of the query top-k (query_topk.hip).  The call checks its arguments,
// brings the dst side's factors into the original basis, maps and sorts the exclusion lists on the device,
// scans the dst rows slice by slice and merges the slice partials.  It reads the model and writes nothing of
// it: no factor, basis, Gram, counter or timing of als_recommend or of a half-sweep changes.  Every buffer
// is owned by the call.  The exclusion-list front and the scan tier (engine.h) serve als_similar and
// als_similar_vectors too (similar_host.cpp), which write their own timing from their own marks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"

using namespace albedo;

namespace albedo {

int exclusion_ranges(const char* who, int too_many, int64_t n_q, const int64_t* excl_ptr, const int32_t** excl_ids,
                     std::vector<int64_t>* ptr0) {
  const std::string w(who);
  ptr0->clear();
  if (!excl_ptr || n_q <= 0) return ALS_OK;
  if (excl_ptr[0] < 0) return fail(ALS_E_INVALID_ARGUMENT, w + ": excl_ptr is negative");
  for (int64_t i = 0; i < n_q; ++i)
    if (excl_ptr[i + 1] < excl_ptr[i])
      return fail(ALS_E_INVALID_ARGUMENT, w + ": excl_ptr does not ascend at query " + std::to_string(i));
  const int64_t n_e = excl_ptr[n_q] - excl_ptr[0];
  if (n_e > (int64_t)0x7FFFFFFF) return fail(too_many, w + " takes at most 2^31 - 1 exclusions a call");
  if (n_e > 0 && !*excl_ids)
    return fail(ALS_E_INVALID_ARGUMENT, w + ": excl_ids is null and excl_ptr names a non-empty range");
  if (n_e > 0) {
    ptr0->resize((size_t)n_q + 1);
    for (int64_t i = 0; i <= n_q; ++i) (*ptr0)[(size_t)i] = excl_ptr[i] - excl_ptr[0];
    *excl_ids += excl_ptr[0];
  }
  return ALS_OK;
}

int Exclusions::upload(als_ctx* c, int64_t n_q, const std::vector<int64_t>& ptr0, const int32_t* excl_ids) {
  n_e = ptr0.empty() ? 0 : ptr0.back();
  if (n_e <= 0) return ALS_OK;
  temp_bytes = query_sort_temp_bytes(n_e);
  HIPCHK(d_ptr.ensure((size_t)(n_q + 1) * 8));
  HIPCHK(d_eid.ensure((size_t)n_e * 4));
  HIPCHK(d_key.ensure((size_t)n_e * 8));
  HIPCHK(d_keys.ensure((size_t)n_e * 8));
  HIPCHK(d_tmp.ensure(std::max<size_t>(temp_bytes, 16)));
  HIPCHK(hipMemcpyAsync(d_ptr.p, ptr0.data(), (size_t)(n_q + 1) * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(d_eid.p, excl_ids, (size_t)n_e * 4, hipMemcpyHostToDevice, c->st));
  return ALS_OK;
}

int Exclusions::map(als_ctx* c, int64_t n_q, const int32_t* d_ids, int64_t n_dst) {
  if (n_e > 0)
    HIPCHK(query_map_exclusions(d_ptr.as<int64_t>(), n_q, d_eid.as<int32_t>(), n_e, d_ids, n_dst, d_key.as<uint64_t>(),
                                d_keys.as<uint64_t>(), d_tmp.p, temp_bytes, c->st));
  return ALS_OK;
}

int ScanBuffers::ensure(const als_ctx* c, int64_t n_dst, int64_t n_q, int k) {
  const size_t part = (size_t)query_plan(n_dst, n_q, c->n_cu).n_slices * n_q * k;
  HIPCHK(d_ps.ensure(part * 4));
  HIPCHK(d_pr.ensure(part * 4));
  HIPCHK(d_oi.ensure((size_t)n_q * k * 4));
  HIPCHK(d_os.ensure((size_t)n_q * k * 4));
  return ALS_OK;
}

int scan_lists(als_ctx* c, const ScanBuffers& b, int k, const float* d_Y, int64_t n_dst, const float* d_q, int64_t n_q,
               const int64_t* d_ptr, const uint64_t* d_keys, const int32_t* d_ids, hipEvent_t* scan_done,
               hipEvent_t* merge_done, int32_t* ids_out, float* scores_out) {
  hipStream_t st = c->st;
  const QueryPlan plan = query_plan(n_dst, n_q, c->n_cu);
  HIPCHK(launch_query_scan(c->KP, c->p.rank, d_Y, n_dst, d_q, n_q, k, d_ptr, d_keys, plan, b.d_ps.as<float>(),
                           b.d_pr.as<uint32_t>(), c->n_cu, st));
  HIPCHK(mark_event(scan_done, st));
  HIPCHK(launch_query_merge(b.d_ps.as<float>(), b.d_pr.as<uint32_t>(), plan.n_slices, n_q, k, d_ids,
                            b.d_oi.as<int32_t>(), b.d_os.as<float>(), st));
  HIPCHK(mark_event(merge_done, st));
  HIPCHK(hipMemcpyAsync(ids_out, b.d_oi.p, (size_t)n_q * k * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(scores_out, b.d_os.p, (size_t)n_q * k * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return ALS_OK;
}

}  // namespace albedo

namespace {

// ptr0: the exclusion ranges shifted to start at 0 ([n_q + 1]), empty when the call has none
int recommend_vectors(als_ctx* c, int side, int k, int64_t n_q, const float* q, const std::vector<int64_t>& ptr0,
                      const int32_t* excl_ids, int32_t* ids_out, float* scores_out) {
  Side& S = c->s[side];
  const int rank = c->p.rank;
  hipStream_t st = c->st;
  TRYC(materialize(c, side));
  DevBuf d_q, d_ids;
  Exclusions X;
  ScanBuffers B;
  Marks<4> clk;
  Drain queued{st};
  HIPCHK(d_q.ensure((size_t)n_q * rank * 4));
  HIPCHK(d_ids.ensure((size_t)std::max<int64_t>(S.n, 1) * 4));
  TRYC(B.ensure(c, S.n, n_q, k));  // ahead of mark 0: no allocation inside a timed stage
  HIPCHK(hipMemcpyAsync(d_q.p, q, (size_t)n_q * rank * 4, hipMemcpyHostToDevice, st));
  if (S.n > 0) HIPCHK(hipMemcpyAsync(d_ids.p, S.ids.data(), (size_t)S.n * 4, hipMemcpyHostToDevice, st));
  TRYC(X.upload(c, n_q, ptr0, excl_ids));
  HIPCHK(clk.mark(0, st));
  TRYC(X.map(c, n_q, d_ids.as<int32_t>(), S.n));
  HIPCHK(clk.mark(1, st));
  TRYC(scan_lists(c, B, k, S.d_orig.as<float>(), S.n, d_q.as<float>(), n_q, X.ptr(), X.keys(), d_ids.as<int32_t>(),
                  &clk.e[2], &clk.e[3], ids_out, scores_out));
  c->query_ms[0] = X.n_e > 0 ? event_ms(clk.e[0], clk.e[1]) : 0.0;
  c->query_ms[1] = event_ms(clk.e[1], clk.e[2]);
  c->query_ms[2] = event_ms(clk.e[2], clk.e[3]);
  c->query_ms[3] = event_ms(clk.e[0], clk.e[3]);
  return ALS_OK;
}

}  // namespace

extern "C" int als_recommend_vectors(als_ctx* c, int side, int32_t k, int64_t n_q, const float* q, const int64_t* excl_ptr,
                                     const int32_t* excl_ids, int32_t* ids_out, float* scores_out) {
  if (!c || (side != 0 && side != 1) || k < 1 || n_q < 0 || (n_q > 0 && (!q || !ids_out || !scores_out)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (k > 64) return fail(ALS_E_UNSUPPORTED, "als_recommend_vectors keeps at most 64 rows per query (k <= 64)");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "als_recommend_vectors is single-process (world = 1)");
  if (n_q > (int64_t)0x7FFFFFFF)
    return fail(ALS_E_UNSUPPORTED, "als_recommend_vectors takes at most 2^31 - 1 queries a call");
  std::vector<int64_t> ptr0;
  TRYC(exclusion_ranges("als_recommend_vectors", ALS_E_INVALID_ARGUMENT, n_q, excl_ptr, &excl_ids, &ptr0));
  for (double& v : c->query_ms) v = 0.0;
  if (n_q == 0) return ALS_OK;
  if (!c->s[side].has_factors)
    return fail(ALS_E_STATE, std::string("als_recommend_vectors needs the ") + (side == ALS_USER ? "user" : "item") +
                                 " factors (fit, inject or load them first)");
  TRYC(set_device(c));
  return recommend_vectors(c, side, k, n_q, q, ptr0, excl_ids, ids_out, scores_out);
}

extern "C" int als_recommend_vectors_timing(const als_ctx* c, double* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->query_ms[i];
  return ALS_OK;
}
