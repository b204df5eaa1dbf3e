// als_explain: host side of the explanation (explain.hip).  The call does what the fold-in does up to the
// factorisation, through the fold-in's own host code (FoldFront, fold_host.h): the src side's factors in the
// original basis, the fp64 src Gram from the side's fold-in cache (or formed there), the triples as a CSR on
// the device.  It maps the pairs onto that CSR and runs one workgroup per row that a valid pair names.  It
// reads the model and writes nothing of it; the fold-in's timing and stats are not touched either.  Every
// buffer but the cached Gram (Side::d_foldG) is owned by the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "fold_host.h"
#include "kernels.h"

using namespace albedo;

namespace {

// what a pair that cannot be explained gets, and the whole answer when there are no triples
void fill_unexplained(int64_t n_pairs, int32_t m, double* total, int32_t* ids, double* contrib) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::fill(total, total + n_pairs, nan);
  std::fill(ids, ids + n_pairs * m, -1);
  std::fill(contrib, contrib + n_pairs * m, nan);
}

int explain(als_ctx* c, int side, double reg, double alpha, int implicit, int64_t n, const int32_t* row_id,
            const int32_t* src_id, const float* rating, int64_t n_pairs, const int32_t* pair_row_id,
            const int32_t* pair_target_id, int32_t m, double* total_out, int32_t* src_ids_out, double* contrib_out) {
  hipStream_t st = c->st;
  TRYC(materialize(c, 1 - side));
  FoldFront F;
  DevBuf p_row, p_tgt, p_key, p_keys, p_target, p_hi, p_slot, p_runs, p_cnt, p_ptr, p_nr, p_deg, p_degs, p_iota, p_order;
  DevBuf d_total, d_oids, d_contrib;
  Marks<4> clk;
  Drain queued{st};
  for (DevBuf* b : {&p_row, &p_tgt, &p_target, &p_hi, &p_slot, &p_runs, &p_deg, &p_degs, &p_iota, &p_order})
    HIPCHK(b->ensure((size_t)n_pairs * 4));
  HIPCHK(p_cnt.ensure((size_t)(n_pairs + 1) * 4));
  HIPCHK(p_key.ensure((size_t)n_pairs * 8));
  HIPCHK(p_keys.ensure((size_t)n_pairs * 8));
  HIPCHK(p_ptr.ensure((size_t)(n_pairs + 1) * 8));
  HIPCHK(p_nr.ensure(8));
  HIPCHK(d_total.ensure((size_t)n_pairs * 8));
  HIPCHK(d_oids.ensure((size_t)n_pairs * m * 4));
  HIPCHK(d_contrib.ensure((size_t)n_pairs * m * 8));
  TRYC(F.upload(c, side, n, row_id, src_id, rating, explain_sort_temp_bytes(n_pairs)));  // one temp buffer for both maps
  HIPCHK(hipMemcpyAsync(p_row.p, pair_row_id, (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(p_tgt.p, pair_target_id, (size_t)n_pairs * 4, hipMemcpyHostToDevice, st));
  HIPCHK(clk.mark(0, st));
  TRYC(F.build_csr(c));
  ExplainPairs x{};
  x.key = p_key.as<uint64_t>();
  x.key_sorted = p_keys.as<uint64_t>();
  x.target = p_target.as<uint32_t>();
  x.hi = p_hi.as<uint32_t>();
  x.slot = p_slot.as<uint32_t>();
  x.runs = p_runs.as<uint32_t>();
  x.counts = p_cnt.as<int32_t>();
  x.ptr = p_ptr.as<int64_t>();
  x.n_runs = p_nr.as<int64_t>();
  x.deg = p_deg.as<uint32_t>();
  x.deg_sorted = p_degs.as<uint32_t>();
  x.iota = p_iota.as<int32_t>();
  x.order = p_order.as<int32_t>();
  int64_t nu = 0;
  HIPCHK(explain_map_pairs(p_row.as<int32_t>(), p_tgt.as<int32_t>(), n_pairs, F.f.ids, F.f.deg, F.n_rows,
                           F.d_sids.as<int32_t>(), c->s[1 - side].n, F.d_tmp.p, F.temp_bytes, x, &nu, st));
  HIPCHK(launch_explain_fill(n_pairs, m, d_total.as<double>(), d_oids.as<int32_t>(), d_contrib.as<double>(), st));
  HIPCHK(clk.mark(1, st));
  TRYC(F.gram(c, implicit));
  HIPCHK(clk.mark(2, st));
  ExplainArgs a{};
  int n_wg = 0;
  TRYC(F.plan(c, nu, reg, alpha, implicit, &a.f, &n_wg));
  a.runs = x.runs;
  a.pptr = x.ptr;
  a.order = x.order;
  a.n_runs = nu;
  a.slot = x.slot;
  a.target = x.target;
  a.src_ids = F.d_sids.as<int32_t>();
  a.m = m;
  a.total = d_total.as<double>();
  a.ids = d_oids.as<int32_t>();
  a.contrib = d_contrib.as<double>();
  HIPCHK(launch_explain(c->KP, a, n_wg, st));
  HIPCHK(clk.mark(3, st));
  int bad = INT_MAX;
  HIPCHK(hipMemcpyAsync(&bad, F.d_bad.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->explain_ms[0] = event_ms(clk.e[0], clk.e[1]);
  c->explain_ms[1] = F.form_gram ? event_ms(clk.e[1], clk.e[2]) : 0.0;
  c->explain_ms[2] = event_ms(clk.e[2], clk.e[3]);
  c->explain_ms[3] = event_ms(clk.e[0], clk.e[3]);
  TRYC(F.finish(c, bad, "explanation"));
  HIPCHK(copy_st(c, total_out, d_total.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
  HIPCHK(copy_st(c, src_ids_out, d_oids.p, (size_t)n_pairs * m * 4, hipMemcpyDeviceToHost));
  HIPCHK(copy_st(c, contrib_out, d_contrib.p, (size_t)n_pairs * m * 8, hipMemcpyDeviceToHost));
  return ALS_OK;
}

}  // namespace

extern "C" int als_explain(als_ctx* c, int side, const als_fold_params* fp, int64_t n, const int32_t* row_id,
                           const int32_t* src_id, const float* rating, int64_t n_pairs, const int32_t* pair_row_id,
                           const int32_t* pair_target_id, int32_t m, double* total_out, int32_t* src_ids_out,
                           double* contrib_out) {
  if (!c || (side != 0 && side != 1) || n < 0 || n_pairs < 0 || m < 1 || (n > 0 && (!row_id || !src_id || !rating)) ||
      (n_pairs > 0 && (!pair_row_id || !pair_target_id || !total_out || !src_ids_out || !contrib_out)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (fp && (std::isnan(fp->reg_param) || fp->reg_param < 0.0 || std::isnan(fp->alpha) || fp->alpha < 0.0))
    return fail(ALS_E_INVALID_ARGUMENT, "als_explain: regParam and alpha should be >= 0");
  if (!fp && c->model_only)
    return fail(ALS_E_INVALID_ARGUMENT,
                "als_explain: a model-only context has no regParam, alpha or implicitPrefs: pass als_fold_params");
  if ((fp && fp->nonnegative != 0) || (!fp && c->p.nonnegative))
    return fail(ALS_E_UNSUPPORTED,
                "als_explain: an NNLS row is not linear in its ratings, so this decomposition is not its score");
  if (m > EXPLAIN_MAX_M) return fail(ALS_E_UNSUPPORTED, "als_explain lists at most 64 ratings a pair");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "als_explain is single-process (world = 1)");
  if (n > (int64_t)0x7FFFFFFF || n_pairs > (int64_t)0x7FFFFFFF)
    return fail(ALS_E_UNSUPPORTED, "als_explain takes at most 2^31 - 1 triples and 2^31 - 1 pairs a call");
  for (double& v : c->explain_ms) v = 0.0;
  if (n_pairs == 0) return ALS_OK;
  if (!c->s[1 - side].has_factors)
    return fail(ALS_E_STATE, std::string("als_explain needs the ") + (side == ALS_USER ? "item" : "user") +
                                 " factors (fit, inject or load them first)");
  if (n == 0) {  // no row has a triple: no pair can be explained
    fill_unexplained(n_pairs, m, total_out, src_ids_out, contrib_out);
    return ALS_OK;
  }
  TRYC(set_device(c));
  const double reg = fp ? fp->reg_param : c->p.reg_param, alpha = fp ? fp->alpha : c->p.alpha;
  const int implicit = fp ? fp->implicit_prefs != 0 : c->p.implicit_prefs != 0;
  return explain(c, side, reg, alpha, implicit, n, row_id, src_id, rating, n_pairs, pair_row_id, pair_target_id, m,
                 total_out, src_ids_out, contrib_out);
}

extern "C" int als_explain_timing(const als_ctx* c, double* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->explain_ms[i];
  return ALS_OK;
}
