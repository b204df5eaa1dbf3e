// als_fold_in: host side of the fold-in (foldin.hip).  The call brings the src side's factors into the
// original basis, takes the fp64 src Gram from the side's fold-in cache (or forms it there), turns the
// triples into a CSR on the device and solves every distinct row, by Cholesky or (als_fold_params.nonnegative)
// by Spark's NNLS.solve.  It reads the model and writes nothing
// of it: no factor, basis, Gram, timing or path counter of a half-sweep changes.  Every buffer but the
// cached Gram (Side::d_foldG) is owned by the call.  Everything up to the solve's launch is FoldFront
// (fold_host.h), which als_explain runs too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "fold_host.h"
#include "kernels.h"

using namespace albedo;

namespace albedo {

int FoldFront::upload(als_ctx* c, int side_, int64_t n_, const int32_t* row_id, const int32_t* src_id,
                      const float* rating, size_t min_temp) {
  side = side_;
  n = n_;
  const Side& S = c->s[1 - side];
  hipStream_t st = c->st;
  for (DevBuf* b : {&d_row, &d_src, &d_val, &d_vals, &d_hi, &d_col, &d_runs, &d_ids, &d_deg, &d_degs, &d_iota, &d_order})
    HIPCHK(b->ensure((size_t)n * 4));
  HIPCHK(d_cnt.ensure((size_t)(n + 1) * 4));
  HIPCHK(d_key.ensure((size_t)n * 8));
  HIPCHK(d_keys.ensure((size_t)n * 8));
  HIPCHK(d_ptr.ensure((size_t)(n + 1) * 8));
  HIPCHK(d_nr.ensure(8));
  HIPCHK(d_bad.ensure(4));
  HIPCHK(d_sids.ensure((size_t)std::max<int64_t>(S.n, 1) * 4));
  temp_bytes = std::max(fold_sort_temp_bytes(n), min_temp);
  HIPCHK(d_tmp.ensure(std::max<size_t>(temp_bytes, 16)));
  HIPCHK(hipMemcpyAsync(d_row.p, row_id, (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_src.p, src_id, (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_val.p, rating, (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_sids.p, S.ids.data(), (size_t)S.n * 4, hipMemcpyHostToDevice, st));
  bad0 = INT_MAX;
  HIPCHK(hipMemcpyAsync(d_bad.p, &bad0, 4, hipMemcpyHostToDevice, st));
  return ALS_OK;
}

int FoldFront::build_csr(als_ctx* c) {
  f.key = d_key.as<uint64_t>();
  f.key_sorted = d_keys.as<uint64_t>();
  f.val_sorted = d_vals.as<float>();
  f.hi = d_hi.as<uint32_t>();
  f.col = d_col.as<uint32_t>();
  f.runs = d_runs.as<uint32_t>();
  f.counts = d_cnt.as<int32_t>();
  f.ptr = d_ptr.as<int64_t>();
  f.n_rows = d_nr.as<int64_t>();
  f.ids = d_ids.as<int32_t>();
  f.deg = d_deg.as<uint32_t>();
  f.deg_sorted = d_degs.as<uint32_t>();
  f.iota = d_iota.as<int32_t>();
  f.order = d_order.as<int32_t>();
  HIPCHK(fold_build_csr(d_row.as<int32_t>(), d_src.as<int32_t>(), d_val.as<float>(), n, d_sids.as<int32_t>(),
                        c->s[1 - side].n, d_tmp.p, temp_bytes, f, &n_rows, c->st));
  return ALS_OK;
}

int FoldFront::gram(als_ctx* c, int implicit) {
  Side& S = c->s[1 - side];
  const int KP = c->KP;
  form_gram = implicit && !S.fold_gram_valid;
  if (form_gram) {  // into the side's own buffer: c->d_G belongs to the half-sweeps
    const int nblk = audit_gram_blocks(S.n);
    HIPCHK(d_slab.ensure((size_t)nblk * KP * KP * 8));
    HIPCHK(S.d_foldG.ensure((size_t)KP * KP * 8));
    HIPCHK(launch_audit_gram(KP, S.d_orig.as<float>(), S.n, d_slab.as<double>(), nblk, S.d_foldG.as<double>(), c->st));
  }
  return ALS_OK;
}

int FoldFront::plan(als_ctx* c, int64_t n_work, double reg, double alpha, int implicit, FoldArgs* a, int* n_wg) {
  Side& S = c->s[1 - side];
  *n_wg = fold_workgroups(c->KP, n_work, c->n_cu);
  const size_t sd = fold_scratch_doubles(c->KP, *n_wg);
  if (sd) HIPCHK(d_scratch.ensure(sd * 8));
  a->Y = S.d_orig.as<float>();
  a->G = implicit ? S.d_foldG.as<double>() : nullptr;
  a->ptr = f.ptr;
  a->deg = f.deg;
  a->col = f.col;
  a->val = f.val_sorted;
  a->k = c->p.rank;
  a->implicit = implicit;
  a->alpha = alpha;
  a->reg = reg;
  a->scratch = sd ? d_scratch.as<double>() : nullptr;
  a->bad = d_bad.as<int>();
  return ALS_OK;
}

int FoldFront::finish(als_ctx* c, int bad, const char* what) {
  if (form_gram) c->s[1 - side].fold_gram_valid = true;
  if (bad == INT_MAX) return ALS_OK;
  int32_t id = 0;
  HIPCHK(copy_st(c, &id, f.ids + bad, 4, hipMemcpyDeviceToHost));
  return fail(ALS_E_NOT_POSITIVE_DEFINITE,
              "LAPACK.dppsv-equivalent Cholesky met a non-positive pivot because A is not positive definite. Is A "
              "derived from a singular matrix (e.g. collinear column values)? (" +
                  std::string(what) + " of " + (side == ALS_USER ? "user" : "item") + " " + std::to_string(id) +
                  ", the lowest failing id)");
}

}  // namespace albedo

namespace {

int fold_in(als_ctx* c, int side, double reg, double alpha, int implicit, int nonneg, int64_t n, const int32_t* row_id,
            const int32_t* src_id, const float* rating, int64_t cap, int64_t* n_rows_out, int32_t* ids_out,
            int64_t* degree_out, float* factors_out) {
  const int k = c->p.rank;
  hipStream_t st = c->st;
  TRYC(materialize(c, 1 - side));
  FoldFront F;
  DevBuf d_stats, d_X;
  Marks<4> clk;
  Drain queued{st};
  HIPCHK(d_stats.ensure(4 * 8));
  TRYC(F.upload(c, side, n, row_id, src_id, rating, 0));
  HIPCHK(hipMemsetAsync(d_stats.p, 0, 4 * 8, st));
  HIPCHK(clk.mark(0, st));
  TRYC(F.build_csr(c));
  const int64_t nr = F.n_rows;
  HIPCHK(clk.mark(1, st));
  TRYC(F.gram(c, implicit));
  HIPCHK(clk.mark(2, st));
  FoldArgs a{};
  int n_wg = 0;
  TRYC(F.plan(c, nr, reg, alpha, implicit, &a, &n_wg));
  HIPCHK(d_X.ensure((size_t)nr * k * 4));
  a.order = F.f.order;
  a.n_rows = nr;
  a.X = d_X.as<float>();
  a.nonnegative = nonneg;
  a.stats = d_stats.as<unsigned long long>();
  HIPCHK(launch_fold_solve(c->KP, a, n_wg, st));
  HIPCHK(clk.mark(3, st));
  int bad = INT_MAX;
  unsigned long long stats[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(&bad, F.d_bad.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(stats, d_stats.p, sizeof stats, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < 4; ++i) c->fold_stats[i] = (int64_t)stats[i];
  c->fold_ms[0] = event_ms(clk.e[0], clk.e[1]);
  c->fold_ms[1] = F.form_gram ? event_ms(clk.e[1], clk.e[2]) : 0.0;
  c->fold_ms[2] = event_ms(clk.e[2], clk.e[3]);
  c->fold_ms[3] = event_ms(clk.e[0], clk.e[3]);
  *n_rows_out = nr;
  TRYC(F.finish(c, bad, "fold-in"));
  if (nr > cap) return ALS_OK;
  if (ids_out) HIPCHK(copy_st(c, ids_out, F.d_ids.p, (size_t)nr * 4, hipMemcpyDeviceToHost));
  if (degree_out) {
    std::vector<uint32_t> deg(nr);
    HIPCHK(copy_st(c, deg.data(), F.d_deg.p, (size_t)nr * 4, hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < nr; ++r) degree_out[r] = deg[r];
  }
  if (factors_out) HIPCHK(copy_st(c, factors_out, d_X.p, (size_t)nr * k * 4, hipMemcpyDeviceToHost));
  return ALS_OK;
}

}  // namespace

extern "C" int als_fold_in(als_ctx* c, int side, const als_fold_params* fp, int64_t n, const int32_t* row_id,
                           const int32_t* src_id, const float* rating, int64_t cap, int64_t* n_rows_out,
                           int32_t* ids_out, int64_t* degree_out, float* factors_out) {
  if (!c || (side != 0 && side != 1) || n < 0 || !n_rows_out || (n > 0 && (!row_id || !src_id || !rating)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (fp && (std::isnan(fp->reg_param) || fp->reg_param < 0.0 || std::isnan(fp->alpha) || fp->alpha < 0.0))
    return fail(ALS_E_INVALID_ARGUMENT, "als_fold_in: regParam and alpha should be >= 0");
  if (!fp && c->model_only)
    return fail(ALS_E_INVALID_ARGUMENT,
                "als_fold_in: a model-only context has no regParam, alpha or implicitPrefs: pass als_fold_params");
  if (!fp && c->p.nonnegative)
    return fail(ALS_E_UNSUPPORTED,
                "als_fold_in without als_fold_params does not solve by NNLS: pass als_fold_params with nonnegative = 1");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "als_fold_in is single-process (world = 1)");
  if (n > (int64_t)0x7FFFFFFF) return fail(ALS_E_UNSUPPORTED, "als_fold_in takes at most 2^31 - 1 triples a call");
  *n_rows_out = 0;
  for (double& v : c->fold_ms) v = 0.0;
  for (int64_t& v : c->fold_stats) v = 0;
  if (n == 0) return ALS_OK;
  if (!c->s[1 - side].has_factors)
    return fail(ALS_E_STATE, std::string("als_fold_in needs the ") + (side == ALS_USER ? "item" : "user") +
                                 " factors (fit, inject or load them first)");
  TRYC(set_device(c));
  const double reg = fp ? fp->reg_param : c->p.reg_param, alpha = fp ? fp->alpha : c->p.alpha;
  const int implicit = fp ? fp->implicit_prefs != 0 : c->p.implicit_prefs != 0;
  const int nonneg = fp ? fp->nonnegative != 0 : 0;  // fp == NULL on a nonnegative context was refused above
  return fold_in(c, side, reg, alpha, implicit, nonneg, n, row_id, src_id, rating, cap, n_rows_out, ids_out, degree_out,
                 factors_out);
}

extern "C" int als_fold_in_stats(const als_ctx* c, int64_t* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->fold_stats[i];
  return ALS_OK;
}

extern "C" int als_fold_in_timing(const als_ctx* c, double* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->fold_ms[i];
  return ALS_OK;
}
