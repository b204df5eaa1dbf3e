// als_audit_rows: host side of the row audit (audit.hip).  The call brings both sides' current factors
// into the original basis, forms the fp64 src Gram, runs the audit kernels over the dst rows in batches
// and reads back the summary (and the per-row values when asked).  It uses nothing a half-sweep left
// behind except the factors and their bases; every buffer but the context's Gram (d_G, which the
// all-reduce works on and every half-sweep rewrites) is owned by the call, and a guard declared after
// them drains the stream on every return.  The chunk plan and the batches are row_plan.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"
#include "row_plan.h"

using namespace albedo;

namespace {

int audit(als_ctx* c, int t, double tol, double* eta_out, als_audit* out) {
  Side& S = c->s[1 - t];
  Side& T = c->s[t];
  const int KP = c->KP;
  hipStream_t st = c->st;
  if (c->world > 1) TRYC(drain(c));
  DevBuf own_s, padded_s, own_t, slab, gx, d_eta, d_neg, d_sum;
  RowPlan plan;
  Drain queued{st};
  // both sides in the original basis: Y as the CSR's col indexes it, X by own row
  const float *Y, *Yown, *X;
  if (c->world == 1) {
    TRYC(materialize(c, 1 - t));
    TRYC(materialize(c, t));
    Y = Yown = S.d_orig.as<float>();
    X = T.d_orig.as<float>();
  } else {
    TRYC(original_rows(c, 1 - t, &own_s, &padded_s));
    TRYC(original_rows(c, t, &own_t, nullptr));
    Y = padded_s.as<float>();
    Yown = own_s.as<float>();
    X = own_t.as<float>();
  }
  AuditArgs g{};
  g.Y = Y;
  g.X = X;
  g.ptr = T.d_ptr.as<int64_t>();
  g.col = T.d_col.as<int32_t>();
  g.val = T.d_val.as<float>();
  g.implicit = c->p.implicit_prefs;
  g.nonneg = c->p.nonnegative;
  g.alpha = c->p.alpha;
  g.reg = c->p.reg_param;
  const int64_t batch = row_batch_len(T.own_n, KP);
  if (c->p.implicit_prefs) {
    const int nblk = audit_gram_blocks(S.own_n);
    HIPCHK(slab.ensure((size_t)nblk * KP * KP * 8));
    HIPCHK(launch_audit_gram(KP, Yown, S.own_n, slab.as<double>(), nblk, c->d_G.as<double>(), st));
    TRYC(allreduce_G(c));
    std::vector<double> G((size_t)KP * KP);
    HIPCHK(copy_st(c, G.data(), c->d_G.p, G.size() * 8, hipMemcpyDeviceToHost));
    double ss = 0.0;
    for (double v : G) ss += v * v;
    g.gnorm = std::sqrt(ss);
    g.G = c->d_G.as<double>();
    HIPCHK(gx.ensure((size_t)batch * KP * 8));
    g.GX = gx.as<double>();
  }
  g.chunk = row_chunk_len(c, T.own_nnz, "ALBEDO_AUDIT_CHUNK");
  TRYC(plan.build(c, T, 2 * KP + 2, &g));
  HIPCHK(d_eta.ensure((size_t)std::max<int64_t>(T.own_n, 1) * 8));
  HIPCHK(d_neg.ensure((size_t)std::max<int64_t>(T.own_n, 1) * 4));
  HIPCHK(d_sum.ensure((size_t)(AUDIT_SUM_BLOCKS + 1) * sizeof(AuditSummary)));
  g.eta = d_eta.as<double>();
  g.neg = d_neg.as<int32_t>();
  HIPCHK(launch_audit_chunks(KP, g, st));
  TRYC(plan.batches(T.own_n, batch, [&](int64_t row0, int64_t nb, int64_t l0, int64_t n_long) -> int {
    g.row0 = row0;
    g.nb = nb;
    HIPCHK(launch_audit_rows(KP, g, l0, n_long, st));
    return ALS_OK;
  }));
  AuditSummary* part = d_sum.as<AuditSummary>();
  HIPCHK(launch_audit_summary(g.eta, g.neg, T.own_n, tol, part + 1, part, st));
  AuditSummary sum{};
  HIPCHK(copy_st(c, &sum, d_sum.p, sizeof sum, hipMemcpyDeviceToHost));
  if (eta_out) {
    std::fill(eta_out, eta_out + T.n, std::numeric_limits<double>::quiet_NaN());
    HIPCHK(copy_st(c, eta_out + T.own0, d_eta.p, (size_t)T.own_n * 8, hipMemcpyDeviceToHost));
  }
  out->rows = T.own_n;
  out->rows_over = sum.over;
  out->non_finite = sum.non_finite;
  out->negative = sum.negative;
  out->sum_eta = sum.sum;
  out->worst_eta = sum.worst_row < 0 ? 0.0 : sum.worst_eta;
  out->worst_id = sum.worst_row < 0 ? -1 : T.ids[T.own0 + sum.worst_row];
  out->worst_degree = sum.worst_row < 0 ? 0 : T.h_deg[sum.worst_row];
  out->worst_path = sum.worst_row < 0 ? -1 : row_path(c, T, sum.worst_row);
  return ALS_OK;
}

}  // namespace

extern "C" int als_audit_rows(als_ctx* c, int dst_side, double tol, double* eta_out, als_audit* out) {
  if (!c || (dst_side != 0 && dst_side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (std::isnan(tol)) return fail(ALS_E_INVALID_ARGUMENT, "als_audit_rows: tol is NaN");
  if (!c->has_ratings || c->model_only) return fail(ALS_E_STATE, "als_audit_rows needs a context holding ratings");
  if (!c->s[0].has_factors || !c->s[1].has_factors)
    return fail(ALS_E_STATE, "als_audit_rows needs the factors of both sides (fit or inject them first)");
  TRYC(set_device(c));
  return audit(c, dst_side, tol, eta_out, out);
}
