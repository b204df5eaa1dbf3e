// als_audit_rows: host side of the row audit (audit.hip).  The call brings both sides' current factors
// into the original basis, forms the fp64 src Gram, runs the audit kernels over the dst rows in batches
// and reads back the summary (and the per-row values when asked).  It uses nothing a half-sweep left
// behind except the factors and their bases; every buffer but the context's Gram (d_G, which the
// all-reduce works on and every half-sweep rewrites) is owned by the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"

using namespace albedo;

namespace {

// Ratings per chunk of a long row.  A row is one wave's work, so a launch runs as long as its longest
// row; the rule for skewed gathers is to cut lists longer than a quarter of one wave's share of the
// work (ratings / waves in flight) into chunks of that size.  The waves are counted at the hardware's 8
// per SIMD, more than the row kernel's registers allow: the smaller share errs towards more chunks,
// which cost one record each.  512, the size that rule was measured at, is the floor: below it a chunk
// record (2·KP + 2 doubles) stops being small beside the gather it stands for.  ALBEDO_AUDIT_CHUNK
// overrides it (tests: 256).
int64_t audit_chunk_len(const als_ctx* c, int64_t own_nnz) {
  const char* e = std::getenv("ALBEDO_AUDIT_CHUNK");
  if (e && *e && std::atoll(e) > 0) return std::atoll(e);
  const int64_t waves = (int64_t)c->n_cu * 4 * 8;
  return std::max<int64_t>(512, own_nnz / (4 * waves));
}

int audit(als_ctx* c, int t, double tol, double* eta_out, als_audit* out) {
  Side& S = c->s[1 - t];
  Side& T = c->s[t];
  const int KP = c->KP;
  hipStream_t st = c->st;
  if (c->world > 1) TRYC(drain(c));
  // both sides in the original basis: Y as the CSR's col indexes it, X by own row
  DevBuf own_s, padded_s, own_t;
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
  DevBuf slab, gx;
  const int64_t batch = std::max<int64_t>(64, std::min<int64_t>(T.own_n, ((int64_t)256 << 20) / (KP * 8)));
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
  // long rows and their chunks, rows ascending
  g.chunk = audit_chunk_len(c, T.own_nnz);
  std::vector<int32_t> crow, cidx, lrow;
  std::vector<int64_t> slot0{0};
  for (int64_t r = 0; r < T.own_n; ++r) {
    if (T.h_deg[r] <= g.chunk) continue;
    const int64_t nch = (T.h_deg[r] + g.chunk - 1) / g.chunk;
    for (int64_t k = 0; k < nch; ++k) {
      crow.push_back((int32_t)r);
      cidx.push_back((int32_t)k);
    }
    lrow.push_back((int32_t)r);
    slot0.push_back((int64_t)crow.size());
  }
  DevBuf d_crow, d_cidx, d_lrow, d_slot0, d_partial, d_eta, d_neg, d_sum;
  g.n_chunks = (int64_t)crow.size();
  if (g.n_chunks > 0) {
    HIPCHK(d_crow.ensure(crow.size() * 4));
    HIPCHK(d_cidx.ensure(cidx.size() * 4));
    HIPCHK(d_lrow.ensure(lrow.size() * 4));
    HIPCHK(d_slot0.ensure(slot0.size() * 8));
    HIPCHK(d_partial.ensure(crow.size() * (size_t)(2 * KP + 2) * 8));
    HIPCHK(copy_st(c, d_crow.p, crow.data(), crow.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, d_cidx.p, cidx.data(), cidx.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, d_lrow.p, lrow.data(), lrow.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, d_slot0.p, slot0.data(), slot0.size() * 8, hipMemcpyHostToDevice));
    g.chunk_row = d_crow.as<int32_t>();
    g.chunk_idx = d_cidx.as<int32_t>();
    g.long_row = d_lrow.as<int32_t>();
    g.long_slot0 = d_slot0.as<int64_t>();
    g.partial = d_partial.as<double>();
  }
  HIPCHK(d_eta.ensure((size_t)std::max<int64_t>(T.own_n, 1) * 8));
  HIPCHK(d_neg.ensure((size_t)std::max<int64_t>(T.own_n, 1) * 4));
  HIPCHK(d_sum.ensure((size_t)(AUDIT_SUM_BLOCKS + 1) * sizeof(AuditSummary)));
  g.eta = d_eta.as<double>();
  g.neg = d_neg.as<int32_t>();
  // From here to the synchronisation below the kernels read the call's buffers: a failed launch waits
  // for the queued ones before the buffers go
  auto run = [&]() -> int {
    HIPCHK(launch_audit_chunks(KP, g, st));
    int64_t l0 = 0;
    for (int64_t r0 = 0; r0 < T.own_n; r0 += batch) {
      g.row0 = r0;
      g.nb = std::min<int64_t>(batch, T.own_n - r0);
      int64_t l1 = l0;
      while (l1 < (int64_t)lrow.size() && lrow[l1] < r0 + g.nb) ++l1;
      HIPCHK(launch_audit_rows(KP, g, l0, l1 - l0, st));
      l0 = l1;
    }
    AuditSummary* part = d_sum.as<AuditSummary>();
    HIPCHK(launch_audit_summary(g.eta, g.neg, T.own_n, tol, part + 1, part, st));
    return ALS_OK;
  };
  AuditSummary sum{};
  int rc = run();
  if (rc == ALS_OK) {
    const hipError_t e = copy_st(c, &sum, d_sum.p, sizeof sum, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(ALS_E_HIP, std::string("HIP error: ") + hipGetErrorString(e) + " in the row audit");
  }
  if (rc != ALS_OK) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
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
