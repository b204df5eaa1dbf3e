// als_objective: host side of the training loss (objective.hip).  The call brings both sides' current
// factors into the original basis, forms the fp64 src Gram (implicit prefs), runs the row kernels over
// the dst rows in batches, adds the other side's regulariser from that side's own ratings and reads back
// the sums (and the per-row losses when asked).  It reads the model and writes nothing of it; every
// buffer, the Gram included, is owned by the call.  The chunk plan and the batches are row_plan.h's,
// shared with the row audit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"
#include "row_plan.h"

using namespace albedo;

namespace albedo {

int objective(als_ctx* c, int t, double* row_loss_out, als_objective_t* out) {
  Side& S = c->s[1 - t];
  Side& T = c->s[t];
  const int KP = c->KP;
  hipStream_t st = c->st;
  // both sides in the original basis: Y as the CSR's col indexes it (world = 1: the dense row), X by row
  TRYC(materialize(c, 1 - t));
  TRYC(materialize(c, t));
  DevBuf slab, d_G, gx, d_rec, d_other, d_part, d_sum;
  RowPlan plan;
  Marks<3> clk;
  Drain queued{st};
  ObjectiveArgs g{};
  g.Y = S.d_orig.as<float>();
  g.X = T.d_orig.as<float>();
  g.ptr = T.d_ptr.as<int64_t>();
  g.col = T.d_col.as<int32_t>();
  g.val = T.d_val.as<float>();
  g.implicit = c->p.implicit_prefs;
  g.alpha = c->p.alpha;
  g.reg = c->p.reg_param;
  const int64_t batch = row_batch_len(T.own_n, KP);
  HIPCHK(clk.mark(0, st));
  if (c->p.implicit_prefs) {  // into a buffer of the call: c->d_G belongs to the half-sweeps
    const int nblk = audit_gram_blocks(S.own_n);
    HIPCHK(slab.ensure((size_t)nblk * KP * KP * 8));
    HIPCHK(d_G.ensure((size_t)KP * KP * 8));
    HIPCHK(gx.ensure((size_t)batch * KP * 8));
    HIPCHK(launch_audit_gram(KP, g.Y, S.own_n, slab.as<double>(), nblk, d_G.as<double>(), st));
    g.G = d_G.as<double>();
    g.GX = gx.as<double>();
  }
  HIPCHK(clk.mark(1, st));
  g.chunk = row_chunk_len(c, T.own_nnz, "ALBEDO_OBJECTIVE_CHUNK");
  TRYC(plan.build(c, T, OBJ_CHUNK_REC, &g));
  HIPCHK(d_rec.ensure((size_t)std::max<int64_t>(T.own_n, 1) * OBJ_REC * 8));
  HIPCHK(d_other.ensure((size_t)std::max<int64_t>(S.own_n, 1) * 8));
  HIPCHK(d_part.ensure((size_t)OBJ_SUM_BLOCKS * OBJ_REC * 8));
  HIPCHK(d_sum.ensure((size_t)(OBJ_REC + 1) * 8));
  g.rec = d_rec.as<double>();
  HIPCHK(launch_objective_chunks(KP, g, st));
  TRYC(plan.batches(T.own_n, batch, [&](int64_t row0, int64_t nb, int64_t l0, int64_t n_long) -> int {
    g.row0 = row0;
    g.nb = nb;
    HIPCHK(launch_objective_rows(KP, g, l0, n_long, st));
    return ALS_OK;
  }));
  // the other side's n_i ‖y_i‖² from its own rows, then the sums: the records' columns and that vector
  HIPCHK(launch_objective_other(KP, g.Y, S.d_ptr.as<int64_t>(), c->p.implicit_prefs ? S.d_val.as<float>() : nullptr,
                                S.own_n, d_other.as<double>(), st));
  double* sum = d_sum.as<double>();
  HIPCHK(launch_objective_colsum(g.rec, T.own_n, OBJ_REC, d_part.as<double>(), sum, st));
  HIPCHK(launch_objective_colsum(d_other.as<double>(), S.own_n, 1, d_part.as<double>(), sum + OBJ_REC, st));
  HIPCHK(clk.mark(2, st));
  double h[OBJ_REC + 1];
  HIPCHK(copy_st(c, h, d_sum.p, sizeof h, hipMemcpyDeviceToHost));
  if (row_loss_out && T.own_n > 0) {
    std::vector<double> rec((size_t)T.own_n * OBJ_REC);
    HIPCHK(copy_st(c, rec.data(), d_rec.p, rec.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t r = 0; r < T.own_n; ++r) row_loss_out[r] = rec[(size_t)r * OBJ_REC + OBJ_LOSS];
  }
  c->objective_ms[0] = c->p.implicit_prefs ? event_ms(clk.e[0], clk.e[1]) : 0.0;
  c->objective_ms[1] = event_ms(clk.e[1], clk.e[2]);
  c->objective_ms[2] = event_ms(clk.e[0], clk.e[2]);
  out->all_pairs = h[OBJ_ALL_PAIRS];
  out->ratings = h[OBJ_RATINGS];
  out->reg_side = h[OBJ_REG];
  out->reg_other = c->p.reg_param * h[OBJ_REC];
  out->sse = h[OBJ_SSE];
  out->abs_terms = h[OBJ_ABS] + std::fabs(out->reg_other);
  out->total = out->all_pairs + out->ratings + out->reg_side + out->reg_other;
  out->n_ratings = (int64_t)h[OBJ_DEGREE];  // a sum of integers below 2^53: exact
  out->rows = T.own_n;
  return ALS_OK;
}

int objective_ready(const als_ctx* c, const char* who) {
  if (!c->has_ratings || c->model_only) return fail(ALS_E_STATE, std::string(who) + " needs a context holding ratings");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, std::string(who) + " is single-process (world = 1)");
  return ALS_OK;
}

}  // namespace albedo

extern "C" int als_objective(als_ctx* c, int side, double* row_loss_out, als_objective_t* out) {
  if (!c || (side != 0 && side != 1) || !out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  TRYC(objective_ready(c, "als_objective"));
  if (!c->s[0].has_factors || !c->s[1].has_factors)
    return fail(ALS_E_STATE, "als_objective needs the factors of both sides (fit or inject them first)");
  TRYC(set_device(c));
  return objective(c, side, row_loss_out, out);
}

extern "C" int als_objective_timing(const als_ctx* c, double* out3) {
  if (!c || !out3) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 3; ++i) out3[i] = c->objective_ms[i];
  return ALS_OK;
}
