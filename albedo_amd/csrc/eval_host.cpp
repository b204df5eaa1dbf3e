// Host side of held-out pair ranking (eval_pairs.hip): the per-user lists of
// RankingMetricFormatter("als") on ALSModel.transform(pairs) with coldStartStrategy = "drop"
// (ALSRecommenderCV.scala:54-90, RankingMetricFormatter.scala:59-64) and RankingEvaluator.evaluate of
// them (RankingEvaluator.scala:83-139).  C ABI entry points als_rank_pairs, als_evaluate_pairs and
// als_eval_pairs_timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"

namespace albedo {
namespace {

// Stage marks 0 .. n - 1 were taken in order (at most six a call); after the stream is synchronised
// ms5[i] = device time between mark i and mark i + 1, 0 for the stages the call did not reach
void stage_ms(const Marks<6>& clk, int n, double* ms5) {
  for (int i = 0; i < 5; ++i) ms5[i] = i + 1 < n ? event_ms(clk.e[i], clk.e[i + 1]) : 0.0;
}

// The lists of one call on the device: run r (user row rows[r], ascending) has len[r] entries in
// items / scores [n_runs][width]; len[r] = 0 when every score of the user was NaN
struct PairLists {
  DevBuf d_user, d_item, d_uids, d_iids, d_urow, d_irow, d_urows, d_irows, d_runs, d_cnt, d_off, d_nr, d_tmp, d_ent;
  DevBuf d_items, d_scores, d_len, d_segoff, d_segcnt, d_segkeys, d_keyoff, d_keycnt, d_run;
  int64_t n_runs = 0;
  std::vector<int32_t> rows, len;
};

int check_pair_args(const als_ctx* c, int32_t top_k, int32_t width, const char* wname, int64_t n, const int32_t* user,
                    const int32_t* item) {
  if (!c || (n > 0 && (!user || !item))) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (top_k <= 0) return fail(ALS_E_INVALID_ARGUMENT, "top_k should be positive");
  if (width <= 0) return fail(ALS_E_INVALID_ARGUMENT, std::string(wname) + " should be positive");
  if (top_k > TOPK_KC || width > TOPK_KC)
    return fail(ALS_E_UNSUPPORTED,
                std::string("pair ranking on the device supports top_k and ") + wname + " <= " + std::to_string(TOPK_KC));
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "pair ranking is single-process (world = 1)");
  return ALS_OK;
}

// map, group, score, select of n > 0 pairs on c->st (marks 0 .. 4 of the clock, counted in n_marks)
int build_pair_lists(als_ctx* c, int top_k, int width, int64_t n, const int32_t* user, const int32_t* item,
                     PairLists& L, Marks<6>& clk, int& n_marks) {
  Side& S = c->s[ALS_USER];
  Side& T = c->s[ALS_ITEM];
  hipStream_t st = c->st;
  HIPCHK(L.d_user.ensure(n * 4));
  HIPCHK(L.d_item.ensure(n * 4));
  HIPCHK(L.d_uids.ensure(S.n * 4));
  HIPCHK(L.d_iids.ensure(T.n * 4));
  for (DevBuf* b : {&L.d_urow, &L.d_irow, &L.d_urows, &L.d_irows, &L.d_runs, &L.d_cnt}) HIPCHK(b->ensure(n * 4));
  HIPCHK(L.d_off.ensure(n * 8));
  HIPCHK(L.d_nr.ensure(8));
  HIPCHK(L.d_ent.ensure(n * 8));
  const size_t tb = pairs_sort_temp_bytes(n, S.n);
  HIPCHK(L.d_tmp.ensure(std::max<size_t>(tb, 16)));
  HIPCHK(hipMemcpyAsync(L.d_user.p, user, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(L.d_item.p, item, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(L.d_uids.p, S.ids.data(), S.n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(L.d_iids.p, T.ids.data(), T.n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(clk.mark(n_marks++, st));
  HIPCHK(pairs_map(L.d_user.as<int32_t>(), L.d_item.as<int32_t>(), n, L.d_uids.as<int32_t>(), S.n,
                   L.d_iids.as<int32_t>(), T.n, L.d_urow.as<uint32_t>(), L.d_irow.as<uint32_t>(), st));
  HIPCHK(clk.mark(n_marks++, st));
  int64_t nr = 0;
  HIPCHK(pairs_group(n, S.n, L.d_tmp.p, tb, L.d_urow.as<uint32_t>(), L.d_urows.as<uint32_t>(), L.d_irow.as<uint32_t>(),
                     L.d_irows.as<uint32_t>(), L.d_runs.as<uint32_t>(), L.d_cnt.as<int32_t>(), L.d_off.as<int64_t>(),
                     L.d_nr.as<int64_t>(), &nr, st));
  HIPCHK(clk.mark(n_marks++, st));
  if (nr <= 0 || nr > n) return fail(ALS_E_STATE, "pair ranking: run count out of range");
  L.rows.resize(nr);
  std::vector<int32_t> cnt(nr);
  HIPCHK(hipMemcpyAsync(L.rows.data(), L.d_runs.p, nr * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(cnt.data(), L.d_cnt.p, nr * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int64_t n_live = n;
  if ((uint32_t)L.rows[nr - 1] == (uint32_t)S.n) {  // the pairs with an unknown id: dropped
    n_live -= cnt[nr - 1];
    --nr;
  }
  L.rows.resize(nr);
  L.n_runs = nr;
  L.len.assign(nr, 0);
  if (nr == 0) {
    for (int i = 0; i < 2; ++i) HIPCHK(clk.mark(n_marks++, st));
    return ALS_OK;
  }
  HIPCHK(pairs_score(c->KP, c->p.rank, S.d_orig.as<float>(), T.d_orig.as<float>(), L.d_urows.as<uint32_t>(),
                     L.d_irows.as<uint32_t>(), L.d_iids.as<int32_t>(), n_live, L.d_ent.as<uint2>(), st));
  HIPCHK(clk.mark(n_marks++, st));
  HIPCHK(L.d_items.ensure(nr * width * 4));
  HIPCHK(L.d_scores.ensure(nr * width * 4));
  HIPCHK(L.d_len.ensure(nr * 4));
  HIPCHK(pairs_select(L.d_ent.as<uint2>(), L.d_off.as<int64_t>(), L.d_cnt.as<int32_t>(), nr, top_k, width,
                      L.d_items.as<int32_t>(), L.d_scores.as<float>(), L.d_len.as<int32_t>(), st));
  // the users above PAIRS_SEG pairs: one wave per segment, then one merge per user
  std::vector<int64_t> seg_off, key_off;
  std::vector<int32_t> seg_cnt, key_cnt, run;
  int64_t o = 0;
  for (int64_t r = 0; r < nr; ++r) {
    if (cnt[r] > PAIRS_SEG) {
      key_off.push_back((int64_t)seg_off.size() * 64);
      for (int64_t q = 0; q < cnt[r]; q += PAIRS_SEG) {
        seg_off.push_back(o + q);
        seg_cnt.push_back((int32_t)std::min<int64_t>(PAIRS_SEG, cnt[r] - q));
      }
      key_cnt.push_back((int32_t)(seg_off.size() * 64 - key_off.back()));
      run.push_back((int32_t)r);
    }
    o += cnt[r];
  }
  if (!run.empty()) {
    const size_t ns = seg_off.size(), nl = run.size();
    HIPCHK(L.d_segoff.ensure(ns * 8));
    HIPCHK(L.d_segcnt.ensure(ns * 4));
    HIPCHK(L.d_segkeys.ensure(ns * 64 * 8));
    HIPCHK(L.d_keyoff.ensure(nl * 8));
    HIPCHK(L.d_keycnt.ensure(nl * 4));
    HIPCHK(L.d_run.ensure(nl * 4));
    HIPCHK(hipMemcpyAsync(L.d_segoff.p, seg_off.data(), ns * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.d_segcnt.p, seg_cnt.data(), ns * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.d_keyoff.p, key_off.data(), nl * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.d_keycnt.p, key_cnt.data(), nl * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.d_run.p, run.data(), nl * 4, hipMemcpyHostToDevice, st));
    HIPCHK(pairs_select_long(L.d_ent.as<uint2>(), L.d_segoff.as<int64_t>(), L.d_segcnt.as<int32_t>(), (int64_t)ns,
                             L.d_segkeys.as<uint64_t>(), L.d_keyoff.as<int64_t>(), L.d_keycnt.as<int32_t>(),
                             L.d_run.as<int32_t>(), (int64_t)nl, top_k, width, L.d_items.as<int32_t>(),
                             L.d_scores.as<float>(), L.d_len.as<int32_t>(), st));
    HIPCHK(hipStreamSynchronize(st));  // the host arrays above are read by the copies until here
  }
  HIPCHK(clk.mark(n_marks++, st));
  HIPCHK(hipMemcpyAsync(L.len.data(), L.d_len.p, nr * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return ALS_OK;
}

int prepare(als_ctx* c) {
  TRYC(set_device(c));
  TRYC(materialize(c, ALS_USER));
  TRYC(materialize(c, ALS_ITEM));
  c->last_rescan.clear();
  c->last_rescan_ready = true;
  for (double& v : c->eval_ms) v = 0.0;
  return ALS_OK;
}

}  // namespace
}  // namespace albedo

using namespace albedo;

extern "C" {

int als_rank_pairs(als_ctx* c, int32_t top_k, int32_t width, int64_t n, const int32_t* user, const int32_t* item,
                   int64_t* n_users_out, int32_t* users_out, int32_t* len_out, int32_t* items_out, float* scores_out,
                   int64_t cap) {
  TRYC(check_pair_args(c, top_k, width, "width", n, user, item));
  if (!n_users_out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  TRYC(prepare(c));
  *n_users_out = 0;
  const Side& S = c->s[ALS_USER];
  if (n <= 0 || S.n == 0 || c->s[ALS_ITEM].n == 0) return ALS_OK;
  PairLists L;
  Marks<6> clk;
  int n_marks = 0;
  Drain queued{c->st};
  TRYC(build_pair_lists(c, top_k, width, n, user, item, L, clk, n_marks));
  stage_ms(clk, n_marks, c->eval_ms);
  int64_t nu = 0;
  for (int64_t r = 0; r < L.n_runs; ++r) nu += L.len[r] > 0;
  *n_users_out = nu;
  if (nu == 0 || nu > cap) return ALS_OK;
  std::vector<int32_t> hi;
  std::vector<float> hs;
  if (items_out) {
    hi.resize((size_t)L.n_runs * width);
    HIPCHK(copy_st(c, hi.data(), L.d_items.p, hi.size() * 4, hipMemcpyDeviceToHost));
  }
  if (scores_out) {
    hs.resize((size_t)L.n_runs * width);
    HIPCHK(copy_st(c, hs.data(), L.d_scores.p, hs.size() * 4, hipMemcpyDeviceToHost));
  }
  int64_t w = 0;
  for (int64_t r = 0; r < L.n_runs; ++r) {
    if (L.len[r] <= 0) continue;
    if (users_out) users_out[w] = S.ids[L.rows[r]];
    if (len_out) len_out[w] = L.len[r];
    if (items_out) std::memcpy(items_out + w * width, &hi[(size_t)r * width], (size_t)width * 4);
    if (scores_out) std::memcpy(scores_out + w * width, &hs[(size_t)r * width], (size_t)width * 4);
    ++w;
  }
  return ALS_OK;
}

int als_evaluate_pairs(als_ctx* c, int32_t metric, int32_t top_k, int32_t k, int64_t n_pairs, const int32_t* user,
                       const int32_t* item, int64_t n_act, const int32_t* act_user, const int32_t* act_item,
                       const int64_t* act_key, double* mean_out, int64_t* n_users_out, int32_t* users_out,
                       double* per_user_out, int64_t cap) {
  TRYC(check_pair_args(c, top_k, k, "k", n_pairs, user, item));
  if (!mean_out || !n_users_out || (n_act > 0 && (!act_user || !act_item || !act_key)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (metric != ALS_METRIC_NDCG && metric != ALS_METRIC_PRECISION && metric != ALS_METRIC_MAP)
    return fail(ALS_E_INVALID_ARGUMENT, "unknown metric " + std::to_string(metric));
  TRYC(prepare(c));
  *mean_out = NAN;
  *n_users_out = 0;
  const Side& S = c->s[ALS_USER];
  if (n_pairs <= 0 || n_act <= 0 || S.n == 0 || c->s[ALS_ITEM].n == 0) return ALS_OK;
  hipStream_t st = c->st;
  PairLists L;
  DevBuf d_au, d_ai, d_ak, d_row, d_rows, d_idx, d_idxs, d_runs, d_cnt, d_off, d_nr, d_tmp, d_act, d_actn, d_gain;
  DevBuf d_prow, d_arow, d_vals;
  Marks<6> clk;
  int n_marks = 0;
  Drain queued{st};
  TRYC(build_pair_lists(c, top_k, k, n_pairs, user, item, L, clk, n_marks));
  // intoUserActualItems of the actual rows, restricted to the model's users (as als_evaluate_ndcg)
  HIPCHK(d_au.ensure(n_act * 4));
  HIPCHK(d_ai.ensure(n_act * 4));
  HIPCHK(d_ak.ensure(n_act * 8));
  HIPCHK(hipMemcpyAsync(d_au.p, act_user, n_act * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ai.p, act_item, n_act * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ak.p, act_key, n_act * 8, hipMemcpyHostToDevice, st));
  for (DevBuf* b : {&d_row, &d_rows, &d_idx, &d_idxs, &d_runs, &d_cnt}) HIPCHK(b->ensure(n_act * 4));
  HIPCHK(d_off.ensure(n_act * 8));
  HIPCHK(d_nr.ensure(8));
  const size_t tb = eval_sort_temp_bytes(n_act);
  HIPCHK(d_tmp.ensure(std::max<size_t>(tb, 16)));
  HIPCHK(eval_group_users(d_au.as<int32_t>(), n_act, L.d_uids.as<int32_t>(), S.n, d_tmp.p, tb, d_row.as<uint32_t>(),
                          d_rows.as<uint32_t>(), d_idx.as<uint32_t>(), d_idxs.as<uint32_t>(), d_runs.as<uint32_t>(),
                          d_cnt.as<int32_t>(), d_off.as<int64_t>(), d_nr.as<int64_t>(), st));
  int64_t na = 0;
  HIPCHK(hipMemcpyAsync(&na, d_nr.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (na < 0 || na > n_act) return fail(ALS_E_STATE, "pair evaluation: run count out of range");
  std::vector<int32_t> arows(na);
  HIPCHK(hipMemcpyAsync(arows.data(), d_runs.p, na * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (na > 0 && (uint32_t)arows[na - 1] == 0xFFFFFFFFu) --na;  // users unknown to the model
  // inner join of the two ascending row lists
  std::vector<int32_t> prow, arow;
  for (int64_t i = 0, j = 0; i < L.n_runs && j < na;) {
    if (L.rows[i] < arows[j]) ++i;
    else if (L.rows[i] > arows[j]) ++j;
    else {
      if (L.len[i] > 0) prow.push_back((int32_t)i), arow.push_back((int32_t)j);
      ++i, ++j;
    }
  }
  const int64_t ne = (int64_t)prow.size();
  *n_users_out = ne;
  if (ne == 0) {
    HIPCHK(hipStreamSynchronize(st));
    stage_ms(clk, n_marks, c->eval_ms);
    return ALS_OK;
  }
  HIPCHK(d_act.ensure(na * k * 4));
  HIPCHK(d_actn.ensure(na * 4));
  HIPCHK(eval_actual_lists(d_idxs.as<uint32_t>(), d_off.as<int64_t>(), d_cnt.as<int32_t>(), na, d_ak.as<int64_t>(),
                           d_ai.as<int32_t>(), k, d_act.as<int32_t>(), d_actn.as<int32_t>(), st));
  // ndcgAt's gains from the host's libm: the host evaluator's table (1.0 / math.log(i + 2))
  std::vector<double> gain(k);
  for (int i = 0; i < k; ++i) gain[i] = 1.0 / std::log((double)(i + 2));
  HIPCHK(d_gain.ensure(k * 8));
  HIPCHK(d_prow.ensure(ne * 4));
  HIPCHK(d_arow.ensure(ne * 4));
  HIPCHK(d_vals.ensure(ne * 8));
  HIPCHK(hipMemcpyAsync(d_gain.p, gain.data(), k * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_prow.p, prow.data(), ne * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_arow.p, arow.data(), ne * 4, hipMemcpyHostToDevice, st));
  HIPCHK(eval_metric(metric, L.d_items.as<int32_t>(), k, L.d_len.as<int32_t>(), 0, d_prow.as<int32_t>(),
                     d_act.as<int32_t>(), d_actn.as<int32_t>(), d_arow.as<int32_t>(), ne, k, d_gain.as<double>(),
                     d_vals.as<double>(), st));
  HIPCHK(clk.mark(n_marks++, st));
  std::vector<double> vals(ne);
  HIPCHK(hipMemcpyAsync(vals.data(), d_vals.p, ne * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  stage_ms(clk, n_marks, c->eval_ms);
  double sum = 0.0;  // mean over users in ascending id order (RankingMetrics: RDD mean)
  for (int64_t i = 0; i < ne; ++i) sum += vals[i];
  *mean_out = sum / (double)ne;
  if (ne <= cap) {
    if (users_out)
      for (int64_t i = 0; i < ne; ++i) users_out[i] = S.ids[L.rows[prow[i]]];
    if (per_user_out) std::memcpy(per_user_out, vals.data(), ne * 8);
  }
  return ALS_OK;
}

int als_eval_pairs_timing(const als_ctx* c, double* out5) {
  if (!c || !out5) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 5; ++i) out5[i] = c->eval_ms[i];
  return ALS_OK;
}

}  // extern "C"
