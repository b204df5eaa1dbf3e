// als_similar / als_similar_vectors: cosine top-k of one side against itself (similar.hip holds the kernels).
// Both calls build the side's unit image on the device and hand it to a scan the project already has:
//   scan tier    scan_lists of query_topk_host.cpp (launch_query_scan / launch_query_merge), the unit image as Y,
//                the gathered unit rows as queries and each query's own row as its one exclusion;
//   passes tier  a transient model-only context whose two sides both view the unit image (restricted to the
//                rows that have a direction, which keeps it inside als_recommend_unseen's finite-factor
//                contract), served by als_recommend_unseen with the pairs (id, id).  The context lives and
//                dies with the call; nothing is cached on the parent and none of its counters move.
// Both tiers score with the F2J sdot and keep (score desc, id asc), so their lists are bit-identical.  The
// calls read the model and write nothing of it but similar_ms / similar_stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "kernels.h"

using namespace albedo;

namespace {

// Rows asked from which the passes tier is the default.  Measured on one MI355X at c2 (rank 64, k = 30, two
// sweeps; profiles/similar_c2.json, DESIGN.md "Similar rows within one side"), wall ms scan / passes:
//   item side (200K rows)  1,024 rows 2.5 / 27.9    16,384 rows 20.2 / 73.2    all 200K rows 197.9 / 734.8
//   user side (1M rows)    1,024 rows 9.1 / 59.8    all 1M rows 4,439 / 829
// On the item side the two tiers' wall times do not cross: the scan wins at every row count, the whole side
// included (57 % of the item rows fail the passes' certification and are rescored).  On the user side they
// cross somewhere between 1,024 and 1M rows; no row count in between was measured.  A threshold on n_q alone
// cannot serve both, so it is set above the item side's row count, where the scan was seen to win, and below
// the user side's, where the passes were.  Between the two it is not backed by a measurement, and a straight
// line through the two user-side points puts that side's crossing near 16K rows: a caller asking tens of
// thousands of user rows should force the passes tier (ALBEDO_SIMILAR_TIER=passes).
constexpr int64_t SIMILAR_PASSES_MIN_ROWS = (int64_t)1 << 18;

int choose_tier(int64_t n_q) {
  const char* e = std::getenv("ALBEDO_SIMILAR_TIER");  // read per call
  if (e && !std::strcmp(e, "scan")) return 0;
  if (e && !std::strcmp(e, "passes")) return 1;
  return n_q >= SIMILAR_PASSES_MIN_ROWS ? 1 : 0;
}

// ALBEDO_SIMILAR_TRACE=1 (diagnostic, like ALBEDO_TOPK_TRACE): the passes tier prints one line on stderr with
// what only the transient context knows and als_similar_stats has no room for: its build time, its
// als_recommend_unseen timers and counters and its als_topk_stats (chunks scanned against a full scan, rows
// rescored).  tools/similar_time.py reads it; include/albedo_als.h names it beside ALBEDO_SIMILAR_TIER
bool trace_on() {
  const char* e = std::getenv("ALBEDO_SIMILAR_TRACE");
  return e && *e && *e != '0';
}

struct Transient {  // the passes tier's context, destroyed with the call
  als_ctx* c = nullptr;
  Transient() = default;
  Transient(const Transient&) = delete;
  Transient& operator=(const Transient&) = delete;
  ~Transient() {
    if (c) als_destroy(c);
  }
};

void pad_lists(int32_t* ids, float* scores, int64_t n) {
  std::fill(ids, ids + n, -1);
  std::fill(scores, scores + n, NAN);
}

// similar_ms of a scan-tier call from its five marks: 0 start, 1 unit image, 2 queries, 3 scan, 4 merge
void scan_timing(als_ctx* c, const Marks<5>& clk) {
  c->similar_ms[0] = event_ms(clk.e[0], clk.e[2]);
  c->similar_ms[1] = event_ms(clk.e[2], clk.e[3]);
  c->similar_ms[2] = event_ms(clk.e[3], clk.e[4]);
  c->similar_ms[3] = event_ms(clk.e[0], clk.e[4]);
}

// The side's unit image and direction flags on c->st (queued); the side is materialised
int unit_image(als_ctx* c, const Side& S, DevBuf& d_unit, DevBuf& d_flag) {
  HIPCHK(d_unit.ensure((size_t)std::max<int64_t>(S.n, 1) * c->KP * 4));
  HIPCHK(d_flag.ensure((size_t)std::max<int64_t>(S.n, 1) * 4));
  HIPCHK(launch_similar_unit(S.d_orig.as<float>(), c->KP, S.n, c->p.rank, d_unit.as<float>(), c->KP, d_flag.as<int32_t>(),
                             c->st));
  return ALS_OK;
}

int64_t count_zero(const std::vector<int32_t>& f) { return (int64_t)std::count(f.begin(), f.end(), 0); }

// rows [nq]: the dense row of each requested id, -1 when unknown (null: every row in order)
int similar_scan(als_ctx* c, int side, int k, const int32_t* rows, int64_t nq, int32_t* ids_out, float* scores_out) {
  Side& S = c->s[side];
  hipStream_t st = c->st;
  const int rank = c->p.rank;
  DevBuf d_unit, d_flag, d_rows, d_q, d_ptr, d_keys, d_ids;
  ScanBuffers B;
  Marks<5> clk;
  std::vector<int32_t> flag((size_t)S.n);
  Drain queued{st};
  HIPCHK(d_q.ensure((size_t)nq * rank * 4));
  HIPCHK(d_ptr.ensure((size_t)(nq + 1) * 8));
  HIPCHK(d_keys.ensure((size_t)nq * 8));
  HIPCHK(d_ids.ensure((size_t)std::max<int64_t>(S.n, 1) * 4));
  if (rows) {
    HIPCHK(d_rows.ensure((size_t)nq * 4));
    HIPCHK(hipMemcpyAsync(d_rows.p, rows, (size_t)nq * 4, hipMemcpyHostToDevice, st));
  }
  if (S.n > 0) HIPCHK(hipMemcpyAsync(d_ids.p, S.ids.data(), (size_t)S.n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(clk.mark(0, st));
  TRYC(unit_image(c, S, d_unit, d_flag));
  HIPCHK(clk.mark(1, st));
  HIPCHK(launch_similar_gather(d_unit.as<float>(), c->KP, rank, d_flag.as<int32_t>(), rows ? d_rows.as<int32_t>() : nullptr,
                               nq, d_q.as<float>(), d_ptr.as<int64_t>(), d_keys.as<uint64_t>(), st));
  HIPCHK(clk.mark(2, st));
  if (S.n > 0) HIPCHK(hipMemcpyAsync(flag.data(), d_flag.p, (size_t)S.n * 4, hipMemcpyDeviceToHost, st));
  TRYC(B.ensure(c, S.n, nq, k));  // behind mark 2, where these allocations have always stood
  TRYC(scan_lists(c, B, k, d_unit.as<float>(), S.n, d_q.as<float>(), nq, d_ptr.as<int64_t>(), d_keys.as<uint64_t>(),
                  d_ids.as<int32_t>(), &clk.e[3], &clk.e[4], ids_out, scores_out));
  scan_timing(c, clk);
  c->similar_stats[1] = count_zero(flag);
  return ALS_OK;
}

int similar_passes(als_ctx* c, int side, int k, const int32_t* rows, int64_t nq, int32_t* ids_out, float* scores_out) {
  Side& S = c->s[side];
  hipStream_t st = c->st;
  const int KP = c->KP;
  DevBuf d_unit, d_flag, d_good, d_comp;
  Transient tr;  // after the buffers its sides view: it goes first
  Marks<4> clk;
  std::vector<int32_t> flag((size_t)S.n);
  Drain queued{st};
  HIPCHK(clk.mark(0, st));
  TRYC(unit_image(c, S, d_unit, d_flag));
  HIPCHK(clk.mark(1, st));
  HIPCHK(hipMemcpyAsync(flag.data(), d_flag.p, (size_t)S.n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int32_t> good;  // dense rows that have a direction, ascending
  good.reserve((size_t)S.n);
  for (int64_t r = 0; r < S.n; ++r)
    if (flag[(size_t)r]) good.push_back((int32_t)r);
  const int64_t ng = (int64_t)good.size();
  c->similar_stats[1] = S.n - ng;
  // the requested ids that can have a list, in caller order, and where each one's list goes
  std::vector<int32_t> sub;
  std::vector<int64_t> at;
  const bool whole = !rows && ng == S.n;  // every row asked and served: no subset, no scatter
  if (!whole) {
    for (int64_t i = 0; i < nq; ++i) {
      const int64_t r = rows ? rows[i] : i;
      if (r < 0 || !flag[(size_t)r]) continue;
      sub.push_back(S.ids[(size_t)r]);
      at.push_back(i);
    }
  }
  const int64_t ns = whole ? nq : (int64_t)sub.size();
  if (ns < nq) pad_lists(ids_out, scores_out, nq * k);
  if (ns == 0) {
    c->similar_ms[0] = c->similar_ms[3] = event_ms(clk.e[0], clk.e[1]);
    return ALS_OK;
  }
  const auto w0 = std::chrono::steady_clock::now();
  HIPCHK(clk.mark(2, st));
  const float* img = d_unit.as<float>();
  if (ng < S.n) {
    HIPCHK(d_good.ensure((size_t)ng * 4));
    HIPCHK(d_comp.ensure((size_t)ng * KP * 4));
    HIPCHK(hipMemcpyAsync(d_good.p, good.data(), (size_t)ng * 4, hipMemcpyHostToDevice, st));
    HIPCHK(launch_similar_compact(img, KP, d_good.as<int32_t>(), ng, d_comp.as<float>(), st));
    img = d_comp.as<float>();
  }
  HIPCHK(clk.mark(3, st));
  HIPCHK(hipStreamSynchronize(st));  // the transient context reads the image on its own stream
  // Side as als_model_create leaves it, from device buffers: both sides view the one image
  TRYC(bare_context(c->p.rank, c->dev, &tr.c));
  als_ctx* t = tr.c;
  t->model_only = true;
  const DevBuf& image = ng < S.n ? d_comp : d_unit;
  for (int s = 0; s < 2; ++s) {
    Side& X = t->s[s];
    X.n = ng;
    X.ids.resize((size_t)ng);
    for (int64_t j = 0; j < ng; ++j) X.ids[(size_t)j] = S.ids[(size_t)good[(size_t)j]];
    X.d_orig.share(image);
    X.orig_valid = true;
    X.fold_gram_valid = false;
    X.has_factors = true;
    X.starts = {0, ng};
    X.maxrows = ng;
    X.chpad = std::max<int64_t>(1, ng);
  }
  const double build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  // each requested id leaves itself out: the pairs (id, id), once per id
  std::vector<int32_t> self = whole ? t->s[0].ids : sub;
  if (!whole) {
    std::sort(self.begin(), self.end());
    self.erase(std::unique(self.begin(), self.end()), self.end());
  }
  std::vector<int32_t> tid;
  std::vector<float> tsc;
  int32_t* oi = ids_out;
  float* os = scores_out;
  if (ns < nq) {
    tid.resize((size_t)ns * k);
    tsc.resize((size_t)ns * k);
    oi = tid.data();
    os = tsc.data();
  }
  TRYC(als_recommend_unseen(t, 0, k, whole ? nullptr : sub.data(), ns, ALS_EXCLUDE_PAIRS, (int64_t)self.size(),
                            self.data(), self.data(), nullptr, oi, os));
  if (ns < nq)
    for (int64_t j = 0; j < ns; ++j) {
      std::memcpy(ids_out + at[(size_t)j] * k, oi + j * k, (size_t)k * 4);
      std::memcpy(scores_out + at[(size_t)j] * k, os + j * k, (size_t)k * 4);
    }
  c->similar_stats[3] = t->unseen_stats[1];
  c->similar_ms[0] = event_ms(clk.e[0], clk.e[1]) + event_ms(clk.e[2], clk.e[3]);
  c->similar_ms[1] = t->unseen_ms[0] + t->unseen_ms[1] + t->unseen_ms[3];
  c->similar_ms[2] = t->unseen_ms[2];
  c->similar_ms[3] = c->similar_ms[0] + t->unseen_ms[4];
  if (trace_on())
    std::fprintf(stderr,
                 "[similar] passes: rows %lld of %lld with a direction, context %.3f ms (wall), unit image %.3f ms, "
                 "compaction %.3f ms; unseen ms %.3f %.3f %.3f %.3f %.3f; unseen stats %lld %lld %lld %lld; topk stats "
                 "%lld %lld %lld %lld\n",
                 (long long)ng, (long long)S.n, build_ms, event_ms(clk.e[0], clk.e[1]), event_ms(clk.e[2], clk.e[3]),
                 t->unseen_ms[0], t->unseen_ms[1], t->unseen_ms[2], t->unseen_ms[3], t->unseen_ms[4],
                 (long long)t->unseen_stats[0], (long long)t->unseen_stats[1], (long long)t->unseen_stats[2],
                 (long long)t->unseen_stats[3], (long long)t->topk_stats[0], (long long)t->topk_stats[1],
                 (long long)t->topk_stats[2], (long long)t->topk_stats[3]);
  return ALS_OK;
}

// ptr0: the exclusion ranges shifted to start at 0 ([n_q + 1]), empty when the call has none
int similar_vectors(als_ctx* c, int side, int k, int64_t n_q, const float* q, const std::vector<int64_t>& ptr0,
                    const int32_t* excl_ids, int32_t* ids_out, float* scores_out) {
  Side& S = c->s[side];
  hipStream_t st = c->st;
  const int rank = c->p.rank;
  DevBuf d_unit, d_flag, d_raw, d_q, d_ids;
  Exclusions X;
  ScanBuffers B;
  Marks<5> clk;
  std::vector<int32_t> flag((size_t)S.n);
  Drain queued{st};
  HIPCHK(d_raw.ensure((size_t)n_q * rank * 4));
  HIPCHK(d_q.ensure((size_t)n_q * rank * 4));
  HIPCHK(d_ids.ensure((size_t)std::max<int64_t>(S.n, 1) * 4));
  HIPCHK(hipMemcpyAsync(d_raw.p, q, (size_t)n_q * rank * 4, hipMemcpyHostToDevice, st));
  if (S.n > 0) HIPCHK(hipMemcpyAsync(d_ids.p, S.ids.data(), (size_t)S.n * 4, hipMemcpyHostToDevice, st));
  TRYC(X.upload(c, n_q, ptr0, excl_ids));
  HIPCHK(clk.mark(0, st));
  TRYC(unit_image(c, S, d_unit, d_flag));
  HIPCHK(clk.mark(1, st));
  HIPCHK(launch_similar_unit(d_raw.as<float>(), rank, n_q, rank, d_q.as<float>(), rank, nullptr, st));
  TRYC(X.map(c, n_q, d_ids.as<int32_t>(), S.n));
  HIPCHK(clk.mark(2, st));
  if (S.n > 0) HIPCHK(hipMemcpyAsync(flag.data(), d_flag.p, (size_t)S.n * 4, hipMemcpyDeviceToHost, st));
  TRYC(B.ensure(c, S.n, n_q, k));  // behind mark 2, as in similar_scan
  TRYC(scan_lists(c, B, k, d_unit.as<float>(), S.n, d_q.as<float>(), n_q, X.ptr(), X.keys(), d_ids.as<int32_t>(),
                  &clk.e[3], &clk.e[4], ids_out, scores_out));
  scan_timing(c, clk);
  c->similar_stats[1] = count_zero(flag);
  return ALS_OK;
}

const char* side_name(int side) { return side == ALS_USER ? "user" : "item"; }

}  // namespace

extern "C" int als_similar(als_ctx* c, int side, int32_t k, const int32_t* subset, int64_t n_subset, int32_t* src_ids_out,
                           int32_t* ids_out, float* scores_out) {
  if (!c || (side != 0 && side != 1) || k < 1 || (subset && n_subset < 0) || !ids_out || !scores_out)
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (k > 64) return fail(ALS_E_UNSUPPORTED, "als_similar keeps at most 64 rows per list (k <= 64)");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "als_similar is single-process (world = 1)");
  if (subset && n_subset > (int64_t)0x7FFFFFFF)
    return fail(ALS_E_UNSUPPORTED, "als_similar takes at most 2^31 - 1 rows a call");
  for (double& v : c->similar_ms) v = 0.0;
  for (int64_t& v : c->similar_stats) v = 0;
  Side& S = c->s[side];
  if (!S.has_factors)
    return fail(ALS_E_STATE, std::string("als_similar needs the ") + side_name(side) +
                                 " factors (fit, inject or load them first)");
  const int64_t nq = subset ? n_subset : S.n;
  if (src_ids_out && nq > 0) std::memcpy(src_ids_out, subset ? subset : S.ids.data(), (size_t)nq * 4);
  if (nq == 0) return ALS_OK;
  TRYC(set_device(c));
  TRYC(materialize(c, side));
  std::vector<int32_t> rows;
  int64_t n_known = nq;
  if (subset) {
    rows.resize((size_t)nq);
    n_known = 0;
    for (int64_t i = 0; i < nq; ++i) {
      rows[(size_t)i] = (int32_t)find_row(S, subset[i]);
      n_known += rows[(size_t)i] >= 0;
    }
  }
  c->similar_stats[0] = n_known;
  const int tier = choose_tier(nq);
  c->similar_stats[2] = tier;
  const int32_t* r = subset ? rows.data() : nullptr;
  return tier == 0 ? similar_scan(c, side, k, r, nq, ids_out, scores_out)
                   : similar_passes(c, side, k, r, nq, ids_out, scores_out);
}

extern "C" int als_similar_vectors(als_ctx* c, int dst_side, int32_t k, int64_t n_q, const float* q, const int64_t* excl_ptr,
                                   const int32_t* excl_ids, int32_t* ids_out, float* scores_out) {
  if (!c || (dst_side != 0 && dst_side != 1) || k < 1 || n_q < 0 || (n_q > 0 && (!q || !ids_out || !scores_out)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (k > 64) return fail(ALS_E_UNSUPPORTED, "als_similar_vectors keeps at most 64 rows per query (k <= 64)");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "als_similar_vectors is single-process (world = 1)");
  if (n_q > (int64_t)0x7FFFFFFF) return fail(ALS_E_UNSUPPORTED, "als_similar_vectors takes at most 2^31 - 1 queries a call");
  std::vector<int64_t> ptr0;
  TRYC(exclusion_ranges("als_similar_vectors", ALS_E_UNSUPPORTED, n_q, excl_ptr, &excl_ids, &ptr0));
  for (double& v : c->similar_ms) v = 0.0;
  for (int64_t& v : c->similar_stats) v = 0;
  if (n_q == 0) return ALS_OK;
  if (!c->s[dst_side].has_factors)
    return fail(ALS_E_STATE, std::string("als_similar_vectors needs the ") + side_name(dst_side) +
                                 " factors (fit, inject or load them first)");
  TRYC(set_device(c));
  TRYC(materialize(c, dst_side));
  c->similar_stats[0] = n_q;
  return similar_vectors(c, dst_side, k, n_q, q, ptr0, excl_ids, ids_out, scores_out);
}

extern "C" int als_similar_timing(const als_ctx* c, double* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->similar_ms[i];
  return ALS_OK;
}

extern "C" int als_similar_stats(const als_ctx* c, int64_t* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->similar_stats[i];
  return ALS_OK;
}
