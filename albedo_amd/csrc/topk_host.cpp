// Host side of top-k (topk.hip) and NDCG (eval.hip): the per-call plan of the dst side, the passes over
// the src rows, the three ways a call's lists reach the caller's arrays, and the C ABI entry points
// als_recommend, als_recommend_unseen (the same passes at the filter's depth, their lists filtered on the
// device), als_evaluate_ndcg, als_evaluate_ranking and the top-k counters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <numeric>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "albedo_als.h"
#include "engine.h"
#include "host_math.h"
#include "kernels.h"

namespace albedo {

// One recommendForAll* call's prepared dst side (topk.hip): max row norms (the pre-selection's error
// bound), fp16 power-of-two scales, the descending-norm fp16 image with chunk head norms, dst ids on
// the device; plus the per-chunk scratch reused by every src chunk.
struct TopkPlan {
  int src = 0, k = 0;
  bool exact_only = false;
  double tmax = 0.0, smax = 0.0, ssc = 1.0, tsc = 1.0;
  int CH = 0;
  int64_t n_chunks = 0, n_super = 0;
  bool prune = false;
  DevBuf d_th, d_keys, d_perm, d_nperm, d_tp, d_tmp, d_dstids, d_VP, d_cfeat, d_supf, d_probe, d_slab, d_G;
  DevBuf d_scan;
  // a pass's device buffers; two sets, so that a pass's select / rescans (on the post stream) can run
  // while the next pass orders and scans with the other set (r06)
  struct PassBufs {
    DevBuf d_src, d_ls, d_lc, d_flag, d_okeys, d_order, d_srcs, d_otmp, d_thr, d_sf, d_mask, d_kth, d_inv;
    DevBuf d_cnt;  // int [4]: the range's flagged count, the rescan work counter, the set's flagged total
  } pb[2];
  // per call (topk_begin .. topk_finish): the passes run back to back with no host round trip; their
  // event pairs, scan counters (d_scan[pass]) and rows per scan workgroup are read at the end
  // per pass: start, order + mask done, scan done, then per output range: select done, rescans done
  std::vector<hipEvent_t> evs;
  struct PassRec { int rpw; size_t e0; int ranges; };
  std::vector<PassRec> passes;
  int64_t n_passes = 0;
  hipError_t event(size_t i, hipEvent_t* e) {  // the i-th event of the pool (created on demand)
    while (evs.size() <= i) {
      hipEvent_t x;
      const hipError_t r = hipEventCreate(&x);
      if (r != hipSuccess) return r;
      evs.push_back(x);
    }
    *e = evs[i];
    return hipSuccess;
  }
  ~TopkPlan() {
    for (hipEvent_t e : evs)
      if (e) (void)hipEventDestroy(e);
  }
};

// The dst side's Gram Σ t tᵀ (original basis) on the device, copied into c->h_plan ([KP][KP] fp64)
// on st; `done` is recorded behind the copy, so the host can wait for it alone.
int topk_dst_gram(als_ctx* c, const Side& T, TopkPlan& P, hipEvent_t done) {
  const int KP = c->KP;
  const int nblk = gram_slab_blocks(KP, T.n);
  double* slab = c->slab.as<double>();  // the sweeps' Gram scratch (idle here, same stream) when it fits
  if (c->slab_blocks < nblk || !slab) {
    HIPCHK(P.d_slab.ensure(gram_slab_doubles(KP, nblk) * 8));
    slab = P.d_slab.as<double>();
  }
  HIPCHK(P.d_G.ensure((size_t)KP * KP * 8));
  HIPCHK(launch_gram(KP, T.d_orig.as<float>(), T.n, slab, nblk, P.d_G.as<double>(), c->st));
  // into pinned memory: a pageable copy would block the host here until the stream drains
  HIPCHK(hipMemcpyAsync(c->h_plan, P.d_G.p, (size_t)KP * KP * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipEventRecord(done, c->st));
  return ALS_OK;
}

// The leading TOPK_M eigenvectors of that Gram, fp64 [TOPK_M][KP]: the directions the top-k chunk
// bound keeps exactly (topk.hip).  Runs on the host while the row norms are computed on the device.
int topk_dst_basis(als_ctx* c, const double* Gf, std::vector<double>& VP) {
  const int KP = c->KP, k = c->p.rank;
  std::vector<double> Gk((size_t)k * k), w(k), V((size_t)k * k);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) Gk[(size_t)i * k + j] = Gf[(size_t)i * KP + j];
  if (!sym_eig(k, Gk.data(), w.data(), V.data()))
    return fail(ALS_E_NOT_POSITIVE_DEFINITE,
                "the dst Gram matrix is not finite (row norms above ~2^63) or its eigendecomposition did not converge");
  std::vector<int> idx(k);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return w[a] > w[b]; });
  VP.assign((size_t)TOPK_M * KP, 0.0);
  for (int d = 0; d < TOPK_M && d < k; ++d)
    for (int i = 0; i < k; ++i) VP[(size_t)d * KP + i] = V[(size_t)i * k + idx[d]];
  return ALS_OK;
}

// The scan prunes against the kt-th best candidate so far, not the 64th: certification needs a gap
// between the k-th exact score and the kt-th approximate one (~1e-3 relative), and k + 16 leaves one
// while the threshold rises faster than at 64 (fewer dst chunks scanned once the factors converge).
// The lists still hold 64 and the best 64 are rescored.
// the running threshold's rank in the candidate lists: k + 16 (c4 all users after 25 sweeps: k + 8 /
// 12 / 16 / 24 -> 33.6 / 47.6 / 50.7 / 46.9M users/s; fewer leave more rows to the exact rescan)
int topk_threshold_rank(int k) { return std::max(k, std::min(TOPK_KC, k + ALBEDO_TOPK_KT_EXTRA)); }

int topk_plan(als_ctx* c, int src, int k, TopkPlan& P, const std::function<void(const char*)>& stamp = nullptr) {
  auto st = [&](const char* w) {
    if (stamp) stamp(w);
  };
  P.src = src;
  P.k = k;
  P.exact_only = k > TOPK_KC;  // no MFMA pre-selection: exact full scan of every row
  TRYC(materialize(c, src));
  TRYC(materialize(c, 1 - src));
  st("  plan: materialize dst");
  Side& S = c->s[src];
  Side& T = c->s[1 - src];
  const int KP = c->KP;
  // the dst Gram first; its host eigensolve overlaps the row-norm launches behind it
  std::vector<double> VP;
  hipEvent_t ev_gram;
  HIPCHK(P.event(0, &ev_gram));
  if (!c->h_plan) HIPCHK(hipHostMalloc((void**)&c->h_plan, ((size_t)KP * KP + 2) * 8, hipHostMallocDefault));
  {
    DevBuf d_nrm;
    HIPCHK(d_nrm.ensure(16));
    // d_nrm outlives the work queued on it: an early return drains the stream before it is freed
    Drain queued{c->st};
    TRYC(topk_dst_gram(c, T, P, ev_gram));
    HIPCHK(launch_rownorm_max(T.d_orig.as<float>(), T.n, KP, c->p.rank, d_nrm.as<unsigned long long>(), c->st));
    HIPCHK(launch_rownorm_max(S.d_orig.as<float>(), S.n, KP, c->p.rank, d_nrm.as<unsigned long long>() + 1, c->st));
    double* nr = c->h_plan + (size_t)KP * KP;
    HIPCHK(hipMemcpyAsync(nr, d_nrm.p, 16, hipMemcpyDeviceToHost, c->st));
    st("  plan: dst Gram + row norms enqueued");
    HIPCHK(hipEventSynchronize(ev_gram));
    st("  plan: dst Gram");
    TRYC(topk_dst_basis(c, c->h_plan, VP));
    st("  plan: host eigensolve (row norms on the device)");
    HIPCHK(hipStreamSynchronize(c->st));
    queued.s = nullptr;
    P.tmax = nr[0];
    P.smax = nr[1];
  }
  // |entry| <= row norm, so scaling by 2^(13 - ceil(log2 max norm)) keeps every fp16 value < 2^13
  auto pow2_scale = [](double m) {
    if (!(m > 0.0) || !std::isfinite(m)) return 1.0;
    int e = 0;
    std::frexp(m, &e);  // m < 2^e
    e = std::max(-60, std::min(60, 13 - e));
    return std::ldexp(1.0, e);
  };
  P.ssc = pow2_scale(P.smax);
  P.tsc = pow2_scale(P.tmax);
  // dst side in descending-norm order, fp16 rows + chunk head norms (also for k > 64: the exact scan
  // visits the dst rows in this norm order and stops early)
  P.CH = topk_chunk_rows(KP);
  P.n_chunks = (T.n + P.CH - 1) / P.CH;
  P.n_super = (P.n_chunks + TOPK_SUPER - 1) / TOPK_SUPER;
  // the chunk bound prunes only catalogues larger than the candidate lists (smaller ones are scanned
  // whole: the lists then hold every dst row, which select's n_dst <= TOPK_KC shortcut relies on)
  P.prune = T.n > TOPK_KC;
  st("  plan: row norms");
  HIPCHK(P.d_VP.ensure(VP.size() * 8));
  HIPCHK(hipMemcpyAsync(P.d_VP.p, VP.data(), VP.size() * 8, hipMemcpyHostToDevice, c->st));
  const int64_t nn = std::max<int64_t>(T.n, 1);
  HIPCHK(P.d_th.ensure((size_t)std::max<int64_t>(P.n_chunks, 1) * P.CH * KP * 2));
  HIPCHK(P.d_keys.ensure((size_t)nn * 16));
  HIPCHK(P.d_perm.ensure((size_t)nn * 8));
  HIPCHK(P.d_nperm.ensure((size_t)nn * 8));
  HIPCHK(P.d_tp.ensure((size_t)nn * TOPK_M * 8));
  HIPCHK(P.d_cfeat.ensure((size_t)std::max<int64_t>(P.n_chunks, 1) * TOPK_CF * 4));
  HIPCHK(P.d_supf.ensure((size_t)std::max<int64_t>(P.n_super, 1) * TOPK_CF * 4));
  HIPCHK(P.d_probe.ensure((size_t)TOPK_NPROBE * KP * 2));
  const size_t tb = topk_sort_temp_bytes(T.n);
  HIPCHK(P.d_tmp.ensure(std::max<size_t>(tb, 16)));
  if (T.n > 0)
    HIPCHK(topk_prepare(KP, c->p.rank, T.d_orig.as<float>(), T.n, (float)P.tsc, P.d_VP.as<double>(), P.d_tmp.p, tb,
                        P.d_keys.as<uint32_t>(), P.d_perm.as<uint32_t>(), P.d_nperm.as<uint32_t>(),
                        P.d_tp.as<double>(), P.d_th.p, P.d_cfeat.as<float>(), P.d_supf.as<float>(), P.d_probe.p,
                        c->st));
  st("  plan: dst sort + fp16 pack + chunk features");
  HIPCHK(P.d_dstids.ensure(std::max<int64_t>(T.n, 1) * 4));
  HIPCHK(hipMemcpyAsync(P.d_dstids.p, T.ids.data(), T.n * 4, hipMemcpyHostToDevice, c->st));
  HIPCHK(P.d_scan.ensure(8));
  st("  plan: dst ids");
  return ALS_OK;
}

// Src rows per top-k pass: 2^25 (candidate lists 32 GiB of the 288 GB), or what half of the free
// device memory holds at ~1.5 KiB per src row (the TOPK_CAP-entry candidate list plus the row's
// features, order keys and output slots), so a smaller GPU or ranks sharing one fall back to more passes
int64_t topk_pass_rows(als_ctx* c) {
  size_t fr = 0, tot = 0;
  int64_t cap = (int64_t)1 << 25;
  if (set_device(c) == ALS_OK && hipMemGetInfo(&fr, &tot) == hipSuccess) {
    const int64_t fit = (int64_t)(fr / 2 / 1536);
    cap = std::min<int64_t>(cap, std::max<int64_t>((int64_t)1 << 16, fit & ~(int64_t)0xFFFF));
  }
  return cap;
}

// Rows per pass of a call: ALBEDO_TOPK_PASS (test knob, at least 65,536) or topk_pass_rows, which is
// one pass for any realistic row count.  halve > 0 (ALBEDO_TOPK_OVERLAP, no knob set): a call of
// `halve` rows runs as two passes.
int64_t topk_rows_per_pass(als_ctx* c, int64_t halve = 0) {
  const char* e = std::getenv("ALBEDO_TOPK_PASS");
  if (e && *e) return std::max<int64_t>(1 << 16, std::atoll(e));
  const int64_t cap = topk_pass_rows(c);
  return halve > 0 ? std::min<int64_t>(cap, (halve + 1) / 2) : cap;
}

// Rank r's contiguous slice [lo, hi) of n rows dealt to `world` ranks, per = ceil(n / world) rows each
struct RankSlice {
  int64_t per, lo, hi;
};
RankSlice rank_slice(int64_t n, int rank, int world) {
  const int64_t per = (n + world - 1) / world, lo = std::min<int64_t>(n, (int64_t)rank * per);
  return {per, lo, std::min<int64_t>(n, lo + per)};
}

// A call's top-k passes: topk_begin (n_rows positions, at most n_passes passes; the rescan flags of
// position p land in c->d_last_need[p]), topk_run_rows per pass, topk_finish (one synchronisation:
// timers and counters).
int topk_begin(als_ctx* c, TopkPlan& P, int64_t n_rows, int64_t n_passes, const int32_t* rows) {
  HIPCHK(P.d_scan.ensure((size_t)std::max<int64_t>(n_passes, 1) * 8));
  HIPCHK(hipMemsetAsync(P.d_scan.p, 0, (size_t)std::max<int64_t>(n_passes, 1) * 8, c->st));
  for (auto& B : P.pb) {
    HIPCHK(B.d_cnt.ensure(16));
    HIPCHK(hipMemsetAsync(B.d_cnt.p, 0, 16, c->st));
  }
  HIPCHK(c->d_last_need.ensure((size_t)std::max<int64_t>(n_rows, 1) * 4));
  HIPCHK(hipMemsetAsync(c->d_last_need.p, 0, (size_t)std::max<int64_t>(n_rows, 1) * 4, c->st));
  c->last_need_n = n_rows;
  c->last_src = P.src;
  c->last_rows_dense = rows == nullptr;
  if (rows) c->last_rows.assign(rows, rows + n_rows);
  else c->last_rows.clear();
  c->last_rescan.clear();
  c->last_rescan_ready = false;
  P.n_passes = n_passes;
  P.passes.clear();
  return ALS_OK;
}

int topk_finish(als_ctx* c, TopkPlan& P, hipStream_t sp = nullptr) {
  if (sp) HIPCHK(hipStreamSynchronize(sp));
  HIPCHK(hipStreamSynchronize(c->st));
  const int64_t np = (int64_t)P.passes.size();
  std::vector<unsigned long long> scanned((size_t)std::max<int64_t>(np, 1), 0ull);
  int cnt[4] = {0, 0, 0, 0}, cnt1[4] = {0, 0, 0, 0};
  if (np > 0) HIPCHK(copy_st(c, scanned.data(), P.d_scan.p, np * 8, hipMemcpyDeviceToHost));
  HIPCHK(copy_st(c, cnt, P.pb[0].d_cnt.p, 16, hipMemcpyDeviceToHost));
  HIPCHK(copy_st(c, cnt1, P.pb[1].d_cnt.p, 16, hipMemcpyDeviceToHost));
  cnt[2] += cnt1[2];
  for (int64_t q = 0; q < np; ++q) {
    const TopkPlan::PassRec& R = P.passes[q];
    const hipEvent_t* e = P.evs.data() + R.e0;
    c->topk_ms[0] += event_ms(e[0], e[1]);
    c->topk_ms[1] += event_ms(e[1], e[2]);
    for (int r = 0; r < R.ranges; ++r) {
      c->topk_ms[2] += event_ms(r == 0 ? e[2] : e[3 + 2 * r - 1], e[3 + 2 * r]);
      c->topk_ms[3] += event_ms(e[3 + 2 * r], e[4 + 2 * r]);
    }
    c->topk_stats[2] += (int64_t)scanned[q];
    c->topk_ms[4] += (double)scanned[q] * (R.rpw / 4) * 2.0 * c->KP;  // per wave: rpw / 4 src rows x each dst row
  }
  c->topk_stats[1] += cnt[2];
  return ALS_OK;
}

// One pass: the nc src rows `rows` (host, dense row indices; nullptr: rows row0 .. row0 + nc - 1,
// generated on the device) at positions pos0 .. pos0 + nc - 1 of the call, into the lists of `out`.
// Rows that fail certification are compacted on the device and re-scored by a persistent exact scan
// in the same stream: nothing here waits for the GPU.
using TopkReady = std::function<int(int64_t, int64_t)>;
// Where a pass's lists go and how they are finished
struct TopkPassOut {
  int32_t* ids = nullptr;      // device-visible lists [nc][k], score desc, id asc
  float* scores = nullptr;
  // after the scan the results are finished in output ranges of `range` rows (select, then the
  // rescans of the range); ready(o0, o1), when given, is called once a range's work is enqueued, so
  // the caller can copy those rows out while the next range computes
  int64_t range = INT64_MAX;
  TopkReady ready;
  // buffer set `set`; with a post stream the select / rescans wait for the scan on it, so the
  // caller's next pass (the other set) can order and scan meanwhile
  int set = 0;
  hipStream_t post = nullptr;
};
int topk_run_rows(als_ctx* c, TopkPlan& P, const int32_t* rows, int64_t row0, int64_t pos0, int64_t nc,
                  const TopkPassOut& out) {
  TopkPlan::PassBufs& B = P.pb[out.set];
  const int64_t range = out.range;
  const TopkReady& ready = out.ready;
  hipStream_t sp = out.post, ps = sp ? sp : c->st;
  Side& S = c->s[P.src];
  Side& T = c->s[1 - P.src];
  const int KP = c->KP, k = P.k;
  if (nc <= 0) return ALS_OK;
  HIPCHK(B.d_src.ensure(nc * 4));
  if (!P.exact_only) {
    HIPCHK(B.d_ls.ensure(nc * TOPK_CAP * 8));
    HIPCHK(B.d_lc.ensure(nc * 4));
  }
  if (rows) HIPCHK(hipMemcpyAsync(B.d_src.p, rows, nc * 4, hipMemcpyHostToDevice, c->st));
  else HIPCHK(launch_iota_i32(B.d_src.as<int32_t>(), nc, row0, c->st));
  TopkArgs a{};
  a.S = S.d_orig.as<float>();
  a.T = T.d_orig.as<float>();
  a.src_rows = B.d_src.as<int32_t>();
  a.n_src = nc;
  a.n_dst = T.n;
  a.dst_ids = P.d_dstids.as<int32_t>();
  a.kreal = c->p.rank;
  a.k = k;
  a.kt = topk_threshold_rank(k);
  a.tmax_norm = (float)(P.tmax * (1.0 + 1e-6));
  a.Th = P.d_th.p;
  a.perm = P.d_perm.as<uint32_t>();
  a.n_chunks = P.n_chunks;
  a.VP = P.d_VP.as<double>();
  a.cfeat = P.prune ? P.d_cfeat.as<float>() : nullptr;
  a.probe = P.d_probe.p;
  a.ssc = (float)P.ssc;
  a.tsc = (float)P.tsc;
  a.unscale = (float)(1.0 / (P.ssc * P.tsc));
  a.scaled = (float)(P.ssc * P.tsc);
  a.lent = B.d_ls.as<uint2>();
  a.lcnt = B.d_lc.as<int32_t>();
  // scan order: 12 bits of depth, then 7 / 7 / 6 bits of direction (topk_order_key_kernel; c4 all
  // users: scan 260 -> 193 ms, order + mask 56 -> 39 ms against the depth-only key; 18 / 22 / 24
  // direction bits 206 / 206 / 276 ms, other splits of 20 the same 193)
  a.order_dir_bits = 7 | (7 << 8) | (6 << 16);
  a.out_ids = out.ids;
  a.out_scores = out.scores;
  int32_t* d_need = c->d_last_need.as<int32_t>() + pos0;
  a.need_exact = d_need;
  if (!P.exact_only) {
    HIPCHK(B.d_kth.ensure(nc * 4));
    a.kth0 = B.d_kth.as<float>();
  }
  const int64_t pass = (int64_t)P.passes.size();
  if (pass >= P.n_passes) return fail(ALS_E_STATE, "top-k: more passes than planned");
  a.scanned = P.d_scan.as<unsigned long long>() + pass;
  if (P.exact_only) {
    HIPCHK(launch_topk_exact(KP, a, nullptr, nc, c->st));
    if (ready) TRYC(ready(0, nc));
    return ALS_OK;
  }
  const int64_t nr = std::max<int64_t>(1, (nc + range - 1) / range);  // output ranges
  const size_t e0 = P.evs.size();
  hipEvent_t ev[3];
  for (int i = 0; i < 3; ++i) HIPCHK(P.event(e0 + i, &ev[i]));
  // scan order: rows that stop at similar depths share a workgroup (topk_order); the select writes
  // each row's results back to its own slot
  TopkArgs b = a;
  HIPCHK(hipEventRecord(ev[0], c->st));
  HIPCHK(B.d_okeys.ensure(nc * 8));
  HIPCHK(B.d_order.ensure(nc * 8));
  HIPCHK(B.d_srcs.ensure(nc * 4));
  const size_t otb = topk_order_temp_bytes(nc);
  HIPCHK(B.d_otmp.ensure(std::max<size_t>(otb, 16)));
  HIPCHK(B.d_thr.ensure(nc * 8));
  HIPCHK(B.d_sf.ensure((size_t)nc * TOPK_SF * 8));
  float* sf_tmp = B.d_sf.as<float>();
  float* sf_sorted = sf_tmp + (size_t)nc * TOPK_SF;
  HIPCHK(topk_order(KP, a, B.d_otmp.p, otb, B.d_okeys.as<uint32_t>(), B.d_order.as<uint32_t>(), B.d_srcs.as<int32_t>(),
                    B.d_thr.as<float>(), B.d_thr.as<float>() + nc, sf_tmp, sf_sorted, c->st));
  b.src_rows = B.d_srcs.as<int32_t>();
  b.out_pos = B.d_order.as<uint32_t>();
  b.thr0 = B.d_thr.as<float>() + nc;
  b.sfeat = sf_sorted;
  const int rpw = topk_rows_per_workgroup(KP, nc, c->n_cu);
  if (P.prune) {  // per scan workgroup, the chunks its rows can need against the starting thresholds
    const int64_t n_wg = (nc + rpw - 1) / rpw;
    b.mask_words = (P.n_super + 1) / 2;
    HIPCHK(B.d_mask.ensure((size_t)n_wg * b.mask_words * 4));
    b.mask = B.d_mask.as<uint32_t>();
    HIPCHK(launch_topk_mask(b, rpw, P.d_supf.as<float>(), P.n_super, B.d_mask.as<uint32_t>(), c->st));
  }
  HIPCHK(hipEventRecord(ev[1], c->st));
  HIPCHK(launch_topk(KP, b, c->n_cu, c->st));
  HIPCHK(hipEventRecord(ev[2], c->st));
  HIPCHK(B.d_flag.ensure(nc * 4));
  if (nr > 1) HIPCHK(B.d_inv.ensure(nc * 4));
  if (sp) HIPCHK(hipStreamWaitEvent(sp, ev[2], 0));  // the select needs this pass's scan
  if (nr > 1) {  // select by output slot: slot -> scan position
    HIPCHK(launch_invert_perm(b.out_pos, nc, B.d_inv.as<uint32_t>(), ps));
  }
  P.passes.push_back(TopkPlan::PassRec{rpw, e0, 0});
  for (int64_t r = 0; r < nr; ++r) {
    const int64_t o0 = r * range, n = std::min<int64_t>(range, nc - o0);
    hipEvent_t es, ex;
    HIPCHK(P.event(e0 + 3 + 2 * r, &es));
    HIPCHK(P.event(e0 + 4 + 2 * r, &ex));
    TopkArgs bs = b;
    if (nr > 1) {
      bs.in_pos = B.d_inv.as<uint32_t>();
      bs.slot0 = o0;
      bs.n_slots = n;
    }
    HIPCHK(launch_topk_select(KP, bs, ps));
    HIPCHK(hipEventRecord(es, ps));
    // certification failures of the range: compacted on the device (range-local positions), re-scored
    // in place
    TopkArgs ar = a;
    ar.src_rows = a.src_rows + o0;
    ar.out_ids = a.out_ids + o0 * k;
    ar.out_scores = a.out_scores + o0 * k;
    ar.kth0 = a.kth0 + o0;
    ar.n_src = n;
    HIPCHK(hipMemsetAsync(B.d_cnt.p, 0, 8, ps));  // this range's count and work counter
    HIPCHK(launch_topk_exact_flagged(KP, ar, d_need + o0, n, B.d_flag.as<int32_t>(), B.d_cnt.as<int>(), c->n_cu, ps));
    HIPCHK(hipEventRecord(ex, ps));
    P.passes.back().ranges = (int)(r + 1);
    if (ready) TRYC(ready(o0, o0 + n));
  }
  c->topk_stats[0] += nc;
  c->topk_stats[3] += (nc + rpw - 1) / rpw * 4 * P.n_chunks * P.CH;  // dst rows x waves
  return ALS_OK;
}

// ---- a call's output ----------------------------------------------------------------------------

// The two host arrays a call writes, registered with HIP by a helper thread (so the plan runs
// meanwhile).  Joins the thread and unregisters when it goes.
struct HostPin {
  void* p[2] = {nullptr, nullptr};
  size_t bytes = 0;
  unsigned flags = 0;
  int state = 0;  // bit i: p[i] is registered (the helper thread's until wait())
  std::thread thr;
  HostPin() = default;
  HostPin(const HostPin&) = delete;
  HostPin& operator=(const HostPin&) = delete;
  ~HostPin() { release(); }
  void start(int dev, void* a, void* b, size_t nbytes, unsigned fl) {
    p[0] = a, p[1] = b, bytes = nbytes, flags = fl;
    auto pin = [this, dev]() {
      if (hipSetDevice(dev) != hipSuccess) return;
      if (hipHostRegister(p[0], bytes, flags) != hipSuccess) return;
      state |= 1;
      if (hipHostRegister(p[1], bytes, flags) == hipSuccess) state |= 2;
    };
    try {
      thr = std::thread(pin);
    } catch (const std::system_error&) {
      pin();  // no thread: pin here
    }
  }
  int wait() {  // for the helper thread: the state
    if (thr.joinable()) thr.join();
    return state;
  }
  void release() {
    wait();
    for (int i = 0; i < 2; ++i)
      if (state & (1 << i)) (void)hipHostUnregister(p[i]);
    state = 0;
  }
};

// How the lists of a call's known rows [lo, hi) (this rank's slice) reach the caller's arrays `ids` and
// `scores` ([nq][k]).  The passes ask it where their lists go (begin_pass) and hand them over
// (end_pass); when it goes it waits for its streams and for c->st, unregisters the arrays, and only
// then destroys its events, streams and buffers.
//   IN_PLACE  Zero-copy results (r06, default): the select / exact kernels write the lists straight
//             into the mapped caller arrays over PCIe.  The DMA pipeline moved the 4.8 GB of an
//             all-users c4 call at ~29 GB/s and finished ~110 ms after the last kernel; written in
//             place, the select runs at the link's rate with nothing behind it.  ALBEDO_TOPK_ZEROCOPY=2
//             (default) selects in output-slot ranges, so a workgroup's four lists leave as one block
//             of 16-B stores (c4 all users: DMA 0.339 s, mode 1 (scan order, the whole pass at once)
//             0.298-0.318 s, mode 2 0.291 s on the box that ran mode 1 at 0.318).
//   STAGED    ALBEDO_TOPK_ZEROCOPY=0, the DMA pipeline: two device buffer pairs across passes, each
//             finished range of a pass goes down on a copy stream while the next range computes.
//   SYNC      one device buffer pair, copied back after each pass: straight into the arrays when every
//             queried row is known, else row by row through `pos`.
// The asynchronous sinks need dense output of more than one range (every row of the side, the
// recommendForAll* case) and the arrays registered; whatever of their set-up fails, the next simpler
// sink runs and no error is raised.
struct TopkOutput {
  enum Mode { SYNC, STAGED, IN_PLACE };
  als_ctx* c;
  int32_t* ids;
  float* scores;
  int k;
  int64_t lo;
  const int64_t* pos;  // the output row of known row i (null: row i, the output is dense)
  int64_t range;       // rows per output range
  int zmode;           // ALBEDO_TOPK_ZEROCOPY
  Mode mode = SYNC;
  HostPin pin;
  int32_t* z_ids = nullptr;  // IN_PLACE: the device's view of ids + lo·k, scores + lo·k
  float* z_scores = nullptr;
  Stream copy, post;
  Event copied[2], posted[2];  // buffer set b: its copies are done / its last select and rescans are done
  std::deque<Event> finished;  // STAGED: one per finished range, the copy stream waits for it
  DevBuf d_ids[2], d_scores[2];

  TopkOutput(als_ctx* c_, int32_t* ids_, float* scores_, int k_, int64_t lo_, const int64_t* pos_, int64_t range_)
      : c(c_), ids(ids_), scores(scores_), k(k_), lo(lo_), pos(pos_), range(range_) {
    const char* e = std::getenv("ALBEDO_TOPK_ZEROCOPY");
    zmode = e ? std::atoi(e) : 2;
  }
  TopkOutput(const TopkOutput&) = delete;
  TopkOutput& operator=(const TopkOutput&) = delete;
  ~TopkOutput() {
    const bool registered = pin.wait() != 0;
    if (post.s) (void)hipStreamSynchronize(post.s);
    if (copy.s) (void)hipStreamSynchronize(copy.s);
    if (registered) (void)hipStreamSynchronize(c->st);
    pin.release();
  }
  bool wants_in_place() const { return zmode == 1 || zmode == 2; }

  // registers this rank's n rows of both arrays on a helper thread
  void start_pin(int64_t n) {
    pin.start(c->dev, ids + lo * k, scores + lo * k, (size_t)n * k * 4,
              wants_in_place() ? hipHostRegisterMapped : hipHostRegisterDefault);
  }

  // after the plan: the best sink whose set-up succeeds
  void choose(int64_t n_pass) {
    const bool registered = pin.wait() == 3;
    (void)hipGetLastError();  // a refused registration is not an error: the synchronous sink runs
    if (!registered) {
      pin.release();  // the ids alone
      return;
    }
    bool in_place = wants_in_place();
    if (in_place) {
      void* pi = nullptr;
      void* ps = nullptr;
      if (hipHostGetDevicePointer(&pi, pin.p[0], 0) == hipSuccess &&
          hipHostGetDevicePointer(&ps, pin.p[1], 0) == hipSuccess) {
        z_ids = static_cast<int32_t*>(pi);
        z_scores = static_cast<float*>(ps);
      } else {
        in_place = false;
        (void)hipGetLastError();
      }
    }
    // the copy stream and its events: one set-up for both asynchronous sinks (in place the stream stays
    // idle, and the post stream is the process's next one either way); without them: synchronous
    if (!(copy.create() && copied[0].create() && copied[1].create())) {
      for (Event& e : copied) e.reset();
      copy.reset();
      pin.release();
      (void)hipGetLastError();
      return;
    }
    mode = in_place ? IN_PLACE : STAGED;
    // Any in-place call of more than one pass runs its select and rescans on the post stream, with the
    // two buffer sets alternating, so that they overlap the next pass's order and scan
    // (ALBEDO_TOPK_OVERLAP=1 only makes two passes of a large one-pass call).  Measured slower on the
    // call that matters (c4 all users 0.318 vs 0.293 s, profiles/r06_bench_c4_topk_overlap_REJECTED
    // .json): the store-bound select waves slow the concurrent scan, and the second pass adds its own
    // order, sort and mask.  Without the stream or its events the passes stay sequential.
    const bool post_stream_passes = mode == IN_PLACE && n_pass > 1;
    if (post_stream_passes && !(post.create() && posted[0].create() && posted[1].create())) {
      for (Event& e : posted) e.reset();
      post.reset();
      (void)hipGetLastError();
    }
  }

  const char* name() const {  // ALBEDO_TOPK_TRACE
    switch (mode) {
      case IN_PLACE:
        if (zmode == 2) return post.s ? "pass: in place by slot ranges, post stream" : "pass: in place by slot ranges";
        return post.s ? "pass: in place in scan order, post stream" : "pass: in place in scan order";
      case STAGED: return "pass: staged copies";
      default: return pos ? "pass: synchronous scatter" : "pass: synchronous copy-back";
    }
  }

  // where pass `it` (nc known rows from q0) puts its lists
  int begin_pass(int64_t it, int64_t q0, int64_t nc, TopkPassOut& o) {
    const int b = (int)(it & 1);
    switch (mode) {
      case IN_PLACE:  // mode 2: select in output-slot order by ranges (consecutive waves write consecutive lists)
        o.ids = z_ids + (q0 - lo) * k;
        o.scores = z_scores + (q0 - lo) * k;
        o.range = zmode == 2 ? range : INT64_MAX;
        if (post.s) {  // buffer set b, reused once its previous select / rescans are done
          if (it >= 2 && hipStreamWaitEvent(c->st, posted[b].e, 0) != hipSuccess) return fail(ALS_E_HIP, "stream wait");
          o.set = b;
          o.post = post.s;
        }
        return ALS_OK;
      case STAGED:
        if (it >= 2 && hipStreamWaitEvent(c->st, copied[b].e, 0) != hipSuccess) return fail(ALS_E_HIP, "stream wait");
        if (d_ids[b].ensure(nc * k * 4) != hipSuccess || d_scores[b].ensure(nc * k * 4) != hipSuccess)
          return fail(ALS_E_OUT_OF_MEMORY, "top-k output buffers");
        o.ids = d_ids[b].as<int32_t>();
        o.scores = d_scores[b].as<float>();
        o.range = range;
        o.ready = [this, b, q0](int64_t o0, int64_t o1) { return copy_range(b, q0, o0, o1); };
        return ALS_OK;
      default:
        HIPCHK(d_ids[0].ensure(nc * k * 4));
        HIPCHK(d_scores[0].ensure(nc * k * 4));
        o.ids = d_ids[0].as<int32_t>();
        o.scores = d_scores[0].as<float>();
        return ALS_OK;
    }
  }

  // STAGED: rows [o0, o1) of the pass from q0 are enqueued on c->st; they go down on the copy stream
  int copy_range(int b, int64_t q0, int64_t o0, int64_t o1) {
    finished.emplace_back();
    Event& e = finished.back();
    if (!e.create()) return fail(ALS_E_HIP, "top-k copy event");
    const size_t nb = (size_t)(o1 - o0) * k * 4;
    if (hipEventRecord(e.e, c->st) != hipSuccess || hipStreamWaitEvent(copy.s, e.e, 0) != hipSuccess ||
        hipMemcpyAsync(ids + (q0 + o0) * k, d_ids[b].as<int32_t>() + o0 * k, nb, hipMemcpyDeviceToHost, copy.s) !=
            hipSuccess ||
        hipMemcpyAsync(scores + (q0 + o0) * k, d_scores[b].as<float>() + o0 * k, nb, hipMemcpyDeviceToHost, copy.s) !=
            hipSuccess)
      return fail(ALS_E_HIP, "top-k result copy");
    return ALS_OK;
  }

  // pass `it` is enqueued
  int end_pass(int64_t it, int64_t q0, int64_t nc) {
    const int b = (int)(it & 1);
    switch (mode) {
      case IN_PLACE:
        if (post.s && hipEventRecord(posted[b].e, post.s) != hipSuccess) return fail(ALS_E_HIP, "post event");
        return ALS_OK;
      case STAGED:
        if (hipEventRecord(copied[b].e, copy.s) != hipSuccess) return fail(ALS_E_HIP, "top-k result copy");
        return ALS_OK;
      default: break;
    }
    const size_t nb = (size_t)nc * k * 4;
    if (!pos) {
      HIPCHK(hipMemcpyAsync(ids + q0 * k, d_ids[0].p, nb, hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipMemcpyAsync(scores + q0 * k, d_scores[0].p, nb, hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipStreamSynchronize(c->st));
      return ALS_OK;
    }
    std::vector<int32_t> oid(nc * k);
    std::vector<float> osc(nc * k);
    HIPCHK(hipMemcpyAsync(oid.data(), d_ids[0].p, nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(osc.data(), d_scores[0].p, nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (int64_t i = 0; i < nc; ++i) {
      std::memcpy(ids + pos[q0 + i] * k, &oid[i * k], k * 4);
      std::memcpy(scores + pos[q0 + i] * k, &osc[i * k], k * 4);
    }
    return ALS_OK;
  }
};

// A subset's ids -> dense src rows: id -> row by a merge walk when ascending (the usual case), binary
// search otherwise.  known: the rows of the known ids, in subset order; pos: their output rows; the
// output rows of unknown ids are padded here.
void map_subset(const Side& S, const int32_t* subset, int64_t nq, int k, int32_t* ids_out, float* scores_out,
                std::vector<int32_t>& known, std::vector<int64_t>& pos) {
  std::vector<int32_t> qrow(nq);
  if (std::is_sorted(subset, subset + nq)) {
    int64_t r = 0;
    for (int64_t i = 0; i < nq; ++i) {
      while (r < S.n && S.ids[r] < subset[i]) ++r;
      qrow[i] = (r < S.n && S.ids[r] == subset[i]) ? (int32_t)r : -1;
    }
  } else {
    for (int64_t i = 0; i < nq; ++i) qrow[i] = (int32_t)find_row(S, subset[i]);
  }
  known.reserve(nq);
  pos.reserve(nq);
  for (int64_t i = 0; i < nq; ++i)
    if (qrow[i] >= 0) {
      known.push_back(qrow[i]);
      pos.push_back(i);
    } else {
      std::fill(ids_out + i * k, ids_out + (i + 1) * k, -1);
      std::fill(scores_out + i * k, scores_out + (i + 1) * k, NAN);
    }
}

// world > 1: every rank ends with every list -- one all-gather of the ranks' slices of the n known
// rows, a row's k ids and k scores travelling as one block of floats (pos: see TopkOutput)
int allgather_lists(als_ctx* c, int64_t n, int k, const int64_t* pos, int32_t* ids, float* scores) {
  const int64_t per = rank_slice(n, c->rank, c->world).per;
  if (per == 0) return ALS_OK;
  std::vector<float> blk((size_t)c->world * per * k * 2, 0.f);
  // rank r's block <- / -> the caller's arrays
  auto each_row = [&](int r, bool pack) {
    const RankSlice sl = rank_slice(n, r, c->world);
    float* bb = blk.data() + (size_t)r * per * k * 2;
    for (int64_t i = sl.lo; i < sl.hi; ++i) {
      float* rec = bb + (size_t)(i - sl.lo) * k * 2;
      int32_t* row_ids = ids + (pos ? pos[i] : i) * k;
      float* row_sc = scores + (pos ? pos[i] : i) * k;
      if (pack) std::memcpy(rec, row_ids, k * 4), std::memcpy(rec + k, row_sc, k * 4);
      else std::memcpy(row_ids, rec, k * 4), std::memcpy(row_sc, rec + k, k * 4);
    }
  };
  each_row(c->rank, true);
  TRYC(allgather_host(c, blk.data(), per * k * 2));
  for (int r = 0; r < c->world; ++r)
    if (r != c->rank) each_row(r, false);
  return ALS_OK;
}

// ---- als_recommend_unseen -------------------------------------------------------------------------

namespace {

// Stage marks on a stream, as many as the passes need
struct MarkList {
  std::vector<hipEvent_t> e;
  MarkList() = default;
  MarkList(const MarkList&) = delete;
  MarkList& operator=(const MarkList&) = delete;
  ~MarkList() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipError_t mark(hipStream_t s) {
    hipEvent_t x;
    const hipError_t r = hipEventCreate(&x);
    if (r != hipSuccess) return r;
    e.push_back(x);
    return hipEventRecord(x, s);
  }
};

// The depth of the filter's lists: ALBEDO_UNSEEN_DEPTH, else 48, clamped to [k, TOPK_KC].  A tuning choice:
// no result depends on it.  c2, all users, k = 30: the lists cost 9.7 ms of device time at 48 and 294 ms at
// 64, where the running threshold sits at the last place of the 64-entry candidate lists (topk_threshold_rank)
// and certification has no gap left; the 0.9 % of the rows that 48 sends to the exact scan cost 8.7 ms
// ("Recommendations without the known pairs", profiles/unseen_c2.json).
int unseen_depth(int k) {
  int d = 48;
  const char* e = std::getenv("ALBEDO_UNSEEN_DEPTH");
  if (e && *e) d = std::atoi(e);
  return std::max(k, std::min(TOPK_KC, d));
}

}  // namespace

// Tier 1: the certified top-`depth` lists of the existing passes, kept on the device and filtered there.
// Tier 2: the rows the filter cannot certify, through an exact scan that knows each row's exclusion range.
int recommend_unseen(als_ctx* c, int src, int k, const int32_t* subset, int64_t n_subset, int mode, int64_t n_excl,
                     const int32_t* excl_src, const int32_t* excl_dst, int32_t* src_ids_out, int32_t* ids_out,
                     float* scores_out) {
  TRYC(materialize(c, src));
  Side& S = c->s[src];
  Side& T = c->s[1 - src];
  hipStream_t st = c->st;
  const int KP = c->KP, depth = unseen_depth(k);
  const bool all_rows = subset == nullptr;
  const int64_t nq = all_rows ? S.n : n_subset;
  std::vector<int32_t> known;
  std::vector<int64_t> pos;
  if (!all_rows) map_subset(S, subset, nq, k, ids_out, scores_out, known, pos);
  if (src_ids_out && nq > 0) std::memcpy(src_ids_out, all_rows ? S.ids.data() : subset, (size_t)nq * 4);
  const int64_t n_known = all_rows ? nq : (int64_t)known.size();
  const int32_t* rows = all_rows ? nullptr : known.data();
  const int64_t* out_pos = n_known == nq ? nullptr : pos.data();
  c->last_rescan.clear();
  c->last_rescan_ready = true;
  c->unseen_stats[0] = n_known;
  if (n_known == 0) return ALS_OK;
  if (T.n == 0) {
    std::fill(ids_out, ids_out + nq * k, -1);
    std::fill(scores_out, scores_out + nq * k, NAN);
    return ALS_OK;
  }
  TopkPlan P;
  DevBuf d_es, d_ed, d_sids, d_key, d_keys, d_tmp, d_ptr, d_lid, d_lsc, d_flag, d_cnt, d_stat;
  MarkList clk;
  TopkOutput out(c, ids_out, scores_out, k, 0, out_pos, INT64_MAX);  // never pinned: the synchronous sink
  Drain queued{st};
  HIPCHK(clk.mark(st));  // 0
  TRYC(topk_plan(c, src, depth, P));
  HIPCHK(clk.mark(st));  // 1
  UnseenExcl x{};
  if (mode == ALS_EXCLUDE_RATINGS) {
    x.ptr = S.d_ptr.as<int64_t>();
    x.col = S.d_col.as<int32_t>();
  } else {
    HIPCHK(d_ptr.ensure((size_t)(S.n + 1) * 8));
    x.ptr = d_ptr.as<int64_t>();
    if (n_excl == 0) {
      HIPCHK(hipMemsetAsync(d_ptr.p, 0, (size_t)(S.n + 1) * 8, st));  // every range empty: nothing is looked up
    } else {
      const size_t tb = unseen_sort_temp_bytes(n_excl);
      HIPCHK(d_es.ensure((size_t)n_excl * 4));
      HIPCHK(d_ed.ensure((size_t)n_excl * 4));
      HIPCHK(d_sids.ensure((size_t)S.n * 4));
      HIPCHK(d_key.ensure((size_t)n_excl * 8));
      HIPCHK(d_keys.ensure((size_t)n_excl * 8));
      HIPCHK(d_tmp.ensure(std::max<size_t>(tb, 16)));
      HIPCHK(hipMemcpyAsync(d_es.p, excl_src, (size_t)n_excl * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_ed.p, excl_dst, (size_t)n_excl * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_sids.p, S.ids.data(), (size_t)S.n * 4, hipMemcpyHostToDevice, st));
      HIPCHK(unseen_pair_ranges(d_es.as<int32_t>(), d_ed.as<int32_t>(), n_excl, d_sids.as<int32_t>(), S.n,
                                P.d_dstids.as<int32_t>(), T.n, d_key.as<uint64_t>(), d_keys.as<uint64_t>(), d_tmp.p, tb,
                                d_ptr.as<int64_t>(), st));
      x.key = d_keys.as<uint64_t>();
    }
  }
  HIPCHK(clk.mark(st));  // 2
  HIPCHK(d_cnt.ensure(8));
  HIPCHK(d_stat.ensure(24));
  HIPCHK(hipMemsetAsync(d_stat.p, 0, 24, st));
  const int64_t chunk = topk_rows_per_pass(c);
  const int64_t n_pass = (n_known + chunk - 1) / chunk;
  TRYC(topk_begin(c, P, n_known, n_pass, rows));
  for (int64_t it = 0; it < n_pass; ++it) {  // marks 3 + 4·it ..: lists, filter, exact scan, copies
    const int64_t q0 = it * chunk, nc = std::min<int64_t>(chunk, n_known - q0);
    HIPCHK(d_lid.ensure((size_t)nc * depth * 4));
    HIPCHK(d_lsc.ensure((size_t)nc * depth * 4));
    HIPCHK(d_flag.ensure((size_t)nc * 4));
    TopkPassOut lists;
    lists.ids = d_lid.as<int32_t>();
    lists.scores = d_lsc.as<float>();
    TRYC(topk_run_rows(c, P, rows ? rows + q0 : nullptr, q0, q0, nc, lists));
    HIPCHK(clk.mark(st));
    TopkPassOut o;
    TRYC(out.begin_pass(0, q0, nc, o));
    const int32_t* src_rows = P.pb[0].d_src.as<int32_t>();
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, 8, st));
    HIPCHK(launch_unseen_filter(d_lid.as<int32_t>(), d_lsc.as<float>(), depth, k, nc, T.n, src_rows,
                                P.d_dstids.as<int32_t>(), x, o.ids, o.scores, d_flag.as<int32_t>(), d_cnt.as<int>(),
                                d_stat.as<unsigned long long>(), st));
    HIPCHK(clk.mark(st));
    TopkArgs a{};
    a.S = S.d_orig.as<float>();
    a.T = T.d_orig.as<float>();
    a.src_rows = src_rows;
    a.n_src = nc;
    a.n_dst = T.n;
    a.dst_ids = P.d_dstids.as<int32_t>();
    a.kreal = c->p.rank;
    a.k = k;
    a.tmax_norm = (float)(P.tmax * (1.0 + 1e-6));
    a.perm = P.d_perm.as<uint32_t>();
    a.n_chunks = P.n_chunks;
    a.VP = P.d_VP.as<double>();
    a.cfeat = P.prune ? P.d_cfeat.as<float>() : nullptr;
    a.out_ids = o.ids;
    a.out_scores = o.scores;
    HIPCHK(launch_unseen_exact(KP, a, x, d_flag.as<int32_t>(), d_cnt.as<int>(), d_stat.as<unsigned long long>() + 1, nc,
                               c->n_cu, st));
    HIPCHK(clk.mark(st));
    TRYC(out.end_pass(0, q0, nc));
    HIPCHK(clk.mark(st));
  }
  TRYC(topk_finish(c, P));
  unsigned long long stat[3] = {0, 0, 0};
  HIPCHK(copy_st(c, stat, d_stat.p, 24, hipMemcpyDeviceToHost));
  c->unseen_stats[1] = (int64_t)stat[2];
  c->unseen_stats[2] = (int64_t)stat[0];
  c->unseen_stats[3] = (int64_t)stat[1];
  const std::vector<hipEvent_t>& e = clk.e;
  c->unseen_ms[0] = mode == ALS_EXCLUDE_PAIRS && n_excl > 0 ? event_ms(e[1], e[2]) : 0.0;
  c->unseen_ms[1] = event_ms(e[0], e[1]);
  for (int64_t it = 0; it < n_pass; ++it) {
    const hipEvent_t* m = e.data() + 3 + 4 * it;
    c->unseen_ms[1] += event_ms(m[-1], m[0]);
    c->unseen_ms[2] += event_ms(m[0], m[1]);
    c->unseen_ms[3] += event_ms(m[1], m[2]);
  }
  c->unseen_ms[4] = event_ms(e.front(), e.back());
  return ALS_OK;
}

}  // namespace albedo

using namespace albedo;

extern "C" {

int als_recommend_unseen(als_ctx* c, int side, int32_t k, const int32_t* subset, int64_t n_subset, int32_t mode,
                         int64_t n_excl, const int32_t* excl_src, const int32_t* excl_dst, int32_t* src_ids_out,
                         int32_t* dst_ids_out, float* scores_out) {
  if (!c || (side != 0 && side != 1) || !dst_ids_out || !scores_out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (mode != ALS_EXCLUDE_RATINGS && mode != ALS_EXCLUDE_PAIRS)
    return fail(ALS_E_INVALID_ARGUMENT, "als_recommend_unseen: unknown exclusion mode " + std::to_string(mode));
  if (k < 1) return fail(ALS_E_INVALID_ARGUMENT, "num must be positive");
  if ((subset && n_subset < 0) || n_excl < 0)
    return fail(ALS_E_INVALID_ARGUMENT, "als_recommend_unseen: a count is negative");
  if (mode == ALS_EXCLUDE_PAIRS && n_excl > 0 && (!excl_src || !excl_dst))
    return fail(ALS_E_INVALID_ARGUMENT, "als_recommend_unseen: null exclusion pairs with n_excl > 0");
  if (k > TOPK_KC)
    return fail(ALS_E_UNSUPPORTED, "als_recommend_unseen keeps at most " + std::to_string(TOPK_KC) + " rows per list (k <= 64)");
  if (c->world > 1) return fail(ALS_E_UNSUPPORTED, "als_recommend_unseen is single-process (world = 1)");
  if (mode == ALS_EXCLUDE_PAIRS && n_excl > (int64_t)0x7FFFFFFF)
    return fail(ALS_E_UNSUPPORTED, "als_recommend_unseen takes at most 2^31 - 1 exclusion pairs a call");
  for (int s = 0; s < 2; ++s)
    if (!c->s[s].has_factors)
      return fail(ALS_E_STATE, std::string("als_recommend_unseen needs the ") + (s == ALS_USER ? "user" : "item") +
                                   " factors (fit, inject or load them first)");
  if (mode == ALS_EXCLUDE_RATINGS && (!c->has_ratings || c->model_only))
    return fail(ALS_E_STATE,
                "als_recommend_unseen: this context holds no ratings to exclude (a loaded model); pass the known pairs "
                "(ALS_EXCLUDE_PAIRS)");
  TRYC(set_device(c));
  for (int64_t& v : c->unseen_stats) v = 0;
  for (double& v : c->unseen_ms) v = 0.0;
  return recommend_unseen(c, side, k, subset, n_subset, mode, mode == ALS_EXCLUDE_PAIRS ? n_excl : 0, excl_src, excl_dst,
                          src_ids_out, dst_ids_out, scores_out);
}

int als_recommend_unseen_stats(const als_ctx* c, int64_t* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->unseen_stats[i];
  return ALS_OK;
}

int als_recommend_unseen_timing(const als_ctx* c, double* out5) {
  if (!c || !out5) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 5; ++i) out5[i] = c->unseen_ms[i];
  return ALS_OK;
}

int als_recommend(als_ctx* c, int side, int32_t k, const int32_t* subset, int64_t n_subset, int32_t* src_ids_out,
                  int32_t* dst_ids_out, float* scores_out) {
  if (!c || (side != 0 && side != 1) || !dst_ids_out || !scores_out)
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (k <= 0) return fail(ALS_E_INVALID_ARGUMENT, "num must be positive");
  if (k > TOPK_MAX)
    return fail(ALS_E_UNSUPPORTED, "num above " + std::to_string(TOPK_MAX) + " is not supported by this engine");
  TRYC(set_device(c));
  // ALBEDO_TOPK_TRACE (diagnostic): wall-clock stamps of the call's phases on stderr, the stream
  // synchronised at each (so the stamps bracket device work); each pass's stamp names its output sink
  static const bool trace = [] {
    const char* e = std::getenv("ALBEDO_TOPK_TRACE");
    return e && *e && *e != '0';
  }();
  const auto t_start = std::chrono::steady_clock::now();
  auto stamp = [&](const char* what) {
    if (!trace) return;
    (void)hipStreamSynchronize(c->st);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    std::fprintf(stderr, "[topk] %9.2f ms  %s\n", ms, what);
  };
  const int src = side;
  TRYC(materialize(c, src));
  stamp("materialize src");
  Side& S = c->s[src];
  const Side& T = c->s[1 - src];
  const int64_t nq = subset ? n_subset : S.n;
  // recommendForAll*: every src row, in row order -- no host index arrays (the device generates the
  // row indices of each pass); a subset: its known ids' rows, unknown ids padded
  const bool all_rows = subset == nullptr;
  std::vector<int32_t> known;
  std::vector<int64_t> pos;
  if (!all_rows) map_subset(S, subset, nq, k, dst_ids_out, scores_out, known, pos);
  if (src_ids_out) std::memcpy(src_ids_out, all_rows ? S.ids.data() : subset, (size_t)nq * 4);
  const int64_t n_known = all_rows ? nq : (int64_t)known.size();
  const int32_t* rows = all_rows ? nullptr : known.data();
  const int64_t* out_pos = n_known == nq ? nullptr : pos.data();  // null: results land in place, no scatter
  c->last_rescan.clear();
  c->last_rescan_ready = true;
  if (n_known == 0 || T.n == 0) return ALS_OK;
  stamp("host id mapping");
  // world > 1 (SURVEY §8(e) "Top-k: shard users"): rank r scores the r-th contiguous slice of the
  // known src rows against the replicated dst factors; the lists are all-gathered afterwards
  const RankSlice sl = rank_slice(n_known, c->rank, c->world);
  const int64_t n_here = sl.hi - sl.lo;
  // Src rows per pass: up to 2^25 (candidate lists 32 GiB of the 288 GB).  One scan launch over every
  // row dispatches the heaviest workgroups (lowest relative thresholds) first and fills in behind
  // them; split into 4M-row passes, each pass paid its own heavy tail (c4 all users: scan 436 ms in
  // five passes, 260 ms in one; profiles/r05_bench_c4_topk_pass{4M,10M,20M}.json).  The results are
  // finished and copied out in ranges of pass / 8 rows (at most 4M) while the next range computes.
  // ALBEDO_TOPK_OVERLAP=1 (r06 experiment): a call of >= 2M rows runs as two passes, see
  // TopkOutput::choose for what more than one pass means in place.
  const bool want_overlap = [] {
    const char* e = std::getenv("ALBEDO_TOPK_OVERLAP");
    return e && std::atoi(e) == 1;
  }();
  const int64_t chunk = topk_rows_per_pass(c, want_overlap && n_here >= ((int64_t)1 << 21) ? n_here : 0);
  const int64_t range = std::min<int64_t>((int64_t)1 << 22, std::max<int64_t>(chunk / 8, 1 << 16));
  const int64_t n_pass = (n_here + chunk - 1) / chunk;
  TopkPlan P;  // outlives the output sink, which waits for the streams that use the plan's buffers
  {
    TopkOutput out(c, dst_ids_out, scores_out, k, sl.lo, out_pos, range);
    if (!out_pos && n_here > range) out.start_pin(n_here);  // while the plan runs
    TRYC(topk_plan(c, src, k, P, trace ? std::function<void(const char*)>(stamp) : nullptr));
    out.pin.wait();
    stamp("plan (materialize dst, Gram + host eig, dst sort + fp16 pack) + pin the output arrays");
    out.choose(n_pass);
    TRYC(topk_begin(c, P, n_known, n_pass, rows));
    for (int64_t it = 0; it < n_pass; ++it) {
      const int64_t q0 = sl.lo + it * chunk, nc = std::min<int64_t>(chunk, sl.hi - q0);
      TopkPassOut o;
      TRYC(out.begin_pass(it, q0, nc, o));
      TRYC(topk_run_rows(c, P, rows ? rows + q0 : nullptr, q0, q0, nc, o));
      TRYC(out.end_pass(it, q0, nc));
      stamp(out.name());
    }
    TRYC(topk_finish(c, P, out.post.s));
  }
  stamp("last copies + unpin");
  if (c->world > 1) TRYC(allgather_lists(c, n_known, k, out_pos, dst_ids_out, scores_out));
  return ALS_OK;
}

// RankingEvaluator.evaluate of the users' own top-k lists: als_evaluate_ndcg (metric = ALS_METRIC_NDCG, through
// eval_ndcg) and als_evaluate_ranking (Precision@k and MAP through eval_metric)
static int evaluate_topk_lists(als_ctx* c, int32_t metric, int32_t k, int64_t n, const int32_t* user, const int32_t* item,
                               const int64_t* key, double* ndcg_out, int64_t* n_users_out, int32_t* users_out,
                               double* per_user_out, int64_t cap) {
  if (!c || !ndcg_out || !n_users_out || (n > 0 && (!user || !item || !key)))
    return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (k <= 0) return fail(ALS_E_INVALID_ARGUMENT, "ranking position k should be positive");
  if (k > TOPK_KC) return fail(ALS_E_UNSUPPORTED, "NDCG@k on the device supports k <= " + std::to_string(TOPK_KC));
  TRYC(set_device(c));
  TRYC(materialize(c, ALS_USER));
  Side& S = c->s[ALS_USER];
  *ndcg_out = NAN;
  *n_users_out = 0;
  c->last_rescan.clear();
  c->last_rescan_ready = true;
  if (n <= 0 || S.n == 0) return ALS_OK;
  hipStream_t st = c->st;
  // 1. intoUserActualItems on the device: group by model user (inner join), top-k by (key desc, item asc)
  DevBuf d_user, d_item, d_key, d_ids, d_row, d_rows, d_idx, d_idxs, d_runs, d_cnt, d_off, d_nr, d_tmp;
  HIPCHK(d_user.ensure(n * 4));
  HIPCHK(d_item.ensure(n * 4));
  HIPCHK(d_key.ensure(n * 8));
  HIPCHK(d_ids.ensure(S.n * 4));
  HIPCHK(hipMemcpyAsync(d_user.p, user, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_item.p, item, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_key.p, key, n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ids.p, S.ids.data(), S.n * 4, hipMemcpyHostToDevice, st));
  for (DevBuf* b : {&d_row, &d_rows, &d_idx, &d_idxs, &d_runs, &d_cnt}) HIPCHK(b->ensure(n * 4));
  HIPCHK(d_off.ensure(n * 8));
  HIPCHK(d_nr.ensure(8));
  const size_t tb = eval_sort_temp_bytes(n);
  HIPCHK(d_tmp.ensure(std::max<size_t>(tb, 16)));
  HIPCHK(eval_group_users(d_user.as<int32_t>(), n, d_ids.as<int32_t>(), S.n, d_tmp.p, tb, d_row.as<uint32_t>(),
                          d_rows.as<uint32_t>(), d_idx.as<uint32_t>(), d_idxs.as<uint32_t>(), d_runs.as<uint32_t>(),
                          d_cnt.as<int32_t>(), d_off.as<int64_t>(), d_nr.as<int64_t>(), st));
  int64_t nr = 0;
  HIPCHK(hipMemcpyAsync(&nr, d_nr.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int32_t> rows(nr);
  HIPCHK(hipMemcpyAsync(rows.data(), d_runs.p, nr * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (nr > 0 && (uint32_t)rows[nr - 1] == 0xFFFFFFFFu) --nr;  // ids unknown to the model: dropped
  rows.resize(nr);
  *n_users_out = nr;
  if (nr == 0) return ALS_OK;
  DevBuf d_act, d_actn, d_gain, d_vals;
  HIPCHK(d_act.ensure(nr * k * 4));
  HIPCHK(d_actn.ensure(nr * 4));
  HIPCHK(eval_actual_lists(d_idxs.as<uint32_t>(), d_off.as<int64_t>(), d_cnt.as<int32_t>(), nr, d_key.as<int64_t>(),
                           d_item.as<int32_t>(), k, d_act.as<int32_t>(), d_actn.as<int32_t>(), st));
  // ndcgAt's gains from the host's libm: the host evaluator's table (1.0 / math.log(i + 2))
  std::vector<double> gain(k);
  for (int i = 0; i < k; ++i) gain[i] = 1.0 / std::log((double)(i + 2));
  HIPCHK(d_gain.ensure(k * 8));
  HIPCHK(hipMemcpyAsync(d_gain.p, gain.data(), k * 8, hipMemcpyHostToDevice, st));
  HIPCHK(d_vals.ensure(nr * 8));
  // 2. intoUserPredictedItems: the users' top-k lists stay on the device; 3. ndcgAt per user
  TopkPlan P;
  TRYC(topk_plan(c, ALS_USER, k, P));
  const RankSlice sl = rank_slice(nr, c->rank, c->world);
  const int64_t per_rank = sl.per, lo = sl.lo, hi = sl.hi;
  const int64_t chunk = topk_rows_per_pass(c);
  DevBuf d_oid, d_osc;
  TRYC(topk_begin(c, P, nr, (hi - lo + chunk - 1) / chunk, rows.data()));
  for (int64_t q0 = lo; q0 < hi; q0 += chunk) {
    const int64_t nc = std::min<int64_t>(chunk, hi - q0);
    HIPCHK(d_oid.ensure(nc * k * 4));
    HIPCHK(d_osc.ensure(nc * k * 4));
    TopkPassOut o;
    o.ids = d_oid.as<int32_t>();
    o.scores = d_osc.as<float>();
    TRYC(topk_run_rows(c, P, rows.data() + q0, 0, q0, nc, o));
    if (metric == ALS_METRIC_NDCG)
      HIPCHK(eval_ndcg(d_oid.as<int32_t>(), d_act.as<int32_t>() + q0 * k, d_actn.as<int32_t>() + q0, nc, k,
                       c->s[ALS_ITEM].n, d_gain.as<double>(), d_vals.as<double>() + q0, st));
    else
      HIPCHK(eval_metric(metric, d_oid.as<int32_t>(), k, nullptr, (int)std::min<int64_t>(k, c->s[ALS_ITEM].n), nullptr,
                         d_act.as<int32_t>() + q0 * k, d_actn.as<int32_t>() + q0, nullptr, nc, k, d_gain.as<double>(),
                         d_vals.as<double>() + q0, st));
  }
  TRYC(topk_finish(c, P));
  std::vector<double> vals((size_t)std::max<int64_t>(per_rank, 1) * c->world, 0.0);
  if (hi > lo)
    HIPCHK(hipMemcpyAsync(vals.data() + (size_t)c->rank * per_rank, d_vals.as<double>() + lo, (hi - lo) * 8,
                          hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c->world > 1) TRYC(allgather_host(c, reinterpret_cast<float*>(vals.data()), per_rank * 2));
  double sum = 0.0;  // mean over users in ascending id order (RankingMetrics: RDD mean)
  for (int64_t i = 0; i < nr; ++i) sum += vals[i];
  *ndcg_out = sum / (double)nr;
  if (nr <= cap) {
    if (users_out)
      for (int64_t i = 0; i < nr; ++i) users_out[i] = S.ids[rows[i]];
    if (per_user_out) std::memcpy(per_user_out, vals.data(), nr * 8);
  }
  return ALS_OK;
}

int als_evaluate_ndcg(als_ctx* c, int32_t k, int64_t n, const int32_t* user, const int32_t* item, const int64_t* key,
                      double* ndcg_out, int64_t* n_users_out, int32_t* users_out, double* per_user_out, int64_t cap) {
  return evaluate_topk_lists(c, ALS_METRIC_NDCG, k, n, user, item, key, ndcg_out, n_users_out, users_out, per_user_out,
                             cap);
}

int als_evaluate_ranking(als_ctx* c, int32_t metric, int32_t k, int64_t n, const int32_t* user, const int32_t* item,
                         const int64_t* key, double* mean_out, int64_t* n_users_out, int32_t* users_out,
                         double* per_user_out, int64_t cap) {
  if (metric != ALS_METRIC_NDCG && metric != ALS_METRIC_PRECISION && metric != ALS_METRIC_MAP)
    return fail(ALS_E_INVALID_ARGUMENT, "unknown metric " + std::to_string(metric));
  return evaluate_topk_lists(c, metric, k, n, user, item, key, mean_out, n_users_out, users_out, per_user_out, cap);
}

int als_topk_stats(const als_ctx* c, int64_t* out4) {
  if (!c || !out4) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 4; ++i) out4[i] = c->topk_stats[i];
  return ALS_OK;
}

int als_topk_timing(const als_ctx* c, double* out5) {
  if (!c || !out5) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  for (int i = 0; i < 5; ++i) out5[i] = c->topk_ms[i];
  return ALS_OK;
}

int als_topk_last_rescan(const als_ctx* c, int32_t* src_ids_out, int64_t cap, int64_t* n_out) {
  if (!c || !n_out) return fail(ALS_E_INVALID_ARGUMENT, "bad args");
  if (!c->last_rescan_ready) {  // first query after a top-k call: read its device flags
    TRYC(set_device(const_cast<als_ctx*>(c)));
    std::vector<int32_t> need((size_t)c->last_need_n);
    if (c->last_need_n > 0) {
      HIPCHK(hipStreamSynchronize(c->st));
      HIPCHK(copy_st(c, need.data(), c->d_last_need.p, need.size() * 4, hipMemcpyDeviceToHost));
    }
    const Side& S = c->s[c->last_src];
    c->last_rescan.clear();
    const int64_t nrow = (int64_t)S.ids.size();
    for (int64_t p = 0; p < c->last_need_n; ++p) {
      if (!need[p]) continue;
      const int64_t r = c->last_rows_dense ? p : (p < (int64_t)c->last_rows.size() ? c->last_rows[p] : -1);
      if (r < 0 || r >= nrow) return fail(ALS_E_STATE, "top-k rescan flags out of range of the src rows");
      c->last_rescan.push_back(S.ids[r]);
    }
    c->last_rescan_ready = true;
  }
  *n_out = (int64_t)c->last_rescan.size();
  if (src_ids_out && *n_out <= cap) std::memcpy(src_ids_out, c->last_rescan.data(), c->last_rescan.size() * 4);
  return ALS_OK;
}

}  // extern "C"
