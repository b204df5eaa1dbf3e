// Held-out pair ranking on the device: RankingMetricFormatter("als") of ALSModel.transform(pairs) with
// coldStartStrategy = "drop" (albedo ALSRecommenderCV.scala:54-90, RankingMetricFormatter.scala:59-64,
// RankingEvaluator.scala:131-139), and the three metrics of RankingEvaluator (:21, :97-101) on lists of
// per-user length.
//
//  map     raw (user, item) -> dense rows by binary search over the ascending id tables; a pair with an
//          unknown user or item gets the key n_users, which sorts behind every user and is never scored
//  group   radix sort of (user row, item row) by the user row (only the bits n_users needs), run-length
//          encode, exclusive scan: the sequence of eval_group_users
//  score   one flat pass over the sorted pairs, a wave per 64 consecutive pairs: both rows of a pair
//          arrive in 32-column blocks, eight lanes per row with 16-B loads, through the wave's LDS stage
//          (topk.hip's f2j_dot_rows with a row per lane on both sides); each lane then walks its pair in
//          F2J order (product, then add, left to right, no contraction: f2j_dot_v4's value).  Consecutive
//          pairs share the user, so its row comes from cache.  Writes 8 B per pair: score bits, raw item.
//  select  one wave per user streams its entries in rounds of 64 through a wave bitonic merge on one
//          64-bit key (score order, then item ascending); a NaN score is an empty slot (Spark's "drop" on
//          the prediction).  m = #entries with rank() <= top_k (score >= the top_k-th largest: ties at
//          the boundary all stay), the list is the first min(width, m) entries.  A user with more than
//          PAIRS_SEG entries is cut into segments of PAIRS_SEG, one wave each, whose best 64 are merged by one
//          more wave: the degree head (10^5 and more) never runs on a single wave.
//  metric  one wave per evaluated user: ndcgAt / precisionAt / meanAveragePrecision of mllib 2.2.0 in
//          fp64, in index order, on a predicted list of its own length.
//
// An F2J sum starts from +0.0f, so it is never -0.0f (x + (-x) and +0 + -0 round to +0): the order key
// still folds the two zeros together, and a score is recovered from its key.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <algorithm>
#include <cstdint>
#include "device_common.h"
#include "id_front.h"
#include "kernels.h"

namespace albedo {
namespace {

__global__ void ep_map_kernel(const int32_t* __restrict__ user, const int32_t* __restrict__ item, int64_t n,
                              const int32_t* __restrict__ uids, int64_t n_u, const int32_t* __restrict__ iids,
                              int64_t n_i, uint32_t* __restrict__ urow, uint32_t* __restrict__ irow) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = find_id(uids, n_u, user[i]);
    const int64_t v = find_id(iids, n_i, item[i]);
    const bool live = u >= 0 && v >= 0;
    urow[i] = live ? (uint32_t)u : (uint32_t)n_u;  // cold start "drop": behind every user, never scored
    irow[i] = live ? (uint32_t)v : 0u;
  }
}

constexpr int EP_LD = 36;  // LDS row stride: the b128 reads of 16 consecutive rows hit 16 distinct bank groups

// sorted pairs [0, n_live): ent[p] = {bits of F2J(U[urow[p]], V[irow[p]]), raw item id}
template <int KP>
__global__ __launch_bounds__(128) void ep_score_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                       const uint32_t* __restrict__ urow,
                                                       const uint32_t* __restrict__ irow,
                                                       const int32_t* __restrict__ iids, int64_t n_live, int kreal,
                                                       uint2* __restrict__ ent) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float s_stage[2][2 * 64 * EP_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u8 = lane & 7;
  float* su = s_stage[wave];
  float* sv = su + 64 * EP_LD;
  const int64_t n_tiles = (n_live + 63) / 64;
  for (int64_t t = (int64_t)blockIdx.x * 2 + wave; t < n_tiles; t += (int64_t)gridDim.x * 2) {
    const int64_t p = t * 64 + lane;
    const bool in = p < n_live;
    const int ur = in ? (int)urow[p] : -1;
    const int ir = in ? (int)irow[p] : -1;
    int um[8], im[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      um[m] = __shfl(ur, (lane >> 3) + 8 * m);
      im[m] = __shfl(ir, (lane >> 3) + 8 * m);
    }
    float acc = 0.f;
    const float* tu = su + lane * EP_LD;
    const float* tv = sv + lane * EP_LD;
    for (int cb = 0; cb < kreal; cb += 32) {
      f32x4 a[8], b[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        a[m] = um[m] >= 0 ? ld4(U + (int64_t)um[m] * KP + cb + 4 * u8) : zero4();
        b[m] = im[m] >= 0 ? ld4(V + (int64_t)im[m] * KP + cb + 4 * u8) : zero4();
      }
      WAVE_LDS_SYNC();  // the previous block's reads are done
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        *reinterpret_cast<f32x4*>(su + ((lane >> 3) + 8 * m) * EP_LD + 4 * u8) = a[m];
        *reinterpret_cast<f32x4*>(sv + ((lane >> 3) + 8 * m) * EP_LD + 4 * u8) = b[m];
      }
      WAVE_LDS_SYNC();
      const int ce = kreal - cb < 32 ? kreal - cb : 32;
      if (ce == 32) {
#pragma unroll
        for (int c = 0; c < 32; c += 4) {
          const f32x4 x = ld4(tu + c), y = ld4(tv + c);
          const float p0 = x[0] * y[0], p1 = x[1] * y[1], p2 = x[2] * y[2], p3 = x[3] * y[3];
          acc = acc + p0;
          acc = acc + p1;
          acc = acc + p2;
          acc = acc + p3;
        }
      } else {
        for (int c = 0; c < ce; ++c) {
          const float pr = tu[c] * tv[c];
          acc = acc + pr;
        }
      }
    }
    if (in) ent[p] = make_uint2(__float_as_uint(acc), (uint32_t)iids[ir]);
  }
}

// One order key per entry, larger = earlier in (score desc, item asc): the score's order-preserving
// image (the two zeros folded, IEEE order otherwise, -inf -> 0x007FFFFF) above the complement of the
// item's.  0 is no entry's key: the empty slot, behind every entry; a NaN score maps to it.
__device__ __forceinline__ uint64_t ep_key(uint2 e) {
  const float f = __uint_as_float(e.x);
  if (f != f) return 0ull;
  uint32_t b = f == 0.f ? 0u : e.x;
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint32_t)~(e.y ^ 0x80000000u);
}
__device__ __forceinline__ float ep_key_score(uint64_t k) {
  const uint32_t b = (uint32_t)(k >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b);
}
__device__ __forceinline__ int32_t ep_key_item(uint64_t k) { return (int32_t)(~(uint32_t)k ^ 0x80000000u); }

// wave bitonic sort of 128 keys, 2 per lane (element e = lane + 64h), descending
__device__ __forceinline__ void ep_bitonic128(uint64_t (&ky)[2]) {
  const int lane = threadIdx.x & 63;
  for (int K = 2; K <= 128; K <<= 1) {
    for (int J = K >> 1; J > 0; J >>= 1) {
      if (J == 64) {  // across the two registers of a lane; K = 128: always "up"
        if (ky[1] > ky[0]) {
          const uint64_t t = ky[0];
          ky[0] = ky[1];
          ky[1] = t;
        }
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = lane + 64 * h;
          const uint64_t o = __shfl_xor(ky[h], J);
          const bool lower = (lane & J) == 0;
          const bool up = (e & K) == 0;
          if ((lower == up) ? (o > ky[h]) : (o < ky[h])) ky[h] = o;
        }
      }
    }
  }
}

// One wave per work item w: the best 64 keys of cnt[w] inputs from off[w] (KEYS: keys of an earlier
// launch; else entries), descending.  PARTIAL: the 64 keys go to keys_out[w][64] (a segment of a long
// user).  Otherwise the list of output row dst[w] (or w) is written: the first min(width, m) of them.
template <bool KEYS, bool PARTIAL>
__global__ __launch_bounds__(256) void ep_select_kernel(const uint2* __restrict__ ent, const uint64_t* __restrict__ keys_in,
                                                        const int64_t* __restrict__ off, const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ dst, int64_t n_work, int max_direct,
                                                        int top_k, int width, uint64_t* __restrict__ keys_out,
                                                        int32_t* __restrict__ items, float* __restrict__ scores,
                                                        int32_t* __restrict__ len) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_work) return;
  const int64_t o = off[w];
  const int n = cnt[w];
  if (!KEYS && !PARTIAL && n > max_direct) return;  // a long user: its segments and their merge write the row
  uint64_t ky[2] = {0ull, 0ull};
  for (int b = 0; b < n; b += 64) {  // kept best 64 in slot 0, the next 64 inputs in slot 1
    const int e = b + lane;
    if (e < n) ky[1] = KEYS ? keys_in[o + e] : ep_key(ent[o + e]);
    else ky[1] = 0ull;
    ep_bitonic128(ky);
  }
  if (PARTIAL) {
    keys_out[w * 64 + lane] = ky[0];
    return;
  }
  const int64_t r = dst ? dst[w] : w;
  const bool live = ky[0] != 0ull;
  const int n_live = __popcll(__ballot(live));  // of the best 64
  int m = n_live;
  if (n_live >= top_k) {  // rank() <= top_k: score >= the top_k-th largest
    const uint32_t thr = (uint32_t)(__shfl(ky[0], top_k - 1) >> 32);
    m = __popcll(__ballot(live && (uint32_t)(ky[0] >> 32) >= thr));
  }
  m = min(m, width);
  if (lane < width) {
    items[r * width + lane] = lane < m ? ep_key_item(ky[0]) : -1;
    scores[r * width + lane] = lane < m ? ep_key_score(ky[0]) : __uint_as_float(0x7FC00000u);
  }
  if (lane == 0) len[r] = m;
}

// one wave per evaluated user u: the metric of predicted list prow[u] (length plen, or np for every user)
// against actual list arow[u]
__global__ __launch_bounds__(256) void ep_metric_kernel(int metric, const int32_t* __restrict__ pred, int pw,
                                                       const int32_t* __restrict__ plen, int np_all,
                                                       const int32_t* __restrict__ prow, const int32_t* __restrict__ act,
                                                       const int32_t* __restrict__ act_n,
                                                       const int32_t* __restrict__ arow, int64_t n_users, int k,
                                                       const double* __restrict__ gain, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int64_t pr = prow ? prow[u] : u, ar = arow ? arow[u] : u;
  const int np = min(plen ? plen[pr] : np_all, k);  // evaluate's slice(0, k)
  const int32_t p = lane < np ? pred[pr * pw + lane] : -1;
  const int nl = act_n[ar];
  const int32_t lab = lane < nl ? act[ar * k + lane] : -1;
  bool hit = false, dup = false;
  for (int j = 0; j < nl; ++j) {
    const int32_t v = __shfl(lab, j);
    hit |= (lane < np && p == v);  // -1 is a valid raw id: only the position tells padding
    dup |= (j < lane && v == lab);
  }
  const int ns = __popcll(__ballot(lane < nl && !dup));  // |labSet|
  const uint64_t hits = __ballot(hit);
  if (lane == 0) {
    double v = 0.0;
    if (ns > 0) {
      if (metric == 0) {  // ndcgAt
        const int n = min(max(np, ns), k);
        double dcg = 0.0, mx = 0.0;
        for (int i = 0; i < n; ++i) {
          if (i < np && ((hits >> i) & 1)) dcg += gain[i];
          if (i < ns) mx += gain[i];
        }
        v = dcg / mx;
      } else if (metric == 1) {  // precisionAt
        v = (double)__popcll(hits) / (double)k;
      } else {  // meanAveragePrecision
        int h = 0;
        double prec = 0.0;
        for (int i = 0; i < np; ++i)
          if ((hits >> i) & 1) {
            ++h;
            prec += (double)h / ((double)i + 1.0);
          }
        v = prec / (double)ns;
      }
    }
    out[u] = v;
  }
}

int ep_key_bits(int64_t n_u) {  // bits of the largest sort key, n_u
  int b = 1;
  while (b < 32 && ((int64_t)1 << b) <= n_u) ++b;
  return b;
}

}  // namespace

size_t pairs_sort_temp_bytes(int64_t n, int64_t n_users) {
  size_t a = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)n, 0, ep_key_bits(n_users), (hipStream_t)0);
  return std::max(a, group_temp_bytes<false, false>(n));
}

hipError_t pairs_map(const int32_t* user, const int32_t* item, int64_t n, const int32_t* uids, int64_t n_u,
                     const int32_t* iids, int64_t n_i, uint32_t* urow, uint32_t* irow, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n_u >= (int64_t)0xFFFFFFFF) return hipErrorInvalidValue;
  ep_map_kernel<<<front_grid(n), 256, 0, s>>>(user, item, n, uids, n_u, iids, n_i, urow, irow);
  return hipGetLastError();
}

hipError_t pairs_group(int64_t n, int64_t n_u, void* temp, size_t temp_bytes, const uint32_t* urow,
                       uint32_t* urow_sorted, const uint32_t* irow, uint32_t* irow_sorted, uint32_t* runs,
                       int32_t* counts, int64_t* offsets, int64_t* n_runs, int64_t* n_runs_host, hipStream_t s) {
  size_t tb = temp_bytes;
  hipError_t e = rocprim::radix_sort_pairs(temp, tb, urow, urow_sorted, irow, irow_sorted, (size_t)n, 0,
                                           ep_key_bits(n_u), s);
  if (e != hipSuccess) return e;
  return group_runs<false>(temp, temp_bytes, urow_sorted, n, runs, counts, offsets, n_runs, n_runs_host, s);
}

hipError_t pairs_score(int KP, int kreal, const float* U, const float* V, const uint32_t* urow_sorted,
                       const uint32_t* irow_sorted, const int32_t* iids, int64_t n_live, uint2* ent, hipStream_t s) {
  if (n_live <= 0) return hipSuccess;
  const int grid = front_grid((n_live + 63) / 64, 2);
  switch (KP) {
    case 64: ep_score_kernel<64><<<grid, 128, 0, s>>>(U, V, urow_sorted, irow_sorted, iids, n_live, kreal, ent); break;
    case 128: ep_score_kernel<128><<<grid, 128, 0, s>>>(U, V, urow_sorted, irow_sorted, iids, n_live, kreal, ent); break;
    case 256: ep_score_kernel<256><<<grid, 128, 0, s>>>(U, V, urow_sorted, irow_sorted, iids, n_live, kreal, ent); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

namespace {
template <bool KEYS, bool PARTIAL>
hipError_t ep_select_launch(const uint2* ent, const uint64_t* keys_in, const int64_t* off, const int32_t* cnt,
                            const int32_t* dst, int64_t n_work, int top_k, int width, uint64_t* keys_out, int32_t* items,
                            float* scores, int32_t* len, hipStream_t s) {
  for (int64_t w0 = 0; w0 < n_work; w0 += max_rows_per_launch(64)) {
    const int64_t nw = std::min<int64_t>(n_work - w0, max_rows_per_launch(64));
    // direct launches write row w (dst == null): the row pointers move with w0
    const bool direct = !KEYS && !PARTIAL;
    ep_select_kernel<KEYS, PARTIAL><<<(int)((nw + 3) / 4), 256, 0, s>>>(
        ent, keys_in, off + w0, cnt + w0, dst ? dst + w0 : nullptr, nw, PAIRS_SEG, top_k, width,
        PARTIAL ? keys_out + w0 * 64 : nullptr, direct ? items + w0 * width : items, direct ? scores + w0 * width : scores,
        direct ? len + w0 : len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace

hipError_t pairs_select(const uint2* ent, const int64_t* offsets, const int32_t* counts, int64_t n_runs, int top_k,
                        int width, int32_t* items, float* scores, int32_t* len, hipStream_t s) {
  if (n_runs <= 0) return hipSuccess;
  if (top_k < 1 || top_k > 64 || width < 1 || width > 64) return hipErrorInvalidValue;
  return ep_select_launch<false, false>(ent, nullptr, offsets, counts, nullptr, n_runs, top_k, width, nullptr, items,
                                        scores, len, s);
}

hipError_t pairs_select_long(const uint2* ent, const int64_t* seg_off, const int32_t* seg_cnt, int64_t n_seg,
                             uint64_t* seg_keys, const int64_t* key_off, const int32_t* key_cnt, const int32_t* run,
                             int64_t n_long, int top_k, int width, int32_t* items, float* scores, int32_t* len,
                             hipStream_t s) {
  if (n_long <= 0) return hipSuccess;
  if (top_k < 1 || top_k > 64 || width < 1 || width > 64) return hipErrorInvalidValue;
  hipError_t e = ep_select_launch<false, true>(ent, nullptr, seg_off, seg_cnt, nullptr, n_seg, top_k, width, seg_keys,
                                               nullptr, nullptr, nullptr, s);
  if (e != hipSuccess) return e;
  return ep_select_launch<true, false>(nullptr, seg_keys, key_off, key_cnt, run, n_long, top_k, width, nullptr, items,
                                       scores, len, s);
}

hipError_t eval_metric(int metric, const int32_t* pred, int pred_width, const int32_t* pred_len, int np_all,
                       const int32_t* pred_row, const int32_t* act, const int32_t* act_n, const int32_t* act_row,
                       int64_t n_users, int k, const double* gain, double* out, hipStream_t s) {
  if (n_users <= 0) return hipSuccess;
  if (k < 1 || k > 64 || metric < 0 || metric > 2 || pred_width < 1 || pred_width > 64) return hipErrorInvalidValue;
  for (int64_t u0 = 0; u0 < n_users; u0 += max_rows_per_launch(64)) {
    const int64_t nu = std::min<int64_t>(n_users - u0, max_rows_per_launch(64));
    // without row maps user u reads list u: the list pointers move with u0
    ep_metric_kernel<<<(int)((nu + 3) / 4), 256, 0, s>>>(
        metric, pred_row ? pred : pred + u0 * pred_width, pred_width, pred_len ? (pred_row ? pred_len : pred_len + u0) : nullptr,
        np_all, pred_row ? pred_row + u0 : nullptr, act_row ? act : act + u0 * k, act_row ? act_n : act_n + u0,
        act_row ? act_row + u0 : nullptr, nu, k, gain, out + u0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace albedo
