// als_recommend_vectors: exact top-k of caller-supplied query vectors against one side's factors, with an
// optional exclusion list per query (include/albedo_als.h).  Every listed row is scored with the F2J sdot
// (fp32 products added left to right, multiply and add rounded separately), the best k are kept in
// (score desc, row asc) order; NaN scores are never listed.
//
// Written like audit.hip and foldin.hip: a path beside the tuned one (topk.hip) that must not disturb, or
// depend on, it.  Plain HIP, no inline asm, no MFMA, none of device_common.h; the id search and the grid
// helper are id_front.h's.
//
//   query_excl_key_kernel  raw exclusion ids to dst rows by binary search; key (query << 32 | row), row
//                          0xFFFFFFFF for an id the model does not know.  One 64-bit radix sort then leaves
//                          every query's range ascending and still delimited by excl_ptr.
//   query_scan_kernel      work item = (dst slice, tile of QT_Q = 16 queries), grid-stride.  The queries sit in
//                          LDS as [column][query]; the slice goes through LDS QT_ROWS = 256 rows x QT_COLS = 32
//                          columns at a time (coalesced 16-byte loads, row stride 33 floats so that the thread
//                          of row r reads bank r + c).  A thread scores one row against the 16 queries,
//                          accumulators in registers.  The scores of a tile then go through LDS to the wave
//                          that owns the query (four queries a wave): it keeps the query's list sorted, one
//                          entry per lane, and looks only at scores that beat the k-th entry.  Such a score is
//                          searched in the query's exclusion range and inserted with one shuffle.  The kept
//                          set is fixed by the total order, whatever the order of arrival.
//   query_merge_kernel     one wave per query: the slice partials [slice][query][k] through the same list.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "id_front.h"
#include "kernels.h"

namespace albedo {

namespace {

constexpr uint32_t QT_NOROW = 0xFFFFFFFFu;
constexpr int QT_ROWS = 256, QT_COLS = 32, QT_LD = QT_COLS + 1, QT_WAVES = QT_ROWS / 64;
constexpr int QT_QW = QT_Q / QT_WAVES;  // queries a wave owns
constexpr int QT_MERGE_AHEAD = 8;       // 64-entry loads of the merge in flight
static_assert(QT_Q % QT_WAVES == 0 && QT_Q % 4 == 0, "query tile and waves do not match");
static_assert(QT_Q * QT_ROWS <= QT_ROWS * QT_LD, "the scores of a tile take the place of the tile");

__global__ void query_excl_key_kernel(const int64_t* __restrict__ excl_ptr, int64_t n_q, const int32_t* __restrict__ excl_ids,
                                      int64_t n_e, const int32_t* __restrict__ ids, int64_t n_ids,
                                      uint64_t* __restrict__ key) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n_q;  // the query whose range holds i: the last q with excl_ptr[q] <= i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (excl_ptr[mid + 1] <= i) lo = mid + 1;
      else hi = mid;
    }
    const int64_t r = find_id(ids, n_ids, excl_ids[i]);
    key[i] = ((uint64_t)lo << 32) | (r >= 0 ? (uint32_t)r : QT_NOROW);
  }
}

// a ranks above b under (score desc, row asc); -0.0 and +0.0 tie
__device__ __forceinline__ bool ranks_above(float sa, uint32_t ra, float sb, uint32_t rb) {
  return sa > sb || (sa == sb && ra < rb);
}

// v of lane `i`, the same i in every lane: a register read, where __shfl goes through the LDS crossbar
__device__ __forceinline__ float lane_value(float v, int i) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(i)));
}
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int i) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(i));
}

// One wave, every lane active.  The list (ls, lr) holds its i-th best entry in lane i, len <= k of them.  Each
// lane offers one (s, r) when `valid`; an offer that beats the k-th entry (or finds the list short) is looked
// up in the ascending exclusion range ex[e0, e1) (low halves of the keys) and inserted.  Lowest lane first.
__device__ __forceinline__ void wave_offer(float s, uint32_t r, bool valid, int k, float& ls, uint32_t& lr, int& len,
                                           const uint64_t* __restrict__ ex, int64_t e0, int64_t e1) {
  const int lane = threadIdx.x & 63;
  for (;;) {
    const float ts = lane_value(ls, k - 1);
    const uint32_t tr = lane_value(lr, k - 1);
    const bool pass = valid && (len < k || ranks_above(s, r, ts, tr));
    const unsigned long long m = __ballot(pass);
    if (!m) break;
    const int src = __ffsll((long long)m) - 1;
    const float cs = lane_value(s, src);
    const uint32_t cr = lane_value(r, src);
    if (lane == src) valid = false;
    int64_t lo = e0, hi = e1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint32_t)ex[mid] < cr) lo = mid + 1;
      else hi = mid;
    }
    if (lo < e1 && (uint32_t)ex[lo] == cr) continue;  // excluded
    const bool above = lane < len && ranks_above(ls, lr, cs, cr);
    const int pos = __popcll(__ballot(above));  // < k: the offer beat the k-th entry or the list is short
    const float us = __shfl_up(ls, 1);
    const uint32_t ur = (uint32_t)__shfl_up((int)lr, 1);
    if (lane > pos) {
      ls = us;
      lr = ur;
    } else if (lane == pos) {
      ls = cs;
      lr = cr;
    }
    if (len < k) ++len;
  }
}

struct ScanArgs {
  const float* Y;        // [n][KP] dst factors, original basis
  int64_t n;
  int KP, rank, k;
  const float* q;        // [n_q][rank]
  int64_t n_q;
  const int64_t* eptr;   // [n_q + 1] or null
  const uint64_t* ekey;  // sorted exclusion keys
  int64_t slice_rows, n_slices, n_qtiles;
  float* ps;             // [n_slices][n_q][k]
  uint32_t* pr;
};

__global__ __launch_bounds__(QT_ROWS) void query_scan_kernel(const ScanArgs a) {
#pragma clang fp contract(off)  // the F2J score has no fused product (hipcc contracts by default, __fmul_rn included)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tile = smem;                    // [QT_ROWS][QT_LD], then the scores [QT_Q][QT_ROWS]
  float* qs = smem + QT_ROWS * QT_LD;    // [rank][QT_Q]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KP = a.KP, rank = a.rank, k = a.k;
  const int64_t n_work = a.n_slices * a.n_qtiles;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const int64_t slice = w / a.n_qtiles, q0 = (w % a.n_qtiles) * QT_Q;
    const int64_t r0 = slice * a.slice_rows, r1 = r0 + a.slice_rows < a.n ? r0 + a.slice_rows : a.n;
    __syncthreads();  // the previous item's readers of qs are done
    for (int e = tid; e < rank * QT_Q; e += QT_ROWS) {
      const int c = e / QT_Q, j = e % QT_Q;
      qs[e] = q0 + j < a.n_q ? a.q[(q0 + j) * rank + c] : 0.f;
    }
    float ls[QT_QW];
    uint32_t lr[QT_QW];
    int len[QT_QW];
    int64_t e0[QT_QW], e1[QT_QW];
#pragma unroll
    for (int u = 0; u < QT_QW; ++u) {
      ls[u] = 0.f;
      lr[u] = QT_NOROW;
      len[u] = 0;
      const int64_t qi = q0 + wave * QT_QW + u;
      e0[u] = a.eptr && qi < a.n_q ? a.eptr[qi] : 0;
      e1[u] = a.eptr && qi < a.n_q ? a.eptr[qi + 1] : 0;
    }
    for (int64_t t0 = r0; t0 < r1; t0 += QT_ROWS) {
      float acc[QT_Q];
#pragma unroll
      for (int j = 0; j < QT_Q; ++j) acc[j] = 0.f;
      for (int c0 = 0; c0 < rank; c0 += QT_COLS) {
        float4 v[QT_COLS / 4];
#pragma unroll
        for (int u = 0; u < QT_COLS / 4; ++u) {
          const int e = tid + u * QT_ROWS, r = e / (QT_COLS / 4), c4 = e % (QT_COLS / 4);
          v[u] = t0 + r < r1 ? *reinterpret_cast<const float4*>(a.Y + (t0 + r) * KP + c0 + 4 * c4)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();  // the previous block of columns (or the previous tile's scores) is read
#pragma unroll
        for (int u = 0; u < QT_COLS / 4; ++u) {
          const int e = tid + u * QT_ROWS, r = e / (QT_COLS / 4), c4 = e % (QT_COLS / 4);
          float* d = tile + r * QT_LD + 4 * c4;
          d[0] = v[u].x;
          d[1] = v[u].y;
          d[2] = v[u].z;
          d[3] = v[u].w;
        }
        __syncthreads();
        const int ce = rank - c0 < QT_COLS ? rank - c0 : QT_COLS;
        const float* tr = tile + tid * QT_LD;
        for (int c = 0; c < ce; ++c) {
          const float t = tr[c];
          const float4* qc = reinterpret_cast<const float4*>(qs + (c0 + c) * QT_Q);
#pragma unroll
          for (int j4 = 0; j4 < QT_Q / 4; ++j4) {
            const float4 qv = qc[j4];
            acc[4 * j4 + 0] = acc[4 * j4 + 0] + qv.x * t;
            acc[4 * j4 + 1] = acc[4 * j4 + 1] + qv.y * t;
            acc[4 * j4 + 2] = acc[4 * j4 + 2] + qv.z * t;
            acc[4 * j4 + 3] = acc[4 * j4 + 3] + qv.w * t;
          }
        }
      }
      __syncthreads();  // the last block of columns is read: the scores take its place
#pragma unroll
      for (int j = 0; j < QT_Q; ++j) tile[j * QT_ROWS + tid] = acc[j];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < QT_QW; ++u) {
        const int j = wave * QT_QW + u;
        if (q0 + j >= a.n_q) continue;  // uniform over the wave
        for (int b = 0; b < QT_ROWS; b += 64) {
          if (t0 + b >= r1) break;
          const float s = tile[j * QT_ROWS + b + lane];
          const int64_t row = t0 + b + lane;
          wave_offer(s, (uint32_t)row, row < r1 && !(s != s), k, ls[u], lr[u], len[u], a.ekey, e0[u], e1[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < QT_QW; ++u) {
      const int64_t qi = q0 + wave * QT_QW + u;
      if (qi >= a.n_q || lane >= k) continue;
      const int64_t o = (slice * a.n_q + qi) * k + lane;
      a.ps[o] = lane < len[u] ? ls[u] : 0.f;
      a.pr[o] = lane < len[u] ? lr[u] : QT_NOROW;
    }
  }
}

__global__ __launch_bounds__(256) void query_merge_kernel(const float* __restrict__ ps, const uint32_t* __restrict__ pr,
                                                          int64_t n_slices, int64_t n_q, int k,
                                                          const int32_t* __restrict__ ids, int32_t* __restrict__ ids_out,
                                                          float* __restrict__ scores_out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t qi = wave0; qi < n_q; qi += n_waves) {
    float ls = 0.f;
    uint32_t lr = QT_NOROW;
    int len = 0;
    const int64_t total = n_slices * k;
    for (int64_t f0 = 0; f0 < total; f0 += 64 * QT_MERGE_AHEAD) {
      float s[QT_MERGE_AHEAD];  // every load of the step is issued before the first entry is looked at
      uint32_t r[QT_MERGE_AHEAD];
#pragma unroll
      for (int u = 0; u < QT_MERGE_AHEAD; ++u) {
        const int64_t f = f0 + 64 * u + lane;
        s[u] = 0.f;
        r[u] = QT_NOROW;
        if (f < total) {
          const int64_t o = ((f / k) * n_q + qi) * k + f % k;
          s[u] = ps[o];
          r[u] = pr[o];
        }
      }
#pragma unroll
      for (int u = 0; u < QT_MERGE_AHEAD; ++u)
        wave_offer(s[u], r[u], r[u] != QT_NOROW, k, ls, lr, len, nullptr, 0, 0);
    }
    if (lane < k) {
      ids_out[qi * k + lane] = lane < len ? ids[lr] : -1;
      scores_out[qi * k + lane] = lane < len ? ls : __int_as_float(0x7FC00000);
    }
  }
}

}  // namespace

size_t query_sort_temp_bytes(int64_t n_e) { return sort_keys64_temp_bytes(n_e); }

hipError_t query_map_exclusions(const int64_t* excl_ptr, int64_t n_q, const int32_t* excl_ids, int64_t n_e,
                                const int32_t* dst_ids, int64_t n_dst, uint64_t* key, uint64_t* key_sorted, void* temp,
                                size_t temp_bytes, hipStream_t s) {
  if (n_e <= 0) return hipSuccess;
  if (n_e > (int64_t)0x7FFFFFFF || n_q <= 0 || n_q > (int64_t)0x7FFFFFFF || n_dst >= (int64_t)QT_NOROW)
    return hipErrorInvalidValue;
  query_excl_key_kernel<<<front_grid(n_e), 256, 0, s>>>(excl_ptr, n_q, excl_ids, n_e, dst_ids, n_dst, key);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t tb = temp_bytes;
  return rocprim::radix_sort_keys(temp, tb, key, key_sorted, (size_t)n_e, 0, 64, s);
}

// About two workgroups per CU over slices x query tiles; a slice is a whole number of 256-row tiles
QueryPlan query_plan(int64_t n_dst, int64_t n_q, int n_cu) {
  QueryPlan p{};
  p.n_qtiles = (n_q + QT_Q - 1) / QT_Q;
  const int64_t want = std::max<int64_t>(1, (2 * (int64_t)std::max(n_cu, 1) + p.n_qtiles - 1) / std::max<int64_t>(p.n_qtiles, 1));
  int64_t rows = (std::max<int64_t>(n_dst, 1) + want - 1) / want;
  rows = (rows + QT_ROWS - 1) / QT_ROWS * QT_ROWS;
  const char* e = std::getenv("ALBEDO_QUERY_SLICE_ROWS");
  if (e && *e && std::atoll(e) > 0) rows = std::atoll(e);
  p.slice_rows = rows;
  p.n_slices = std::max<int64_t>(1, (n_dst + rows - 1) / rows);
  return p;
}

hipError_t launch_query_scan(int KP, int rank, const float* Y, int64_t n_dst, const float* q, int64_t n_q, int k,
                             const int64_t* excl_ptr, const uint64_t* excl_key, const QueryPlan& p, float* part_score,
                             uint32_t* part_row, int n_cu, hipStream_t s) {
  if (n_q <= 0) return hipSuccess;
  if (k < 1 || k > 64 || rank < 1 || rank > KP || KP % QT_COLS || n_dst < 0 || n_dst >= (int64_t)QT_NOROW ||
      p.slice_rows < 1 || p.n_slices < 1 || p.n_slices * p.slice_rows < n_dst || p.n_qtiles * QT_Q < n_q)
    return hipErrorInvalidValue;
  ScanArgs a{};
  a.Y = Y;
  a.n = n_dst;
  a.KP = KP;
  a.rank = rank;
  a.k = k;
  a.q = q;
  a.n_q = n_q;
  a.eptr = excl_ptr;
  a.ekey = excl_key;
  a.slice_rows = p.slice_rows;
  a.n_slices = p.n_slices;
  a.n_qtiles = p.n_qtiles;
  a.ps = part_score;
  a.pr = part_row;
  const size_t lds = (size_t)(QT_ROWS * QT_LD + rank * QT_Q) * 4;
  const int64_t n_work = p.n_slices * p.n_qtiles;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_work, 8 * (int64_t)std::max(n_cu, 1)));
  query_scan_kernel<<<grid, QT_ROWS, lds, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_query_merge(const float* part_score, const uint32_t* part_row, int64_t n_slices, int64_t n_q, int k,
                              const int32_t* dst_ids, int32_t* ids_out, float* scores_out, hipStream_t s) {
  if (n_q <= 0) return hipSuccess;
  if (k < 1 || k > 64 || n_slices < 1) return hipErrorInvalidValue;
  query_merge_kernel<<<front_grid(n_q * 64), 256, 0, s>>>(part_score, part_row, n_slices, n_q, k, dst_ids, ids_out,
                                                          scores_out);
  return hipGetLastError();
}

}  // namespace albedo
