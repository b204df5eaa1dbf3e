// als_explain: how much each rating of a fold-in row contributes to the row's score for a target
// (include/albedo_als.h).  With A_j = G + Σ_i c_i y_i y_iᵀ + λ n_j I the row's system (foldin.hip) and y_t the
// target's factor, the score is linear in the ratings:
//   s_jt = y_tᵀ A_j⁻¹ Σ_i w_i y_i = Σ_i e_i,   e_i = w_i · y_iᵀ z_t,   z_t = A_j⁻¹ y_t.
//
// Written like foldin.hip and audit.hip: plain HIP, no inline asm, no MFMA, none of device_common.h, the
// factors in the original basis and everything fp64 from the first product on, at the model rank.
//
//   explain_pair_kernel .. explain_deg_kernel   the pairs over the fold-in's CSR: row ids to CSR rows and target
//                      ids to src rows by binary search, one 64-bit radix sort on (CSR row, input position), run
//                      lengths: every row that a valid pair names, its range of pairs, these rows by descending degree
//   explain_kernel     one workgroup per listed row, persistent over the degree-ordered list.
//     build, factor    the fold-in's own sections (fold_front.h): L is left in the packed triangle (LDS at
//                      KP <= 128, the workgroup's slab of global scratch at KP = 256), 1 / diag(L) in LDS.
//     then EXPLAIN_TB of the row's targets at a time:
//     solve   L u = y_t and Lᵀ z = u for the whole batch, column by column: the threads are spread over
//             (target, row) and keep their entries in registers; the owner of entry j leaves it in LDS once it
//             is final (two alternating buffers), so one barrier per column serves every target, and each
//             entry is updated by one thread in column order.  A target's z is the same bits wherever it
//             stands in a batch; the unused places of a batch are solved as zeros.
//     score   the row's src rows are read again, FOLD_TILE ratings at a time, straight from global memory (the
//             triangle holds the tile's LDS; the rows are in L2 from the build): thread (rating, target) sums
//             y_i[m]·z_t[m] in ascending m and scales by w_i.  The FOLD_TILE x EXPLAIN_TB values go through LDS
//     select  to the wave that owns the target: it keeps the target's list sorted, one entry per lane, by
//             (value desc, src row asc), looks only at the ratings that rank above the m-th entry, inserts
//             those with one shuffle each, and adds the total in CSR order.  The src rows ascend with their
//             raw ids, so the row decides a tie as the id would.
//   Nothing per (rating, pair) reaches global memory; the outputs are written once per pair, at its input slot.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "fold_front.h"
#include "id_front.h"
#include "kernels.h"

namespace albedo {

namespace {

__global__ void explain_pair_kernel(const int32_t* __restrict__ pair_row, const int32_t* __restrict__ pair_target,
                                    int64_t n_pairs, const int32_t* __restrict__ row_ids, int64_t n_rows,
                                    const int32_t* __restrict__ src_ids, int64_t n_src, uint64_t* __restrict__ key,
                                    uint32_t* __restrict__ target) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t rv = pair_row[p], tv = pair_target[p];
    const int64_t r = lower_bound_id(row_ids, n_rows, rv), t = lower_bound_id(src_ids, n_src, tv);
    const bool ok = r < n_rows && row_ids[r] == rv && t < n_src && src_ids[t] == tv;
    target[p] = ok ? (uint32_t)t : EXPLAIN_NONE;
    key[p] = ((uint64_t)(ok ? (uint32_t)r : EXPLAIN_NONE) << 32) | (uint32_t)p;
  }
}

__global__ void explain_deg_kernel(const uint32_t* __restrict__ runs, int64_t n_runs, const uint32_t* __restrict__ row_deg,
                                   uint32_t* __restrict__ deg, int32_t* __restrict__ iota) {
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n_runs; u += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = runs[u];
    deg[u] = r == EXPLAIN_NONE ? 0u : row_deg[r];
    iota[u] = (int32_t)u;
  }
}

__global__ void explain_fill_kernel(int64_t n_pairs, int64_t n_entries, double* __restrict__ total,
                                    int32_t* __restrict__ ids, double* __restrict__ contrib) {
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_entries; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n_pairs) total[i] = nan;
    ids[i] = -1;
    contrib[i] = nan;
  }
}

// One wave, every lane active: lane i holds the i-th entry of a list sorted by (value desc, row asc); row < 0
// marks an empty place (value NaN).  The candidate goes behind every entry that ranks above it or equals it (a
// copy of a pair is an entry of its own); a candidate past the m-th place is dropped.  -0.0 == +0.0: they tie.
__device__ __forceinline__ void explain_insert(double& lv, int& lr, const double e, const int r, const int m,
                                               const int lane) {
  const bool above = lr >= 0 && !(e > lv || (e == lv && r < lr));
  const int pos = __popcll(__ballot(above));
  if (pos >= m) return;  // uniform
  const double uv = __shfl_up(lv, 1);
  const int ur = __shfl_up(lr, 1);
  if (lane > pos) {
    lv = uv;
    lr = ur;
  } else if (lane == pos) {
    lv = e;
    lr = r;
  }
}

__device__ __forceinline__ int explain_lane_int(int v, int i) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(i));
}
__device__ __forceinline__ double explain_lane_double(double v, int i) {
  return __hiloint2double(explain_lane_int(__double2hiint(v), i), explain_lane_int(__double2loint(v), i));
}

// Each lane offers one (e, r) when `valid`.  Only the offers that rank above the m-th entry (or find the list
// short) are inserted, lowest lane first: once a list holds its best m, most of a tile passes with one ballot.
// The kept set is fixed by the total order, whatever the order of arrival.
__device__ __forceinline__ void explain_offer(double& lv, int& lr, const double e, const int r, bool valid, const int m,
                                              const int lane) {
  for (;;) {
    const double kv = explain_lane_double(lv, m - 1);
    const int kr = explain_lane_int(lr, m - 1);
    const unsigned long long pass = __ballot(valid && (kr < 0 || e > kv || (e == kv && r < kr)));
    if (!pass) break;
    const int src = __ffsll((long long)pass) - 1;
    explain_insert(lv, lr, explain_lane_double(e, src), explain_lane_int(r, src), m, lane);
    if (lane == src) valid = false;
  }
}

template <int KP, int TS, bool TRI_LDS>
__global__ __launch_bounds__(TS* TS) void explain_kernel(const ExplainArgs g) {
  constexpr int NT = TS * TS, NB = KP / TS, NW = NT / 64, TB = EXPLAIN_TB;
  constexpr int TPW = (TB + NW - 1) / NW;  // lists a wave keeps
  constexpr int TG = NT / KP, PT = TB / TG;  // the threads cover TG targets x KP entries: PT entries a thread
  constexpr int PS = (TB * FOLD_TILE + NT - 1) / NT;  // (rating, target) products a thread
  static_assert(FOLD_TILE * TB <= 4 * KP, "the tile's contributions take the place of b, the column buffers and z");
  static_assert(NT % KP == 0 && TB % TG == 0 && FOLD_TILE <= 64 && 2 * TB <= FOLD_TILE, "batch and thread grid do not match");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FoldArgs& a = g.f;
  float* tile = reinterpret_cast<float*>(smem);  // [FOLD_TILE][KP]
  double* vec = reinterpret_cast<double*>(smem + fold_front_bytes(KP, TRI_LDS));
  double* colb = vec + KP;
  double* zb = colb + 2 * KP;
  double* dinv = zb + KP;
  double* cw = colb + fold_work_doubles(KP, false);
  double* ww = cw + FOLD_TILE;
  double* pw = ww + FOLD_TILE;
  double* zt = pw + FOLD_TILE;  // [TB][KP] z_t of the batch
  double* eb = vec;             // [TB][FOLD_TILE] once the factor is done
  double* pv = cw;              // [2][TB] the substitutions' pivot entries, once the build is done
  double* A = TRI_LDS ? reinterpret_cast<double*>(smem) : a.scratch + (size_t)blockIdx.x * fold_tri(KP);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ti = tid % KP, tg = tid / KP;
  const int k = a.k, m_out = g.m;
  for (int64_t li = blockIdx.x; li < g.n_runs; li += gridDim.x) {
    const int64_t u = g.order[li];
    const uint32_t row = g.runs[u];
    if (row == EXPLAIN_NONE) continue;  // the pairs that cannot be explained keep what the fill left
    const int64_t q0 = g.pptr[u], q1 = g.pptr[u + 1];
    const int64_t p0 = a.ptr[row];
    const int64_t deg = a.deg[row];
    if (deg == 0) {  // no rating survived: a sum of nothing, an empty list
      for (int64_t q = q0 + tid; q < q1; q += NT) g.total[g.slot[q]] = 0.0;
      continue;
    }
    {
      double acc[NB][NB];
      fold_build<KP, TS>(a, p0, deg, k, tid, tile, cw, ww, pw, vec, acc);
      const bool ok = fold_factor<KP, TS>(k, tid, acc, A, vec, colb, zb, dinv);
      __syncthreads();
      if (!ok) {
        if (tid == 0) atomicMin(a.bad, (int)row);
        continue;
      }
    }
    for (int64_t b0 = q0; b0 < q1; b0 += TB) {
      const int nb = q1 - b0 < TB ? (int)(q1 - b0) : TB;
      // ---- z_t = A⁻¹ y_t for the batch: thread (tg, ti) keeps entry ti of the targets tg, tg + TG, .. ----
      double zr[PT];
#pragma unroll
      for (int u = 0; u < PT; ++u) {
        const int t = tg + TG * u;
        zr[u] = t < nb && ti < k ? (double)a.Y[(int64_t)g.target[g.slot[b0 + t]] * KP + ti] : 0.0;
      }
      // L u = y, column by column.  Entry j is final once column j - 1 has been applied: its owner then leaves it
      // in pv (two alternating buffers, so one barrier per column serves every target) for all to read
      if (ti == 0)
#pragma unroll
        for (int u = 0; u < PT; ++u) pv[tg + TG * u] = zr[u];
      __syncthreads();  // also: the last batch's z and values have been read
      for (int j = 0; j < k; ++j) {
        const double dj = dinv[j];
        const double *pj = pv + (j & 1) * TB;
        double* pn = pv + ((j + 1) & 1) * TB;
        if (ti > j && ti < k) {
          const double l = A[tri_at(ti, j)];
#pragma unroll
          for (int u = 0; u < PT; ++u) zr[u] -= l * (pj[tg + TG * u] * dj);
          if (ti == j + 1)
#pragma unroll
            for (int u = 0; u < PT; ++u) pn[tg + TG * u] = zr[u];
        }
        __syncthreads();
      }
      const double di = ti < k ? dinv[ti] : 0.0;
#pragma unroll
      for (int u = 0; u < PT; ++u) zr[u] *= di;
      // Lᵀ z = u, from the last column: row j of L is contiguous in the triangle
      if (ti == k - 1)
#pragma unroll
        for (int u = 0; u < PT; ++u) pv[((k - 1) & 1) * TB + tg + TG * u] = zr[u];
      __syncthreads();
      for (int j = k - 1; j >= 0; --j) {
        const double dj = dinv[j];
        const double *pj = pv + (j & 1) * TB;
        double* pn = pv + ((j + 1) & 1) * TB;
        if (ti < j) {
          const double l = A[tri_at(j, ti)];
#pragma unroll
          for (int u = 0; u < PT; ++u) zr[u] -= l * (pj[tg + TG * u] * dj);
          if (ti == j - 1)
#pragma unroll
            for (int u = 0; u < PT; ++u) pn[tg + TG * u] = zr[u];
        }
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < PT; ++u) zt[(tg + TG * u) * KP + ti] = zr[u] * di;
      // ---- the contributions, a tile of ratings at a time, and the lists ----
      double lv[TPW], tot[TPW];
      int lr[TPW];
#pragma unroll
      for (int s = 0; s < TPW; ++s) {
        lv[s] = __longlong_as_double(0x7FF8000000000000ll);
        lr[s] = -1;
        tot[s] = 0.0;
      }
      for (int64_t t0 = 0; t0 < deg; t0 += FOLD_TILE) {
        const int nt = deg - t0 < FOLD_TILE ? (int)(deg - t0) : FOLD_TILE;
        __syncthreads();  // z is there; the last tile's values have been read
#pragma unroll
        for (int v = 0; v < PS; ++v) {
          const int e = tid + v * NT, t = e / FOLD_TILE, r = e % FOLD_TILE;
          if (t >= nb || r >= nt) continue;  // t >= TB included
          const float rt = a.val[p0 + t0 + r];
          const double w = a.implicit ? (rt > 0.f ? 1.0 + a.alpha * (double)fabsf(rt) : 0.0) : (double)rt;
          const float* y = a.Y + (int64_t)a.col[p0 + t0 + r] * KP;
          const double* z = zt + t * KP;
          double d = 0.0;
          int mm = 0;
          for (; mm + 4 <= k; mm += 4) {
            const float4 y4 = *reinterpret_cast<const float4*>(y + mm);
            d += (double)y4.x * z[mm];
            d += (double)y4.y * z[mm + 1];
            d += (double)y4.z * z[mm + 2];
            d += (double)y4.w * z[mm + 3];
          }
          for (; mm < k; ++mm) d += (double)y[mm] * z[mm];
          eb[e] = w * d;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
          const int t = wave + NW * s;
          if (t >= nb) continue;  // uniform in the wave
          for (int r = 0; r < nt; ++r) tot[s] += eb[t * FOLD_TILE + r];  // CSR order
          const bool valid = lane < nt;  // lane r offers rating r of the tile
          explain_offer(lv[s], lr[s], valid ? eb[t * FOLD_TILE + lane] : 0.0, valid ? (int)a.col[p0 + t0 + lane] : 0,
                        valid, m_out, lane);
        }
      }
#pragma unroll
      for (int s = 0; s < TPW; ++s) {
        const int t = wave + NW * s;
        if (t >= nb) continue;
        const size_t slot = g.slot[b0 + t];
        if (lane == 0) g.total[slot] = tot[s];
        if (lane < m_out) {
          g.ids[slot * m_out + lane] = lr[s] >= 0 ? g.src_ids[lr[s]] : -1;
          g.contrib[slot * m_out + lane] = lv[s];
        }
      }
      __syncthreads();  // z and the tile's values have been read: the next batch, or the next row's build, may write
    }
  }
}

template <int KP, int TS, bool TRI_LDS>
hipError_t explain_launch(const ExplainArgs& a, int n_wg, hipStream_t s) {
  constexpr size_t lds = fold_lds_bytes(KP, TRI_LDS) + (size_t)EXPLAIN_TB * KP * 8;
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(explain_kernel<KP, TS, TRI_LDS>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  explain_kernel<KP, TS, TRI_LDS><<<n_wg, TS * TS, lds, s>>>(a);
  return hipGetLastError();
}

}  // namespace

size_t explain_sort_temp_bytes(int64_t n) {
  return std::max(sort_keys64_temp_bytes(n), group_temp_bytes<true, true>(n));
}

hipError_t explain_map_pairs(const int32_t* pair_row_id, const int32_t* pair_target_id, int64_t n_pairs,
                             const int32_t* row_ids, const uint32_t* row_deg, int64_t n_rows, const int32_t* src_ids,
                             int64_t n_src, void* temp, size_t temp_bytes, const ExplainPairs& x, int64_t* n_runs_host,
                             hipStream_t s) {
  if (n_pairs <= 0 || n_pairs > (int64_t)0x7FFFFFFF || n_rows <= 0 || n_rows >= (int64_t)EXPLAIN_NONE ||
      n_src >= (int64_t)EXPLAIN_NONE)
    return hipErrorInvalidValue;
  explain_pair_kernel<<<front_grid(n_pairs), 256, 0, s>>>(pair_row_id, pair_target_id, n_pairs, row_ids, n_rows,
                                                            src_ids, n_src, x.key, x.target);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t tb = temp_bytes;
  e = rocprim::radix_sort_keys(temp, tb, x.key, x.key_sorted, (size_t)n_pairs, 0, 64, s);
  if (e != hipSuccess) return e;
  split_keys_kernel<<<front_grid(n_pairs), 256, 0, s>>>(x.key_sorted, n_pairs, x.hi, x.slot);
  e = group_runs<true>(temp, temp_bytes, x.hi, n_pairs, x.runs, x.counts, x.ptr, x.n_runs, n_runs_host, s);
  if (e != hipSuccess) return e;
  const int64_t nu = *n_runs_host;
  explain_deg_kernel<<<front_grid(nu), 256, 0, s>>>(x.runs, nu, row_deg, x.deg, x.iota);
  return degree_order<false>(temp, temp_bytes, x.deg, x.deg_sorted, x.iota, x.order, nu, s);
}

hipError_t launch_explain_fill(int64_t n_pairs, int m, double* total, int32_t* ids, double* contrib, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  if (m < 1 || m > EXPLAIN_MAX_M) return hipErrorInvalidValue;
  explain_fill_kernel<<<front_grid(n_pairs * m), 256, 0, s>>>(n_pairs, n_pairs * m, total, ids, contrib);
  return hipGetLastError();
}

// LDS: the fold-in's layout and the batch's z: 24 KB at KP = 64 (six rows per CU), 80 KB at KP = 128 (two per
// CU), 60 KB at KP = 256 (1024 threads: one per CU)
hipError_t launch_explain(int KP, const ExplainArgs& a, int n_wg, hipStream_t s) {
  if (a.n_runs <= 0) return hipSuccess;
  if (n_wg <= 0 || a.f.k <= 0 || a.f.k > KP || a.m < 1 || a.m > EXPLAIN_MAX_M) return hipErrorInvalidValue;
  if (KP == 256 && !a.f.scratch) return hipErrorInvalidValue;
  if (KP == 64) return explain_launch<64, 8, true>(a, n_wg, s);
  if (KP == 128) return explain_launch<128, 16, true>(a, n_wg, s);
  if (KP == 256) return explain_launch<256, 32, false>(a, n_wg, s);
  return hipErrorInvalidValue;
}

}  // namespace albedo
