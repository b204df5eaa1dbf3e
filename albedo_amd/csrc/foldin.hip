// als_fold_in: the factors of rows that were not in the fit, each solved against the frozen factors of
// the other side (include/albedo_als.h).  For row j with ratings r_i of src rows y_i
//   (G + Σ_i c_i y_i y_iᵀ + λ n I) x = Σ_i w_i y_i
// with G, c, w and n as the row audit (audit.hip) defines them: Spark's computeFactors for one row.
//
// Written like audit.hip and for the same reason: it must not disturb, or depend on, the solve kernels
// of the half-sweep.  Plain HIP, no inline asm, no MFMA, none of device_common.h; the factors are in the
// original basis and everything is fp64 from the first product on.  The system has the model rank k,
// not the padded one.
//
//   fold_key_kernel .. fold_rows_kernel   the triples as a CSR: src ids to rows by binary search, one
//                      64-bit radix sort on (row id, src row), run lengths, degrees, rows by descending degree
//   fold_solve_kernel  one workgroup per row, persistent over the degree-ordered list.  The build and the factor
//             are the __device__ functions of fold_front.h, which explain.hip (als_explain) includes too.
//     build   FOLD_TILE src rows at a time are gathered into LDS as fp32 (every load of a tile is issued
//             before the first is stored).  The threads form a TS x TS grid; thread (ty, tx) owns the
//             entries (i, m) with i = ty mod TS, m = tx mod TS of the lower triangle, 36 doubles at
//             KP = 64 (TS = 8, one wave), KP = 128 (TS = 16) and KP = 256 (TS = 32), and adds c·y_i·y_m
//             rating by rating in CSR order: no atomics, no split, one fixed order of addition.
//     factor  right-looking Cholesky, column by column, on the sums where they are: the column goes through
//             LDS, every thread scales the entries it needs and updates its own part of the trailing
//             triangle in registers.  The finished columns of L are left in the packed lower triangle
//             (row-major), which takes the place of the tile in LDS at KP <= 128 (66 KB at 128: two rows
//             per CU); at KP = 256 it is 263 KB and lives in the workgroup's slab of global scratch, written
//             once per column.  L z = b rides along with the columns; the back substitution reads the
//             triangle, one column per step.
//     A pivot <= 0 or NaN ends the row and leaves its index in *bad (integer atomicMin).
//   fold_solve_kernel<.., NNLS = true>  the same build, then Spark 2.2.0's NNLS.solve (mllib/optimization/NNLS.scala,
//     restated in oracle/spark_als.py:nnls) on the row's system in place of the factorisation: the owners leave A
//     in the packed triangle (LDS at KP <= 128, the scratch slab at KP = 256) and fold_nnls iterates on it.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "fold_front.h"
#include "id_front.h"
#include "kernels.h"

namespace albedo {

namespace {

constexpr uint32_t FOLD_DROPPED = 0xFFFFFFFFu;

__global__ void fold_key_kernel(const int32_t* __restrict__ row_id, const int32_t* __restrict__ src_id, int64_t n,
                                const int32_t* __restrict__ ids, int64_t n_ids, uint64_t* __restrict__ key) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = find_id(ids, n_ids, src_id[i]);
    const uint32_t c = r >= 0 ? (uint32_t)r : FOLD_DROPPED;
    key[i] = ((uint64_t)((uint32_t)row_id[i] ^ 0x80000000u) << 32) | c;
  }
}

// per row: its raw id and the count of its live triples (the dropped ones end its range)
__global__ void fold_rows_kernel(const uint32_t* __restrict__ runs, const int64_t* __restrict__ ptr,
                                 const uint32_t* __restrict__ col, int64_t n_rows, int32_t* __restrict__ ids,
                                 uint32_t* __restrict__ deg) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = ptr[r], hi = ptr[r + 1];
    const int64_t p0 = lo;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (col[mid] != FOLD_DROPPED) lo = mid + 1;
      else hi = mid;
    }
    deg[r] = (uint32_t)(lo - p0);
    ids[r] = (int32_t)(runs[r] ^ 0x80000000u);
  }
}

// ---- the solve (its LDS layout, build and factorisation: fold_front.h) -----------------------------------
// ---- Spark's NNLS.solve on the packed triangle ------------------------------------------------------------
// Thread tid = p * KP + r is thread p of row r: NT / KP = KP / 64 threads a row, each with 64 columns.
// out = the part of (A v)_r over the columns [64 p, 64 p + 64) ∩ [0, k), added in ascending column order with
// a product and a sum per entry, as the oracle's loop does (no fma: at k <= 64 the sum is the oracle's to the
// bit).  Lanes are consecutive rows: entry (r, c) of the triangle lies at T(r) + c for c <= r, where the
// triangular numbers spread 32 consecutive rows over all the 8-byte banks, and at T(c) + r above the diagonal,
// which is contiguous across the lanes.
template <int KP, int NV>
__device__ __forceinline__ void fold_symv(const double* A, const int k, const int r, const int p, const double* v0,
                                          const double* v1, double& s0, double& s1) {
#pragma clang fp contract(off)
  s0 = 0.0;
  s1 = 0.0;
  if (r >= k) return;
  const int c0 = 64 * p, c1 = k < c0 + 64 ? k : c0 + 64, tr = r * (r + 1) / 2;
  int tc = c0 * (c0 + 1) / 2;  // T(c): p is the same in every lane of a wave, so c and T(c) stay scalar
#pragma unroll 8
  for (int c = c0; c < c1; ++c) {
    const int below = tr + c, above = tc + r;  // both formed, one selected: no branch per entry
    const double e = A[c <= r ? below : above];
    s0 += e * v0[c];
    if (NV == 2) s1 += e * v1[c];
    tc += c + 1;
  }
}

// Σ over the rows of N values at once: a butterfly inside each of the KP / 64 waves that hold the row threads
// (every lane ends with the same bits: a + b = b + a), lane 0 leaves the wave's sums in wp[wave][4].  The caller's
// barrier follows; thread 0 then adds the waves in ascending order.
template <int KP, int N>
__device__ __forceinline__ void fold_wave_sums(const int tid, double (&v)[N], double* wp) {
  if (tid < KP) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] += __shfl_xor(v[q], off);
    if ((tid & 63) == 0)
#pragma unroll
      for (int q = 0; q < N; ++q) wp[(tid >> 6) * 4 + q] = v[q];
  }
}

__device__ __forceinline__ double fold_add_waves(const double* wp, const int nw, const int q) {
  double s = wp[q];
  for (int w = 1; w < nw; ++w) s += wp[w * 4 + q];
  return s;
}

__device__ __forceinline__ bool fold_nnls_stop(const double step, const double ndir, const double nx) {
  return step != step || step < 1e-7 || step > 1e40 || ndir < 1e-12 * nx || ndir < 1e-32;
}

// NNLS.solve for the k x k system (A in the packed triangle, b) of one row: x0 = 0, at most max(400, 20 k)
// iterations of: res = A x - b, the projected gradient, the steepest-descent step, the conjugate direction once
// iterno > lastWall + 1, the stop test, the step clamp, the update with the wall rule.  Every sum has one fixed
// order.  The scalars of an iteration (the norms, alpha, step, stop, which direction, whether a wall was hit)
// are computed by thread 0 or set as a flag in LDS and read by every thread behind a barrier, so every thread
// takes the same branches and leaves the loop in the same iteration.  Returns the iterations taken; x is left
// in w[0 .. k).
template <int KP, int NT>
__device__ __forceinline__ int fold_nnls(const double* A, const int k, const int tid, const double* b, double* w,
                                         double* wp) {
#pragma clang fp contract(off)
  constexpr int P = NT / KP, NW = KP / 64;
  static_assert(P == NW && NW >= 1 && NW <= 4, "64 columns per thread of a row");
  double *x = w, *res = x + KP, *grad = res + KP, *dir = grad + KP, *last = dir + KP;
  double* pg = last + KP;           // [P - 1][KP] partial products with grad (or x)
  double* pd = pg + (P - 1) * KP;   // [P - 1][KP] and with dir
  double* sc = wp + 16;             // 0 ngrad, 1 grad·res, 2 ‖x‖², 3 alpha, 4 step
  int* fl = reinterpret_cast<int*>(sc + 8);  // 0 stop, 1 dir = grad after all, 2 the clamp binds, 3 a wall was hit
  // a wave holds 64 consecutive threads and KP is a multiple of 64: p is uniform in the wave, and kept scalar
  const int r = tid % KP, p = __builtin_amdgcn_readfirstlane(tid) / KP;
  const bool mine = p == 0 && r < k;  // this thread finishes row r
  const int iter_max = 20 * k > 400 ? 20 * k : 400;
  if (tid < KP) {
    x[tid] = 0.0;
    last[tid] = 0.0;
  }
  double last_norm = 0.0;
  int iterno = 0, last_wall = 0;
  __syncthreads();  // A, b and x = 0 are there
  while (iterno < iter_max) {
    double s0, s1;
    fold_symv<KP, 1>(A, k, r, p, x, x, s0, s1);
    if (P > 1) {
      if (p > 0 && r < k) pg[(p - 1) * KP + r] = s0;
      __syncthreads();
    }
    double g = 0.0, rs = 0.0, xi = 0.0;
    if (mine) {
      for (int q = 1; q < P; ++q) s0 += pg[(q - 1) * KP + r];
      rs = s0 - b[r];
      xi = x[r];
      g = rs > 0.0 && xi == 0.0 ? 0.0 : rs;
      res[r] = rs;
      grad[r] = g;
    }
    double v3[3] = {g * g, g * rs, xi * xi};
    fold_wave_sums<KP, 3>(tid, v3, wp);
    __syncthreads();
    const bool cg = iterno > last_wall + 1;
    if (tid == 0) {
      const double ngrad = fold_add_waves(wp, NW, 0);
      sc[0] = ngrad;
      sc[1] = fold_add_waves(wp, NW, 1);
      sc[2] = fold_add_waves(wp, NW, 2);
      sc[3] = ngrad / last_norm;  // read only when cg
    }
    __syncthreads();
    const double ngrad = sc[0];
    double d = g;
    if (mine) {
      if (cg) d = g + sc[3] * last[r];
      dir[r] = d;
    }
    __syncthreads();
    // A grad and A dir in one pass over the triangle
    if (cg) fold_symv<KP, 2>(A, k, r, p, grad, dir, s0, s1);
    else fold_symv<KP, 1>(A, k, r, p, grad, grad, s0, s1);
    if (P > 1) {
      if (p > 0 && r < k) {
        pg[(p - 1) * KP + r] = s0;
        pd[(p - 1) * KP + r] = s1;
      }
      __syncthreads();
    }
    double v4[4] = {0.0, 0.0, 0.0, 0.0};
    if (mine) {
      for (int q = 1; q < P; ++q) {
        s0 += pg[(q - 1) * KP + r];
        s1 += pd[(q - 1) * KP + r];
      }
      v4[0] = s0 * g;
      if (cg) {
        v4[1] = d * rs;
        v4[2] = s1 * d;
        v4[3] = d * d;
      }
    }
    fold_wave_sums<KP, 4>(tid, v4, wp);
    __syncthreads();
    if (tid == 0) {
      const double nx = sc[2];
      double step = sc[1] / (fold_add_waves(wp, NW, 0) + 1e-20), ndir = ngrad;
      int back = 0;
      if (cg) {
        const double dstep = fold_add_waves(wp, NW, 1) / (fold_add_waves(wp, NW, 2) + 1e-20);
        const double nd = fold_add_waves(wp, NW, 3);
        if (fold_nnls_stop(dstep, nd, nx)) {
          back = 1;
        } else {
          step = dstep;
          ndir = nd;
        }
      }
      sc[4] = step;
      fl[0] = fold_nnls_stop(step, ndir, nx);
      fl[1] = back;
      fl[2] = 0;
      fl[3] = 0;
    }
    __syncthreads();
    if (fl[0]) break;
    double step = sc[4];
    if (mine) {
      if (fl[1]) {
        d = g;
        dir[r] = d;
      }
      if (step * d > xi) fl[2] = 1;
    }
    __syncthreads();
    if (fl[2]) {
      // The clamp binds somewhere.  Spark's loop `if (step * dir[i] > x[i]) step = x[i] / dir[i]` runs in index
      // order with the step shrinking as it goes; wave 0 runs it 64 indices at a time: the first index whose
      // test holds at the current step sets the step, and only the indices behind it are tested again.  The
      // same products, comparisons and quotients in the same order as the serial loop.
      if (tid < 64) {
        double st = step;
        for (int base = 0; base < k; base += 64) {
          const int i = base + tid;
          const double di = i < k ? dir[i] : 0.0, xv = i < k ? x[i] : 0.0;
          const double q = xv / di;  // taken only where the test holds, which needs dir[i] > 0
          unsigned long long todo = ~0ull;
          for (;;) {
            const unsigned long long m = __ballot(st * di > xv) & todo;
            if (!m) break;
            const int j = __ffsll(m) - 1;
            st = __shfl(q, j);
            todo = j == 63 ? 0ull : ~0ull << (j + 1);
          }
        }
        if (tid == 0) sc[4] = st;
      }
      __syncthreads();
      step = sc[4];
    }
    if (mine) {
      if (step * d > xi * (1 - 1e-14)) {
        x[r] = 0.0;
        fl[3] = 1;
      } else {
        x[r] = xi - step * d;
      }
      last[r] = d;
    }
    __syncthreads();
    if (fl[3]) last_wall = iterno;
    ++iterno;
    last_norm = ngrad;
  }
  return iterno;
}

template <int KP, int TS, bool TRI_LDS, bool NNLS>
__global__ __launch_bounds__(TS* TS) void fold_solve_kernel(const FoldArgs a) {
  constexpr int NT = TS * TS, NB = KP / TS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);  // [FOLD_TILE][KP]
  double* vec = reinterpret_cast<double*>(smem + fold_front_bytes(KP, TRI_LDS));  // b, then x
  double* colb = vec + KP;                                                        // two column buffers (NNLS: fold_nnls's vectors)
  double* zb = colb + 2 * KP;
  double* dinv = zb + KP;
  double* cw = colb + fold_work_doubles(KP, NNLS);
  double* ww = cw + FOLD_TILE;
  double* pw = ww + FOLD_TILE;
  double* A = TRI_LDS ? reinterpret_cast<double*>(smem) : a.scratch + (size_t)blockIdx.x * fold_tri(KP);
  const int tid = threadIdx.x, tx = tid % TS, ty = tid / TS;
  const int k = a.k;
  for (int64_t li = blockIdx.x; li < a.n_rows; li += gridDim.x) {
    const int64_t row = a.order[li];
    const int64_t p0 = a.ptr[row];
    const int64_t deg = a.deg[row];
    float* xo = a.X + row * k;
    if (deg == 0) {  // nothing survived: Spark leaves such a row out, here it is zero
      for (int i = tid; i < k; i += NT) xo[i] = 0.f;
      continue;
    }
    // ---- build (fold_front.h) ----
    double acc[NB][NB];
    fold_build<KP, TS>(a, p0, deg, k, tid, tile, cw, ww, pw, vec, acc);
    if constexpr (NNLS) {
      // ---- NNLS.solve on A: the owners leave their entries in the packed triangle ----
      __syncthreads();  // the last tile is read, the triangle may take its place
#pragma unroll
      for (int ia = 0; ia < NB; ++ia)
#pragma unroll
        for (int ib = 0; ib <= ia; ++ib) {
          const int i = ty + TS * ia, m = tx + TS * ib;
          if (m <= i && i < k) A[tri_at(i, m)] = acc[ia][ib];
        }
      const int it = fold_nnls<KP, NT>(A, k, tid, vec, colb, pw + FOLD_TILE);
      for (int i = tid; i < k; i += NT) xo[i] = (float)colb[i];
      if (tid == 0) {  // integers: the order of arrival does not show
        atomicAdd(a.stats, (unsigned long long)it);
        atomicMax(a.stats + 1, (unsigned long long)it);
        atomicAdd(a.stats + 2, 1ull);
        if (it >= (20 * k > 400 ? 20 * k : 400)) atomicAdd(a.stats + 3, 1ull);
      }
      continue;
    }
    // ---- A = L Lᵀ in the registers that built A, L z = b riding along (fold_front.h) ----
    const bool ok = fold_factor<KP, TS>(k, tid, acc, A, vec, colb, zb, dinv);
    __syncthreads();
    if (!ok) {
      if (tid == 0) atomicMin(a.bad, (int)row);
      continue;
    }
    // ---- Lᵀ x = z (x in vec) ----
    for (int j = k - 1; j >= 0; --j) {
      const double x = zb[j] * dinv[j];
      for (int m = tid; m < j; m += NT) zb[m] -= A[tri_at(j, m)] * x;
      if (tid == 0) vec[j] = x;
      __syncthreads();
    }
    for (int i = tid; i < k; i += NT) xo[i] = (float)vec[i];
  }
}

template <int KP, int TS, bool TRI_LDS, bool NNLS>
hipError_t fold_launch(const FoldArgs& a, int n_wg, hipStream_t s) {
  constexpr size_t lds = fold_lds_bytes(KP, TRI_LDS, NNLS);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fold_solve_kernel<KP, TS, TRI_LDS, NNLS>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  fold_solve_kernel<KP, TS, TRI_LDS, NNLS><<<n_wg, TS * TS, lds, s>>>(a);
  return hipGetLastError();
}

}  // namespace

size_t fold_sort_temp_bytes(int64_t n) {
  size_t a = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (float*)nullptr, (float*)nullptr,
                                  (size_t)n, 0, 64, (hipStream_t)0);
  return std::max(a, group_temp_bytes<true, true>(n));
}

hipError_t fold_build_csr(const int32_t* row_id, const int32_t* src_id, const float* rating, int64_t n,
                          const int32_t* src_ids, int64_t n_src, void* temp, size_t temp_bytes, const FoldCsr& f,
                          int64_t* n_rows_host, hipStream_t s) {
  if (n <= 0 || n > (int64_t)0x7FFFFFFF || n_src >= (int64_t)FOLD_DROPPED) return hipErrorInvalidValue;
  fold_key_kernel<<<front_grid(n), 256, 0, s>>>(row_id, src_id, n, src_ids, n_src, f.key);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t tb = temp_bytes;
  e = rocprim::radix_sort_pairs(temp, tb, f.key, f.key_sorted, rating, f.val_sorted, (size_t)n, 0, 64, s);
  if (e != hipSuccess) return e;
  split_keys_kernel<<<front_grid(n), 256, 0, s>>>(f.key_sorted, n, f.hi, f.col);
  e = group_runs<true>(temp, temp_bytes, f.hi, n, f.runs, f.counts, f.ptr, f.n_rows, n_rows_host, s);
  if (e != hipSuccess) return e;
  const int64_t nr = *n_rows_host;
  fold_rows_kernel<<<front_grid(nr), 256, 0, s>>>(f.runs, f.ptr, f.col, nr, f.ids, f.deg);
  return degree_order<true>(temp, temp_bytes, f.deg, f.deg_sorted, f.iota, f.order, nr, s);
}

// KP = 64: one wave per row (its barriers cost nothing) and 19 KB of LDS, eight rows per CU; KP = 128: 69 KB
// of LDS, two per CU; KP = 256: 1024 threads at the registers of the build, one per CU.  The NNLS instances
// take 20 KB, 74 KB and 57 KB: the same counts fit
int fold_workgroups(int KP, int64_t n_rows, int n_cu) {
  int64_t wgs = (int64_t)n_cu * (KP == 64 ? 8 : KP == 128 ? 2 : 1);
  const char* e = std::getenv("ALBEDO_FOLD_WGS");
  if (e && *e && std::atoll(e) > 0) wgs = std::min<int64_t>(wgs, std::atoll(e));
  return (int)std::max<int64_t>(1, std::min<int64_t>(wgs, n_rows));
}

size_t fold_scratch_doubles(int KP, int n_wg) { return KP == 256 ? (size_t)n_wg * fold_tri(256) : 0; }

hipError_t launch_fold_solve(int KP, const FoldArgs& a, int n_wg, hipStream_t s) {
  if (a.n_rows <= 0) return hipSuccess;
  if (n_wg <= 0 || a.k <= 0 || a.k > KP || a.n_rows > (int64_t)0x7FFFFFFF) return hipErrorInvalidValue;
  if (KP == 256 && !a.scratch) return hipErrorInvalidValue;
  if (a.nonnegative) {
    if (!a.stats) return hipErrorInvalidValue;
    if (KP == 64) return fold_launch<64, 8, true, true>(a, n_wg, s);
    if (KP == 128) return fold_launch<128, 16, true, true>(a, n_wg, s);
    if (KP == 256) return fold_launch<256, 32, false, true>(a, n_wg, s);
    return hipErrorInvalidValue;
  }
  if (KP == 64) return fold_launch<64, 8, true, false>(a, n_wg, s);
  if (KP == 128) return fold_launch<128, 16, true, false>(a, n_wg, s);
  if (KP == 256) return fold_launch<256, 32, false, false>(a, n_wg, s);
  return hipErrorInvalidValue;
}

}  // namespace albedo
