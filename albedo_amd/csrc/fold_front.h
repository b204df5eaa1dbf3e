// The front half of a fold-in row, shared by fold_solve_kernel (foldin.hip) and explain_kernel (explain.hip):
// the LDS layout, the build of the row's system in registers and its Cholesky factorisation.  Both kernels
// include these sections as they are, so a row's A and L are the same bits in either.  Device code only; plain
// HIP, none of device_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace albedo {
namespace {

__host__ __device__ constexpr int fold_tri(int KP) { return KP * (KP + 1) / 2; }
// the triangle shares its LDS with the gather tile: the build holds its sums in registers until the last
// tile has been read
__host__ __device__ constexpr size_t fold_front_bytes(int KP, bool tri_lds) {
  const size_t tile = (size_t)FOLD_TILE * KP * 4, tri = tri_lds ? (size_t)fold_tri(KP) * 8 : 0;
  return tile > tri ? tile : tri;
}
// doubles behind the right-hand side.  Cholesky: two column buffers, z and 1 / diag(L).  NNLS: x, res, grad, dir
// and lastDir, then the partial products of the threads 1 .. KP / 64 - 1 of each row for two vectors
__host__ __device__ constexpr int fold_work_doubles(int KP, bool nnls) {
  return nnls ? (5 + 2 * (KP / 64 - 1)) * KP : 4 * KP;
}
constexpr int FOLD_NNLS_SCALARS = 32;  // per-wave partial sums [4][4], 8 broadcast doubles, 4 ints
// + the right-hand side / solution, the solver's vectors, c, w and (r > 0) of the tile's ratings, and the NNLS
// loop's partial sums and broadcast scalars
__host__ __device__ constexpr size_t fold_lds_bytes(int KP, bool tri_lds, bool nnls = false) {
  return fold_front_bytes(KP, tri_lds) +
         (size_t)(KP + fold_work_doubles(KP, nnls) + 3 * FOLD_TILE + (nnls ? FOLD_NNLS_SCALARS : 0)) * 8;
}

__device__ inline int tri_at(int i, int m) { return i * (i + 1) / 2 + m; }  // m <= i

// ---- build: A = G + Σ c y yᵀ + λ n I in acc, b = Σ w y in vec -----------------------------------------------
// The threads form a TS x TS grid; thread (ty, tx) owns the entries (i, m) with i = ty mod TS, m = tx mod TS of
// the lower triangle.  The row's deg > 0 live triples start at p0 of the CSR.
template <int KP, int TS>
__device__ __forceinline__ void fold_build(const FoldArgs& a, const int64_t p0, const int64_t deg, const int k,
                                           const int tid, float* tile, double* cw, double* ww, double* pw, double* vec,
                                           double (&acc)[KP / TS][KP / TS]) {
  constexpr int NT = TS * TS, NB = KP / TS, Q = KP / 4;
  constexpr int PER = FOLD_TILE * Q / NT;  // 16-byte loads per thread and tile
  static_assert(FOLD_TILE * Q % NT == 0 && KP <= NT && FOLD_TILE <= NT, "tile and thread grid do not match");
  const int tx = tid % TS, ty = tid / TS;
#pragma unroll
  for (int ia = 0; ia < NB; ++ia)
#pragma unroll
    for (int ib = 0; ib < NB; ++ib) acc[ia][ib] = 0.0;
  double bacc = 0.0, npos = 0.0;
  for (int64_t t0 = 0; t0 < deg; t0 += FOLD_TILE) {
    const int nt = deg - t0 < FOLD_TILE ? (int)(deg - t0) : FOLD_TILE;
    float4 v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * NT, r = e / Q, c4 = e % Q;
      v[u] = r < nt ? *reinterpret_cast<const float4*>(a.Y + (int64_t)a.col[p0 + t0 + r] * KP + 4 * c4)
                    : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // the tile's (or the last row's triangle's and solution's) readers are done
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * NT;
      *reinterpret_cast<float4*>(tile + 4 * e) = v[u];
    }
    if (tid < FOLD_TILE) {
      const float r = tid < nt ? a.val[p0 + t0 + tid] : 0.f;
      double c, w, pos;
      if (a.implicit) {
        c = a.alpha * (double)fabsf(r);
        w = r > 0.f ? 1.0 + c : 0.0;
        pos = r > 0.f ? 1.0 : 0.0;
      } else {
        c = tid < nt ? 1.0 : 0.0;
        w = (double)r;
        pos = c;
      }
      cw[tid] = c;
      ww[tid] = w;
      pw[tid] = pos;
    }
    __syncthreads();
    for (int r = 0; r < nt; ++r) {
      const float* y = tile + r * KP;
      const double c = cw[r];
      float yi[NB], ym[NB];  // widened where they are used: the sums take the registers
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        yi[q] = y[ty + TS * q];
        ym[q] = y[tx + TS * q];
      }
#pragma unroll
      for (int ia = 0; ia < NB; ++ia) {
        const double cy = c * (double)yi[ia];
#pragma unroll
        for (int ib = 0; ib <= ia; ++ib) acc[ia][ib] += cy * (double)ym[ib];
      }
      if (tid < KP) bacc += ww[r] * (double)y[tid];
      npos += pw[r];
    }
  }
  const double ln = a.reg * npos;
#pragma unroll
  for (int ia = 0; ia < NB; ++ia)
#pragma unroll
    for (int ib = 0; ib <= ia; ++ib) {
      const int i = ty + TS * ia, m = tx + TS * ib;
      if (m > i || i >= k) continue;
      if (a.G) acc[ia][ib] += a.G[(size_t)i * KP + m];
      if (i == m) acc[ia][ib] += ln;
    }
  if (tid < KP) vec[tid] = bacc;
}

// ---- A = L Lᵀ, right-looking, in the registers that built A ------------------------------------------------
// Column j: its owners (tx = j mod TS) put it into LDS, every thread reads the pivot and the entries of
// its own rows and columns, and updates its part of the trailing triangle in registers; the owners leave
// the finished column of L in the packed triangle A (below the diagonal; 1 / L_jj goes to dinv[j]) for the
// substitutions.  One barrier per column: the column buffer alternates, so column j + 2 is written only after
// every thread has passed barrier j + 1.  L z = b rides along (b in vec, z to zb).  False at a pivot <= 0 or NaN,
// in every thread alike; the caller's barrier follows.
template <int KP, int TS>
__device__ __forceinline__ bool fold_factor(const int k, const int tid, double (&acc)[KP / TS][KP / TS], double* A,
                                            double* vec, double* colb, double* zb, double* dinv) {
  constexpr int NB = KP / TS;
  const int tx = tid % TS, ty = tid / TS;
  bool ok = true;
#pragma unroll
  for (int jb = 0; jb < NB; ++jb) {
    const int jend = !ok ? 0 : (k - jb * TS < TS ? k - jb * TS : TS);
    for (int jj = 0; jj < jend; ++jj) {
      const int j = jb * TS + jj;
      double* cb = colb + (j & 1) * KP;
      if (tx == jj) {
#pragma unroll
        for (int ia = jb; ia < NB; ++ia) {
          const int i = ty + TS * ia;
          if (i >= j && i < k) cb[i] = acc[ia][jb];
        }
      }
      __syncthreads();  // also: the last tile is read, the triangle may take its place
      const double d = cb[j];  // the same value in every thread: the exit is uniform
      if (!(d > 0.0)) {
        ok = false;
        break;
      }
      const double rs = 1.0 / sqrt(d);
      double li[NB], lm[NB];
#pragma unroll
      for (int q = jb; q < NB; ++q) {
        const int i = ty + TS * q, m = tx + TS * q;
        li[q] = i > j && i < k ? cb[i] * rs : 0.0;
        lm[q] = m > j && m < k ? cb[m] * rs : 0.0;
      }
#pragma unroll
      for (int ia = jb; ia < NB; ++ia)
#pragma unroll
        for (int ib = jb; ib <= ia; ++ib) acc[ia][ib] -= li[ia] * lm[ib];
      if (tx == jj) {
#pragma unroll
        for (int ia = jb; ia < NB; ++ia) {
          const int i = ty + TS * ia;
          if (i > j && i < k) A[tri_at(i, j)] = li[ia];
        }
      }
      // L z = b rides along: vec[j] is final once column j - 1 has been applied (before this column's barrier)
      const double z = vec[j] * rs;
      if (tid > j && tid < k) vec[tid] -= cb[tid] * rs * z;
      if (tid == 0) {
        zb[j] = z;
        dinv[j] = rs;
      }
    }
  }
  return ok;
}

}  // namespace
}  // namespace albedo
