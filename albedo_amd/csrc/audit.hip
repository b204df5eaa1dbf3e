// als_audit_rows: the normal-equation residual of every dst row, in fp64, from the current factors of
// both sides in the original basis (include/albedo_als.h).  For dst row j with factors x
//   r = G·x + Σ_i c_i (y_i·x) y_i + λ n x − b,   b = Σ_i w_i y_i
//   eta = ‖r‖₂ / ((‖G‖_F + Σ_i c_i ‖y_i‖² + λ n)·‖x‖₂ + ‖b‖₂)        (0 when the denominator is 0)
// which needs no k x k build: one pass over the CSR with the gather of the solve's build, O(nnz·k).
//
// This file is a yardstick of the solve kernels, so it shares nothing with them: plain HIP, no inline
// asm, no MFMA, none of device_common.h.  With the other yardstick, objective.hip, it shares the row pass
// (row_pass.h: the gather, the three row kernels and their launches) and the two fp64 products below.
// Everything is fp64 arithmetic on the fp32 factors and ratings.
//
// Per rating the pass hands over t = y·x and every lane adds c·t·y and w·y for its components and c·y²
// for the norm term; the groups are summed once per row, and a row ends as G·x + λ n x − b and the norms.
//   audit_gram_kernel / audit_gram_reduce_kernel   G = Σ y yᵀ in fp64 (launch_gram's 64-row fp32
//                              partials leave G at 1e-7, four decades above what the audit resolves)
//   row_gx_kernel              G·x of a batch of dst rows (a tiled fp64 GEMM; per row it would re-read G)
//   audit_sum_kernel (twice)   the summary: counts, the worst row and the sum, in a fixed order
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "row_pass.h"

namespace albedo {

namespace {

// ---- tiled fp64 products -----------------------------------------------------------------------------
// Both products are C[i][j] = Σ_k A[k][i]·B[k][j] over 64 x 64 tiles of C with 16 k at a time in LDS and
// a 4 x 4 block of C per thread (256 threads).
struct Tile {  // the Gram's operands
  double a[16][64 + 4];  // + 4 as in row_gx_kernel, whose transposing store walks a column
  double b[16][64];
};

__device__ inline void tile_fma(const double (&a)[16][64 + 4], const double (&b)[16][64], int ty, int tx,
                                double (&acc)[4][4]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    double av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      av[i] = a[k][4 * ty + i];
      bv[i] = b[k][4 * tx + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
  }
}

// slab[blockIdx.x][KP][KP] = Σ over this block's rows of x xᵀ; grid (nblk, KP/64, KP/64)
template <int KP>
__global__ __launch_bounds__(256) void audit_gram_kernel(const float* __restrict__ X, int64_t n, int64_t per_blk,
                                                         double* __restrict__ slab) {
  __shared__ Tile t;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.z * 64;
  const int64_t rb = (int64_t)blockIdx.x * per_blk;
  const int64_t re = rb + per_blk < n ? rb + per_blk : n;
  double acc[4][4] = {};
  for (int64_t r0 = rb; r0 < re; r0 += 16) {
    {  // 16 rows x 64 columns of each operand: one float4 per thread
      const int r = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
      if (r0 + r < re) {
        va = *reinterpret_cast<const float4*>(X + (r0 + r) * KP + i0 + c4);
        vb = *reinterpret_cast<const float4*>(X + (r0 + r) * KP + j0 + c4);
      }
      t.a[r][c4 + 0] = va.x, t.a[r][c4 + 1] = va.y, t.a[r][c4 + 2] = va.z, t.a[r][c4 + 3] = va.w;
      t.b[r][c4 + 0] = vb.x, t.b[r][c4 + 1] = vb.y, t.b[r][c4 + 2] = vb.z, t.b[r][c4 + 3] = vb.w;
    }
    __syncthreads();
    tile_fma(t.a, t.b, ty, tx, acc);
    __syncthreads();
  }
  double* out = slab + (size_t)blockIdx.x * KP * KP;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(size_t)(i0 + 4 * ty + i) * KP + j0 + 4 * tx + j] = acc[i][j];
}

// G[e] = Σ_b slab[b][e] in block order
__global__ void audit_gram_reduce_kernel(const double* __restrict__ slab, int nblk, int64_t kk, double* __restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= kk) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += slab[(size_t)b * kk + e];
  G[e] = s;
}

// GX[r][m] = Σ_l X[row0 + r][l]·G[l][m] for r < nb; grid (ceil(nb / 64), KP/64).  The operands are two
// arrays, as the objective's copy of this kernel had them, not one Tile: 62 VGPRs against 154 and half the time
template <int KP>
__global__ __launch_bounds__(256) void row_gx_kernel(const float* __restrict__ X, const double* __restrict__ G,
                                                     double* __restrict__ GX, int64_t row0, int64_t nb) {
  __shared__ double ta[16][64 + 4];  // X, l-major
  __shared__ double tb[16][64];      // G
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int m0 = blockIdx.y * 64;
  double acc[4][4] = {};
  for (int l0 = 0; l0 < KP; l0 += 16) {
    {  // 64 rows x 16 l of X, stored l-major; 16 l x 64 m of G
      const int r = threadIdx.x >> 2, l4 = (threadIdx.x & 3) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < nb) v = *reinterpret_cast<const float4*>(X + (row0 + r0 + r) * KP + l0 + l4);
      ta[l4 + 0][r] = v.x, ta[l4 + 1][r] = v.y, ta[l4 + 2][r] = v.z, ta[l4 + 3][r] = v.w;
      const int l = threadIdx.x >> 4, m4 = (threadIdx.x & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) tb[l][m4 + i] = G[(size_t)(l0 + l) * KP + m0 + m4 + i];
    }
    __syncthreads();
    tile_fma(ta, tb, ty, tx, acc);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = r0 + 4 * ty + i;
    if (r >= nb) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) GX[r * KP + m0 + 4 * tx + j] = acc[i][j];
  }
}

// ---- the audit's row pass (row_pass.h) -----------------------------------------------------------------
struct AuditPass {
  using Args = AuditArgs;
  // What a lane holds for its 4 components of a dst row, after group_sums() the row's (or chunk's) totals
  struct Acc {
    double a[4] = {0.0, 0.0, 0.0, 0.0};  // Σ c (y·x) y
    double b[4] = {0.0, 0.0, 0.0, 0.0};  // Σ w y
    double q = 0.0;                      // Σ c ‖y‖²
    double n = 0.0;                      // implicit: ratings > 0; explicit: the degree
  };
  template <int KP>
  static constexpr int rec_doubles = 2 * KP + 2;  // a chunk's record: a[KP], b[KP], q, n

  struct W {
    double c, w, pos;
  };
  // explicit: a dead lane gathered zeros and adds them with c = 0
  __device__ static W weigh(const Args& g, bool live, float r) {
    double c, w, pos;
    if (g.implicit) {
      c = g.alpha * (double)fabsf(r);
      w = r > 0.f ? 1.0 + c : 0.0;
      pos = r > 0.f ? 1.0 : 0.0;
    } else {
      c = live ? 1.0 : 0.0;
      w = (double)r;
      pos = c;
    }
    return {c, w, pos};
  }

  __device__ static void add(const Args&, Acc& A, const W& k, bool, float, double y0, double y1, double y2, double y3,
                             double t) {
    const double c = k.c, w = k.w, pos = k.pos;
    const double ct = c * t;
    A.a[0] += ct * y0, A.a[1] += ct * y1, A.a[2] += ct * y2, A.a[3] += ct * y3;
    A.b[0] += w * y0, A.b[1] += w * y1, A.b[2] += w * y2, A.b[3] += w * y3;
    A.q += c * (y0 * y0 + y1 * y1 + y2 * y2 + y3 * y3);
    A.n += pos;
  }

  // every lane ends with the totals of its components
  template <int KP>
  __device__ static void group_sums(Acc& A) {
    constexpr int L = KP / 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      A.a[i] = lanes_sum<L, 64>(A.a[i]);
      A.b[i] = lanes_sum<L, 64>(A.b[i]);
    }
    A.n = lanes_sum<L, 64>(A.n);
    A.q = lanes_sum<1, 64>(A.q);  // a lane's part covers its components only
  }

  template <int KP>
  __device__ static void store(double* rec, const Acc& A) {
    const int lane = threadIdx.x & 63;
    if (lane < KP / 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rec[4 * lane + i] = A.a[i];
        rec[KP + 4 * lane + i] = A.b[i];
      }
    }
    if (lane == 0) {
      rec[2 * KP] = A.q;
      rec[2 * KP + 1] = A.n;
    }
  }

  template <int KP>
  __device__ static void load(const double* rec, Acc& A) {
    const int sub = (threadIdx.x & 63) % (KP / 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      A.a[i] += rec[4 * sub + i];
      A.b[i] += rec[KP + 4 * sub + i];
    }
    A.q += rec[2 * KP];
    A.n += rec[2 * KP + 1];
  }

  // r = G·x + a + λ n x − b (KKT form when nonnegative), the norms and eta of dst row `row`; a row of
  // degree 0 (not an ingested row) gets its eta from G·x alone
  template <int KP>
  __device__ static void finish_row(const Args& g, int64_t row, int64_t, const float4 xf, const Acc& A,
                                    const double* gx) {
    constexpr int L = KP / 4;
    const int lane = threadIdx.x & 63, sub = lane % L;
    const double x[4] = {xf.x, xf.y, xf.z, xf.w};
    const double ln = g.reg * A.n;
    double rr = 0.0, xx = 0.0, bb = 0.0;
    bool neg = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double r = (gx ? gx[4 * sub + i] : 0.0) + A.a[i] + ln * x[i] - A.b[i];
      if (g.nonneg) {
        if (!(x[i] > 0.0) && r > 0.0) r = 0.0;  // min(r, 0) off the support; a NaN stays
        neg = neg || x[i] < 0.0;
      }
      rr += r * r;
      xx += x[i] * x[i];
      bb += A.b[i] * A.b[i];
    }
    rr = lanes_sum<1, L>(rr);
    xx = lanes_sum<1, L>(xx);
    bb = lanes_sum<1, L>(bb);
    const bool any_neg = __any(neg);
    if (lane != 0) return;
    const double s = (g.gnorm + A.q + ln) * sqrt(xx) + sqrt(bb);
    g.eta[row] = s == 0.0 ? 0.0 : sqrt(rr) / s;
    g.neg[row] = any_neg ? 1 : 0;
  }
};

// ---- summary -------------------------------------------------------------------------------------------
// a ranks above b: a non-finite eta above every finite one, then the larger eta, then the lower row
__device__ inline bool worse(double ea, int64_t ia, double eb, int64_t ib) {
  if (ib < 0) return ia >= 0;
  if (ia < 0) return false;
  const bool na = !isfinite(ea), nb = !isfinite(eb);
  if (na != nb) return na;
  if (!na && ea != eb) return ea > eb;
  return ia < ib;
}

__device__ inline void merge(AuditSummary& a, const AuditSummary& b) {
  a.over += b.over;
  a.non_finite += b.non_finite;
  a.negative += b.negative;
  a.sum += b.sum;
  if (worse(b.worst_eta, b.worst_row, a.worst_eta, a.worst_row)) {
    a.worst_eta = b.worst_eta;
    a.worst_row = b.worst_row;
  }
}

// Pass 1 (part = null): block b sums rows [b·per, (b + 1)·per) of eta / neg into out[b].
// Pass 2 (one block): the n records of `part` into out[0].  Both add in a fixed order.
__global__ __launch_bounds__(256) void audit_sum_kernel(const double* __restrict__ eta, const int32_t* __restrict__ neg,
                                                        const AuditSummary* __restrict__ part, int64_t n, int64_t per,
                                                        double tol, AuditSummary* __restrict__ out) {
  __shared__ AuditSummary sh[256];
  AuditSummary s{0, 0, 0, -1, 0.0, 0.0};
  const int64_t b0 = part ? 0 : (int64_t)blockIdx.x * per;
  const int64_t b1 = b0 + per < n ? b0 + per : n;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) {
    if (part) {
      merge(s, part[i]);
      continue;
    }
    const double e = eta[i];
    const AuditSummary one{!(e <= tol) ? 1 : 0, !isfinite(e) ? 1 : 0, neg[i] != 0 ? 1 : 0, i, e, e};
    merge(s, one);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) merge(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

}  // namespace

int audit_gram_blocks(int64_t n) { return (int)(n < 256 ? 1 : (n / 256 > 128 ? 128 : n / 256)); }

hipError_t launch_audit_gram(int KP, const float* X, int64_t n, double* slab, int nblk, double* G, hipStream_t s) {
  return for_kp(KP, [&](auto kp) {
    constexpr int K = decltype(kp)::value;
    const int64_t per = (n + nblk - 1) / nblk;
    audit_gram_kernel<K><<<dim3(nblk, K / 64, K / 64), 256, 0, s>>>(X, n, per, slab);
    const int64_t kk = (int64_t)K * K;
    audit_gram_reduce_kernel<<<(unsigned)((kk + 255) / 256), 256, 0, s>>>(slab, nblk, kk, G);
    return hipGetLastError();
  });
}

hipError_t launch_row_gx(int KP, const float* X, const double* G, double* GX, int64_t row0, int64_t nb, hipStream_t s) {
  return for_kp(KP, [&](auto kp) {
    constexpr int K = decltype(kp)::value;
    row_gx_kernel<K><<<dim3((unsigned)((nb + 63) / 64), K / 64), 256, 0, s>>>(X, G, GX, row0, nb);
    return hipGetLastError();
  });
}

hipError_t launch_audit_chunks(int KP, const AuditArgs& g, hipStream_t s) { return row_pass_chunks<AuditPass>(KP, g, s); }

hipError_t launch_audit_rows(int KP, const AuditArgs& g, int64_t l0, int64_t n_long, hipStream_t s) {
  return row_pass_batch<AuditPass>(KP, g, l0, n_long, s);
}

hipError_t launch_audit_summary(const double* eta, const int32_t* neg, int64_t n, double tol, AuditSummary* part,
                                AuditSummary* out, hipStream_t s) {
  const int64_t nblk = n <= 0 ? 1 : (n + 4095) / 4096 < AUDIT_SUM_BLOCKS ? (n + 4095) / 4096 : AUDIT_SUM_BLOCKS;
  const int64_t per = n <= 0 ? 0 : (n + nblk - 1) / nblk;
  audit_sum_kernel<<<(unsigned)nblk, 256, 0, s>>>(eta, neg, nullptr, n, per, tol, part);
  audit_sum_kernel<<<1, 256, 0, s>>>(nullptr, nullptr, part, nblk, nblk, tol, out);
  return hipGetLastError();
}

}  // namespace albedo
