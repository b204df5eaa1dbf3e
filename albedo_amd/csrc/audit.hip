// als_audit_rows: the normal-equation residual of every dst row, in fp64, from the current factors of
// both sides in the original basis (include/albedo_als.h).  For dst row j with factors x
//   r = G·x + Σ_i c_i (y_i·x) y_i + λ n x − b,   b = Σ_i w_i y_i
//   eta = ‖r‖₂ / ((‖G‖_F + Σ_i c_i ‖y_i‖² + λ n)·‖x‖₂ + ‖b‖₂)        (0 when the denominator is 0)
// which needs no k x k build: one pass over the CSR with the gather of the solve's build, O(nnz·k).
//
// This file is the yardstick of the solve kernels, so it shares nothing with them: plain HIP, no inline
// asm, no MFMA, none of device_common.h.  Everything is fp64 arithmetic on the fp32 factors and ratings.
//
// Layout.  A wave is cut into groups of KP/4 lanes; a lane holds 4 consecutive components (one 16-byte
// load of a factor row), so a group covers one src row and a wave gathers 64 / (KP/4) = 4, 2 or 1 src
// rows per step (KP = 64, 128, 256).  AUDIT_UNROLL steps are loaded before any is used: the row gathers
// are the cost, and their addresses depend only on the column indices, which are loaded together too.
// Per rating the group reduces t = y·x across its lanes (shuffles of doubles) and every lane adds c·t·y
// and w·y for its components and c·y² for the norm term; the groups are summed once per row.
//   audit_gram_kernel / audit_gram_reduce_kernel   G = Σ y yᵀ in fp64 (launch_gram's 64-row fp32
//                              partials leave G at 1e-7, four decades above what the audit resolves)
//   audit_gx_kernel            G·x of a batch of dst rows (a tiled fp64 GEMM; per row it would re-read G)
//   audit_rows_kernel          one wave per dst row of at most `chunk` ratings, start to eta
//   audit_chunk_kernel         longer rows: one wave per chunk of `chunk` ratings -> an fp64 partial record
//   audit_long_kernel          one wave per long row: its records added in chunk order (deterministic, no
//                              float atomics), then G·x + λ n x − b and the norms like any other row
//   audit_sum_kernel (twice)   the summary: counts, the worst row and the sum, in a fixed order
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace albedo {

namespace {

constexpr int AUDIT_WAVES = 4;   // waves (dst rows or chunks) per workgroup
constexpr int AUDIT_UNROLL = 4;  // gather steps in flight per wave

// ---- tiled fp64 products -----------------------------------------------------------------------------
// Both products are C[i][j] = Σ_k A[k][i]·B[k][j] over 64 x 64 tiles of C with 16 k at a time in LDS and
// a 4 x 4 block of C per thread (256 threads).
struct Tile {
  double a[16][64 + 4];  // + 4: the transposing store of audit_gx_kernel walks a column
  double b[16][64];
};

__device__ inline void tile_fma(const Tile& t, int ty, int tx, double (&acc)[4][4]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    double av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      av[i] = t.a[k][4 * ty + i];
      bv[i] = t.b[k][4 * tx + i];
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
    tile_fma(t, ty, tx, acc);
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

// GX[r][m] = Σ_l X[row0 + r][l]·G[l][m] for r < nb; grid (ceil(nb / 64), KP/64)
template <int KP>
__global__ __launch_bounds__(256) void audit_gx_kernel(const float* __restrict__ X, const double* __restrict__ G,
                                                       double* __restrict__ GX, int64_t row0, int64_t nb) {
  __shared__ Tile t;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int m0 = blockIdx.y * 64;
  double acc[4][4] = {};
  for (int l0 = 0; l0 < KP; l0 += 16) {
    {  // 64 rows x 16 l of X, stored l-major; 16 l x 64 m of G
      const int r = threadIdx.x >> 2, l4 = (threadIdx.x & 3) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < nb) v = *reinterpret_cast<const float4*>(X + (row0 + r0 + r) * KP + l0 + l4);
      t.a[l4 + 0][r] = v.x, t.a[l4 + 1][r] = v.y, t.a[l4 + 2][r] = v.z, t.a[l4 + 3][r] = v.w;
      const int l = threadIdx.x >> 4, m4 = (threadIdx.x & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) t.b[l][m4 + i] = G[(size_t)(l0 + l) * KP + m0 + m4 + i];
    }
    __syncthreads();
    tile_fma(t, ty, tx, acc);
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

// ---- per-row accumulation ------------------------------------------------------------------------------
// What a lane holds for its 4 components of a dst row, after group_sums() the row's (or chunk's) totals
struct Acc {
  double a[4] = {0.0, 0.0, 0.0, 0.0};  // Σ c (y·x) y
  double b[4] = {0.0, 0.0, 0.0, 0.0};  // Σ w y
  double q = 0.0;                      // Σ c ‖y‖²
  double n = 0.0;                      // implicit: ratings > 0; explicit: the degree
};

template <int FROM, int TO>
__device__ inline double lanes_sum(double v) {  // butterfly over the lane bits FROM <= 2^s < TO
#pragma unroll
  for (int o = FROM; o < TO; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ratings [p0, p1) of one dst row whose factors are x (this lane's 4 components)
template <int KP>
__device__ inline void accumulate(const AuditArgs& g, int64_t p0, int64_t p1, const float4 xf, Acc& A) {
  constexpr int L = KP / 4, NG = 64 / L;
  const int lane = threadIdx.x & 63, sub = lane % L, grp = lane / L;
  const double x0 = xf.x, x1 = xf.y, x2 = xf.z, x3 = xf.w;
  for (int64_t base = p0; base < p1; base += NG * AUDIT_UNROLL) {  // wave-uniform: the shuffles need every lane
    int32_t col[AUDIT_UNROLL];
    float r[AUDIT_UNROLL];
    float4 y[AUDIT_UNROLL];
#pragma unroll
    for (int u = 0; u < AUDIT_UNROLL; ++u) {
      const int64_t p = base + u * NG + grp;
      col[u] = p < p1 ? g.col[p] : -1;
      r[u] = p < p1 ? g.val[p] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < AUDIT_UNROLL; ++u)
      y[u] = col[u] >= 0 ? *reinterpret_cast<const float4*>(g.Y + (int64_t)col[u] * KP + 4 * sub)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < AUDIT_UNROLL; ++u) {
      const bool live = col[u] >= 0;
      double c, w, pos;
      if (g.implicit) {
        c = g.alpha * (double)fabsf(r[u]);
        w = r[u] > 0.f ? 1.0 + c : 0.0;
        pos = r[u] > 0.f ? 1.0 : 0.0;
      } else {
        c = live ? 1.0 : 0.0;
        w = (double)r[u];
        pos = c;
      }
      const double y0 = y[u].x, y1 = y[u].y, y2 = y[u].z, y3 = y[u].w;
      const double t = lanes_sum<1, L>(y0 * x0 + y1 * x1 + y2 * x2 + y3 * x3);
      const double ct = c * t;
      A.a[0] += ct * y0, A.a[1] += ct * y1, A.a[2] += ct * y2, A.a[3] += ct * y3;
      A.b[0] += w * y0, A.b[1] += w * y1, A.b[2] += w * y2, A.b[3] += w * y3;
      A.q += c * (y0 * y0 + y1 * y1 + y2 * y2 + y3 * y3);
      A.n += pos;
    }
  }
}

// the groups of a wave took different ratings: every lane ends with the totals of its components
template <int KP>
__device__ inline void group_sums(Acc& A) {
  constexpr int L = KP / 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    A.a[i] = lanes_sum<L, 64>(A.a[i]);
    A.b[i] = lanes_sum<L, 64>(A.b[i]);
  }
  A.n = lanes_sum<L, 64>(A.n);
  A.q = lanes_sum<1, 64>(A.q);  // a lane's part covers its components only
}

// r = G·x + a + λ n x − b (KKT form when nonnegative), the norms and eta of dst row `row`
template <int KP>
__device__ inline void finish_row(const AuditArgs& g, int64_t row, const float4 xf, const Acc& A, const double* gx) {
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

template <int KP>
__device__ inline float4 load_x(const AuditArgs& g, int64_t row) {
  return *reinterpret_cast<const float4*>(g.X + row * KP + 4 * ((threadIdx.x & 63) % (KP / 4)));
}

template <int KP>
__global__ __launch_bounds__(64 * AUDIT_WAVES) void audit_rows_kernel(const AuditArgs g) {
  const int64_t i = (int64_t)blockIdx.x * AUDIT_WAVES + (threadIdx.x >> 6);
  if (i >= g.nb) return;
  const int64_t row = g.row0 + i;
  const int64_t p0 = g.ptr[row], p1 = g.ptr[row + 1];
  if (p1 - p0 > g.chunk) return;  // audit_chunk_kernel + audit_long_kernel
  const float4 xf = load_x<KP>(g, row);
  Acc A;
  accumulate<KP>(g, p0, p1, xf, A);  // degree 0 (not an ingested row): nothing to add, eta from G·x alone
  group_sums<KP>(A);
  finish_row<KP>(g, row, xf, A, g.GX ? g.GX + i * KP : nullptr);
}

// partial record of chunk ci: a[KP], b[KP], q, n
template <int KP>
__global__ __launch_bounds__(64 * AUDIT_WAVES) void audit_chunk_kernel(const AuditArgs g) {
  constexpr int L = KP / 4;
  const int64_t ci = (int64_t)blockIdx.x * AUDIT_WAVES + (threadIdx.x >> 6);
  if (ci >= g.n_chunks) return;
  const int64_t row = g.chunk_row[ci];
  const int64_t p0 = g.ptr[row] + (int64_t)g.chunk_idx[ci] * g.chunk;
  const int64_t pe = g.ptr[row + 1], p1 = p0 + g.chunk < pe ? p0 + g.chunk : pe;
  Acc A;
  accumulate<KP>(g, p0, p1, load_x<KP>(g, row), A);
  group_sums<KP>(A);
  const int lane = threadIdx.x & 63;
  double* rec = g.partial + (size_t)ci * (2 * KP + 2);
  if (lane < L) {
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

// long rows [l0, l0 + n_long) of the list, all inside the batch [row0, row0 + nb)
template <int KP>
__global__ __launch_bounds__(64 * AUDIT_WAVES) void audit_long_kernel(const AuditArgs g, int64_t l0, int64_t n_long) {
  constexpr int L = KP / 4;
  const int64_t li = (int64_t)blockIdx.x * AUDIT_WAVES + (threadIdx.x >> 6);
  if (li >= n_long) return;
  const int64_t row = g.long_row[l0 + li];
  const int sub = (threadIdx.x & 63) % L;
  Acc A;
  for (int64_t ci = g.long_slot0[l0 + li]; ci < g.long_slot0[l0 + li + 1]; ++ci) {  // chunk order
    const double* rec = g.partial + (size_t)ci * (2 * KP + 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      A.a[i] += rec[4 * sub + i];
      A.b[i] += rec[KP + 4 * sub + i];
    }
    A.q += rec[2 * KP];
    A.n += rec[2 * KP + 1];
  }
  finish_row<KP>(g, row, load_x<KP>(g, row), A, g.GX ? g.GX + (row - g.row0) * KP : nullptr);
}

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

template <int KP>
hipError_t audit_launch(const AuditArgs& g, int64_t l0, int64_t n_long, hipStream_t s) {
  const int64_t wg = (g.nb + AUDIT_WAVES - 1) / AUDIT_WAVES;
  if (g.GX)
    audit_gx_kernel<KP><<<dim3((unsigned)((g.nb + 63) / 64), KP / 64), 256, 0, s>>>(g.X, g.G, g.GX, g.row0, g.nb);
  audit_rows_kernel<KP><<<(unsigned)wg, 64 * AUDIT_WAVES, 0, s>>>(g);
  if (n_long > 0)
    audit_long_kernel<KP><<<(unsigned)((n_long + AUDIT_WAVES - 1) / AUDIT_WAVES), 64 * AUDIT_WAVES, 0, s>>>(g, l0, n_long);
  return hipGetLastError();
}

template <int KP>
hipError_t chunks_launch(const AuditArgs& g, hipStream_t s) {
  audit_chunk_kernel<KP><<<(unsigned)((g.n_chunks + AUDIT_WAVES - 1) / AUDIT_WAVES), 64 * AUDIT_WAVES, 0, s>>>(g);
  return hipGetLastError();
}

template <int KP>
hipError_t gram_launch(const float* X, int64_t n, double* slab, int nblk, double* G, hipStream_t s) {
  const int64_t per = (n + nblk - 1) / nblk;
  audit_gram_kernel<KP><<<dim3(nblk, KP / 64, KP / 64), 256, 0, s>>>(X, n, per, slab);
  const int64_t kk = (int64_t)KP * KP;
  audit_gram_reduce_kernel<<<(unsigned)((kk + 255) / 256), 256, 0, s>>>(slab, nblk, kk, G);
  return hipGetLastError();
}

}  // namespace

int audit_gram_blocks(int64_t n) { return (int)(n < 256 ? 1 : (n / 256 > 128 ? 128 : n / 256)); }

hipError_t launch_audit_gram(int KP, const float* X, int64_t n, double* slab, int nblk, double* G, hipStream_t s) {
  if (KP == 64) return gram_launch<64>(X, n, slab, nblk, G, s);
  if (KP == 128) return gram_launch<128>(X, n, slab, nblk, G, s);
  if (KP == 256) return gram_launch<256>(X, n, slab, nblk, G, s);
  return hipErrorInvalidValue;
}

hipError_t launch_audit_chunks(int KP, const AuditArgs& g, hipStream_t s) {
  if (g.n_chunks <= 0) return hipSuccess;
  if (KP == 64) return chunks_launch<64>(g, s);
  if (KP == 128) return chunks_launch<128>(g, s);
  if (KP == 256) return chunks_launch<256>(g, s);
  return hipErrorInvalidValue;
}

hipError_t launch_audit_rows(int KP, const AuditArgs& g, int64_t l0, int64_t n_long, hipStream_t s) {
  if (g.nb <= 0) return hipSuccess;
  if (KP == 64) return audit_launch<64>(g, l0, n_long, s);
  if (KP == 128) return audit_launch<128>(g, l0, n_long, s);
  if (KP == 256) return audit_launch<256>(g, l0, n_long, s);
  return hipErrorInvalidValue;
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
