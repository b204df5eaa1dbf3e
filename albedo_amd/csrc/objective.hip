// als_objective: the loss ALS minimises, in fp64, from the current factors of both sides in the original
// basis (include/albedo_als.h).  For dst row j with factors x, per rating r on src row y with s = x·y
//   implicit:  c = α|r|, w = (r > 0 ? 1 + c : 0),  t = c s² − 2 w s + w,  n = #(r > 0),  G = Σ y yᵀ (all src rows)
//   explicit:  t = (r − s)²,                                               n = degree,    G = 0
//   loss_j = xᵀ G x + Σ t + λ n ‖x‖²,   total = Σ_j loss_j + λ Σ_i n_i ‖y_i‖²
// One pass over the CSR with the gather of the row audit, O(nnz·k), and no k x k build.
//
// Like audit.hip this is a yardstick of the solve kernels and shares nothing with them: plain HIP, no
// inline asm, no MFMA, none of device_common.h.  Everything is fp64 arithmetic on the fp32 factors and
// ratings; nothing is added by a floating-point atomic, every sum has one fixed order.
//
// Layout (audit.hip's).  A wave is cut into groups of KP/4 lanes; a lane holds 4 consecutive components
// (one 16-byte load of a factor row), so a group covers one src row and a wave gathers 64 / (KP/4) = 4, 2
// or 1 src rows per step.  OBJ_UNROLL steps are loaded before any is used.  Per rating the group reduces
// s across its lanes (shuffles of doubles) and adds to four scalars: Σ t, Σ (r − s)², Σ |terms| and n.
// The audit keeps 2·4 + 2 doubles per lane for its vectors, this kernel four.
//   objective_gx_kernel        G·x of a batch of dst rows (a tiled fp64 product; per row it would re-read G)
//   objective_rows_kernel      one wave per dst row of at most `chunk` ratings, start to its record
//   objective_chunk_kernel     longer rows: one wave per chunk of `chunk` ratings -> 4 doubles
//   objective_long_kernel      one wave per long row: its chunk records added in chunk order, then the record
//   objective_other_kernel     one wave per src row: n_i ‖y_i‖² from that side's own ratings
//   objective_colsum_kernel    (twice per table) column sums of a table of doubles, in a fixed order
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace albedo {

namespace {

constexpr int OBJ_WAVES = 4;   // waves (dst rows or chunks) per workgroup
constexpr int OBJ_UNROLL = 4;  // gather steps in flight per wave

// ---- G·x -----------------------------------------------------------------------------------------------
// GX[r][m] = Σ_l X[row0 + r][l]·G[l][m] for r < nb over 64 x 64 tiles of GX, 16 l at a time in LDS, a
// 4 x 4 block per thread (256 threads); grid (ceil(nb / 64), KP/64)
template <int KP>
__global__ __launch_bounds__(256) void objective_gx_kernel(const float* __restrict__ X, const double* __restrict__ G,
                                                           double* __restrict__ GX, int64_t row0, int64_t nb) {
  __shared__ double ta[16][64 + 4];  // X, l-major; + 4: the transposing store walks a column
  __shared__ double tb[16][64];      // G
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int m0 = blockIdx.y * 64;
  double acc[4][4] = {};
  for (int l0 = 0; l0 < KP; l0 += 16) {
    {
      const int r = threadIdx.x >> 2, l4 = (threadIdx.x & 3) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < nb) v = *reinterpret_cast<const float4*>(X + (row0 + r0 + r) * KP + l0 + l4);
      ta[l4 + 0][r] = v.x, ta[l4 + 1][r] = v.y, ta[l4 + 2][r] = v.z, ta[l4 + 3][r] = v.w;
      const int l = threadIdx.x >> 4, m4 = (threadIdx.x & 15) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) tb[l][m4 + i] = G[(size_t)(l0 + l) * KP + m0 + m4 + i];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = ta[k][4 * ty + i];
        bv[i] = tb[k][4 * tx + i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
    }
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
// A lane's sums over the ratings its group took; after group_sums() the row's (or chunk's) totals
struct Acc {
  double t = 0.0;    // Σ t_r
  double sse = 0.0;  // Σ (r − s)²
  double abs = 0.0;  // Σ |c s²| + |2 w s| + |w|   (explicit: Σ t_r)
  double n = 0.0;    // implicit: ratings > 0; explicit: the degree
};

template <int FROM, int TO>
__device__ inline double lanes_sum(double v) {  // butterfly over the lane bits FROM <= 2^s < TO
#pragma unroll
  for (int o = FROM; o < TO; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ratings [p0, p1) of one dst row whose factors are x (this lane's 4 components)
template <int KP>
__device__ inline void accumulate(const ObjectiveArgs& g, int64_t p0, int64_t p1, const float4 xf, Acc& A) {
  constexpr int L = KP / 4, NG = 64 / L;
  const int lane = threadIdx.x & 63, sub = lane % L, grp = lane / L;
  const double x0 = xf.x, x1 = xf.y, x2 = xf.z, x3 = xf.w;
  for (int64_t base = p0; base < p1; base += NG * OBJ_UNROLL) {  // wave-uniform: the shuffles need every lane
    int32_t col[OBJ_UNROLL];
    float r[OBJ_UNROLL];
    float4 y[OBJ_UNROLL];
#pragma unroll
    for (int u = 0; u < OBJ_UNROLL; ++u) {
      const int64_t p = base + u * NG + grp;
      col[u] = p < p1 ? g.col[p] : -1;
      r[u] = p < p1 ? g.val[p] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < OBJ_UNROLL; ++u)
      y[u] = col[u] >= 0 ? *reinterpret_cast<const float4*>(g.Y + (int64_t)col[u] * KP + 4 * sub)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < OBJ_UNROLL; ++u) {
      const double y0 = y[u].x, y1 = y[u].y, y2 = y[u].z, y3 = y[u].w;
      const double s = lanes_sum<1, L>(y0 * x0 + y1 * x1 + y2 * x2 + y3 * x3);
      const double e = (double)r[u] - s;
      double t = e * e, a = t, pos = 1.0;
      if (g.implicit) {
        const double c = g.alpha * (double)fabsf(r[u]);
        const double w = r[u] > 0.f ? 1.0 + c : 0.0;
        const double cs2 = c * s * s, ws2 = 2.0 * w * s;
        t = cs2 - ws2 + w;
        a = fabs(cs2) + fabs(ws2) + w;
        pos = r[u] > 0.f ? 1.0 : 0.0;
      }
      if (col[u] >= 0) {  // past the row's end there is nothing to add
        A.t += t;
        A.sse += e * e;
        A.abs += a;
        A.n += pos;
      }
    }
  }
}

// the groups of a wave took different ratings; the lanes of a group hold equal sums
template <int KP>
__device__ inline void group_sums(Acc& A) {
  constexpr int L = KP / 4;
  A.t = lanes_sum<L, 64>(A.t);
  A.sse = lanes_sum<L, 64>(A.sse);
  A.abs = lanes_sum<L, 64>(A.abs);
  A.n = lanes_sum<L, 64>(A.n);
}

// the record of dst row `row`: xᵀGx from G·x (gx, null when explicit), the regulariser and the loss
template <int KP>
__device__ inline void finish_row(const ObjectiveArgs& g, int64_t row, int64_t degree, const float4 xf, const Acc& A,
                                  const double* gx) {
  constexpr int L = KP / 4;
  const int lane = threadIdx.x & 63, sub = lane % L;
  const double x[4] = {xf.x, xf.y, xf.z, xf.w};
  double xx = 0.0, xgx = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xx += x[i] * x[i];
    if (gx) xgx += gx[4 * sub + i] * x[i];
  }
  xx = lanes_sum<1, L>(xx);
  xgx = lanes_sum<1, L>(xgx);
  if (lane != 0) return;
  const double reg = g.reg * A.n * xx;
  double* rec = g.rec + row * OBJ_REC;
  rec[OBJ_ALL_PAIRS] = xgx;
  rec[OBJ_RATINGS] = A.t;
  rec[OBJ_REG] = reg;
  rec[OBJ_SSE] = A.sse;
  rec[OBJ_ABS] = fabs(xgx) + A.abs + fabs(reg);
  rec[OBJ_DEGREE] = (double)degree;
  rec[OBJ_LOSS] = xgx + A.t + reg;
  rec[OBJ_REC - 1] = 0.0;
}

template <int KP>
__device__ inline float4 load_x(const ObjectiveArgs& g, int64_t row) {
  return *reinterpret_cast<const float4*>(g.X + row * KP + 4 * ((threadIdx.x & 63) % (KP / 4)));
}

template <int KP>
__global__ __launch_bounds__(64 * OBJ_WAVES) void objective_rows_kernel(const ObjectiveArgs g) {
  const int64_t i = (int64_t)blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
  if (i >= g.nb) return;
  const int64_t row = g.row0 + i;
  const int64_t p0 = g.ptr[row], p1 = g.ptr[row + 1];
  if (p1 - p0 > g.chunk) return;  // objective_chunk_kernel + objective_long_kernel
  const float4 xf = load_x<KP>(g, row);
  Acc A;
  accumulate<KP>(g, p0, p1, xf, A);
  group_sums<KP>(A);
  finish_row<KP>(g, row, p1 - p0, xf, A, g.GX ? g.GX + i * KP : nullptr);
}

// partial record of chunk ci: Σ t, Σ (r − s)², Σ |terms|, n
template <int KP>
__global__ __launch_bounds__(64 * OBJ_WAVES) void objective_chunk_kernel(const ObjectiveArgs g) {
  const int64_t ci = (int64_t)blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
  if (ci >= g.n_chunks) return;
  const int64_t row = g.chunk_row[ci];
  const int64_t p0 = g.ptr[row] + (int64_t)g.chunk_idx[ci] * g.chunk;
  const int64_t pe = g.ptr[row + 1], p1 = p0 + g.chunk < pe ? p0 + g.chunk : pe;
  Acc A;
  accumulate<KP>(g, p0, p1, load_x<KP>(g, row), A);
  group_sums<KP>(A);
  if ((threadIdx.x & 63) != 0) return;
  double* rec = g.partial + (size_t)ci * OBJ_CHUNK_REC;
  rec[0] = A.t, rec[1] = A.sse, rec[2] = A.abs, rec[3] = A.n;
}

// long rows [l0, l0 + n_long) of the list, all inside the batch [row0, row0 + nb)
template <int KP>
__global__ __launch_bounds__(64 * OBJ_WAVES) void objective_long_kernel(const ObjectiveArgs g, int64_t l0, int64_t n_long) {
  const int64_t li = (int64_t)blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
  if (li >= n_long) return;
  const int64_t row = g.long_row[l0 + li];
  Acc A;
  for (int64_t ci = g.long_slot0[l0 + li]; ci < g.long_slot0[l0 + li + 1]; ++ci) {  // chunk order
    const double* rec = g.partial + (size_t)ci * OBJ_CHUNK_REC;
    A.t += rec[0], A.sse += rec[1], A.abs += rec[2], A.n += rec[3];
  }
  finish_row<KP>(g, row, g.ptr[row + 1] - g.ptr[row], load_x<KP>(g, row), A,
                 g.GX ? g.GX + (row - g.row0) * KP : nullptr);
}

// out[i] = n_i·‖y_i‖² of row i of the other side, n_i from that side's own ratings (val null: the degree)
template <int KP>
__global__ __launch_bounds__(64 * OBJ_WAVES) void objective_other_kernel(const float* __restrict__ Y,
                                                                          const int64_t* __restrict__ ptr,
                                                                          const float* __restrict__ val, int64_t n,
                                                                          double* __restrict__ out) {
  constexpr int L = KP / 4;
  const int64_t i = (int64_t)blockIdx.x * OBJ_WAVES + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const int64_t p0 = ptr[i], p1 = ptr[i + 1];
  long long cnt = p1 - p0;
  if (val) {  // a count of integers: any order gives the same number
    int mine = 0;
    for (int64_t p = p0 + lane; p < p1; p += 64) mine += val[p] > 0.f ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mine += __shfl_xor(mine, o, 64);
    cnt = mine;
  }
  double yy = 0.0;
  if (lane < L) {
    const float4 v = *reinterpret_cast<const float4*>(Y + i * KP + 4 * lane);
    const double y0 = v.x, y1 = v.y, y2 = v.z, y3 = v.w;
    yy = y0 * y0 + y1 * y1 + y2 * y2 + y3 * y3;
  }
  yy = lanes_sum<1, 64>(yy);
  if (lane == 0) out[i] = (double)cnt * yy;
}

// out[blockIdx.x][w] = Σ of column w over rows [b·per, (b + 1)·per) of in [n][W], W <= OBJ_REC: each thread
// adds its rows in ascending order, then the threads are added in a fixed tree
__global__ __launch_bounds__(256) void objective_colsum_kernel(const double* __restrict__ in, int64_t n, int W,
                                                               int64_t per, double* __restrict__ out) {
  __shared__ double sh[256][OBJ_REC + 1];
  const int64_t b0 = (int64_t)blockIdx.x * per;
  const int64_t b1 = b0 + per < n ? b0 + per : n;
  double s[OBJ_REC];
#pragma unroll
  for (int w = 0; w < OBJ_REC; ++w) s[w] = 0.0;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256)
#pragma unroll
    for (int w = 0; w < OBJ_REC; ++w)
      if (w < W) s[w] += in[i * W + w];
#pragma unroll
  for (int w = 0; w < OBJ_REC; ++w) sh[threadIdx.x][w] = s[w];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int w = 0; w < OBJ_REC; ++w) sh[threadIdx.x][w] += sh[threadIdx.x + o][w];
    __syncthreads();
  }
  if ((int)threadIdx.x < W) out[(size_t)blockIdx.x * W + threadIdx.x] = sh[0][threadIdx.x];
}

template <int KP>
hipError_t rows_launch(const ObjectiveArgs& g, int64_t l0, int64_t n_long, hipStream_t s) {
  const int64_t wg = (g.nb + OBJ_WAVES - 1) / OBJ_WAVES;
  if (g.GX)
    objective_gx_kernel<KP><<<dim3((unsigned)((g.nb + 63) / 64), KP / 64), 256, 0, s>>>(g.X, g.G, g.GX, g.row0, g.nb);
  objective_rows_kernel<KP><<<(unsigned)wg, 64 * OBJ_WAVES, 0, s>>>(g);
  if (n_long > 0)
    objective_long_kernel<KP><<<(unsigned)((n_long + OBJ_WAVES - 1) / OBJ_WAVES), 64 * OBJ_WAVES, 0, s>>>(g, l0, n_long);
  return hipGetLastError();
}

template <int KP>
hipError_t chunks_launch(const ObjectiveArgs& g, hipStream_t s) {
  objective_chunk_kernel<KP><<<(unsigned)((g.n_chunks + OBJ_WAVES - 1) / OBJ_WAVES), 64 * OBJ_WAVES, 0, s>>>(g);
  return hipGetLastError();
}

template <int KP>
hipError_t other_launch(const float* Y, const int64_t* ptr, const float* val, int64_t n, double* out, hipStream_t s) {
  objective_other_kernel<KP><<<(unsigned)((n + OBJ_WAVES - 1) / OBJ_WAVES), 64 * OBJ_WAVES, 0, s>>>(Y, ptr, val, n, out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_objective_chunks(int KP, const ObjectiveArgs& g, hipStream_t s) {
  if (g.n_chunks <= 0) return hipSuccess;
  if (KP == 64) return chunks_launch<64>(g, s);
  if (KP == 128) return chunks_launch<128>(g, s);
  if (KP == 256) return chunks_launch<256>(g, s);
  return hipErrorInvalidValue;
}

hipError_t launch_objective_rows(int KP, const ObjectiveArgs& g, int64_t l0, int64_t n_long, hipStream_t s) {
  if (g.nb <= 0) return hipSuccess;
  if (KP == 64) return rows_launch<64>(g, l0, n_long, s);
  if (KP == 128) return rows_launch<128>(g, l0, n_long, s);
  if (KP == 256) return rows_launch<256>(g, l0, n_long, s);
  return hipErrorInvalidValue;
}

hipError_t launch_objective_other(int KP, const float* Y, const int64_t* ptr, const float* val, int64_t n, double* out,
                                  hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (KP == 64) return other_launch<64>(Y, ptr, val, n, out, s);
  if (KP == 128) return other_launch<128>(Y, ptr, val, n, out, s);
  if (KP == 256) return other_launch<256>(Y, ptr, val, n, out, s);
  return hipErrorInvalidValue;
}

hipError_t launch_objective_colsum(const double* in, int64_t n, int W, double* part, double* out, hipStream_t s) {
  if (W < 1 || W > OBJ_REC) return hipErrorInvalidValue;
  const int64_t nblk = n <= 0 ? 1 : (n + 4095) / 4096 < OBJ_SUM_BLOCKS ? (n + 4095) / 4096 : OBJ_SUM_BLOCKS;
  const int64_t per = n <= 0 ? 0 : (n + nblk - 1) / nblk;
  objective_colsum_kernel<<<(unsigned)nblk, 256, 0, s>>>(in, n, W, per, part);
  objective_colsum_kernel<<<1, 256, 0, s>>>(part, nblk, W, nblk, out);
  return hipGetLastError();
}

}  // namespace albedo
