// als_objective: the loss ALS minimises, in fp64, from the current factors of both sides in the original
// basis (include/albedo_als.h).  For dst row j with factors x, per rating r on src row y with s = x·y
//   implicit:  c = α|r|, w = (r > 0 ? 1 + c : 0),  t = c s² − 2 w s + w,  n = #(r > 0),  G = Σ y yᵀ (all src rows)
//   explicit:  t = (r − s)²,                                               n = degree,    G = 0
//   loss_j = xᵀ G x + Σ t + λ n ‖x‖²,   total = Σ_j loss_j + λ Σ_i n_i ‖y_i‖²
// One pass over the CSR with the gather of the row audit, O(nnz·k), and no k x k build.
//
// Like audit.hip this is a yardstick of the solve kernels and shares nothing with them: plain HIP, no
// inline asm, no MFMA, none of device_common.h.  With audit.hip it shares the row pass (row_pass.h: the
// gather, the three row kernels and their launches), G·x (launch_row_gx) and the fp64 Gram.  Everything
// is fp64 arithmetic on the fp32 factors and ratings; nothing is added by a floating-point atomic, every
// sum has one fixed order.
//
// Per rating the pass hands over s and a lane adds to four scalars: Σ t, Σ (r − s)², Σ |terms| and n.
// The audit keeps 2·4 + 2 doubles per lane for its vectors, this pass four; a chunk's record is 4 doubles.
//   objective_other_kernel     one wave per src row: n_i ‖y_i‖² from that side's own ratings
//   objective_colsum_kernel    (twice per table) column sums of a table of doubles, in a fixed order
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "row_pass.h"

namespace albedo {

namespace {

// ---- the objective's row pass (row_pass.h) -------------------------------------------------------------
struct ObjectivePass {
  using Args = ObjectiveArgs;
  // A lane's sums over the ratings its group took; after group_sums() the row's (or chunk's) totals
  struct Acc {
    double t = 0.0;    // Σ t_r
    double sse = 0.0;  // Σ (r − s)²
    double abs = 0.0;  // Σ |c s²| + |2 w s| + |w|   (explicit: Σ t_r)
    double n = 0.0;    // implicit: ratings > 0; explicit: the degree
  };
  template <int KP>
  static constexpr int rec_doubles = OBJ_CHUNK_REC;  // a chunk's record: Σ t, Σ (r − s)², Σ |terms|, n

  struct W {};  // nothing ahead of s
  __device__ static W weigh(const Args&, bool, float) { return {}; }

  __device__ static void add(const Args& g, Acc& A, const W&, bool live, float r, double, double, double, double,
                             double s) {
    const double e = (double)r - s;
    double t = e * e, a = t, pos = 1.0;
    if (g.implicit) {
      const double c = g.alpha * (double)fabsf(r);
      const double w = r > 0.f ? 1.0 + c : 0.0;
      const double cs2 = c * s * s, ws2 = 2.0 * w * s;
      t = cs2 - ws2 + w;
      a = fabs(cs2) + fabs(ws2) + w;
      pos = r > 0.f ? 1.0 : 0.0;
    }
    if (live) {  // past the row's end there is nothing to add
      A.t += t;
      A.sse += e * e;
      A.abs += a;
      A.n += pos;
    }
  }

  // the lanes of a group hold equal sums
  template <int KP>
  __device__ static void group_sums(Acc& A) {
    constexpr int L = KP / 4;
    A.t = lanes_sum<L, 64>(A.t);
    A.sse = lanes_sum<L, 64>(A.sse);
    A.abs = lanes_sum<L, 64>(A.abs);
    A.n = lanes_sum<L, 64>(A.n);
  }

  template <int KP>
  __device__ static void store(double* rec, const Acc& A) {
    if ((threadIdx.x & 63) != 0) return;
    rec[0] = A.t, rec[1] = A.sse, rec[2] = A.abs, rec[3] = A.n;
  }

  template <int KP>
  __device__ static void load(const double* rec, Acc& A) {
    A.t += rec[0], A.sse += rec[1], A.abs += rec[2], A.n += rec[3];
  }

  // the record of dst row `row`: xᵀGx from G·x (gx, null when explicit), the regulariser and the loss
  template <int KP>
  __device__ static void finish_row(const Args& g, int64_t row, int64_t degree, const float4 xf, const Acc& A,
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
};

// out[i] = n_i·‖y_i‖² of row i of the other side, n_i from that side's own ratings (val null: the degree)
template <int KP>
__global__ __launch_bounds__(64 * ROW_WAVES) void objective_other_kernel(const float* __restrict__ Y,
                                                                          const int64_t* __restrict__ ptr,
                                                                          const float* __restrict__ val, int64_t n,
                                                                          double* __restrict__ out) {
  constexpr int L = KP / 4;
  const int64_t i = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
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

}  // namespace

hipError_t launch_objective_chunks(int KP, const ObjectiveArgs& g, hipStream_t s) {
  return row_pass_chunks<ObjectivePass>(KP, g, s);
}

hipError_t launch_objective_rows(int KP, const ObjectiveArgs& g, int64_t l0, int64_t n_long, hipStream_t s) {
  return row_pass_batch<ObjectivePass>(KP, g, l0, n_long, s);
}

hipError_t launch_objective_other(int KP, const float* Y, const int64_t* ptr, const float* val, int64_t n, double* out,
                                  hipStream_t s) {
  if (n <= 0) return hipSuccess;
  return for_kp(KP, [&](auto kp) {
    objective_other_kernel<decltype(kp)::value>
        <<<(unsigned)((n + ROW_WAVES - 1) / ROW_WAVES), 64 * ROW_WAVES, 0, s>>>(Y, ptr, val, n, out);
    return hipGetLastError();
  });
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
