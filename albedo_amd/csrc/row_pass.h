// The fp64 row pass under the two yardsticks of the solve kernels, the row audit (audit.hip) and the
// objective (objective.hip): one pass over the dst CSR with the gather of the solve's build, O(nnz·k).
// The two share this file with each other and nothing with the solves: plain HIP, no inline asm, no MFMA,
// none of device_common.h.  Everything is fp64 arithmetic on the fp32 factors and ratings; nothing is added
// by a floating-point atomic, every sum has one fixed order.
//
// Layout.  A wave is cut into groups of KP/4 lanes; a lane holds 4 consecutive components (one 16-byte
// load of a factor row), so a group covers one src row and a wave gathers 64 / (KP/4) = 4, 2 or 1 src
// rows per step (KP = 64, 128, 256).  ROW_UNROLL steps are loaded before any is used: the row gathers
// are the cost, and their addresses depend only on the column indices, which are loaded together too.
// Per rating the group reduces y·x across its lanes (shuffles of doubles) and hands it to the pass.
//   row_pass_rows_kernel    one wave per dst row of at most `chunk` ratings, start to finish_row
//   row_pass_chunk_kernel   longer rows: one wave per chunk of `chunk` ratings -> an fp64 partial record
//   row_pass_long_kernel    one wave per long row: its records added in chunk order (deterministic), then
//                           finish_row like any other row
// G·x of a batch comes from launch_row_gx (audit.hip) in front of the batch's rows.
//
// A pass P supplies
//   Args                             RowPassArgs plus its own fields
//   Acc                              what a lane sums over the ratings its group took, zero when constructed
//   rec_doubles<KP>                  doubles per chunk record
//   W, weigh(g, live, r)             what a pass derives from the rating r alone; live is false past the
//                                    row's end, where r and y are zero.  It stands ahead of the shuffles
//                                    in the code too: the audit's weights taken after them cost 4 VGPRs,
//                                    which at KP = 64 takes its chunk kernel over 128 and a wave off a SIMD
//   add(g, A, w, live, r, y0..y3, dot)  one rating on src row y (this lane's components), dot = y·x
//   group_sums<KP>(A)                the groups of a wave took different ratings: the row's (or chunk's) totals
//   store<KP>(rec, A) / load<KP>(rec, A)   a chunk's totals into its record / added to A from it
//   finish_row<KP>(g, row, degree, xf, A, gx)   the row's output; gx: its row of G·x, null when explicit
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kernels.h"

namespace albedo {

constexpr int ROW_WAVES = 4;   // waves (dst rows or chunks) per workgroup
constexpr int ROW_UNROLL = 4;  // gather steps in flight per wave

// f(KP as a compile-time constant) for the three padded ranks
template <class F>
hipError_t for_kp(int KP, F&& f) {
  if (KP == 64) return f(std::integral_constant<int, 64>{});
  if (KP == 128) return f(std::integral_constant<int, 128>{});
  if (KP == 256) return f(std::integral_constant<int, 256>{});
  return hipErrorInvalidValue;
}

template <int FROM, int TO>
__device__ inline double lanes_sum(double v) {  // butterfly over the lane bits FROM <= 2^s < TO
#pragma unroll
  for (int o = FROM; o < TO; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int KP>
__device__ inline float4 load_x(const RowPassArgs& g, int64_t row) {
  return *reinterpret_cast<const float4*>(g.X + row * KP + 4 * ((threadIdx.x & 63) % (KP / 4)));
}

// ratings [p0, p1) of one dst row whose factors are x (this lane's 4 components), each handed to the pass
template <int KP, class P>
__device__ inline void accumulate(const typename P::Args& g, int64_t p0, int64_t p1, const float4 xf,
                                  typename P::Acc& A) {
  constexpr int L = KP / 4, NG = 64 / L;
  const int lane = threadIdx.x & 63, sub = lane % L, grp = lane / L;
  const double x0 = xf.x, x1 = xf.y, x2 = xf.z, x3 = xf.w;
  for (int64_t base = p0; base < p1; base += NG * ROW_UNROLL) {  // wave-uniform: the shuffles need every lane
    int32_t col[ROW_UNROLL];
    float r[ROW_UNROLL];
    float4 y[ROW_UNROLL];
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u) {
      const int64_t p = base + u * NG + grp;
      col[u] = p < p1 ? g.col[p] : -1;
      r[u] = p < p1 ? g.val[p] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u)
      y[u] = col[u] >= 0 ? *reinterpret_cast<const float4*>(g.Y + (int64_t)col[u] * KP + 4 * sub)
                         : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u) {
      const auto w = P::weigh(g, col[u] >= 0, r[u]);
      const double y0 = y[u].x, y1 = y[u].y, y2 = y[u].z, y3 = y[u].w;
      const double dot = lanes_sum<1, L>(y0 * x0 + y1 * x1 + y2 * x2 + y3 * x3);
      P::add(g, A, w, col[u] >= 0, r[u], y0, y1, y2, y3, dot);
    }
  }
}

template <int KP, class P>
__global__ __launch_bounds__(64 * ROW_WAVES) void row_pass_rows_kernel(const typename P::Args g) {
  const int64_t i = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (i >= g.nb) return;
  const int64_t row = g.row0 + i;
  const int64_t p0 = g.ptr[row], p1 = g.ptr[row + 1];
  if (p1 - p0 > g.chunk) return;  // row_pass_chunk_kernel + row_pass_long_kernel
  const float4 xf = load_x<KP>(g, row);
  typename P::Acc A;
  accumulate<KP, P>(g, p0, p1, xf, A);  // degree 0 (not an ingested row): nothing to add
  P::template group_sums<KP>(A);
  P::template finish_row<KP>(g, row, p1 - p0, xf, A, g.GX ? g.GX + i * KP : nullptr);
}

template <int KP, class P>
__global__ __launch_bounds__(64 * ROW_WAVES) void row_pass_chunk_kernel(const typename P::Args g) {
  const int64_t ci = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (ci >= g.n_chunks) return;
  const int64_t row = g.chunk_row[ci];
  const int64_t p0 = g.ptr[row] + (int64_t)g.chunk_idx[ci] * g.chunk;
  const int64_t pe = g.ptr[row + 1], p1 = p0 + g.chunk < pe ? p0 + g.chunk : pe;
  typename P::Acc A;
  accumulate<KP, P>(g, p0, p1, load_x<KP>(g, row), A);
  P::template group_sums<KP>(A);
  P::template store<KP>(g.partial + (size_t)ci * P::template rec_doubles<KP>, A);
}

// long rows [l0, l0 + n_long) of the list, all inside the batch [row0, row0 + nb)
template <int KP, class P>
__global__ __launch_bounds__(64 * ROW_WAVES) void row_pass_long_kernel(const typename P::Args g, int64_t l0,
                                                                       int64_t n_long) {
  const int64_t li = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (li >= n_long) return;
  const int64_t row = g.long_row[l0 + li];
  typename P::Acc A;
  for (int64_t ci = g.long_slot0[l0 + li]; ci < g.long_slot0[l0 + li + 1]; ++ci)  // chunk order
    P::template load<KP>(g.partial + (size_t)ci * P::template rec_doubles<KP>, A);
  P::template finish_row<KP>(g, row, g.ptr[row + 1] - g.ptr[row], load_x<KP>(g, row), A,
                             g.GX ? g.GX + (row - g.row0) * KP : nullptr);
}

// the partial records of every chunk of the long rows
template <class P>
hipError_t row_pass_chunks(int KP, const typename P::Args& g, hipStream_t s) {
  if (g.n_chunks <= 0) return hipSuccess;
  return for_kp(KP, [&](auto kp) {
    row_pass_chunk_kernel<decltype(kp)::value, P>
        <<<(unsigned)((g.n_chunks + ROW_WAVES - 1) / ROW_WAVES), 64 * ROW_WAVES, 0, s>>>(g);
    return hipGetLastError();
  });
}

// one batch: G·x, the rows of at most `chunk` ratings, then the batch's long rows
template <class P>
hipError_t row_pass_batch(int KP, const typename P::Args& g, int64_t l0, int64_t n_long, hipStream_t s) {
  if (g.nb <= 0) return hipSuccess;
  if (g.GX) {
    const hipError_t e = launch_row_gx(KP, g.X, g.G, g.GX, g.row0, g.nb, s);
    if (e != hipSuccess) return e;
  }
  return for_kp(KP, [&](auto kp) {
    constexpr int K = decltype(kp)::value;
    row_pass_rows_kernel<K, P><<<(unsigned)((g.nb + ROW_WAVES - 1) / ROW_WAVES), 64 * ROW_WAVES, 0, s>>>(g);
    if (n_long > 0)
      row_pass_long_kernel<K, P>
          <<<(unsigned)((n_long + ROW_WAVES - 1) / ROW_WAVES), 64 * ROW_WAVES, 0, s>>>(g, l0, n_long);
    return hipGetLastError();
  });
}

}  // namespace albedo
