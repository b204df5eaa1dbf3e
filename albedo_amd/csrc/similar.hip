// als_similar / als_similar_vectors: the unit image of one side and the queries taken from it
// (include/albedo_als.h).  The top-k itself is the query scan of query_topk.hip or the tuned passes behind
// als_recommend_unseen (similar_host.cpp); the kernels here only prepare what those read.
//
// The unit row of a row y (fp32, `rank` columns) is pinned bit for bit:
//   s = F2J sdot(y, y)   fp32, left to right from +0.0, multiply and add rounded separately
//   r = sqrt(s)          correctly rounded
//   u_c = y_c / r        correctly rounded, per column
// A row has no direction when !(s > 0 && s < inf) (all zero, NaN or inf inside, s overflowed or underflowed
// to 0): its unit row is NaN and its flag 0.
//
// Plain HIP like query_topk.hip: no inline asm, no MFMA, none of device_common.h.
//
//   similar_unit_kernel     256 rows a workgroup.  The rows go through LDS 32 columns at a time (coalesced
//                           loads, row stride 33 floats), a thread sums its own row's squares in column
//                           order; the divide then runs over the block's elements in memory order.
//   similar_gather_kernel   requested dense rows -> query block [n_q][rank] and each query's one-entry
//                           exclusion range (its own row): excl_ptr[i] = i, key[i] = (i << 32 | row).  One key
//                           per query in query order is already sorted.  A negative row (unknown id) or a row
//                           without a direction gives a NaN query, whose scores are never listed.
//   similar_compact_kernel  the rows `rows[j]` of the image, in that order (the passes tier's finite sides)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace albedo {

namespace {

constexpr int SM_ROWS = 256, SM_COLS = 32, SM_LD = SM_COLS + 1;
constexpr uint32_t SM_NOROW = 0xFFFFFFFFu;

inline int similar_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536)); }

__global__ __launch_bounds__(SM_ROWS) void similar_unit_kernel(const float* __restrict__ in, int64_t ld_in, int64_t n,
                                                               int rank, float* __restrict__ out, int64_t ld_out,
                                                               int32_t* __restrict__ flag) {
#pragma clang fp contract(off)  // the square and the add stay two roundings (hipcc contracts by default)
  __shared__ float tile[SM_ROWS * SM_LD];
  __shared__ float rr[SM_ROWS];
  const int tid = threadIdx.x;
  const int64_t n_blocks = (n + SM_ROWS - 1) / SM_ROWS;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t t0 = b * SM_ROWS;
    const int nr = (int)(n - t0 < SM_ROWS ? n - t0 : SM_ROWS);
    float s = 0.f;
    for (int c0 = 0; c0 < rank; c0 += SM_COLS) {
      const int ce = rank - c0 < SM_COLS ? rank - c0 : SM_COLS;
      __syncthreads();  // the previous block of columns (or the previous block's rr) is read
      for (int e = tid; e < SM_ROWS * SM_COLS; e += SM_ROWS) {
        const int r = e / SM_COLS, c = e % SM_COLS;
        tile[r * SM_LD + c] = (r < nr && c < ce) ? in[(t0 + r) * ld_in + c0 + c] : 0.f;
      }
      __syncthreads();
      const float* tr = tile + tid * SM_LD;
      for (int c = 0; c < ce; ++c) {
        const float t = tr[c];
        s = s + t * t;
      }
    }
    const bool dir = s > 0.f && s < __int_as_float(0x7F800000);
    // sqrtf: in the gfx950 listing v_sqrt_f32 followed by the two v_fma_f32 residual tests that step the root
    // down or up one ulp (correctly rounded).  __fsqrt_rn is not used: without OCML_BASIC_ROUNDED_OPERATIONS
    // __clang_hip_math.h maps it to __ocml_native_sqrt_f32, a bare v_sqrt_f32 that is off by one ulp for some
    // inputs (seen as a last-bit score difference against numpy).  The listing holds no fused multiply-add
    // outside the sqrt and divide sequences: the square is v_mul_f32 and the sum v_add_f32
    rr[tid] = dir ? sqrtf(s) : __int_as_float(0x7FC00000);
    if (flag && tid < nr) flag[t0 + tid] = dir ? 1 : 0;
    __syncthreads();
    const int64_t total = (int64_t)nr * ld_out;
    for (int64_t e = tid; e < total; e += SM_ROWS) {
      const int r = (int)(e / ld_out), c = (int)(e % ld_out);
      out[(t0 + r) * ld_out + c] = c < rank ? __fdiv_rn(in[(t0 + r) * ld_in + c], rr[r]) : 0.f;
    }
  }
}

__global__ void similar_gather_kernel(const float* __restrict__ unit, int KP, int rank, const int32_t* __restrict__ flag,
                                      const int32_t* __restrict__ rows, int64_t n_q, float* __restrict__ q,
                                      int64_t* __restrict__ excl_ptr, uint64_t* __restrict__ excl_key) {
  const int64_t total = n_q * rank;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / rank;
    const int c = (int)(e % rank);
    const int64_t row = rows ? rows[i] : i;
    const bool dir = row >= 0 && flag[row] != 0;
    q[e] = dir ? unit[row * KP + c] : __int_as_float(0x7FC00000);
    if (c == 0) {
      excl_ptr[i] = i;
      excl_key[i] = ((uint64_t)i << 32) | (row >= 0 ? (uint32_t)row : SM_NOROW);
      if (i == 0) excl_ptr[n_q] = n_q;
    }
  }
}

__global__ void similar_compact_kernel(const float* __restrict__ unit, int KP, const int32_t* __restrict__ rows, int64_t n,
                                       float* __restrict__ out) {
  const int K4 = KP / 4;
  const int64_t total = n * K4;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / K4;
    const int c4 = (int)(e % K4);
    reinterpret_cast<float4*>(out)[j * K4 + c4] = reinterpret_cast<const float4*>(unit)[(int64_t)rows[j] * K4 + c4];
  }
}

}  // namespace

hipError_t launch_similar_unit(const float* in, int64_t ld_in, int64_t n, int rank, float* out, int64_t ld_out,
                               int32_t* flag, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (rank < 1 || ld_in < rank || ld_out < rank || ld_out > (int64_t)1 << 20) return hipErrorInvalidValue;
  similar_unit_kernel<<<similar_grid(n), SM_ROWS, 0, s>>>(in, ld_in, n, rank, out, ld_out, flag);
  return hipGetLastError();
}

hipError_t launch_similar_gather(const float* unit, int KP, int rank, const int32_t* flag, const int32_t* rows, int64_t n_q,
                                 float* q, int64_t* excl_ptr, uint64_t* excl_key, hipStream_t s) {
  if (n_q <= 0) return hipSuccess;
  if (rank < 1 || rank > KP || n_q > (int64_t)0x7FFFFFFF) return hipErrorInvalidValue;
  similar_gather_kernel<<<similar_grid(n_q * rank), 256, 0, s>>>(unit, KP, rank, flag, rows, n_q, q, excl_ptr, excl_key);
  return hipGetLastError();
}

hipError_t launch_similar_compact(const float* unit, int KP, const int32_t* rows, int64_t n, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (KP < 4 || KP % 4) return hipErrorInvalidValue;
  similar_compact_kernel<<<similar_grid(n * (KP / 4)), 256, 0, s>>>(unit, KP, rows, n, out);
  return hipGetLastError();
}

}  // namespace albedo
