// The front of the calls that take raw ids from the caller at call time and turn them into device ranges:
// als_evaluate_ndcg / als_evaluate_ranking (eval.hip), als_rank_pairs / als_evaluate_pairs (eval_pairs.hip),
// als_fold_in (foldin.hip), als_explain (explain.hip), als_recommend_vectors (query_topk.hip) and
// als_recommend_unseen (topk.hip).  Each of them maps ids to dense rows by binary search over the ascending
// id table, radix-sorts keys of its own layout (the sorts stay in the feature's file: the key is its
// contract) and, where it needs ranges, run-length encodes the sorted high halves.  What they share is here:
//   find_id          raw id -> dense row, -1 when unknown; the caller writes its own sentinel (lower_bound_id:
//                    the search under it, for explain_pair_kernel, which tests two matches at once)
//   front_grid       grid of the grid-stride kernels: one block per `per` items, at most 16384
//   split_keys_kernel  sorted 64-bit keys into their high and low halves
//   group_runs       run-length encode, the run count on the host behind one synchronisation, exclusive scan
//   degree_order     positions by descending degree (ties: ascending position); the positions are filled here
//                    (the fold-in) or by the caller's degree kernel (the explanation)
//   group_temp_bytes, sort_keys64_temp_bytes   rocprim temp sizes of the above and of the 64-bit key sort
// Plain HIP, no inline asm, none of device_common.h.  The kernels and the host functions that call rocprim
// are templates for one reason only: a template is compiled where it is used, so an object holds only the
// kernels its file launches (as plain functions every one of them, rocprim's included, lands in all six
// objects).  Where nothing real varies the type parameter is a dummy: Half and Deg are always uint32_t, T is
// always int32_t, Key always uint64_t.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>

namespace albedo {

// the first position of the ascending table ids[0 .. n) whose id is not below v (n: none)
__device__ __forceinline__ int64_t lower_bound_id(const int32_t* __restrict__ ids, int64_t n, int32_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// dense row of raw id v in that table, -1 when the table does not hold it
__device__ __forceinline__ int64_t find_id(const int32_t* __restrict__ ids, int64_t n, int32_t v) {
  const int64_t lo = lower_bound_id(ids, n, v);
  return (lo < n && ids[lo] == v) ? lo : -1;
}

inline int front_grid(int64_t n, int per = 256) {
  const int64_t b = (n + per - 1) / per;
  return (int)std::max<int64_t>(1, std::min<int64_t>(b, 16384));
}

template <class Half>
__global__ void split_keys_kernel(const uint64_t* __restrict__ key, int64_t n, Half* __restrict__ hi,
                                  Half* __restrict__ lo) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    hi[i] = (Half)(key[i] >> 32);
    lo[i] = (Half)key[i];
  }
}

template <class T>
__global__ void iota_kernel(T* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (T)i;
}

// temp bytes of group_runs<TOTAL> over n keys, and of degree_order over as many when ORDER
template <bool TOTAL, bool ORDER>
size_t group_temp_bytes(int64_t n) {
  size_t a = 0, b = 0, c = 0;
  (void)rocprim::run_length_encode(nullptr, a, (uint32_t*)nullptr, (size_t)n, (uint32_t*)nullptr, (int32_t*)nullptr,
                                   (int64_t*)nullptr, (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)n + (TOTAL ? 1 : 0),
                                rocprim::plus<int64_t>(), (hipStream_t)0);
  if constexpr (ORDER)
    (void)rocprim::radix_sort_pairs_desc(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr,
                                         (int32_t*)nullptr, (size_t)n, 0, 32, (hipStream_t)0);
  return std::max(a, std::max(b, c));
}

// temp bytes of a 64-bit radix_sort_keys over n keys
template <class Key = uint64_t>
size_t sort_keys64_temp_bytes(int64_t n) {
  size_t a = 0;
  (void)rocprim::radix_sort_keys(nullptr, a, (Key*)nullptr, (Key*)nullptr, (size_t)n, 0, 64, (hipStream_t)0);
  return a;
}

// (keys and deg below are read only; their pointers are not const so that the rocprim kernels are the ones the
// temp-size queries name, instantiated once)
// The runs of the ascending keys [n]: runs[r] with counts[r] keys from offsets[r].  The run count goes to
// *n_runs (device) and, behind the one synchronisation of the front, to *n_runs_host.
//   TOTAL   counts[0 .. n] is cleared first and one entry past the runs is scanned, so offsets[runs] = n
//           (a CSR's ptr), and a run count outside 1 .. n is hipErrorInvalidValue
//   else    offsets holds the runs' starts alone and the caller judges the count
template <bool TOTAL>
hipError_t group_runs(void* temp, size_t temp_bytes, uint32_t* keys, int64_t n, uint32_t* runs, int32_t* counts,
                      int64_t* offsets, int64_t* n_runs, int64_t* n_runs_host, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (TOTAL) e = hipMemsetAsync(counts, 0, (size_t)(n + 1) * 4, s);
  if (e != hipSuccess) return e;
  size_t tb = temp_bytes;
  e = rocprim::run_length_encode(temp, tb, keys, (size_t)n, runs, counts, n_runs, s);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(n_runs_host, n_runs, 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  const int64_t nr = *n_runs_host;
  if (TOTAL && (nr <= 0 || nr > n)) return hipErrorInvalidValue;
  tb = temp_bytes;
  return rocprim::exclusive_scan(temp, tb, counts, offsets, (int64_t)0, (size_t)nr + (TOTAL ? 1 : 0),
                                 rocprim::plus<int64_t>(), s);
}

// order [n]: the positions 0 .. n - 1 by descending deg (a stable sort: ties keep ascending position).
// FILL_IOTA: iota [n] is written here, by a launch of its own; else the caller's degree kernel has queued it
template <bool FILL_IOTA, class Deg>
hipError_t degree_order(void* temp, size_t temp_bytes, Deg* deg, Deg* deg_sorted, int32_t* iota, int32_t* order,
                        int64_t n, hipStream_t s) {
  if constexpr (FILL_IOTA) iota_kernel<<<front_grid(n), 256, 0, s>>>(iota, n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t tb = temp_bytes;
  return rocprim::radix_sort_pairs_desc(temp, tb, deg, deg_sorted, iota, order, (size_t)n, 0, 32, s);
}

}  // namespace albedo
