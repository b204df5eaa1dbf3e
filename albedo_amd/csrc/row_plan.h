// Host side of the fp64 row pass (row_pass.h) under audit_host.cpp and objective_host.cpp: how long rows
// are cut into chunks, the lists the chunk and long-row kernels read, and the batches of dst rows.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "engine.h"
#include "kernels.h"

namespace albedo {

// Ratings per chunk of a long row.  A row is one wave's work, so a launch runs as long as its longest
// row; the rule for skewed gathers is to cut lists longer than a quarter of one wave's share of the
// work (ratings / waves in flight) into chunks of that size.  The waves are counted at the hardware's 8
// per SIMD, more than the row kernels' registers allow: the smaller share errs towards more chunks,
// which cost one record each.  512, the size that rule was measured at, is the floor: below it a chunk
// record (the audit's is 2·KP + 2 doubles) stops being small beside the gather it stands for.  The
// environment variable `env` (ALBEDO_AUDIT_CHUNK, ALBEDO_OBJECTIVE_CHUNK), read per call, overrides it
// (tests: 256).
inline int64_t row_chunk_len(const als_ctx* c, int64_t own_nnz, const char* env) {
  const char* e = std::getenv(env);
  if (e && *e && std::atoll(e) > 0) return std::atoll(e);
  const int64_t waves = (int64_t)c->n_cu * 4 * 8;
  return std::max<int64_t>(512, own_nnz / (4 * waves));
}

// dst rows per batch: G·x of a batch ([batch][KP] fp64) stays within 256 MB
inline int64_t row_batch_len(int64_t own_n, int KP) {
  return std::max<int64_t>(64, std::min<int64_t>(own_n, ((int64_t)256 << 20) / (KP * 8)));
}

// The long rows of a side and their chunks, rows ascending, on the device with the chunks' records
struct RowPlan {
  std::vector<int32_t> lrow;  // the rows above the chunk length
  DevBuf d_crow, d_cidx, d_lrow, d_slot0, d_partial;

  // cuts T's rows above g->chunk (set by the caller) into chunks of rec_doubles doubles each and fills g's
  // chunk_row, chunk_idx, n_chunks, long_row, long_slot0 and partial
  int build(const als_ctx* c, const Side& T, int rec_doubles, RowPassArgs* g) {
    std::vector<int32_t> crow, cidx;
    std::vector<int64_t> slot0{0};
    for (int64_t r = 0; r < T.own_n; ++r) {
      if (T.h_deg[r] <= g->chunk) continue;
      const int64_t nch = (T.h_deg[r] + g->chunk - 1) / g->chunk;
      for (int64_t k = 0; k < nch; ++k) {
        crow.push_back((int32_t)r);
        cidx.push_back((int32_t)k);
      }
      lrow.push_back((int32_t)r);
      slot0.push_back((int64_t)crow.size());
    }
    g->n_chunks = (int64_t)crow.size();
    if (g->n_chunks == 0) return ALS_OK;
    HIPCHK(d_crow.ensure(crow.size() * 4));
    HIPCHK(d_cidx.ensure(cidx.size() * 4));
    HIPCHK(d_lrow.ensure(lrow.size() * 4));
    HIPCHK(d_slot0.ensure(slot0.size() * 8));
    HIPCHK(d_partial.ensure(crow.size() * (size_t)rec_doubles * 8));
    HIPCHK(copy_st(c, d_crow.p, crow.data(), crow.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, d_cidx.p, cidx.data(), cidx.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, d_lrow.p, lrow.data(), lrow.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_st(c, d_slot0.p, slot0.data(), slot0.size() * 8, hipMemcpyHostToDevice));
    g->chunk_row = d_crow.as<int32_t>();
    g->chunk_idx = d_cidx.as<int32_t>();
    g->long_row = d_lrow.as<int32_t>();
    g->long_slot0 = d_slot0.as<int64_t>();
    g->partial = d_partial.as<double>();
    return ALS_OK;
  }

  // launch(row0, nb, l0, n_long) per batch of `batch` rows: rows [row0, row0 + nb), whose long rows are
  // [l0, l0 + n_long) of the list
  template <class F>
  int batches(int64_t own_n, int64_t batch, F&& launch) const {
    int64_t l0 = 0;
    for (int64_t r0 = 0; r0 < own_n; r0 += batch) {
      const int64_t nb = std::min<int64_t>(batch, own_n - r0);
      int64_t l1 = l0;
      while (l1 < (int64_t)lrow.size() && lrow[l1] < r0 + nb) ++l1;
      TRYC(launch(r0, nb, l0, l1 - l0));
      l0 = l1;
    }
    return ALS_OK;
  }
};

}  // namespace albedo
