// Host side of what als_fold_in (foldin_host.cpp) and als_explain (explain_host.cpp) do alike, up to the
// launch of their own kernel: the triples as a CSR on the device (fold_build_csr), the fp64 src Gram from the
// side's fold-in cache, the persistent grid with its scratch, and the report of a row that is not positive
// definite.  The functions are in foldin_host.cpp.
#pragma once
#include "engine.h"
#include "kernels.h"

namespace albedo {

// Owns every buffer of the front; the caller declares it before its Drain.  The stage marks stay with the
// caller: upload | mark 0 | build_csr (the explanation: and its pair map) | mark 1 | gram | mark 2 | plan, launch
struct FoldFront {
  DevBuf d_row, d_src, d_val, d_sids, d_key, d_keys, d_vals, d_hi, d_col, d_runs, d_cnt, d_ptr, d_nr, d_ids, d_deg, d_degs;
  DevBuf d_iota, d_order, d_tmp, d_slab, d_scratch, d_bad;
  int side = 0;            // the side of the new rows; the src side is the other one
  int64_t n = 0;           // triples
  FoldCsr f{};
  size_t temp_bytes = 0;   // of d_tmp: fold_sort_temp_bytes(n) or the caller's larger need
  int64_t n_rows = 0;      // distinct row ids (after build_csr)
  bool form_gram = false;  // this call forms the cached Gram (after gram)
  int bad0 = 0;            // what upload copies into d_bad: it lives until the call's stream is drained

  // the buffers of n > 0 triples and a temp buffer of at least min_temp bytes; the triples, the src id table
  // and bad = INT_MAX queued on c->st.  The src side is materialised by the caller
  int upload(als_ctx* c, int side, int64_t n, const int32_t* row_id, const int32_t* src_id, const float* rating,
             size_t min_temp);
  int build_csr(als_ctx* c);
  // implicit and the cache is stale: the Gram into Side::d_foldG.  The cache is marked valid by finish
  int gram(als_ctx* c, int implicit);
  // the persistent grid over n_work rows (*n_wg) with its scratch, and the fields of FoldArgs that both calls
  // fill: Y, G, ptr, deg, col, val, k, implicit, alpha, reg, scratch, bad
  int plan(als_ctx* c, int64_t n_work, double reg, double alpha, int implicit, FoldArgs* a, int* n_wg);
  // behind the synchronisation that brought `bad` (FoldArgs::bad) to the host: the cache becomes valid;
  // ALS_E_NOT_POSITIVE_DEFINITE naming `what` ("fold-in", "explanation") and the lowest failing id
  int finish(als_ctx* c, int bad, const char* what);
};

}  // namespace albedo
