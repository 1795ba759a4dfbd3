// The pooled lookup over a tier: tfra_tier_find_combine and tfra_tier_find_combine_ragged, the forward of
// embedding_lookup_sparse / safe_embedding_lookup_sparse over BOTH tables of a tier in the launches tfra_table_find_combine and
// tfra_table_find_combine_ragged take for one table.  An entry's row is the one the upper table holds, else the one the lower table
// holds, else default_row: upper wins, as everywhere in the tier.  These calls are reads — nothing moves between the tiers, neither
// table is written, no score is touched and the driver's statistics stay as they are — and they use none of the driver's staging,
// so the batch is not limited by max_batch.
// The kernels are find_combine_row (tfra_pool_device.h) with its TIER axis: the mapping, the entry batching and the arithmetic of
// the one-table kernels, in the same order, so the result equals tfra_tier_find + tfra_sparse_segment_combine, and
// tfra_table_find_combine on one table that holds the same newest rows, bit for bit.  The argument checks and the launch ladders are
// those of the one-table calls (check_find_combine, check_find_combine_ragged, with_pool_class, with_ragged_class: tfra_pool.h),
// applied to the upper table: tfra_tier_create has made sure that both tables have its value dtype, dim and device.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_pool_device.h"
#include "tfra_tier.h"

using namespace tfra;

namespace {

// find_combine_kernel's launch shape — 256 threads, one 16-lane group per output row, no LDS — with the lower table's view beside
// the upper one's.
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void tier_find_combine_kernel(TableView up, TableView lo, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                const float* __restrict__ w, const int* __restrict__ start_end,
                                                                int combiner, const unsigned char* __restrict__ default_row,
                                                                float* __restrict__ out) {
  find_combine_row<DT, U, NCH, false, false, true>(up, n_rows, dim, ids, w, start_end, combiner, default_row, out,
                                                   ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, RaggedArgs{}, &lo);
}

template <int DT, int U, int NCH, bool SAFE>
__global__ __launch_bounds__(256) void tier_find_combine_ragged_kernel(TableView up, TableView lo, size_t n_rows, int dim,
                                                                       const i64* __restrict__ ids, const float* __restrict__ w,
                                                                       const i64* __restrict__ row_splits, int nnz, int combiner,
                                                                       unsigned flags, i64 fill_id,
                                                                       const unsigned char* __restrict__ default_row,
                                                                       float* __restrict__ out) {
  find_combine_row<DT, U, NCH, true, SAFE, true>(up, n_rows, dim, ids, w, nullptr, combiner, default_row, out,
                                                 ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4,
                                                 RaggedArgs{row_splits, nnz, flags, fill_id}, &lo);
}

}  // namespace

extern "C" int tfra_tier_find_combine(tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                      const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                      tfra_stream_t stream) {
  const std::string fn = "tfra_tier_find_combine: ";
  if (!tier) return set_error(TFRA_ERR_INVALID, fn + "null tier");
  Table* t = tier->upper;
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out,
                               [&] { return Check{tier_enter(tier, s, &entry)}; });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine otherwise)";
  if (c.code) return report(fn, c);
  if (!c.active) return TFRA_OK;
  const int dim = t->opts.dim;
  if (nnz == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * sizeof(float), s));
    return TFRA_OK;
  }
  int rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  // the views are taken here, under the locks: a lower table that grew since the last call has another one
  const TableView up = t->view_of(t->cur), lo = tier->lower->view_of(tier->lower->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto U, auto NCH) {
    tier_find_combine_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(up, lo, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                                    (const unsigned char*)default_row, out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

extern "C" int tfra_tier_find_combine_ragged(tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                             const int64_t* ids, const float* weights, int combiner, uint32_t flags, int64_t fill_id,
                                             const void* default_row, float* out, tfra_stream_t stream) {
  const std::string fn = "tfra_tier_find_combine_ragged: ";
  if (!tier) return set_error(TFRA_ERR_INVALID, fn + "null tier");
  Table* t = tier->upper;
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row, out,
                                      [&] { return Check{tier_enter(tier, s, &entry)}; });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine otherwise)";
  if (c.code) return report(fn, c);
  if (!c.active) return TFRA_OK;
  const int dim = t->opts.dim;
  if (nnz == 0 && !(flags & TFRA_RAGGED_FILL)) {
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * sizeof(float), s));
    return TFRA_OK;
  }
  const TableView up = t->view_of(t->cur), lo = tier->lower->view_of(tier->lower->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), ragged_safe(flags, weights), [&](auto DT, auto U, auto NCH, auto SAFE) {
    tier_find_combine_ragged_kernel<DT, U, NCH, SAFE><<<grid, 256, 0, s>>>(up, lo, n_rows, dim, (const i64*)ids, weights,
                                                                                 (const i64*)row_splits, (int)nnz, combiner, flags,
                                                                                 (i64)fill_id, (const unsigned char*)default_row, out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
