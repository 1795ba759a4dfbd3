// The gradient of the pooled lookup's WEIGHTS over a tier: tfra_tier_find_combine_backprop_weights and
// tfra_tier_find_combine_ragged_backprop_weights, the calls tfra_table_find_combine_backprop_weights and its ragged form are for one
// table, over BOTH tables of a tier and in their launches.  An entry's row is the one the upper table holds, else the one the lower
// table holds, else default_row: upper wins, as everywhere in the tier.  These calls are reads — nothing moves between the tiers,
// neither table is written, no score is touched and the driver's statistics stay as they are — and they use none of the driver's
// staging, so the batch is not limited by max_batch.
// The kernels are wgrad_row (tfra_wgrad_device.h) with its TIER axis: the mapping, the entry batching and the arithmetic of the
// one-table kernels, in the same order, so the result equals tfra_tier_find + tfra_sparse_segment_combine_backprop_weights, and
// tfra_table_find_combine_backprop_weights on one table that holds the same newest rows, bit for bit.  The host frames are those of
// tfra_tier_find_combine* (tfra_tierpool.hip) with the one-table gradient's dw_out check, memset and early returns.
// The *_typed calls are tfra_wgrad.hip's over a tier: the same frames, wgrad_row's GHALF axis in kernels of their own
// names for a float16 / bfloat16 grad_out, float32 without a scale forwarded to the untyped call.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_tier.h"
#include "tfra_wgrad_device.h"

using namespace tfra;

namespace {

// wgrad_kernel's launch shape — 256 threads, one 16-lane group per output row, no LDS — with the lower table's view beside the
// upper one's.
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void tier_wgrad_kernel(TableView up, TableView lo, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                         const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                         const unsigned char* __restrict__ default_row,
                                                         const float* __restrict__ grad_out, float* dw) {
  wgrad_row<DT, U, NCH, false, false, true>(up, n_rows, dim, ids, w, start_end, nullptr, 0, combiner, default_row, grad_out, dw,
                                            ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, &lo);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void tier_wgrad_ragged_kernel(TableView up, TableView lo, size_t n_rows, int dim,
                                                                const i64* __restrict__ ids, const float* __restrict__ w,
                                                                const i64* __restrict__ row_splits, int nnz, int combiner,
                                                                const unsigned char* __restrict__ default_row,
                                                                const float* __restrict__ grad_out, float* dw) {
  wgrad_row<DT, U, NCH, true, PRUNE, true>(up, n_rows, dim, ids, w, nullptr, row_splits, nnz, combiner, default_row, grad_out, dw,
                                           ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, &lo);
}

// the same two over a float16 / bfloat16 grad_out (wgrad_row's GHALF axis)
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void tier_wgrad_half_kernel(TableView up, TableView lo, size_t n_rows, int dim,
                                                              const i64* __restrict__ ids, const float* __restrict__ w,
                                                              const int* __restrict__ start_end, int combiner,
                                                              const unsigned char* __restrict__ default_row,
                                                              const float* __restrict__ grad_out, float* dw,
                                                              const float* __restrict__ d_scale, int is_bf16) {
  wgrad_row<DT, U, NCH, false, false, true, true>(up, n_rows, dim, ids, w, start_end, nullptr, 0, combiner, default_row, grad_out, dw,
                                                  ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, &lo, d_scale, is_bf16);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void tier_wgrad_ragged_half_kernel(TableView up, TableView lo, size_t n_rows, int dim,
                                                                     const i64* __restrict__ ids, const float* __restrict__ w,
                                                                     const i64* __restrict__ row_splits, int nnz, int combiner,
                                                                     const unsigned char* __restrict__ default_row,
                                                                     const float* __restrict__ grad_out, float* dw,
                                                                     const float* __restrict__ d_scale, int is_bf16) {
  wgrad_row<DT, U, NCH, true, PRUNE, true, true>(up, n_rows, dim, ids, w, nullptr, row_splits, nnz, combiner, default_row, grad_out, dw,
                                                 ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, &lo, d_scale, is_bf16);
}

// The two calls, untyped (hg == nullptr) and over a half grad_out (hg, checked by check_typed; grad_out is what the twin's checks
// look at then): one function each, fn names the caller in the refusals.
int tier_wgrad_impl(const std::string& fn, tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                    const float* weights, int combiner, size_t n_rows, const void* default_row, const float* grad_out,
                    const tfra_grads* hg, float* dw_out, tfra_stream_t stream) {
  if (!tier) return set_error(TFRA_ERR_INVALID, fn + "null tier");
  Table* t = tier->upper;
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grad_out,
                               [&] { return Check{tier_enter(tier, s, &entry)}; });
  if (c.msg == NEEDS_DIM)
    c.msg += " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report(fn + "(out = grad_out) ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report(fn, d);
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries in no row: 0
  if (!c.active) return TFRA_OK;                                // (no rows)
  const int dim = t->opts.dim;
  int rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  // the views are taken here, under the locks: a lower table that grew since the last call has another one
  const TableView up = t->view_of(t->cur), lo = tier->lower->view_of(tier->lower->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto U, auto NCH) {
    if (hg)
      tier_wgrad_half_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(up, lo, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                              (const unsigned char*)default_row, (const float*)hg->grads, dw_out,
                                                              hg->d_scale, hg->dtype == TFRA_BF16);
    else
      tier_wgrad_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(up, lo, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                             (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tier_wgrad_ragged_impl(const std::string& fn, tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                           const int64_t* ids, const float* weights, int combiner, uint32_t flags, int64_t fill_id,
                           const void* default_row, const float* grad_out, const tfra_grads* hg, float* dw_out, tfra_stream_t stream) {
  if (!tier) return set_error(TFRA_ERR_INVALID, fn + "null tier");
  Table* t = tier->upper;
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row, grad_out,
                                      [&] { return Check{tier_enter(tier, s, &entry)}; });
  if (c.msg == NEEDS_DIM)
    c.msg += " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report(fn + "(out = grad_out) ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report(fn, d);
  (void)fill_id;   // a row that takes the fill row has no members: its entries are 0 whatever fill_id holds, in either table
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries outside the clamped cover: 0
  if (!c.active) return TFRA_OK;                                // (no rows)
  const int dim = t->opts.dim;
  const TableView up = t->view_of(t->cur), lo = tier->lower->view_of(tier->lower->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  // the ladder's fourth axis is PRUNE here, as in the one-table call: FILL changes nothing, and PRUNE without weights neither
  with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), (flags & TFRA_RAGGED_PRUNE) && weights,
                    [&](auto DT, auto U, auto NCH, auto PRUNE) {
    if (hg)
      tier_wgrad_ragged_half_kernel<DT, U, NCH, PRUNE><<<grid, 256, 0, s>>>(up, lo, n_rows, dim, (const i64*)ids, weights,
                                                                            (const i64*)row_splits, (int)nnz, combiner,
                                                                            (const unsigned char*)default_row, (const float*)hg->grads,
                                                                            dw_out, hg->d_scale, hg->dtype == TFRA_BF16);
    else
      tier_wgrad_ragged_kernel<DT, U, NCH, PRUNE><<<grid, 256, 0, s>>>(up, lo, n_rows, dim, (const i64*)ids, weights,
                                                                           (const i64*)row_splits, (int)nnz, combiner,
                                                                           (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

}  // namespace

extern "C" int tfra_tier_find_combine_backprop_weights(tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                       const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                       const void* default_row, const float* grad_out, float* dw_out,
                                                       tfra_stream_t stream) {
  return tier_wgrad_impl("tfra_tier_find_combine_backprop_weights: ", tier, ws, nnz, ids, seg, weights, combiner, n_rows, default_row,
                         grad_out, nullptr, dw_out, stream);
}

extern "C" int tfra_tier_find_combine_ragged_backprop_weights(tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                              const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                              int64_t fill_id, const void* default_row, const float* grad_out,
                                                              float* dw_out, tfra_stream_t stream) {
  return tier_wgrad_ragged_impl("tfra_tier_find_combine_ragged_backprop_weights: ", tier, n_rows, row_splits, nnz, ids, weights, combiner,
                                flags, fill_id, default_row, grad_out, nullptr, dw_out, stream);
}

// ---- the *_typed calls: the record is checked first, before the tier is looked at; then the twin's checks, in the twin's words
extern "C" int tfra_tier_find_combine_backprop_weights_typed(tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                             const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                             const void* default_row, const tfra_grads* grad_out, float* dw_out,
                                                             tfra_stream_t stream) {
  const std::string fn = "tfra_tier_find_combine_backprop_weights_typed: ";
  bool forward;
  if (const Check c = check_typed(grad_out, &forward); c.code) return report(fn, c);
  if (forward)
    return tfra_tier_find_combine_backprop_weights(tier, ws, nnz, ids, seg, weights, combiner, n_rows, default_row,
                                                   (const float*)grad_out->grads, dw_out, stream);
  return tier_wgrad_impl(fn, tier, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grads_for_twin(*grad_out), grad_out, dw_out,
                         stream);
}

extern "C" int tfra_tier_find_combine_ragged_backprop_weights_typed(tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                                    const int64_t* ids, const float* weights, int combiner,
                                                                    uint32_t flags, int64_t fill_id, const void* default_row,
                                                                    const tfra_grads* grad_out, float* dw_out, tfra_stream_t stream) {
  const std::string fn = "tfra_tier_find_combine_ragged_backprop_weights_typed: ";
  bool forward;
  if (const Check c = check_typed(grad_out, &forward); c.code) return report(fn, c);
  if (forward)
    return tfra_tier_find_combine_ragged_backprop_weights(tier, n_rows, row_splits, nnz, ids, weights, combiner, flags, fill_id,
                                                          default_row, (const float*)grad_out->grads, dw_out, stream);
  return tier_wgrad_ragged_impl(fn, tier, n_rows, row_splits, nnz, ids, weights, combiner, flags, fill_id, default_row,
                                grads_for_twin(*grad_out), grad_out, dw_out, stream);
}
