// The gradient of the pooled lookup with respect to its WEIGHTS, straight from the table (tfra_table_find_combine_backprop_weights
// and its ragged form).  The reference gets it from TensorFlow's autodiff of `embeddings *= weights`, segment_sum and the divide
// (PY/dynamic_embedding_ops.py:233-291), which needs the [nnz, dim] rows the pooled lookup was built to avoid.  Here the launch has
// the forward's shape (find_combine_row, tfra_pool.hip): one 16-lane group per OUTPUT ROW, one probe and one row read per entry, the
// row's incoming gradient held in registers where the forward holds its accumulator, and [nnz] floats out.
// The arithmetic and its ONE evaluation order are tfra_combine_device.h's (wgrad_dot4, wgrad_reduce16, wgrad_s, wgrad_finish), the
// code seg_combine_wgrad_kernel (tfra_combine.hip: rows from a [U, dim] tensor) compiles, so the two routes agree bit for bit.
// The argument checks and the launch ladders are the forward's (tfra_pool.h); the kernels' body, wgrad_row, is in
// tfra_wgrad_device.h, where the tier's kernels (tfra_tierwgrad.hip) find it too.
// The *_typed calls take grad_out as a tfra_grads: float32 without a scale forwards to the untyped call; a float16 /
// bfloat16 matrix runs the same host frame and wgrad_row with its GHALF axis, in kernels of their own names (wgrad_half_kernel,
// wgrad_ragged_half_kernel) — the float kernels keep their names and their code (profiles/wgrad_half_isa_stats.txt).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_wgrad_device.h"

using namespace tfra;

namespace {

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void wgrad_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                    const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                    const unsigned char* __restrict__ default_row,
                                                    const float* __restrict__ grad_out, float* dw) {
  wgrad_row<DT, U, NCH, false, false>(v, n_rows, dim, ids, w, start_end, nullptr, 0, combiner, default_row, grad_out, dw,
                                      ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void wgrad_ragged_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                           const float* __restrict__ w, const i64* __restrict__ row_splits, int nnz,
                                                           int combiner, const unsigned char* __restrict__ default_row,
                                                           const float* __restrict__ grad_out, float* dw) {
  wgrad_row<DT, U, NCH, true, PRUNE>(v, n_rows, dim, ids, w, nullptr, row_splits, nnz, combiner, default_row, grad_out, dw,
                                     ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

// the same two over a float16 / bfloat16 grad_out (wgrad_row's GHALF axis): the twins' launch shape and bounds
// (how they stay in the twins' register classes: the note at the load site, tfra_wgrad_device.h)
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void wgrad_half_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                         const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                         const unsigned char* __restrict__ default_row,
                                                         const float* __restrict__ grad_out, float* dw,
                                                         const float* __restrict__ d_scale, int is_bf16) {
  wgrad_row<DT, U, NCH, false, false, false, true>(v, n_rows, dim, ids, w, start_end, nullptr, 0, combiner, default_row, grad_out, dw,
                                                   ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, nullptr, d_scale, is_bf16);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void wgrad_ragged_half_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                const float* __restrict__ w, const i64* __restrict__ row_splits,
                                                                int nnz, int combiner, const unsigned char* __restrict__ default_row,
                                                                const float* __restrict__ grad_out, float* dw,
                                                                const float* __restrict__ d_scale, int is_bf16) {
  wgrad_row<DT, U, NCH, true, PRUNE, false, true>(v, n_rows, dim, ids, w, nullptr, row_splits, nnz, combiner, default_row, grad_out, dw,
                                                  ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, nullptr, d_scale, is_bf16);
}

// The two calls, untyped (hg == nullptr) and over a half grad_out (hg, checked by check_typed; grad_out is what the twin's checks
// look at then): one function each, `who` names the caller in the refusals.
int wgrad_impl(const std::string& who, tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
               const float* weights, int combiner, size_t n_rows, const void* default_row, const float* grad_out, const tfra_grads* hg,
               float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grad_out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report(who + " (out = grad_out): ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report(who + ": ", d);
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries in no row: 0
  if (!c.active) return TFRA_OK;                                // (no rows)
  const int dim = t->opts.dim;
  int rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto U, auto NCH) {
    if (hg)
      wgrad_half_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                         (const unsigned char*)default_row, (const float*)hg->grads, dw_out,
                                                         hg->d_scale, hg->dtype == TFRA_BF16);
    else
      wgrad_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                        (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int wgrad_ragged_impl(const std::string& who, tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz, const int64_t* ids,
                      const float* weights, int combiner, uint32_t flags, int64_t fill_id, const void* default_row,
                      const float* grad_out, const tfra_grads* hg, float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row, grad_out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report(who + " (out = grad_out): ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report(who + ": ", d);
  (void)fill_id;   // a row that takes the fill row has no members: its entries are 0 whatever fill_id holds
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries outside the clamped cover: 0
  if (!c.active) return TFRA_OK;                                // (no rows)
  const int dim = t->opts.dim;
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  // the ladder's fourth axis is PRUNE here: FILL changes nothing, and PRUNE without weights neither
  with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), (flags & TFRA_RAGGED_PRUNE) && weights,
                    [&](auto DT, auto U, auto NCH, auto PRUNE) {
    if (hg)
      wgrad_ragged_half_kernel<DT, U, NCH, PRUNE><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, (const i64*)row_splits,
                                                                       (int)nnz, combiner, (const unsigned char*)default_row,
                                                                       (const float*)hg->grads, dw_out, hg->d_scale,
                                                                       hg->dtype == TFRA_BF16);
    else
      wgrad_ragged_kernel<DT, U, NCH, PRUNE><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, (const i64*)row_splits, (int)nnz,
                                                                    combiner, (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

}  // namespace

extern "C" int tfra_table_find_combine_backprop_weights(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                        const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                        const void* default_row, const float* grad_out, float* dw_out,
                                                        tfra_stream_t stream) {
  return wgrad_impl("find_combine_backprop_weights", tp, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grad_out, nullptr,
                    dw_out, stream);
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                               const int64_t* ids, const float* weights, int combiner,
                                                               uint32_t flags, int64_t fill_id, const void* default_row,
                                                               const float* grad_out, float* dw_out, tfra_stream_t stream) {
  return wgrad_ragged_impl("find_combine_ragged_backprop_weights", tp, n_rows, row_splits, nnz, ids, weights, combiner, flags, fill_id,
                           default_row, grad_out, nullptr, dw_out, stream);
}

// ---- the *_typed calls: the record is checked first, before the table is looked at; then the twin's checks, in the twin's words
extern "C" int tfra_table_find_combine_backprop_weights_typed(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                              const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                              const void* default_row, const tfra_grads* grad_out, float* dw_out,
                                                              tfra_stream_t stream) {
  bool forward;
  if (const Check c = check_typed(grad_out, &forward); c.code) return report("find_combine_backprop_weights_typed: ", c);
  if (forward)
    return tfra_table_find_combine_backprop_weights(tp, ws, nnz, ids, seg, weights, combiner, n_rows, default_row,
                                                    (const float*)grad_out->grads, dw_out, stream);
  return wgrad_impl("find_combine_backprop_weights_typed", tp, ws, nnz, ids, seg, weights, combiner, n_rows, default_row,
                    grads_for_twin(*grad_out), grad_out, dw_out, stream);
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights_typed(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits,
                                                                     size_t nnz, const int64_t* ids, const float* weights, int combiner,
                                                                     uint32_t flags, int64_t fill_id, const void* default_row,
                                                                     const tfra_grads* grad_out, float* dw_out, tfra_stream_t stream) {
  bool forward;
  if (const Check c = check_typed(grad_out, &forward); c.code) return report("find_combine_ragged_backprop_weights_typed: ", c);
  if (forward)
    return tfra_table_find_combine_ragged_backprop_weights(tp, n_rows, row_splits, nnz, ids, weights, combiner, flags, fill_id,
                                                           default_row, (const float*)grad_out->grads, dw_out, stream);
  return wgrad_ragged_impl("find_combine_ragged_backprop_weights_typed", tp, n_rows, row_splits, nnz, ids, weights, combiner, flags,
                           fill_id, default_row, grads_for_twin(*grad_out), grad_out, dw_out, stream);
}
