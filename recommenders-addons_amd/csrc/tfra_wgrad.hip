// The gradient of the pooled lookup with respect to its WEIGHTS, straight from the table (tfra_table_find_combine_backprop_weights
// and its ragged form).  The reference gets it from TensorFlow's autodiff of `embeddings *= weights`, segment_sum and the divide
// (PY/dynamic_embedding_ops.py:233-291), which needs the [nnz, dim] rows the pooled lookup was built to avoid.  Here the launch has
// the forward's shape (find_combine_row, tfra_pool.hip): one 16-lane group per OUTPUT ROW, one probe and one row read per entry, the
// row's incoming gradient held in registers where the forward holds its accumulator, and [nnz] floats out.
// The arithmetic and its ONE evaluation order are tfra_combine_device.h's (wgrad_dot4, wgrad_reduce16, wgrad_s, wgrad_finish), the
// code seg_combine_wgrad_kernel (tfra_combine.hip: rows from a [U, dim] tensor) compiles, so the two routes agree bit for bit.
// The argument checks and the launch ladders are the forward's (tfra_pool.h); the kernels' body, wgrad_row, is in
// tfra_wgrad_device.h, where the tier's kernels (tfra_tierwgrad.hip) find it too.
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

}  // namespace

extern "C" int tfra_table_find_combine_backprop_weights(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                        const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                        const void* default_row, const float* grad_out, float* dw_out,
                                                        tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grad_out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report("find_combine_backprop_weights (out = grad_out): ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report("find_combine_backprop_weights: ", d);
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
    wgrad_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                        (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                               const int64_t* ids, const float* weights, int combiner,
                                                               uint32_t flags, int64_t fill_id, const void* default_row,
                                                               const float* grad_out, float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row, grad_out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report("find_combine_ragged_backprop_weights (out = grad_out): ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report("find_combine_ragged_backprop_weights: ", d);
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
    wgrad_ragged_kernel<DT, U, NCH, PRUNE><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, (const i64*)row_splits, (int)nnz,
                                                                    combiner, (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
