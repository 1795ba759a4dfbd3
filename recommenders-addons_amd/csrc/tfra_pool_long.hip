// The pooled lookup and the gradient of its weights for LONG rows: tfra_table_find_combine_long, tfra_table_find_combine_ragged_long
// and their *_backprop_weights_long forms.  The twins (tfra_pool.hip, tfra_wgrad.hip) give an output row to one 16-lane
// group, which is right for the 1 - 30 ids of a categorical feature; a sequence feature — a click or watch history of a few hundred
// ids pooled by sum or mean — leaves a handful of waves walking their rows one latency after the other.  Here ONE 256-thread block
// owns an output row: its 16 groups probe and read the row's entries in parallel, window by window, and the adds alone stay serial,
// in entry order and with the twins' expressions (the bodies and why the bits are the twins': tfra_pool_long_device.h).
// The calls take their twins' argument lists and run their twins' host frames (the four *_call templates of tfra_pool.h over a
// TableOwner: checks, lock, early returns, the tuple forms' memset and bounds launch); what stands here is each call's launch.  The
// ragged forward is one launch.  float32 out and grad_out only: no typed or tiered forms (the grouped forms: tfra_pool_long_many.hip).
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
#include "tfra_pool_long_device.h"

using namespace tfra;

namespace {

template <int DT, int NCH, bool RAGGED, bool SAFE>
__global__ __launch_bounds__(LONG_THREADS) void find_combine_long_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                         const float* __restrict__ w, const int* __restrict__ start_end,
                                                                         RaggedArgs rg, int combiner,
                                                                         const unsigned char* __restrict__ default_row,
                                                                         float* __restrict__ out) {
  find_combine_long_row<DT, NCH, RAGGED, SAFE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out, blockIdx.x, rg);
}

template <int DT, int NCH, bool RAGGED, bool PRUNE>
__global__ __launch_bounds__(LONG_THREADS) void wgrad_long_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                  const float* __restrict__ w, const int* __restrict__ start_end,
                                                                  RaggedArgs rg, int combiner,
                                                                  const unsigned char* __restrict__ default_row,
                                                                  const float* __restrict__ grad_out, float* dw) {
  wgrad_long_row<DT, NCH, RAGGED, PRUNE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, grad_out, dw, blockIdx.x, rg);
}

}  // namespace

extern "C" int tfra_table_find_combine_long(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                            const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                            tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_call("find_combine_long", TableOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out, out,
                           sizeof(float), s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto, auto NCH) {
      find_combine_long_kernel<DT, NCH, false, false><<<(unsigned)n_rows, LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, out);
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_long(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                   const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                   int64_t fill_id, const void* default_row, float* out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_call("find_combine_ragged_long", TableOwner(tp), n_rows, row_splits, nnz, ids, weights, combiner, flags,
                                  default_row, out, out, sizeof(float), s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};
    with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), ragged_safe(flags, weights), [&](auto DT, auto, auto NCH, auto SAFE) {
      find_combine_long_kernel<DT, NCH, true, SAFE><<<(unsigned)n_rows, LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, out);
    });
  });
}

extern "C" int tfra_table_find_combine_backprop_weights_long(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                             const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                             const void* default_row, const float* grad_out, float* dw_out,
                                                             tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_wgrad_call("find_combine_backprop_weights_long", TableOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows,
                                 default_row, grad_out, dw_out, s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto, auto NCH) {
      wgrad_long_kernel<DT, NCH, false, false><<<(unsigned)n_rows, LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, grad_out, dw_out);
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights_long(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits,
                                                                    size_t nnz, const int64_t* ids, const float* weights, int combiner,
                                                                    uint32_t flags, int64_t fill_id, const void* default_row,
                                                                    const float* grad_out, float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_wgrad_call("find_combine_ragged_backprop_weights_long", TableOwner(tp), n_rows, row_splits, nnz, ids,
                                        weights, combiner, flags, default_row, grad_out, dw_out, s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};   // (fill_id is not looked up: a filled row has no members)
    with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), wgrad_prune(flags, weights), [&](auto DT, auto, auto NCH, auto PRUNE) {
      wgrad_long_kernel<DT, NCH, true, PRUNE><<<(unsigned)n_rows, LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, grad_out, dw_out);
    });
  });
}
