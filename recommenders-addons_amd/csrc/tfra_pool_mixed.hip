// The pooled lookup and the gradient of its weights for MIXED row lengths: tfra_table_find_combine_mixed,
// tfra_table_find_combine_ragged_mixed and their *_backprop_weights_mixed forms.  The twins (tfra_pool.hip,
// tfra_wgrad.hip) give an output row to one 16-lane group, the long forms (tfra_pool_long.hip) to one 256-thread block; each loses
// several times on the other's ground, and a heavy-tailed sequence feature — most histories a handful of events, a few of them
// hundreds — has both kinds of rows in every batch.  Here a block owns 16 consecutive rows: the rows below long_from entries are
// walked by one group each with the twins' own functions, the rows from long_from on are done by the whole block one after the
// other with the long forms' windows (the bodies, the block-uniform mask every barrier hangs on, and the LDS budget:
// tfra_pool_mixed_device.h).  Whichever side of long_from a row falls on, its bits are the twins'.
// The calls take their twins' argument lists plus long_from and run their twins' host frames (the four *_call templates of
// tfra_pool.h over a TableOwner: checks, lock, early returns, the tuple forms' memset and bounds launch); what stands here is each
// call's launch.  float32 out and grad_out only: no typed, tiered or grouped forms.
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
#include "tfra_pool_mixed_device.h"

using namespace tfra;

namespace {

template <int DT, int NCH, bool RAGGED, bool SAFE>
__global__ __launch_bounds__(LONG_THREADS) void find_combine_mixed_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                          const float* __restrict__ w, const int* __restrict__ start_end,
                                                                          RaggedArgs rg, int combiner,
                                                                          const unsigned char* __restrict__ default_row,
                                                                          float* __restrict__ out, unsigned long_from) {
  find_combine_mixed_block<DT, NCH, RAGGED, SAFE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out, long_from, rg);
}

template <int DT, int NCH, bool RAGGED, bool PRUNE>
__global__ __launch_bounds__(LONG_THREADS) void wgrad_mixed_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                   const float* __restrict__ w, const int* __restrict__ start_end,
                                                                   RaggedArgs rg, int combiner,
                                                                   const unsigned char* __restrict__ default_row,
                                                                   const float* __restrict__ grad_out, float* dw, unsigned long_from) {
  wgrad_mixed_block<DT, NCH, RAGGED, PRUNE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, grad_out, dw, long_from, rg);
}

// 0: the library's default; a block per 16 rows (the frames launch only with n_rows > 0)
unsigned long_from_of(uint32_t long_from) { return long_from ? long_from : (uint32_t)TFRA_MIXED_LONG_FROM_DEFAULT; }
unsigned mixed_grid(size_t n_rows) { return (unsigned)((n_rows + MIXED_ROWS - 1) / MIXED_ROWS); }

}  // namespace

extern "C" int tfra_table_find_combine_mixed(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                             const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                             uint32_t long_from, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_call("find_combine_mixed", TableOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out, out,
                           sizeof(float), s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto, auto NCH) {
      find_combine_mixed_kernel<DT, NCH, false, false><<<mixed_grid(n_rows), LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, out,
          long_from_of(long_from));
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_mixed(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                    const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                    int64_t fill_id, const void* default_row, float* out, uint32_t long_from,
                                                    tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_call("find_combine_ragged_mixed", TableOwner(tp), n_rows, row_splits, nnz, ids, weights, combiner, flags,
                                  default_row, out, out, sizeof(float), s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};
    with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), ragged_safe(flags, weights), [&](auto DT, auto, auto NCH, auto SAFE) {
      find_combine_mixed_kernel<DT, NCH, true, SAFE><<<mixed_grid(n_rows), LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, out,
          long_from_of(long_from));
    });
  });
}

extern "C" int tfra_table_find_combine_backprop_weights_mixed(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                              const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                              const void* default_row, const float* grad_out, float* dw_out,
                                                              uint32_t long_from, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_wgrad_call("find_combine_backprop_weights_mixed", TableOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows,
                                 default_row, grad_out, dw_out, s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto, auto NCH) {
      wgrad_mixed_kernel<DT, NCH, false, false><<<mixed_grid(n_rows), LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, grad_out, dw_out,
          long_from_of(long_from));
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights_mixed(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits,
                                                                     size_t nnz, const int64_t* ids, const float* weights, int combiner,
                                                                     uint32_t flags, int64_t fill_id, const void* default_row,
                                                                     const float* grad_out, float* dw_out, uint32_t long_from,
                                                                     tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_wgrad_call("find_combine_ragged_backprop_weights_mixed", TableOwner(tp), n_rows, row_splits, nnz, ids,
                                        weights, combiner, flags, default_row, grad_out, dw_out, s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};   // (fill_id is not looked up: a filled row has no members)
    with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), wgrad_prune(flags, weights), [&](auto DT, auto, auto NCH, auto PRUNE) {
      wgrad_mixed_kernel<DT, NCH, true, PRUNE><<<mixed_grid(n_rows), LONG_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, grad_out, dw_out,
          long_from_of(long_from));
    });
  });
}
