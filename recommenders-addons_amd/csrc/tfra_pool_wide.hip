// The pooled lookup and the gradient of its weights for WIDE rows: tfra_table_find_combine_wide, tfra_table_find_combine_ragged_wide
// and their *_backprop_weights_wide forms.  The twins (tfra_pool.hip, tfra_wgrad.hip) serve dim <= 256: one 16-lane
// group per output row, NCH <= 4 chunks of 64 columns per lane.  A table stores rows of any width, and a variable of 384, 512, 768 or
// 1024 columns — pretrained text or image embeddings, a wide user tower — had the op chain alone: unique, a host read of the count,
// tfra_table_find into a [U, dim] matrix and tfra_sparse_segment_combine reading it back.  Here ONE wave64 owns an output row, four
// rows per block: the forward splits the wave over columns, the gradient over entries (the bodies and why the bits are the chain's:
// tfra_pool_wide_device.h).  float32, float16 and bfloat16 tables with dim % 4 == 0 and 256 < dim <= 1024.
// The calls take their twins' argument lists and run their twins' host frames (the four *_call templates of tfra_pool.h) over a
// WideOwner, whose one difference from TableOwner is the width it asks for; what stands here is each call's launch.
// Not provided in this form: typed outputs (tfra_rows_out), a half grad_out (tfra_grads), tiers, the grouped *_many calls, long-row
// blocks at wide dims, and the planned write-back beyond dim 256 (a training lookup of such a variable keeps the op chain).
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
#include "tfra_pool_wide_device.h"

using namespace tfra;

namespace {

template <int DT, int NCW, bool RAGGED, bool SAFE>
__global__ __launch_bounds__(WIDE_THREADS) void find_combine_wide_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                         const float* __restrict__ w, const int* __restrict__ start_end,
                                                                         RaggedArgs rg, int combiner,
                                                                         const unsigned char* __restrict__ default_row,
                                                                         float* __restrict__ out) {
  find_combine_wide_row<DT, NCW, RAGGED, SAFE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out,
                                               (size_t)blockIdx.x * WIDE_ROWS + (threadIdx.x >> 6), rg);
}

template <int DT, int NCW, bool RAGGED, bool PRUNE>
__global__ __launch_bounds__(WIDE_THREADS) void wgrad_wide_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                  const float* __restrict__ w, const int* __restrict__ start_end,
                                                                  RaggedArgs rg, int combiner,
                                                                  const unsigned char* __restrict__ default_row,
                                                                  const float* __restrict__ grad_out, float* dw) {
  wgrad_wide_row<DT, NCW, RAGGED, PRUNE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, grad_out, dw,
                                         (size_t)blockIdx.x * WIDE_ROWS + (threadIdx.x >> 6), rg);
}

// launch(DT, NCW, FLAG) for a table's storage type, NCW = ceil(dim / 256) in 2 .. 4 (WideOwner's rule has refused every other dim)
// and the ragged forms' last axis (SAFE / PRUNE; false for the tuple forms)
template <class F>
void with_wide_class(int st, int dim, bool flag, F&& launch) {
  with_stored(st, [&](auto DT) {
    auto by_flag = [&](auto NCW) {
      if (flag) launch(DT, NCW, std::true_type{});
      else launch(DT, NCW, std::false_type{});
    };
    switch ((dim + 255) / 256) {
      case 2: by_flag(std::integral_constant<int, 2>{}); break;
      case 3: by_flag(std::integral_constant<int, 3>{}); break;
      default: by_flag(std::integral_constant<int, 4>{}); break;
    }
  });
}
unsigned wide_grid(size_t n_rows) { return (unsigned)((n_rows + WIDE_ROWS - 1) / WIDE_ROWS); }

}  // namespace

extern "C" int tfra_table_find_combine_wide(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                            const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                            tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_call("find_combine_wide", WideOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out, out,
                           sizeof(float), s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_wide_class(st_index(t->opts.value_dtype), dim, false, [&](auto DT, auto NCW, auto) {
      find_combine_wide_kernel<DT, NCW, false, false><<<wide_grid(n_rows), WIDE_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, out);
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_wide(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                   const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                   int64_t fill_id, const void* default_row, float* out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_call("find_combine_ragged_wide", WideOwner(tp), n_rows, row_splits, nnz, ids, weights, combiner, flags,
                                  default_row, out, out, sizeof(float), s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};
    with_wide_class(st_index(t->opts.value_dtype), dim, ragged_safe(flags, weights), [&](auto DT, auto NCW, auto SAFE) {
      find_combine_wide_kernel<DT, NCW, true, SAFE><<<wide_grid(n_rows), WIDE_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, out);
    });
  });
}

extern "C" int tfra_table_find_combine_backprop_weights_wide(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                             const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                             const void* default_row, const float* grad_out, float* dw_out,
                                                             tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_wgrad_call("find_combine_backprop_weights_wide", WideOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows,
                                 default_row, grad_out, dw_out, s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_wide_class(st_index(t->opts.value_dtype), dim, false, [&](auto DT, auto NCW, auto) {
      wgrad_wide_kernel<DT, NCW, false, false><<<wide_grid(n_rows), WIDE_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, grad_out, dw_out);
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights_wide(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits,
                                                                    size_t nnz, const int64_t* ids, const float* weights, int combiner,
                                                                    uint32_t flags, int64_t fill_id, const void* default_row,
                                                                    const float* grad_out, float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_wgrad_call("find_combine_ragged_backprop_weights_wide", WideOwner(tp), n_rows, row_splits, nnz, ids,
                                        weights, combiner, flags, default_row, grad_out, dw_out, s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};   // (fill_id is not looked up: a filled row has no members)
    with_wide_class(st_index(t->opts.value_dtype), dim, wgrad_prune(flags, weights), [&](auto DT, auto NCW, auto PRUNE) {
      wgrad_wide_kernel<DT, NCW, true, PRUNE><<<wide_grid(n_rows), WIDE_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, grad_out, dw_out);
    });
  });
}
