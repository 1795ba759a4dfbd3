// The pooled lookup and the gradient of its weights for LONG WIDE rows: tfra_table_find_combine_wide_long,
// tfra_table_find_combine_ragged_wide_long and their *_backprop_weights_wide_long forms.  The wide forms
// (tfra_pool_wide.hip) give an output row of a 256 < dim <= 1024 table to one wave64, which suits the handful of ids of a categorical
// feature; a click or watch history of a few hundred items, each a 512 to 1024 column content embedding, leaves that wave walking
// the row four entries at a time with three quarters of its cycles spent waiting.  Here ONE block owns an output row: the forward
// gives each of its NCW = ceil(dim / 256) waves a 256-column chunk and the block 4 NCW probes in flight, the gradient gives each of
// its sixteen 16-lane groups an entry (the bodies and why the bits are the wide forms': tfra_pool_wide_long_device.h).
// The calls take the wide forms' argument lists and run their host frames (the four *_call templates of tfra_pool.h over a
// WideOwner): checks, refusals, locking, nnz == 0 behaviour and what is enqueued are theirs; what stands here is each call's launch.
// Not provided in this form: typed outputs (tfra_rows_out), a half grad_out (tfra_grads), tiers, the grouped *_many calls, and a
// mixed short / long dispatch at wide dims.
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
#include "tfra_pool_wide_long_device.h"

using namespace tfra;

namespace {

constexpr int WGRAD_THREADS = 16 * WIDE_LONG_GROUPS;   // sixteen groups, one entry each

template <int DT, int NCW, bool RAGGED, bool SAFE>
__global__ __launch_bounds__(64 * NCW) void find_combine_wide_long_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                          const float* __restrict__ w,
                                                                          const int* __restrict__ start_end, RaggedArgs rg, int combiner,
                                                                          const unsigned char* __restrict__ default_row,
                                                                          float* __restrict__ out) {
  find_combine_wide_long_row<DT, NCW, RAGGED, SAFE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out, blockIdx.x, rg);
}

template <int DT, int NCW, bool RAGGED, bool PRUNE>
__global__ __launch_bounds__(WGRAD_THREADS) void wgrad_wide_long_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                        const float* __restrict__ w, const int* __restrict__ start_end,
                                                                        RaggedArgs rg, int combiner,
                                                                        const unsigned char* __restrict__ default_row,
                                                                        const float* __restrict__ grad_out, float* dw) {
  wgrad_wide_long_row<DT, NCW, RAGGED, PRUNE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, grad_out, dw, blockIdx.x, rg);
}

// launch(DT, NCW, FLAG) for a table's storage type, NCW = ceil(dim / 256) in 2 .. 4 (WideOwner's rule has refused every other dim)
// and the ragged forms' last axis (SAFE / PRUNE; false for the tuple forms).  The grid is n_rows: one block per output row.
template <class F>
void with_wide_long_class(int st, int dim, bool flag, F&& launch) {
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

}  // namespace

extern "C" int tfra_table_find_combine_wide_long(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                 const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                 const void* default_row, float* out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_call("find_combine_wide_long", WideOwner(tp), ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out, out,
                           sizeof(float), s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_wide_long_class(st_index(t->opts.value_dtype), dim, false, [&](auto DT, auto NCW, auto) {
      find_combine_wide_long_kernel<DT, NCW, false, false><<<(unsigned)n_rows, 64 * NCW, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, out);
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_wide_long(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                        const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                        int64_t fill_id, const void* default_row, float* out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_call("find_combine_ragged_wide_long", WideOwner(tp), n_rows, row_splits, nnz, ids, weights, combiner,
                                  flags, default_row, out, out, sizeof(float), s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};
    with_wide_long_class(st_index(t->opts.value_dtype), dim, ragged_safe(flags, weights), [&](auto DT, auto NCW, auto SAFE) {
      find_combine_wide_long_kernel<DT, NCW, true, SAFE><<<(unsigned)n_rows, 64 * NCW, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, out);
    });
  });
}

extern "C" int tfra_table_find_combine_backprop_weights_wide_long(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz,
                                                                  const int64_t* ids, const int64_t* seg, const float* weights,
                                                                  int combiner, size_t n_rows, const void* default_row,
                                                                  const float* grad_out, float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_wgrad_call("find_combine_backprop_weights_wide_long", WideOwner(tp), ws, nnz, ids, seg, weights, combiner,
                                 n_rows, default_row, grad_out, dw_out, s, [&](const int* se) {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    with_wide_long_class(st_index(t->opts.value_dtype), dim, false, [&](auto DT, auto NCW, auto) {
      wgrad_wide_long_kernel<DT, NCW, false, false><<<(unsigned)n_rows, WGRAD_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, se, RaggedArgs{}, combiner, (const unsigned char*)default_row, grad_out, dw_out);
    });
  });
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights_wide_long(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits,
                                                                         size_t nnz, const int64_t* ids, const float* weights,
                                                                         int combiner, uint32_t flags, int64_t fill_id,
                                                                         const void* default_row, const float* grad_out, float* dw_out,
                                                                         tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  return find_combine_ragged_wgrad_call("find_combine_ragged_backprop_weights_wide_long", WideOwner(tp), n_rows, row_splits, nnz, ids,
                                        weights, combiner, flags, default_row, grad_out, dw_out, s, [&] {
    const int dim = t->opts.dim;
    const TableView v = t->view_of(t->cur);
    const RaggedArgs rg{(const i64*)row_splits, (int)nnz, flags, (i64)fill_id};   // (fill_id is not looked up: a filled row has no members)
    with_wide_long_class(st_index(t->opts.value_dtype), dim, wgrad_prune(flags, weights), [&](auto DT, auto NCW, auto PRUNE) {
      wgrad_wide_long_kernel<DT, NCW, true, PRUNE><<<(unsigned)n_rows, WGRAD_THREADS, 0, s>>>(
          v, n_rows, dim, (const i64*)ids, weights, nullptr, rg, combiner, (const unsigned char*)default_row, grad_out, dw_out);
    });
  });
}
