// The pooled lookups with a half-precision output: tfra_table_find_combine_typed, tfra_table_find_combine_ragged_typed,
// tfra_multi_find_combine_typed and tfra_multi_find_combine_ragged_typed.  Each equals its twin of tfra_pool.hip followed by the
// elementwise conversion of the twin's float32 output, bit for bit: the body is the twin's, find_combine_row (tfra_pool_device.h),
// with its OT axis, which narrows the float4 at the function's two stores and nowhere else.  A float32 output forwards to the twin.
// The four kernels are tfra_pool.hip's with that axis.  They are instantiated HERE, under names of their own, for the two half
// outputs only: the untyped kernels keep their names, their unit and their code (profiles/typed_lookup_isa_stats.txt).
// Host side: the single calls run the twins' checks (check_find_combine / check_find_combine_ragged, tfra_pool.h) behind the check
// of the output record (check_rows_out) and the twins' launch ladders with the output type in front; the grouped calls are the
// twins' frames (tfra_pool_many.h), where the output type is one more launch-class axis.
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
#include "tfra_pool_device.h"
#include "tfra_pool_many.h"

using namespace tfra;

namespace {

template <int DT, int U, int NCH, int OT>
__global__ __launch_bounds__(256) void find_combine_typed_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                 const float* __restrict__ w, const int* __restrict__ start_end,
                                                                 int combiner, const unsigned char* __restrict__ default_row,
                                                                 float* __restrict__ out) {
  find_combine_row<DT, U, NCH, false, false, false, OT>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out,
                                                        ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

template <int DT, int U, int NCH, int OT>
__global__ __launch_bounds__(256) void find_combine_many_typed_kernel(const ManyRec* __restrict__ recs,
                                                                      const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const ManyRec rec = recs[d];
  find_combine_row<DT, U, NCH, false, false, false, OT>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, rec.combiner,
                                                        rec.default_row, rec.out,
                                                        ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

template <int DT, int U, int NCH, bool SAFE, int OT>
__global__ __launch_bounds__(256) void find_combine_ragged_typed_kernel(TableView v, size_t n_rows, int dim,
                                                                        const i64* __restrict__ ids, const float* __restrict__ w,
                                                                        const i64* __restrict__ row_splits, int nnz, int combiner,
                                                                        unsigned flags, i64 fill_id,
                                                                        const unsigned char* __restrict__ default_row,
                                                                        float* __restrict__ out) {
  find_combine_row<DT, U, NCH, true, SAFE, false, OT>(v, n_rows, dim, ids, w, nullptr, combiner, default_row, out,
                                                      ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4,
                                                      RaggedArgs{row_splits, nnz, flags, fill_id});
}

// (NCH == 2 without SAFE: the untyped twins and the single-table typed kernels hold 75 to 77 VGPRs, 6 waves per SIMD; left alone,
// the register allocator gives the float32 -> bfloat16 instantiation of THIS kernel 82, 5 waves.  Told the twins' class it finds
// 77 for all six, with nothing spilled.)
template <int DT, int U, int NCH, bool SAFE, int OT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NCH == 2 && !SAFE ? 6 : 1)))
void find_combine_ragged_many_typed_kernel(const RaggedRec* __restrict__ recs,
                                                                             const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const RaggedRec rec = recs[d];
  find_combine_row<DT, U, NCH, true, SAFE, false, OT>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.combiner,
                                                      rec.default_row, rec.out,
                                                      ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4,
                                                      RaggedArgs{rec.row_splits, rec.nnz, rec.flags, rec.fill_id});
}

// launch(DT, U, NCH, OT) / launch(DT, U, NCH, SAFE, OT): the twins' ladders with the half output type (st_index: 1 | 2) in front
template <class F>
void with_half_out(int ot, F&& f) {
  if (ot == 1) f(std::integral_constant<int, TFRA_F16>{});
  else f(std::integral_constant<int, TFRA_BF16>{});
}
template <class F>
void with_pool_out_class(int ot, int st, int nch, F&& launch) {
  with_half_out(ot, [&](auto OT) { with_pool_class(st, nch, [&](auto DT, auto U, auto NCH) { launch(DT, U, NCH, OT); }); });
}
template <class F>
void with_ragged_out_class(int ot, int st, int nch, bool safe, F&& launch) {
  with_half_out(ot, [&](auto OT) {
    with_ragged_class(st, nch, safe, [&](auto DT, auto U, auto NCH, auto SAFE) { launch(DT, U, NCH, SAFE, OT); });
  });
}

}  // namespace

namespace tfra {
// cls = (output type index - 1) * 9 + storage type index * 3 + NCH index (tfra_pool_many.h)
void launch_find_combine_many_typed(hipStream_t s, int cls, unsigned grid, const ManyRec* recs, const unsigned* prefix, unsigned n) {
  with_pool_out_class(cls / 9 + 1, cls % 9 / 3, cls % 3, [&](auto DT, auto U, auto NCH, auto OT) {
    find_combine_many_typed_kernel<DT, U, NCH, OT><<<grid, 256, 0, s>>>(recs, prefix, n);
  });
}
void launch_find_combine_ragged_many_typed(hipStream_t s, int cls, bool safe, unsigned grid, const RaggedRec* recs,
                                           const unsigned* prefix, unsigned n) {
  with_ragged_out_class(cls / 9 + 1, cls % 9 / 3, cls % 3, safe, [&](auto DT, auto U, auto NCH, auto SAFE, auto OT) {
    find_combine_ragged_many_typed_kernel<DT, U, NCH, SAFE, OT><<<grid, 256, 0, s>>>(recs, prefix, n);
  });
}
}  // namespace tfra

extern "C" int tfra_table_find_combine_typed(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                             const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                             const void* default_row, const tfra_rows_out* out, tfra_stream_t stream) {
  if (Check c = check_rows_out(out); c.code) return report("find_combine_typed: ", c);
  if (out->dtype == TFRA_F32)   // the twin's own type: its code and its launches
    return tfra_table_find_combine(tp, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, static_cast<float*>(out->rows), stream);
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out_for_twin(*out), [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_unique + tfra_table_find + tfra_sparse_segment_combine otherwise)";
  if (c.code) return report("find_combine_typed: ", c);
  if (!c.active) return TFRA_OK;
  const int dim = t->opts.dim;
  if (nnz == 0) {   // the twin's zeros: +0.0 is all-zero bits in every type
    HIP_TRY(hipMemsetAsync(out->rows, 0, n_rows * (size_t)dim * 2, s));
    return TFRA_OK;
  }
  int rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_pool_out_class(st_index(out->dtype), st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto U, auto NCH, auto OT) {
    find_combine_typed_kernel<DT, U, NCH, OT><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                                     (const unsigned char*)default_row, static_cast<float*>(out->rows));
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

extern "C" int tfra_table_find_combine_ragged_typed(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                    const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                    int64_t fill_id, const void* default_row, const tfra_rows_out* out,
                                                    tfra_stream_t stream) {
  if (Check c = check_rows_out(out); c.code) return report("find_combine_ragged_typed: ", c);
  if (out->dtype == TFRA_F32)   // the twin's own type: its code and its launches
    return tfra_table_find_combine_ragged(tp, n_rows, row_splits, nnz, ids, weights, combiner, flags, fill_id, default_row,
                                          static_cast<float*>(out->rows), stream);
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row,
                                      out_for_twin(*out), [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_unique + tfra_table_find + tfra_sparse_segment_combine otherwise)";
  if (c.code) return report("find_combine_ragged_typed: ", c);
  if (!c.active) return TFRA_OK;
  const int dim = t->opts.dim;
  if (nnz == 0 && !(flags & TFRA_RAGGED_FILL)) {
    HIP_TRY(hipMemsetAsync(out->rows, 0, n_rows * (size_t)dim * 2, s));
    return TFRA_OK;
  }
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_ragged_out_class(st_index(out->dtype), st_index(t->opts.value_dtype), nch_index(dim), ragged_safe(flags, weights),
                        [&](auto DT, auto U, auto NCH, auto SAFE, auto OT) {
    find_combine_ragged_typed_kernel<DT, U, NCH, SAFE, OT><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights,
                                                                                  (const i64*)row_splits, (int)nnz, combiner, flags,
                                                                                  (i64)fill_id, (const unsigned char*)default_row,
                                                                                  static_cast<float*>(out->rows));
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

// ---- the grouped calls: the twins' frames over descriptors that carry an output record ------------------------------------------------
static PoolDesc typed_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_typed_desc& d = static_cast<const tfra_find_combine_typed_desc*>(descs)[i];
  PoolDesc p{d.struct_size == sizeof(tfra_find_combine_typed_desc), false, reinterpret_cast<Table*>(d.table), nullptr, d.combiner, d.nnz,
             d.ids, d.seg, nullptr, d.weights, d.n_rows, 0, 0, 0, d.default_row, nullptr};
  p.typed = &d.out;
  return p;
}
extern "C" int tfra_multi_find_combine_typed(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_typed_desc* descs,
                                             uint32_t* launches_out, tfra_stream_t stream) {
  return multi_find_combine_frame("multi_find_combine_typed", ws, n_tables, descs, typed_desc_at, launches_out, (hipStream_t)stream);
}

static PoolDesc typed_ragged_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_ragged_typed_desc& d = static_cast<const tfra_find_combine_ragged_typed_desc*>(descs)[i];
  PoolDesc p{d.struct_size == sizeof(tfra_find_combine_ragged_typed_desc), false, reinterpret_cast<Table*>(d.table), nullptr, d.combiner,
             d.nnz, d.ids, nullptr, d.row_splits, d.weights, d.n_rows, d.flags, d.reserved, d.fill_id, d.default_row, nullptr};
  p.typed = &d.out;
  return p;
}
extern "C" int tfra_multi_find_combine_ragged_typed(tfra_workspace_t* ws, size_t n_tables,
                                                    const tfra_find_combine_ragged_typed_desc* descs, uint32_t* launches_out,
                                                    tfra_stream_t stream) {
  return multi_find_combine_ragged_frame("multi_find_combine_ragged_typed", ws, n_tables, descs, typed_ragged_desc_at, launches_out,
                                         (hipStream_t)stream);
}
