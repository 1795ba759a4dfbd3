// Pooled lookup: the forward of embedding_lookup_sparse / safe_embedding_lookup_sparse straight from the table
// (tfra_table_find_combine).  The reference runs it as an op chain (PY/dynamic_embedding_ops.py:120-293):
//   tf.unique(ids)                                  :218-221   (a [U] tensor, idx[nnz], a host-visible count)
//   embedding_lookup(params, unique ids)            :223-231   (a [U, dim] tensor)
//   gather(idx) * weights, segment_sum, / sum w | / sqrt(sum w^2)   :233-291   (a [nnz, dim] tensor between them)
// A read needs no de-duplication (repeats of a hot id hit the cache), so here one 16-lane group per OUTPUT ROW walks the row's
// entries in input order, probes the table once per entry and accumulates w * row in registers: neither tensor exists and
// nothing is counted on the host.  The arithmetic is tfra_combine_device.h's, the code seg_combine_kernel (tfra_combine.hip)
// compiles, in the same order, so the result equals tfra_table_find + tfra_sparse_segment_combine bit for bit.
// tfra_multi_find_combine is the same lookup for a list of tables; its host side is the frame the grouped lookup over tiers shares
// (multi_find_combine_frame, tfra_tierpool_many.hip, on the grouped-call pieces of tfra_many.h), which launches this unit's kernels
// through launch_find_combine_many.  Both calls run ONE function for their argument checks (check_find_combine) and one launch
// ladder (with_pool_class); those live in tfra_pool.h, which the gradient of the lookup's weights (tfra_wgrad.hip) shares.
// tfra_table_find_combine_ragged / tfra_multi_find_combine_ragged are the two calls over a rank-2 RaggedTensor (PY/ragged_embedding_ops.py:
// 129-442): the row's entry range comes from row_splits, so ONE launch serves a call, and safe_embedding_lookup_sparse's pruning by
// weight and its default_id run inside that launch (find_combine_row's RAGGED and SAFE axes; check_find_combine_ragged, with_ragged_class).
// find_combine_row itself, the body of every kernel here, lives in tfra_pool_device.h: the tier's pooled lookup (tfra_tierpool.hip) shares it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

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

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void find_combine_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                           const float* __restrict__ w, const int* __restrict__ start_end,
                                                           int combiner, const unsigned char* __restrict__ default_row,
                                                           float* __restrict__ out) {
  find_combine_row<DT, U, NCH>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out,
                               ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

// ---- the grouped form (tfra_multi_find_combine): the lookups of a LIST of tables in one launch per (value dtype, NCH) class ------
// What a single-table launch takes as kernel arguments is a record in device memory here (ManyRec: tfra_pool_many.h, which the
// tier's grouped kernels share).
// (BoundsRec, the record of the bounds launch, and many_desc_of, the search that takes a block to its descriptor: tfra_many.h)

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void find_combine_many_kernel(const ManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                                unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const ManyRec rec = recs[d];
  find_combine_row<DT, U, NCH>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, rec.combiner, rec.default_row, rec.out,
                               ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

// ---- the ragged forms (tfra_table_find_combine_ragged / tfra_multi_find_combine_ragged): the bounds come with the batch -------------
// The same launch shape — 256 threads, one 16-lane group per output row, no LDS — and no launch before it: a ragged batch carries
// each row's entry range, which the tuple form recovers from seg with a memset and a bounds launch.  SAFE is chosen on the host:
// a call whose flags change nothing (no FILL, and PRUNE without weights) runs the kernel that does not look at them.
template <int DT, int U, int NCH, bool SAFE>
__global__ __launch_bounds__(256) void find_combine_ragged_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                                  const float* __restrict__ w, const i64* __restrict__ row_splits,
                                                                  int nnz, int combiner, unsigned flags, i64 fill_id,
                                                                  const unsigned char* __restrict__ default_row,
                                                                  float* __restrict__ out) {
  find_combine_row<DT, U, NCH, true, SAFE>(v, n_rows, dim, ids, w, nullptr, combiner, default_row, out,
                                           ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4, RaggedArgs{row_splits, nnz, flags, fill_id});
}

// (RaggedRec, the ragged record: tfra_pool_many.h)
template <int DT, int U, int NCH, bool SAFE>
__global__ __launch_bounds__(256) void find_combine_ragged_many_kernel(const RaggedRec* __restrict__ recs,
                                                                       const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const RaggedRec rec = recs[d];
  find_combine_row<DT, U, NCH, true, SAFE>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.combiner, rec.default_row, rec.out,
                                           ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4,
                                           RaggedArgs{rec.row_splits, rec.nnz, rec.flags, rec.fill_id});
}

// seg64_bounds_kernel (tfra_combine.hip) over a list: descriptor d owns ceil(nnz / 256) blocks and p counts ITS entries, so the
// neighbours p - 1 / p + 1 are never read across a descriptor's end.  se zeroed before (empty rows: 0, 0).
__global__ __launch_bounds__(256) void seg64_bounds_many_kernel(const BoundsRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                                unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const BoundsRec rec = recs[d];
  const size_t p = (size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x;
  if (p >= rec.nnz) return;
  const i64 s = rec.seg[p];
  if (s < 0 || (size_t)s >= rec.n_rows) return;
  if (p == 0 || rec.seg[p - 1] != s) rec.se[s] = (int)p;
  if (p == rec.nnz - 1 || rec.seg[p + 1] != s) rec.se[rec.n_rows + s] = (int)p + 1;
}

}  // namespace

extern "C" int tfra_table_find_combine(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                       const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                       tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_unique + tfra_table_find + tfra_sparse_segment_combine otherwise)";
  if (c.code) return report("find_combine: ", c);
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
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto U, auto NCH) {
    find_combine_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                               (const unsigned char*)default_row, out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

namespace tfra {
int comb_bounds_many(hipStream_t s, unsigned grid, const BoundsRec* recs, const unsigned* prefix, unsigned n) {
  seg64_bounds_many_kernel<<<grid, 256, 0, s>>>(recs, prefix, n);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

// the one instantiation of the grouped one-table kernels, for the frames of tfra_tierpool_many.hip (cls: tfra_pool_many.h)
void launch_find_combine_many(hipStream_t s, int cls, unsigned grid, const ManyRec* recs, const unsigned* prefix, unsigned n) {
  with_pool_class(cls / 3, cls % 3, [&](auto DT, auto U, auto NCH) {
    find_combine_many_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(recs, prefix, n);
  });
}
void launch_find_combine_ragged_many(hipStream_t s, int cls, bool safe, unsigned grid, const RaggedRec* recs, const unsigned* prefix,
                                     unsigned n) {
  with_ragged_class(cls / 3, cls % 3, safe, [&](auto DT, auto U, auto NCH, auto SAFE) {
    find_combine_ragged_many_kernel<DT, U, NCH, SAFE><<<grid, 256, 0, s>>>(recs, prefix, n);
  });
}

void destroy_workspace_many(void* p) {
  ManyStage* st = reinterpret_cast<ManyStage*>(p);
  if (!st) return;
  for (int i = 0; i < ManyStage::RING; ++i) {
    if (st->pending[i]) (void)hipEventSynchronize(st->ev[i]);
    if (st->ev[i]) (void)hipEventDestroy(st->ev[i]);
  }
  if (st->host) (void)hipHostFree(st->host);
  delete st;
}
}  // namespace tfra

// The grouped calls' host side is ONE frame per form (multi_find_combine_frame / multi_find_combine_ragged_frame, tfra_tierpool_many.hip),
// over descriptors of this ABI or of the tier ABI; the launches of the one-table classes come back here (the launchers above).
static PoolDesc plain_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_desc& d = static_cast<const tfra_find_combine_desc*>(descs)[i];
  return PoolDesc{d.struct_size == sizeof(tfra_find_combine_desc), false, reinterpret_cast<Table*>(d.table), nullptr, d.combiner, d.nnz,
                  d.ids, d.seg, nullptr, d.weights, d.n_rows, 0, 0, 0, d.default_row, d.out};
}
extern "C" int tfra_multi_find_combine(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_desc* descs,
                                       uint32_t* launches_out, tfra_stream_t stream) {
  return multi_find_combine_frame("multi_find_combine", ws, n_tables, descs, plain_desc_at, launches_out, (hipStream_t)stream);
}

// ---- the ragged calls ------------------------------------------------------------------------------------------------------------------
extern "C" int tfra_table_find_combine_ragged(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz, const int64_t* ids,
                                              const float* weights, int combiner, uint32_t flags, int64_t fill_id,
                                              const void* default_row, float* out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row, out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_unique + tfra_table_find + tfra_sparse_segment_combine otherwise)";
  if (c.code) return report("find_combine_ragged: ", c);
  if (!c.active) return TFRA_OK;
  const int dim = t->opts.dim;
  if (nnz == 0 && !(flags & TFRA_RAGGED_FILL)) {
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * sizeof(float), s));
    return TFRA_OK;
  }
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), ragged_safe(flags, weights), [&](auto DT, auto U, auto NCH, auto SAFE) {
    find_combine_ragged_kernel<DT, U, NCH, SAFE><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, (const i64*)row_splits,
                                                                           (int)nnz, combiner, flags, (i64)fill_id,
                                                                           (const unsigned char*)default_row, out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

static PoolDesc plain_ragged_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_ragged_desc& d = static_cast<const tfra_find_combine_ragged_desc*>(descs)[i];
  return PoolDesc{d.struct_size == sizeof(tfra_find_combine_ragged_desc), false, reinterpret_cast<Table*>(d.table), nullptr, d.combiner,
                  d.nnz, d.ids, nullptr, d.row_splits, d.weights, d.n_rows, d.flags, d.reserved, d.fill_id, d.default_row, d.out};
}
extern "C" int tfra_multi_find_combine_ragged(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_ragged_desc* descs,
                                              uint32_t* launches_out, tfra_stream_t stream) {
  return multi_find_combine_ragged_frame("multi_find_combine_ragged", ws, n_tables, descs, plain_ragged_desc_at, launches_out,
                                         (hipStream_t)stream);
}
