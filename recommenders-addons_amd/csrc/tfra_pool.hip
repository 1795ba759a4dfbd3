// Pooled lookup: the forward of embedding_lookup_sparse / safe_embedding_lookup_sparse straight from the table
// (tfra_table_find_combine).  The reference runs it as an op chain (PY/dynamic_embedding_ops.py:120-293):
//   tf.unique(ids)                                  :218-221   (a [U] tensor, idx[nnz], a host-visible count)
//   embedding_lookup(params, unique ids)            :223-231   (a [U, dim] tensor)
//   gather(idx) * weights, segment_sum, / sum w | / sqrt(sum w^2)   :233-291   (a [nnz, dim] tensor between them)
// A read needs no de-duplication (repeats of a hot id hit the cache), so here one 16-lane group per OUTPUT ROW walks the row's
// entries in input order, probes the table once per entry and accumulates w * row in registers: neither tensor exists and
// nothing is counted on the host.  The arithmetic is tfra_combine_device.h's, the code seg_combine_kernel (tfra_combine.hip)
// compiles, in the same order, so the result equals tfra_table_find + tfra_sparse_segment_combine bit for bit.
// tfra_multi_find_combine is the same lookup for a list of tables; its host side stands on the grouped-call frame of tfra_many.h,
// and both calls run ONE function for their argument checks (check_find_combine) and one launch ladder (with_pool_class); those
// live in tfra_pool.h, which the gradient of the lookup's weights (tfra_wgrad.hip) shares.
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
// What a single-table launch takes as kernel arguments is a record in device memory here (26 tables' records do not fit the 4 KB
// of kernel arguments: a TableView alone is 80 B).  The grid is the concatenation of the class's descriptors, descriptor d owning
// the blocks [prefix[d], prefix[d + 1]) = ceil(n_rows * 16 / 256) blocks, so that a block never straddles two descriptors.
struct ManyRec {
  TableView v;
  size_t n_rows;
  const i64* ids;
  const float* w;
  const int* se;
  const unsigned char* default_row;
  float* out;
  int dim;
  int combiner;
};
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

struct RaggedRec {
  TableView v;
  size_t n_rows;
  const i64* ids;
  const float* w;
  const i64* row_splits;
  const unsigned char* default_row;
  float* out;
  i64 fill_id;
  int nnz;
  int dim;
  int combiner;
  unsigned flags;
};

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

extern "C" int tfra_multi_find_combine(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_desc* descs,
                                       uint32_t* launches_out, tfra_stream_t stream) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, "multi_find_combine: null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and no out is written
  constexpr int NCLASS = 9;   // (float32 | float16 | bfloat16) x (NCH 1 | 2 | 4)
  std::vector<int> cls(n_tables, -1);
  std::vector<size_t> se_off(n_tables, 0);   // a descriptor's bounds in the bounds area, in input order
  size_t n_act = 0, n_bnd = 0, total_rows = 0;
  u64 bnd_blocks = 0;
  for (size_t i = 0; i < n_tables; ++i) {
    const tfra_find_combine_desc& d = descs[i];
    if (d.struct_size != sizeof(tfra_find_combine_desc))
      return set_error(TFRA_ERR_INVALID, "multi_find_combine: descriptor " + std::to_string(i) + ": descriptor size mismatch");
    const Table* t = reinterpret_cast<const Table*>(d.table);
    const Check c = check_find_combine(t, ws, d.nnz, d.ids, d.seg, d.weights, d.combiner, d.n_rows, d.default_row, d.out, [] { return Check{}; });
    if (c.code) return report("multi_find_combine: descriptor " + std::to_string(i) + ": ", c);
    if (!c.active) continue;
    cls[i] = st_index(t->opts.value_dtype) * 3 + nch_index(t->opts.dim);
    ++n_act;
    n_bnd += d.nnz ? 1 : 0;
    bnd_blocks += (d.nnz + 255) / 256;
    se_off[i] = 2 * total_rows;
    total_rows += d.n_rows;
  }
  if (n_act == 0) return TFRA_OK;
  // the records' order: class by class, input order inside a class
  auto row_blocks = [&](size_t i) { return (unsigned)((descs[i].n_rows * 16 + 255) / 256); };
  auto bnd_blocks_of = [&](size_t i) { return (unsigned)((descs[i].nnz + 255) / 256); };
  std::vector<size_t> order;
  order.reserve(n_act);
  size_t cls_first[NCLASS + 1];
  for (int c = 0; c < NCLASS; ++c) {
    cls_first[c] = order.size();
    u64 blocks = 0;
    for (size_t i = 0; i < n_tables; ++i)
      if (cls[i] == c) { order.push_back(i); blocks += row_blocks(i); }
    if (blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, "multi_find_combine: too many rows in one call");
  }
  cls_first[NCLASS] = order.size();
  if (bnd_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, "multi_find_combine: too many entries in one call");

  // (one table may stand in several descriptors: locked once)
  std::vector<Table*> tabs;
  tabs.reserve(n_act);
  for (size_t i : order) tabs.push_back(reinterpret_cast<Table*>(descs[i].table));
  std::vector<std::unique_lock<std::mutex>> locks;
  int rc = lock_and_enter(std::move(tabs), s, &locks);
  if (rc) return rc;

  // device memory: [bounds of all rows | blob], the blob = [records | per-class block prefixes | bounds records | their block prefix]
  const size_t se_bytes = (2 * total_rows * sizeof(int) + 255) / 256 * 256;
  Blob blob;
  const size_t rec_off = blob.add<ManyRec>(n_act), cpre_off = blob.add<unsigned>(ClassPool::words(n_act, NCLASS, false));
  const size_t brec_off = blob.add<BoundsRec>(n_bnd), bpre_off = blob.add<unsigned>(ClassPool::words(n_bnd, 1, false));
  ManyUpload up;
  rc = many_begin(ws, se_bytes, blob.bytes(), s, &up);
  if (rc) return rc;
  int* se_base = (int*)ws->buf;
  ManyRec* recs = section<ManyRec>(up.host, rec_off);
  BoundsRec* brecs = section<BoundsRec>(up.host, brec_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  for (size_t k = 0; k < n_act; ++k) {
    const tfra_find_combine_desc& d = descs[order[k]];
    Table* t = reinterpret_cast<Table*>(d.table);
    recs[k] = ManyRec{t->view_of(t->cur), d.n_rows, (const i64*)d.ids, d.weights, se_base + se_off[order[k]],
                      (const unsigned char*)d.default_row, d.out, t->opts.dim, d.combiner};
  }
  // the records stand in class order: a class is a range of them and needs no index
  ClassPool cpool{section<unsigned>(up.host, cpre_off)};
  ManyClass row_cls[NCLASS];
  for (int c = 0; c < NCLASS; ++c)
    row_cls[c] = cpool.put(n_act, false, [&](size_t k) { return k >= cls_first[c] && k < cls_first[c + 1]; },
                           [&](size_t k) { return row_blocks(order[k]); });
  auto bounded = [&](size_t i) { return cls[i] >= 0 && descs[i].nnz != 0; };
  {
    size_t k = 0;
    for (size_t i = 0; i < n_tables; ++i)
      if (bounded(i)) brecs[k++] = BoundsRec{(const i64*)descs[i].seg, se_base + se_off[i], descs[i].nnz, descs[i].n_rows};
  }
  const ManyClass bnd = ClassPool{section<unsigned>(up.host, bpre_off)}.put(n_tables, false, bounded, bnd_blocks_of);
  rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(se_base, 0, 2 * total_rows * sizeof(int), s));   // empty rows (and every row of an nnz == 0 descriptor): 0, 0
  uint32_t launches = 0;
  if (bnd.n) {
    seg64_bounds_many_kernel<<<bnd.grid, 256, 0, s>>>(section<const BoundsRec>(up.dev, brec_off), section<const unsigned>(up.dev, bpre_off), bnd.n);
    ++launches;
  }
  for (int c = 0; c < NCLASS; ++c) {
    const ManyClass& k = row_cls[c];
    if (!k.n) continue;
    const ManyRec* r = section<const ManyRec>(up.dev, rec_off) + cls_first[c];
    const unsigned* p = section<const unsigned>(up.dev, cpre_off) + k.at;
    with_pool_class(c / 3, c % 3, [&](auto DT, auto U, auto NCH) {
      find_combine_many_kernel<DT, U, NCH><<<k.grid, 256, 0, s>>>(r, p, k.n);
    });
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
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

extern "C" int tfra_multi_find_combine_ragged(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_ragged_desc* descs,
                                              uint32_t* launches_out, tfra_stream_t stream) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, "multi_find_combine_ragged: null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and no out is written
  constexpr int NCLASS = 18;   // (float32 | float16 | bfloat16) x (NCH 1 | 2 | 4) x (plain | safe)
  std::vector<int> cls(n_tables, -1);
  size_t n_act = 0;
  for (size_t i = 0; i < n_tables; ++i) {
    const tfra_find_combine_ragged_desc& d = descs[i];
    if (d.struct_size != sizeof(tfra_find_combine_ragged_desc))
      return set_error(TFRA_ERR_INVALID, "multi_find_combine_ragged: descriptor " + std::to_string(i) + ": descriptor size mismatch");
    const Table* t = reinterpret_cast<const Table*>(d.table);
    const Check c = check_find_combine_ragged(t, ws, d.n_rows, d.row_splits, d.nnz, d.ids, d.weights, d.combiner, d.flags, d.reserved,
                                              d.default_row, d.out, [] { return Check{}; });
    if (c.code) return report("multi_find_combine_ragged: descriptor " + std::to_string(i) + ": ", c);
    if (!c.active) continue;
    cls[i] = (st_index(t->opts.value_dtype) * 3 + nch_index(t->opts.dim)) * 2 + (ragged_safe(d.flags, d.weights) ? 1 : 0);
    ++n_act;
  }
  if (n_act == 0) return TFRA_OK;
  // the records' order: class by class, input order inside a class
  auto row_blocks = [&](size_t i) { return (unsigned)((descs[i].n_rows * 16 + 255) / 256); };
  std::vector<size_t> order;
  order.reserve(n_act);
  size_t cls_first[NCLASS + 1];
  for (int c = 0; c < NCLASS; ++c) {
    cls_first[c] = order.size();
    u64 blocks = 0;
    for (size_t i = 0; i < n_tables; ++i)
      if (cls[i] == c) { order.push_back(i); blocks += row_blocks(i); }
    if (blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, "multi_find_combine_ragged: too many rows in one call");
  }
  cls_first[NCLASS] = order.size();

  // (one table may stand in several descriptors: locked once)
  std::vector<Table*> tabs;
  tabs.reserve(n_act);
  for (size_t i : order) tabs.push_back(reinterpret_cast<Table*>(descs[i].table));
  std::vector<std::unique_lock<std::mutex>> locks;
  int rc = lock_and_enter(std::move(tabs), s, &locks);
  if (rc) return rc;

  // device memory: the blob alone = [records | per-class block prefixes]; there are no bounds to keep
  Blob blob;
  const size_t rec_off = blob.add<RaggedRec>(n_act), cpre_off = blob.add<unsigned>(ClassPool::words(n_act, NCLASS, false));
  ManyUpload up;
  rc = many_begin(ws, 0, blob.bytes(), s, &up);
  if (rc) return rc;
  RaggedRec* recs = section<RaggedRec>(up.host, rec_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  for (size_t k = 0; k < n_act; ++k) {
    const tfra_find_combine_ragged_desc& d = descs[order[k]];
    Table* t = reinterpret_cast<Table*>(d.table);
    recs[k] = RaggedRec{t->view_of(t->cur), d.n_rows, (const i64*)d.ids, d.weights, (const i64*)d.row_splits,
                        (const unsigned char*)d.default_row, d.out, (i64)d.fill_id, (int)d.nnz, t->opts.dim, d.combiner, d.flags};
  }
  ClassPool cpool{section<unsigned>(up.host, cpre_off)};
  ManyClass row_cls[NCLASS];
  for (int c = 0; c < NCLASS; ++c)
    row_cls[c] = cpool.put(n_act, false, [&](size_t k) { return k >= cls_first[c] && k < cls_first[c + 1]; },
                           [&](size_t k) { return row_blocks(order[k]); });
  rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true);
  if (rc) return rc;
  uint32_t launches = 0;
  for (int c = 0; c < NCLASS; ++c) {
    const ManyClass& k = row_cls[c];
    if (!k.n) continue;
    const RaggedRec* r = section<const RaggedRec>(up.dev, rec_off) + cls_first[c];
    const unsigned* p = section<const unsigned>(up.dev, cpre_off) + k.at;
    with_ragged_class(c / 6, (c / 2) % 3, c & 1, [&](auto DT, auto U, auto NCH, auto SAFE) {
      find_combine_ragged_many_kernel<DT, U, NCH, SAFE><<<k.grid, 256, 0, s>>>(r, p, k.n);
    });
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}
