// The grouped pooled lookups over tiers: tfra_multi_tier_find_combine and tfra_multi_tier_find_combine_ragged, the
// pooled lookups of a LIST whose members are tiers (tfra_tier_find_combine / _ragged: tfra_tierpool.hip) or plain tables
// (tfra_table_find_combine / _ragged: tfra_pool.hip), in the enqueues tfra_multi_find_combine / _ragged take for plain tables alone.
// These are reads, as the single tier calls are: nothing moves between the tiers, no table is written, no score is touched, the
// drivers' statistics and staging are left alone.
// The kernels are find_combine_row (tfra_pool_device.h) with its TIER axis in the launch shape of find_combine_many_kernel; the
// plain members of a list run the kernels of tfra_pool.hip through its launchers (one instantiation of each kernel in the library).
// The host side of all four grouped pooled calls is here, ONE frame per form over a descriptor of either ABI (PoolDesc,
// tfra_pool_many.h): tfra_multi_find_combine / _ragged (tfra_pool.hip) call the same two functions with descriptors that name no tier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_pool_device.h"
#include "tfra_pool_many.h"
#include "tfra_tier.h"

using namespace tfra;

namespace {

// find_combine_many_kernel's launch shape — 256 threads, one 16-lane group per output row, descriptor d owning the blocks
// [prefix[d], prefix[d + 1]) — over records that hold both views.  Both views are copied out of the record (scalar loads: the
// record's address is uniform in the wave), as the single tier kernels get them as arguments: the generated code then has those
// kernels' register counts (within 2) and their waves per SIMD.  Handing find_combine_row the address of the record's lower view instead saves 2 scalar
// registers and costs 2 to 4 vector registers, which takes the safe ragged NCH = 2 kernels from 96 to 100 VGPRs, 5 to 4 waves per
// SIMD (both variants: profiles/tier_pooled_many_isa_stats.txt).
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void tier_find_combine_many_kernel(const TierManyRec* __restrict__ recs,
                                                                     const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const ManyRec rec = recs[d].r;
  const TableView lo = recs[d].lo;
  find_combine_row<DT, U, NCH, false, false, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, rec.combiner, rec.default_row,
                                                   rec.out, ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, RaggedArgs{},
                                                   &lo);
}

template <int DT, int U, int NCH, bool SAFE>
__global__ __launch_bounds__(256) void tier_find_combine_ragged_many_kernel(const TierRaggedRec* __restrict__ recs,
                                                                            const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const RaggedRec rec = recs[d].r;
  const TableView lo = recs[d].lo;
  find_combine_row<DT, U, NCH, true, SAFE, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.combiner, rec.default_row,
                                                 rec.out, ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4,
                                                 RaggedArgs{rec.row_splits, rec.nnz, rec.flags, rec.fill_id}, &lo);
}

}  // namespace

namespace tfra {

void launch_tier_find_combine_many(hipStream_t s, int cls, unsigned grid, const TierManyRec* recs, const unsigned* prefix, unsigned n) {
  with_pool_class(cls / 3, cls % 3, [&](auto DT, auto U, auto NCH) {
    tier_find_combine_many_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(recs, prefix, n);
  });
}
void launch_tier_find_combine_ragged_many(hipStream_t s, int cls, bool safe, unsigned grid, const TierRaggedRec* recs,
                                          const unsigned* prefix, unsigned n) {
  with_ragged_class(cls / 3, cls % 3, safe, [&](auto DT, auto U, auto NCH, auto SAFE) {
    tier_find_combine_ragged_many_kernel<DT, U, NCH, SAFE><<<grid, 256, 0, s>>>(recs, prefix, n);
  });
}

// ---- the tuple form ----------------------------------------------------------------------------------------------------------------
int multi_find_combine_frame(const char* who_c, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                             uint32_t* launches_out, hipStream_t s) {
  const std::string who = who_c;
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  // every descriptor is checked before anything is enqueued: one bad descriptor and no out is written
  // plain: (out float32 | float16 | bfloat16) x (float32 | float16 | bfloat16) x (NCH 1 | 2 | 4), out float32 first: the untyped
  // calls' classes in their order; tiered: (float32 | float16 | bfloat16) x NCH
  constexpr int NUNTYPED = 9, NPLAIN = 27, NCLASS = 36;
  std::vector<PoolDesc> ds(n_tables);
  std::vector<int> cls(n_tables, -1);
  std::vector<size_t> se_off(n_tables, 0);   // a descriptor's bounds in the bounds area, in input order
  size_t n_bnd = 0, total_rows = 0;
  u64 bnd_blocks = 0;
  for (size_t i = 0; i < n_tables; ++i) {
    const PoolDesc& d = ds[i] = at(descs, i);
    auto at_i = [&] { return who + ": descriptor " + std::to_string(i) + ": "; };
    Table* t = nullptr;
    const char* why = nullptr;
    if (int rc = desc_owner(d, &t, &why)) return set_error(rc, at_i() + why);
    if (d.typed)
      if (const Check c = check_rows_out(d.typed); c.code) return report(at_i(), c);
    const Check c = check_find_combine(t, ws, d.nnz, d.ids, d.seg, d.weights, d.combiner, d.n_rows, d.default_row, out_checked(d),
                                       [] { return Check{}; });
    if (c.code) return report(at_i(), c);
    if (!c.active) continue;
    cls[i] = (d.tier ? NPLAIN : out_index(d) * NUNTYPED) + pool_class(t);
    n_bnd += d.nnz ? 1 : 0;
    bnd_blocks += (d.nnz + 255) / 256;
    se_off[i] = 2 * total_rows;
    total_rows += d.n_rows;
  }
  std::vector<size_t> order;
  size_t first[NCLASS + 1];
  if (int rc = order_by_class(who, ds, cls, NCLASS, &order, first)) return rc;
  const size_t n_act = order.size(), n_plain = first[NPLAIN];
  if (n_act == 0) return TFRA_OK;
  if (bnd_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, who + ": too many entries in one call");

  PoolLocks locks;
  int rc = lock_owners(ds, order, s, &locks);
  if (rc) return rc;

  // device memory: [bounds of all rows | blob], the blob = [one-table records | tier records | per-class block prefixes | bounds
  // records | their block prefix]
  const size_t se_bytes = (2 * total_rows * sizeof(int) + 255) / 256 * 256;
  Blob blob;
  const size_t rec_off = blob.add<ManyRec>(n_plain), trec_off = blob.add<TierManyRec>(n_act - n_plain);
  const size_t cpre_off = blob.add<unsigned>(ClassPool::words(n_act, NCLASS, false));
  const size_t brec_off = blob.add<BoundsRec>(n_bnd), bpre_off = blob.add<unsigned>(ClassPool::words(n_bnd, 1, false));
  ManyUpload up;
  rc = many_begin(ws, se_bytes, blob.bytes(), s, &up);
  if (rc) return rc;
  int* se_base = (int*)ws->buf;
  ManyRec* recs = section<ManyRec>(up.host, rec_off);
  TierManyRec* trecs = section<TierManyRec>(up.host, trec_off);
  BoundsRec* brecs = section<BoundsRec>(up.host, brec_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  for (size_t k = 0; k < n_act; ++k) {
    const PoolDesc& d = ds[order[k]];
    Table* t = d.tier ? d.tier->upper : d.table;
    const ManyRec r{t->view_of(t->cur), d.n_rows, (const i64*)d.ids, d.weights, se_base + se_off[order[k]],
                    (const unsigned char*)d.default_row, out_rows(d), t->opts.dim, d.combiner};
    if (d.tier) trecs[k - n_plain] = TierManyRec{r, d.tier->lower->view_of(d.tier->lower->cur)};
    else recs[k] = r;
  }
  // the records stand in class order: a class is a range of them and needs no index
  ClassPool cpool{section<unsigned>(up.host, cpre_off)};
  ManyClass row_cls[NCLASS];
  for (int c = 0; c < NCLASS; ++c)
    row_cls[c] = cpool.put(n_act, false, [&](size_t k) { return k >= first[c] && k < first[c + 1]; },
                           [&](size_t k) { return row_blocks(ds[order[k]]); });
  auto bounded = [&](size_t i) { return cls[i] >= 0 && ds[i].nnz != 0; };
  {
    size_t k = 0;
    for (size_t i = 0; i < n_tables; ++i)
      if (bounded(i)) brecs[k++] = BoundsRec{(const i64*)ds[i].seg, se_base + se_off[i], ds[i].nnz, ds[i].n_rows};
  }
  const ManyClass bnd = ClassPool{section<unsigned>(up.host, bpre_off)}.put(n_tables, false, bounded,
                                                                          [&](size_t i) { return (unsigned)((ds[i].nnz + 255) / 256); });
  rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(se_base, 0, 2 * total_rows * sizeof(int), s));   // empty rows (and every row of an nnz == 0 descriptor): 0, 0
  uint32_t launches = 0;
  if (bnd.n) {   // ONE bounds launch over all descriptors, tiered or not
    rc = comb_bounds_many(s, bnd.grid, section<const BoundsRec>(up.dev, brec_off), section<const unsigned>(up.dev, bpre_off), bnd.n);
    if (rc) return rc;
    ++launches;
  }
  for (int c = 0; c < NCLASS; ++c) {
    const ManyClass& k = row_cls[c];
    if (!k.n) continue;
    const unsigned* p = section<const unsigned>(up.dev, cpre_off) + k.at;
    if (c < NUNTYPED) launch_find_combine_many(s, c, k.grid, section<const ManyRec>(up.dev, rec_off) + first[c], p, k.n);
    else if (c < NPLAIN) launch_find_combine_many_typed(s, c - NUNTYPED, k.grid, section<const ManyRec>(up.dev, rec_off) + first[c], p, k.n);
    else launch_tier_find_combine_many(s, c - NPLAIN, k.grid, section<const TierManyRec>(up.dev, trec_off) + (first[c] - n_plain), p, k.n);
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

// ---- the ragged form ---------------------------------------------------------------------------------------------------------------
int multi_find_combine_ragged_frame(const char* who_c, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                                    uint32_t* launches_out, hipStream_t s) {
  const std::string who = who_c;
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  // every descriptor is checked before anything is enqueued: one bad descriptor and no out is written
  // plain: (out float32 | float16 | bfloat16) x (float32 | float16 | bfloat16) x (NCH 1 | 2 | 4) x (plain | safe), out float32
  // first: the untyped calls' classes in their order; tiered: (float32 | float16 | bfloat16) x NCH x (plain | safe)
  constexpr int NUNTYPED = 18, NPLAIN = 54, NCLASS = 72;
  std::vector<PoolDesc> ds(n_tables);
  std::vector<int> cls(n_tables, -1);
  for (size_t i = 0; i < n_tables; ++i) {
    const PoolDesc& d = ds[i] = at(descs, i);
    auto at_i = [&] { return who + ": descriptor " + std::to_string(i) + ": "; };
    Table* t = nullptr;
    const char* why = nullptr;
    if (int rc = desc_owner(d, &t, &why)) return set_error(rc, at_i() + why);
    if (d.typed)
      if (const Check c = check_rows_out(d.typed); c.code) return report(at_i(), c);
    const Check c = check_find_combine_ragged(t, ws, d.n_rows, d.row_splits, d.nnz, d.ids, d.weights, d.combiner, d.flags, d.reserved,
                                              d.default_row, out_checked(d), [] { return Check{}; });
    if (c.code) return report(at_i(), c);
    if (!c.active) continue;
    cls[i] = (d.tier ? NPLAIN : out_index(d) * NUNTYPED) + pool_class(t) * 2 + (ragged_safe(d.flags, d.weights) ? 1 : 0);
  }
  std::vector<size_t> order;
  size_t first[NCLASS + 1];
  if (int rc = order_by_class(who, ds, cls, NCLASS, &order, first)) return rc;
  const size_t n_act = order.size(), n_plain = first[NPLAIN];
  if (n_act == 0) return TFRA_OK;

  PoolLocks locks;
  int rc = lock_owners(ds, order, s, &locks);
  if (rc) return rc;

  // device memory: the blob alone = [one-table records | tier records | per-class block prefixes]; there are no bounds to keep
  Blob blob;
  const size_t rec_off = blob.add<RaggedRec>(n_plain), trec_off = blob.add<TierRaggedRec>(n_act - n_plain);
  const size_t cpre_off = blob.add<unsigned>(ClassPool::words(n_act, NCLASS, false));
  ManyUpload up;
  rc = many_begin(ws, 0, blob.bytes(), s, &up);
  if (rc) return rc;
  RaggedRec* recs = section<RaggedRec>(up.host, rec_off);
  TierRaggedRec* trecs = section<TierRaggedRec>(up.host, trec_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  for (size_t k = 0; k < n_act; ++k) {
    const PoolDesc& d = ds[order[k]];
    Table* t = d.tier ? d.tier->upper : d.table;
    const RaggedRec r{t->view_of(t->cur), d.n_rows, (const i64*)d.ids, d.weights, (const i64*)d.row_splits,
                      (const unsigned char*)d.default_row, out_rows(d), (i64)d.fill_id, (int)d.nnz, t->opts.dim, d.combiner, d.flags};
    if (d.tier) trecs[k - n_plain] = TierRaggedRec{r, d.tier->lower->view_of(d.tier->lower->cur)};
    else recs[k] = r;
  }
  ClassPool cpool{section<unsigned>(up.host, cpre_off)};
  ManyClass row_cls[NCLASS];
  for (int c = 0; c < NCLASS; ++c)
    row_cls[c] = cpool.put(n_act, false, [&](size_t k) { return k >= first[c] && k < first[c + 1]; },
                           [&](size_t k) { return row_blocks(ds[order[k]]); });
  rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true);
  if (rc) return rc;
  uint32_t launches = 0;
  for (int c = 0; c < NCLASS; ++c) {
    const ManyClass& k = row_cls[c];
    if (!k.n) continue;
    const unsigned* p = section<const unsigned>(up.dev, cpre_off) + k.at;
    if (c < NUNTYPED) launch_find_combine_ragged_many(s, c / 2, c & 1, k.grid, section<const RaggedRec>(up.dev, rec_off) + first[c], p, k.n);
    else if (c < NPLAIN)
      launch_find_combine_ragged_many_typed(s, (c - NUNTYPED) / 2, c & 1, k.grid, section<const RaggedRec>(up.dev, rec_off) + first[c], p, k.n);
    else launch_tier_find_combine_ragged_many(s, (c - NPLAIN) / 2, c & 1, k.grid,
                                              section<const TierRaggedRec>(up.dev, trec_off) + (first[c] - n_plain), p, k.n);
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

}  // namespace tfra

// ---- the entry points ----------------------------------------------------------------------------------------------------------------
static PoolDesc tier_desc_at(const void* descs, size_t i) {
  const tfra_tier_find_combine_desc& d = static_cast<const tfra_tier_find_combine_desc*>(descs)[i];
  return PoolDesc{d.struct_size == sizeof(tfra_tier_find_combine_desc), true, reinterpret_cast<Table*>(d.table), d.tier, d.combiner, d.nnz,
                  d.ids, d.seg, nullptr, d.weights, d.n_rows, 0, 0, 0, d.default_row, d.out};
}
extern "C" int tfra_multi_tier_find_combine(tfra_workspace_t* ws, size_t n_tables, const tfra_tier_find_combine_desc* descs,
                                            uint32_t* launches_out, tfra_stream_t stream) {
  return multi_find_combine_frame("multi_tier_find_combine", ws, n_tables, descs, tier_desc_at, launches_out, (hipStream_t)stream);
}

static PoolDesc tier_ragged_desc_at(const void* descs, size_t i) {
  const tfra_tier_find_combine_ragged_desc& d = static_cast<const tfra_tier_find_combine_ragged_desc*>(descs)[i];
  return PoolDesc{d.struct_size == sizeof(tfra_tier_find_combine_ragged_desc), true, reinterpret_cast<Table*>(d.table), d.tier, d.combiner,
                  d.nnz, d.ids, nullptr, d.row_splits, d.weights, d.n_rows, d.flags, d.reserved, d.fill_id, d.default_row, d.out};
}
extern "C" int tfra_multi_tier_find_combine_ragged(tfra_workspace_t* ws, size_t n_tables, const tfra_tier_find_combine_ragged_desc* descs,
                                                   uint32_t* launches_out, tfra_stream_t stream) {
  return multi_find_combine_ragged_frame("multi_tier_find_combine_ragged", ws, n_tables, descs, tier_ragged_desc_at, launches_out,
                                         (hipStream_t)stream);
}
