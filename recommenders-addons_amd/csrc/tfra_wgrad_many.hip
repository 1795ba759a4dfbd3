// The grouped weight gradients of the pooled lookups: tfra_multi_find_combine_backprop_weights and
// tfra_multi_find_combine_ragged_backprop_weights, the gradients of a LIST whose members are plain tables
// (tfra_table_find_combine[_ragged]_backprop_weights: tfra_wgrad.hip) or tiers (tfra_tier_find_combine[_ragged]_backprop_weights:
// tfra_tierwgrad.hip), in the enqueues the grouped pooled lookups take (tfra_tierpool_many.hip) plus ONE zero-fill of all dw_out.
// These are reads, as the single calls are: no table is written, no score is touched, nothing moves between tiers, the drivers'
// statistics and staging are left alone.
// The kernels are wgrad_row (tfra_wgrad_device.h), unchanged, in the launch shape of find_combine_many_kernel; the host side is one
// frame per form in the steps of multi_find_combine_frame: check every descriptor, classify, lock, lay out, fill, send, launch.
// The *_typed calls run the same frames over descriptors that carry a tfra_grads: float-or-half is one more axis of
// the launch classes.  A float32 descriptor runs the kernels it always ran; a float16 / bfloat16 one runs wgrad_row's GHALF axis
// in kernels of their own names, its scale's address and format in a record beside the descriptor's (WgradHalf: the float
// records, and with them the float kernels' code, stay as they are).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_pool_many.h"
#include "tfra_tier.h"
#include "tfra_wgrad_device.h"

using namespace tfra;

namespace {

// ---- the records: ManyRec / RaggedRec / Tier*Rec (tfra_pool_many.h) with grad_out and dw in the place of out; the ragged one
// carries neither flags nor fill_id: PRUNE is the kernel's template axis, FILL changes nothing.
struct WgradRec {
  TableView v;
  size_t n_rows;
  const i64* ids;
  const float* w;
  const int* se;
  const unsigned char* default_row;
  const float* grad_out;
  float* dw;
  int dim;
  int combiner;
};
struct WgradRaggedRec {
  TableView v;
  size_t n_rows;
  const i64* ids;
  const float* w;
  const i64* row_splits;
  const unsigned char* default_row;
  const float* grad_out;
  float* dw;
  int nnz;
  int dim;
  int combiner;
};
struct TierWgradRec {
  WgradRec r;
  TableView lo;
};
struct TierWgradRaggedRec {
  WgradRaggedRec r;
  TableView lo;
};
// a half descriptor's scale and format, at the index of its record: wave-uniform, as kernel arguments are
struct WgradHalf {
  const float* d_scale;
  int is_bf16;
  int pad;
};
// the zero-fill of one descriptor's dw_out, which owns ceil(nnz / 256) blocks; tuple form: also its rows' bounds (BoundsRec)
struct ZeroRec {
  const i64* seg;
  int* se;
  float* dw;
  size_t nnz;
  size_t n_rows;
};

// find_combine_many_kernel's launch shape: 256 threads, one 16-lane group per output row, descriptor d owning the blocks
// [prefix[d], prefix[d + 1]).  The record is wave-uniform: scalar loads, as kernel arguments are.
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void wgrad_many_kernel(const WgradRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                         unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRec rec = recs[d];
  wgrad_row<DT, U, NCH, false, false>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, nullptr, 0, rec.combiner, rec.default_row,
                                      rec.grad_out, rec.dw, ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void wgrad_ragged_many_kernel(const WgradRaggedRec* __restrict__ recs,
                                                                const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRaggedRec rec = recs[d];
  wgrad_row<DT, U, NCH, true, PRUNE>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.row_splits, rec.nnz, rec.combiner,
                                     rec.default_row, rec.grad_out, rec.dw,
                                     ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

// Over records that hold both views.  Both are copied out of the record, as the single tier kernels get them as arguments
// (tier_find_combine_many_kernel, tfra_tierpool_many.hip: handing the row function the address of the record's lower view costs
// vector registers).
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void tier_wgrad_many_kernel(const TierWgradRec* __restrict__ recs,
                                                              const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRec rec = recs[d].r;
  const TableView lo = recs[d].lo;
  wgrad_row<DT, U, NCH, false, false, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, nullptr, 0, rec.combiner,
                                            rec.default_row, rec.grad_out, rec.dw,
                                            ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, &lo);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void tier_wgrad_ragged_many_kernel(const TierWgradRaggedRec* __restrict__ recs,
                                                                     const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRaggedRec rec = recs[d].r;
  const TableView lo = recs[d].lo;
  wgrad_row<DT, U, NCH, true, PRUNE, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.row_splits, rec.nnz, rec.combiner,
                                           rec.default_row, rec.grad_out, rec.dw,
                                           ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, &lo);
}

// The four over a float16 / bfloat16 grad_out (wgrad_row's GHALF axis): rec.grad_out is the half matrix's address, hrecs[d] the
// scale's address and the format.
// (how they stay in the twins' register classes: the note at the load site, tfra_wgrad_device.h)
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void wgrad_many_half_kernel(const WgradRec* __restrict__ recs, const WgradHalf* __restrict__ hrecs,
                                                              const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRec rec = recs[d];
  const WgradHalf h = hrecs[d];
  wgrad_row<DT, U, NCH, false, false, false, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, nullptr, 0, rec.combiner,
                                                   rec.default_row, rec.grad_out, rec.dw,
                                                   ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, nullptr, h.d_scale,
                                                   h.is_bf16);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void wgrad_ragged_many_half_kernel(const WgradRaggedRec* __restrict__ recs,
                                                                     const WgradHalf* __restrict__ hrecs,
                                                                     const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRaggedRec rec = recs[d];
  const WgradHalf h = hrecs[d];
  wgrad_row<DT, U, NCH, true, PRUNE, false, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.row_splits, rec.nnz,
                                                  rec.combiner, rec.default_row, rec.grad_out, rec.dw,
                                                  ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, nullptr, h.d_scale,
                                                  h.is_bf16);
}

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void tier_wgrad_many_half_kernel(const TierWgradRec* __restrict__ recs,
                                                                   const WgradHalf* __restrict__ hrecs,
                                                                   const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRec rec = recs[d].r;
  const TableView lo = recs[d].lo;
  const WgradHalf h = hrecs[d];
  wgrad_row<DT, U, NCH, false, false, true, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, nullptr, 0, rec.combiner,
                                                  rec.default_row, rec.grad_out, rec.dw,
                                                  ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, &lo, h.d_scale, h.is_bf16);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void tier_wgrad_ragged_many_half_kernel(const TierWgradRaggedRec* __restrict__ recs,
                                                                          const WgradHalf* __restrict__ hrecs,
                                                                          const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const WgradRaggedRec rec = recs[d].r;
  const TableView lo = recs[d].lo;
  const WgradHalf h = hrecs[d];
  wgrad_row<DT, U, NCH, true, PRUNE, true, true>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.row_splits, rec.nnz,
                                                 rec.combiner, rec.default_row, rec.grad_out, rec.dw,
                                                 ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4, &lo, h.d_scale, h.is_bf16);
}

// The zero-fill of all dw_out in one launch: the 0 of an entry in no row, or outside the clamped cover (the single calls' memset
// of dw_out).  BOUNDS (tuple form): a copy of seg64_bounds_many_kernel (tfra_pool.hip) that stores the entry's 0 before it looks
// at seg, so that the rows' bounds and the zeros are one launch; se zeroed before (empty rows: 0, 0).  A descriptor without rows
// (n_rows == 0) is zero-filled and writes no bound: every seg lies outside [0, 0).
template <bool BOUNDS>
__global__ __launch_bounds__(256) void wgrad_zero_many_kernel(const ZeroRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                              unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const ZeroRec rec = recs[d];
  const size_t p = (size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x;
  if (p >= rec.nnz) return;
  rec.dw[p] = 0.f;
  if constexpr (BOUNDS) {
    const i64 s = rec.seg[p];
    if (s < 0 || (size_t)s >= rec.n_rows) return;
    if (p == 0 || rec.seg[p - 1] != s) rec.se[s] = (int)p;
    if (p == rec.nnz - 1 || rec.seg[p + 1] != s) rec.se[rec.n_rows + s] = (int)p + 1;
  }
}

// ---- what the two frames share ---------------------------------------------------------------------------------------------------
const char* const HINT_TABLE = " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
const char* const HINT_TIER = " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine_backprop_weights otherwise)";

// The checks of the single call behind `c`, the forward's checks with grad_out in the place of out: its NEEDS_DIM hint, then
// dw_out.  TFRA_OK, or the code with the message recorded behind `at` ("<who>: descriptor <i>: ").
int check_wgrad_desc(const std::string& at, const PoolDesc& d, Check c) {
  if (c.msg == NEEDS_DIM) c.msg += d.tier ? HINT_TIER : HINT_TABLE;
  if (c.code) return report(at + "(out = grad_out) ", c);
  if (Check w = check_dw_out(d.nnz, d.dw_out); w.code) return report(at, w);
  return TFRA_OK;
}
unsigned zero_blocks(const PoolDesc& d) { return (unsigned)((d.nnz + 255) / 256); }

// A typed descriptor's record (tfra_grads): checked as the single typed call checks it, BEFORE any descriptor's table or tier is
// looked at.  TFRA_OK, or the code with the message recorded behind `at`.
int check_desc_grads(const std::string& at, const PoolDesc& d) {
  if (!d.hgrads || !d.size_ok) return TFRA_OK;   // (a wrong size is desc_owner's to refuse: the record cannot be trusted then)
  bool forward;
  if (const Check c = check_typed(d.hgrads, &forward); c.code) return report(at, c);
  return TFRA_OK;
}
// whether a descriptor's grad_out is float16 / bfloat16, what the twin's checks look at in the place of grad_out, and what the
// kernel is handed (the half kernels read the matrix through the same field)
bool desc_half(const PoolDesc& d) { return d.hgrads && d.hgrads->dtype != TFRA_F32; }
const float* grad_checked(const PoolDesc& d) {
  return desc_half(d) ? grads_for_twin(*d.hgrads) : d.hgrads ? (const float*)d.hgrads->grads : d.grad_out;
}
const float* grad_rows(const PoolDesc& d) { return d.hgrads ? (const float*)d.hgrads->grads : d.grad_out; }
WgradHalf half_rec(const PoolDesc& d) {
  return desc_half(d) ? WgradHalf{d.hgrads->d_scale, d.hgrads->dtype == TFRA_BF16, 0} : WgradHalf{nullptr, 0, 0};
}

// ---- the tuple form ----------------------------------------------------------------------------------------------------------------
int multi_wgrad_frame(const std::string& who, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                      uint32_t* launches_out, hipStream_t s) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  // every descriptor is checked before anything is enqueued: one bad descriptor and no dw_out is written
  // (plain | tiered) x (float | half grad_out) x (float32 | float16 | bfloat16 rows) x (NCH 1 | 2 | 4)
  constexpr int NBASE = 9, NPLAIN = 2 * NBASE, NCLASS = 2 * NPLAIN;
  bool any_half = false;
  std::vector<PoolDesc> ds(n_tables);
  std::vector<int> cls(n_tables, -1);
  std::vector<size_t> se_off(n_tables, 0);   // a descriptor's bounds in the bounds area, in input order
  std::vector<size_t> zeroed;                // the descriptors with nnz > 0: their dw_out is written, with rows or without
  size_t total_rows = 0;
  u64 z_blocks = 0;
  // (typed lists) every record first: no table or tier handle is looked at before all of them have passed
  for (size_t i = 0; i < n_tables; ++i)
    if (int rc = check_desc_grads(who + ": descriptor " + std::to_string(i) + ": ", at(descs, i))) return rc;
  for (size_t i = 0; i < n_tables; ++i) {
    const PoolDesc& d = ds[i] = at(descs, i);
    const std::string at_i = who + ": descriptor " + std::to_string(i) + ": ";
    Table* t = nullptr;
    const char* why = nullptr;
    if (int rc = desc_owner(d, &t, &why)) return set_error(rc, at_i + why);
    const Check c = check_find_combine(t, ws, d.nnz, d.ids, d.seg, d.weights, d.combiner, d.n_rows, d.default_row, grad_checked(d),
                                       [] { return Check{}; });
    if (int rc = check_wgrad_desc(at_i, d, c)) return rc;
    if (d.nnz == 0) continue;   // nothing to write
    zeroed.push_back(i);
    z_blocks += zero_blocks(d);
    if (!c.active) continue;    // no rows: zeros alone
    cls[i] = (d.tier ? NPLAIN : 0) + (desc_half(d) ? NBASE : 0) + pool_class(t);
    any_half = any_half || desc_half(d);
    se_off[i] = 2 * total_rows;
    total_rows += d.n_rows;
  }
  if (zeroed.empty()) return TFRA_OK;
  std::vector<size_t> order;
  size_t first[NCLASS + 1];
  if (int rc = order_by_class(who, ds, cls, NCLASS, &order, first)) return rc;
  const size_t n_act = order.size(), n_plain = first[NPLAIN], n_zero = zeroed.size();
  if (z_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, who + ": too many entries in one call");

  PoolLocks locks;   // of every descriptor that is written, as the single call enters its table before its memset
  int rc = lock_owners(ds, zeroed, s, &locks);
  if (rc) return rc;

  // device memory: [bounds of all rows | blob], the blob = [one-table records | tier records | per-class block prefixes | zero-fill
  // records | their block prefix]
  const size_t se_bytes = (2 * total_rows * sizeof(int) + 255) / 256 * 256;
  Blob blob;
  const size_t rec_off = blob.add<WgradRec>(n_plain), trec_off = blob.add<TierWgradRec>(n_act - n_plain);
  const size_t hrec_off = blob.add<WgradHalf>(any_half ? n_act : 0);   // at the records' positions k, plain and tier alike
  const size_t cpre_off = blob.add<unsigned>(ClassPool::words(n_act, NCLASS, false));
  const size_t zrec_off = blob.add<ZeroRec>(n_zero), zpre_off = blob.add<unsigned>(ClassPool::words(n_zero, 1, false));
  ManyUpload up;
  rc = many_begin(ws, se_bytes, blob.bytes(), s, &up);
  if (rc) return rc;
  int* se_base = (int*)ws->buf;
  WgradRec* recs = section<WgradRec>(up.host, rec_off);
  TierWgradRec* trecs = section<TierWgradRec>(up.host, trec_off);
  ZeroRec* zrecs = section<ZeroRec>(up.host, zrec_off);
  WgradHalf* hrecs = section<WgradHalf>(up.host, hrec_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  for (size_t k = 0; k < n_act; ++k) {
    const PoolDesc& d = ds[order[k]];
    Table* t = d.tier ? d.tier->upper : d.table;
    const WgradRec r{t->view_of(t->cur), d.n_rows, (const i64*)d.ids, d.weights, se_base + se_off[order[k]],
                     (const unsigned char*)d.default_row, grad_rows(d), d.dw_out, t->opts.dim, d.combiner};
    if (d.tier) trecs[k - n_plain] = TierWgradRec{r, d.tier->lower->view_of(d.tier->lower->cur)};
    else recs[k] = r;
    if (any_half) hrecs[k] = half_rec(d);
  }
  // the records stand in class order: a class is a range of them and needs no index
  ClassPool cpool{section<unsigned>(up.host, cpre_off)};
  ManyClass row_cls[NCLASS];
  for (int c = 0; c < NCLASS; ++c)
    row_cls[c] = cpool.put(n_act, false, [&](size_t k) { return k >= first[c] && k < first[c + 1]; },
                           [&](size_t k) { return row_blocks(ds[order[k]]); });
  for (size_t k = 0; k < n_zero; ++k) {
    const PoolDesc& d = ds[zeroed[k]];
    zrecs[k] = ZeroRec{(const i64*)d.seg, se_base + se_off[zeroed[k]], d.dw_out, d.nnz, d.n_rows};
  }
  const ManyClass zero = ClassPool{section<unsigned>(up.host, zpre_off)}.put(n_zero, false, [](size_t) { return true; },
                                                                           [&](size_t k) { return zero_blocks(ds[zeroed[k]]); });
  rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true);
  if (rc) return rc;
  if (total_rows) HIP_TRY(hipMemsetAsync(se_base, 0, 2 * total_rows * sizeof(int), s));   // empty rows: 0, 0
  // ONE launch: every dw_out zeroed and all rows' bounds
  wgrad_zero_many_kernel<true><<<zero.grid, 256, 0, s>>>(section<const ZeroRec>(up.dev, zrec_off),
                                                         section<const unsigned>(up.dev, zpre_off), zero.n);
  uint32_t launches = 1;
  for (int c = 0; c < NCLASS; ++c) {
    const ManyClass& k = row_cls[c];
    if (!k.n) continue;
    const unsigned* p = section<const unsigned>(up.dev, cpre_off) + k.at;
    const bool half = (c % NPLAIN) >= NBASE;
    // a half class's scales and formats stand at its records' positions (any_half holds then)
    const WgradHalf* hr = half ? section<const WgradHalf>(up.dev, hrec_off) + first[c] : nullptr;
    with_pool_class((c % NBASE) / 3, c % 3, [&](auto DT, auto U, auto NCH) {
      if (c < NPLAIN) {
        const WgradRec* pr = section<const WgradRec>(up.dev, rec_off) + first[c];
        if (half) wgrad_many_half_kernel<DT, U, NCH><<<k.grid, 256, 0, s>>>(pr, hr, p, k.n);
        else wgrad_many_kernel<DT, U, NCH><<<k.grid, 256, 0, s>>>(pr, p, k.n);
      } else {
        const TierWgradRec* tr = section<const TierWgradRec>(up.dev, trec_off) + (first[c] - n_plain);
        if (half) tier_wgrad_many_half_kernel<DT, U, NCH><<<k.grid, 256, 0, s>>>(tr, hr, p, k.n);
        else tier_wgrad_many_kernel<DT, U, NCH><<<k.grid, 256, 0, s>>>(tr, p, k.n);
      }
    });
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

// ---- the ragged form ---------------------------------------------------------------------------------------------------------------
int multi_wgrad_ragged_frame(const std::string& who, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                             uint32_t* launches_out, hipStream_t s) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  // every descriptor is checked before anything is enqueued: one bad descriptor and no dw_out is written
  // (plain | tiered) x (float | half grad_out) x (float32 | float16 | bfloat16 rows) x (NCH 1 | 2 | 4) x (plain | pruning)
  constexpr int NBASE = 18, NPLAIN = 2 * NBASE, NCLASS = 2 * NPLAIN;
  bool any_half = false;
  std::vector<PoolDesc> ds(n_tables);
  std::vector<int> cls(n_tables, -1);
  std::vector<size_t> zeroed;   // the descriptors with nnz > 0: their dw_out is written, with rows or without
  u64 z_blocks = 0;
  // (typed lists) every record first: no table or tier handle is looked at before all of them have passed
  for (size_t i = 0; i < n_tables; ++i)
    if (int rc = check_desc_grads(who + ": descriptor " + std::to_string(i) + ": ", at(descs, i))) return rc;
  for (size_t i = 0; i < n_tables; ++i) {
    const PoolDesc& d = ds[i] = at(descs, i);
    const std::string at_i = who + ": descriptor " + std::to_string(i) + ": ";
    Table* t = nullptr;
    const char* why = nullptr;
    if (int rc = desc_owner(d, &t, &why)) return set_error(rc, at_i + why);
    const Check c = check_find_combine_ragged(t, ws, d.n_rows, d.row_splits, d.nnz, d.ids, d.weights, d.combiner, d.flags, d.reserved,
                                              d.default_row, grad_checked(d), [] { return Check{}; });
    if (int rc = check_wgrad_desc(at_i, d, c)) return rc;
    if (d.nnz == 0) continue;   // nothing to write
    zeroed.push_back(i);
    z_blocks += zero_blocks(d);
    if (!c.active) continue;    // no rows: zeros alone
    // the fourth axis is PRUNE, as in the single calls: FILL changes nothing, and PRUNE without weights neither
    cls[i] = (d.tier ? NPLAIN : 0) + (desc_half(d) ? NBASE : 0) + pool_class(t) * 2 + (((d.flags & TFRA_RAGGED_PRUNE) && d.weights) ? 1 : 0);
    any_half = any_half || desc_half(d);
  }
  if (zeroed.empty()) return TFRA_OK;
  std::vector<size_t> order;
  size_t first[NCLASS + 1];
  if (int rc = order_by_class(who, ds, cls, NCLASS, &order, first)) return rc;
  const size_t n_act = order.size(), n_plain = first[NPLAIN], n_zero = zeroed.size();
  if (z_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, who + ": too many entries in one call");

  PoolLocks locks;   // of every descriptor that is written, as the single call enters its table before its memset
  int rc = lock_owners(ds, zeroed, s, &locks);
  if (rc) return rc;

  // device memory: the blob alone = [one-table records | tier records | per-class block prefixes | zero-fill records | their block
  // prefix]; there are no bounds to keep
  Blob blob;
  const size_t rec_off = blob.add<WgradRaggedRec>(n_plain), trec_off = blob.add<TierWgradRaggedRec>(n_act - n_plain);
  const size_t hrec_off = blob.add<WgradHalf>(any_half ? n_act : 0);   // at the records' positions k, plain and tier alike
  const size_t cpre_off = blob.add<unsigned>(ClassPool::words(n_act, NCLASS, false));
  const size_t zrec_off = blob.add<ZeroRec>(n_zero), zpre_off = blob.add<unsigned>(ClassPool::words(n_zero, 1, false));
  ManyUpload up;
  rc = many_begin(ws, 0, blob.bytes(), s, &up);
  if (rc) return rc;
  WgradRaggedRec* recs = section<WgradRaggedRec>(up.host, rec_off);
  TierWgradRaggedRec* trecs = section<TierWgradRaggedRec>(up.host, trec_off);
  ZeroRec* zrecs = section<ZeroRec>(up.host, zrec_off);
  WgradHalf* hrecs = section<WgradHalf>(up.host, hrec_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  for (size_t k = 0; k < n_act; ++k) {
    const PoolDesc& d = ds[order[k]];
    Table* t = d.tier ? d.tier->upper : d.table;
    const WgradRaggedRec r{t->view_of(t->cur), d.n_rows, (const i64*)d.ids, d.weights, (const i64*)d.row_splits,
                           (const unsigned char*)d.default_row, grad_rows(d), d.dw_out, (int)d.nnz, t->opts.dim, d.combiner};
    if (d.tier) trecs[k - n_plain] = TierWgradRaggedRec{r, d.tier->lower->view_of(d.tier->lower->cur)};
    else recs[k] = r;
    if (any_half) hrecs[k] = half_rec(d);
  }
  ClassPool cpool{section<unsigned>(up.host, cpre_off)};
  ManyClass row_cls[NCLASS];
  for (int c = 0; c < NCLASS; ++c)
    row_cls[c] = cpool.put(n_act, false, [&](size_t k) { return k >= first[c] && k < first[c + 1]; },
                           [&](size_t k) { return row_blocks(ds[order[k]]); });
  for (size_t k = 0; k < n_zero; ++k) zrecs[k] = ZeroRec{nullptr, nullptr, ds[zeroed[k]].dw_out, ds[zeroed[k]].nnz, 0};
  const ManyClass zero = ClassPool{section<unsigned>(up.host, zpre_off)}.put(n_zero, false, [](size_t) { return true; },
                                                                           [&](size_t k) { return zero_blocks(ds[zeroed[k]]); });
  rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true);
  if (rc) return rc;
  // ONE launch: every dw_out zeroed (entries outside the clamped cover: 0)
  wgrad_zero_many_kernel<false><<<zero.grid, 256, 0, s>>>(section<const ZeroRec>(up.dev, zrec_off),
                                                          section<const unsigned>(up.dev, zpre_off), zero.n);
  uint32_t launches = 1;
  for (int c = 0; c < NCLASS; ++c) {
    const ManyClass& k = row_cls[c];
    if (!k.n) continue;
    const unsigned* p = section<const unsigned>(up.dev, cpre_off) + k.at;
    const int pc = (c % NBASE) / 2;
    const bool half = (c % NPLAIN) >= NBASE;
    const WgradHalf* hr = half ? section<const WgradHalf>(up.dev, hrec_off) + first[c] : nullptr;
    with_ragged_class(pc / 3, pc % 3, c & 1, [&](auto DT, auto U, auto NCH, auto PRUNE) {
      if (c < NPLAIN) {
        const WgradRaggedRec* pr = section<const WgradRaggedRec>(up.dev, rec_off) + first[c];
        if (half) wgrad_ragged_many_half_kernel<DT, U, NCH, PRUNE><<<k.grid, 256, 0, s>>>(pr, hr, p, k.n);
        else wgrad_ragged_many_kernel<DT, U, NCH, PRUNE><<<k.grid, 256, 0, s>>>(pr, p, k.n);
      } else {
        const TierWgradRaggedRec* tr = section<const TierWgradRaggedRec>(up.dev, trec_off) + (first[c] - n_plain);
        if (half) tier_wgrad_ragged_many_half_kernel<DT, U, NCH, PRUNE><<<k.grid, 256, 0, s>>>(tr, hr, p, k.n);
        else tier_wgrad_ragged_many_kernel<DT, U, NCH, PRUNE><<<k.grid, 256, 0, s>>>(tr, p, k.n);
      }
    });
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

PoolDesc wgrad_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_wgrad_desc& d = static_cast<const tfra_find_combine_wgrad_desc*>(descs)[i];
  return PoolDesc{d.struct_size == sizeof(tfra_find_combine_wgrad_desc), true, reinterpret_cast<Table*>(d.table), d.tier, d.combiner, d.nnz,
                  d.ids, d.seg, nullptr, d.weights, d.n_rows, 0, 0, 0, d.default_row, nullptr, d.grad_out, d.dw_out};
}
PoolDesc wgrad_ragged_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_ragged_wgrad_desc& d = static_cast<const tfra_find_combine_ragged_wgrad_desc*>(descs)[i];
  return PoolDesc{d.struct_size == sizeof(tfra_find_combine_ragged_wgrad_desc), true, reinterpret_cast<Table*>(d.table), d.tier, d.combiner,
                  d.nnz, d.ids, nullptr, d.row_splits, d.weights, d.n_rows, d.flags, d.reserved, d.fill_id, d.default_row, nullptr,
                  d.grad_out, d.dw_out};
}

// the typed descriptors: the twins' fields, with the tfra_grads record in the float pointer's place
PoolDesc wgrad_typed_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_wgrad_typed_desc& d = static_cast<const tfra_find_combine_wgrad_typed_desc*>(descs)[i];
  PoolDesc p{d.struct_size == sizeof(tfra_find_combine_wgrad_typed_desc), true, reinterpret_cast<Table*>(d.table), d.tier, d.combiner, d.nnz,
             d.ids, d.seg, nullptr, d.weights, d.n_rows, 0, 0, 0, d.default_row, nullptr, nullptr, d.dw_out};
  p.hgrads = &d.grad_out;
  return p;
}
PoolDesc wgrad_ragged_typed_desc_at(const void* descs, size_t i) {
  const tfra_find_combine_ragged_wgrad_typed_desc& d = static_cast<const tfra_find_combine_ragged_wgrad_typed_desc*>(descs)[i];
  PoolDesc p{d.struct_size == sizeof(tfra_find_combine_ragged_wgrad_typed_desc), true, reinterpret_cast<Table*>(d.table), d.tier,
             d.combiner, d.nnz, d.ids, nullptr, d.row_splits, d.weights, d.n_rows, d.flags, d.reserved, d.fill_id, d.default_row, nullptr,
             nullptr, d.dw_out};
  p.hgrads = &d.grad_out;
  return p;
}

}  // namespace

// ---- the entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int tfra_multi_find_combine_backprop_weights(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_wgrad_desc* descs,
                                                        uint32_t* launches_out, tfra_stream_t stream) {
  return multi_wgrad_frame("multi_find_combine_backprop_weights", ws, n_tables, descs, wgrad_desc_at, launches_out, (hipStream_t)stream);
}

extern "C" int tfra_multi_find_combine_ragged_backprop_weights(tfra_workspace_t* ws, size_t n_tables,
                                                               const tfra_find_combine_ragged_wgrad_desc* descs,
                                                               uint32_t* launches_out, tfra_stream_t stream) {
  return multi_wgrad_ragged_frame("multi_find_combine_ragged_backprop_weights", ws, n_tables, descs, wgrad_ragged_desc_at, launches_out,
                                  (hipStream_t)stream);
}

extern "C" int tfra_multi_find_combine_backprop_weights_typed(tfra_workspace_t* ws, size_t n_tables,
                                                              const tfra_find_combine_wgrad_typed_desc* descs, uint32_t* launches_out,
                                                              tfra_stream_t stream) {
  return multi_wgrad_frame("multi_find_combine_backprop_weights_typed", ws, n_tables, descs, wgrad_typed_desc_at, launches_out,
                           (hipStream_t)stream);
}

extern "C" int tfra_multi_find_combine_ragged_backprop_weights_typed(tfra_workspace_t* ws, size_t n_tables,
                                                                     const tfra_find_combine_ragged_wgrad_typed_desc* descs,
                                                                     uint32_t* launches_out, tfra_stream_t stream) {
  return multi_wgrad_ragged_frame("multi_find_combine_ragged_backprop_weights_typed", ws, n_tables, descs, wgrad_ragged_typed_desc_at,
                                  launches_out, (hipStream_t)stream);
}
