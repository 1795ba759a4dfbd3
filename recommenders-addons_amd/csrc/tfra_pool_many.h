// What the four grouped pooled lookups share across their two units (tfra_multi_find_combine / _ragged: tfra_pool.hip;
// tfra_multi_tier_find_combine / _ragged: tfra_tierpool_many.hip): the records of their launches, the launchers that
// cross the units (each kernel is instantiated in ONE unit) and the host frame of each form, written once over a descriptor of
// either ABI (PoolDesc) — check every descriptor, classify, lock, lay out, fill, send, launch (tfra_many.h).
// The grouped weight gradients (tfra_multi_find_combine[_ragged]_backprop_weights: tfra_wgrad_many.hip) read the same
// descriptor and take the same steps: what a frame needs for them — a descriptor's owner, its class, the records' order, the
// locks — is at the end of this file, ONE copy for the three units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_tier.h"

namespace tfra {

// ---- the records: what a single-table launch takes as kernel arguments (26 tables' do not fit the 4 KB of kernel arguments: a
// TableView alone is 80 B).  The grid is the concatenation of the class's descriptors, descriptor d owning the blocks
// [prefix[d], prefix[d + 1]) = ceil(n_rows * 16 / 256) blocks, so that a block never straddles two descriptors.
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
// a tier's descriptor: the one-table record over the cache (r.v = the upper table's view) and the lower table's view behind it
struct TierManyRec {
  ManyRec r;
  TableView lo;
};
struct TierRaggedRec {
  RaggedRec r;
  TableView lo;
};

// ---- the launchers (hidden: shared by the library's units, none of its dynamic symbols).  cls = storage type index * 3 + NCH
// index (tfra_pool.h: st_index, nch_index); recs / prefix in device memory, grid = prefix[n].
#define TFRA_HIDDEN __attribute__((visibility("hidden")))
TFRA_HIDDEN void launch_find_combine_many(hipStream_t s, int cls, unsigned grid, const ManyRec* recs, const unsigned* prefix, unsigned n);
TFRA_HIDDEN void launch_find_combine_ragged_many(hipStream_t s, int cls, bool safe, unsigned grid, const RaggedRec* recs,
                                                 const unsigned* prefix, unsigned n);
// the typed lookups' kernels (tfra_pool_typed.hip): cls = (output type index - 1) * 9 + the class above — float16, then bfloat16 rows
TFRA_HIDDEN void launch_find_combine_many_typed(hipStream_t s, int cls, unsigned grid, const ManyRec* recs, const unsigned* prefix,
                                                unsigned n);
TFRA_HIDDEN void launch_find_combine_ragged_many_typed(hipStream_t s, int cls, bool safe, unsigned grid, const RaggedRec* recs,
                                                       const unsigned* prefix, unsigned n);
TFRA_HIDDEN void launch_tier_find_combine_many(hipStream_t s, int cls, unsigned grid, const TierManyRec* recs, const unsigned* prefix,
                                               unsigned n);
TFRA_HIDDEN void launch_tier_find_combine_ragged_many(hipStream_t s, int cls, bool safe, unsigned grid, const TierRaggedRec* recs,
                                                      const unsigned* prefix, unsigned n);

// ---- a descriptor of any of the grouped pooled calls, as the frames read it: exactly one of table / tier for the tier ABI (the
// weight gradients' too), the table alone for the one-table ABI (tier_abi false: `tier` is not looked at and a NULL table is the
// single call's "null table").
struct PoolDesc {
  bool size_ok;              // struct_size is the ABI's
  bool tier_abi;
  Table* table;
  tfra_tier* tier;
  int combiner;
  size_t nnz;
  const void* ids;
  const void* seg;           // tuple form
  const void* row_splits;    // ragged form
  const float* weights;
  size_t n_rows;
  uint32_t flags, reserved;  // ragged form
  int64_t fill_id;           // ragged form
  const void* default_row;
  float* out;                // the lookups
  const float* grad_out;     // the weight gradients: grad_out in the place of out, and dw_out
  float* dw_out;
  const tfra_rows_out* typed;   // the typed lookups (plain tables only): the output record in the place of out; NULL otherwise
  const tfra_grads* hgrads;     // the typed weight gradients: the record in the place of grad_out; NULL otherwise
};
typedef PoolDesc (*PoolDescAt)(const void* descs, size_t i);

// who: the entry point's message prefix without its colon ("multi_find_combine", "multi_tier_find_combine", ...)
TFRA_HIDDEN int multi_find_combine_frame(const char* who, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                                         uint32_t* launches_out, hipStream_t s);
TFRA_HIDDEN int multi_find_combine_ragged_frame(const char* who, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                                                uint32_t* launches_out, hipStream_t s);

namespace {

// ---- what the frames share (host code, hidden: an anonymous namespace, as tfra_pool.h's checks) ------------------------------------
// The table a descriptor's checks run on: its table, or its tier's upper table (tfra_tier_create has made sure that both tables of a
// tier have its value dtype, dim and device).  What only a descriptor can get wrong is refused here, before the operation's checks.
int desc_owner(const PoolDesc& d, Table** t, const char** why) {
  if (!d.size_ok) { *why = "descriptor size mismatch"; return TFRA_ERR_INVALID; }
  if (d.tier_abi && (d.table != nullptr) == (d.tier != nullptr)) {
    *why = "exactly one of table / tier must be set";
    return TFRA_ERR_INVALID;
  }
  *t = d.tier ? d.tier->upper : d.table;
  return TFRA_OK;
}
int pool_class(const Table* t) { return st_index(t->opts.value_dtype) * 3 + nch_index(t->opts.dim); }
// A typed descriptor's output: its type is one more class axis of the plain classes — index 0, float32, runs the
// untyped kernels — and its rows stand in the record where out stands (the kernels of a half class address 2-byte elements).
int out_index(const PoolDesc& d) { return d.typed ? st_index(d.typed->dtype) : 0; }
const float* out_checked(const PoolDesc& d) { return d.typed ? out_for_twin(*d.typed) : d.out; }   // what the twin's checks look at
float* out_rows(const PoolDesc& d) { return d.typed ? static_cast<float*>(d.typed->rows) : d.out; }
unsigned row_blocks(const PoolDesc& d) { return (unsigned)((d.n_rows * 16 + 255) / 256); }

// The records' order: class by class, input order inside a class; first[c] is where class c starts, first[n_class] the number of
// active descriptors.  The classes of plain tables come first: they are the one-table call's, in its order.
int order_by_class(const std::string& who, const std::vector<PoolDesc>& ds, const std::vector<int>& cls, int n_class,
                   std::vector<size_t>* order, size_t* first) {
  for (int c = 0; c < n_class; ++c) {
    first[c] = order->size();
    u64 blocks = 0;
    for (size_t i = 0; i < ds.size(); ++i)
      if (cls[i] == c) { order->push_back(i); blocks += row_blocks(ds[i]); }
    if (blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, who + ": too many rows in one call");
  }
  first[n_class] = order->size();
  return TFRA_OK;
}

// The locks of a call (TierLocks, lock_tiers_and_tables: tfra_tier.h, shared with the grouped admission): each distinct tier's own
// mutex, then every table of the call (plain ones, uppers and lowers: a table may be named directly in one descriptor and stand in
// a tier of another) once.
typedef TierLocks PoolLocks;
int lock_owners(const std::vector<PoolDesc>& ds, const std::vector<size_t>& order, hipStream_t s, PoolLocks* l) {
  std::vector<tfra_tier*> tiers;
  std::vector<Table*> tabs;
  tabs.reserve(2 * order.size());
  for (size_t i : order) {
    const PoolDesc& d = ds[i];
    if (d.tier) {
      tiers.push_back(d.tier);
      tabs.push_back(d.tier->upper);
      tabs.push_back(d.tier->lower);
    } else {
      tabs.push_back(d.table);
    }
  }
  return lock_tiers_and_tables(std::move(tiers), std::move(tabs), s, l);
}

}  // namespace

}  // namespace tfra
