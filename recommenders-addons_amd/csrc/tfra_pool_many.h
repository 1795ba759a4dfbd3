// What the four grouped pooled lookups share across their two units (tfra_multi_find_combine / _ragged: tfra_pool.hip;
// tfra_multi_tier_find_combine / _ragged: tfra_tierpool_many.hip): the records of their launches, the launchers that
// cross the units (each kernel is instantiated in ONE unit) and the host frame of each form, written once over a descriptor of
// either ABI (PoolDesc) — check every descriptor, classify, lock, lay out, fill, send, launch (tfra_many.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
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
TFRA_HIDDEN void launch_tier_find_combine_many(hipStream_t s, int cls, unsigned grid, const TierManyRec* recs, const unsigned* prefix,
                                               unsigned n);
TFRA_HIDDEN void launch_tier_find_combine_ragged_many(hipStream_t s, int cls, bool safe, unsigned grid, const TierRaggedRec* recs,
                                                      const unsigned* prefix, unsigned n);

// ---- a descriptor of any of the four calls, as the frames read it: exactly one of table / tier for the tier ABI, the table alone
// for the one-table ABI (tier_abi false: `tier` is not looked at and a NULL table is the single call's "null table").
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
  float* out;
};
typedef PoolDesc (*PoolDescAt)(const void* descs, size_t i);

// who: the entry point's message prefix without its colon ("multi_find_combine", "multi_tier_find_combine", ...)
TFRA_HIDDEN int multi_find_combine_frame(const char* who, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                                         uint32_t* launches_out, hipStream_t s);
TFRA_HIDDEN int multi_find_combine_ragged_frame(const char* who, tfra_workspace* ws, size_t n_tables, const void* descs, PoolDescAt at,
                                                uint32_t* launches_out, hipStream_t s);

}  // namespace tfra
