// The LONG launch classes of the grouped pooled calls (tfra_multi_find_combine[_ragged]_long and their *_backprop_weights_long forms:
// tfra_pool_long_many.hip): what the twins' frames (tfra_tierpool_many.hip, tfra_wgrad_many.hip) need to serve a list
// member one block per row — the descriptor list of the long ABI, the gradients' records and the launchers of this unit's kernels.
// A long class's grid is the concatenation of its members, member d owning exactly n_rows_d blocks (row_blocks, tfra_pool_many.h):
// no block lies past a member's last row, so every thread of every block reaches every barrier of its row.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_pool_many.h"

namespace tfra {

// What a *_long entry point hands its twin's frame in the place of the descriptor array: the array and the flags beside it
// (NULL: every member is long).  The entry's PoolDescAt reads both: PoolDesc::long_abi, PoolDesc::long_rows.
struct LongDescs {
  const void* descs;
  const uint8_t* long_rows;
  bool flagged(size_t i) const { return !long_rows || long_rows[i] != 0; }
};

// The gradients' records: ManyRec / RaggedRec with grad_out and dw in the place of out (the ragged one carries neither flags nor
// fill_id: PRUNE is the kernel's template axis, FILL changes nothing).
struct LongWgradRec {
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
struct LongWgradRaggedRec {
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

// cls = storage type index * 3 + NCH index (pool_class); recs / prefix in device memory, grid = prefix[n] = the members' rows
TFRA_HIDDEN void launch_find_combine_long_many(hipStream_t s, int cls, unsigned grid, const ManyRec* recs, const unsigned* prefix,
                                               unsigned n);
TFRA_HIDDEN void launch_find_combine_ragged_long_many(hipStream_t s, int cls, bool safe, unsigned grid, const RaggedRec* recs,
                                                      const unsigned* prefix, unsigned n);
TFRA_HIDDEN void launch_wgrad_long_many(hipStream_t s, int cls, unsigned grid, const LongWgradRec* recs, const unsigned* prefix,
                                        unsigned n);
TFRA_HIDDEN void launch_wgrad_ragged_long_many(hipStream_t s, int cls, bool prune, unsigned grid, const LongWgradRaggedRec* recs,
                                               const unsigned* prefix, unsigned n);

}  // namespace tfra
