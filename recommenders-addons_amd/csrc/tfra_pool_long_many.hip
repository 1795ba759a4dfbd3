// The grouped pooled calls with LONG members: tfra_multi_find_combine_long, tfra_multi_find_combine_ragged_long and
// the kernels of their *_backprop_weights_long forms (whose entry points stand with their frames, tfra_wgrad_many.hip).
// A model with sequence features is a many-table model: some twenty categorical features of 1 - 30 ids a row and a handful of
// histories of a few hundred.  The grouped calls (tfra_pool.hip, tfra_wgrad_many.hip) walk every member's rows by one 16-lane group
// each, which costs the histories the 3.5x - 5x that the single *_long calls (tfra_pool_long.hip) gain; taking the histories out of
// the list brings back the per-table enqueues.  Here "long or not" is one more launch-class axis of the twins' frames, chosen per
// member by a flag byte: a flagged member's rows run ONE 256-thread block each, an unflagged member runs the twins' kernels in the
// twins' classes, untouched.
// The launch shape: a long class's grid is the concatenation of its members, member d owning the blocks [prefix[d], prefix[d + 1])
// = exactly n_rows_d of them (not ceil(16 n_rows / 256)).  A block finds its member by many_desc_of over the class's prefix and
// reads the member's record ONCE: block index, search, record address and record are uniform in the block, so the record stays in
// scalar registers as kernel arguments do.  Then it runs find_combine_long_row / wgrad_long_row (tfra_pool_long_device.h) as they
// stand — one device body, two callers — so a member's result is the single *_long call's bit for bit, and with it the 16-lane
// twin's.  The windows, the two 16 KiB slabs, the gradient's park of d_p / w_p and its overflow past LONG_PARK entries, and the
// barrier discipline are those bodies': no block exists past a member's last row, so none can leave a row's barriers early.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"
#include "tfra_pool_long_device.h"
#include "tfra_pool_long_many.h"
#include "tfra_pool_many.h"

using namespace tfra;

namespace {

template <int DT, int NCH>
__global__ __launch_bounds__(LONG_THREADS) void find_combine_long_many_kernel(const ManyRec* __restrict__ recs,
                                                                              const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const ManyRec rec = recs[d];
  find_combine_long_row<DT, NCH, false, false>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, rec.combiner, rec.default_row,
                                               rec.out, (size_t)(blockIdx.x - prefix[d]), RaggedArgs{});
}

template <int DT, int NCH, bool SAFE>
__global__ __launch_bounds__(LONG_THREADS) void find_combine_ragged_long_many_kernel(const RaggedRec* __restrict__ recs,
                                                                                     const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const RaggedRec rec = recs[d];
  find_combine_long_row<DT, NCH, true, SAFE>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.combiner, rec.default_row, rec.out,
                                             (size_t)(blockIdx.x - prefix[d]),
                                             RaggedArgs{rec.row_splits, rec.nnz, rec.flags, rec.fill_id});
}

// The gradients: every dw_out has been zeroed (tuple form: and every row's bounds written) by the frame's ONE preparatory launch.
template <int DT, int NCH>
__global__ __launch_bounds__(LONG_THREADS) void wgrad_long_many_kernel(const LongWgradRec* __restrict__ recs,
                                                                       const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const LongWgradRec rec = recs[d];
  wgrad_long_row<DT, NCH, false, false>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, rec.combiner, rec.default_row, rec.grad_out,
                                        rec.dw, (size_t)(blockIdx.x - prefix[d]), RaggedArgs{});
}

template <int DT, int NCH, bool PRUNE>
__global__ __launch_bounds__(LONG_THREADS) void wgrad_ragged_long_many_kernel(const LongWgradRaggedRec* __restrict__ recs,
                                                                              const unsigned* __restrict__ prefix, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const LongWgradRaggedRec rec = recs[d];
  wgrad_long_row<DT, NCH, true, PRUNE>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, nullptr, rec.combiner, rec.default_row, rec.grad_out,
                                       rec.dw, (size_t)(blockIdx.x - prefix[d]), RaggedArgs{rec.row_splits, rec.nnz, 0u, (i64)0});
}

}  // namespace

namespace tfra {

void launch_find_combine_long_many(hipStream_t s, int cls, unsigned grid, const ManyRec* recs, const unsigned* prefix, unsigned n) {
  with_pool_class(cls / 3, cls % 3, [&](auto DT, auto, auto NCH) {
    find_combine_long_many_kernel<DT, NCH><<<grid, LONG_THREADS, 0, s>>>(recs, prefix, n);
  });
}
void launch_find_combine_ragged_long_many(hipStream_t s, int cls, bool safe, unsigned grid, const RaggedRec* recs,
                                          const unsigned* prefix, unsigned n) {
  with_ragged_class(cls / 3, cls % 3, safe, [&](auto DT, auto, auto NCH, auto SAFE) {
    find_combine_ragged_long_many_kernel<DT, NCH, SAFE><<<grid, LONG_THREADS, 0, s>>>(recs, prefix, n);
  });
}
void launch_wgrad_long_many(hipStream_t s, int cls, unsigned grid, const LongWgradRec* recs, const unsigned* prefix, unsigned n) {
  with_pool_class(cls / 3, cls % 3, [&](auto DT, auto, auto NCH) {
    wgrad_long_many_kernel<DT, NCH><<<grid, LONG_THREADS, 0, s>>>(recs, prefix, n);
  });
}
void launch_wgrad_ragged_long_many(hipStream_t s, int cls, bool prune, unsigned grid, const LongWgradRaggedRec* recs,
                                   const unsigned* prefix, unsigned n) {
  with_ragged_class(cls / 3, cls % 3, prune, [&](auto DT, auto, auto NCH, auto PRUNE) {
    wgrad_ragged_long_many_kernel<DT, NCH, PRUNE><<<grid, LONG_THREADS, 0, s>>>(recs, prefix, n);
  });
}

}  // namespace tfra

// ---- the forward entry points: the twins' frames over the twins' descriptors, each with its flag beside it --------------------------
static PoolDesc long_desc_at(const void* descs, size_t i) {
  const LongDescs& l = *static_cast<const LongDescs*>(descs);
  const tfra_find_combine_desc& d = static_cast<const tfra_find_combine_desc*>(l.descs)[i];
  PoolDesc p{d.struct_size == sizeof(tfra_find_combine_desc), false, reinterpret_cast<Table*>(d.table), nullptr, d.combiner, d.nnz,
             d.ids, d.seg, nullptr, d.weights, d.n_rows, 0, 0, 0, d.default_row, d.out};
  p.long_abi = true;
  p.long_rows = l.flagged(i);
  return p;
}
extern "C" int tfra_multi_find_combine_long(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_desc* descs,
                                            uint32_t* launches_out, const uint8_t* long_rows, tfra_stream_t stream) {
  const LongDescs l{descs, long_rows};
  return multi_find_combine_frame("multi_find_combine_long", ws, n_tables, descs ? &l : nullptr, long_desc_at, launches_out,
                                  (hipStream_t)stream);
}

static PoolDesc long_ragged_desc_at(const void* descs, size_t i) {
  const LongDescs& l = *static_cast<const LongDescs*>(descs);
  const tfra_find_combine_ragged_desc& d = static_cast<const tfra_find_combine_ragged_desc*>(l.descs)[i];
  PoolDesc p{d.struct_size == sizeof(tfra_find_combine_ragged_desc), false, reinterpret_cast<Table*>(d.table), nullptr, d.combiner,
             d.nnz, d.ids, nullptr, d.row_splits, d.weights, d.n_rows, d.flags, d.reserved, d.fill_id, d.default_row, d.out};
  p.long_abi = true;
  p.long_rows = l.flagged(i);
  return p;
}
extern "C" int tfra_multi_find_combine_ragged_long(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_ragged_desc* descs,
                                                   uint32_t* launches_out, const uint8_t* long_rows, tfra_stream_t stream) {
  const LongDescs l{descs, long_rows};
  return multi_find_combine_ragged_frame("multi_find_combine_ragged_long", ws, n_tables, descs ? &l : nullptr, long_ragged_desc_at,
                                         launches_out, (hipStream_t)stream);
}
