// What the grouped calls share (tfra_multi_find_combine: tfra_pool.hip; tfra_multi_apply_planned_combined: tfra_apply.hip, with its
// entry-record kernels in tfra_frontend.hip): the search that takes a block to its descriptor, the records of the launches that
// run in more than one unit, and the pinned staging ring the records reach the device through.
// The types live in namespace tfra (not in an anonymous one): their launchers cross translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"

namespace tfra {

// The descriptor of block `blk`: the d with prefix[d] <= blk < prefix[d + 1] (prefix[0] = 0, prefix[n] = the grid; strictly
// ascending: no descriptor has zero blocks).  blk is blockIdx.x, so the search, the record's address and the record are
// wave-uniform: scalar loads into scalar registers, as kernel arguments are.
__device__ __forceinline__ unsigned many_desc_of(const unsigned* __restrict__ prefix, unsigned n, unsigned blk) {
  unsigned lo = 0, hi = n;
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (prefix[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// seg64_bounds_many_kernel (tfra_pool.hip): one descriptor's rows' bounds; it owns ceil(nnz / 256) blocks
struct BoundsRec {
  const i64* seg;
  int* se;
  size_t nnz;
  size_t n_rows;
};
// grid = prefix[n]; recs / prefix in device memory
int comb_bounds_many(hipStream_t s, unsigned grid, const BoundsRec* recs, const unsigned* prefix, unsigned n);

// comb_den_many_kernel / comb_ent_many_kernel (tfra_frontend.hip): one descriptor's denominators (ceil(n_rows / 256) blocks) and
// per-entry records (ceil(nnz / 256) blocks), what comb_entries makes for one table
struct CombManyRec {
  const i64* seg;
  const float* w;
  const int* se;
  float* den;
  CombEnt* ent;
  size_t nnz;
  size_t n_rows;
  int combiner;
};
// two launches: the denominators of all descriptors' rows, then all descriptors' entry records
int comb_den_ent_many(hipStream_t s, unsigned den_grid, unsigned ent_grid, const CombManyRec* recs, const unsigned* den_prefix,
                      const unsigned* ent_prefix, unsigned n);

// The records reach the device by ONE asynchronous copy per call from a pinned staging slot.  Two calls may be enqueued back to
// back with nothing waited for in between, so a slot must not be rewritten while its copy has not run: the slots form a ring,
// each guarded by an event recorded behind its copy.  Taking a slot waits for ITS event only — in the steady state the copy of
// RING calls ago, long done — never for the stream.  A list that outgrows the slots waits for the pending copies and reallocates.
// One ring per workspace (tfra_workspace::many), whichever grouped call uses it.
struct ManyStage {
  static constexpr int RING = 8;
  unsigned char* host = nullptr;
  size_t slot_bytes = 0;
  hipEvent_t ev[RING] = {};
  bool pending[RING] = {};
  unsigned next = 0;

  static int hip_rc(hipError_t e, const char* what) {
    if (e == hipSuccess) return TFRA_OK;
    return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  int drain() {
    for (int i = 0; i < RING; ++i)
      if (pending[i]) {
        if (int rc = hip_rc(hipEventSynchronize(ev[i]), "staging ring: hipEventSynchronize")) return rc;
        pending[i] = false;
      }
    return TFRA_OK;
  }
  int take(size_t need, unsigned char** out, int* slot) {
    if (!ev[0])
      for (int i = 0; i < RING; ++i)
        if (int rc = hip_rc(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), "staging ring: hipEventCreateWithFlags")) return rc;
    if (need > slot_bytes) {
      int rc = drain();
      if (rc) return rc;
      if (host) {
        if ((rc = hip_rc(hipHostFree(host), "staging ring: hipHostFree"))) return rc;
        host = nullptr; slot_bytes = 0;
      }
      const size_t want = (std::max<size_t>(need, 8192) + 4095) / 4096 * 4096;
      if ((rc = hip_rc(hipHostMalloc((void**)&host, want * RING, hipHostMallocDefault), "staging ring: hipHostMalloc"))) { host = nullptr; return rc; }
      slot_bytes = want;
    }
    const int i = (int)(next++ % RING);
    if (pending[i]) {
      if (int rc = hip_rc(hipEventSynchronize(ev[i]), "staging ring: hipEventSynchronize")) return rc;
      pending[i] = false;
    }
    *out = host + (size_t)i * slot_bytes;
    *slot = i;
    return TFRA_OK;
  }
  // behind the copy out of slot `slot` on stream s
  int sent(int slot, hipStream_t s) {
    if (int rc = hip_rc(hipEventRecord(ev[slot], s), "staging ring: hipEventRecord")) return rc;
    pending[slot] = true;
    return TFRA_OK;
  }
};

// the workspace's ring, made on first use
inline ManyStage* many_stage_of(tfra_workspace* ws) {
  if (!ws->many) ws->many = new ManyStage();
  return reinterpret_cast<ManyStage*>(ws->many);
}

}  // namespace tfra
