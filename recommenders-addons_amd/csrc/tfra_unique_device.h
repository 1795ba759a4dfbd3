// What the kernels of tfra_unique (tfra_unique.hip) and of its grouped form tfra_multi_unique (tfra_unique_many.hip) share: the
// tile shapes, the LDS grouping of a block's equal ids, the first-occurrence flags with their block scan, and a persistent set.
// Both helpers are inlined into their kernels; the single kernels' generated code is what it was with the helpers in their unit
// (profiles/unique_many_isa_stats.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_device.h"

namespace tfra {

constexpr int UNQ_ITEMS = 4;                   // contiguous ids per thread
constexpr int UNQ_TILE = 256 * UNQ_ITEMS;      // ids per block

// scratch open-addressing set: CAS the id in, remember the smallest input index per distinct id.
// Equal ids of one block are grouped in LDS first and only the group's first position touches the
// global set: a Zipf head id (24 000 repeats in a 131 072-id batch) then costs n/512 global atomics
// on its slot instead of one per repeat (516 us -> tens of us for the whole op).
constexpr int UNQ_INS = 512;       // ids = threads per insert block
constexpr unsigned UNQ_LCAP = 1024;  // LDS group table (2x the block: short chains)

// The head of the insert kernels: the block's equal ids grouped in LDS.  Returns the id's place h in the group table; after it
// l_first[h] is the smallest thread of the group (the caller tests l_first[h] == t: first position of its id in this block).
// `zero`: a block counter of the caller's, cleared under the head's first barrier.
__device__ __forceinline__ unsigned unq_group_in_block(int t, bool ok, i64 id, i64* l_id, unsigned* l_own, int* l_first,
                                                       unsigned* zero = nullptr) {
  l_id[t] = id;
  for (unsigned q = t; q < UNQ_LCAP; q += UNQ_INS) { l_own[q] = 0; l_first[q] = 0x7fffffff; }
  if (zero && t == 0) *zero = 0;
  __syncthreads();
  unsigned h = 0;
  if (ok) {
    h = (unsigned)(fmix64((u64)id) >> 20) & (UNQ_LCAP - 1);
    for (;;) {
      unsigned o = l_own[h];
      if (o == 0) {
        o = atomicCAS(&l_own[h], 0u, (unsigned)t + 1u);
        if (o == 0) break;
      }
      if (l_id[o - 1] == id) break;
      h = (h + 1) & (UNQ_LCAP - 1);
    }
    atomicMin(&l_first[h], t);
  }
  __syncthreads();
  return h;
}

// First-occurrence flags of this thread's UNQ_ITEMS ids (id i is the first of its value iff hfirst[slot_of[i]] == i) and the
// exclusive scan of their number over the block in thread order (= input order): returns the number of first occurrences in
// front of this thread's ids in the tile; wsum[0..3] hold the four waves' sums after it.
__device__ __forceinline__ int unq_flags_scan(size_t n, size_t base, const int* hfirst, const int* slot_of, int (&flag)[UNQ_ITEMS],
                                              int* wsum) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < UNQ_ITEMS; ++k) {
    const size_t i = base + k;
    flag[k] = (i < n) && hfirst[slot_of[i]] == (int)i;
    c += flag[k];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int woff = 0;
  for (int k = 0; k < w; ++k) woff += wsum[k];
  return woff + incl - c;
}

// One of the two persistent, self-emptying sets of a three-launch unique (unq2_insert_kernel, tfra_unique.hip)
struct UnqSet {
  i64* hkeys;       // [slots]
  int* hfirst;      // [slots]
  int* hrank;       // [slots]
  unsigned* used;   // [nmax] slots taken by the set's last call
  unsigned* nused;  // their number (zero before its call)
};

}  // namespace tfra
