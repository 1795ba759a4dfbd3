// Device side of the planned admitting lookups that more than one unit launches: the row a 16-lane group holds in registers, and
// the bins launch that copies a key's row and flag from its last position L(k) to the positions in the plan's bins.  Launched by
// tfra_table_find_or_insert_planned (tfra_find_insert.hip) behind find_plan_keys_kernel, and by
// tfra_tier_find_or_insert_planned (tfra_tierplan.hip) behind the tier's chain, with `where` in the place of `found`.
// Both stand here with the lines they had in tfra_find_insert.hip, and keep their code (profiles/tier_planned_isa_stats.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_plan.h"

// A row of at most 1024 bytes in the registers of a 16-lane group: lane `sub` holds granule sub, sub + 16, ... (G = 16 or 8).
// (Native vector types: an array of HIP's uint4 that is filled under a condition is not split into registers, it goes to LDS.)
template <int G>
struct GroupRow {
  typedef unsigned T __attribute__((ext_vector_type(G / 4)));
  T r0, r1, r2, r3;
  __device__ __forceinline__ void load(const unsigned char* src, unsigned bytes, int sub) {
    const unsigned off = (unsigned)sub * G;
    r0 = r1 = r2 = r3 = T(0u);
    if (off < bytes) r0 = *reinterpret_cast<const T*>(src + off);
    if (off + 16 * G < bytes) r1 = *reinterpret_cast<const T*>(src + off + 16 * G);
    if (off + 32 * G < bytes) r2 = *reinterpret_cast<const T*>(src + off + 32 * G);
    if (off + 48 * G < bytes) r3 = *reinterpret_cast<const T*>(src + off + 48 * G);
  }
  __device__ __forceinline__ void store(unsigned char* dst, unsigned bytes, int sub) const {
    const unsigned off = (unsigned)sub * G;
    if (off < bytes) *reinterpret_cast<T*>(dst + off) = r0;
    if (off + 16 * G < bytes) *reinterpret_cast<T*>(dst + off + 16 * G) = r1;
    if (off + 32 * G < bytes) *reinterpret_cast<T*>(dst + off + 32 * G) = r2;
    if (off + 48 * G < bytes) *reinterpret_cast<T*>(dst + off + 48 * G) = r3;
  }
};

// Bins launch, behind the key launch's kernel boundary: one block per bin of SEG entries, a 16-lane group per 16-entry item (the
// layout plan_dest_bins_kernel walks).  The item's run belongs to one key, whose row and flag the key launch left at L(k): every
// other position of the item copies them from there.  (rows[L(k)] itself is written by nobody in this launch.)
template <int G>
__global__ __launch_bounds__(NTA) void find_plan_bins_kernel(const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                                             const unsigned* __restrict__ binmap, const unsigned* __restrict__ d_counts,
                                                             const int* __restrict__ prow_dest, unsigned char* rows, uint8_t* found,
                                                             unsigned fb, unsigned n) {
  constexpr int NG = NTA / 16;
  __shared__ unsigned char s_kind[NG];   // 0 = continues the run of the item before, 1 = first item of a run, 2 = empty item
  __shared__ unsigned s_row[NG];
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, g = threadIdx.x >> 4;
  const unsigned nbins = d_counts[PC_BINS];
  for (unsigned ib = blockIdx.x; ib < nbins; ib += gridDim.x) {
    const unsigned bin = binmap[ib];
    const unsigned e = hent[(size_t)bin * SEG + threadIdx.x];
    const unsigned e0 = (unsigned)__shfl((int)e, gshift);
    const bool empty = (e0 & E_SKIP) != 0, first = (e0 & E_HEAD) != 0;
    if (sub == 0) {
      s_kind[g] = empty ? 2 : (first ? 1 : 0);
      s_row[g] = (first && !empty) ? hout[(size_t)bin * 32 + g] : 0u;
    }
    __syncthreads();
    if (!empty) {   // (uniform in the group)
      int g2 = g;
      while (g2 > 0 && s_kind[g2] == 0) --g2;
      const unsigned L = (unsigned)prow_dest[s_row[g2]];
      if (L < n) {
        GroupRow<G> r;
        r.load(rows + (size_t)L * fb, fb, sub);
        const uint8_t f = found ? found[L] : 0;
        for (int j = 0; j < 16; ++j) {
          const unsigned ej = (unsigned)__shfl((int)e, gshift + j);
          const unsigned p = ej & E_POS;
          if ((ej & E_SKIP) || p == L || p >= n) continue;
          r.store(rows + (size_t)p * fb, fb, sub);
          if (found && sub == 0) found[p] = f;
        }
      }
    }
    __syncthreads();
  }
}
