// Device side of the tier calls that more than one unit launches: the body of find_missed (tfra_tier.hip: find_missed_kernel,
// find_missed_touch_kernel), taking the index of its block as an argument so that the grouped admission (tfra_tierstep_many.hip,
// DESIGN §4.25) runs the SAME code on a block index local to its descriptor.  The single kernels hand in blockIdx.x and keep
// their code (profiles/tier_admit_many_isa_stats.txt).
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_host.h"
#include "tfra_tier.h"

// ---- find_missed ----------------------------------------------------------------------------------------------------------------
// A block is TILES tiles of 64 keys, one wave per 16 keys, all through find_wave at once; each wave leaves its 16-bit miss mask in
// LDS.  Then ONE wave scans the 4 * TILES counts, ONE lane takes the block's range with ONE atomicAdd (none when the block has no
// miss), and every wave stores its pairs at the base it was given: plain vector stores, behind every load group of the lookup.
// X: TierMissed, or TierMissedTouch (the tier driver's step 1) with its miss mask zeroed.
// blk: the block's index among the blocks of THIS key list (blockIdx.x in a launch over one list).
template <int G, int U, bool PF1, int TILES, class X>
__device__ __forceinline__ void find_missed_body(tfra::TableView v, size_t n, const tfra::i64* __restrict__ keys, unsigned char* __restrict__ out,
                                                 uint8_t* __restrict__ exists, const unsigned char* __restrict__ defaults, int full,
                                                 const long long* __restrict__ d_n, MissOut mo, X x, const unsigned blk) {
  using namespace tfra;
  constexpr int NW = 4 * TILES;   // waves per block
  __shared__ unsigned s_mask[NW];
  __shared__ u64 s_base[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned wave = blk * NW + w;
  find_wave<G, U, G == 16, PF1, X>(v, served(n, d_n), keys, out, exists, defaults, full, 0u, wave, &x);
  if (!mo.counter) return;   // (uniform) find plus scores
  if (lane == 0) s_mask[w] = x.miss;
  __syncthreads();
  if (w == 0) {
    const unsigned c = lane < NW ? (unsigned)__popc(s_mask[lane]) : 0u;
    unsigned incl = c;
#pragma unroll
    for (int o = 1; o < NW; o <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, o);
      if (lane >= o) incl += up;
    }
    const unsigned total = (unsigned)__shfl((int)incl, NW - 1);
    u64 b = 0;
    if (lane == 0 && total) b = atomicAdd(mo.counter, (u64)total);
    b = (u64)shfl_i64((i64)b, 0);
    if (lane < NW) s_base[lane] = b + (incl - c);
  }
  __syncthreads();
  if (!mo.keys && !mo.idx) return;   // count only
  if (lane >= 16 || !((x.miss >> lane) & 1u)) return;
  const unsigned i = wave * 16 + lane;   // (a bit is only set for i < n)
  const u64 p = s_base[w] + (unsigned)__popc(x.miss & ((1u << lane) - 1u));
  if (p >= mo.cap) return;
  if (mo.keys) mo.keys[p] = keys[i];
  if (mo.idx) mo.idx[p] = (int)i;
}
