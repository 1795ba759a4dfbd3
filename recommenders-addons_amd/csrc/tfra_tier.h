// What the tier calls of a table (tfra_tier.hip) share with the tier driver (tfra_tierstep.hip): the block shape of
// find_missed_kernel, the miss list it appends to, and its ONE launcher.
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_host.h"

// 64-key tiles (four waves each) that ONE block of find_missed_kernel covers — a block of 256 * TIER_TILES threads — and so the keys
// behind one atomicAdd on the miss counter: 64 * TIER_TILES.  Adds to one address serialise (DESIGN §4 measured ~150 M/s), so
// B = 131 072 keys cost 2048 / TIER_TILES adds.  The tiles of a block run side by side, not one after the other: the launch has
// find_kernel's waves in flight whatever the value.  The value kept is the one scripts/mb_find_missed.py measured best
// (profiles/find_missed_mb.jsonl); a build with -DTFRA_TIER_TILES=N tries another.
#ifndef TFRA_TIER_TILES
#define TFRA_TIER_TILES 4
#endif
constexpr int TIER_TILES = TFRA_TIER_TILES;
static_assert(TIER_TILES == 1 || TIER_TILES == 2 || TIER_TILES == 4, "a block has at most 1024 threads");

// Where the miss list goes (tfra_table_export_batch_if's counter and cap rules).
struct MissOut {
  tfra::u64* counter;    // device size_t, advanced by every miss whatever cap is; null: no list
  tfra::u64 cap;         // pairs at positions >= cap are not written
  tfra::i64* keys;       // may be null
  int* idx;              // may be null
  tfra::u64* scores;     // find_missed's scores_out: may be null
};

__device__ __forceinline__ size_t served(size_t n, const long long* d_n) {   // min(n, *d_n), a negative count = 0 (find_kernel's)
  if (!d_n) return n;
  const long long dn = *d_n;
  return dn < 0 ? 0 : min(n, (size_t)dn);
}
static inline unsigned blocks_of(size_t n, int tiles) { return (unsigned)((n + 64 * (size_t)tiles - 1) / (64 * (size_t)tiles)); }

// The launch of tfra_table_find_missed behind its argument checks, for a caller that holds the table's lock and has entered it on s.
// touch: the hits' scores are touched as tfra_table_assign touches them (find_missed_touch_kernel; the tier driver's step 1).
// (Hidden: shared by the library's units, not one of its dynamic symbols.)
__attribute__((visibility("hidden"))) void launch_find_missed(tfra::Table* t, hipStream_t s, size_t n, const long long* d_n, const tfra::i64* keys,
                        unsigned char* values, uint8_t* exists, const unsigned char* defaults, int full, const MissOut& mo, bool touch);
