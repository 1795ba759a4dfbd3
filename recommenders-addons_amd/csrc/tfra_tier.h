// What the tier calls of a table (tfra_tier.hip) share with the tier driver (tfra_tierstep.hip): the block shape of
// find_missed_kernel, the miss list it appends to, and its ONE launcher; and what the driver shares with the tier's pooled lookup
// (tfra_tierpool.hip) and its weight gradient (tfra_tierwgrad.hip): the driver's object and the locks a call on it takes; and with
// the grouped admission (tfra_tierstep_many.hip): the checks of tfra_tier_find_or_insert, the fetch's operands, the grouped locks;
// and with the planned admission (tfra_tierplan.hip): the stages of the chain behind its own key launch.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "tfra_host.h"
#include "tfra_many.h"

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

// What tier_fetch_kernel (tfra_tierstep.hip) and its grouped twin (tfra_tierstep_many.hip) read and write beside the lower table.
struct FetchIO {
  const tfra::i64* keys;          // the miss list, *d_count entries of at most cap
  const int* pos_of;              // the batch position of each
  const tfra::u64* d_count;
  size_t cap;
  unsigned char* out;             // [n, field_bytes] by batch position; may be null
  uint8_t* where;                 // [n] by batch position: 2 = found below, 0 = never seen; may be null
  const unsigned char* defaults;  // the row of a key that is not below: row `position` when full, else row 0
  int full;
  unsigned char* stage;           // null (tier_find), or [cap, whole]: row j = the whole row of listed key j
  tfra::u64* lower_hits;          // statistics word
};

// The driver's words on the device: the cumulative statistics, then the two counters of the call in flight.
enum { TS_CALLS = 0, TS_MISSED = 1, TS_LOWER_HITS = 2, TS_DEMOTED = 3, TS_NOT_RESIDENT = 4, TS_WORDS = 8, TC_MISSED = 8, TC_DOWN = 9, TIER_WORDS = 10 };

// The tier driver's object (tfra_tierstep.hip makes and drives it; the tier's pooled lookup, tfra_tierpool.hip, reads its tables).
struct tfra_tier {
  tfra::Table* upper = nullptr;
  tfra::Table* lower = nullptr;
  size_t max_batch = 0;
  unsigned fb = 0, whole = 0;       // bytes of the embedding field and of the whole co-located row
  unsigned char* block = nullptr;   // ONE allocation, carved below
  tfra::u64* words = nullptr;       // [TIER_WORDS]
  tfra::i64* miss_keys = nullptr;   // [max_batch] what the upper table missed ...
  int* miss_idx = nullptr;          // [max_batch] ... and at which batch position
  int* miss_rec = nullptr;          // [max_batch] the planned admission (tfra_tierplan.hip): ... and which key of the plan it is
  unsigned char* up_rows = nullptr;    // [max_batch, whole] what comes up
  tfra::i64* down_keys = nullptr;      // [max_batch] what goes down: keys,
  unsigned char* down_rows = nullptr;  // [max_batch, whole] whole rows
  tfra::u64* down_scores = nullptr;    // [max_batch] and scores
  std::mutex mu;                    // the staging belongs to one call at a time
};

// The head of every call on a tier: the driver's lock and both tables' (tfra_many.h: each once, in one global order, entered on s).
struct TierEntry {
  std::unique_lock<std::mutex> own;
  std::vector<std::unique_lock<std::mutex>> tables;
};
static inline int tier_enter(tfra_tier* tier, hipStream_t s, TierEntry* e) {
  e->own = std::unique_lock<std::mutex>(tier->mu);
  return tfra::lock_and_enter({tier->upper, tier->lower}, s, &e->tables);
}

// The locks of a grouped call over tiers: each distinct tier's own mutex once, in address order, BEFORE any table lock — the
// hierarchy of tier_enter — then every table of the call (plain ones, uppers and lowers) once, in the global order, entered on s.
// (Members are released in reverse order.)
struct TierLocks {
  std::vector<std::unique_lock<std::mutex>> tiers, tables;
};
static inline int lock_tiers_and_tables(std::vector<tfra_tier*> tiers, std::vector<tfra::Table*> tabs, hipStream_t s, TierLocks* l) {
  std::sort(tiers.begin(), tiers.end(), std::less<tfra_tier*>());
  tiers.erase(std::unique(tiers.begin(), tiers.end()), tiers.end());
  l->tiers.reserve(tiers.size());
  for (tfra_tier* t : tiers) l->tiers.emplace_back(t->mu);
  return tfra::lock_and_enter(std::move(tabs), s, &l->tables);
}

// The argument checks of tfra_tier_find_or_insert, in its order, for that call and for every descriptor of
// tfra_multi_tier_find_or_insert (tfra_many.h: an operation's checks are ONE function).
static inline tfra::Check check_tier_find_or_insert(const tfra_tier* tier, size_t n, const void* keys, const void* init_values,
                                                    uint32_t flags) {
  if (!tier) return tfra::refuse(TFRA_ERR_INVALID, "null tier");
  if (flags & ~TFRA_TIER_VERIFY) return tfra::refuse(TFRA_ERR_INVALID, "unknown flag bits");
  if (n == 0) return tfra::nothing_to_do();
  if (!keys || !init_values) return tfra::refuse(TFRA_ERR_INVALID, "null buffer");
  if (n > tier->max_batch) return tfra::refuse(TFRA_ERR_INVALID, "more keys than the tier's max_batch");
  return tfra::Check{};
}

// The stages of a tier's admitting chain that the planned admission (tfra_tierplan.hip) runs behind its own key launch, for a
// caller that holds the tier's locks (tier_enter); defined in tfra_tierstep.hip.  tier_begin: the launch of tier_begin_kernel.
// launch_fetch: step 2, tier_fetch_kernel over the miss list.  tier_put: steps 3 and 4, `values` into the upper table, what that
// displaces as whole rows into the lower one.  (Hidden: shared by the library's units, not dynamic symbols.)
__attribute__((visibility("hidden"))) void tier_begin(tfra_tier* tier, hipStream_t s);
__attribute__((visibility("hidden"))) void launch_fetch(tfra::Table* lower, hipStream_t s, size_t n, const FetchIO& io, const tfra::AuxInitPod& ai);
__attribute__((visibility("hidden"))) int tier_put(tfra_tier* tier, hipStream_t s, size_t n, const long long* d_n, const tfra::i64* keys,
                                                   const unsigned char* values, bool whole_in);

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
