// Device side of the write-back plans (tfra_csr.hip builds the CSR plan, tfra_setplan.hip the SET plan): the CSR plan's layout and
// records, the SET plan's table and its probes, and the control words of a plan's count blocks (host and device).  Shared by the
// plan kernels, the gradient half (tfra_apply_device.h), the ownership pass (tfra_own_device.h) and the overlapped step
// (tfra_step_impl.h).
//
// Everything here stays in the anonymous namespace, as it was when one file held all of it: kernels take these types by value,
// and a kernel's mangled name (what rocprofv3 and scripts/summarize_profile.py see) carries its parameters' namespaces.
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_device.h"
#include "tfra_reduce_device.h"

namespace {

using namespace tfra;
using namespace tfra::red;

constexpr int DIRECT = 8;                 // occurrences the update kernel gathers by itself
constexpr int SEG = 512;                  // entries of a hot bin = rows one hot_sums block reduces
constexpr unsigned E_SKIP = 1u << 31, E_HEAD = 1u << 30, E_POS = (1u << 18) - 1;
constexpr unsigned TABW = 2048;           // u32 entries of the per-pass tile table (8 KB: 8 keys x 256 tiles per round)
constexpr unsigned CTR_STRIDE = 16;       // u64 words between two counters (one 128-B line each)
constexpr int MAXPASS_SPLIT = 64;
// Output space is handed out by ATOMIC counters, and same-line atomics of different workgroups serialise at ~25 ns
// each on this chip (1024 bucket blocks on ONE counter line: 25 us, measured).  So the outputs are split into NSH
// shards with private counters and private ranges: bucket b allocates in shard b % NSH (P/NSH = 16 atomics per line),
// and the last plan kernel publishes dense maps (keymap / binmap) over the shards for the kernels of the other half.
constexpr unsigned NSH = 64;
constexpr unsigned REC_WORDS = 16;        // a key record = 64 B: [0,1] key [2] count; few occurrences: [3] last position, [4..11] its batch
                                          // positions, ascending; many: [3] first partial row [4] #partials [5] entry
                                          // address of its last occurrence
constexpr unsigned KM_MANY = 1u << 31;    // keymap: the record lives in `hrec`

// ---------------------------------------------------------------------------------------------
// The plan's CONTROL WORDS: the one map of the 32-bit words a plan object's count blocks hold, for the host and for the kernels of
// every unit (which are compiled separately: a word that moves here moves in all of them, and none may move by accident —
// the static_asserts below and in tfra_own_device.h).
//   d_counts block (PC_*; PC_WORDS words): the head of whichever buffer holds the object's last build — the CSR buffer's
//     (plan_lay_out, tfra_csr.hip) or the SET buffer's (set_counts; setplan_prepare, tfra_setplan.hip).  The last CSR plan kernel
//     publishes words [0, PC_PUBLISHED); the write-backs keep their own words behind them.
//   SET buffer (SC_*; SC_WORDS words, of which the first PC_WORDS are its d_counts block): each of the two tables has two USE
//     blocks that alternate from build to build.  A use block is laid out as the head of a d_counts block ON PURPOSE — {0, distinct
//     keys, 0, 0, 0, 0}: PC_HOT = 0, PC_COLD = the count, no bins, no overflow — so that CsrKeys::d_counts may point at it (keys_of)
//     and every consumer of a plan's keys reads "PC_HOT + PC_COLD keys" whatever the plan's kind.
//   pinned copy (HC_*; host_counts): the generation of the last COMPLETED CSR build, then its published words.
enum : unsigned {
  PC_HOT = 0,             // keys with more than DIRECT occurrences (a SET use block: always 0 — the one-launch unique counts its blocks here)
  PC_COLD = 1,            // the other keys (a SET use block: all distinct keys)
  PC_BINS = 3,            // hot bins of the build
  PC_OVERFLOW = 5,        // errors of the build, latched: its keys are incomplete
  PC_PUBLISHED = 6,       // words the last CSR plan kernel publishes, device and pinned copy (words 2 and 4: unused, zero)
  PC_ANY_DEFERRED = 8,    // = use_gen of the last write-back that deferred a key to its eviction phase
  PC_OWN_CTRS = 12,       // the two OwnCtrs sets of the ownership write-back (tfra_own_device.h), PC_OWN_CTRS_WORDS in all
  PC_OWN_CTRS_WORDS = 8,
  PC_PART_COUNT = 32,     // i64 (two words): PC_HOT + PC_COLD as tfra_partition reads a count (tfra_plan_partition)
  PC_WORDS = 64,
  SC_USE_BASE = 64,       // first use block: table p, use u at SC_USE_BASE + SC_TAB_STRIDE p + SC_USE_STRIDE (u & 1)
  SC_USE_STRIDE = 8,
  SC_TAB_STRIDE = 16,     // a table's two use blocks: what filling a table zeroes
  SC_USE_COUNT = PC_COLD, // the count inside a use block (SetTab::count points at it)
  SC_ZERO = 120,          // a word that is always zero: the "list length" of a table that has no list
  SC_WORDS = 128,
  HC_GEN = 0,             // pinned copy: the generation word ...
  HC_SHIFT = 1,           // ... and published word k at HC_SHIFT + k
};
static_assert(PC_HOT == 0 && PC_COLD == 1 && PC_BINS == 3 && PC_OVERFLOW == 5 && PC_PUBLISHED == 6 && PC_ANY_DEFERRED == 8 &&
              PC_OWN_CTRS == 12 && PC_PART_COUNT == 32 && SC_USE_BASE == 64 && SC_USE_STRIDE == 8 && SC_TAB_STRIDE == 16 &&
              SC_USE_COUNT == 1 && SC_ZERO == 120 && HC_GEN == 0 && HC_SHIFT == 1,
              "kernels of other units read these words: the layout does not move");
static_assert(PC_PUBLISHED <= PC_ANY_DEFERRED && PC_ANY_DEFERRED < PC_OWN_CTRS && PC_OWN_CTRS + PC_OWN_CTRS_WORDS <= PC_PART_COUNT &&
              PC_PART_COUNT % 2 == 0 && PC_PART_COUNT + 2 <= PC_WORDS, "the d_counts block's words do not overlap");
static_assert(SC_USE_BASE >= PC_WORDS && SC_TAB_STRIDE == 2 * SC_USE_STRIDE && PC_PUBLISHED <= SC_USE_STRIDE &&
              SC_USE_BASE + 2 * SC_TAB_STRIDE <= SC_ZERO && SC_ZERO < SC_WORDS, "the SET buffer's use blocks end before the always-zero word");
// the count word of use `use` of table `table` of a SET buffer whose control words start at `base`
__host__ inline unsigned* set_count_word(unsigned* base, unsigned table, unsigned use) {
  return base + SC_USE_BASE + SC_TAB_STRIDE * table + SC_USE_STRIDE * (use & 1u) + SC_USE_COUNT;
}

// global descriptor store: bucket b owns [b*CMAX, b*CMAX + cm); overflow list behind it
struct CsrDesc {
  i64* key;
  unsigned* ord;        // tile << 18 | (count == 1: position in tile, else: run index in the tile) << 9 | (count - 1)
  unsigned* cursor;     // [P] one per 128-B line
  i64* ovf_key;
  unsigned* ovf_ord;
  unsigned* ovf_bucket;
  unsigned* ovf_count;
  unsigned ovf_cap;
};

struct CsrOut {
  u64* counters;        // [NSH] one per line: few-keys | many-keys << 16 | partials << 32 | bins << 48; [NSH]: deferred keys
  unsigned* crec;       // [NSH*cr] records of the keys with <= DIRECT occurrences
  unsigned* hrec;       // [NSH*hr] records of the others
  unsigned* hent;       // [NSH*br] bins of SEG entries: batch position | E_HEAD | E_SKIP
  unsigned* hout;       // [NSH*br*32] per 16-entry item: partial row of the run starting there
  unsigned cr, hr, pr, br;   // per-shard capacities: records, records, partial rows, bins
};

// ---------------------------------------------------------------------------------------------
struct CsrKeys {
  const unsigned* keymap;
  const i64* dkeys;
  const unsigned* crec; const unsigned* hrec;
  const unsigned* hent;
  const unsigned* d_counts;
  // SET plan (assign-only, see setplan_kernel): dense distinct keys, their slots, (last position + 1, occurrences) per slot
  const i64* ukeys;
  const unsigned* uslot;
  const struct SetEnt* sent;
};
// One slot of a SET plan's open-addressing table: 16 B, so that a probe is ONE load (the overlapped step's lookup probes the
// previous batch's plan for every id: find_fwd_role, tfra_step_impl.h)
struct SetEnt { i64 key; unsigned pos1, cnt; };   // key (EMPTY_KEY = free) | last position + 1 | occurrences
__device__ __forceinline__ uint2 set_pc(const SetEnt* e) { return *reinterpret_cast<const uint2*>(&e->pos1); }
// A SET plan's table as something to PROBE (read-only): is this key one of the batch's ids, and where is its last occurrence?
// Probe chains stay inside a WINDOW of SET_WIN consecutive slots (home slot = hash & (m2 - 1); the slot behind the window's last
// is its first): the overlapped step builds a plan one window per workgroup, in LDS, without atomics (tfra_step_impl.h), and
// every other builder and every prober follows the same rule.  (m2 >= 2 n slots for n ids: a window overflows never.)
constexpr unsigned SET_WIN = 2048, SET_WIN_LOG2 = 11;
constexpr unsigned SEG_CAP = 32;   // pairs per (window, tile) segment of a scatter (tfra_step_impl.h); more: the overflow list
__host__ __device__ __forceinline__ unsigned set_wmask(unsigned m2) { return (m2 < SET_WIN ? m2 : SET_WIN) - 1u; }
__device__ __forceinline__ unsigned set_at(unsigned slot, unsigned g, unsigned wm) { return (slot & ~wm) | ((slot + g) & wm); }   // g slots on, inside the window
struct SetProbe { const SetEnt* ent; unsigned m2; };   // m2 entries (a power of two) + the two sentinel slots + padding
__device__ __forceinline__ unsigned set_home(const SetProbe& p, i64 key, u64 h) {   // h = fmix64(key)
  return is_reserved_key(key) ? p.m2 + (unsigned)reserved_index(key) : (unsigned)(h >> 20) & (p.m2 - 1);
}
// All 16 lanes of a key group: does the table hold `key`?  Lanes 0..3 look at four consecutive entries per round (linear
// probing, slots are never freed during a build: a match anywhere is the key, an EMPTY entry before it ends the search).
__device__ __forceinline__ bool set_contains_group(const SetProbe& p, i64 key, int sub, int gshift) {
  const bool resv = is_reserved_key(key);
  unsigned slot = set_home(p, key, fmix64((u64)key));
  const unsigned wm = set_wmask(p.m2);
  for (int round = 0; round < 512; ++round) {
    const unsigned e = resv ? slot + (unsigned)(sub & 3) : set_at(slot, (unsigned)(sub & 3), wm);
    const i64 k = p.ent[e].key;
    const bool match = resv ? ((sub & 3) == 0 && k != EMPTY_KEY) : k == key;
    const unsigned mm = (unsigned)(__ballot(match && sub < 4) >> gshift) & 0xfu;
    const unsigned em = (unsigned)(__ballot(k == EMPTY_KEY && sub < 4) >> gshift) & 0xfu;
    if (mm) return true;
    if (em || resv) return false;
    slot = set_at(slot, 4u, wm);
  }
  return true;   // (a chain this long does not exist: 2 n slots for n ids; say "present", the conservative answer)
}

// The same for TWO plans at once (lanes 0..3 probe p, lanes 4..7 probe q: one round trip for both): is the key in either?
__device__ __forceinline__ bool set_contains_either_group(const SetProbe& p, const SetProbe& q, i64 key, int sub, int gshift) {
  const bool resv = is_reserved_key(key);
  const SetProbe& t = (sub & 4) ? q : p;
  unsigned slot = set_home(t, key, fmix64((u64)key));
  const unsigned wm = set_wmask(t.m2);
  unsigned open = 3u;   // bit 0: still looking in p, bit 1: in q
  for (int round = 0; round < 512 && open; ++round) {
    const unsigned e = resv ? slot + (unsigned)(sub & 3) : set_at(slot, (unsigned)(sub & 3), wm);
    const i64 k = t.ent[e].key;
    const bool match = resv ? ((sub & 3) == 0 && k != EMPTY_KEY) : k == key;
    const unsigned mm = (unsigned)(__ballot(match && sub < 8) >> gshift) & 0xffu;
    const unsigned em = (unsigned)(__ballot(k == EMPTY_KEY && sub < 8) >> gshift) & 0xffu;
    if ((mm & 0x0fu) && (open & 1u)) return true;
    if ((mm & 0xf0u) && (open & 2u)) return true;
    if ((em & 0x0fu) || resv) open &= ~1u;
    if ((em & 0xf0u) || resv) open &= ~2u;
    slot = set_at(slot, 4u, wm);
  }
  return open != 0;   // (a chain this long does not exist; "present" is the conservative answer)
}

// one coalesced 64-B load per key group: lane i holds word i of the key's record
__device__ __forceinline__ unsigned load_record(const CsrKeys& ks, unsigned g, int sub, bool& many) {
  const unsigned km = ks.keymap[g];
  many = (km & KM_MANY) != 0;
  return (many ? ks.hrec : ks.crec)[(size_t)(km & ~KM_MANY) * REC_WORDS + sub];
}

constexpr unsigned SET_PAD = 4;   // entries behind the two sentinel slots, never used: a probe reads 4 consecutive entries
struct SetTab {   // one of the plan's two tables
  SetEnt* ent;      // [m2 + 2 + SET_PAD]  key: EMPTY_KEY = free (the two sentinel slots [m2], [m2 + 1]: EMPTY_KEY = free, else taken)
  i64* ukeys;       // [n] dense list: the distinct keys, in no particular order
  unsigned* uslot;  // [n] their slots
  unsigned* count;  // number of distinct keys of the table's current use (zero before its build)
};

}  // namespace
