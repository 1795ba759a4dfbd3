// Device side of the ASSIGN write-back with bucket ownership: the pass's arguments and per-key protocol (own_batch16), the
// locked protocol of the keys it leaves over (locked_upsert_kv).  Shared by the ownership kernels (tfra_own.hip) and the
// overlapped step's OWN / TAIL roles (tfra_step_impl.h).  Anonymous namespace: see tfra_plan_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_optim_device.h"
#include "tfra_plan_device.h"

namespace {

constexpr unsigned SLOW_CAP = 8192;   // items of the left-over list of an ownership pass (more: the flags of all keys are scanned)

// ---------------------------------------------------------------------------------------------
// ASSIGN write-back, single pass with BUCKET OWNERSHIP (without owner tags — TFRA_OPTION_NO_OWNER_TAGS — every key takes the
// locked protocol of upsert_rest_kernel).
// Every bucket has an owner tag (one 32-bit word in a dense side array — NOT in the bucket's key line: an atomic and a
// load issued together on the same 128-B line cost 41 us per 157 K instead of 11 us on separate lines,
// scripts/mb/atomic_probe.hip).  Every key of the launch swaps the launch's generation into the tags of its two home
// buckets (two atomic exchanges in flight with its line loads) and owns a bucket iff the tag it got back is from an
// older launch.  A key that owns BOTH home buckets is the
// only writer of the launch that can touch them — every other key of the launch whose sequence includes one of them
// fails that claim and leaves the table alone — so it resolves hit / free slot / minimum-score eviction with plain
// loads and stores: no CAS, no LOCKED state, no score re-read, no publish ordering, and ONE dependent round trip (the
// four lines and the two claims are in flight together) instead of the five of the locked protocol.
//
// LEFT-OVER keys: a key that loses a claim (two keys of one batch sharing a home bucket: ~(2U)^2 / (2 nb) of them, 16 of
// 23 K / 185 of 78 K on 10^9 slots) or that cannot be placed within its two home buckets appends a self-contained ITEM
// (key, value position, input score) to the launch's list; upsert_rest_kernel takes the items afterwards with the locked
// protocol.  A key that MAY live beyond its home buckets (both overflow flags set, ~0.1 % of the buckets of a table filled
// to capacity) is looked for with reads in the main pass and claims the bucket it is found in.
//
// Round 3 measurements on the 10^9-slot table (scripts/mb_own.py, mb_sweep.py; rocprofv3 per-kernel times):
//   * the pass costs 13 us + 0.23 us per 1000 keys: 3.0 us launch + key load, 5.5 us until the four lines AND the two
//     claims are back (the lines alone 3.5 us — every access is a TLB miss on 273 GB), 4 us of dependent ALU / cross-lane
//     work for ONE wave's 16 keys, 0.5 us value rows, 1 us stores;
//   * the claims are ~5 us of 32 (78 K keys), their footprint does not matter (tags folded into 8 MB: same time);
//   * tried and dropped: the left-over keys in two more OWNERSHIP rounds — by the last block of the pass (ticket) or by a
//     one-block kernel behind it — 14-19 us against 10-12 us for 32 blocks of the locked protocol (one workgroup is one
//     dependent chain per round, and the code of the rounds costs the pass registers); claim-after-look with shared /
//     exclusive claim words in the score lines (an atomic on a line that has just been read is still a fabric
//     read-modify-write, and it now sits behind the lines instead of beside them): 35 / 38 us against 30 / 24;
//     the value row prefetched with the lines (direct keys): 42 us against 31 (16 more registers per lane, spills).

// One left-over key with the locked protocol for every kind of write: locate or claim the key's slot, LOCK it (CAS key
// -> LOCKED: a concurrent evictor of this pass may have taken it, then start over), or lock a victim (evict_and_lock);
// write row and score write-through, publish the key.  With every writer of the pass holding its slot locked, an assign
// can no longer race with the eviction of the same slot, which is what the two separate kernels (assign / claim, then
// evict) are for when they handle a whole batch.
// hint (a left-over key of the ownership pass that FOUND its key but had lost a claim): the slot it saw the key in — locked
// straight away, without reading the lines again (two dependent round trips less for 15 of the 16 left-over keys of the
// metric's batch); somebody took the slot in between: the ordinary way.
template <int G>
__device__ __forceinline__ void locked_upsert_kv(const TableView& v, const unsigned char* __restrict__ vals, i64 key, unsigned last,
                                                 u64 in_score, const AuxInitPod& ai, const ScoreP& sp, int sub, int gshift,
                                                 int& fresh, int& failed, bool hinted = false, unsigned hint_word = 0,
                                                 i64* evicted_key = nullptr, int acc = 0, int acc_dt = 0, i64* given_back = nullptr,
                                                 int* n_given_back = nullptr) {
  // evicted_key (optional): set to the key this upsert replaced by eviction (untouched when it evicted nothing)
  // acc: the reference's insert_or_accum for this key (accumrase_fn, cuckoohash_map.hh:619-633) instead of an assign —
  //   1 (exists): present -> row += delta, one add per element; absent -> nothing.   2 (!exists): absent -> insert; present -> nothing
  const bool lru_like = sp.strategy == TFRA_EVICT_LRU || sp.strategy == TFRA_EVICT_EPOCHLRU;
  const u64 cmp = sp.strategy == TFRA_EVICT_EPOCHLFU ? ((sp.epoch << 32) | in_score) : in_score;
  i64 row = -1;
  u64 word = 0;
  bool is_new = false, evicted = false, side = false;
  if (hinted) {
    i64 old = 0;
    if (sub == 0) old = (i64)atomicCAS((u64*)key_word(v, (u64)hint_word), (u64)key, (u64)LOCKED_KEY);
    old = shfl_i64(old, gshift);
    if (old == key) { word = hint_word; row = (i64)((word >> 4) * SLOTS + (word & 15)); }
  }
  for (int attempt = 0; acc == 1 && attempt < 64 && row < 0; ++attempt) {   // accumulate: find the key (never claim a slot) and lock it
    const i64 r = probe_find<true>(v, key, sub, gshift);
    if (r < 0) return;                                   // absent & exists: dropped
    if (r >= (i64)(v.nb * SLOTS)) { row = r; side = true; break; }
    u64 rb;
    unsigned rs;
    split_row((u64)r, rb, rs);
    const u64 wd = rb * 16 + rs;
    i64 old = 0;
    if (sub == 0) old = (i64)atomicCAS((u64*)key_word(v, wd), (u64)key, (u64)LOCKED_KEY);
    old = shfl_i64(old, gshift);
    if (old == key) { row = r; word = wd; }              // else: an evictor of this pass took the slot; look again
  }
  for (int attempt = 0; acc != 1 && attempt < 64 && row < 0; ++attempt) {
    // This pass is one wave-lifetime of dependent round trips (~1.2 us each): both home buckets' key AND score lines
    // travel together up front (first attempt) instead of b0 -> b1 -> score lines one after the other.
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    const u64 b1 = bucket1(h, b0, v.nb);
    const bool pre = attempt == 0 && has_scores(v) && sp.bounded != 0;
    i64 kk2[2], sc2[2] = {0, 0};
    kk2[0] = load_key_coherent(key_line(v, b0) + sub);
    kk2[1] = pre ? load_key_coherent(key_line(v, b1) + sub) : 0;
    if (pre) {
      sc2[0] = (i64)__hip_atomic_load(score_line(v, b0) + sub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sc2[1] = (i64)__hip_atomic_load(score_line(v, b1) + sub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      keep_live(kk2[0], kk2[1], sc2[0], sc2[1]);
    }
    bool claimed = false;
    i64 r = locate_or_claim_from(v, key, h, b0, kk2[0], sub, gshift, claimed, sp.bounded, pre ? &kk2[1] : nullptr);
    if (r == NEED_EVICT) {
      bool ce = false;
      u64 wd = 0;
      i64 vk = EMPTY_KEY;
      r = evict_and_lock(v, key, cmp, lru_like, sub, gshift, &wd, ce, pre ? kk2 : nullptr, pre ? sc2 : nullptr, &vk, given_back, n_given_back);
      if (r == -1) break;                        // not admitted (its score is below every resident one): dropped
      if (r == -3) { failed += (sub == 0); break; }
      row = r; word = wd; is_new = true; evicted = !ce;
      if (evicted && evicted_key) *evicted_key = vk;
      fresh += (ce && sub == 0);
      break;
    }
    if (r < 0) { failed += (sub == 0); break; }
    if (acc == 2 && !claimed) return;                    // present & !exists: dropped (nothing was claimed or locked)
    fresh += (claimed && sub == 0);
    is_new = is_new || claimed;
    if (r >= (i64)(v.nb * SLOTS)) { row = r; side = true; break; }   // sentinel keys live in the side rows: nothing evicts there
    u64 rb;
    unsigned rs;
    split_row((u64)r, rb, rs);
    const u64 wd = rb * 16 + rs;
    i64 old = 0;
    if (sub == 0) old = (i64)atomicCAS((u64*)key_word(v, wd), (u64)key, (u64)LOCKED_KEY);
    old = shfl_i64(old, gshift);
    if (old == key) { row = r; word = wd; }   // else: an evictor of this pass took the slot; look again
  }
  if (row < 0) return;
  unsigned char* pr = row_ptr(v, row);
  if (acc == 1 && G == 16) {
    const unsigned char* dl = vals + (size_t)last * v.field_bytes;
    for (unsigned off = sub * 16; off < v.field_bytes; off += 256)
      store_wt16(pr + off, add16_dt(*reinterpret_cast<const uint4*>(pr + off), *reinterpret_cast<const uint4*>(dl + off), acc_dt));
  } else copy_bytes16_wt<G>(pr, vals + (size_t)last * v.field_bytes, v.field_bytes, sub);
  if (is_new) {
    for (unsigned f = 1; f < v.n_fields; ++f) {   // slot fields of the new row start at aux_init
      const unsigned pat = ai.pattern[(f - 1) & 3];
      unsigned char* q = pr + f * v.field_bytes;
      if ((v.field_bytes & 3) == 0)
        for (unsigned off = sub * 4; off < v.field_bytes; off += 64)
          __hip_atomic_store(reinterpret_cast<unsigned*>(q + off), pat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        for (unsigned off = sub; off < v.field_bytes; off += 16)
          __hip_atomic_store(q + off, (unsigned char)(pat >> (8 * (off % ai.elem_bytes))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (side) return;
  if (evicted && sub == 0) store_wt8(score_word(v, word), 0);   // the slot starts a new life
  update_score<true>(v, row, is_new, sp.strategy, in_score, sp.epoch, sub);
  publish_key(v, word, key, sub);
}

// A left-over key of the ownership pass, self-contained: the remainder pass needs nothing of the plan.
struct OwnItem {          // 32 B, written as two 16-B stores
  i64 key;
  unsigned last;          // batch position of the key's value row
  unsigned g;             // index of the key in the launch (its dflag byte)
  u64 ins;                // input score
  unsigned hinted, word;  // hinted != 0: the pass saw the key in slot `word` (bucket * 16 + slot) and did not write it
};
// Counters of one use by the ownership write-back (two sets alternate, the last kernel of use k zeroes the set of
// use k+1: nothing of use k-1 is still running by stream order).
struct OwnCtrs { unsigned n_a, spare[3]; };
static_assert(2 * sizeof(OwnCtrs) == PC_OWN_CTRS_WORDS * sizeof(unsigned), "the two sets are words [PC_OWN_CTRS, + PC_OWN_CTRS_WORDS) of a plan's d_counts block");

// Where the keys of a launch come from:
//   SRC_PLAN    the unique keys of a de-duplication plan (value row = the key's LAST occurrence in the batch)
//   SRC_DIRECT  a caller's array of UNIQUE keys, value row i belongs to key i (tfra_table_insert_or_assign with
//               TFRA_FLAG_UNIQUE_KEYS: the reference's Insert op, hkv_hashtable_op_gpu.cu.cc:253-290)
//   SRC_SET     the distinct keys of a SET plan (assign-only: last position and count per key, no positions list)
enum { SRC_PLAN = 0, SRC_DIRECT = 1, SRC_SET = 2, SRC_GIVEN = 3 };   // SRC_GIVEN: the caller hands key and value position (the overlapped step: from LDS)

struct OwnArgs {
  TableView v;
  const unsigned char* vals;
  const u64* scores;
  CsrKeys ks;              // SRC_PLAN
  const i64* keys;         // SRC_DIRECT
  unsigned nkeys;          // SRC_DIRECT
  const long long* d_nkeys;   // SRC_DIRECT, optional: the key count on the device (nkeys = the buffers' length then)
  AuxInitPod ai;
  ScoreP sp;
  uint8_t* dflag;          // one byte per key of the launch: 4 = left over.  All zero between launches: only left-over keys
                           // are flagged, and whoever takes a left-over key clears its flag
  unsigned* tags;
  OwnItem* items;          // [item_cap] left-over list of the launch
  unsigned item_cap;
  const uint8_t* exists;   // ACC (insert_or_accum of unique keys, SRC_DIRECT): the caller's exists flag per key
  int acc_dt;              // ACC: tfra_dtype of the rows
  SetProbe own_set;        // HF outside the step launch (SRC_SET): the launch's own SET plan, as something to probe
  unsigned* stats_host;    // pinned (Table::own_stats_host) or null: where the remainder kernel leaves the pass's sample
};
// (OwnArgs stays a read-only kernel argument: a private, modified copy would live in scratch memory — its aux_init
// pattern is indexed dynamically — and every field access of the hot loop would become a scratch load.)
struct OwnFlags { bool with_scores, spec, lru, lru_like; };

template <bool SIMPLE>
__device__ __forceinline__ OwnFlags own_setup(const OwnArgs& a) {
  OwnFlags fl;
  fl.with_scores = SIMPLE || has_scores(a.v);
  const bool dense = a.sp.bounded > 1 || (a.sp.bounded == 1 && *a.v.dense_flag);
  fl.spec = fl.with_scores && dense;   // an eviction is likely: the score lines travel with the key lines
  fl.lru = SIMPLE || a.sp.strategy == TFRA_EVICT_LRU;
  fl.lru_like = fl.lru || a.sp.strategy == TFRA_EVICT_EPOCHLRU;
  return fl;
}

// 16-lane minimum of (score, index) pairs with DPP row rotations (row_ror 8, 4, 2, 1: every lane ends up with the row's
// minimum; ~8 cycles per move instead of an LDS round trip per __shfl_xor — the four dependent rounds of the victim choice
// were a fifth of the 4 us a wave spends deciding)
__device__ __forceinline__ unsigned dpp_ror(unsigned x, int n) {
  switch (n) {
    case 8: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false);
    case 4: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xf, 0xf, false);
    case 2: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x122, 0xf, 0xf, false);
    default: return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x121, 0xf, 0xf, false);
  }
}
// Victim choice among the 30 slots of (b0, b1), as select_victim_merged (tfra_device.h): minimum score, the lower index
// (b0's slots before b1's) on ties, EMPTY counts as score 0, LOCKED slots are not candidates.
__device__ __forceinline__ void select_victim_dpp(u64 b0, u64 b1, const i64 (&kk2)[2], const i64 (&sc2)[2], int sub, int gshift,
                                                  u64& best_score, u64& best_word) {
  u64 s0 = (u64)sc2[0], s1 = (u64)sc2[1];
  if (kk2[0] == EMPTY_KEY) s0 = 0;
  if (kk2[1] == EMPTY_KEY) s1 = 0;
  if (sub >= SLOTS || kk2[0] == LOCKED_KEY) s0 = ~0ULL;
  if (sub >= SLOTS || kk2[1] == LOCKED_KEY) s1 = ~0ULL;
  u64 my = s0;
  unsigned idx = (unsigned)sub;
  if (s1 < s0) { my = s1; idx = 16u + (unsigned)sub; }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const u64 os = ((u64)dpp_ror((unsigned)(my >> 32), o) << 32) | dpp_ror((unsigned)my, o);
    const unsigned oi = dpp_ror(idx, o);
    if (os < my || (os == my && oi < idx)) { my = os; idx = oi; }
  }
  best_score = my;
  best_word = (idx >= 16u ? b1 : b0) * 16 + (idx & 15u);
}

// keep_live over U in-flight values (U = 2 or 4)
template <int U, typename T>
__device__ __forceinline__ void keep_live_u(T (&x)[U]) {
  if (U == 4) keep_live(x[0], x[1], x[2], x[3]);
  else keep_live(x[0], x[U - 1], x[0], x[U - 1]);
}
template <int U, typename T>
__device__ __forceinline__ void keep_live_u2(T (&x)[U][2], int k) {
  if (U == 4) keep_live(x[0][k], x[1][k], x[2][k], x[3][k]);
  else keep_live(x[0][k], x[U - 1][k], x[0][k], x[U - 1][k]);
}

// One batch of 16 keys of one wave.  What is scalar per key — the key word, its hash, the two ownership claims, the plan
// record (count, last position), the input score — is done ONE LANE PER KEY (lane j of every group holds key j; group 0
// issues the claims): one instruction stream for 16 keys.  What needs a whole line — the four bucket lines, the ballots,
// the victim choice, the row copy — is done one 16-lane group per key, 4 keys per group in flight (the scalar results
// reach the group by shuffle).  SIMPLE: the common shape — rows without optimizer slots, LRU scores, no caller scores —
// with everything else compiled out.
// ORDER (round 3, from the phase timings above): the clock is read first (s_memrealtime is slow); every cross-lane
// broadcast is issued before the first use of any; the claims are issued BEHIND the line loads and consumed LAST — memory
// returns in order, so a claim issued first would hold back the lines, and consumed first it would stall the decisions,
// which do not need it.
// gj = the lane's key: index into the plan's dense keys / the caller's key array (clamped to a valid index; `valid` says
// whether the lane's key is real).
// U: keys per 16-lane group in flight (the wave's batch is 4 U keys: lanes 0 .. 4U-1 of every group hold them).  2 for up
// to a batch's worth of keys (22.7 K keys are 1420 waves of 16 keys on 1024 SIMDs: the 4 us of dependent cross-lane work
// per wave halve, the waves double and still fit in one round), 4 beyond.
// CF (the overlapped step, tfra_step_impl.h): the lookup of the NEXT batch runs beside this pass and reads the table rows of every key
// that is not in this batch — an entry this pass is about to EVICT must not be one of them: `cf` = the next batch's plan; a victim
// that is in it defers the new key to the remainder pass (which runs after that lookup and corrects its output).
// ACC (SRC_DIRECT, 16-B granules): the reference's insert_or_accum of unique keys (accumrase_fn, cuckoohash_map.hh:619-633;
// HkvHashTableOfTensorsGpu::Accum, K/hkv_hashtable_op_gpu.cu.cc:292-335) instead of an assign — a.exists[i] set: the key is
// expected in the table, present => row += value row (one add per element), absent => dropped; not set: absent => insert,
// present => dropped.  A dropped key writes nothing, whatever its claims say (the keys of a call are unique: any order of
// them is a valid serial order).
template <int G, bool SIMPLE, int SRC, int U, bool CF = false, bool ACC = false, bool HF = false>
__device__ __forceinline__ void own_batch16(const OwnArgs& a, const OwnFlags fl, unsigned gj, bool valid, unsigned gen, unsigned* slow_ctr,
                                            int lane, int& fresh, const SetProbe* cf = nullptr, unsigned* cf_stat = nullptr,
                                            i64 kgiven = 0, unsigned lastgiven = 0, const SetProbe* own_plan = nullptr, int* not_hits = nullptr) {
  constexpr bool hf = HF;   // (CF && HF: the overlapped step's launch; HF alone: upsert_own_kernel over a SET plan, victims checked against that plan)
  const u64* const scores = SIMPLE ? nullptr : a.scores;
  const TableView& v = a.v;
  const CsrKeys& ks = a.ks;
  const int sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const u64 now = fl.lru_like ? (u64)wall_clock64() : 0;   // one clock read for the 16 keys (LRU scores tie within a wave)
  // ---- one lane per key ------------------------------------------------------------------------------------
  i64 kreg;
  unsigned kmreg = 0, lastreg = gj;
  u64 insreg = 1;
  if (SRC == SRC_PLAN) { kreg = ks.dkeys[gj]; kmreg = ks.keymap[gj]; }
  else if (SRC == SRC_SET) { kreg = ks.ukeys[gj]; kmreg = ks.uslot[gj]; }
  else if (SRC == SRC_GIVEN) { kreg = kgiven; lastreg = lastgiven; }
  else kreg = a.keys[gj];
  const unsigned exreg = ACC ? (unsigned)a.exists[gj] : 0u;
  u64 hreg;
  const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
  const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
  const bool reserved = is_reserved_key(kreg);   // sentinel keys live in the side rows: the general path
  // ---- one group per key: every broadcast first, then the lines of 4 keys in flight -------------------------
  i64 key[U], kk[U][2], sc[U][2];
  unsigned b0[U], b1[U], gk[U];
  bool on[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * 4 + grp;
    key[u] = shfl_i64(kreg, j);
    b0[u] = (unsigned)__shfl((int)b0reg, j);
    b1[u] = (unsigned)__shfl((int)b1reg, j);
    gk[u] = (unsigned)__shfl((int)gj, j);
    on[u] = __shfl((int)(valid && !reserved), j) != 0;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    // plain loads: everything written before this launch is visible, and nobody else writes a bucket this key owns
    kk[u][0] = key_line(v, b0[u])[sub];
    kk[u][1] = key_line(v, b1[u])[sub];
    // (HF, the step launch: 96 % of the keys are hits, which write their score word and never read a score line — the lines are fetched
    // below, and only by the waves that hold a key in need of a victim: 5.8 MB less random reads per launch on the metric's stream)
    sc[u][0] = (fl.spec && !hf) ? (i64)score_line(v, b0[u])[sub] : 0;
    sc[u][1] = (fl.spec && !hf) ? (i64)score_line(v, b1[u])[sub] : 0;
  }
  // ---- per key again, while the lines travel: count and last position from the plan record, input score ---
  if (SRC == SRC_PLAN) {
    const bool hot = (kmreg & KM_MANY) != 0;
    const unsigned* rec = (hot ? ks.hrec : ks.crec) + (size_t)(kmreg & ~KM_MANY) * REC_WORDS;
    const uint2 cl = *reinterpret_cast<const uint2*>(rec + 2);   // (count, last position of a key with few occurrences)
    const unsigned cnt = cl.x;
    lastreg = cl.y;
    if (hot) lastreg = ks.hent[rec[5]];                          // many: where it is stored
    lastreg &= E_POS;
    const u64 in_one = scores ? scores[lastreg] : 1;
    insreg = a.sp.strategy == TFRA_EVICT_LFU ? (scores ? in_one : (u64)cnt) : in_one;
  } else if (SRC == SRC_SET) {
    const uint2 pc = set_pc(ks.sent + kmreg);   // (last position + 1, occurrences) of the key's slot in the plan's table
    lastreg = pc.x - 1;
    const u64 in_one = scores ? scores[lastreg] : 1;
    insreg = a.sp.strategy == TFRA_EVICT_LFU ? (scores ? in_one : (u64)pc.y) : in_one;
  } else if (SRC != SRC_GIVEN) {
    insreg = scores ? scores[lastreg] : 1;
  }
  // the claims, behind the loads in program order (a clamped duplicate must not claim: it would lock out the real key)
  unsigned c0 = 0, c1 = 0;
  if (!hf && grp == 0 && valid && !reserved) {
    c0 = atomicExch(a.tags + b0reg, gen);
    c1 = atomicExch(a.tags + b1reg, gen);
  }
  keep_live_u2<U>(kk, 0);
  keep_live_u2<U>(kk, 1);
  if (fl.spec && !hf) {
    keep_live_u2<U>(sc, 0);
    keep_live_u2<U>(sc, 1);
  }
  // ---- what each key would do, from its lines alone (the claims are still travelling) -----------------------
  u64 word[U], in_s[U];
  int act[U];   // 0 nothing to write, 1 assign (hit), 2 new key in a free slot, 3 new key over an evicted entry
  int why[U];   // 0 handled, 1 lost a claim, 2 cannot be placed within the home buckets: the locked protocol
  bool flag_b0[U];   // the key goes to b1 although b0 never overflowed before: finds must go on to b1
  unsigned bxc[U];   // bucket beyond the home buckets the key was found in (it must be claimed too); ~0: none
  bool ex[U];        // ACC: the caller's exists flag
  bool need_v[U], ovf0_u[U];   // HF: the key needs a victim (score lines fetched below); b0's overflow flag as the decision saw it
  auto choose_victim = [&](int u, bool ovf0) {
    u64 best_score, best_word;
    select_victim_dpp(b0[u], b1[u], kk[u], sc[u], sub, gshift, best_score, best_word);
    const u64 cmp = a.sp.strategy == TFRA_EVICT_EPOCHLFU ? ((a.sp.epoch << 32) | in_s[u]) : in_s[u];
    if (fl.lru_like || cmp >= best_score) {   // else: not admitted, dropped like HKV does
      word[u] = best_word;
      act[u] = 3;
      flag_b0[u] = !ovf0 && (best_word >> 4) == b1[u];
      if (CF || HF) {
        const int vsrc = gshift + (int)(best_word & 15u);
        const i64 ka = shfl_i64(kk[u][0], vsrc), kb = shfl_i64(kk[u][1], vsrc);
        const i64 vk = (best_word >> 4) == (u64)b1[u] ? kb : ka;
        // CF: the next lookup wants it; HF: nor may it be a key of THIS batch — those are written without a claim, see below
        bool wanted = false;
        if (vk != EMPTY_KEY) {
          if (CF && HF) wanted = set_contains_either_group(*cf, *own_plan, vk, sub, gshift);
          else if (CF) wanted = set_contains_group(*cf, vk, sub, gshift);
          else wanted = own_plan ? set_contains_group(*own_plan, vk, sub, gshift) : true;   // (no plan to ask: defer — launch_own never picks HF then)
        }
        if (wanted) {   // deferred to the remainder
          act[u] = 0; why[u] = 3;
          if (cf_stat && sub == 0) atomicAdd(cf_stat, 1u);
        }
      }
    }
  };
#pragma unroll
  for (int u = 0; u < U; ++u) {
    need_v[u] = false; ovf0_u[u] = false;
    ex[u] = ACC && __shfl((int)exreg, u * 4 + grp) != 0;
    in_s[u] = 1;
    if (!fl.lru_like) in_s[u] = (u64)shfl_i64((i64)insreg, u * 4 + grp);   // (LRU-type scores ignore the input score)
    act[u] = 0; why[u] = 0; word[u] = 0; flag_b0[u] = false; bxc[u] = ~0u;
    if (!on[u]) continue;
    const unsigned hit0 = (unsigned)(__ballot(sub < SLOTS && kk[u][0] == key[u]) >> gshift) & 0x7fffu;
    const unsigned hit1 = (unsigned)(__ballot(sub < SLOTS && kk[u][1] == key[u]) >> gshift) & 0x7fffu;
    const unsigned emp0 = (unsigned)(__ballot(sub < SLOTS && kk[u][0] == EMPTY_KEY) >> gshift) & 0x7fffu;
    const unsigned emp1 = (unsigned)(__ballot(sub < SLOTS && kk[u][1] == EMPTY_KEY) >> gshift) & 0x7fffu;
    const bool ovf0 = ((__ballot(sub == 15 && ((u64)kk[u][0] & META_OVF0)) >> gshift) & 0xffffu) != 0;
    const bool ovf1 = ((__ballot(sub == 15 && ((u64)kk[u][1] & META_OVF1)) >> gshift) & 0xffffu) != 0;
    if (hit0) { word[u] = (u64)b0[u] * 16 + (__ffs(hit0) - 1); act[u] = 1; }
    else if (hit1) { word[u] = (u64)b1[u] * 16 + (__ffs(hit1) - 1); act[u] = 1; }
    else {
      bool absent = !(ovf0 && ovf1);   // the flags end the search at b0 / b1
      if (!absent) {
        // The key may live further along (placed while the table still walked): follow the flags with READS.  Found in
        // bucket bx: it claims bx too — every key that could evict from bx has bx as a home bucket and claimed it at its
        // start, so the exchange tells who goes first.
        unsigned bx = b1[u];
#pragma unroll 1
        for (int stepn = 0; stepn < 8 && !absent && !act[u] && !why[u]; ++stepn) {
          bx = bx + 1 == (unsigned)v.nb ? 0u : bx + 1;
          const i64 kx = load_key_coherent(key_line(v, bx) + sub);
          const unsigned hitx = (unsigned)(__ballot(sub < SLOTS && kx == key[u]) >> gshift) & 0x7fffu;
          if (hitx) { word[u] = (u64)bx * 16 + (__ffs(hitx) - 1); act[u] = 1; if (bx != b0[u] && bx != b1[u]) bxc[u] = bx; }
          else if (!((__ballot(sub == 15 && ((u64)kx & META_OVF1)) >> gshift) & 0xffffu)) absent = true;
          else if (stepn == 7) why[u] = 2;   // a long chain (an unbounded table): the general path
        }
      }
      if (absent && !(ACC && ex[u])) {   // not in the table (ACC: absent & exists is dropped)
        if (emp0) { word[u] = (u64)b0[u] * 16 + (__ffs(emp0) - 1); act[u] = 2; }   // first empty slot in probe order
        else if (emp1) { word[u] = (u64)b1[u] * 16 + (__ffs(emp1) - 1); act[u] = 2; flag_b0[u] = !ovf0; }
        else if (fl.spec) {
          // both home buckets full on a table that no longer walks: replace the minimum-score entry of the 30 slots
          if (hf) need_v[u] = true;                   // (its score lines are not here yet: below)
          else choose_victim(u, ovf0);
          ovf0_u[u] = ovf0;
        } else why[u] = 2;   // a table that still walks (not at capacity / unbounded): placed further along by the general path
      }
    }
  }
  if (hf && fl.spec) {
    bool any_v = false;
#pragma unroll
    for (int u = 0; u < U; ++u) any_v = any_v || need_v[u];
    if (__ballot(any_v)) {   // (wave-uniform) one more round trip, for the waves that hold a key in need of a victim
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sc[u][0] = (i64)score_line(v, b0[u])[sub];
        sc[u][1] = (i64)score_line(v, b1[u])[sub];
      }
      keep_live_u2<U>(sc, 0);
      keep_live_u2<U>(sc, 1);
#pragma unroll
      for (int u = 0; u < U; ++u) if (need_v[u]) choose_victim(u, ovf0_u[u]);
    }
  }
  // ---- now the claims -------------------------------------------------------------------------------------------
  const unsigned lostreg = reserved ? 2u : ((c0 == gen || c1 == gen) ? 1u : 0u);   // (group 0's lanes)
  // HF (the overlapped step): a HIT needs no claim.  It writes its own row and score word and nothing else of the bucket; the only
  // writer that could take its slot away is an eviction, and an eviction never takes a key of this batch (the victim check above
  // looks the victim up in the batch's own plan too).  Only the keys that CHANGE a bucket — a new key into a free slot or over a
  // victim — claim their two home buckets, now, behind the decision: 96 % of a Zipf batch's keys issue no atomic at all, two keys of
  // a batch sharing a home bucket no longer collide unless both are new, and the item list is empty in nearly every step.
  bool lost_hf[U];
#pragma unroll
  for (int u = 0; u < U; ++u) lost_hf[u] = false;
  if (hf) {
    bool any = false;
#pragma unroll
    for (int u = 0; u < U; ++u) { lost_hf[u] = false; any = any || act[u] >= 2; }
    if (__ballot(any)) {   // (wave-uniform: one more round trip for the waves that hold a new key)
      unsigned cx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        cx[u] = 0;
        if (act[u] >= 2 && sub < 2) cx[u] = atomicExch(a.tags + (sub == 0 ? b0[u] : b1[u]), gen) == gen ? 1u : 0u;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) lost_hf[u] = ((__ballot(cx[u] != 0) >> gshift) & 0xffffu) != 0;
    }
  }
  unsigned last[U], hint[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * 4 + grp;
    last[u] = (unsigned)__shfl((int)lastreg, j);
    const bool real = __shfl((int)valid, j) != 0;
    const int lost = hf ? ((real && !on[u]) ? 2 : (lost_hf[u] ? 1 : 0)) : __shfl((int)lostreg, j);   // (without HF: lane j of group 0 made the claims)
    hint[u] = 0;
    if (lost) {
      if (lost == 1 && act[u] == 1 && (word[u] >> 32) == 0) hint[u] = 1;   // found, not written: the remainder pass locks this very slot
      act[u] = 0; why[u] = lost;
    }
    if (!hf && bxc[u] != ~0u && act[u]) {   // (rare) found beyond its home buckets: that bucket's claim
      unsigned cx = 0;
      if (sub == 0) cx = atomicExch(a.tags + bxc[u], gen) == gen ? 1u : 0u;
      if (__shfl((int)cx, gshift)) { act[u] = 0; why[u] = 1; }
    }
    if (!real) { act[u] = 0; why[u] = 0; }
    if (ACC) {
      if (act[u] == 1 && !ex[u]) act[u] = 0;                                   // present & !exists: dropped
      if (why[u] == 1 && hint[u] && !ex[u]) { why[u] = 0; hint[u] = 0; }        // (the same, seen without the claim)
      if (why[u] == 1 && !hint[u] && ex[u] && bxc[u] == ~0u) { }               // lost its claim, not seen: the remainder looks again
      if (ex[u]) hint[u] |= 2u;                                                // the item carries the flag
    }
    if (act[u] && flag_b0[u] && sub == 15) atomicOr((u64*)(key_line(v, b0[u]) + 15), META_OVF0);   // finds go on to b1
    if (sub == 0 && why[u]) { if (CF) __hip_atomic_store(a.dflag + gk[u], (uint8_t)4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else a.dflag[gk[u]] = 4; }
    fresh += (act[u] == 2 && sub == 0);
    if (not_hits) *not_hits += (real && act[u] != 1 && sub == 0);   // (a new key, an eviction, a key handed to the remainder)
  }
  {   // left-over keys of the wave -> the list: one atomic add for all of them
    u64 sm[U];
    unsigned nslow = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) { sm[u] = __ballot(why[u] != 0 && sub == 0); nslow += (unsigned)__popcll(sm[u]); }
    if (nslow) {
      unsigned at = 0;
      if (lane == 0) at = atomicAdd(slow_ctr, nslow);
      at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (why[u] != 0 && sub < 2) {
          const unsigned pos = at + (unsigned)__popcll(sm[u] & ((1ULL << gshift) - 1));
          if (pos < a.item_cap) {
            uint4 w;
            if (sub == 0) w = make_uint4((unsigned)(u64)key[u], (unsigned)((u64)key[u] >> 32), last[u], gk[u]);
            else w = make_uint4((unsigned)in_s[u], (unsigned)(in_s[u] >> 32), hint[u], (unsigned)word[u]);
            if (CF) store_wt16(reinterpret_cast<unsigned char*>(a.items + pos) + sub * 16, w);   // (read by the tail role of the same launch)
            else *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(a.items + pos) + sub * 16) = w;
          }
        }
        at += (unsigned)__popcll(sm[u]);
      }
    }
  }
  // value rows of the 4 keys: loads together (always from a valid address), stores for the keys that write
  typedef typename Granule<G>::T T;
  unsigned char* dst[U];
#pragma unroll
  for (int u = 0; u < U; ++u) dst[u] = row_at(v, word[u] >> 4, (unsigned)word[u] & 15u);
  for (unsigned off = sub * G; off < v.field_bytes; off += 16 * G) {
    T tmp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) tmp[u] = *reinterpret_cast<const T*>(a.vals + (u64)last[u] * (u64)v.field_bytes + off);
    keep_live_u<U>(tmp);
    if (ACC && G == 16) {   // accumulate: the rows themselves travel with the deltas (a key that only inserts adds nothing)
      T cur[U];
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = *reinterpret_cast<const T*>(dst[u] + off);
      keep_live_u<U>(cur);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (act[u] == 1) *reinterpret_cast<uint4*>(&tmp[u]) = add16_dt(*reinterpret_cast<uint4*>(&cur[u]), *reinterpret_cast<uint4*>(&tmp[u]), a.acc_dt);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!act[u]) continue;
      // write-through: the rows leave L2 during the kernel instead of at the boundary to the next one
      if (G == 16) store_wt16(dst[u] + off, *reinterpret_cast<uint4*>(&tmp[u]));
      else __hip_atomic_store(reinterpret_cast<T*>(dst[u] + off), tmp[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!act[u]) continue;
    if (act[u] >= 2) {
      if (!SIMPLE && v.n_fields > 1) {
        for (unsigned f = 1; f < v.n_fields; ++f) {   // slot fields of a brand-new row start at aux_init
          const unsigned pat = a.ai.pattern[(f - 1) & 3];
          unsigned char* q = dst[u] + f * v.field_bytes;
          if ((v.field_bytes & 3) == 0)
            for (unsigned off = sub * 4; off < v.field_bytes; off += 64)
              __hip_atomic_store(reinterpret_cast<unsigned*>(q + off), pat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else
            for (unsigned off = sub; off < v.field_bytes; off += 16)
              __hip_atomic_store(q + off, (unsigned char)(pat >> (8 * (off % a.ai.elem_bytes))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (sub == 0) { if (CF) store_wt8(key_word(v, word[u]), (u64)key[u]); else *key_word(v, word[u]) = key[u]; }   // owned bucket: a plain store (CF: write-through, the
                                                                                                                   // left-over keys follow in the same launch)
    }
    if (!fl.with_scores) continue;
    if (fl.lru) { if (sub == 0) { if (CF) store_wt8(score_word(v, word[u]), now); else *score_word(v, word[u]) = now; } }
    else if (act[u] == 3 && a.sp.strategy == TFRA_EVICT_LFU) { if (sub == 0) store_wt8(score_word(v, word[u]), in_s[u]); }   // the slot starts a new life
    else update_score<true>(v, (i64)((word[u] >> 4) * SLOTS + (word[u] & 15)), act[u] >= 2, a.sp.strategy, in_s[u], a.sp.epoch, sub);
  }
}

}  // namespace
