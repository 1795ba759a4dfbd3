// The OVERLAPPED STEP: lookup of batch i+1 in the same launch as the write-back of batch i — its kernel (StepArgs, the roles,
// the step_k_* instances).  The driver that launches it is tfra_step.hip; the ownership pass it runs is tfra_own_device.h's,
// the plans it probes and builds are tfra_plan_device.h's.
//
// Reference semantics kept (hkv_hashtable_op_gpu.cu.cc:192-213,256-267: Insert exclusive, Find shared => lookup i+1 sees
// update i; lookup_table_op_hkv.h:522-537 upsert, :719-756 get with default fill): the results are those of
//     lookup(ids_0); insert_or_assign(ids_0, values_0); lookup(ids_1); insert_or_assign(ids_1, values_1); ...
// executed one after the other.
//
// Why it may overlap.  What keeps lookup(i+1) behind write-back(i) is the keys the two share — and for exactly those the row
// the lookup must return is known without the table: values_i[last position of the key in batch i], which the SET plan of
// batch i (an open-addressing table key -> last position, built one batch ahead) gives in one probe.  So:
//   * lookup(i+1) probes plan(i) for every id; a hit is served from values_i (STORE-TO-LOAD FORWARDING), everything else
//     from the table.  Keys that are NOT in batch i keep their row through write-back(i) — unless write-back(i) EVICTS them;
//   * write-back(i) therefore probes plan(i+1) for every victim it is about to replace: a victim the next lookup looks for
//     is not evicted in the pass; the new key goes to the remainder pass, which runs AFTER the lookup, evicts then, and
//     rewrites the lookup's output rows of that victim with the default row (what a lookup after the eviction returns).
//     (~160 evictions per step on the metric's configuration, practically none of them of a key of the next batch.)
//   * everything else the pass does to a bucket (rows of keys of batch i, free-slot inserts, flags) is invisible to a lookup of
//     OTHER keys: slots are 8-byte words, flags are monotone.
// Forwarding needs every key of batch i to END UP in the table (a key the table does not admit must read as absent):
// LRU-type scores on a bounded table at capacity — the metric's configuration.  Anything else takes the sequential fallback
// inside the same entry point.
//
// ONE launch per step, six roles by block index (block-uniform branches; grid order = dispatch order):
//   BUILD    one 2048-slot window of plan(i+2)'s table per block, in LDS, from the segments a SCATTER filled one launch ago
//   SCATTER  one tile of 1024 ids of batch i+3 per block: distinct (id, last position) pairs into per-(window, tile) segments
//            (a plan is built over two launches WITHOUT a global atomic; ids two batches ahead)
//   MAP      (round 5) 1024 positions of the NEXT lookup per block, probed in this batch's plan and sorted by where their row will
//            come from (forwarded / table): the next launch's lookup reads its entries instead of probing, whole waves of one kind
//   OWN      write-back(i): own_batch16 over slices of plan(i)'s table (~40 keys per block), victims checked against plan(i+1)
//   FIND     lookup(i+1) with forwarding from plan(i) / values_i, driven by the list the previous launch's MAP made
//   TAIL     the last 32 blocks: wait for the OWN blocks (a counter), take the keys the pass left over (lost claims, deferred
//            evictions) with the locked protocol, note every victim that batch i+1 looks up, and — if any — wait for the FIND
//            blocks and correct their output rows.  Nothing a TAIL block waits for waits for anything itself.
// One stream, no events, no host in the loop: the sequence is enqueued many steps ahead (tfra_table_steps_overlap).
// Measurements on the metric's configuration (10^9 slots, 131 072 Zipf-1.2 ids, 22.5 K distinct): round 4 31-33 us per launch
// (roles ALONE, TFRA_STEP_ABLATE: builders 9.6 us, lookup + builders 19.8, write-back + tail 23.0); round 5 21.3-21.5 us on average
// under rocprofv3 — the MAP role (31.0 -> 26.0 us on one box) and 448-slot write-back slices (26.2 -> 20.8): 12 K waves that wait on
// memory 75 % of their time, 92.4 MB of HBM traffic for 80.0 MB algorithmic; DESIGN.md sections 4.5 and 5.

#pragma once
#include <hip/hip_runtime.h>

#include "tfra_device.h"
#include "tfra_own_device.h"
#include "tfra_plan_device.h"

namespace {

struct StepArgs {
  OwnArgs own;                 // write-back of the PREVIOUS batch (its keys come from `fwd`, the previous batch's plan); own_blocks == 0: none pending
  OwnCtrs* ctr;                // the plan's left-over counters (the step counts in sync[1]; these belong to the sequential path)
  unsigned own_gen;
  unsigned* progress;          // pinned: [0] step
  unsigned progress_val;
  SetProbe fwd;                // the previous batch's plan: ids found here are served from own.vals
  SetProbe nxt;                // THIS batch's plan: victims found here are not evicted in the pass
  // lookup of this batch
  unsigned n;
  const i64* ids;
  unsigned char* out;
  uint8_t* exists;
  const unsigned char* defaults;
  int full;
  // BUILD role: the plan of the NEXT batch, one window of its table per block, from the segments a scatter filled one launch ago
  SetEnt* build_ent;           // the table (every slot is written)
  unsigned build_m2, build_tiles, build_blocks;
  const SetEnt* build_pairs; const unsigned* build_cnt; const SetEnt* build_ovf; const unsigned* build_ovf_cnt;
  unsigned* build_ucnt;        // [windows] distinct keys per window of the table being built (plain stores: no atomic on a hot word —
                               // 586 fire-and-forget adds from the write-back's blocks to ONE counter cost the launch 4 us)
  const unsigned* own_ucnt;    // the same array of the plan being written back (nullptr: not built by a step launch); block 0 sums it
  unsigned own_ucnt_n;         // into progress[1] (pinned): the host sizes later launches' slices from it
  // SCATTER role: the batch after next, one tile of 1024 ids per block -> per (window, tile) segments
  unsigned scat_n, scat_m2, scat_tiles, scat_blocks;
  const i64* scat_ids;
  SetEnt* scat_pairs; unsigned* scat_cnt; SetEnt* scat_ovf; unsigned* scat_ovf_cnt; unsigned* scat_ovf_cnt_next;   // (two overflow counters alternate: this scatter zeroes the next one's)
  // MAP role: the positions of the NEXT batch, sorted by where their row will come from — probed in `nxt` (THIS batch's plan, the
  // one the next lookup forwards from): entries {position, last position + 1 in this batch | 0, key}; per segment of 1024 positions
  // the table entries from the front, the forwarded ones from the back.  find_list != nullptr: the list a MAP role made of THIS batch one launch ago
  unsigned map_n, map_blocks;
  const i64* map_ids;
  uint4* map_out;
  const uint4* find_list;
  unsigned own_slice;          // plan slots per write-back block
  unsigned find_first;         // lookup blocks dispatched in FRONT of the write-back's (the list's table-bound chunks: the long chains start with the launch)
  unsigned own_blocks, find_blocks, tail_blocks;
  unsigned* sync;              // this launch's counters, one 128-byte line each: [0] write-back blocks done, [32 .. 32*8] lookup blocks done
                               // (8 shards), [32*9] tail blocks through their items; sync_next: the next launch's (two sets alternate).  [1] the
                               // write-back's left-over keys (item list length), [32*9+1] = patch_count: each read WITH the arrivals beside it
  unsigned* sync_next;
  unsigned* zero4;             // the left-over counters of the plan's NEXT use (armed by the tail)
  int ablate;                  // (tuning) roles that return at once: 1 builders, 2 write-back + tail, 4 lookup, 8 tail
  int serial_probe;            // the lookup reads the table's lines only for the ids the previous batch's plan does not hold
  unsigned* stat;              // [0] evictions the pass deferred, [1] victims the remainder noted, [2] output rows corrected
  u64* tbuf;                   // TIMING: [TIMING_SLOTS][TIMING_BLOCKS][2] block start / end stamps (nullptr otherwise)
  i64* patch_keys;             // tail: the launch's list of keys whose slot changed hands and which this batch looks up
  unsigned* patch_count;       // its length; patch_count_next: the next step's (two alternate)
  unsigned* patch_count_next;
};

// LDS of a block, whatever its role (24.6 KB): a 2048-slot table (scatter: the tile's ids; build: the window) or, for the
// write-back, the compacted keys of its slice of the plan
struct StepLds {
  i64 key[SET_WIN];
  unsigned pos[SET_WIN + 2];   // (+2: the two sentinel key values)
  unsigned cnt[256];           // scatter: pairs per window
  unsigned n;
};
// Plan slots per write-back block (StepArgs::own_slice; TFRA_STEP_OWN_SLICE overrides it for tuning, <= 768).  Rounds 3-4 used 288
// (~25 keys at 22.7 K keys in 2^18 slots: one round of the block's four waves; 911 blocks) — the write-back's blocks, dispatched in
// front of the lookup's, then took every wave slot of the chip for the first 6 us of the launch.  With the lookup's blocks short
// (MAP lists, below) the balance is elsewhere: 448 slots = 586 blocks of ~39 keys (two rounds) leave 300 slots to the lookup from
// the first microsecond, and the write-back itself ENDS EARLIER (16 us instead of 19: fewer waves contend for the same lines).
// Measured on the metric's configuration, one box: 288 -> 26.2 us per step, 384 -> 21.3, 448 -> 21.1, 512 -> 20.8 / 22.4 (two boxes),
// 576 -> 24.1, 768 -> 29.2.  The optimum follows the keys per block, not the slots: the driver sizes the slice for ~40 keys from the
// distinct-key count of an earlier batch (the tail leaves it in pinned memory), between 96 and 512 slots — a batch of all-distinct
// ids (m2 = 2 n: every second slot taken) gets 96-slot slices instead of 224 keys = seven rounds per block; configs[2]'s 78 K keys
// per batch 128 (measured there, per-step with 65 K evictions: 96 -> 72 us, 160 -> 76, 288 -> 66, 448 -> 88).
constexpr unsigned OWN_SLICE_DEFAULT = 448;

// ---- SCATTER role: setplan_kernel's LDS phase, then plain stores ------------------------------------------------------
// Equal ids of the tile meet in LDS (compare-and-swap on the key, max on position + 1); every distinct id then goes, with its
// last position in the tile, into the segment (window of its home slot, this tile): a position inside the segment from an LDS
// counter, a plain 16-byte store.  No global atomic (an id-heavy window — 32 distinct ids of ONE tile in ONE of the >= 128
// windows — spills into an overflow list with one).  The round-3 plan kernel put every distinct id of every tile into ONE global
// table with a compare-and-swap and a max: 100 K device-scope atomics per batch, the hot ids' slots taking one from every tile
// — inside the step's launch each such round trip took 7 us (queues at the hot slots) and the role 21 us, as long as lookup
// and write-back together.
__device__ __forceinline__ void scatter_role(const StepArgs& a, unsigned tile, StepLds& L) {
  const unsigned tid = threadIdx.x;
  const unsigned wins = a.scat_m2 >> SET_WIN_LOG2;
  for (unsigned i = tid; i < SET_WIN + 2; i += 256) { if (i < SET_WIN) L.key[i] = EMPTY_KEY; L.pos[i] = 0; }
  L.cnt[tid] = 0;
  if (tile == 0 && tid == 0) *a.scat_ovf_cnt_next = 0;
  i64 id[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned g = tile * 1024u + (unsigned)r * 256u + tid;
    id[r] = g < a.scat_n ? a.scat_ids[g] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned g = tile * 1024u + (unsigned)r * 256u + tid;
    if (g >= a.scat_n) continue;
    unsigned slot;
    if (is_reserved_key(id[r])) slot = SET_WIN + (unsigned)reserved_index(id[r]);
    else {
      slot = (unsigned)(fmix64((u64)id[r]) >> 41) & (SET_WIN - 1);
      for (;;) {
        const i64 was = (i64)atomicCAS(reinterpret_cast<unsigned long long*>(&L.key[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)id[r]);
        if (was == EMPTY_KEY || was == id[r]) break;
        slot = (slot + 1) & (SET_WIN - 1);
      }
    }
    atomicMax(&L.pos[slot], g + 1u);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < (int)(SET_WIN / 256); ++r) {
    const unsigned sl = tid + (unsigned)r * 256u;
    const unsigned p1 = L.pos[sl];
    if (!p1) continue;
    const i64 key = L.key[sl];
    const unsigned w = ((unsigned)(fmix64((u64)key) >> 20) & (a.scat_m2 - 1)) >> SET_WIN_LOG2;
    const unsigned at = atomicAdd(&L.cnt[w], 1u);
    const uint4 pair = make_uint4((unsigned)(u64)key, (unsigned)((u64)key >> 32), p1, 0u);
    if (at < SEG_CAP) *reinterpret_cast<uint4*>(a.scat_pairs + ((size_t)w * a.scat_tiles + tile) * SEG_CAP + at) = pair;
    else *reinterpret_cast<uint4*>(a.scat_ovf + atomicAdd(a.scat_ovf_cnt, 1u)) = pair;
  }
  if (tid < 2 && L.pos[SET_WIN + tid] != 0) {   // a sentinel key value occurred in this tile: window 0 carries it
    const i64 key = EMPTY_KEY + (i64)tid;
    const unsigned at = atomicAdd(&L.cnt[0], 1u);
    const uint4 pair = make_uint4((unsigned)(u64)key, (unsigned)((u64)key >> 32), L.pos[SET_WIN + tid], 0u);
    if (at < SEG_CAP) *reinterpret_cast<uint4*>(a.scat_pairs + ((size_t)0 * a.scat_tiles + tile) * SEG_CAP + at) = pair;
    else *reinterpret_cast<uint4*>(a.scat_ovf + atomicAdd(a.scat_ovf_cnt, 1u)) = pair;
  }
  __syncthreads();
  if (tid < wins) a.scat_cnt[(size_t)tid * a.scat_tiles + tile] = min(L.cnt[tid], SEG_CAP);
}

// ---- BUILD role: one window of the next batch's plan ---------------------------------------------------------------------
// Thread t takes the pairs tile t left for this window (a handful), inserts them into the window's image in LDS (linear probing
// inside the window, max on the position: the rule every prober follows, set_at) and the block writes the image out — all
// 2048 slots, so the table needs no emptying between its uses.  Two dependent round trips (counts, pairs), no atomics.
__device__ __forceinline__ void build_role(const StepArgs& a, unsigned win, StepLds& L) {
  const unsigned tid = threadIdx.x;
  for (unsigned i = tid; i < SET_WIN + 2; i += 256) { if (i < SET_WIN) L.key[i] = EMPTY_KEY; L.pos[i] = 0; }
  if (tid == 0) L.n = 0;
  const unsigned c = tid < a.build_tiles ? a.build_cnt[(size_t)win * a.build_tiles + tid] : 0u;
  const unsigned novf = *a.build_ovf_cnt;
  __syncthreads();
  auto insert = [&](i64 key, unsigned p1) {
    unsigned slot;
    if (is_reserved_key(key)) slot = SET_WIN + (unsigned)reserved_index(key);
    else {
      slot = ((unsigned)(fmix64((u64)key) >> 20) & (a.build_m2 - 1)) & (SET_WIN - 1);
      for (;;) {
        const i64 was = (i64)atomicCAS(reinterpret_cast<unsigned long long*>(&L.key[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)key);
        if (was == EMPTY_KEY || was == key) break;
        slot = (slot + 1) & (SET_WIN - 1);
      }
    }
    atomicMax(&L.pos[slot], p1);
  };
  const SetEnt* seg = a.build_pairs + ((size_t)win * a.build_tiles + tid) * SEG_CAP;
  for (unsigned j = 0; j < c; j += 4) {   // (c <= SEG_CAP; four pairs in flight)
    uint4 pr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) pr[q] = *reinterpret_cast<const uint4*>(seg + min(j + (unsigned)q, c - 1));
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j + (unsigned)q < c) insert((i64)(((u64)pr[q].y << 32) | pr[q].x), pr[q].z);
  }
  for (unsigned i = tid; i < novf; i += 256) {   // (an adversarial batch)
    const uint4 pr = *reinterpret_cast<const uint4*>(a.build_ovf + i);
    const i64 key = (i64)(((u64)pr.y << 32) | pr.x);
    const unsigned w = is_reserved_key(key) ? 0u : ((unsigned)(fmix64((u64)key) >> 20) & (a.build_m2 - 1)) >> SET_WIN_LOG2;
    if (w == win) insert(key, pr.z);
  }
  __syncthreads();
  SetEnt* out = a.build_ent + (size_t)win * SET_WIN;
  const unsigned wslots = a.build_m2 < SET_WIN ? a.build_m2 : SET_WIN;
  unsigned occ = 0;
  for (unsigned sl = tid; sl < wslots; sl += 256) {
    const i64 k = L.key[sl];
    const unsigned p1 = L.pos[sl];
    occ += p1 != 0;
    *reinterpret_cast<uint4*>(out + sl) = make_uint4((unsigned)(u64)k, (unsigned)((u64)k >> 32), p1, 0u);
  }
  if (a.build_ucnt) {   // distinct keys of this window (for the host's choice of the write-back's slice size, two launches from now)
    for (int off = 32; off > 0; off >>= 1) occ += (unsigned)__shfl_xor((int)occ, off);
    if ((tid & 63) == 0) atomicAdd(&L.n, occ);
    __syncthreads();
    if (tid == 0) a.build_ucnt[win] = L.n;
  }
  if (win == 0 && tid < 2) {   // the two sentinel slots behind the table: key word = "taken" marker
    const unsigned p1 = L.pos[SET_WIN + tid];
    *reinterpret_cast<uint4*>(a.build_ent + a.build_m2 + tid) = p1 ? make_uint4(1u, 0u, p1, 0u) : make_uint4(0u, 0x80000000u, 0u, 0u);
  }
}

// ---- FIND role: find_kernel<16, 4, WT, PF1> + forwarding -----------------------------------------------------------
// A wave takes KW = 4 U ids (U = 4: 16, U = 8: 32): lane j < KW — and its 64 / KW replicas — holds id j and hashes it; for the
// plan probe the replicas of an id read consecutive entries of its chain (one 16-B load per lane, all 64 lanes busy, no
// redundancy); the table probe is find_kernel's, one 16-lane group per id, U ids per group in flight.
// (Tried, U = 8: 32 ids per wave, twice the loads in flight in registers the write-back's roles need anyway — a lookup block then
// takes 14.6 us instead of 7.4 for twice the ids, the step 34.5 us instead of 31.9: what a wave waits for is served at a rate, not
// after a latency.  SQ counters of the launch: 12.8 K waves, 300 vector + 204 scalar instructions per wave, 77 % of the wave cycles
// parked on s_waitcnt, L2 hit ratio 24 % — plan, value rows and table lines of eight XCDs' worth of batch do not fit eight 4-MB L2s.)
template <int N, typename T>
__device__ __forceinline__ void keep_live_n(T (&x)[N]) {
  static_assert(N % 4 == 0, "keep_live_n: multiples of four");
#pragma unroll
  for (int q = 0; q < N; q += 4) keep_live(x[q], x[q + 1], x[q + 2], x[q + 3]);
}
template <int U>
__device__ __forceinline__ void find_fwd_role(const StepArgs& a, unsigned blk) {
  constexpr int KW = 4 * U, REP = 64 / KW;
  const TableView& v = a.own.v;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const int rep = lane / KW;                       // which of the id's replicas this lane is
  const unsigned wave = blk * 4u + (threadIdx.x >> 6);
  const unsigned base = wave * (unsigned)KW;
  if (base >= a.n) return;
  const unsigned last = a.n - 1;
  const i64 kreg = a.ids[min(base + (unsigned)(lane & (KW - 1)), last)];
  u64 hreg;
  const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
  const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
  const bool resv = is_reserved_key(kreg);
  const unsigned home = set_home(a.fwd, kreg, hreg);
  const unsigned wm = set_wmask(a.fwd.m2);
  const unsigned eidx = resv ? home + (unsigned)rep : set_at(home, (unsigned)rep, wm);
  uint4 e = *reinterpret_cast<const uint4*>(a.fwd.ent + eidx);
  i64 key[U], k0[U], k1[U];
  unsigned b0[U], b1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * 4 + grp;
    key[u] = shfl_i64(kreg, j);
    b0[u] = (unsigned)__shfl((int)b0reg, j);
    b1[u] = (unsigned)__shfl((int)b1reg, j);
  }
  keep_live(e.x, e.y, e.z, e.w);
  // the plan probe, per id: a match in any of its replicas' entries is the id; none and no EMPTY among them: go on (rare)
  const i64 ekey = (i64)(((u64)e.y << 32) | e.x);
  const bool match = resv ? (rep == 0 && ekey != EMPTY_KEY) : ekey == kreg;
  unsigned p1 = match ? e.z : 0u;
  unsigned stop = (ekey == EMPTY_KEY || resv) ? 1u : 0u;
#pragma unroll
  for (int o = KW; o < 64; o <<= 1) { p1 |= (unsigned)__shfl_xor((int)p1, o); stop |= (unsigned)__shfl_xor((int)stop, o); }
  if (!p1 && !stop) {
    for (unsigned t = REP; t <= wm; ++t) {
      const SetEnt* q = a.fwd.ent + set_at(home, t, wm);
      const i64 k = q->key;
      if (k == kreg) { p1 = q->pos1; break; }
      if (k == EMPTY_KEY) break;
    }
  }
  unsigned fwd_pos[U];
#pragma unroll
  for (int u = 0; u < U; ++u) fwd_pos[u] = (unsigned)__shfl((int)p1, u * 4 + grp);
  {
    // The table's lines BEHIND the plan probe, and only for the ids the plan does not hold: on a Zipf stream most positions of a
    // batch repeat ids of the batch before (85 % on the metric's configuration), and every line of a 273-GB table is a random,
    // TLB-missing access.  The loads stay unconditional (one wait for all of them): a forwarded id reads one hot line of the plan.
    // (Tried: the lines of every id in flight WITH the plan probe — one trip less, two random lines more per forwarded id: no gain.)
    const i64* hot = reinterpret_cast<const i64*>(a.fwd.ent);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      k0[u] = (fwd_pos[u] ? hot : key_line(v, b0[u]))[sub];
      k1[u] = (fwd_pos[u] ? hot : key_line(v, b1[u]))[sub];
    }
    keep_live_n<U>(k0);
    keep_live_n<U>(k1);
  }
  const unsigned char* src[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned fw = fwd_pos[u];
    const unsigned idx = min(base + (unsigned)(u * 4 + grp), last);
    i64 word = 0;
    if (!fw) word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift, &k1[u]);
    // (write-through like the rows: the tail's corrections come from another workgroup and must land BEHIND this store)
    if (a.exists && sub == 0) __hip_atomic_store(a.exists + idx, (uint8_t)(fw != 0 || word >= 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    src[u] = fw ? a.own.vals + (u64)(fw - 1u) * (u64)v.field_bytes
                : (word >= 0 ? word_row_ptr(v, (u64)word) : a.defaults + (a.full ? (u64)idx * (u64)v.field_bytes : 0));
  }
  for (unsigned off = sub * 16; off < v.field_bytes; off += 256) {
    uint4 tmp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) tmp[u] = *reinterpret_cast<const uint4*>(src[u] + off);
    keep_live_n<U>(tmp);
#pragma unroll
    for (int u = 0; u < U; ++u)
      store_wt16(a.out + (u64)min(base + (unsigned)(u * 4 + grp), last) * (u64)v.field_bytes + off, tmp[u]);
  }
}
// ---- MAP role (round 5): where will each position of the NEXT batch get its row from? -----------------------------------------
// The lookup's chain was ids -> plan entry -> table lines -> rows -> stores, and 85 % of a Zipf batch's positions stop at the plan
// entry (forwarded from the rows being written) — but a wave of 16 ids nearly always holds one that does not, so every wave went
// the whole way.  The plan the next lookup forwards from (this batch's) is complete when this launch starts and the next ids are
// announced: one launch AHEAD, off the lookup's chain, a block probes 1024 positions in it and writes them out as 16-byte entries
// {position, last position + 1 | 0, key} into ITS segment of the list — positions that need the table packed from the front of
// the segment, forwarded ones from its back: ranks by ballot and LDS, no atomic, no counter.  The next launch's lookup reads its
// entries with its first (coalesced) trip; all but one wave per segment are of one kind, and a wave of forwarded positions goes
// entry -> value rows -> stores: no hash, no plan probe, no table line.
// (First form: ONE list, packed from both ends with two returned atomics per block — 31.0 -> 26.8 us per step on one box, its MAP
// blocks 10 us long, most of it the atomics' round trip.)
constexpr unsigned MAP_SEG = 1024;
__device__ __forceinline__ void map_role(const StepArgs& a, unsigned tile, StepLds& L) {
  const unsigned tid = threadIdx.x;
  const int lane = tid & 63;
  const unsigned wave = tid >> 6;
  i64 id[4];
  unsigned p1[4];
  bool valid[4];
  const unsigned wm = set_wmask(a.nxt.m2);
  unsigned home[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const unsigned g = tile * MAP_SEG + (unsigned)r * 256u + tid;
    valid[r] = g < a.map_n;
    id[r] = a.map_ids[valid[r] ? g : a.map_n - 1];
  }
  uint4 e[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    home[r] = set_home(a.nxt, id[r], fmix64((u64)id[r]));
    e[r] = *reinterpret_cast<const uint4*>(a.nxt.ent + home[r]);
  }
  keep_live(e[0], e[1], e[2], e[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const i64 ek = (i64)(((u64)e[r].y << 32) | e[r].x);
    if (is_reserved_key(id[r])) p1[r] = ek != EMPTY_KEY ? e[r].z : 0u;
    else if (ek == id[r]) p1[r] = e[r].z;
    else if (ek == EMPTY_KEY) p1[r] = 0u;
    else {   // (rare: the plan's table is < 10 % full) further down the chain, inside the window
      p1[r] = 0u;
      for (unsigned t = 1; t <= wm; ++t) {
        const SetEnt* q = a.nxt.ent + set_at(home[r], t, wm);
        const i64 k = q->key;
        if (k == id[r]) { p1[r] = q->pos1; break; }
        if (k == EMPTY_KEY) break;
      }
    }
  }
  // ranks inside the segment: per round and wave by ballot, across the waves by LDS
  unsigned rank[4], nf_w = 0, nt_w = 0;
  const u64 below = (1ULL << lane) - 1ULL;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const u64 mf = __ballot(valid[r] && p1[r] != 0), mt = __ballot(valid[r] && p1[r] == 0);
    rank[r] = p1[r] ? nf_w + (unsigned)__popcll(mf & below) : nt_w + (unsigned)__popcll(mt & below);
    nf_w += (unsigned)__popcll(mf); nt_w += (unsigned)__popcll(mt);
  }
  if (lane == 0) { L.cnt[wave] = nf_w; L.cnt[4 + wave] = nt_w; }
  __syncthreads();
  unsigned bf = 0, bt = 0;
  for (unsigned w = 0; w < wave; ++w) { bf += L.cnt[w]; bt += L.cnt[4 + w]; }
  const unsigned seg0 = tile * MAP_SEG, m = min(MAP_SEG, a.map_n - seg0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (!valid[r]) continue;
    const unsigned g = seg0 + (unsigned)r * 256u + tid;
    const unsigned at = p1[r] ? seg0 + m - 1u - (bf + rank[r]) : seg0 + bt + rank[r];
    a.map_out[at] = make_uint4(g, p1[r], (unsigned)(u64)id[r], (unsigned)((u64)id[r] >> 32));
  }
}

// ---- FIND role from a MAP list: T tiles of 16 entries per wave --------------------------------------------------------------
// Block b takes chunk b / nseg of segment b % nseg (chunk-major: the FRONT chunks of every segment — the table-bound positions, the
// long chains — are the first blocks of the role; the all-forwarded chunks fill in behind them).  A wave takes T consecutive tiles of
// its chunk, the next tile's entries loaded before the current tile's rows are stored.
template <int U, int T>
__device__ __forceinline__ void find_list_role(const StepArgs& a, unsigned blk) {
  constexpr int KW = 4 * U;
  constexpr unsigned CH = 64u * (unsigned)T;   // entries per block
  const TableView& v = a.own.v;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const unsigned nseg = (a.n + MAP_SEG - 1) / MAP_SEG;
  const unsigned sg = blk % nseg, ch = blk / nseg;
  const unsigned base0 = sg * MAP_SEG + ch * CH + (threadIdx.x >> 6) * (unsigned)(KW * T);
  if (base0 >= a.n) return;
  const unsigned last = a.n - 1;
  uint4 ent = a.find_list[min(base0 + (unsigned)(lane & (KW - 1)), last)];
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    const unsigned base = base0 + (unsigned)(t * KW);
    if (base >= a.n) break;
    const uint4 cur = ent;
    if (t + 1 < T) ent = a.find_list[min(base + (unsigned)KW + (unsigned)(lane & (KW - 1)), last)];
    const bool all_fwd = __ballot(cur.y == 0) == 0ULL;
    unsigned pos[U], fwd_pos[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = u * 4 + grp;
      pos[u] = (unsigned)__shfl((int)cur.x, j);
      fwd_pos[u] = (unsigned)__shfl((int)cur.y, j);
    }
    const unsigned char* src[U];
    if (all_fwd) {   // (wave-uniform) every row of this tile is one of the rows being written
#pragma unroll
      for (int u = 0; u < U; ++u) {
        src[u] = a.own.vals + (u64)(fwd_pos[u] - 1u) * (u64)v.field_bytes;
        if (a.exists && sub == 0) __hip_atomic_store(a.exists + pos[u], (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      const i64 kreg = (i64)(((u64)cur.w << 32) | cur.z);
      u64 hreg;
      const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
      const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
      i64 key[U], k0[U], k1[U];
      unsigned b0[U], b1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = u * 4 + grp;
        key[u] = shfl_i64(kreg, j);
        b0[u] = (unsigned)__shfl((int)b0reg, j);
        b1[u] = (unsigned)__shfl((int)b1reg, j);
      }
      const i64* hot = reinterpret_cast<const i64*>(a.fwd.ent);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        k0[u] = (fwd_pos[u] ? hot : key_line(v, b0[u]))[sub];
        k1[u] = (fwd_pos[u] ? hot : key_line(v, b1[u]))[sub];
      }
      keep_live_n<U>(k0);
      keep_live_n<U>(k1);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned fw = fwd_pos[u];
        i64 word = 0;
        if (!fw) word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift, &k1[u]);
        if (a.exists && sub == 0) __hip_atomic_store(a.exists + pos[u], (uint8_t)(fw != 0 || word >= 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        src[u] = fw ? a.own.vals + (u64)(fw - 1u) * (u64)v.field_bytes
                    : (word >= 0 ? word_row_ptr(v, (u64)word) : a.defaults + (a.full ? (u64)pos[u] * (u64)v.field_bytes : 0));
      }
    }
    for (unsigned off = sub * 16; off < v.field_bytes; off += 256) {
      uint4 tmp[U];
#pragma unroll
      for (int u = 0; u < U; ++u) tmp[u] = *reinterpret_cast<const uint4*>(src[u] + off);
      keep_live_n<U>(tmp);
#pragma unroll
      for (int u = 0; u < U; ++u) store_wt16(a.out + (u64)pos[u] * (u64)v.field_bytes + off, tmp[u]);
    }
  }
}
// a lookup block is done: its output rows are in memory (write-through, acknowledged).  Only the tail's rare corrections wait for this.
__device__ __forceinline__ void find_arrive(const StepArgs& a) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && a.tail_blocks) __hip_atomic_fetch_add(a.sync + 32 * (1 + (blockIdx.x & 7u)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- OWN role: the ownership pass over the previous batch's plan, read straight from its TABLE ---------------------------
// The plan keeps no dense list of its keys any more (that list was a returned atomic per tile and a dependent round trip of
// the builder): the block takes a slice of own_slice slots of the plan's table (one 16-byte load per thread and a few more),
// compacts the occupied ones in LDS — key, last position, slot (the key's flag byte) — and its four waves take them 4 U at a
// time through own_batch16, victims checked against this batch's plan.
template <bool SIMPLE, int U>
__device__ __forceinline__ void own_role(const StepArgs& a, unsigned blk, StepLds& L) {
  const OwnArgs& o = a.own;
  const unsigned tid = threadIdx.x;
  const int lane = tid & 63;
  const unsigned lo = blk * a.own_slice, total_slots = a.fwd.m2 + 2;
  if (tid == 0) L.n = 0;
  uint4 e[3];
  bool have[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const unsigned off = tid + (unsigned)r * 256u;
    have[r] = off < a.own_slice && lo + off < total_slots;
    e[r] = *reinterpret_cast<const uint4*>(a.fwd.ent + (have[r] ? lo + off : lo));
  }
  if (blk == 0 && tid == 0 && a.progress) __hip_atomic_store(a.progress, a.progress_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const bool publish = blk == 0 && a.own_ucnt && a.progress;   // (block-uniform)
  unsigned ucnt = 0;
  if (publish) {
    if (tid == 0) L.cnt[200] = 0;
    ucnt = tid < a.own_ucnt_n ? a.own_ucnt[tid] : 0u;
  }
  __syncthreads();
  if (publish) {
    for (int off = 32; off > 0; off >>= 1) ucnt += (unsigned)__shfl_xor((int)ucnt, off);
    if (lane == 0) atomicAdd(&L.cnt[200], ucnt);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const unsigned slot = lo + tid + (unsigned)r * 256u;
    const i64 k = (i64)(((u64)e[r].y << 32) | e[r].x);
    if (have[r] && k != EMPTY_KEY) {
      const unsigned at = atomicAdd(&L.n, 1u);
      L.key[at] = slot >= a.fwd.m2 ? EMPTY_KEY + (i64)(slot - a.fwd.m2) : k;   // (sentinel slots hold a marker, the slot says which key)
      L.pos[at] = e[r].z;
      L.pos[1024 + at] = slot;
    }
  }
  __syncthreads();
  const unsigned cnt = L.n;
  if (publish && tid == 0) __hip_atomic_store(a.progress + 1, L.cnt[200], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // this batch's distinct keys
  // (Tried: ONE round per block — 16 U keys — and the few keys beyond it straight onto the item list, so that no block runs the
  // chain of round trips twice: the slowest write-back blocks are not the ones with a second round — the role ended at 19 us as
  // before — and the tail, with 60 items instead of a dozen, ran longer: 31.9 -> 37.3 us per step.)
  int fresh = 0;
  const OwnFlags fl = own_setup<SIMPLE>(o);
  for (unsigned wbase = (tid >> 6) * (4 * U); wbase < cnt; wbase += 4 * (4 * U)) {
    const unsigned i = wbase + (unsigned)(lane & 15);
    const unsigned c = min(i, cnt - 1);
    own_batch16<16, SIMPLE, SRC_GIVEN, U, true, false, true>(o, fl, L.pos[1024 + c], (lane & 15) < 4 * U && i < cnt, a.own_gen, a.sync + 1, lane, fresh, &a.nxt,
                                                             a.stat, L.key[c], L.pos[c] - 1u, &a.fwd);
  }
  for (int off = 32; off > 0; off >>= 1) fresh += __shfl_xor(fresh, off);
  if (lane == 0 && fresh) size_add(o.v, blk * 4u + (tid >> 6), fresh);
  // this block's part of the pass is in memory (everything it wrote went write-through or by atomics): the tail may go on
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_fetch_add(a.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (Tried: the write-back over a DENSE KEY LIST of the plan — a plan built by setplan_kernel as a launch of its own — instead of
// slices of its table: 8 keys for every wave, no empty slots to skip — 43.5 us per step against 45.0 with that plan launch, 33 without.)

// TIMING (tuning builds only): every block notes its start and end on the device clock in a.tbuf (a slot per launch and block):
// when does each role of a launch run?
constexpr unsigned TIMING_BLOCKS = 4096, TIMING_SLOTS = 64;
__device__ __forceinline__ void role_stamp(const StepArgs& a, u64 t0) {
  __syncthreads();
  if (threadIdx.x == 0 && a.tbuf && blockIdx.x < TIMING_BLOCKS) {
    u64* w = a.tbuf + ((size_t)(a.progress_val % TIMING_SLOTS) * TIMING_BLOCKS + blockIdx.x) * 2;
    w[0] = t0;
    w[1] = (u64)wall_clock64();
  }
}
// role of block b: 0 build, 1 scatter, 2 write-back, 3 lookup, 4 tail; *idx = its index in the role.  Grid order: the builders
// (short chains of dependent round trips, few blocks), the whole write-back (the tail waits for it), the lookup, the TAIL.
// Tried, measured on the metric's configuration, dropped: (a) the write-back's blocks spread evenly among the lookup's — no
// change; (b) the tail IN FRONT of the lookup's blocks, so that it holds its wave slots from the start instead of getting them
// 18 us into the launch: its 32 polling blocks (one lane each, s_sleep between polls) slow the write-back they wait for from 19
// to 34 us — the step went from 33 to 45 us.  Behind the lookup's blocks the tail starts when the write-back is (nearly) done
// and hardly ever polls; (c) the write-back's blocks in front of the builders': no change.
__host__ __device__ __forceinline__ int step_role(unsigned b, unsigned build_blocks, unsigned scat_blocks, unsigned map_blocks, unsigned F1, unsigned O,
                                                  unsigned F, unsigned T, unsigned* idx) {
  (void)T;
  if (b < build_blocks) { *idx = b; return 0; }
  b -= build_blocks;
  if (b < scat_blocks) { *idx = b; return 1; }
  b -= scat_blocks;
  if (b < map_blocks) { *idx = b; return 5; }   // (MAP: numbered behind the roles the tuning scripts know)
  b -= map_blocks;
  if (b < F1) { *idx = b; return 3; }            // the lookup's first blocks in front of the write-back's
  b -= F1;
  if (b < O) { *idx = b; return 2; }
  b -= O;
  if (b < F - F1) { *idx = F1 + b; return 3; }
  *idx = b - (F - F1);
  return 4;
}
__device__ __forceinline__ void tail_role(const StepArgs& a, unsigned blk, StepLds& L);
// A kernel gets the registers of its hungriest role for EVERY wave: the lookup and the builders need 58, the write-back 91, the
// tail's locked protocol 113 — 4 blocks per CU for 32 blocks of the grid.  The kernels are compiled for 5 waves per SIMD
// (amdgpu_waves_per_eu: 96 registers, six spilled ones, all in the tail): 1280 resident blocks instead of 1024, the lookup's
// first blocks start with the launch instead of behind the builders — 33.3 -> 31.4 us per step.  6 waves (80 registers, 62
// spilled, some in the write-back): 32.6 us.
template <bool SIMPLE, int U, bool TIMING, int WAVES>
__device__ __forceinline__ void step_body(const StepArgs& a) {
  __shared__ StepLds L;
  const u64 t0 = TIMING ? (u64)wall_clock64() : 0;
  unsigned idx;
  const int role = step_role(blockIdx.x, a.build_blocks, a.scat_blocks, a.map_blocks, a.find_first, a.own_blocks, a.find_blocks, a.tail_blocks, &idx);
  if (role == 0) { if (!(a.ablate & 1)) build_role(a, idx, L); }
  else if (role == 1) { if (!(a.ablate & 1)) scatter_role(a, idx, L); }
  else if (role == 5) { if (!(a.ablate & 1)) map_role(a, idx, L); }
  else if (role == 2) { if (!(a.ablate & 2)) own_role<SIMPLE, U>(a, idx, L); }
  else if (role == 3) { if (!(a.ablate & 4)) { if (a.find_list) find_list_role<4, 1>(a, idx); else find_fwd_role<4>(a, idx); } find_arrive(a); }
  else { if (!(a.ablate & (2 | 8))) tail_role(a, idx, L); }
  if (TIMING) role_stamp(a, t0);
}
// Instantiations (the budgets are attributes, not template arguments): 256-thread blocks are admitted per CU up to
// floor(800 / (ceil(sgpr / 16) * 16 + 16)) — ~106 scalar registers (what the big argument block costs) allow 6, 96 allow 7, 80 allow 8.
#define TFRA_STEP_KERNEL(NAME, SIMPLE, UU, TIMING, W)                                                                \
  __global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(104), amdgpu_waves_per_eu(W, W))) void NAME(const StepArgs a) { step_body<SIMPLE, UU, TIMING, W>(a); }
TFRA_STEP_KERNEL(step_k_u2, true, 2, false, 5)
TFRA_STEP_KERNEL(step_k_u2_t, true, 2, true, 5)
TFRA_STEP_KERNEL(step_k_u1, true, 1, false, 5)        // (tuning) 4 keys per wave in the write-back
TFRA_STEP_KERNEL(step_k_u2_w4, true, 2, false, 4)     // (tuning) no spills, 4 blocks per CU
TFRA_STEP_KERNEL(step_k_u2_w6, true, 2, false, 6)     // (tuning) 6 blocks per CU
// Round 6: the strategy read at run time (SIMPLE = false: own_setup takes it from the table's ScoreP) — EPOCHLRU tables, whose scores
// are (epoch << 32 | clock): like LRU a new key is ALWAYS admitted (it carries the highest score of its buckets), which is what the
// forwarding rests on; LFU / EPOCHLFU / CUSTOMIZED may refuse a key and stay on the sequential path.  4 blocks per CU (no spills).
TFRA_STEP_KERNEL(step_k_gen, false, 2, false, 4)
#undef TFRA_STEP_KERNEL

// ---- TAIL role: the remainder of a step INSIDE its launch ------------------------------------------------------------------
// The keys the pass left over (lost claims, evictions it deferred) with the locked protocol, and the corrections of the
// lookup's output.  As a launch of its own behind the step this cost 5.5 us of dependent round trips plus two kernel
// boundaries — a quarter of the step — for a dozen keys.  Here it is the LAST blocks of the grid (blocks are dispatched in index
// order: when a tail block runs, every other block of the launch is running or done — nothing it waits for can be waiting for a
// wave slot), which
//   1. wait until every write-back block has arrived (a.sync[0]; their stores are write-through, acknowledged before they arrive),
//   2. take the item list with the locked protocol, beside the lookup blocks still running — an eviction here may hit a key the
//      lookup has returned (or is about to return) a row for: every victim that is one of this batch's ids (plan `nxt`) goes
//      onto the launch's list;
//   3. meet (a.sync[32*9]); if the list is not empty — rare — wait for every lookup block too, look the listed victims up again
//      and, for those that are absent now, rewrite the lookup's output rows with the default row and clear their exists flags,
//      each block for its share of the batch.  (A victim that is present again was a key of the previous batch whose own
//      left-over write came later.)
// The spins are bounded; a timeout is reported through the table's error counter, never silent.
constexpr unsigned PATCH_CAP = 64, PATCH_GCAP = 4096, TAIL_BLOCKS = 32;
__device__ __forceinline__ bool spin_until(const unsigned* ctr, unsigned want) {
  for (unsigned it = 0; it < (1u << 22); ++it) {
    if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) return true;
    __builtin_amdgcn_s_sleep(8);
  }
  return false;
}
// the same on the LOW word of an 8-byte pair, read as one: *both = the pair as it was when the low word had reached `want` (a count
// kept in the high word by those who arrive is complete then — their additions to it come before their arrival)
__device__ __forceinline__ bool spin_until_pair(const unsigned* ctr, unsigned want, unsigned long long* both) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(ctr);
  for (unsigned it = 0; it < (1u << 22); ++it) {
    const unsigned long long v = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)v >= want) { *both = v; return true; }
    __builtin_amdgcn_s_sleep(8);
  }
  *both = 0;
  return false;
}
__device__ __forceinline__ uint4 load_coherent16(const void* p) {   // written write-through by another workgroup of this launch
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long x = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), y = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_uint4((unsigned)x, (unsigned)(x >> 32), (unsigned)y, (unsigned)(y >> 32));
}
__device__ __forceinline__ void tail_role(const StepArgs& a, unsigned blk, StepLds& L) {
  i64* s_patch = L.key;                                            // [PATCH_CAP]
  i64* s_row = L.key + PATCH_CAP;                                  // [PATCH_CAP] row index now, -1: absent
  unsigned& s_nv = L.n;
  const OwnArgs& o = a.own;
  const unsigned tid = threadIdx.x;
  const int lane = tid & 63, sub = lane & 15, gshift = lane & 48;
  if (blk == 0) {   // arm what the next launch counts in (its users of two launches ago are long gone)
    if (tid < 4 && a.zero4) a.zero4[tid] = 0;
    if (tid >= 32 && tid < 42) a.sync_next[32 * (tid - 32)] = 0;
    if (tid == 62) a.sync_next[1] = 0;          // (the left-over count beside the write-back's arrivals)
    if (tid == 63) *a.patch_count_next = 0;     // (the victim count beside the tail's arrivals)
  }
  bool ok = true;
  // (the chain from here on is the end of the step — the lookup is done by the time the items are: the left-over count arrives WITH
  // the write-back's last arrival, the victim count with the tail's.  Measured: no change, 8 dependent trips are left; neither did
  // an item's value row fetched along with its bucket lines)
  if (tid == 0) {
    unsigned long long both;
    ok = spin_until_pair(a.sync, a.own_blocks, &both);
    L.cnt[1] = (unsigned)(both >> 32);
  }
  if (tid == 0) { L.cnt[2] = ok ? 1u : 0u; if (!ok) atomicAdd(o.v.err_count, 1u); }   // a timeout leaves keys unwritten: reported, never silent
  __syncthreads();
  const unsigned counted = L.cnt[1];
  ok = L.cnt[2] != 0;
  if (counted == 0) return;                                        // no items, no evictions, nothing to correct (the same in every tail block)
  const bool listed = counted <= o.item_cap;
  const unsigned n = listed ? counted : a.fwd.m2 + 2;              // (the list overflowed: the flag byte of every slot of the plan's table)
  const unsigned gi = (blk * 256u + tid) >> 4, ngroups = (a.tail_blocks * 256u) >> 4;
  int fresh = 0, failed = 0;
  // a key whose slot changed hands — or showed LOCKED for a moment — while the lookup was running, and which the lookup looks for
  auto note = [&](i64 k) {
    if (k == EMPTY_KEY || k == LOCKED_KEY || !a.n || !set_contains_group(a.nxt, k, sub, gshift)) return;
    if (sub == 0) {
      const unsigned at = atomicAdd(a.patch_count, 1u);
      atomicAdd(a.stat + 1, 1u);
      if (at < PATCH_GCAP) __hip_atomic_store(a.patch_keys + at, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else atomicAdd(o.v.err_count, 1u);   // (thousands of them in one step: reported by check_errors, never silent)
    }
  };
  for (unsigned i = gi; i < n; i += ngroups) {
    i64 vk = EMPTY_KEY, gb[4];
    int ngb = 0;
    if (listed) {
      const uint4 w0 = load_coherent16(o.items + i), w1 = load_coherent16(reinterpret_cast<const unsigned char*>(o.items + i) + 16);
      const i64 key = (i64)(((u64)w0.y << 32) | w0.x);
      locked_upsert_kv<16>(o.v, o.vals, key, w0.z, ((u64)w1.y << 32) | w1.x, o.ai, o.sp, sub, gshift, fresh, failed, w1.z != 0, w1.w, &vk, 0, 0, gb, &ngb);
      if (sub == 0) o.dflag[w0.w] = 0;
    } else {
      if (__hip_atomic_load(o.dflag + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 4) continue;
      const SetEnt* pe = a.fwd.ent + i;
      const i64 key = i >= a.fwd.m2 ? EMPTY_KEY + (i64)(i - a.fwd.m2) : pe->key;
      locked_upsert_kv<16>(o.v, o.vals, key, pe->pos1 - 1, 1, o.ai, o.sp, sub, gshift, fresh, failed, false, 0, &vk, 0, 0, gb, &ngb);
      if (sub == 0) o.dflag[i] = 0;
    }
    note(vk);
    for (int q = 0; q < ngb && q < 4; ++q) note(gb[q]);
    if (ngb > 4 && sub == 0) atomicAdd(o.v.err_count, 1u);
  }
  for (int off = 32; off > 0; off >>= 1) { fresh += __shfl_xor(fresh, off); failed += __shfl_xor(failed, off); }
  if (lane == 0) {
    if (fresh) size_add(o.v, (blk * 256u + tid) >> 6, fresh);
    if (failed) atomicAdd(o.v.err_count, (unsigned)failed);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's table stores and list entries (write-through / agent-scope) are acknowledged
  __syncthreads();
  if (tid == 0) {
    __hip_atomic_fetch_add(a.sync + 32 * 9, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long both;
    ok = spin_until_pair(a.sync + 32 * 9, a.tail_blocks, &both) && ok;
    unsigned nv = min((unsigned)(both >> 32), PATCH_GCAP);   // a.patch_count, the word beside the arrivals
    if (nv) {   // the corrections overwrite what the lookup wrote: every lookup block must be done
      unsigned have = 0;
      for (unsigned it = 0; it < (1u << 20) && have < a.find_blocks; ++it) {
        have = 0;
        for (int q = 1; q <= 8; ++q) have += __hip_atomic_load(a.sync + 32 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (have < a.find_blocks) __builtin_amdgcn_s_sleep(16);
      }
      ok = ok && have >= a.find_blocks;
    }
    if (!ok) atomicAdd(o.v.err_count, 1u);   // (never seen: nothing anybody waits for here waits for anything itself)
    s_nv = nv;
  }
  __syncthreads();
  const unsigned nv = s_nv;
  for (unsigned base = 0; base < nv; base += PATCH_CAP) {
    const unsigned np = min(PATCH_CAP, nv - base);
    // where are these keys now?  (16 groups, one key each per round; coherent loads)  The lookup is done again for them:
    for (unsigned q = tid >> 4; q < np; q += 16) {
      const i64 vk = __hip_atomic_load(a.patch_keys + base + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const i64 row = probe_find<true>(o.v, vk, sub, gshift);
      if (sub == 0) { s_patch[q] = vk; s_row[q] = row; }
    }
    __syncthreads();
    // ... at this block's share of the batch's positions: the row the table holds now, or the default row
    for (unsigned p = blk * 256u + tid; p < a.n; p += a.tail_blocks * 256u) {
      const i64 id = a.ids[p];
      int hit = -1;
      for (unsigned q = 0; q < np; ++q) if (s_patch[q] == id) hit = (int)q;
      if (hit < 0) continue;
      const i64 row = s_row[hit];
      const unsigned char* d = row >= 0 ? row_ptr(o.v, row) : a.defaults + (a.full ? (u64)p * (u64)o.v.field_bytes : 0);
      unsigned char* w = a.out + (u64)p * (u64)o.v.field_bytes;
      for (unsigned off = 0; off < o.v.field_bytes; off += 16) *reinterpret_cast<uint4*>(w + off) = load_coherent16(d + off);   // (a row another workgroup of this launch may have written)
      if (a.exists) a.exists[p] = row >= 0;
      atomicAdd(a.stat + 2, 1u);
    }
    __syncthreads();
  }
}

}  // namespace
