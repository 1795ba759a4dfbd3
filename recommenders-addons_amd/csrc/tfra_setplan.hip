// The SET plan — the assign-only write-back plan of a batch (tfra_sparse_plan_build with dim 0): distinct ids, the position of each
// one's LAST occurrence, optionally how often it occurred — and what is built on it: tf.unique without the first-occurrence order
// (tfra_unique_unordered) and the lookup fused with it (tfra_table_find_unique).  The CSR plan of the gradient half, the plan
// object's life and tfra_sparse_plan_read are tfra_csr.hip's; the two units share the tfra_sparse_plan object (tfra_plan.h) and the
// control words of its count blocks (tfra_plan_device.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_plan.h"

using namespace tfra;

namespace {

// ---------------------------------------------------------------------------------------------
// SET plan: the id-only half of an ASSIGN write-back (tfra_sparse_plan_build with dim 0) in ONE kernel.
// An assign needs, per distinct id, the position of its LAST occurrence (and how often it occurred: LFU scores) — not the
// CSR of all positions the gradient sums need.  The CSR plan's three kernels take 29 us for 131 072 ids and six of the
// step's nine kernel launches; the step driver that builds it one batch ahead was bound by the host's launch rate
// (52 us per step of host time for 39 us of kernels on the main stream).
//   phase A  one block per 1024 ids: equal ids meet in an LDS hash table (compare-and-swap on the key word, atomic max on
//            position + 1, atomic add on the count);
//   phase B  every distinct id of the block goes into a global open-addressing table of >= 2 n slots (compare-and-swap on
//            the key, atomic max / add on (position + 1, count)): its slot is the same for every block.  The block whose
//            swap installed the key appends (key, slot) to the dense list of distinct keys — one counter add per block;
//   phase C  the plan keeps TWO such tables and alternates: while build k fills one, it empties the slots build k-1 used in
//            the other (its dense list says which) — no memset, no extra launch.
// NO block finishes the build for the others (round 3: the kernel used to end with a ticket — wait for the block's stores,
// draw, the last block reads the count and publishes it to device and pinned memory, resets the counters: four more
// dependent round trips, 6 of the kernel's 17.8 us).  The count of distinct keys IS the append counter, read by the
// consumer after the kernel; each table has two counter words and alternates between them from use to use — block 0 of a
// build zeroes the word of the table's NEXT use (its last reader, the other table's build right after the use before,
// is over by stream order).  The host sizes the consumer's grid from the count the previous write-back saw
// (upsert_own_kernel publishes it), grid-stride covers a batch that has more.
// The two sentinel key values have slots of their own behind the table (no hashing: EMPTY_KEY is the free-slot marker).
constexpr int SP_NT = 1024;
constexpr unsigned SP_LDS = 2048;

// COUNTS: also count the occurrences of every id (LFU scores without caller scores; tfra_sparse_plan_read)
// INDEX: the occurrence-count word of a key's table entry receives the key's position in the dense list instead (tfra_unique_unordered)
// FUSED (tfra_unique_unordered in ONE launch, INDEX only, grids of <= 128 blocks — all co-resident on half the chip): the kernel also
// writes the inverse index idx_out[i] = position of ids[i] in the dense list, the list itself into unique_out and — the last block to
// add its share — its length into num_out.  A key's dense index exists once the block that INSTALLED the key has drawn its base
// from the append counter; the other blocks holding the key poll the entry's index word (index + 1, 0 = not yet) — one poller per
// block and distinct id (the block's ids share the answer through LDS), a wait of one atomic's round trip.
// IPT ids per thread (1; 2 in find_unique_kernel: half the blocks — half the wave slots — for the same ids; the LDS table grows with it)
template <bool COUNTS, bool INDEX, bool FUSED, int IPT = 1>
__device__ __forceinline__ void setplan_block(const unsigned bid, const unsigned nblk, size_t n, const i64* __restrict__ ids, unsigned m2,
                                              const SetTab& cur, const SetTab& old, unsigned* next_use_count, i64* __restrict__ unique_out,
                                              int* __restrict__ idx_out, i64* __restrict__ num_out, unsigned* err = nullptr) {
  static_assert(!FUSED || (INDEX && !COUNTS), "FUSED: the unique-with-index build");
  constexpr unsigned LDSN = SP_LDS * IPT;   // slots of the block's LDS table: two per id
  constexpr int NR = 2 * IPT;               // ... = NR per thread
  __shared__ i64 s_key[LDSN];
  __shared__ unsigned s_pos[LDSN + 2], s_cnt[LDSN + 2];
  __shared__ unsigned s_n, s_base;
  const unsigned tid = threadIdx.x;
  const unsigned n_old = *old.count;
  if (bid == 0 && tid == 0) *next_use_count = 0;
  for (unsigned i = tid; i < LDSN + 2; i += SP_NT) { if (i < LDSN) s_key[i] = EMPTY_KEY; s_pos[i] = 0; if (COUNTS || FUSED) s_cnt[i] = 0; }
  if (tid == 0) s_n = 0;
  __syncthreads();
  // ---- A: equal ids of the block meet in LDS ---------------------------------------------------------------
  const size_t gid = (size_t)bid * SP_NT + tid;   // (phase C's start)
  size_t gids[IPT];
  unsigned lds_slot[IPT];   // FUSED: where each of this thread's ids sits in the block's LDS table
#pragma unroll
  for (int q = 0; q < IPT; ++q) {
    gids[q] = ((size_t)bid * IPT + q) * SP_NT + tid;
    lds_slot[q] = 0;
    if (gids[q] < n) {
      const i64 id = ids[gids[q]];
      unsigned slot;
      if (is_reserved_key(id)) slot = LDSN + (unsigned)reserved_index(id);
      else {
        slot = (unsigned)(fmix64((u64)id) >> 41) & (LDSN - 1);
        for (;;) {
          const i64 was = (i64)atomicCAS(reinterpret_cast<unsigned long long*>(&s_key[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)id);
          if (was == EMPTY_KEY || was == id) break;
          slot = (slot + 1) & (LDSN - 1);
        }
      }
      atomicMax(&s_pos[slot], (unsigned)gids[q] + 1u);
      if (COUNTS) atomicAdd(&s_cnt[slot], 1u);
      lds_slot[q] = slot;
    }
  }
  __syncthreads();
  // ---- B: the block's distinct ids into the global table: the first probes of both of a thread's keys travel together ----
  i64 mykey[NR];
  unsigned myslot[NR], myidx[NR], p1[NR], cn[NR];
  bool have[NR], mine[NR];
  i64 was[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const unsigned s = tid + (unsigned)r * SP_NT;   // 2048 hash slots per id of a thread; the two sentinel slots ride with threads 0 and 1 below
    mine[r] = false;
    mykey[r] = s_key[s];
    p1[r] = s_pos[s]; cn[r] = COUNTS ? s_cnt[s] : 0u;
    have[r] = p1[r] != 0;
    myslot[r] = (unsigned)(fmix64((u64)mykey[r]) >> 20) & (m2 - 1);
    was[r] = 0;
    if (have[r]) was[r] = (i64)atomicCAS(reinterpret_cast<unsigned long long*>(&cur.ent[myslot[r]].key), (unsigned long long)EMPTY_KEY, (unsigned long long)mykey[r]);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (have[r]) {
      for (;;) {
        if (was[r] == EMPTY_KEY) { mine[r] = true; break; }
        if (was[r] == mykey[r]) break;
        myslot[r] = set_at(myslot[r], 1u, set_wmask(m2));
        was[r] = (i64)atomicCAS(reinterpret_cast<unsigned long long*>(&cur.ent[myslot[r]].key), (unsigned long long)EMPTY_KEY, (unsigned long long)mykey[r]);
      }
      // (INDEX — tf.unique: nobody reads a last position, and the entry's other word is what the other blocks POLL for the key's index:
      // an atomic on the line they are reading is the slow kind, NOTEBOOK round 2)
      if (!INDEX) atomicMax(&cur.ent[myslot[r]].pos1, p1[r]);
      if (COUNTS) atomicAdd(&cur.ent[myslot[r]].cnt, cn[r]);
    }
    myidx[r] = mine[r] ? atomicAdd(&s_n, 1u) : 0u;
  }
  if (tid < 2 && s_pos[LDSN + tid] != 0) {   // a sentinel key value occurred in this block
    const unsigned sl = m2 + tid;
    const i64 w = (i64)atomicCAS(reinterpret_cast<unsigned long long*>(&cur.ent[sl].key), (unsigned long long)EMPTY_KEY, 1ULL);
    if (!INDEX) atomicMax(&cur.ent[sl].pos1, s_pos[LDSN + tid]);
    if (COUNTS) atomicAdd(&cur.ent[sl].cnt, s_cnt[LDSN + tid]);
    if (w == EMPTY_KEY) {
      const unsigned at = atomicAdd(cur.count, 1u);   // (rare: its own add)
      cur.ukeys[at] = EMPTY_KEY + (i64)tid;
      cur.uslot[at] = sl;
      if (FUSED) { unique_out[at] = EMPTY_KEY + (i64)tid; __hip_atomic_store(&cur.ent[sl].cnt, at + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      else if (INDEX) cur.ent[sl].cnt = at;
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (FUSED) {
      // the block's share and its ARRIVAL in one 64-bit add — the word in front of the count (always 0 otherwise: the use block's PC_HOT)
      // counts the blocks: the last one to arrive sees the others' shares in the value returned and knows the list's length there
      // and then (a ticket of its own at the end of the kernel was one more round trip); it leaves the word at 0 again
      const unsigned long long r = atomicAdd(reinterpret_cast<unsigned long long*>(cur.count - SC_USE_COUNT), ((unsigned long long)s_n << 32) | 1ULL);
      s_base = (unsigned)(r >> 32);
      if ((unsigned)r == nblk - 1u) {
        *num_out = (i64)(s_base + s_n);
        __hip_atomic_store(cur.count - SC_USE_COUNT, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      s_base = s_n ? atomicAdd(cur.count, s_n) : 0u;
    }
  }
  // ---- C: empty the slots the previous build used in the OTHER table (while the counter add travels) -------------------
  for (size_t i = gid; i < n_old; i += (size_t)nblk * SP_NT) {
    const unsigned sl = old.uslot[i];
    *reinterpret_cast<uint4*>(old.ent + sl) = make_uint4(0u, 0x80000000u, 0u, 0u);   // {EMPTY_KEY, 0, 0}
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (!mine[r]) continue;
    cur.ukeys[s_base + myidx[r]] = mykey[r];
    cur.uslot[s_base + myidx[r]] = myslot[r];
    if (FUSED) { unique_out[s_base + myidx[r]] = mykey[r]; __hip_atomic_store(&cur.ent[myslot[r]].cnt, s_base + myidx[r] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    else if (INDEX) cur.ent[myslot[r]].cnt = s_base + myidx[r];
  }
  if (FUSED) {
    // the dense index of every distinct id of the block -> LDS (s_cnt is free here): drawn above for the keys this block installed,
    // polled from the entry for the others (their installer is a resident block: at most 128 de-duplicating blocks — 256 with
    // TFRA_FU_IPT=1 above 131072 ids, still co-resident: 1024 threads of 57 registers, four blocks per CU).  The poll is bounded; a
    // timeout leaves idx_out = -1 for the block's positions of that id AND counts an error (`err`: the table's counter under
    // tfra_table_find_unique, the workspace's under tfra_unique_unordered), so that nothing indexes with it unnoticed.
    bool timed_out = false;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (!have[r]) continue;
      unsigned v = mine[r] ? s_base + myidx[r] + 1u : 0u;
      for (unsigned it = 0; !v && it < (1u << 24); ++it) {
        v = __hip_atomic_load(&cur.ent[myslot[r]].cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!v) __builtin_amdgcn_s_sleep(2);
      }
      timed_out |= v == 0u;
      s_cnt[tid + (unsigned)r * SP_NT] = v;
    }
    if (tid < 2 && s_pos[LDSN + tid] != 0) {   // a sentinel key value occurred in this block
      unsigned v = 0;
      for (unsigned it = 0; !v && it < (1u << 24); ++it) {
        v = __hip_atomic_load(&cur.ent[m2 + tid].cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!v) __builtin_amdgcn_s_sleep(2);
      }
      timed_out |= v == 0u;
      s_cnt[LDSN + tid] = v;
    }
    if (timed_out && err) atomicAdd(err, 1u);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < IPT; ++q)
      if (gids[q] < n) idx_out[gids[q]] = (int)s_cnt[lds_slot[q]] - 1;   // (-1 only after a poll that timed out: never seen; counted in *err)
  }
}

template <bool COUNTS, bool INDEX = false, bool FUSED = false>
__global__ __launch_bounds__(SP_NT) void setplan_kernel(size_t n, const i64* __restrict__ ids, unsigned m2, SetTab cur, SetTab old,
                                                        unsigned* next_use_count, i64* __restrict__ unique_out = nullptr,
                                                        int* __restrict__ idx_out = nullptr, i64* __restrict__ num_out = nullptr,
                                                        unsigned* err = nullptr) {
  setplan_block<COUNTS, INDEX, FUSED>(blockIdx.x, gridDim.x, n, ids, m2, cur, old, next_use_count, unique_out, idx_out, num_out, err);
}

// TFRA>HkvHashTableEmbeddingLookup in ONE launch (tfra_table_find_unique): the first `ublocks` blocks (<= 128: co-resident, see FUSED)
// de-duplicate the ids — distinct ids, inverse index, count —, the blocks behind them look the SAME ids up in the table.  The
// de-duplication waits (atomics' round trips: 85 % of its wave cycles), the lookup moves bytes: side by side they take the time of
// the longer one instead of the sum plus a launch gap.  16 waves per block, the lookup's waves as in find_kernel.
template <int G, bool PF1, int FU_IPT>
__global__ __launch_bounds__(SP_NT) void find_unique_kernel(unsigned ublocks, size_t n, const i64* __restrict__ ids, unsigned m2, SetTab cur, SetTab old,
                                                            unsigned* next_use_count, i64* __restrict__ unique_out, int* __restrict__ idx_out,
                                                            i64* __restrict__ num_out, TableView v, unsigned char* __restrict__ rows_out,
                                                            uint8_t* __restrict__ exists, const unsigned char* __restrict__ defaults, int full) {
  if (blockIdx.x < ublocks) {
    setplan_block<false, true, true, FU_IPT>(blockIdx.x, ublocks, n, ids, m2, cur, old, next_use_count, unique_out, idx_out, num_out, v.err_count);
    return;
  }
  find_wave<G, 4, G == 16, PF1>(v, n, ids, rows_out, exists, defaults, full, 0u, (blockIdx.x - ublocks) * (SP_NT / 64) + (threadIdx.x >> 6));
}

// tfra_unique_unordered, second launch: idx[i] = position of ids[i] in the plan's dense list (a probe of the plan's table);
// the list itself and its length are copied out on the way.
__global__ __launch_bounds__(256) void unique_idx_kernel(size_t n, const i64* __restrict__ ids, SetProbe pr, const i64* __restrict__ ukeys,
                                                         const unsigned* __restrict__ count, i64* __restrict__ unique_out, int* __restrict__ idx_out,
                                                         i64* __restrict__ num_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned U = *count;
  if (i == 0) *num_out = (i64)U;
  if (i < U) unique_out[i] = ukeys[i];
  if (i >= n) return;
  const i64 id = ids[i];
  unsigned slot = set_home(pr, id, fmix64((u64)id));
  const unsigned wm = set_wmask(pr.m2);
  int found = -1;
  if (is_reserved_key(id)) found = (int)pr.ent[slot].cnt;
  else {
    for (unsigned g = 0; g <= wm; ++g) {
      const SetEnt* e = pr.ent + set_at(slot, g, wm);
      const i64 k = e->key;
      if (k == id) { found = (int)e->cnt; break; }
      if (k == EMPTY_KEY) break;
    }
  }
  idx_out[i] = found;
}

__global__ void fill_setent_kernel(SetEnt* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    *reinterpret_cast<uint4*>(p + i) = make_uint4(0u, 0x80000000u, 0u, 0u);   // {EMPTY_KEY, 0, 0}
}

}  // namespace

// The SET plan of a batch (dim 0): see setplan_kernel.  setplan_prepare = everything but the launch (buffers, which of the two
// tables, its counter words): the overlapped step builds the plan inside its own kernel (the BUILD / SCATTER roles of tfra_step_impl.h).
struct SetPlanLaunch { SetTab cur, old; unsigned* next_use_count; unsigned m2; unsigned blocks; };
static int setplan_ensure(tfra_sparse_plan* pl, size_t n, hipStream_t s) {   // the SET buffer, sized for n ids
  if (n > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, "sparse_plan_build: at most 2^18 ids per plan");
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  if (pl->set_cap < n) {
    if (pl->setbuf) {
      if (hipDeviceSynchronize() != hipSuccess || hipFree(pl->setbuf) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: free");
      pl->setbuf = nullptr; pl->set_cap = 0;
    }
    const size_t cap = std::max<size_t>(n, 4096);
    unsigned m2 = 4096;
    while ((size_t)m2 < 2 * cap) m2 <<= 1;
    const size_t tab = al(((size_t)m2 + 2 + SET_PAD) * sizeof(SetEnt)) + al(cap * 8) + al(cap * 4);   // entries, ukeys, uslot
    const size_t bytes = SC_WORDS * 4 + al((size_t)m2 + 8) + al((size_t)SLOW_CAP * sizeof(OwnItem)) + 2 * tab;   // (flag bytes: per key of a list, or per SLOT for the overlapped step)
    hipError_t e = hipMalloc(&pl->setbuf, bytes);
    if (e != hipSuccess) { pl->setbuf = nullptr; return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, "sparse_plan_build: hipMalloc"); }
    if (hipMemsetAsync(pl->setbuf, 0, bytes, s) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: memset");
    unsigned char* w = (unsigned char*)pl->setbuf;
    pl->set_counts = (unsigned*)w; w += SC_WORDS * 4;   // the control words: PC_* and SC_* of tfra_plan_device.h
    pl->set_dflag = (uint8_t*)w; w += al((size_t)m2 + 8);
    pl->set_items = (OwnItem*)w; w += al((size_t)SLOW_CAP * sizeof(OwnItem));
    for (int p = 0; p < 2; ++p) {
      SetTab& tb = pl->set_tab[p];
      tb.ent = (SetEnt*)w; w += al(((size_t)m2 + 2 + SET_PAD) * sizeof(SetEnt));
      tb.ukeys = (i64*)w; w += al(cap * 8);
      tb.uslot = (unsigned*)w; w += al(cap * 4);
      tb.count = nullptr;   // set per build: the table's two counter words alternate
      fill_setent_kernel<<<256, 256, 0, s>>>(tb.ent, (size_t)m2 + 2 + SET_PAD);
    }
    pl->set_cap = cap; pl->set_m2 = m2; pl->set_parity = 1; pl->set_use[0] = pl->set_use[1] = 0;
    pl->tab_state[0] = pl->tab_state[1] = 0;
  }
  return TFRA_OK;
}
// What each of the object's two tables holds (tab_state): the build rules differ in what they leave behind —
//   a REGULAR build (setplan_kernel) needs an EMPTY target, leaves it LISTED (keys + the dense list of the slots they took) and
//     empties the OTHER table through that table's list;
//   a LIST-LESS build (the step launch's BUILD role) rewrites every slot of its target, leaves it LISTLESS and touches nothing else.
// A plan object may see them in any order (a step driver whose look-ahead is sometimes missing: regular, list-less, regular on one
// object left the third build's target holding the first batch's keys).  setplan_prepare makes both tables what the regular
// build expects, whatever came before: a target that is not known empty is filled, an other table without a list is filled
// instead of walked, and a filled table's counter words are zeroed (a list-less build zeroes none).
static int setplan_fill_table(tfra_sparse_plan* pl, unsigned q, hipStream_t s) {
  fill_setent_kernel<<<256, 256, 0, s>>>(pl->set_tab[q].ent, (size_t)pl->set_m2 + 2 + SET_PAD);
  if (hipMemsetAsync(pl->set_counts + SC_USE_BASE + SC_TAB_STRIDE * q, 0, SC_TAB_STRIDE * sizeof(unsigned), s) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: memset");
  pl->tab_state[q] = TAB_EMPTY;
  return TFRA_OK;
}
static int setplan_prepare(tfra_sparse_plan* pl, size_t n, hipStream_t s, bool counts, SetPlanLaunch* L) {
  int rc = setplan_ensure(pl, n, s);
  if (rc) return rc;
  const unsigned p = pl->set_parity ^ 1u;
  pl->gen += 1;
  const unsigned blocks = (unsigned)((n + SP_NT - 1) / SP_NT);
  if (pl->tab_state[p] != TAB_EMPTY && (rc = setplan_fill_table(pl, p, s)) != TFRA_OK) return rc;
  if (pl->tab_state[p ^ 1u] == TAB_LISTLESS && (rc = setplan_fill_table(pl, p ^ 1u, s)) != TFRA_OK) return rc;
  const unsigned use = ++pl->set_use[p];
  SetTab cur = pl->set_tab[p], old = pl->set_tab[p ^ 1u];
  cur.count = set_count_word(pl->set_counts, p, use);
  // the other table is walked through its list only when it has one; otherwise (never used, just filled) the list is empty: a word that is always zero
  old.count = pl->tab_state[p ^ 1u] == TAB_LISTED ? set_count_word(pl->set_counts, p ^ 1u, pl->set_use[p ^ 1u]) : pl->set_counts + SC_ZERO;
  pl->set_tab[p].count = cur.count;
  pl->tab_state[p] = TAB_LISTED; pl->tab_state[p ^ 1u] = TAB_EMPTY;
  pl->scat_ids = nullptr; pl->scat_n = 0;   // (pairs a step launch scattered for this object belong to a batch this build replaces)
  L->cur = cur; L->old = old; L->next_use_count = set_count_word(pl->set_counts, p, use + 1); L->m2 = pl->set_m2; L->blocks = blocks;
  pl->built_counts = counts;
  pl->set_parity = p;
  pl->d_counts = pl->set_counts; pl->dflag = pl->set_dflag; pl->slow_items = pl->set_items; pl->any_deferred = pl->set_counts + PC_ANY_DEFERRED;
  pl->n = n; pl->dim = 0; pl->kind = 1;
  return TFRA_OK;
}
// The same for a build WITHOUT the dense list and without atomics (the overlapped step: scatter launch + build launch): the
// table that takes the build (every slot of it is written by the build launch), the scatter buffers sized for n ids.
// (The table is sized for at least 131 072 ids — 128 windows — whatever the batch: a scatter tile holds up to 1024 DISTINCT ids, spread over
// the windows into segments of SEG_CAP = 32 entries.  A batch of 22 K all-distinct ids — what one rank of a sharded table serves —
// sized by its own length had 32 windows: 32 ids per segment on average, half the segments overflowed, and the launch took 36 us
// instead of 17: scripts/mb_owner_step.py.)
constexpr size_t LISTLESS_MIN_IDS = 131072;
int tfra::setplan_prepare_listless(tfra_sparse_plan* pl, size_t n, hipStream_t s) {
  int rc = setplan_ensure(pl, std::max(n, LISTLESS_MIN_IDS), s);
  if (rc) return rc;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  if (pl->seg_cap_ids < pl->set_cap) {
    if (pl->segbuf) { if (hipDeviceSynchronize() != hipSuccess || hipFree(pl->segbuf) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: free"); pl->segbuf = nullptr; }
    const size_t wins = pl->set_m2 / SET_WIN, tiles = (pl->set_cap + 1023) / 1024;
    const size_t bytes = 256 + 1024 + al(wins * tiles * SEG_CAP * sizeof(SetEnt)) + al(wins * tiles * 4) + al(pl->set_cap * sizeof(SetEnt));
    hipError_t e = hipMalloc(&pl->segbuf, bytes);
    if (e != hipSuccess) { pl->segbuf = nullptr; return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, "sparse_plan_build: hipMalloc"); }
    if (hipMemsetAsync(pl->segbuf, 0, bytes, s) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: memset");
    unsigned char* w = (unsigned char*)pl->segbuf;
    pl->ovf_cnt = (unsigned*)w; w += 256;
    pl->ucnt = (unsigned*)w; w += 1024;
    pl->seg_pairs = (SetEnt*)w; w += al(wins * tiles * SEG_CAP * sizeof(SetEnt));
    pl->seg_cnt = (unsigned*)w; w += al(wins * tiles * 4);
    pl->ovf_pairs = (SetEnt*)w;
    pl->seg_cap_ids = pl->set_cap;
  }
  return TFRA_OK;
}
// ... and the bookkeeping of the build launch: the object's other table takes the build
void tfra::setplan_take_listless(tfra_sparse_plan* pl, size_t n) {
  const unsigned p = pl->set_parity ^ 1u;
  pl->gen += 1;
  const unsigned use = ++pl->set_use[p];
  pl->set_tab[p].count = set_count_word(pl->set_counts, p, use);   // (unused by a list-less build: kept valid)
  pl->tab_state[p] = TAB_LISTLESS;
  pl->built_counts = false;
  pl->set_parity = p;
  pl->d_counts = pl->set_counts; pl->dflag = pl->set_dflag; pl->slow_items = pl->set_items; pl->any_deferred = pl->set_counts + PC_ANY_DEFERRED;
  pl->n = n; pl->dim = 0; pl->kind = 1;
}
int tfra::setplan_build(tfra_sparse_plan* pl, size_t n, const int64_t* ids, hipStream_t s, bool counts) {
  SetPlanLaunch L;
  int rc = setplan_prepare(pl, n, s, counts, &L);
  if (rc) return rc;
  if (counts) setplan_kernel<true><<<L.blocks, SP_NT, 0, s>>>(n, (const i64*)ids, L.m2, L.cur, L.old, L.next_use_count);
  else setplan_kernel<false><<<L.blocks, SP_NT, 0, s>>>(n, (const i64*)ids, L.m2, L.cur, L.old, L.next_use_count);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: launch failed");
  return TFRA_OK;
}

void tfra::setplan_fill_empty(void* ent, size_t n, hipStream_t s) { fill_setent_kernel<<<1, 64, 0, s>>>(static_cast<SetEnt*>(ent), n); }

// tf.unique WITHOUT the first-occurrence order (which nothing on the embedding path observes: the distinct ids feed Find / Insert,
// the inverse index feeds the gather — PY/dynamic_embedding_ops.py:99-117, PY/shadow_embedding_ops.py:316): the SET plan of the
// ids IS their de-duplication — one launch — and a second launch turns it into the inverse index.  Two launches instead of the
// three (formerly six) of tfra_unique, no look-back chain.
extern "C" int tfra_unique_unordered(tfra_workspace_t* ws, size_t n, const int64_t* ids, int64_t* unique_out, int32_t* idx_out,
                                     int64_t* d_num_unique, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !d_num_unique) return set_error(TFRA_ERR_INVALID, "unique: null argument");
  if (on_device(ws->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "unique: hipSetDevice");
  if (n == 0) { if (hipMemsetAsync(d_num_unique, 0, sizeof(int64_t), s) != hipSuccess) return set_error(TFRA_ERR_HIP, "unique: memset"); return TFRA_OK; }
  if (!ids || !unique_out || !idx_out) return set_error(TFRA_ERR_INVALID, "unique: null buffer");
  if (n > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, "unique_unordered: at most 2^18 ids per call (tfra_unique takes more)");
  if (!ws->h_err && hipHostMalloc(reinterpret_cast<void**>(&ws->h_err), 64, hipHostMallocDefault) == hipSuccess) *ws->h_err = 0;
  if (ws->h_err && __atomic_load_n(ws->h_err, __ATOMIC_RELAXED)) {   // an EARLIER one-launch call gave up waiting for another block's index
    __atomic_store_n(ws->h_err, 0u, __ATOMIC_RELAXED);
    return set_error(TFRA_ERR_HIP, "unique_unordered: an earlier call on this workspace timed out waiting for a block's index (its idx_out holds -1 entries)");
  }
  tfra_sparse_plan* pl = nullptr;
  int rc = workspace_uplan(ws, &pl);
  if (rc) return rc;
  SetPlanLaunch L;
  if ((rc = setplan_prepare(pl, n, s, false, &L))) return rc;
  if (L.blocks <= 128) {   // ONE launch (all blocks co-resident on half the chip: a block may wait for another's index)
    setplan_kernel<false, true, true><<<L.blocks, SP_NT, 0, s>>>(n, (const i64*)ids, L.m2, L.cur, L.old, L.next_use_count, (i64*)unique_out, idx_out,
                                                                 (i64*)d_num_unique, ws->h_err);
  } else {
    setplan_kernel<false, true><<<L.blocks, SP_NT, 0, s>>>(n, (const i64*)ids, L.m2, L.cur, L.old, L.next_use_count);
    unique_idx_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, (const i64*)ids, SetProbe{L.cur.ent, L.m2}, L.cur.ukeys, L.cur.count, (i64*)unique_out,
                                                                 idx_out, (i64*)d_num_unique);
  }
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "unique_unordered: launch failed");
  return TFRA_OK;
}

// TFRA>HkvHashTableEmbeddingLookup (tf_ops/fused_ops_rocm.cc) as ONE launch: Find of all n ids (tfra_table_find's results, default fill
// included) side by side with tfra_unique_unordered of the same ids (find_unique_kernel).  Shapes the one-launch de-duplication does
// not take (rows that are not 16-byte granules) go through the two calls one after the other: same results.
extern "C" int tfra_table_find_unique(tfra_table_t* tp, tfra_workspace_t* ws, size_t n, const int64_t* ids, void* rows_out, uint8_t* exists,
                                      const void* defaults, int default_is_full, int64_t* unique_out, int32_t* idx_out,
                                      int64_t* d_num_unique, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!tp || !ws || !d_num_unique) return set_error(TFRA_ERR_INVALID, "find_unique: null argument");
  Table* t = reinterpret_cast<Table*>(tp);
  if (t->device != ws->device) return set_error(TFRA_ERR_INVALID, "find_unique: table and workspace live on different devices");
  bool one = n != 0 && n <= MAX_IDS && n <= 256u * SP_NT && ids && rows_out && defaults && unique_out && idx_out;
  if (one) {
    const size_t x = (size_t)t->field_bytes | (size_t)(uintptr_t)rows_out | (size_t)(uintptr_t)defaults;
    one = (x & 15) == 0;
  }
  if (!one) {
    int rc = tfra_table_find(tp, n, ids, rows_out, exists, defaults, default_is_full, stream);
    if (rc) return rc;
    return tfra_unique_unordered(ws, n, ids, unique_out, idx_out, d_num_unique, stream);
  }
  std::lock_guard<std::mutex> lock(t->mu);
  { int rc = t->enter(s); if (rc) return rc; }
  tfra_sparse_plan* pl = nullptr;
  int rc = workspace_uplan(ws, &pl);
  if (rc) return rc;
  SetPlanLaunch L;
  if ((rc = setplan_prepare(pl, n, s, false, &L))) return rc;
  const TableView v = t->view_of(t->cur);
  const unsigned fblocks = (unsigned)((n + 16 * (SP_NT / 64) - 1) / (16 * (SP_NT / 64)));   // 16 keys per wave, 16 waves per block
  // one id per thread of a de-duplicating block up to 131072 ids, two above (<= 128 blocks by default; TFRA_FU_IPT=1 above 131072 ids: up to
  // 256, still co-resident).  Two everywhere (TFRA_FU_IPT=2, tuning)
  // makes this launch 0.3 us shorter and the Insert that follows 1.4 us longer (same box, twice): the order of the distinct ids changes
  static const int ipt_env = [] { const char* e = getenv("TFRA_FU_IPT"); return e ? atoi(e) : 0; }();
  const int ipt = ipt_env == 1 || ipt_env == 2 ? ipt_env : (n <= 128u * SP_NT ? 1 : 2);
  const unsigned ublocks = (unsigned)((n + SP_NT * ipt - 1) / (SP_NT * ipt));   // <= 128 (256 with TFRA_FU_IPT=1): dispatched first, co-resident whatever the find's blocks do
  const unsigned grid = ublocks + fblocks;
#define FU_LAUNCH(PF1, IPT) find_unique_kernel<16, PF1, IPT><<<grid, SP_NT, 0, s>>>(ublocks, n, (const i64*)ids, L.m2, L.cur, L.old, L.next_use_count, \
    (i64*)unique_out, idx_out, (i64*)d_num_unique, v, (unsigned char*)rows_out, exists, (const unsigned char*)defaults, default_is_full)
  if (t->dense) { if (ipt == 1) FU_LAUNCH(true, 1); else FU_LAUNCH(true, 2); }
  else { if (ipt == 1) FU_LAUNCH(false, 1); else FU_LAUNCH(false, 2); }
#undef FU_LAUNCH
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "find_unique: launch failed");
  return TFRA_OK;
}
