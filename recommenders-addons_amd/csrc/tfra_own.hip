// ASSIGN half of a write-back (tfra_table_upsert_planned, over a CSR plan of tfra_csr.hip or a SET plan of tfra_setplan.hip; tfra_table_upsert_sparse; a
// caller's unique keys, own_upsert_unique): one pass with bucket ownership (upsert_own_kernel, own_batch16 of tfra_own_device.h),
// then the keys it leaves over with the locked protocol (upsert_rest_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_optim_device.h"
#include "tfra_plan.h"
#include "tfra_reduce_device.h"

using namespace tfra;
using namespace tfra::red;

namespace {

__device__ __forceinline__ unsigned direct_count(const OwnArgs& a) {   // keys of a SRC_DIRECT launch
  if (!a.d_nkeys) return a.nkeys;
  const long long dn = *a.d_nkeys;
  return dn < 0 ? 0u : (unsigned)min((long long)a.nkeys, dn);
}

// the same for key g of a plan: key, last position and input score come from its record
template <int G>
__device__ __forceinline__ void locked_upsert_one(const TableView& v, const unsigned char* __restrict__ vals,
                                                  const u64* __restrict__ scores, const CsrKeys& ks, const AuxInitPod& ai,
                                                  const ScoreP& sp, unsigned g, int sub, int gshift, int& fresh, int& failed) {
  const i64 key = ks.dkeys[g];
  bool hot;
  const unsigned w = load_record(ks, g, sub, hot);
  const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
  unsigned last = (unsigned)__shfl((int)w, gshift + (hot ? 5 : 3));
  if (hot) last = ks.hent[last];
  last &= E_POS;
  const u64 in_one = scores ? scores[last] : 1;
  const u64 in_score = sp.strategy == TFRA_EVICT_LFU ? (scores ? in_one : (u64)cnt) : in_one;
  locked_upsert_kv<G>(v, vals, key, last, in_score, ai, sp, sub, gshift, fresh, failed);
}

// The keys the ownership pass leaves over: 32 blocks (a full grid on a small table, where they are most of the batch) of
// the locked protocol over the item list; the flags of ALL keys when the list overflowed.
template <int G, int SRC, bool ACC = false>
__global__ __launch_bounds__(256) void upsert_rest_kernel(const OwnArgs a, const unsigned* slow_ctr, unsigned* zero4) {
  // slow_ctr == nullptr: there was no ownership pass (no owner tags): EVERY key of the launch, with the locked protocol.
  // This kernel is a chain of dependent round trips for a handful of keys: the group's first item travels together with the
  // list's length (it is used only if the list turns out to reach that far), and the plan's key count is read only by the
  // launches that need it.
  const unsigned gi = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  uint4 f0 = make_uint4(0u, 0u, 0u, 0u), f1 = f0;
  if (slow_ctr) {
    const OwnItem* it = a.items + (gi < a.item_cap ? gi : 0u);
    f0 = reinterpret_cast<const uint4*>(it)[0];
    f1 = reinterpret_cast<const uint4*>(it)[1];
  }
  unsigned total = 0;
  if (!slow_ctr) total = SRC != SRC_DIRECT ? a.ks.d_counts[PC_HOT] + a.ks.d_counts[PC_COLD] : direct_count(a);
  const unsigned counted = slow_ctr ? *slow_ctr : total;
  if ((SRC == SRC_SET || SRC == SRC_DIRECT) && !ACC && slow_ctr && a.stats_host && blockIdx.x == 0 && threadIdx.x == 0) {   // the pass's sample -> the host (launch_own)
    __hip_atomic_store(a.stats_host, slow_ctr[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);       // not plain hits
    __hip_atomic_store(a.stats_host + 1, slow_ctr[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // keys looked at
  }
  if (zero4 && blockIdx.x == 0 && threadIdx.x < 4) zero4[threadIdx.x] = 0;   // last kernel of this use: arm the next use's counters
  if (counted == 0) return;
  const bool listed = slow_ctr && counted <= a.item_cap;
  if (slow_ctr && !listed) total = SRC != SRC_DIRECT ? a.ks.d_counts[PC_HOT] + a.ks.d_counts[PC_COLD] : direct_count(a);
  const unsigned n = listed ? counted : total;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned ngroups = (gridDim.x * blockDim.x) >> 4;
  int fresh = 0, failed = 0;
  for (unsigned i = gi; i < n; i += ngroups) {
    if (listed) {
      uint4 w0 = f0, w1 = f1;
      if (i != gi) {
        w0 = reinterpret_cast<const uint4*>(a.items + i)[0];
        w1 = reinterpret_cast<const uint4*>(a.items + i)[1];
      }
      const i64 key = (i64)(((u64)w0.y << 32) | w0.x);
      locked_upsert_kv<G>(a.v, a.vals, key, w0.z, ((u64)w1.y << 32) | w1.x, a.ai, a.sp, sub, gshift, fresh, failed, (w1.z & 1u) != 0, w1.w, nullptr,
                          ACC ? ((w1.z & 2u) ? 1 : 2) : 0, a.acc_dt);
      if (sub == 0) a.dflag[w0.w] = 0;
    } else {
      if (slow_ctr && a.dflag[i] != 4) continue;
      if (SRC == SRC_PLAN) locked_upsert_one<G>(a.v, a.vals, a.scores, a.ks, a.ai, a.sp, i, sub, gshift, fresh, failed);
      else if (SRC == SRC_SET) {
        const uint2 pc = set_pc(a.ks.sent + a.ks.uslot[i]);
        const u64 in_one = a.scores ? a.scores[pc.x - 1] : 1;
        locked_upsert_kv<G>(a.v, a.vals, a.ks.ukeys[i], pc.x - 1, a.sp.strategy == TFRA_EVICT_LFU ? (a.scores ? in_one : (u64)pc.y) : in_one,
                            a.ai, a.sp, sub, gshift, fresh, failed);
      } else locked_upsert_kv<G>(a.v, a.vals, a.keys[i], i, a.scores ? a.scores[i] : 1, a.ai, a.sp, sub, gshift, fresh, failed, false, 0, nullptr,
                                 ACC ? (a.exists[i] ? 1 : 2) : 0, a.acc_dt);
      if (slow_ctr && sub == 0) a.dflag[i] = 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) { fresh += __shfl_xor(fresh, off); failed += __shfl_xor(failed, off); }
  if (lane == 0) {
    if (fresh) size_add(a.v, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, fresh);
    if (failed) atomicAdd(a.v.err_count, (unsigned)failed);
  }
}

// HF (SRC_SET, round 6 — what the overlapped step's write-back role has done since round 5): a HIT claims nothing and reads no score
// line; a key that changes a bucket claims behind its decision, and a victim that is a key of this very batch (a probe of the batch's own
// SET plan) sends the new key to the remainder.  On a Zipf batch over resident ids (96 % hits) a key then touches its two key lines, its
// value row and its row instead of four lines, two claim words and the rows; a batch of mostly NEW keys pays one more dependent trip per
// wave (the score lines, then the claims) — the host picks the form from a sample of the previous write-back (launch_own).
// SAMPLE: the launch leaves the sample described below (compiled out where nobody reads it: a caller's keys on a table that evicts)
template <int G, bool SIMPLE, int SRC, int U = 4, bool ACC = false, bool HF = false, bool SAMPLE = false>
__global__ __launch_bounds__(256) void upsert_own_kernel(const OwnArgs a, OwnCtrs* ctr, unsigned own_gen, unsigned* progress,
                                                         unsigned progress_val) {
  const int lane = threadIdx.x & 63;
  const unsigned total = SRC != SRC_DIRECT ? a.ks.d_counts[PC_HOT] + a.ks.d_counts[PC_COLD] : direct_count(a);
  const unsigned nwaves = (gridDim.x * blockDim.x) >> 6;
  const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int fresh = 0, not_hits = 0, looked = 0;
  // every 128th wave tells how many of its keys were not plain hits — ONE 64-bit add per such wave (every 16th wave with two adds: ~180
  // same-line atomics piling up at the end of a one-round kernel, 9.9 -> 12.4 us for the DIRECT pass of 22 K keys under rocprofv3)
  const bool sampled = SAMPLE && (wave & 127u) == 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (progress) {   // see hot_sums_kernel; [1]: the keys of this write-back — the host sizes the next one's grid from it
      __hip_atomic_store(progress, progress_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(progress + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (SRC == SRC_PLAN && a.ks.d_counts[PC_OVERFLOW]) atomicAdd(a.v.err_count, a.ks.d_counts[PC_OVERFLOW]);
  }
  const OwnFlags fl = own_setup<SIMPLE>(a);
  for (unsigned wbase = wave * (4 * U); wbase < total; wbase += nwaves * (4 * U)) {
    const unsigned i = wbase + (unsigned)(lane & 15);
    const bool valid = (lane & 15) < 4 * U && i < total;
    own_batch16<G, SIMPLE, SRC, U, false, ACC, HF>(a, fl, min(i, total - 1), valid, own_gen, &ctr->n_a, lane, fresh, nullptr, nullptr, 0, 0,
                                                   (HF && a.own_set.ent) ? &a.own_set : nullptr, (SAMPLE && sampled) ? &not_hits : nullptr);
    if (SAMPLE) looked += (valid && lane < 16);
  }
  for (int off = 32; off > 0; off >>= 1) fresh += __shfl_xor(fresh, off);
  if (lane == 0 && fresh) size_add(a.v, wave, fresh);
  if (SAMPLE && sampled) {
    for (int off = 32; off > 0; off >>= 1) { not_hits += __shfl_xor(not_hits, off); looked += __shfl_xor(looked, off); }
    if (lane == 0 && looked)   // spare[1] (low word: keys looked at) | spare[2] (high word: not plain hits), 8-byte aligned
      atomicAdd(reinterpret_cast<unsigned long long*>(&ctr->spare[1]), ((unsigned long long)(unsigned)not_hits << 32) | (unsigned long long)(unsigned)looked);
  }
}

}  // namespace

// ---- launch of the ownership write-back (plan keys or a caller's unique keys) --------------------------------
template <int SRC>
static void launch_own(hipStream_t s, int g, bool simple, const OwnArgs& a, size_t nkeys, OwnCtrs* ctr, OwnCtrs* next_ctr, unsigned og,
                       unsigned rest_blocks, unsigned* progress, unsigned progress_val) {
  // 4 waves x 16 keys per block and pass; up to a batch's worth of keys 8 keys per wave instead (own_batch16: U): twice the
  // waves, half the dependent work in each, 86 instead of 118 registers.  Measured on the 10^9-slot table: 22.7 K keys
  // 13.1 -> 11.3 us (the step 42.5 -> 41.1), 78 K keys the same kernel time alone and the step 64.0 -> 60.7 us; 4 keys per
  // wave: nothing more on 22.7 K keys (40.8 us), 64.6 us on 78 K
  const bool half = g == 16 && nkeys <= 131072;
  const unsigned blocks = (unsigned)std::max<size_t>(1, half ? (nkeys + 31) / 32 : (nkeys + 63) / 64);
  // a.tags == nullptr (TFRA_OPTION_NO_OWNER_TAGS, or the tags did not allocate): the locked protocol for every key
  const bool smp = a.stats_host != nullptr && (SRC == SRC_SET || SRC == SRC_DIRECT) && g == 16;   // somebody reads the sample
#define TFRA_OWN(GG, SS, UU)                                                                                  \
  if (a.tags) {                                                                                               \
    if (GG == 16 && smp) upsert_own_kernel<GG, SS, SRC, UU, false, false, GG == 16><<<blocks, 256, 0, s>>>(a, ctr, og, progress, progress_val); \
    else upsert_own_kernel<GG, SS, SRC, UU><<<blocks, 256, 0, s>>>(a, ctr, og, progress, progress_val);       \
    upsert_rest_kernel<GG, SRC><<<rest_blocks, 256, 0, s>>>(a, &ctr->n_a, reinterpret_cast<unsigned*>(next_ctr)); \
  } else {                                                                                                    \
    upsert_rest_kernel<GG, SRC><<<(unsigned)std::max<size_t>(1, (nkeys + 15) / 16), 256, 0, s>>>(a, nullptr, nullptr); \
  }
  // The form of the pass (16-byte granules): HF when the last write-back that has ended was mostly plain hits — fewer than a quarter of
  // the keys its sample looked at were new, evicting or left over — (TFRA_OWN_HF=1: always, 0: never; tuning, tests).  Where it may be
  // taken: over a SET plan's keys (a victim is checked against the plan), and over ANY keys — a caller's unique keys included: the
  // reference's Insert op — on a table that never evicts (unbounded: TFRA's default cuckoo flavour), where the only thing a hit's claim
  // protected it from does not exist.
  // (A caller's unique keys on a table that DOES evict have no plan to check a victim against.  The form in which every key in need of
  // a victim goes to the remainder — no eviction inside the pass, so a hit still needs no claim — was measured on the metric's table,
  // picked below one such key in 64: find + Insert of prepared keys 33.4 -> 29.4 us, but the Insert behind the lookup op 41.5 -> 43.1 us
  // and the pair alone 16.4 -> 19.1 us.  Not taken; TFRA_OWN_HF=1 still forces it, for the tests.)
  const char* hf_env = getenv("TFRA_OWN_HF");
  const bool hf_forced = hf_env && *hf_env && atoi(hf_env) != 0;
  if ((SRC == SRC_SET || SRC == SRC_DIRECT) && g == 16 && a.tags && (hf_forced || (SRC == SRC_SET && a.own_set.ent) || a.sp.bounded == 0)) {
    const char* e = hf_env;
    bool hf = false;
    if (e && *e) hf = atoi(e) != 0;
    else if (a.stats_host) {
      const unsigned nh = reinterpret_cast<const volatile unsigned*>(a.stats_host)[0], lk = reinterpret_cast<const volatile unsigned*>(a.stats_host)[1];
      hf = lk >= 32 && (size_t)nh * 4 < (size_t)lk;
    }
    if (hf) {
#define TFRA_OWN_HF_LAUNCH(SS, UU) upsert_own_kernel<16, SS, SRC, UU, false, true, true><<<blocks, 256, 0, s>>>(a, ctr, og, progress, progress_val)
      if (simple) { if (half) TFRA_OWN_HF_LAUNCH(true, 2); else TFRA_OWN_HF_LAUNCH(true, 4); }
      else { if (half) TFRA_OWN_HF_LAUNCH(false, 2); else TFRA_OWN_HF_LAUNCH(false, 4); }
#undef TFRA_OWN_HF_LAUNCH
      upsert_rest_kernel<16, SRC><<<rest_blocks, 256, 0, s>>>(a, &ctr->n_a, reinterpret_cast<unsigned*>(next_ctr));
      return;
    }
  }
  switch (g) {
    case 16:
      if (simple) { if (half) { TFRA_OWN(16, true, 2); } else { TFRA_OWN(16, true, 4); } }
      else { if (half) { TFRA_OWN(16, false, 2); } else { TFRA_OWN(16, false, 4); } }
      break;
    case 8: TFRA_OWN(8, false, 4); break;
    case 4: TFRA_OWN(4, false, 4); break;
    case 2: TFRA_OWN(2, false, 4); break;
    default: TFRA_OWN(1, false, 4); break;
  }
#undef TFRA_OWN
}

// the same pair as the reference's insert_or_accum (own_batch16: ACC) over a caller's unique keys; 16-byte granules only
static void launch_own_accum(hipStream_t s, bool simple, const OwnArgs& a, size_t nkeys, OwnCtrs* ctr, OwnCtrs* next_ctr, unsigned og,
                             unsigned rest_blocks) {
  const bool half = nkeys <= 131072;
  const unsigned blocks = (unsigned)std::max<size_t>(1, half ? (nkeys + 31) / 32 : (nkeys + 63) / 64);
#define TFRA_OWN_ACC(SS, UU) upsert_own_kernel<16, SS, SRC_DIRECT, UU, true><<<blocks, 256, 0, s>>>(a, ctr, og, nullptr, 0)
  if (simple) { if (half) TFRA_OWN_ACC(true, 2); else TFRA_OWN_ACC(true, 4); }
  else { if (half) TFRA_OWN_ACC(false, 2); else TFRA_OWN_ACC(false, 4); }
#undef TFRA_OWN_ACC
  upsert_rest_kernel<16, SRC_DIRECT, true><<<rest_blocks, 256, 0, s>>>(a, &ctr->n_a, reinterpret_cast<unsigned*>(next_ctr));
}

// Expected left-over keys of an ownership pass over `nkeys` keys: two keys sharing a home bucket, (2 n)^2 / (2 nb).
static double expect_leftover(double nkeys, double nb) { return 2.0 * nkeys * nkeys / nb; }

static unsigned next_own_gen(Table* t) {
  if (++t->own_gen == 0) t->own_gen = 1;     // bucket-owner tag of this launch (tags start at 0; a stale equal tag after a wrap only
  return t->own_gen;                         // sends a key to the remainder pass)
}

int tfra::own_prepare(Table* t, const tfra_sparse_plan_t* pl, const void* values, const uint64_t* scores, hipStream_t s,
                       const unsigned* progress, OwnLaunch* L) {
  // caller holds t->mu and has called t->enter(s)
  if (!values) return set_error(TFRA_ERR_INVALID, "upsert_planned: null values");
  if (t->opts.device != pl->device && t->opts.device >= 0) return set_error(TFRA_ERR_INVALID, "upsert_planned: plan and table live on different devices");
  if (pl->kind == 1 && !pl->built_counts && t->opts.strategy == TFRA_EVICT_LFU && !scores)
    return set_error(TFRA_ERR_INVALID, "upsert_planned: this plan was built without occurrence counts (by a step driver of a table whose scores do not read them); an LFU table without caller scores needs them");
  int rc = t->prepare_insert(pl->n, s);
  if (rc) return rc;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  if (pl->kind == 1 && progress) {
    // an assign-only plan does not tell the host how many distinct keys it found; the step driver's batches resemble each
    // other: the count the last write-back that has started saw, plus a quarter (a batch with more: grid-stride)
    const unsigned seen = reinterpret_cast<const volatile unsigned*>(progress)[1];
    if (seen) key_blocks = (unsigned)std::max<size_t>(1, (std::min<size_t>(pl->n, (size_t)seen + seen / 4 + 1024) * 16 + 255) / 256);
  }
  uint8_t* bounded_now;
  rc = t->bounded_flags(1, s, &bounded_now);
  if (rc) return rc;
  const ScoreP sp = score_of(t, bounded_now);
  const int g = granule_of(t->field_bytes, values, nullptr);
  ++pl->use_gen;
  unsigned* tags = t->ensure_own_tags(s);    // nullptr (no owner tags): every key takes the locked protocol
  L->og = tags ? next_own_gen(t) : 0;
  const unsigned par = pl->ups_uses[pl->kind == 1 ? 1 : 0]++ & 1u;   // (its own count per buffer: apply_planned uses of the plan do not touch the counters)
  L->ctr = reinterpret_cast<OwnCtrs*>(pl->d_counts + PC_OWN_CTRS) + par;
  L->next_ctr = reinterpret_cast<OwnCtrs*>(pl->d_counts + PC_OWN_CTRS) + (par ^ 1u);
  // Left-over keys of the ownership pass.  Few (a big table): the remainder kernel walks their list with a handful of
  // blocks.  Many (a small table): full grid.
  const double nkeys = (double)key_blocks * 16.0;   // unique keys of the plan when its counts have arrived, else the id count
  L->rem_blocks = expect_leftover(nkeys, (double)t->cur.nb) < 2048.0 ? 32u : key_blocks;
  L->key_blocks = key_blocks;
  L->simple = t->opts.aux_fields == 0 && t->opts.strategy == TFRA_EVICT_LRU && !scores;
  L->g = g;
  OwnArgs& a = L->a;
  a = OwnArgs{};
  a.v = t->view_of(t->cur); a.vals = (const unsigned char*)values; a.scores = (const u64*)scores; a.ks = keys_of(pl); a.keys = nullptr; a.nkeys = 0;
  a.ai = t->aux; a.sp = sp;
  a.dflag = pl->dflag; a.tags = tags; a.items = pl->slow_items; a.item_cap = SLOW_CAP;
  if (pl->kind == 1) {   // a SET plan: its table as something to probe (HF), and where the pass's sample goes
    const SetTab& tb = pl->set_tab[pl->set_parity];
    a.own_set = SetProbe{tb.ent, pl->set_m2};
    a.stats_host = t->own_stats_host;
  }
  return TFRA_OK;
}

int tfra::upsert_planned_impl(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const void* values, const uint64_t* scores,
                               tfra_stream_t stream, unsigned* progress, unsigned progress_val) {
  // caller holds t->mu
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t || !pl) return set_error(TFRA_ERR_INVALID, "upsert_planned: null argument");
  hipStream_t s = (hipStream_t)stream;
  int rc = t->enter(s);
  if (rc) return rc;
  if (pl->n == 0) return TFRA_OK;
  OwnLaunch L;
  rc = own_prepare(t, pl, values, scores, s, progress, &L);
  if (rc) return rc;
  if (pl->kind == 1) launch_own<SRC_SET>(s, L.g, L.simple, L.a, (size_t)L.key_blocks * 16, L.ctr, L.next_ctr, L.og, L.rem_blocks, progress, progress_val);
  else launch_own<SRC_PLAN>(s, L.g, L.simple, L.a, (size_t)L.key_blocks * 16, L.ctr, L.next_ctr, L.og, L.rem_blocks, progress, progress_val);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "upsert_planned: launch failed");
  t->step_epoch();
  return TFRA_OK;
}

// tfra_table_insert_or_assign with TFRA_FLAG_UNIQUE_KEYS (the reference's Insert op hands HKV unique keys,
// hkv_hashtable_op_gpu.cu.cc:253-290 -> lookup_table_op_hkv.h:522-537): the same single pass with bucket ownership, fed
// with the caller's key array — value row i belongs to key i, no plan.  *taken = false: not for this call (no owner tags,
// or so many keys for the table's size that most of them would collide on a home bucket: a bulk load) — the caller runs
// the locked two-phase kernels.  Caller holds t->mu and has called prepare_insert.
namespace tfra {
int own_upsert_unique(Table* t, hipStream_t s, size_t n, const i64* keys, const void* values, const u64* scores, bool* taken,
                      const uint8_t* accum_exists, const int64_t* d_n) {
  // accum_exists != nullptr: insert_or_accum (tfra_table_accum_or_assign with TFRA_FLAG_UNIQUE_KEYS) instead of an assign
  *taken = false;
  if (accum_exists && (((size_t)t->field_bytes | (size_t)(uintptr_t)values) & 15)) return TFRA_OK;   // 16-byte granules only
  if (n == 0 || n > (1u << 24)) return TFRA_OK;
  const double expect = expect_leftover((double)n, (double)t->cur.nb);
  if (expect >= 2048.0) return TFRA_OK;   // most keys would collide on a home bucket (a bulk load): the locked kernels
  // the table's own scratch of this path: 2 counter sets | item list | one flag byte per key
  const size_t head = 256 + (size_t)SLOW_CAP * sizeof(OwnItem);
  const size_t need = head + ((n + 255) / 256) * 256;
  if (t->capture_safe && (t->own_ws_bytes < need || !t->own_tags || t->own_tags_nb != t->cur.nb)) return TFRA_OK;   // no allocation while capturing
  unsigned* tags = t->ensure_own_tags(s);
  if (!tags) return TFRA_OK;
  if (t->own_ws_bytes < need) {
    if (t->own_ws) { if (hipStreamSynchronize(s) != hipSuccess) return set_error(TFRA_ERR_HIP, "insert: sync"); t->dfree(t->own_ws, s); t->own_ws = nullptr; t->own_ws_bytes = 0; }
    const size_t want = head + std::max<size_t>(((n + 255) / 256) * 256, (size_t)1 << 18);
    t->own_ws = t->dalloc(want, s);
    if (!t->own_ws) { g_last_error.clear(); return TFRA_OK; }   // no scratch: the locked kernels need none
    if (hipMemsetAsync(t->own_ws, 0, want, s) != hipSuccess) return set_error(TFRA_ERR_HIP, "insert: memset");   // counters and flags start at zero
    t->own_ws_bytes = want;
    t->own_ws_uses = 0;
  }
  uint8_t* bounded_now;
  int rc = t->bounded_flags(1, s, &bounded_now);
  if (rc) return rc;
  const ScoreP sp = score_of(t, bounded_now);
  const int g = granule_of(t->field_bytes, values, nullptr);
  const unsigned og = next_own_gen(t);
  const unsigned par = t->own_ws_uses++ & 1u;
  OwnCtrs* ctr = reinterpret_cast<OwnCtrs*>(t->own_ws) + par;
  OwnCtrs* next_ctr = reinterpret_cast<OwnCtrs*>(t->own_ws) + (par ^ 1u);
  const bool simple = t->opts.aux_fields == 0 && t->opts.strategy == TFRA_EVICT_LRU && !scores;
  OwnArgs a{};
  a.v = t->view_of(t->cur); a.vals = (const unsigned char*)values; a.scores = scores; a.keys = keys; a.nkeys = (unsigned)n;
  a.ai = t->aux; a.sp = sp; a.dflag = (uint8_t*)t->own_ws + head; a.tags = tags;
  a.items = reinterpret_cast<OwnItem*>((unsigned char*)t->own_ws + 256); a.item_cap = SLOW_CAP;
  a.exists = accum_exists; a.acc_dt = t->opts.value_dtype; a.d_nkeys = (const long long*)d_n;
  a.stats_host = sp.bounded == 0 ? t->own_stats_host : nullptr;   // (a table that evicts never takes the other form for a caller's keys: nothing to sample for)
  if (accum_exists) launch_own_accum(s, simple, a, n, ctr, next_ctr, og, 32u);
  else launch_own<SRC_DIRECT>(s, g, simple, a, n, ctr, next_ctr, og, 32u, nullptr, 0);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "insert: launch failed");
  *taken = true;
  return TFRA_OK;
}
}  // namespace tfra

extern "C" int tfra_table_upsert_planned(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const void* values,
                                         const uint64_t* scores, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "upsert_planned: null table");
  std::lock_guard<std::mutex> lock(t->mu);
  return upsert_planned_impl(tp, pl, values, scores, stream, nullptr, 0);
}
// insert_or_assign of a batch whose keys may repeat, last occurrence wins, dedup on the device
extern "C" int tfra_table_upsert_sparse(tfra_table_t* tp, size_t n, const int64_t* ids, const void* values,
                                        const uint64_t* scores, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "upsert_sparse: null table");
  if (n == 0) return TFRA_OK;
  if (!ids || !values) return set_error(TFRA_ERR_INVALID, "upsert_sparse: null buffer");
  tfra_sparse_plan* pl;
  std::lock_guard<std::mutex> lock(t->mu);
  int rc = t->enter((hipStream_t)stream);
  if (rc) return rc;
  rc = own_plan(t, &pl);
  if (rc) return rc;
  // more ids than a plan holds: chunk after chunk on the stream — a later chunk overwrites an earlier one, which is
  // "the last occurrence wins" across chunks too
  for (size_t off = 0; off < n; off += MAX_IDS) {
    const size_t m = std::min<size_t>(MAX_IDS, n - off);
    pl->skip_counts_once = !(t->opts.strategy == TFRA_EVICT_LFU && !scores);   // what reads a key's occurrence count (own_batch16)
    rc = tfra_sparse_plan_build(pl, m, ids + off, 0, stream);
    if (rc) return rc;
    rc = upsert_planned_impl(tp, pl, (const unsigned char*)values + off * (size_t)t->field_bytes, scores ? scores + off : nullptr, stream,
                             nullptr, 0);
    if (rc) return rc;
  }
  return TFRA_OK;
}
