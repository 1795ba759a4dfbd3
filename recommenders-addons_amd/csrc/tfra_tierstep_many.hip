// The grouped admission over tiers: tfra_multi_tier_find_or_insert, the tfra_tier_find_or_insert (tfra_tierstep.hip,
// DESIGN §4.20) of a LIST of tiers as ONE stream-ordered chain: one record upload, then every stage of the single chain once per
// launch class — 6 launches (7 with TFRA_TIER_VERIFY) for a list of aligned float32 tiers whose uppers are full, however long the
// list is, where the loop of single calls enqueues 6 (7) per tier.
// Every kernel here has the launch shape of the grouped calls (tfra_many.h): many_desc_of takes the block to its descriptor, the
// record is read with wave-uniform loads, and the stage's device body runs on a block index local to the descriptor.  A block
// touches only its own descriptor's tables and staging — the call refuses a table that stands twice — so nothing inside a launch
// depends on another descriptor, and the locked protocol of the upserts waits on slots of its own table only, as in the single call.
// The bodies: stages 1 and 5 are find_missed_body (tfra_tier_device.h), the code find_missed_kernel / find_missed_touch_kernel run.
// Stages 2, 3 and 4 are TWINS of tier_fetch_kernel (tfra_tierstep.hip), insert_counted_kernel<G, 4, true> and
// insert_evict_rows_kernel<G> (tfra_upsert.hip): handing those kernels a shared body changed their generated code (registers; by-value
// structs went to LDS: profiles/tier_admit_many_isa_stats.txt), so the body stands twice, as insert_counted_kernel stands beside
// insert_unique_kernel.  A fix in one belongs in the other.
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_tier.h"
#include "tfra_tier_device.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;

namespace {

// One active descriptor: what the single chain's launches take as kernel arguments.
struct TierAdmitRec {
  TableView up, lo;             // taken under the locks, behind both tables' prepare_insert
  AuxInit aux;                  // the upper table's: the slot vectors a never-seen key starts with
  u64* words;                   // the driver's words (TS_*, TC_*)
  size_t n;                     // the buffers' length
  const long long* d_n;         // may be null
  const i64* keys;
  const unsigned char* init;
  unsigned char* out;           // may be null
  uint8_t* where;               // may be null
  i64* miss_keys;
  int* miss_idx;
  unsigned char* up_rows;
  i64* down_keys;
  unsigned char* down_rows;
  u64* down_scores;
  uint8_t* deferred;            // the upper table's phase-2 flags; null off max_capacity
  u64 up_epoch, lo_epoch;
  u64 max_batch;
  int full, up_strategy, lo_strategy, up_bounded;   // up_bounded: bounded_mode of the upper table (0: it can still grow)
  unsigned whole;
};

// ---- stage 0: tier_begin_kernel's work, one thread per active descriptor ----------------------------------------------------------
__global__ __launch_bounds__(256) void tier_begin_many_kernel(const TierAdmitRec* __restrict__ recs, unsigned n) {
  const unsigned d = blockIdx.x * 256 + threadIdx.x;
  if (d >= n) return;
  u64* w = recs[d].words;
  w[TS_CALLS] += 1;
  w[TS_MISSED] += w[TC_MISSED];
  w[TS_DEMOTED] += w[TC_DOWN];
  w[TC_MISSED] = 0;
  w[TC_DOWN] = 0;
}

// ---- stages 1 and 5: find_missed over all upper tables ----------------------------------------------------------------------------
// TOUCH (stage 1): find_missed_touch_kernel — rows and `where` of the hits, their scores touched, the misses to the tier's own list
// behind its own TC_MISSED (ONE counter add per block).  Not TOUCH (stage 5): the count-only find_missed_kernel into TS_NOT_RESIDENT.
template <int G, bool PF1, bool TOUCH>
__global__ __launch_bounds__(256 * TIER_TILES) void tier_find_missed_many_kernel(const TierAdmitRec* __restrict__ recs,
                                                                                 const unsigned* __restrict__ prefix,
                                                                                 const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const TierAdmitRec rec = recs[idx[d]];
  const unsigned blk = blockIdx.x - prefix[d];
  if constexpr (TOUCH) {
    const MissOut mo{rec.words + TC_MISSED, rec.max_batch, rec.miss_keys, rec.miss_idx, nullptr};
    find_missed_body<G, 4, PF1, TIER_TILES>(rec.up, rec.n, rec.keys, rec.out, rec.where, rec.init, rec.full, rec.d_n, mo,
                                            TierMissedTouch{nullptr, 0u, rec.up_strategy, rec.up_epoch}, blk);
  } else {
    const MissOut mo{rec.words + TS_NOT_RESIDENT, 0, nullptr, nullptr, nullptr};
    find_missed_body<G, 4, PF1, TIER_TILES>(rec.up, rec.n, rec.keys, nullptr, nullptr, nullptr, 0, rec.d_n, mo, TierMissed{nullptr, 0u}, blk);
  }
}

// ---- stage 2: tier_fetch over all lower tables (the twin of tier_fetch_kernel) ------------------------------------------------------
template <int G, int U, bool PF1, int TILES>
__device__ __forceinline__ void tier_fetch_body(const TableView& v, const FetchIO& io, const AuxInit& ai, const unsigned blk) {
  constexpr int NW = 4 * TILES;
  __shared__ unsigned s_hits[NW];
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4, w = threadIdx.x >> 6;
  const unsigned wave = blk * NW + w;
  const size_t n = min(io.cap, (size_t)*io.d_count);   // uniform
  TierFetch x;
  x.pos_of = io.pos_of;
  x.where = io.where;
  find_wave<G, U, G == 16, PF1, TierFetch>(v, n, io.keys, io.out, nullptr, io.defaults, io.full, 0u, wave, &x);
  unsigned hits = 0;
  if ((size_t)wave * (4 * U) < n) {   // (the waves find_wave served: x.word / x.pos are set)
    const unsigned whole = v.n_fields * v.field_bytes;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t j = (size_t)wave * (4 * U) + (unsigned)(u * 4 + grp);
      const bool valid = j < n;   // (a clamped tail position is not a key)
      const bool hit = valid && x.word[u] >= 0;
      hits += (unsigned)__popcll(__ballot(hit && sub == 0));
      if (!io.stage || !valid) continue;
      unsigned char* srow = io.stage + j * whole;
      if (hit) {
        copy_bytes16<G>(srow, word_row_ptr(v, (u64)x.word[u]), whole, sub);
      } else {
        copy_bytes16<G>(srow, io.defaults + (io.full ? (size_t)x.pos[u] * v.field_bytes : 0), v.field_bytes, sub);
        for (unsigned f = 1; f < v.n_fields; ++f)
          fill_aux_field(srow + f * v.field_bytes, v.field_bytes, ai.pattern[(f - 1) & 3], ai.elem_bytes, G >= 4 && (v.field_bytes & 3) == 0, sub);
      }
    }
  }
  if (lane == 0) s_hits[w] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) total += s_hits[i];
    if (total) atomicAdd(io.lower_hits, (u64)total);
  }
}
// The grid comes from the host's bound of each descriptor (blocks_of(n)); the count of the miss list is read on the device.
template <int G, bool PF1>
__global__ __launch_bounds__(256 * TIER_TILES) void tier_fetch_many_kernel(const TierAdmitRec* __restrict__ recs,
                                                                           const unsigned* __restrict__ prefix,
                                                                           const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const TierAdmitRec& rec = recs[idx[d]];   // (a reference: the body indexes aux.pattern with a variable, which a copy in registers cannot serve)
  const FetchIO io{rec.miss_keys, rec.miss_idx, rec.words + TC_MISSED, (size_t)min((u64)rec.n, rec.max_batch), rec.out, rec.where,
                   rec.init, rec.full, rec.up_rows, rec.words + TS_LOWER_HITS};
  tier_fetch_body<G, 4, PF1, TIER_TILES>(rec.lo, io, rec.aux, blockIdx.x - prefix[d]);
}

// ---- stages 3 and 4, phase 1: the twin of insert_counted_kernel<G, U, true> ------------------------------------------------------------
// Whole co-located rows of the min(n_buf, *d_n) leading keys into the table (in_score 1), the flags of the entries beyond the count
// cleared for phase 2.  wave: the wave's index among the waves of THIS key list.
template <int G, int U>
__device__ __forceinline__ void insert_whole_counted_body(const TableView& v, size_t n_buf, const i64* __restrict__ keys,
                                                          const unsigned char* __restrict__ vals, int strategy, u64 epoch, int bounded,
                                                          uint8_t* __restrict__ deferred, const long long* __restrict__ d_n,
                                                          const size_t wave) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  constexpr int KPW = 4 * U;
  const size_t base = wave * KPW;
  const long long dn = *d_n;   // uniform load, as find_kernel's
  const size_t n = dn < 0 ? 0 : min(n_buf, (size_t)dn);
  if (deferred && lane < KPW && base + lane >= n && base + lane < n_buf) deferred[base + lane] = 0;
  if (base >= n) return;
  const size_t last = n - 1;
  const unsigned src_bytes = v.n_fields * v.field_bytes;   // one row of vals
  i64 kreg = keys[min(base + (size_t)(lane & (KPW - 1)), last)];
  int fresh = 0, failed = 0;
  i64 key[U], k0[U], k1[U];
  u64 h[U], b0[U];
  const bool pf1 = bounded > 1;
#pragma unroll
  for (int u = 0; u < U; ++u) {  // U first probes in flight (unconditional, tail clamped)
    key[u] = shfl_i64(kreg, u * 4 + grp);
    b0[u] = bucket0(key[u], v.nb, h[u]);
    k0[u] = load_key_coherent(key_line(v, b0[u]) + sub);
    k1[u] = load_key_coherent(key_line(v, pf1 ? bucket1(h[u], b0[u], v.nb) : b0[u]) + sub);
  }
  keep_live(k0[0], k0[1], k0[2], k0[3]);
  keep_live(k1[0], k1[1], k1[2], k1[3]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t i = base + (size_t)(u * 4 + grp);
    if (i >= n) continue;
    bool is_new;
    const i64 row = locate_or_claim_from(v, key[u], h[u], b0[u], k0[u], sub, gshift, is_new, bounded, pf1 ? &k1[u] : nullptr);
    if (deferred && sub == 0) deferred[i] = row == NEED_EVICT;
    if (row >= 0) {
      copy_bytes16<G>(row_ptr(v, row), vals + i * (size_t)src_bytes, src_bytes, sub);
      update_score(v, row, is_new, strategy, 1, epoch, sub);
      fresh += (is_new && sub == 0);
    } else if (row != NEED_EVICT) {
      failed += (sub == 0);
    }
  }
  wave_account(v, wave, lane, fresh, failed);
}
// LOWER false (stage 3): each tier's staged rows into its upper table.  LOWER true (stage 4): its down-list, TC_DOWN long, into its
// lower table (which can still grow: no flags, no phase 2).
template <int G, bool LOWER>
__global__ __launch_bounds__(256) void tier_insert_many_kernel(const TierAdmitRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                               const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const TierAdmitRec rec = recs[idx[d]];
  const size_t wave = ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 6;
  if constexpr (LOWER)
    insert_whole_counted_body<G, 4>(rec.lo, rec.n, rec.down_keys, rec.down_rows, rec.lo_strategy, rec.lo_epoch, 0, nullptr,
                                    (const long long*)(rec.words + TC_DOWN), wave);
  else
    insert_whole_counted_body<G, 4>(rec.up, rec.n, rec.miss_keys, rec.up_rows, rec.up_strategy, rec.up_epoch, rec.up_bounded, rec.deferred,
                                    (const long long*)(rec.words + TC_MISSED), wave);
}

// ---- stage 3, phase 2: the twin of insert_evict_rows_kernel<G> (insert_evict_body<G, true, true>, in_score 1) --------------------------
// The keys whose flag is set replace the minimum-score entry of their home buckets by their whole row; every entry that leaves the
// table, and every key that is not admitted, is appended to `eo` as a whole row.  i: the key of this 16-lane group.
template <int G>
__device__ __forceinline__ void insert_evict_whole_body(const TableView& v, size_t n, const i64* __restrict__ keys,
                                                        const unsigned char* __restrict__ vals, int strategy, u64 epoch,
                                                        const uint8_t* __restrict__ deferred, const EvictOut& eo, const size_t i) {
  const unsigned src_bytes = v.n_fields * v.field_bytes;   // one row of vals
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  int fresh = 0, failed = 0;
  const bool lru_like = strategy == TFRA_EVICT_LRU || strategy == TFRA_EVICT_EPOCHLRU;
  const bool active = i < n && deferred[i];
  i64 key = 0, victim = EMPTY_KEY, row = -3;
  const u64 in_score = 1;
  u64 compare = 0, word = 0;
  bool claimed_empty = false;
  if (active) {
    key = keys[i];
    compare = strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score;
    row = evict_and_lock(v, key, compare, lru_like, sub, gshift, &word, claimed_empty, nullptr, nullptr, &victim);
  }
  // Output positions: ONE counter add per wave.  The wave's groups have left evict_and_lock together (they wait for each other at
  // the end of its loop), so the ballot makes no lock holder wait for anything it did not wait for before.
  const bool report = active && ((row >= 0 && !claimed_empty) || row == -1);
  const u64 m = __ballot(report && sub == 0);
  u64 pos = 0;
  if (m) {
    unsigned lo = 0, hi = 0;
    if (lane == 0) {
      const u64 b = atomicAdd(eo.counter, (u64)__popcll(m));
      lo = (unsigned)b; hi = (unsigned)(b >> 32);
    }
    pos = (((u64)(unsigned)__shfl((int)hi, 0) << 32) | (unsigned)__shfl((int)lo, 0)) + (u64)__popcll(m & ((1ULL << gshift) - 1));
  }
  const bool wr = report && eo.keys && pos < eo.cap;
  unsigned char* out_row = eo.vals ? eo.vals + pos * (u64)eo.row_bytes : nullptr;
  if (row >= 0) {
    if (wr) {
      // the slot is LOCKED: its row and score are stable (evict_and_lock re-read the score under the lock).  Read before write.
      if (sub == 0) {
        eo.keys[pos] = victim;
        if (eo.scores) eo.scores[pos] = __hip_atomic_load(score_word(v, word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (out_row) copy_bytes16_coherent<G>(out_row, row_ptr(v, row), eo.row_bytes, sub);
    }
    replace_locked<G, true>(v, row, word, key, vals + i * (size_t)src_bytes, 0u, AuxInit{}, strategy, in_score, epoch, sub);
    fresh = (claimed_empty && sub == 0);
  } else if (active && row == -3) {
    failed = (sub == 0);
  } else if (wr) {   // -1, not admitted: the caller's own key, whole row and compare score.  No table read.
    if (sub == 0) {
      eo.keys[pos] = key;
      if (eo.scores) eo.scores[pos] = compare;
    }
    if (out_row) copy_bytes16<G>(out_row, vals + i * (size_t)src_bytes, eo.row_bytes, sub);
  }
  wave_account(v, i >> 2, lane, fresh, failed);
}
template <int G>
__global__ __launch_bounds__(256) void tier_evict_many_kernel(const TierAdmitRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                              const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const TierAdmitRec rec = recs[idx[d]];
  const EvictOut eo{rec.words + TC_DOWN, rec.max_batch, rec.down_keys, rec.down_rows, rec.down_scores, rec.whole};
  insert_evict_whole_body<G>(rec.up, rec.n, rec.miss_keys, rec.up_rows, rec.up_strategy, rec.up_epoch, rec.deferred, eo,
                             ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// A stage's class of a descriptor: the granule ladder of with_granule, 16 split by PF1 (a dense table: both home-bucket lines of a
// key in flight together) where the stage has that axis.  0: <16, PF1>, 1: <16>, 2: <8>, 3: <4>, 4: <2>, 5: <1>.
constexpr int NGC = 6;
int granule_class(int g, bool pf1) { return g == 16 ? (pf1 ? 0 : 1) : g == 8 ? 2 : g == 4 ? 3 : g == 2 ? 4 : 5; }
template <class F>
void with_granule_class(int c, F&& f) {
  if (c == 0) f(std::integral_constant<int, 16>{}, std::true_type{});
  else with_granule(16 >> (c - 1), [&](auto G) { f(G, std::false_type{}); });
}

struct Member {
  tfra_tier* tier;
  const tfra_tier_find_or_insert_desc* d;
  int c_find = 0, c_fetch = 0, c_put = 0, c_verify = 0;
};

}  // namespace

extern "C" int tfra_multi_tier_find_or_insert(tfra_workspace_t* ws, size_t n_tiers, const tfra_tier_find_or_insert_desc* descs,
                                              uint32_t* launches_out, tfra_stream_t stream) {
  const std::string who = "multi_tier_find_or_insert";
  if (launches_out) *launches_out = 0;
  if (n_tiers == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and no table, statistic or output changes
  std::vector<Member> act;
  std::map<const void*, size_t> seen_tier, seen_table;   // where a tier / a table of the call stands
  for (size_t i = 0; i < n_tiers; ++i) {
    const tfra_tier_find_or_insert_desc& d = descs[i];
    const std::string at_i = who + ": descriptor " + std::to_string(i) + ": ";
    if (d.struct_size != sizeof(tfra_tier_find_or_insert_desc)) return set_error(TFRA_ERR_INVALID, at_i + "descriptor size mismatch");
    if (d.reserved) return set_error(TFRA_ERR_INVALID, at_i + "reserved must be 0");
    const Check c = check_tier_find_or_insert(d.tier, d.n, d.keys, d.init_values, d.flags);
    if (c.code) return report(at_i, c);
    if (!c.active) continue;
    if (d.tier->upper->device != ws->device) return set_error(TFRA_ERR_INVALID, at_i + "workspace and tier live on different devices");
    // this call WRITES: a tier, and a table in any role, stands once in it (a block touches its own descriptor's tables only)
    if (!seen_tier.emplace(d.tier, i).second)
      return set_error(TFRA_ERR_INVALID, at_i + "the same tier as descriptor " + std::to_string(seen_tier[d.tier]));
    for (Table* t : {d.tier->upper, d.tier->lower})
      if (!seen_table.emplace(t, i).second)
        return set_error(TFRA_ERR_INVALID, at_i + "a table of this tier stands in descriptor " + std::to_string(seen_table[t]) +
                                               " too (a call that writes takes every table once)");
    act.push_back(Member{d.tier, &d});
  }
  const size_t n_act = act.size();
  if (n_act == 0) return TFRA_OK;
  u64 put_blocks = 0;
  for (const Member& m : act) put_blocks += (m.d->n + 15) / 16;   // phase 2's grid, the largest
  if (put_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, who + ": too many keys in one call");

  TierLocks locks;
  {
    std::vector<tfra_tier*> tiers;
    std::vector<Table*> tabs;
    for (const Member& m : act) { tiers.push_back(m.tier); tabs.push_back(m.tier->upper); tabs.push_back(m.tier->lower); }
    if (int rc = lock_tiers_and_tables(std::move(tiers), std::move(tabs), s, &locks)) return rc;
  }

  // insert_counted's host work for ALL members, before the first grouped launch: room for the batch in both tables (a table may
  // grow here), the upper table's phase-2 flags.  A failure leaves earlier tables grown and no row or statistic changed.
  std::vector<uint8_t*> deferred(n_act, nullptr);
  for (size_t k = 0; k < n_act; ++k) {
    tfra_tier* t = act[k].tier;
    const size_t n = act[k].d->n;
    if (int rc = t->upper->prepare_insert(n, s)) return rc;
    if (t->upper->at_max_capacity()) {
      EvictScratch es;
      if (int rc = carve_evict_scratch(t->upper, s, n, false, 0, &es)) return rc;
      deferred[k] = es.deferred;
    }
    if (int rc = t->lower->prepare_insert(n, s)) return rc;
    if (t->lower->at_max_capacity())   // (insert_counted's refusal, before anything is enqueued here)
      return set_error(TFRA_ERR_INVALID, "insert: whole rows into a table at max_capacity need the capturing phase 2");
  }

  // classes, per stage: the template instance the single call would have launched
  for (Member& m : act) {
    const tfra_tier* t = m.tier;
    const tfra_tier_find_or_insert_desc& d = *m.d;
    const int g_find = d.values_out ? granule_of(t->fb, d.values_out, d.init_values) : 16;
    m.c_find = granule_class(g_find, t->upper->dense);
    const int g_fetch = std::min(granule_of(t->fb, d.values_out, d.init_values), granule_of(t->fb, t->up_rows, nullptr));
    m.c_fetch = granule_class(g_fetch, t->lower->dense);
    m.c_put = granule_class(granule_of(t->fb, t->up_rows, t->down_rows), false);
    m.c_verify = granule_class(16, t->upper->dense);
  }

  Blob blob;
  const size_t rec_off = blob.add<TierAdmitRec>(n_act);
  // find, fetch: NGC classes; upper phase 1, phase 2, lower phase 1: NGC - 1 (no PF1 axis); verify: 2
  const size_t pre_off = blob.add<unsigned>(2 * ClassPool::words(n_act, NGC, true) + 3 * ClassPool::words(n_act, NGC - 1, true) +
                                            ClassPool::words(n_act, 2, true));
  ManyUpload up;
  if (int rc = many_begin(ws, 0, blob.bytes(), s, &up)) return rc;
  TierAdmitRec* recs = section<TierAdmitRec>(up.host, rec_off);
  for (size_t k = 0; k < n_act; ++k) {
    tfra_tier* t = act[k].tier;
    const tfra_tier_find_or_insert_desc& d = *act[k].d;
    Table *u = t->upper, *l = t->lower;
    recs[k] = TierAdmitRec{u->view_of(u->cur), l->view_of(l->cur), u->aux, t->words, d.n, (const long long*)d.d_n, (const i64*)d.keys,
                           (const unsigned char*)d.init_values, (unsigned char*)d.values_out, d.where, t->miss_keys, t->miss_idx,
                           t->up_rows, t->down_keys, t->down_rows, t->down_scores, deferred[k], u->global_epoch, l->global_epoch,
                           (u64)t->max_batch, d.init_is_full, u->opts.strategy, l->opts.strategy,
                           bounded_mode(u, deferred[k] != nullptr), t->whole};
  }
  ClassPool pool{section<unsigned>(up.host, pre_off)};
  auto n_of = [&](size_t k) { return act[k].d->n; };
  auto find_blocks = [&](size_t k) { return blocks_of(n_of(k), TIER_TILES); };
  auto put_grid = [&](size_t k) { return (unsigned)((n_of(k) + 63) / 64); };     // 4 waves of 16 keys per block
  auto evict_grid = [&](size_t k) { return (unsigned)((n_of(k) + 15) / 16); };   // one 16-lane group per key
  ManyClass c_find[NGC], c_fetch[NGC], c_up[NGC], c_evict[NGC], c_low[NGC], c_verify[2];
  for (int c = 0; c < NGC; ++c) c_find[c] = pool.put(n_act, true, [&](size_t k) { return act[k].c_find == c; }, find_blocks);
  for (int c = 0; c < NGC; ++c) c_fetch[c] = pool.put(n_act, true, [&](size_t k) { return act[k].c_fetch == c; }, find_blocks);
  for (int c = 1; c < NGC; ++c) c_up[c] = pool.put(n_act, true, [&](size_t k) { return act[k].c_put == c; }, put_grid);
  for (int c = 1; c < NGC; ++c)
    c_evict[c] = pool.put(n_act, true, [&](size_t k) { return act[k].c_put == c && deferred[k]; }, evict_grid);
  for (int c = 1; c < NGC; ++c) c_low[c] = pool.put(n_act, true, [&](size_t k) { return act[k].c_put == c; }, put_grid);
  for (int c = 0; c < 2; ++c)
    c_verify[c] = pool.put(n_act, true, [&](size_t k) { return (act[k].d->flags & TFRA_TIER_VERIFY) && act[k].c_verify == c; }, find_blocks);
  if (int rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true)) return rc;

  const TierAdmitRec* drecs = section<const TierAdmitRec>(up.dev, rec_off);
  const unsigned* dpre = section<const unsigned>(up.dev, pre_off);
  uint32_t launches = 0;
  // a class's kernel arguments: its block prefix, its index of records behind it (ClassPool)
  auto run = [&](const ManyClass& k, auto&& launch) {
    if (!k.n) return;
    launch(k.grid, dpre + k.at, dpre + k.at + k.n + 1, k.n);
    ++launches;
  };
  // 0. the previous call's counters into the statistics
  tier_begin_many_kernel<<<(unsigned)((n_act + 255) / 256), 256, 0, s>>>(drecs, (unsigned)n_act);
  ++launches;
  const dim3 wide(256 * TIER_TILES);
  // 1. the upper tables: rows and `where` of the hits, their scores touched; the misses to each tier's list
  for (int c = 0; c < NGC; ++c)
    run(c_find[c], [&](unsigned grid, const unsigned* p, const unsigned* ix, unsigned n) {
      with_granule_class(c, [&](auto G, auto PF1) { tier_find_missed_many_kernel<G, PF1, true><<<grid, wide, 0, s>>>(drecs, p, ix, n); });
    });
  // 2. the lower tables: the whole row of every listed key, or the row a never-seen key starts with
  for (int c = 0; c < NGC; ++c)
    run(c_fetch[c], [&](unsigned grid, const unsigned* p, const unsigned* ix, unsigned n) {
      with_granule_class(c, [&](auto G, auto PF1) { tier_fetch_many_kernel<G, PF1><<<grid, wide, 0, s>>>(drecs, p, ix, n); });
    });
  // 3. up they go (phase 1; at max_capacity phase 2, capturing what is displaced) ...
  for (int c = 1; c < NGC; ++c)
    run(c_up[c], [&](unsigned grid, const unsigned* p, const unsigned* ix, unsigned n) {
      with_granule_class(c, [&](auto G, auto) { tier_insert_many_kernel<G, false><<<grid, 256, 0, s>>>(drecs, p, ix, n); });
    });
  for (int c = 1; c < NGC; ++c)
    run(c_evict[c], [&](unsigned grid, const unsigned* p, const unsigned* ix, unsigned n) {
      with_granule_class(c, [&](auto G, auto) { tier_evict_many_kernel<G><<<grid, 256, 0, s>>>(drecs, p, ix, n); });
    });
  // 4. ... and what they displaced goes down
  for (int c = 1; c < NGC; ++c)
    run(c_low[c], [&](unsigned grid, const unsigned* p, const unsigned* ix, unsigned n) {
      with_granule_class(c, [&](auto G, auto) { tier_insert_many_kernel<G, true><<<grid, 256, 0, s>>>(drecs, p, ix, n); });
    });
  // 5. how many keys of each VERIFY member's batch are NOT resident now
  for (int c = 0; c < 2; ++c)
    run(c_verify[c], [&](unsigned grid, const unsigned* p, const unsigned* ix, unsigned n) {
      if (c == 0) tier_find_missed_many_kernel<16, true, false><<<grid, wide, 0, s>>>(drecs, p, ix, n);
      else tier_find_missed_many_kernel<16, false, false><<<grid, wide, 0, s>>>(drecs, p, ix, n);
    });
  HIP_TRY(hipGetLastError());
  for (const Member& m : act) { m.tier->upper->step_epoch(); m.tier->lower->step_epoch(); }
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}
