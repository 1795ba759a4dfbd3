// The grouped admitting lookup of plain tables: tfra_multi_find_or_insert, the tfra_table_find_or_insert
// (tfra_find_insert.hip) of a LIST of tables as ONE stream-ordered chain: one record upload, then phase 1 once per
// copy-granule class of the list and, for the members at max_capacity, phase 2 once per granule class among them — 1 launch for a
// list of aligned float32 growing tables however long it is, 2 with full bounded members, at most 10.
// Both kernels have the launch shape of the grouped calls (tfra_many.h): many_desc_of takes the block to its descriptor, the record
// is read with wave-uniform loads, and the body runs on a block index local to the descriptor.  A block touches only its own
// descriptor's table, buffers and scratch — the call refuses a table that stands twice — so the locked protocol waits on slots of
// its own table only, as in the single call.
// The bodies are TWINS of insert_unique_kernel<G, 4, true> (tfra_upsert_device.h) and of insert_evict_kernel<G, false>
// (insert_evict_body<G, false, false>, tfra_upsert.hip): those kernels take their operands as kernel arguments and their key index
// from blockIdx; handing them a shared body that takes both from a record changed the generated code of the same kernels before
// (profiles/tier_admit_many_isa_stats.txt), so the body stands twice.  A fix in one belongs in the other.
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_find_insert.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;

namespace {

// One active descriptor: what the single call's two launches take as kernel arguments.
struct FindInsertRec {
  TableView v;                  // taken under the lock, behind the table's prepare_insert
  AuxInit aux;                  // the slot vectors a never-seen key starts with
  size_t n;                     // the buffers' length
  const long long* d_n;         // may be null
  const i64* keys;
  const unsigned char* init;    // [n, field_bytes] when full, else one row
  const u64* scores;            // may be null
  unsigned char* out;           // may be null
  uint8_t* found;               // may be null
  uint8_t* deferred;            // phase-2 flags; null off max_capacity
  unsigned char* spill;         // one shared init row and no `out` on a table at max_capacity: a deferred key's init row
  const unsigned char* src2;    // row i of this is what phase 2 writes for key i: init (full), else spill, else out
  u64 epoch;
  int full, strategy, bounded;  // bounded: bounded_mode of the table
};

// ---- phase 1: the twin of insert_unique_kernel<G, U, true> ---------------------------------------------------------------------------
// wave: the wave's index among the waves of THIS key list (the shard of the size counter too, as in the single call).
template <int G, int U>
__device__ __forceinline__ void find_insert_body(const FindInsertRec& r, const size_t wave) {
  const TableView& v = r.v;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  constexpr int KPW = 4 * U;
  const size_t base = wave * KPW;
  const size_t n_buf = r.n;
  size_t n = n_buf;
  if (r.d_n) {   // uniform load, as find_kernel's
    const long long dn = *r.d_n;
    n = dn < 0 ? 0 : min(n, (size_t)dn);
  }
  uint8_t* __restrict__ deferred = r.deferred;
  // phase 2 walks the whole buffer: the flags of the keys beyond the count say "not deferred"
  if (deferred && lane < KPW && base + lane >= n && base + lane < n_buf) deferred[base + lane] = 0;
  if (base >= n) return;
  const size_t last = n - 1;
  const i64* __restrict__ keys = r.keys;
  const unsigned char* __restrict__ vals = r.init;
  const u64* __restrict__ scores = r.scores;
  const int bounded = r.bounded, strategy = r.strategy;
  const u64 epoch = r.epoch;
  i64 kreg = keys[min(base + (size_t)(lane & (KPW - 1)), last)];
  int fresh = 0, failed = 0;
  i64 key[U], k0[U], k1[U];
  u64 h[U], b0[U];
  const bool pf1 = bounded > 1;  // table near capacity: both home buckets' lines in flight together
#pragma unroll
  for (int u = 0; u < U; ++u) {  // U first probes in flight (unconditional, tail clamped)
    key[u] = shfl_i64(kreg, u * 4 + grp);
    b0[u] = bucket0(key[u], v.nb, h[u]);
    k0[u] = load_key_coherent(key_line(v, b0[u]) + sub);
    k1[u] = load_key_coherent(key_line(v, pf1 ? bucket1(h[u], b0[u], v.nb) : b0[u]) + sub);  // (same line again: an L2 hit)
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
    const unsigned char* init = vals + (r.full ? i * (size_t)v.field_bytes : 0);
    unsigned char* out = r.out ? r.out + i * (size_t)v.field_bytes : nullptr;
    const bool hit = row >= 0 && !is_new;
    if (r.found && sub == 0) r.found[i] = hit;
    if (hit) {
      if (out) copy_bytes16<G>(out, row_ptr(v, row), v.field_bytes, sub);
    } else {
      if (row >= 0) {
        copy_bytes16<G>(row_ptr(v, row), init, v.field_bytes, sub);
        if (v.n_fields > 1) init_aux_fields(v, r.aux, row, sub, 0);
      } else if (row == NEED_EVICT && r.spill) {
        copy_bytes16<G>(r.spill + i * (size_t)v.field_bytes, init, v.field_bytes, sub);
      }
      if (out) copy_bytes16<G>(out, init, v.field_bytes, sub);
    }
    if (row >= 0) {
      update_score(v, row, is_new, strategy, scores ? scores[i] : 1, epoch, sub);
      fresh += (is_new && sub == 0);
    } else if (row != NEED_EVICT) {
      failed += (sub == 0);
    }
  }
  wave_account(v, wave, lane, fresh, failed);
}
template <int G>
__global__ __launch_bounds__(256) void find_insert_many_kernel(const FindInsertRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                               const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const FindInsertRec& rec = recs[idx[d]];   // (a reference: init_aux_fields indexes aux.pattern with a variable, which a copy in registers cannot serve)
  find_insert_body<G, 4>(rec, ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 6);
}

// ---- phase 2: the twin of insert_evict_kernel<G, false> (insert_evict_body<G, false, false>, field 0) -----------------------------------
// The keys whose flag is set replace the minimum-score entry of their home buckets by row i of r.src2 and their score; a key that
// is not admitted is dropped.  i: the key of this 16-lane group.
template <int G>
__device__ __forceinline__ void find_insert_evict_body(const FindInsertRec& r, const size_t i) {
  const TableView& v = r.v;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  int fresh = 0, failed = 0;
  const int strategy = r.strategy;
  const u64 epoch = r.epoch;
  const bool lru_like = strategy == TFRA_EVICT_LRU || strategy == TFRA_EVICT_EPOCHLRU;
  const bool active = i < r.n && r.deferred[i];
  i64 key = 0, row = -3;
  u64 in_score = 1, compare = 0, word = 0;
  bool claimed_empty = false;
  if (active) {
    key = r.keys[i];
    in_score = r.scores ? r.scores[i] : 1;
    compare = strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score;
    row = evict_and_lock(v, key, compare, lru_like, sub, gshift, &word, claimed_empty, nullptr, nullptr, nullptr);
  }
  if (active) {
    if (row >= 0) {
      replace_locked<G, false>(v, row, word, key, r.src2 + i * (size_t)v.field_bytes, 0u, r.aux, strategy, in_score, epoch, sub);
      fresh = (claimed_empty && sub == 0);
    } else if (row == -3) {
      failed = (sub == 0);
    }   // (-1, not admitted: silently dropped, like HKV — its score is below every resident score)
  }
  wave_account(v, i >> 2, lane, fresh, failed);
}
template <int G>
__global__ __launch_bounds__(256) void find_insert_evict_many_kernel(const FindInsertRec* __restrict__ recs,
                                                                     const unsigned* __restrict__ prefix,
                                                                     const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const FindInsertRec& rec = recs[idx[d]];
  find_insert_evict_body<G>(rec, ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The class of a descriptor: the granule ladder of with_granule.  0: <16>, 1: <8>, 2: <4>, 3: <2>, 4: <1>.
constexpr int NGC = 5;
int granule_class(int g) { return g == 16 ? 0 : g == 8 ? 1 : g == 4 ? 2 : g == 2 ? 3 : 4; }

struct Member {
  Table* t;
  const tfra_find_or_insert_desc* d;
  int cls = 0;
  EvictScratch es;
  bool bounded = false;
};

}  // namespace

extern "C" int tfra_multi_find_or_insert(tfra_workspace_t* ws, size_t n_tables, const tfra_find_or_insert_desc* descs,
                                         uint32_t* launches_out, tfra_stream_t stream) {
  const std::string who = "multi_find_or_insert";
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and no table and no output changes
  std::vector<Member> act;
  std::map<const void*, size_t> seen;   // where a table of the call stands
  u64 evict_blocks = 0;
  for (size_t i = 0; i < n_tables; ++i) {
    const tfra_find_or_insert_desc& d = descs[i];
    const std::string at_i = who + ": descriptor " + std::to_string(i) + ": ";
    if (d.struct_size != sizeof(tfra_find_or_insert_desc)) return set_error(TFRA_ERR_INVALID, at_i + "descriptor size mismatch");
    if (d.flags) return set_error(TFRA_ERR_INVALID, at_i + "unknown flag bits");
    if (d.reserved) return set_error(TFRA_ERR_INVALID, at_i + "reserved must be 0");
    const Check c = check_find_or_insert(d.table, d.n, d.keys, d.init_values);
    if (c.code) return report(at_i, c);
    if (!c.active) continue;
    Table* t = reinterpret_cast<Table*>(d.table);
    if (t->device != ws->device) return set_error(TFRA_ERR_INVALID, at_i + "workspace and table live on different devices");
    // this call WRITES: a table stands once in it (a block touches its own descriptor's table only)
    if (!seen.emplace(t, i).second)
      return set_error(TFRA_ERR_INVALID, at_i + "the same table as descriptor " + std::to_string(seen[t]) +
                                             " (a call that writes takes every table once)");
    Member m;
    m.t = t;
    m.d = &d;
    act.push_back(m);
    evict_blocks += (d.n + 15) / 16;   // phase 2's grid, the larger
  }
  const size_t n_act = act.size();
  if (n_act == 0) return TFRA_OK;
  if (evict_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, who + ": too many keys in one call");

  std::vector<std::unique_lock<std::mutex>> locks;
  {
    std::vector<Table*> tabs;
    for (const Member& m : act) tabs.push_back(m.t);
    if (int rc = lock_and_enter(std::move(tabs), s, &locks)) return rc;
  }

  // the single call's host work for ALL members, before the first grouped launch: room for the batch (a table may grow here or
  // enqueue a size read), the phase-2 scratch of a table at max_capacity.  A failure leaves earlier tables grown and no row changed.
  for (Member& m : act) {
    const tfra_find_or_insert_desc& d = *m.d;
    if (int rc = m.t->prepare_insert(d.n, s)) return rc;   // (n is an upper bound of the keys when d_n is given)
    m.bounded = m.t->at_max_capacity();
    if (m.bounded)
      if (int rc = carve_evict_scratch(m.t, s, d.n, false, !d.init_is_full && !d.values_out ? m.t->field_bytes : 0, &m.es)) return rc;
    m.cls = granule_class(granule_of(m.t->field_bytes, d.init_values, d.values_out));
  }

  Blob blob;
  const size_t rec_off = blob.add<FindInsertRec>(n_act);
  const size_t pre_off = blob.add<unsigned>(2 * ClassPool::words(n_act, NGC, true));
  ManyUpload up;
  if (int rc = many_begin(ws, 0, blob.bytes(), s, &up)) return rc;
  FindInsertRec* recs = section<FindInsertRec>(up.host, rec_off);
  for (size_t k = 0; k < n_act; ++k) {
    const Member& m = act[k];
    const tfra_find_or_insert_desc& d = *m.d;
    const unsigned char* init = (const unsigned char*)d.init_values;
    unsigned char* out = (unsigned char*)d.values_out;
    // phase 2 reads row i of its source: a deferred key's init row is in the spill rows, else in values_out[i], after phase 1
    const unsigned char* src2 = d.init_is_full ? init : m.es.spill ? m.es.spill : out;
    recs[k] = FindInsertRec{m.t->view_of(m.t->cur), m.t->aux, d.n, (const long long*)d.d_n, (const i64*)d.keys, init,
                            (const u64*)d.scores, out, d.found, m.es.deferred, m.es.spill, src2, m.t->global_epoch,
                            d.init_is_full != 0, m.t->opts.strategy, bounded_mode(m.t, m.bounded)};
  }
  ClassPool pool{section<unsigned>(up.host, pre_off)};
  ManyClass c_find[NGC], c_evict[NGC];
  for (int c = 0; c < NGC; ++c)   // 4 waves of 16 keys per block
    c_find[c] = pool.put(n_act, true, [&](size_t k) { return act[k].cls == c; }, [&](size_t k) { return (unsigned)((act[k].d->n + 63) / 64); });
  for (int c = 0; c < NGC; ++c)   // one 16-lane group per key
    c_evict[c] = pool.put(n_act, true, [&](size_t k) { return act[k].cls == c && act[k].bounded; },
                          [&](size_t k) { return (unsigned)((act[k].d->n + 15) / 16); });
  if (int rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true)) return rc;

  const FindInsertRec* drecs = section<const FindInsertRec>(up.dev, rec_off);
  const unsigned* dpre = section<const unsigned>(up.dev, pre_off);
  uint32_t launches = 0;
  // 1. every member finds or claims, copies and scores; at max_capacity the keys without a slot are flagged
  for (int c = 0; c < NGC; ++c) {
    const ManyClass& k = c_find[c];
    if (!k.n) continue;
    with_granule(16 >> c, [&](auto G) { find_insert_many_kernel<G><<<k.grid, 256, 0, s>>>(drecs, dpre + k.at, dpre + k.at + k.n + 1, k.n); });
    ++launches;
  }
  // 2. the flagged keys of the members at max_capacity evict
  for (int c = 0; c < NGC; ++c) {
    const ManyClass& k = c_evict[c];
    if (!k.n) continue;
    with_granule(16 >> c, [&](auto G) { find_insert_evict_many_kernel<G><<<k.grid, 256, 0, s>>>(drecs, dpre + k.at, dpre + k.at + k.n + 1, k.n); });
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  for (const Member& m : act) m.t->step_epoch();
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}
