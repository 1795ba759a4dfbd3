// The locked upsert of the table (tfra_table.hip): insert_or_assign[_n], insert_and_evict[_n], insert_field, and the eviction phase of
// every two-phase call of the family (evict_phase: insert_evict_kernel is compiled here and nowhere else).  The admitting lookups
// are tfra_find_insert.hip, the typed accumulate tfra_accum.hip; what the three share: tfra_upsert_device.h, tfra_upsert.h.
// (Unique keys on a table that is large for the batch take the ownership pass instead: own_upsert_unique, tfra_own.hip.)
// Kernels instantiated here: insert_unique_kernel<G, U, false>, insert_counted_kernel<G, U, false | true>,
// insert_evict_kernel<G, false | true>, insert_evict_rows_kernel<G>, insert_locate_kernel, insert_write_kernel, rearm_winner_kernel.
#include <hip/hip_runtime.h>

#include "tfra_host.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;

// ---- phase 2 of a bounded-table upsert (what it is and what it reports: tfra_upsert_device.h, at EvictOut) ----

// CAPTURE: every entry that leaves the table, and every key that is not admitted, is appended to `eo`.
// WHOLE_IN (TFRA_INSERT_WHOLE_ROWS, capturing only): `vals` rows are whole co-located rows, written and reported as such.
// (The <G, true, true> instance has a TWIN in tfra_tierstep_many.hip, insert_evict_whole_body, which takes its key index as an
// argument; handing this body the index changed these kernels' registers — DESIGN §4.25.  A fix here belongs there too.
// The <G, false, false> instance has one in tfra_find_insert_many.hip, find_insert_evict_body — DESIGN §4.27.  A fix in one belongs
// in the other.  The <G, false, false> instance has a second one in tfra_rows.hip, store_rows_evict_kernel, whose row comes from
// float32 fields — DESIGN §4.34.)
template <int G, bool CAPTURE, bool WHOLE_IN>
__device__ __forceinline__ void insert_evict_body(const TableView& v, size_t n, const i64* __restrict__ keys,
                                                  const unsigned char* __restrict__ vals,
                                                  const u64* __restrict__ scores, unsigned field, const AuxInit& ai,
                                                  int strategy, u64 epoch, const uint8_t* __restrict__ deferred, const EvictOut& eo) {
  const unsigned src_bytes = WHOLE_IN ? v.n_fields * v.field_bytes : v.field_bytes;   // one row of vals
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t i = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  int fresh = 0, failed = 0;
  const bool lru_like = strategy == TFRA_EVICT_LRU || strategy == TFRA_EVICT_EPOCHLRU;
  const bool active = i < n && deferred[i];
  i64 key = 0, victim = EMPTY_KEY, row = -3;
  u64 in_score = 1, compare = 0, word = 0;
  bool claimed_empty = false;
  if (active) {
    key = keys[i];
    in_score = scores ? scores[i] : 1;
    compare = strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score;
    row = evict_and_lock(v, key, compare, lru_like, sub, gshift, &word, claimed_empty, nullptr, nullptr, CAPTURE ? &victim : nullptr);
  }
  bool wr = false;              // this group reports an entry: a replaced one, or its own key that is not admitted
  u64 pos = 0;                  // where
  unsigned char* out_row = nullptr;
  if constexpr (CAPTURE) {
    // Output positions: ONE counter add per wave.  The wave's groups have left evict_and_lock together (they wait for each other
    // at the end of its loop, capturing or not), so the ballot makes no lock holder wait for anything it did not wait for before.
    const bool report = active && ((row >= 0 && !claimed_empty) || row == -1);
    const u64 m = __ballot(report && sub == 0);
    if (m) {
      unsigned lo = 0, hi = 0;
      if (lane == 0) {
        const u64 b = atomicAdd(eo.counter, (u64)__popcll(m));
        lo = (unsigned)b; hi = (unsigned)(b >> 32);
      }
      pos = (((u64)(unsigned)__shfl((int)hi, 0) << 32) | (unsigned)__shfl((int)lo, 0)) + (u64)__popcll(m & ((1ULL << gshift) - 1));
    }
    wr = report && eo.keys && pos < eo.cap;
    out_row = eo.vals ? eo.vals + pos * (u64)eo.row_bytes : nullptr;
  }
  // An idle group has nothing to do below.  (CAPTURE ||: said this way, each instance keeps the control flow its own copy of this
  // body had, and compiles to the same code.)
  if (CAPTURE || active) {
    if (row >= 0) {
      if constexpr (CAPTURE) {
        if (wr) {
          // the slot is LOCKED: its row and score are stable (evict_and_lock re-read the score under the lock).  Read before write.
          if (sub == 0) {
            eo.keys[pos] = victim;
            if (eo.scores) eo.scores[pos] = __hip_atomic_load(score_word(v, word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          if (out_row) copy_bytes16_coherent<G>(out_row, row_ptr(v, row), eo.row_bytes, sub);
        }
      }
      replace_locked<G, WHOLE_IN>(v, row, word, key, vals + i * (size_t)src_bytes, field, ai, strategy, in_score, epoch, sub);
      fresh = (claimed_empty && sub == 0);
    } else if (active && row == -3) {
      failed = (sub == 0);
    } else if (CAPTURE && wr) {   // -1, not admitted: the caller's own key, row and compare score; slot vectors at aux_init.  No table read.
      if (sub == 0) {             // (not capturing: silently dropped, like HKV — its score is below every resident score)
        eo.keys[pos] = key;
        if (eo.scores) eo.scores[pos] = compare;
      }
      if (out_row) {
        if constexpr (WHOLE_IN) {   // the caller's row, slot vectors and all (eo.row_bytes: the field or the whole row)
          copy_bytes16<G>(out_row, vals + i * (size_t)src_bytes, eo.row_bytes, sub);
        } else {
          copy_bytes16<G>(out_row, vals + i * (size_t)v.field_bytes, v.field_bytes, sub);
          // (out_row is aligned to G only: words when G says so)
          for (unsigned f = 1; (f + 1) * v.field_bytes <= eo.row_bytes; ++f)
            fill_aux_field(out_row + f * v.field_bytes, v.field_bytes, ai.pattern[(f - 1) & 3], ai.elem_bytes, G >= 4 && (v.field_bytes & 3) == 0, sub);
        }
      }
    }
  }
  wave_account(v, i >> 2, lane, fresh, failed);
}

// The kernels of the body: insert_evict_kernel under the name and with the code it had, and the whole-row capturing instance.
template <int G, bool CAPTURE = false>
__global__ __launch_bounds__(256) void insert_evict_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                           const unsigned char* __restrict__ vals,
                                                           const u64* __restrict__ scores, unsigned field, AuxInit ai,
                                                           int strategy, u64 epoch, const uint8_t* __restrict__ deferred, EvictOut eo) {
  insert_evict_body<G, CAPTURE, false>(v, n, keys, vals, scores, field, ai, strategy, epoch, deferred, eo);
}
template <int G>
__global__ __launch_bounds__(256) void insert_evict_rows_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                                const unsigned char* __restrict__ vals, const u64* __restrict__ scores,
                                                                AuxInit ai, int strategy, u64 epoch, const uint8_t* __restrict__ deferred,
                                                                EvictOut eo) {
  insert_evict_body<G, true, true>(v, n, keys, vals, scores, 0u, ai, strategy, epoch, deferred, eo);
}

// ---- insert_and_evict_n, phase 1 ----
// insert_unique_kernel's plain write of the embedding field — its probes, claim, score and accounting — over the min(n_buf, *d_n)
// leading keys of buffers of n_buf entries (d_n null: all), the flags of the entries beyond the count cleared for phase 2 as the
// FIND instance clears them.  A kernel of its own so that insert_unique_kernel keeps its code.
// WHOLE (TFRA_INSERT_WHOLE_ROWS): `vals` rows are whole co-located rows; the slot vectors of a new AND of a resident key are the
// caller's, init_aux_fields is not applied.
// (The WHOLE instance has a TWIN in tfra_tierstep_many.hip, insert_whole_counted_body, on a wave index local to a descriptor of
// the grouped admission — DESIGN §4.25.  A fix here belongs there too.  A second one is store_rows_kernel, tfra_rows.hip, whose
// rows come from float32 fields — DESIGN §4.34.)
template <int G, int U, bool WHOLE>
__global__ __launch_bounds__(256) void insert_counted_kernel(TableView v, size_t n_buf, const i64* __restrict__ keys,
                                                             const unsigned char* __restrict__ vals, const u64* __restrict__ scores,
                                                             AuxInit ai, int strategy, u64 epoch, int bounded,
                                                             uint8_t* __restrict__ deferred, const long long* __restrict__ d_n) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  constexpr int KPW = 4 * U;
  const size_t base = wave * KPW;
  size_t n = n_buf;
  if (d_n) {   // uniform load, as find_kernel's
    const long long dn = *d_n;
    n = dn < 0 ? 0 : min(n_buf, (size_t)dn);
  }
  if (deferred && lane < KPW && base + lane >= n && base + lane < n_buf) deferred[base + lane] = 0;
  if (base >= n) return;
  const size_t last = n - 1;
  const unsigned src_bytes = WHOLE ? v.n_fields * v.field_bytes : v.field_bytes;   // one row of vals
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
      if constexpr (!WHOLE) { if (is_new && v.n_fields > 1) init_aux_fields(v, ai, row, sub, 0); }
      update_score(v, row, is_new, strategy, scores ? scores[i] : 1, epoch, sub);
      fresh += (is_new && sub == 0);
    } else if (row != NEED_EVICT) {
      failed += (sub == 0);
    }
  }
  wave_account(v, wave, lane, fresh, failed);
}

// ---- insert_or_assign with duplicates: pass 1 locate/claim + elect the LAST index ----------
template <int U>
__global__ __launch_bounds__(256) void insert_locate_kernel(TableView v, size_t n,
                                                            const i64* __restrict__ keys,
                                                            i64* __restrict__ slot_of, unsigned field,
                                                            AuxInit ai) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  constexpr int KPW = 4 * U;
  const size_t base = wave * KPW;
  if (base >= n) return;
  i64 kreg = (lane < KPW && base + lane < n) ? keys[base + lane] : 0;
  int fresh = 0, failed = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int j = u * 4 + grp;
    size_t i = base + j;
    i64 key = shfl_i64(kreg, j);
    if (i < n) {
      bool is_new;
      i64 row = locate_or_claim(v, key, sub, gshift, is_new);
      if (row >= 0) {
        if (is_new && v.n_fields > 1) init_aux_fields(v, ai, row, sub, field);
        if (sub == 0) {
          // hot keys (Zipf) repeat thousands of times: only occurrences that can still raise the
          // maximum pay for the contended atomic
          if (__hip_atomic_load(&v.winner[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (int)i) atomicMax(&v.winner[row], (int)i);
          slot_of[i] = row | (is_new ? (i64)1 << 62 : 0);
        }
        fresh += (is_new && sub == 0);
      } else {
        if (sub == 0) slot_of[i] = -1;
        failed += (sub == 0);
      }
    }
  }
  wave_account(v, wave, lane, fresh, failed);
}

// pass 2: only the elected occurrence writes the row (sequential "last writer wins" of
// LaunchTensorsInsert with one thread), then re-arms the election word.
template <int G>
__global__ __launch_bounds__(256) void insert_write_kernel(TableView v, size_t n,
                                                           const unsigned char* __restrict__ vals,
                                                           const u64* __restrict__ scores,
                                                           const i64* __restrict__ slot_of,
                                                           unsigned field, int strategy, u64 epoch) {
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const size_t i = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  if (i >= n) return;
  (void)lane;
  i64 so = slot_of[i];
  if (so < 0) return;
  bool is_new = (so >> 62) & 1;
  i64 row = so & (((i64)1 << 62) - 1);
  if (v.winner[row] != (int)i) {
    // LFU counts every upsert, also the overwritten duplicates
    if (strategy == TFRA_EVICT_LFU) update_score(v, row, false, strategy, scores ? scores[i] : 1, epoch, sub);
    return;
  }
  copy_bytes16<G>(row_ptr(v, row) + field * v.field_bytes,
                  vals + i * (size_t)v.field_bytes, v.field_bytes, sub);
  update_score(v, row, is_new, strategy, scores ? scores[i] : 1, epoch, sub);
}

__global__ void rearm_winner_kernel(TableView v, size_t n, const i64* __restrict__ slot_of) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  i64 so = slot_of[i];
  if (so >= 0) v.winner[so & (((i64)1 << 62) - 1)] = -1;
}

void evict_phase(Table* t, hipStream_t s, const TableView& v, int g, size_t n, const i64* keys, const unsigned char* src_rows,
                 const u64* scores, unsigned field, const uint8_t* deferred, const EvictOut* eo, bool whole_in) {
  const dim3 grid((unsigned)((n * 16 + 255) / 256)), block(256);
  const int strat = t->opts.strategy;
  const u64 epoch = t->global_epoch;
  if (eo) {   // one granule for the table row, the caller's rows and the output rows
    const int gc = std::min(g, granule_of(eo->row_bytes, eo->vals, nullptr));
    if (whole_in) with_granule(gc, [&](auto G) { insert_evict_rows_kernel<G><<<grid, block, 0, s>>>(v, n, keys, src_rows, scores, t->aux, strat, epoch, deferred, *eo); });
    else with_granule(gc, [&](auto G) { insert_evict_kernel<G, true><<<grid, block, 0, s>>>(v, n, keys, src_rows, scores, field, t->aux, strat, epoch, deferred, *eo); });
  } else {
    with_granule(g, [&](auto G) { insert_evict_kernel<G><<<grid, block, 0, s>>>(v, n, keys, src_rows, scores, field, t->aux, strat, epoch, deferred, EvictOut{}); });
  }
}

// eo (tfra_table_insert_and_evict): where phase 2 of a table at max_capacity reports what it replaces or does not admit; such a call
// takes the locked kernels (the ownership pass does not capture).  Off max_capacity eo is not looked at.
static int insert_impl(Table* t, hipStream_t s, int field, size_t n, const int64_t* keys, const void* values,
                       const uint64_t* scores, uint32_t flags, const EvictOut* eo = nullptr) {
  if (n == 0) return TFRA_OK;
  int rc = check_batch("insert: ", n, keys && values, [&] {
    return field < 0 || field > t->opts.aux_fields ? set_error(TFRA_ERR_INVALID, "insert: bad field") : TFRA_OK;
  });
  if (rc) return rc;
  rc = t->prepare_insert(n, s);
  if (rc) return rc;
  // TableWrapper::upsert epoch stepping (lookup_table_op_hkv.h:528-536)
  u64 epoch = t->global_epoch;
  unsigned fo = field * t->field_bytes;
  int g = granule_of(t->field_bytes, values, nullptr);
  if (fo) g = std::min(g, granule_of(fo, nullptr, nullptr));
  const i64* k = (const i64*)keys;
  const unsigned char* vals = (const unsigned char*)values;
  const u64* sc = (const u64*)scores;
  int strat = t->opts.strategy;
  constexpr int U = 4;
  size_t waves = (n + 4 * U - 1) / (4 * U);
  dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  // Hkv flavour at max_capacity: the table cannot grow, full home buckets evict by score (2 phases)
  const bool bounded = t->at_max_capacity() && field == 0;
  if (bounded && !(flags & TFRA_FLAG_UNIQUE_KEYS))
    return set_error(TFRA_ERR_UNSUPPORTED, "insert: a bounded (Hkv) table at max_capacity needs TFRA_FLAG_UNIQUE_KEYS "
                                           "(HKV's unique-keys contract) so that eviction is well defined");
  if ((flags & TFRA_FLAG_UNIQUE_KEYS) && field == 0 && !(bounded && eo)) {
    // the single pass with bucket ownership whenever the batch is small for the table: no locks, no CAS
    bool taken = false;
    rc = own_upsert_unique(t, s, n, k, vals, sc, &taken);
    if (rc) return rc;
    if (taken) { t->step_epoch(); return TFRA_OK; }
  }
  if (flags & TFRA_FLAG_UNIQUE_KEYS) {
    EvictScratch es;
    if (bounded) {
      rc = carve_evict_scratch(t, s, n, false, 0, &es);
      if (rc) return rc;
    }
    TableView v = t->view_of(t->cur);
    const int bd = bounded_mode(t, bounded);
    with_granule(g, [&](auto G) { insert_unique_kernel<G, U><<<grid, block, 0, s>>>(v, n, k, vals, sc, field, t->aux, strat, epoch, bd, es.deferred, FindOut{}); });
    if (bounded) evict_phase(t, s, v, g, n, k, vals, sc, field, es.deferred, eo);
  } else {
    rc = t->ensure_winner(s);
    if (rc) return rc;
    rc = t->ensure_scratch(n * sizeof(i64), s);
    if (rc) return rc;
    t->apply_P = 0;  // scratch head is overwritten below
    TableView v = t->view_of(t->cur);
    i64* slot_of = (i64*)t->scratch;
    insert_locate_kernel<U><<<grid, block, 0, s>>>(v, n, k, slot_of, field, t->aux);
    dim3 grid2((unsigned)((n * 16 + 255) / 256));
    with_granule(g, [&](auto G) { insert_write_kernel<G><<<grid2, block, 0, s>>>(v, n, vals, sc, slot_of, field, strat, epoch); });
    rearm_winner_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(v, n, slot_of);
  }
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}

// Unique keys, their number on the device: the ownership pass or nothing (the locked kernels size their scratch by the host's n).
extern "C" int tfra_table_insert_or_assign_n(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const void* values,
                                             const uint64_t* scores, tfra_stream_t stream) {
  TABLE_ENTER();
  if (n == 0) return TFRA_OK;
  int rc = check_batch("insert_or_assign_n: ", n, d_n && keys && values, NoMoreChecks{}, "insert: ");
  if (rc) return rc;
  rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys: a growing table may grow a call early)
  if (rc) return rc;
  bool taken = false;
  rc = own_upsert_unique(t, s, n, (const i64*)keys, values, (const u64*)scores, &taken, nullptr, d_n);
  if (rc) return rc;
  if (!taken) return set_error(TFRA_ERR_UNSUPPORTED, "insert_or_assign_n: the single-pass write-back cannot take this call (owner tags off, "
                                                     "a bulk load, or no scratch while capturing): read the count and call tfra_table_insert_or_assign");
  t->step_epoch();
  return TFRA_OK;
}

extern "C" int tfra_table_insert_or_assign(tfra_table_t* tp, size_t n, const int64_t* keys, const void* values,
                                           const uint64_t* scores, uint32_t flags, tfra_stream_t stream) {
  TABLE_ENTER();
  return insert_impl(t, s, 0, n, keys, values, scores, flags);
}

extern "C" int tfra_table_insert_and_evict(tfra_table_t* tp, size_t n, const int64_t* keys, const void* values, const uint64_t* scores,
                                           uint32_t flags, size_t* d_evicted_counter, size_t cap, int64_t* evicted_keys,
                                           void* evicted_values, uint64_t* evicted_scores, tfra_stream_t stream) {
  if (!tp) return set_error(TFRA_ERR_INVALID, "tfra_table_insert_and_evict: null table");
  if (flags & ~TFRA_EVICT_WHOLE_ROWS) return set_error(TFRA_ERR_INVALID, "tfra_table_insert_and_evict: unknown flag bits");
  if (n == 0) return TFRA_OK;
  if (int rc = check_batch("tfra_table_insert_and_evict: ", n, keys && values && d_evicted_counter, [&] {
        return !evicted_keys && (evicted_values || evicted_scores)
                   ? set_error(TFRA_ERR_INVALID, "tfra_table_insert_and_evict: evicted_keys == NULL counts only, evicted_values and evicted_scores must be NULL too")
                   : TFRA_OK;
      }))
    return rc;
  TABLE_ENTER();
  const unsigned row_bytes = t->field_bytes * ((flags & TFRA_EVICT_WHOLE_ROWS) ? 1u + (unsigned)t->opts.aux_fields : 1u);
  const EvictOut eo{(u64*)d_evicted_counter, (u64)cap, (i64*)evicted_keys, (unsigned char*)evicted_values, (u64*)evicted_scores, row_bytes};
  return insert_impl(t, s, 0, n, keys, values, scores, TFRA_FLAG_UNIQUE_KEYS, &eo);
}

// ---- insert_and_evict_n: the count on the device, whole rows in ----
int insert_counted(Table* t, hipStream_t s, size_t n, const long long* d_n, const i64* keys, const unsigned char* values,
                   const u64* scores, bool whole_in, const EvictOut* eo) {
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys: a growing table may grow a call early)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const int strat = t->opts.strategy;
  const int g = granule_of(t->field_bytes, values, nullptr);   // (divides the whole row too: one granule for field and row)
  constexpr int U = 4;
  const size_t waves = (n + 4 * U - 1) / (4 * U);
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const bool bounded = t->at_max_capacity();
  if (bounded && whole_in && !eo) return set_error(TFRA_ERR_INVALID, "insert: whole rows into a table at max_capacity need the capturing phase 2");
  EvictScratch es;
  if (bounded) {
    rc = carve_evict_scratch(t, s, n, false, 0, &es);
    if (rc) return rc;
  }
  const TableView v = t->view_of(t->cur);
  const int bd = bounded_mode(t, bounded);
  with_granule(g, [&](auto G) {
    if (whole_in) insert_counted_kernel<G, U, true><<<grid, block, 0, s>>>(v, n, keys, values, scores, t->aux, strat, epoch, bd, es.deferred, d_n);
    else insert_counted_kernel<G, U, false><<<grid, block, 0, s>>>(v, n, keys, values, scores, t->aux, strat, epoch, bd, es.deferred, d_n);
  });
  if (bounded) evict_phase(t, s, v, g, n, keys, values, scores, 0, es.deferred, eo, whole_in);
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}

extern "C" int tfra_table_insert_and_evict_n(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const void* values,
                                             const uint64_t* scores, uint32_t flags, size_t* d_evicted_counter, size_t cap,
                                             int64_t* evicted_keys, void* evicted_values, uint64_t* evicted_scores, tfra_stream_t stream) {
  const char* who = "tfra_table_insert_and_evict_n: ";
  if (!tp) return set_error(TFRA_ERR_INVALID, std::string(who) + "null table");
  if (flags & ~(TFRA_EVICT_WHOLE_ROWS | TFRA_INSERT_WHOLE_ROWS)) return set_error(TFRA_ERR_INVALID, std::string(who) + "unknown flag bits");
  if (n == 0) return TFRA_OK;
  if (int rc = check_batch(who, n, keys && values && d_evicted_counter, [&] {
        return !evicted_keys && (evicted_values || evicted_scores)
                   ? set_error(TFRA_ERR_INVALID, std::string(who) + "evicted_keys == NULL counts only, evicted_values and evicted_scores must be NULL too")
                   : TFRA_OK;
      }))
    return rc;
  TABLE_ENTER();
  const unsigned row_bytes = t->field_bytes * ((flags & TFRA_EVICT_WHOLE_ROWS) ? 1u + (unsigned)t->opts.aux_fields : 1u);
  const EvictOut eo{(u64*)d_evicted_counter, (u64)cap, (i64*)evicted_keys, (unsigned char*)evicted_values, (u64*)evicted_scores, row_bytes};
  return insert_counted(t, s, n, (const long long*)d_n, (const i64*)keys, (const unsigned char*)values, (const u64*)scores,
                        (flags & TFRA_INSERT_WHOLE_ROWS) != 0, &eo);
}

extern "C" int tfra_table_insert_field(tfra_table_t* tp, int field, size_t n, const int64_t* keys, const void* values,
                                       uint32_t flags, tfra_stream_t stream) {
  TABLE_ENTER();
  return insert_impl(t, s, field, n, keys, values, nullptr, flags);
}
