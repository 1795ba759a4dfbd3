// The locked upsert and accumulate of the table (tfra_table.hip): insert_or_assign[_n], insert_and_evict, find_or_insert,
// find_or_insert_planned (the same lookup over the distinct keys of a write-back plan, tfra_plan.h), insert_field, accum_or_assign.
// (Unique keys on a table that is large for the batch take the ownership pass instead: own_upsert_unique, tfra_own.hip.)
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "tfra_host.h"
#include "tfra_plan.h"

using namespace tfra;
typedef tfra::AuxInitPod AuxInit;  // elem_bytes = sizeof(V); pattern[f] = aux_init[f] as V, replicated to 32 bits

// ---- aux-field initialisation for a newly claimed row --------------------------------------

// WT: write-through stores (eviction path: the row must be in memory before the key is published, see publish_key)
template <bool WT = false>
__device__ __forceinline__ void init_aux_fields(const TableView& v, const AuxInit& ai, i64 row,
                                                int sub, unsigned skip_field) {
  unsigned char* r = row_ptr(v, row);
  for (unsigned f = 0; f < v.n_fields; ++f) {
    if (f == skip_field) continue;
    unsigned pat = f == 0 ? 0u : ai.pattern[(f - 1) & 3];
    unsigned char* p = r + f * v.field_bytes;
    if ((v.field_bytes & 3) == 0) {
      for (unsigned off = sub * 4; off < v.field_bytes; off += 64) {
        if (WT) __hip_atomic_store(reinterpret_cast<unsigned*>(p + off), pat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *reinterpret_cast<unsigned*>(p + off) = pat;
      }
    } else {
      for (unsigned off = sub; off < v.field_bytes; off += 16) {
        const unsigned char b = (unsigned char)(pat >> (8 * (off % ai.elem_bytes)));
        if (WT) __hip_atomic_store(p + off, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else p[off] = b;
      }
    }
  }
}

// What the FIND instance (tfra_table_find_or_insert) hands back and where its count and init rows come from.
struct FindOut {
  unsigned char* vals;   // [n, field_bytes]: the resident row of a hit, the init row of a miss; may be null
  uint8_t* found;        // may be null
  unsigned char* spill;  // single init row on a table at max_capacity: phase 2 reads row i of its source, so a deferred key's init row goes here
  const long long* d_n;  // null, or the key count on the device (n = the buffers' length)
  int full;              // init rows: one per key, or one for all (find_kernel's defaults)
};

// ---- insert_or_assign, unique-keys fast path (single pass) ---------------------------------
// FIND: a hit is READ — its row goes to fo.vals, nothing of it but the score is written; a miss is written from its
// init row `vals` as the plain instance writes it, and that row is what fo.vals gets.  Unique keys: no other group of the launch
// writes a row that a hit reads, and the rows of earlier launches are behind a kernel boundary, so the row is loaded as find loads it.
template <int G, int U, bool FIND = false>
__global__ __launch_bounds__(256) void insert_unique_kernel(TableView v, size_t n,
                                                            const i64* __restrict__ keys,
                                                            const unsigned char* __restrict__ vals,
                                                            const u64* __restrict__ scores,
                                                            unsigned field, AuxInit ai, int strategy,
                                                            u64 epoch, int bounded, uint8_t* __restrict__ deferred, FindOut fo) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  constexpr int KPW = 4 * U;
  const size_t base = wave * KPW;
  const size_t n_buf = n;
  if constexpr (FIND) {
    if (fo.d_n) {   // uniform load, as find_kernel's
      const long long dn = *fo.d_n;
      n = dn < 0 ? 0 : min(n, (size_t)dn);
    }
    // phase 2 walks the whole buffer: the flags of the keys beyond the count say "not deferred"
    if (deferred && lane < KPW && base + lane >= n && base + lane < n_buf) deferred[base + lane] = 0;
  }
  if (base >= n) return;
  const size_t last = n - 1;
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
    int j = u * 4 + grp;
    size_t i = base + j;
    if (i < n) {
      bool is_new;
      i64 row = locate_or_claim_from(v, key[u], h[u], b0[u], k0[u], sub, gshift, is_new, bounded, pf1 ? &k1[u] : nullptr);
      if (deferred && sub == 0) deferred[i] = row == NEED_EVICT;
      if constexpr (FIND) {
        const unsigned char* init = vals + (fo.full ? i * (size_t)v.field_bytes : 0);
        unsigned char* out = fo.vals ? fo.vals + i * (size_t)v.field_bytes : nullptr;
        const bool hit = row >= 0 && !is_new;
        if (fo.found && sub == 0) fo.found[i] = hit;
        if (hit) {
          if (out) copy_bytes16<G>(out, row_ptr(v, row), v.field_bytes, sub);
        } else {
          if (row >= 0) {
            copy_bytes16<G>(row_ptr(v, row), init, v.field_bytes, sub);
            if (v.n_fields > 1) init_aux_fields(v, ai, row, sub, 0);
          } else if (row == NEED_EVICT && fo.spill) {
            copy_bytes16<G>(fo.spill + i * (size_t)v.field_bytes, init, v.field_bytes, sub);
          }
          if (out) copy_bytes16<G>(out, init, v.field_bytes, sub);
        }
        if (row >= 0) {
          update_score(v, row, is_new, strategy, scores ? scores[i] : 1, epoch, sub);
          fresh += (is_new && sub == 0);
        } else if (row != NEED_EVICT) {
          failed += (sub == 0);
        }
      } else if (row >= 0) {
        copy_bytes16<G>(row_ptr(v, row) + field * v.field_bytes,
                        vals + i * (size_t)v.field_bytes, v.field_bytes, sub);
        if (is_new && v.n_fields > 1) init_aux_fields(v, ai, row, sub, field);
        update_score(v, row, is_new, strategy, scores ? scores[i] : 1, epoch, sub);
        fresh += (is_new && sub == 0);
      } else if (row != NEED_EVICT) {
        failed += (sub == 0);
      }
    }
  }
  // one size update per wave
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, wave, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

// ---- phase 2 of a bounded-table upsert: keys that found neither themselves nor an empty slot
// replace the minimum-score entry of their two home buckets (runs after phase 1 has completed, so
// no row is being written by an assign while it is evicted).

// Where the capturing instance (tfra_table_insert_and_evict) appends what leaves the table: (key, row, score) triples at *counter.
struct EvictOut {
  u64* counter;         // device size_t, advanced by every reported entry whatever cap is
  u64 cap;              // entries at positions >= cap are not written
  i64* keys;            // null: count only
  unsigned char* vals;  // may be null; rows of row_bytes
  u64* scores;          // may be null
  unsigned row_bytes;   // field_bytes, or the whole co-located row (TFRA_EVICT_WHOLE_ROWS)
};

// Row copy whose loads are agent-scope, as load_key_coherent's: the victim may have been published a moment ago by a group of
// this launch on another XCD (write-through stores), and a plain load could be served from a line that predates them.
template <int G>
__device__ __forceinline__ void copy_bytes16_coherent(unsigned char* dst, const unsigned char* src, unsigned bytes, int sub) {
  for (unsigned off = sub * G; off < bytes; off += 16 * G) {
    if constexpr (G >= 8) {
      const u64* p = reinterpret_cast<const u64*>(src + off);
      u64 t[G / 8];
#pragma unroll
      for (int j = 0; j < G / 8; ++j) t[j] = __hip_atomic_load(p + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int j = 0; j < G / 8; ++j) reinterpret_cast<u64*>(dst + off)[j] = t[j];
    } else {
      typedef typename Granule<G>::T T;
      *reinterpret_cast<T*>(dst + off) = __hip_atomic_load(reinterpret_cast<const T*>(src + off), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The slot `word` (row `row`) is LOCKED by this group: the new key's row, aux fields and score, then the key
template <int G>
__device__ __forceinline__ void replace_locked(const TableView& v, i64 row, u64 word, i64 key, const unsigned char* src, unsigned field,
                                               const AuxInit& ai, int strategy, u64 in_score, u64 epoch, int sub) {
  copy_bytes16_wt<G>(row_ptr(v, row) + field * v.field_bytes, src, v.field_bytes, sub);
  if (v.n_fields > 1) init_aux_fields<true>(v, ai, row, sub, field);
  if (sub == 0) store_wt8(score_word(v, word), 0);  // the slot starts a new life: scores count from zero
  update_score<true>(v, row, true, strategy, in_score, epoch, sub);
  publish_key(v, word, key, sub);
}

// CAPTURE: every entry that leaves the table, and every key that is not admitted, is appended to `eo`.
template <int G, bool CAPTURE = false>
__global__ __launch_bounds__(256) void insert_evict_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                           const unsigned char* __restrict__ vals,
                                                           const u64* __restrict__ scores, unsigned field, AuxInit ai,
                                                           int strategy, u64 epoch, const uint8_t* __restrict__ deferred, EvictOut eo) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t i = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  int fresh = 0, failed = 0;
  const bool lru_like = strategy == TFRA_EVICT_LRU || strategy == TFRA_EVICT_EPOCHLRU;
  if constexpr (!CAPTURE) {
    if (i < n && deferred[i]) {
      const i64 key = keys[i];
      const u64 in_score = scores ? scores[i] : 1;
      u64 word = 0;
      bool claimed_empty;
      i64 row = evict_and_lock(v, key, strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score, lru_like, sub,
                               gshift, &word, claimed_empty);
      if (row >= 0) {
        replace_locked<G>(v, row, word, key, vals + i * (size_t)v.field_bytes, field, ai, strategy, in_score, epoch, sub);
        fresh = (claimed_empty && sub == 0);
      } else if (row == -3) {
        failed = (sub == 0);
      }  // -1: not admitted (its score is below every resident score): silently dropped, like HKV
    }
  } else {
    const bool active = i < n && deferred[i];
    i64 key = 0, victim = EMPTY_KEY, row = -3;
    u64 in_score = 1, compare = 0, word = 0;
    bool claimed_empty = false;
    if (active) {
      key = keys[i];
      in_score = scores ? scores[i] : 1;
      compare = strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score;
      row = evict_and_lock(v, key, compare, lru_like, sub, gshift, &word, claimed_empty, nullptr, nullptr, &victim);
    }
    // Output positions: ONE counter add per wave.  The wave's groups have left evict_and_lock together (they wait for each other
    // at the end of its loop, capturing or not), so the ballot makes no lock holder wait for anything it did not wait for before.
    const bool report = active && ((row >= 0 && !claimed_empty) || row == -1);   // a replaced entry, or a key that is not admitted
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
      replace_locked<G>(v, row, word, key, vals + i * (size_t)v.field_bytes, field, ai, strategy, in_score, epoch, sub);
      fresh = (claimed_empty && sub == 0);
    } else if (active && row == -3) {
      failed = (sub == 0);
    } else if (wr) {   // -1, not admitted: the caller's own key, row and compare score; slot vectors at aux_init.  No table read.
      if (sub == 0) {
        eo.keys[pos] = key;
        if (eo.scores) eo.scores[pos] = compare;
      }
      if (out_row) {
        copy_bytes16<G>(out_row, vals + i * (size_t)v.field_bytes, v.field_bytes, sub);
        for (unsigned f = 1; (f + 1) * v.field_bytes <= eo.row_bytes; ++f) {
          const unsigned pat = ai.pattern[(f - 1) & 3];
          unsigned char* p = out_row + f * v.field_bytes;
          if (G >= 4 && (v.field_bytes & 3) == 0) {
            for (unsigned off = sub * 4; off < v.field_bytes; off += 64) *reinterpret_cast<unsigned*>(p + off) = pat;
          } else {
            for (unsigned off = sub; off < v.field_bytes; off += 16) p[off] = (unsigned char)(pat >> (8 * (off % ai.elem_bytes)));
          }
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, i >> 2, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
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
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, wave, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
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

// ---- typed accumulate: row[j] += delta[j], one add per element (ValueArray::operator+=) ----

template <int DT>
__device__ __forceinline__ void row_add(unsigned char* row, const unsigned char* delta, unsigned dim, int sub) {
  for (unsigned j = sub; j < dim; j += 16) {
    if (DT == TFRA_F32) reinterpret_cast<float*>(row)[j] += reinterpret_cast<const float*>(delta)[j];
    else if (DT == TFRA_F64) reinterpret_cast<double*>(row)[j] += reinterpret_cast<const double*>(delta)[j];
    else if (DT == TFRA_I8) reinterpret_cast<signed char*>(row)[j] = (signed char)(reinterpret_cast<signed char*>(row)[j] + reinterpret_cast<const signed char*>(delta)[j]);
    else if (DT == TFRA_I32) reinterpret_cast<unsigned*>(row)[j] += reinterpret_cast<const unsigned*>(delta)[j];
    else if (DT == TFRA_I64) reinterpret_cast<u64*>(row)[j] += reinterpret_cast<const u64*>(delta)[j];
    else if (DT == TFRA_F16) {
      _Float16 a = reinterpret_cast<_Float16*>(row)[j], b = reinterpret_cast<const _Float16*>(delta)[j];
      reinterpret_cast<_Float16*>(row)[j] = (_Float16)((float)a + (float)b);
    } else {
      unsigned short* r = reinterpret_cast<unsigned short*>(row);
      r[j] = f32_to_bf16(bf16_to_f32(r[j]) + bf16_to_f32(reinterpret_cast<const unsigned short*>(delta)[j]));
    }
  }
}

// ---- accum_or_assign.  ROUND >= 0: duplicate-safe mode, processes only the occurrence that is
// currently first-in-line for its key (election word), see host loop. -------------------------
// one (key, values-or-delta, exists) triple: absent & !exists -> insert, present & exists -> row += delta, else nothing
template <int DT, int G>
__device__ __forceinline__ void accum_one(const TableView& v, size_t i, const i64* __restrict__ keys,
                                          const unsigned char* __restrict__ vod, const uint8_t* __restrict__ exists,
                                          const u64* __restrict__ scores, unsigned dim, const AuxInit& ai, int strategy, u64 epoch,
                                          uint8_t* __restrict__ deferred, int bounded_mode, int sub, int gshift, int& fresh,
                                          int& failed) {
  const i64 key = keys[i];
  const bool ex = exists[i] != 0;
  const unsigned char* src = vod + i * (size_t)v.field_bytes;
  if (!ex) {
    bool is_new;
    i64 row;
    if (deferred) {  // bounded table at max_capacity: keys without a free slot evict in phase 2
      u64 h;
      const u64 b0 = bucket0(key, v.nb, h);
      const i64 k0 = load_key_coherent(key_line(v, b0) + sub);
      row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, bounded_mode);
      if (sub == 0) deferred[i] = row == NEED_EVICT;
    } else {
      row = locate_or_claim(v, key, sub, gshift, is_new);
    }
    if (row < 0) failed += (sub == 0 && row != NEED_EVICT);
    else if (is_new) {
      copy_bytes16<G>(row_ptr(v, row), src, v.field_bytes, sub);
      if (v.n_fields > 1) init_aux_fields(v, ai, row, sub, 0);
      update_score(v, row, true, strategy, scores ? scores[i] : 1, epoch, sub);
      fresh += (sub == 0);
    }  // present & !exists: dropped
  } else {
    i64 row = probe_find<true>(v, key, sub, gshift);
    if (row >= 0) {
      row_add<DT>(row_ptr(v, row), src, dim, sub);
      update_score(v, row, false, strategy, scores ? scores[i] : 1, epoch, sub);
    }  // absent & exists: dropped
    if (deferred && sub == 0) deferred[i] = 0;
  }
}

template <int DT, int G>
__global__ __launch_bounds__(256) void accum_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                    const unsigned char* __restrict__ vod,
                                                    const uint8_t* __restrict__ exists,
                                                    const u64* __restrict__ scores, unsigned dim,
                                                    AuxInit ai, int strategy, u64 epoch,
                                                    uint8_t* __restrict__ deferred, int bounded_mode) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t g = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  const size_t wave = g >> 2;
  int fresh = 0, failed = 0;
  if (g < n) accum_one<DT, G>(v, g, keys, vod, exists, scores, dim, ai, strategy, epoch, deferred, bounded_mode, sub, gshift, fresh, failed);
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, wave, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

// Keys that repeat within one call: the reference applies the triples one after the other in index order
// (LaunchTensorsAccum on one thread; accumrase_fn, cuckoohash_map.hh:619-633), and the outcome of an occurrence depends
// on the ones before it (an insert makes the key present for the next).  The (key, index) pairs arrive sorted by key
// (stable radix sort: indices ascend within a key); the group of a key's FIRST sorted position walks the key's
// occurrences in index order, every step through memory (a key that repeats thousands of times is one long chain —
// exact, not fast: TFRA de-duplicates before accum, PY/dynamic_embedding_variable.py:1377-1378).
template <int DT, int G>
__global__ __launch_bounds__(256) void accum_segments_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                             const unsigned char* __restrict__ vod,
                                                             const uint8_t* __restrict__ exists, const u64* __restrict__ scores,
                                                             unsigned dim, AuxInit ai, int strategy, u64 epoch,
                                                             const u64* __restrict__ sorted_keys, const unsigned* __restrict__ sorted_idx) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t p = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  int fresh = 0, failed = 0;
  if (p < n) {
    const u64 k = sorted_keys[p];
    if (p == 0 || sorted_keys[p - 1] != k) {
      for (size_t q = p; q < n && sorted_keys[q] == k; ++q) {
        accum_one<DT, G>(v, (size_t)sorted_idx[q], keys, vod, exists, scores, dim, ai, strategy, epoch, nullptr, 0, sub, gshift, fresh, failed);
        __threadfence_block();   // the next occurrence reads what this one wrote (other lanes of the group, same row)
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, p >> 2, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

__global__ void iota_u32_kernel(unsigned* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (unsigned)i;
}

// eo (tfra_table_insert_and_evict): where phase 2 of a table at max_capacity reports what it replaces or does not admit; such a call
// takes the locked kernels (the ownership pass does not capture).  Off max_capacity eo is not looked at.
static int insert_impl(Table* t, hipStream_t s, int field, size_t n, const int64_t* keys, const void* values,
                       const uint64_t* scores, uint32_t flags, const EvictOut* eo = nullptr) {
  if (n == 0) return TFRA_OK;
  if (!keys || !values) return set_error(TFRA_ERR_INVALID, "insert: null buffer");
  if (field < 0 || field > t->opts.aux_fields) return set_error(TFRA_ERR_INVALID, "insert: bad field");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "insert: more than 2^31-1 keys per call");
  int rc = t->prepare_insert(n, s);
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
    uint8_t* deferred = nullptr;
    if (bounded) {
      rc = t->ensure_scratch(n, s);
      if (rc) return rc;
      t->apply_P = 0;
      deferred = (uint8_t*)t->scratch;
    }
    TableView v = t->view_of(t->cur);
    const int bd = bounded_mode(t, bounded);
    with_granule(g, [&](auto G) { insert_unique_kernel<G, U><<<grid, block, 0, s>>>(v, n, k, vals, sc, field, t->aux, strat, epoch, bd, deferred, FindOut{}); });
    if (bounded) {
      dim3 grid2((unsigned)((n * 16 + 255) / 256));
      if (eo) {   // one granule for the table row, the caller's rows and the output rows
        const int gc = std::min(g, granule_of(eo->row_bytes, eo->vals, nullptr));
        with_granule(gc, [&](auto G) { insert_evict_kernel<G, true><<<grid2, block, 0, s>>>(v, n, k, vals, sc, field, t->aux, strat, epoch, deferred, *eo); });
      } else {
        with_granule(g, [&](auto G) { insert_evict_kernel<G><<<grid2, block, 0, s>>>(v, n, k, vals, sc, field, t->aux, strat, epoch, deferred, EvictOut{}); });
      }
    }
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

static void launch_accum(int dt, int g, dim3 grid, hipStream_t s, TableView v, size_t n, const i64* k, const unsigned char* vod,
                         const uint8_t* ex, const u64* sc, unsigned dim, AuxInit ai, int strat, u64 epoch,
                         const u64* sorted_keys, const unsigned* sorted_idx, uint8_t* deferred, int bmode) {
  with_dtype(dt, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    with_granule(g, [&](auto G) {
      if (sorted_keys) accum_segments_kernel<DT, G><<<grid, 256, 0, s>>>(v, n, k, vod, ex, sc, dim, ai, strat, epoch, sorted_keys, sorted_idx);
      else accum_kernel<DT, G><<<grid, 256, 0, s>>>(v, n, k, vod, ex, sc, dim, ai, strat, epoch, deferred, bmode);
    });
  });
}

// Unique keys, their number on the device: the ownership pass or nothing (the locked kernels size their scratch by the host's n).
extern "C" int tfra_table_insert_or_assign_n(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const void* values,
                                             const uint64_t* scores, tfra_stream_t stream) {
  TABLE_ENTER();
  if (n == 0) return TFRA_OK;
  if (!d_n || !keys || !values) return set_error(TFRA_ERR_INVALID, "insert_or_assign_n: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "insert: more than 2^31-1 keys per call");
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys: a growing table may grow a call early)
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
  if (!keys || !values || !d_evicted_counter) return set_error(TFRA_ERR_INVALID, "tfra_table_insert_and_evict: null buffer");
  if (!evicted_keys && (evicted_values || evicted_scores))
    return set_error(TFRA_ERR_INVALID, "tfra_table_insert_and_evict: evicted_keys == NULL counts only, evicted_values and evicted_scores must be NULL too");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "tfra_table_insert_and_evict: more than 2^31-1 keys per call");
  TABLE_ENTER();
  const unsigned row_bytes = t->field_bytes * ((flags & TFRA_EVICT_WHOLE_ROWS) ? 1u + (unsigned)t->opts.aux_fields : 1u);
  const EvictOut eo{(u64*)d_evicted_counter, (u64)cap, (i64*)evicted_keys, (unsigned char*)evicted_values, (u64*)evicted_scores, row_bytes};
  return insert_impl(t, s, 0, n, keys, values, scores, TFRA_FLAG_UNIQUE_KEYS, &eo);
}

// find_or_insert: always the locked two-phase route, as insert_and_evict; the ownership pass does not serve it.
extern "C" int tfra_table_find_or_insert(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const void* init_values,
                                         int init_is_full, const uint64_t* scores, void* values_out, uint8_t* found,
                                         tfra_stream_t stream) {
  if (!tp) return set_error(TFRA_ERR_INVALID, "tfra_table_find_or_insert: null table");
  if (n == 0) return TFRA_OK;
  if (!keys || !init_values) return set_error(TFRA_ERR_INVALID, "tfra_table_find_or_insert: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "tfra_table_find_or_insert: more than 2^31-1 keys per call");
  TABLE_ENTER();
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys when d_n is given)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const unsigned fb = t->field_bytes;
  const int g = granule_of(fb, init_values, values_out);
  const i64* k = (const i64*)keys;
  const unsigned char* init = (const unsigned char*)init_values;
  const u64* sc = (const u64*)scores;
  const int strat = t->opts.strategy;
  constexpr int U = 4;
  const size_t waves = (n + 4 * U - 1) / (4 * U);
  dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const bool bounded = t->at_max_capacity();
  uint8_t* deferred = nullptr;
  FindOut fo{(unsigned char*)values_out, found, nullptr, (const long long*)d_n, init_is_full != 0};
  const unsigned char* src2 = init;   // phase 2 reads row i of its source
  if (bounded) {
    const size_t flags_bytes = (n + 255) & ~(size_t)255;
    const bool spill = !init_is_full && !values_out;
    rc = t->ensure_scratch(flags_bytes + (spill ? n * (size_t)fb : 0), s);
    if (rc) return rc;
    t->apply_P = 0;
    deferred = (uint8_t*)t->scratch;
    if (spill) fo.spill = (unsigned char*)t->scratch + flags_bytes;
    if (!init_is_full) src2 = spill ? fo.spill : fo.vals;   // a deferred key's init row is in values_out[i] after phase 1
  }
  TableView v = t->view_of(t->cur);
  const int bd = bounded_mode(t, bounded);
  with_granule(g, [&](auto G) { insert_unique_kernel<G, U, true><<<grid, block, 0, s>>>(v, n, k, init, sc, 0, t->aux, strat, epoch, bd, deferred, fo); });
  if (bounded) {
    dim3 grid2((unsigned)((n * 16 + 255) / 256));
    with_granule(g, [&](auto G) { insert_evict_kernel<G><<<grid2, block, 0, s>>>(v, n, k, src2, sc, 0, t->aux, strat, epoch, deferred, EvictOut{}); });
  }
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}

// ---- find_or_insert over a write-back plan: the keys are the CSR plan's distinct keys, every batch position of a
// key gets its row.  Key k's init row and score are those of its LAST batch position L(k), so the outcome does not depend on
// the order the plan holds its keys in.

// What the planned instance reads per batch position and where its rows go.
struct PlanFindIO {
  const unsigned char* init;  // [n, field_bytes] when full, else one row
  const u64* scores;          // null, or [n] per batch position
  unsigned char* rows;        // [n, field_bytes]
  uint8_t* found;             // [n]; may be null
  int full;
  unsigned n;                 // the plan's id count: rows of `rows`, upper bound of its keys
  // a table at max_capacity: phase 2 (insert_evict_kernel) reads entry g of dense per-KEY arrays
  uint8_t* deferred;          // [n] flags; null off max_capacity
  unsigned char* spill;       // [n, field_bytes]: a deferred key's init row
  u64* key_scores;            // [n]: its score; null when scores is
};

// A row of at most 1024 bytes in the registers of a 16-lane group: lane `sub` holds granule sub, sub + 16, ... (G = 16 or 8).
// (Native vector types: an array of HIP's uint4 that is filled under a condition is not split into registers, it goes to LDS.)
template <int G>
struct GroupRow {
  typedef unsigned T __attribute__((ext_vector_type(G / 4)));
  T r0, r1, r2, r3;
  __device__ __forceinline__ void load(const unsigned char* src, unsigned bytes, int sub) {
    const unsigned off = (unsigned)sub * G;
    r0 = r1 = r2 = r3 = T(0u);
    if (off < bytes) r0 = *reinterpret_cast<const T*>(src + off);
    if (off + 16 * G < bytes) r1 = *reinterpret_cast<const T*>(src + off + 16 * G);
    if (off + 32 * G < bytes) r2 = *reinterpret_cast<const T*>(src + off + 32 * G);
    if (off + 48 * G < bytes) r3 = *reinterpret_cast<const T*>(src + off + 48 * G);
  }
  __device__ __forceinline__ void store(unsigned char* dst, unsigned bytes, int sub) const {
    const unsigned off = (unsigned)sub * G;
    if (off < bytes) *reinterpret_cast<T*>(dst + off) = r0;
    if (off + 16 * G < bytes) *reinterpret_cast<T*>(dst + off + 16 * G) = r1;
    if (off + 32 * G < bytes) *reinterpret_cast<T*>(dst + off + 32 * G) = r2;
    if (off + 48 * G < bytes) *reinterpret_cast<T*>(dst + off + 48 * G) = r3;
  }
};

// Key launch: one 16-lane group per plan key (grid-stride, bounded by the count on the device).  Probe, score and the per-wave
// size / error accounting are insert_unique_kernel<G, U, true>'s; the row then goes to every position of a key with at most
// DIRECT occurrences, and to position L(k) of a key whose positions sit in the bins (find_plan_bins_kernel copies it on from there).
template <int G>
__global__ __launch_bounds__(256) void find_plan_keys_kernel(TableView v, CsrKeys ks, PlanFindIO io, AuxInit ai, int strategy, u64 epoch,
                                                             int bounded, int* __restrict__ prow_dest) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = min(ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD], io.n);
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
  const unsigned ngroups = nthreads >> 4;
  if (blockIdx.x == 0 && threadIdx.x == 0 && ks.d_counts[PC_OVERFLOW]) atomicAdd(v.err_count, ks.d_counts[PC_OVERFLOW]);  // plan overflow
  // phase 2 walks all n entries: the flags of the entries beyond the count say "not deferred"
  if (io.deferred)
    for (unsigned i = total + tid; i < io.n; i += nthreads) io.deferred[i] = 0;
  const unsigned fb = v.field_bytes;
  const bool pf1 = bounded > 1;  // table near capacity: both home buckets' lines in flight together
  int fresh = 0, failed = 0;
  for (unsigned g = tid >> 4; g < total; g += ngroups) {
    bool many;
    const unsigned w = load_record(ks, g, sub, many);
    const i64 key = (i64)(((u64)(unsigned)__shfl((int)w, gshift + 1) << 32) | (unsigned)__shfl((int)w, gshift));
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    const i64 k0 = load_key_coherent(key_line(v, b0) + sub);
    const i64 k1 = load_key_coherent(key_line(v, pf1 ? bucket1(h, b0, v.nb) : b0) + sub);  // (same line again: an L2 hit)
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    unsigned lastp = (unsigned)__shfl((int)w, gshift + (many ? 5 : 3));   // few: the last position itself; many: where it is stored
    if (many) lastp = ks.hent[lastp];
    lastp &= E_POS;
    if (lastp >= io.n) continue;   // (no record of a completed build says so)
    const unsigned char* init = io.init + (io.full ? (size_t)lastp * fb : 0);
    const u64 in_score = io.scores ? io.scores[lastp] : 1;
    bool is_new;
    const i64 row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, bounded, pf1 ? &k1 : nullptr);
    const bool hit = row >= 0 && !is_new;
    GroupRow<G> r;
    r.load(hit ? row_ptr(v, row) : init, fb, sub);
    if (io.deferred && sub == 0) io.deferred[g] = row == NEED_EVICT;
    if (!hit) {
      if (row >= 0) {
        r.store(row_ptr(v, row), fb, sub);
        if (v.n_fields > 1) init_aux_fields(v, ai, row, sub, 0);
      } else if (row == NEED_EVICT && io.spill) {
        r.store(io.spill + (size_t)g * fb, fb, sub);
        if (io.key_scores && sub == 0) io.key_scores[g] = in_score;
      }
    }
    if (row >= 0) {
      update_score(v, row, is_new, strategy, in_score, epoch, sub);
      fresh += (is_new && sub == 0);
    } else if (row != NEED_EVICT) {
      failed += (sub == 0);
    }
    if (many) {
      r.store(io.rows + (size_t)lastp * fb, fb, sub);
      if (io.found && sub == 0) io.found[lastp] = hit;
      const unsigned first = (unsigned)__shfl((int)w, gshift + 3), nsrc = (unsigned)__shfl((int)w, gshift + 4);
      for (unsigned t = sub; t < nsrc; t += 16) prow_dest[first + t] = (int)lastp;
    } else {
      for (unsigned e = 0; e < min(cnt, (unsigned)DIRECT); ++e) {
        const unsigned p = (unsigned)__shfl((int)w, gshift + 4 + (int)e);
        if (p >= io.n) continue;
        r.store(io.rows + (size_t)p * fb, fb, sub);
        if (io.found && sub == 0) io.found[p] = hit;
      }
    }
  }
  // one size update per wave
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, tid >> 6, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

// Bins launch, behind the key launch's kernel boundary: one block per bin of SEG entries, a 16-lane group per 16-entry item (the
// layout plan_dest_bins_kernel walks).  The item's run belongs to one key, whose row and flag the key launch left at L(k): every
// other position of the item copies them from there.  (rows[L(k)] itself is written by nobody in this launch.)
template <int G>
__global__ __launch_bounds__(NTA) void find_plan_bins_kernel(const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                                             const unsigned* __restrict__ binmap, const unsigned* __restrict__ d_counts,
                                                             const int* __restrict__ prow_dest, unsigned char* rows, uint8_t* found,
                                                             unsigned fb, unsigned n) {
  constexpr int NG = NTA / 16;
  __shared__ unsigned char s_kind[NG];   // 0 = continues the run of the item before, 1 = first item of a run, 2 = empty item
  __shared__ unsigned s_row[NG];
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, g = threadIdx.x >> 4;
  const unsigned nbins = d_counts[PC_BINS];
  for (unsigned ib = blockIdx.x; ib < nbins; ib += gridDim.x) {
    const unsigned bin = binmap[ib];
    const unsigned e = hent[(size_t)bin * SEG + threadIdx.x];
    const unsigned e0 = (unsigned)__shfl((int)e, gshift);
    const bool empty = (e0 & E_SKIP) != 0, first = (e0 & E_HEAD) != 0;
    if (sub == 0) {
      s_kind[g] = empty ? 2 : (first ? 1 : 0);
      s_row[g] = (first && !empty) ? hout[(size_t)bin * 32 + g] : 0u;
    }
    __syncthreads();
    if (!empty) {   // (uniform in the group)
      int g2 = g;
      while (g2 > 0 && s_kind[g2] == 0) --g2;
      const unsigned L = (unsigned)prow_dest[s_row[g2]];
      if (L < n) {
        GroupRow<G> r;
        r.load(rows + (size_t)L * fb, fb, sub);
        const uint8_t f = found ? found[L] : 0;
        for (int j = 0; j < 16; ++j) {
          const unsigned ej = (unsigned)__shfl((int)e, gshift + j);
          const unsigned p = ej & E_POS;
          if ((ej & E_SKIP) || p == L || p >= n) continue;
          r.store(rows + (size_t)p * fb, fb, sub);
          if (found && sub == 0) found[p] = f;
        }
      }
    }
    __syncthreads();
  }
}

extern "C" int tfra_table_find_or_insert_planned(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const void* init_values,
                                                 int init_is_full, const uint64_t* scores, void* rows_out, uint8_t* found,
                                                 tfra_stream_t stream) {
  const char* who = "tfra_table_find_or_insert_planned: ";
  if (!tp) return set_error(TFRA_ERR_INVALID, std::string(who) + "null table");
  if (!pl) return set_error(TFRA_ERR_INVALID, std::string(who) + "null plan");
  if (!init_values || !rows_out) return set_error(TFRA_ERR_INVALID, std::string(who) + "null buffer");
  if (pl->n == 0) return set_error(TFRA_ERR_INVALID, std::string(who) + "no built plan");
  if (pl->kind == 1)
    return set_error(TFRA_ERR_UNSUPPORTED, std::string(who) + "needs a plan built with the table's dim (an assign-only plan keeps no positions)");
  {
    const Table* tc = reinterpret_cast<const Table*>(tp);
    const int dt = tc->opts.value_dtype, dim = tc->opts.dim;
    if (pl->dim != dim) return set_error(TFRA_ERR_INVALID, std::string(who) + "the plan was built for another dim");
    if (tc->opts.device != pl->device && tc->opts.device >= 0)
      return set_error(TFRA_ERR_INVALID, std::string(who) + "plan and table live on different devices");
    if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
      return set_error(TFRA_ERR_UNSUPPORTED, std::string(who) + "value_dtype must be float32, float16 or bfloat16");
    if (dim % 4 != 0 || dim > 256 || (((uintptr_t)init_values | (uintptr_t)rows_out) & 15))
      return set_error(TFRA_ERR_UNSUPPORTED, std::string(who) + "needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers");
  }
  TABLE_ENTER();
  const size_t n = pl->n;
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const unsigned fb = t->field_bytes;
  const int g = granule_of(fb, init_values, rows_out) >= 16 ? 16 : 8;   // (dim % 4 == 0: rows of at least 8 bytes, at most 1024)
  const int strat = t->opts.strategy;
  const bool bounded = t->at_max_capacity();
  PlanFindIO io{(const unsigned char*)init_values, (const u64*)scores, (unsigned char*)rows_out, found, init_is_full != 0, (unsigned)n,
                nullptr, nullptr, nullptr};
  if (bounded) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t score_bytes = scores ? al(n * 8) : 0;
    rc = t->ensure_scratch(al(n) + score_bytes + n * (size_t)fb, s);
    if (rc) return rc;
    t->apply_P = 0;
    io.deferred = (uint8_t*)t->scratch;
    if (scores) io.key_scores = (u64*)((unsigned char*)t->scratch + al(n));
    io.spill = (unsigned char*)t->scratch + al(n) + score_bytes;
  }
  TableView v = t->view_of(t->cur);
  const int bd = bounded_mode(t, bounded);
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  const CsrKeys ks = keys_of(pl);
  auto launch = [&](auto G) {
    find_plan_keys_kernel<G><<<key_blocks, 256, 0, s>>>(v, ks, io, t->aux, strat, epoch, bd, pl->prow_dest);
    // (always launched: the host does not know the bin count; without bins it does nothing)
    find_plan_bins_kernel<G><<<bin_blocks, NTA, 0, s>>>(pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->prow_dest, io.rows, found, fb,
                                                        (unsigned)n);
  };
  if (g == 16) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 8>{});
  if (bounded) {   // phase 2 over the plan's dense keys: flags, rows and scores by key index
    dim3 grid2((unsigned)((n * 16 + 255) / 256)), block(256);
    with_granule(g, [&](auto G) { insert_evict_kernel<G><<<grid2, block, 0, s>>>(v, n, pl->dkeys, io.spill, io.key_scores, 0, t->aux, strat, epoch, io.deferred, EvictOut{}); });
  }
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}

extern "C" int tfra_table_insert_field(tfra_table_t* tp, int field, size_t n, const int64_t* keys, const void* values,
                                       uint32_t flags, tfra_stream_t stream) {
  TABLE_ENTER();
  return insert_impl(t, s, field, n, keys, values, nullptr, flags);
}

extern "C" int tfra_table_accum_or_assign(tfra_table_t* tp, size_t n, const int64_t* keys, const void* vod,
                                          const uint8_t* exists, const uint64_t* scores, uint32_t flags, tfra_stream_t stream) {
  TABLE_ENTER();
  if (n == 0) return TFRA_OK;
  if (!keys || !vod || !exists) return set_error(TFRA_ERR_INVALID, "accum: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "accum: more than 2^31-1 keys per call");
  int rc = t->prepare_insert(n, s);
  if (rc) return rc;
  int g = granule_of(t->field_bytes, vod, nullptr);
  TableView v = t->view_of(t->cur);
  const i64* k = (const i64*)keys;
  if (flags & TFRA_FLAG_UNIQUE_KEYS) {
    // unique keys (what TFRA hands the op: PY/dynamic_embedding_variable.py:1377-1378): the single pass with bucket ownership,
    // as tfra_table_insert_or_assign does, whenever the batch is small for the table; else the locked kernels
    bool taken = false;
    rc = own_upsert_unique(t, s, n, k, vod, (const u64*)scores, &taken, exists);
    if (rc) return rc;
    if (taken) return TFRA_OK;   // (TableWrapper::accum does not step the epoch: lookup_table_op_hkv.h:539-546)
    dim3 grid((unsigned)((n * 16 + 255) / 256));
    uint8_t* deferred;
    rc = t->bounded_flags(n, s, &deferred);
    if (rc) return rc;
    launch_accum(t->opts.value_dtype, g, grid, s, v, n, k, (const unsigned char*)vod, exists, (const u64*)scores,
                 (unsigned)t->opts.dim, t->aux, t->opts.strategy, t->global_epoch, nullptr, nullptr, deferred,
                 bounded_mode(t, deferred != nullptr));
    if (deferred) {  // phase 2: the absent keys that found no free slot replace a minimum-score entry
      const unsigned char* vals = (const unsigned char*)vod;
      const u64* sc = (const u64*)scores;
      const int strat = t->opts.strategy;
      const u64 epoch = t->global_epoch;
      dim3 block(256);
      with_granule(g, [&](auto G) { insert_evict_kernel<G><<<grid, block, 0, s>>>(v, n, k, vals, sc, 0, t->aux, strat, epoch, deferred, EvictOut{}); });
    }
    HIP_TRY(hipGetLastError());
    return TFRA_OK;
  }
  {
    uint8_t* bounded_now;
    rc = t->bounded_flags(1, s, &bounded_now);
    if (rc) return rc;
    if (bounded_now)
      return set_error(TFRA_ERR_UNSUPPORTED, "accum: a bounded (Hkv) table at max_capacity needs TFRA_FLAG_UNIQUE_KEYS "
                                             "(HKV's unique-keys contract) so that eviction is well defined");
  }
  // Duplicate-safe mode: the reference applies the triples sequentially in index order (LaunchTensorsAccum on one
  // thread).  All on the device, no host copy and no synchronisation: a stable radix sort of (key, index) groups the
  // occurrences of a key with their indices ascending, and accum_segments_kernel walks each group in that order.
  {
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs((void*)nullptr, tmp_bytes, (const u64*)nullptr, (u64*)nullptr, (const unsigned*)nullptr,
                                      (unsigned*)nullptr, n, 0u, 64u, s));
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    rc = t->ensure_scratch(al(n * 8) + 2 * al(n * 4) + al(tmp_bytes), s);
    if (rc) return rc;
    t->apply_P = 0;  // scratch head is overwritten below
    unsigned char* w = (unsigned char*)t->scratch;
    u64* sorted_keys = (u64*)w; w += al(n * 8);
    unsigned* iota = (unsigned*)w; w += al(n * 4);
    unsigned* sorted_idx = (unsigned*)w; w += al(n * 4);
    void* tmp = w;
    iota_u32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(iota, n);
    HIP_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const u64*)keys, sorted_keys, (const unsigned*)iota, sorted_idx, n, 0u, 64u, s));
    dim3 grid((unsigned)((n * 16 + 255) / 256));
    launch_accum(t->opts.value_dtype, g, grid, s, v, n, k, (const unsigned char*)vod, exists, (const u64*)scores,
                 (unsigned)t->opts.dim, t->aux, t->opts.strategy, t->global_epoch, sorted_keys, sorted_idx, nullptr, 0);
  }
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
