// Device side of the locked upsert family, for every unit that compiles it: tfra_upsert.hip (insert_or_assign, insert_and_evict,
// insert_field), tfra_find_insert.hip (find_or_insert and its planned form) and tfra_accum.hip (accum_or_assign).  What more than one
// of them instantiates or calls is here ONCE: the aux-field initialisation of a claimed row, the per-wave size / error accounting,
// the unique-keys kernel (whose FIND instances are the admitting lookup's phase 1), and what the eviction phase takes, reports
// and writes under its lock.
//
// Global namespace, not an anonymous one: the phase-2 launcher (evict_phase, tfra_upsert.h) is defined in one unit and called from
// three, so the types it takes need external linkage; and the kernels keep the mangled names recorded profiles know them by.
// A kernel template of this header is instantiated in exactly ONE unit (see each unit's head).
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_host.h"

using namespace tfra;
typedef tfra::AuxInitPod AuxInit;  // elem_bytes = sizeof(V); pattern[f] = aux_init[f] as V, replicated to 32 bits

// ---- the per-wave tail of a kernel that claims slots: one size update and one error count per wave ----
// fresh / failed: this lane's counts (lane `sub == 0` of a group counts for its key); wave: the shard of the size counter
__device__ __forceinline__ void wave_account(const TableView& v, size_t wave, int lane, int fresh, int failed) {
  for (int o = 32; o > 0; o >>= 1) { fresh += __shfl_xor(fresh, o); failed += __shfl_xor(failed, o); }
  if (lane == 0) {
    if (fresh) size_add(v, wave, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

// ---- aux-field initialisation for a newly claimed row --------------------------------------

// One field of `bytes` bytes at p, by a 16-lane group: the 32-bit pattern `pat` of elements of elem_bytes (AuxInit).  words: 32-bit
// stores — the caller says so when bytes and p are multiples of 4 —, else byte stores.
// WT: write-through stores (eviction path: the row must be in memory before the key is published, see publish_key)
template <bool WT = false>
__device__ __forceinline__ void fill_aux_field(unsigned char* p, unsigned bytes, unsigned pat, unsigned elem_bytes, bool words, int sub) {
  if (words) {
    for (unsigned off = sub * 4; off < bytes; off += 64) {
      if (WT) __hip_atomic_store(reinterpret_cast<unsigned*>(p + off), pat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *reinterpret_cast<unsigned*>(p + off) = pat;
    }
  } else {
    for (unsigned off = sub; off < bytes; off += 16) {
      const unsigned char b = (unsigned char)(pat >> (8 * (off % elem_bytes)));
      if (WT) __hip_atomic_store(p + off, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else p[off] = b;
    }
  }
}

template <bool WT = false>
__device__ __forceinline__ void init_aux_fields(const TableView& v, const AuxInit& ai, i64 row,
                                                int sub, unsigned skip_field) {
  unsigned char* r = row_ptr(v, row);
  for (unsigned f = 0; f < v.n_fields; ++f) {
    if (f == skip_field) continue;
    unsigned pat = f == 0 ? 0u : ai.pattern[(f - 1) & 3];
    fill_aux_field<WT>(r + f * v.field_bytes, v.field_bytes, pat, ai.elem_bytes, (v.field_bytes & 3) == 0, sub);   // (rows are 16-B aligned)
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
// A TWIN of the plain instance lives in tfra_upsert.hip: insert_counted_kernel (the key count on the device, whole rows in; DESIGN
// §4.20) repeats its probes, claim, score and accounting so that this kernel keeps its code.  A fix here belongs there too.
// The FIND instance has a TWIN as well: find_insert_body (tfra_find_insert_many.hip), the same lookup with its
// operands read from a descriptor's record and the wave index local to the descriptor.  A fix in one belongs in the other.
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
  wave_account(v, wave, lane, fresh, failed);
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
// WHOLE: src is a whole co-located row (TFRA_INSERT_WHOLE_ROWS): the slot vectors come from it, aux_init is not applied
template <int G, bool WHOLE = false>
__device__ __forceinline__ void replace_locked(const TableView& v, i64 row, u64 word, i64 key, const unsigned char* src, unsigned field,
                                               const AuxInit& ai, int strategy, u64 in_score, u64 epoch, int sub) {
  if constexpr (WHOLE) {
    copy_bytes16_wt<G>(row_ptr(v, row), src, v.n_fields * v.field_bytes, sub);
  } else {
    copy_bytes16_wt<G>(row_ptr(v, row) + field * v.field_bytes, src, v.field_bytes, sub);
    if (v.n_fields > 1) init_aux_fields<true>(v, ai, row, sub, field);
  }
  if (sub == 0) store_wt8(score_word(v, word), 0);  // the slot starts a new life: scores count from zero
  update_score<true>(v, row, true, strategy, in_score, epoch, sub);
  publish_key(v, word, key, sub);
}
