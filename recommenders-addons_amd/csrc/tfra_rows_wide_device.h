// Device side of whole rows out and back for WIDE rows (tfra_rows_wide.hip): tfra_table_fetch_planned_wide and
// tfra_table_store_rows_wide for 256 < dim <= 1024.  The twins (tfra_rows.hip) give a key to a 16-lane group, a lane owning four
// columns of every 64: a row of five fields of 4 KB is 80 trips of 256-byte accesses per group.  Here the launch shape is
// apply_csr_wide_body's (tfra_apply_wide_device.h): 256 threads, grid-stride, four consecutive keys per wave and trip, and
//   stage A, per 16-lane group, one key each: what is per key — the probe or the claim, the plan's record;
//   stage B, the whole wave, key after key: everything per key comes by shuffle from its group into scalar registers (wave_word);
//            per chunk of 256 columns (WIDE_COLS) lane l owns columns c0 + 4 l — an access is 1 KB contiguous on float rows, 512 B
//            on half rows — and the loads of all fields are issued together, ahead of the first store;
//   stage C, per group again (the store only): score and accounting, under the eviction phase the publication of the key.
// No LDS in the row kernels: nothing is shared between keys.  The work is probes, byte moves and one rounding.
// The sums are sum_rows_wide / hot_sums_wide_body (tfra_apply_wide_device.h): the plan's summation tree per column, so columns
// [a, b) of gsum_out are bit for bit what tfra_table_fetch_planned writes for the gradient columns [a, b).
// Anonymous namespace: see tfra_plan_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_apply_wide_device.h"
#include "tfra_device.h"
#include "tfra_optim_device.h"
#include "tfra_plan_device.h"
#include "tfra_upsert_device.h"

namespace {

constexpr int MAXF = 5;   // fields of a row: the embedding and up to four slot vectors
struct RowsOut { float* field[MAXF]; };
struct RowsIn { const float* field[MAXF]; };

// Four stored elements of a row as ONE granule per lane: 16 bytes of a float row, 8 of a half one (the wave's 64 lanes = 256 columns)
template <int ST> struct Gran4 { typedef uint2 T; };
template <> struct Gran4<TFRA_F32> { typedef float4 T; };
template <int ST> __device__ __forceinline__ float4 up4(const typename Gran4<ST>::T& r) {
  if constexpr (ST == TFRA_F32) return r;
  else return load_stored4<ST>(r);
}
// aux_init[f - 1] as the table stores it (AuxInit::pattern), up-cast
template <int ST> __device__ __forceinline__ float4 aux4(unsigned pat) {
  float a;
  if constexpr (ST == TFRA_F32) a = __uint_as_float(pat);
  else a = bits_to_float<ST>(pat & 0xffffu);
  return make_float4(a, a, a, a);
}
// fn(std::integral_constant<int, F>{}) for the fields F = FIRST .. MAXF - 1: the field index is a constant in every use, so the
// records of field pointers and the aux patterns stay kernel arguments in scalar registers
template <int FIRST, class Fn> __device__ __forceinline__ void for_fields(Fn&& fn) {
  if constexpr (FIRST < MAXF) { fn(std::integral_constant<int, FIRST>{}); for_fields<FIRST + 1>(fn); }
}
template <class GT> __device__ __forceinline__ void keep5(GT (&r)[MAXF]) {
  keep_live(r[0], r[1], r[2], r[3]);
  GT d = r[4];
  keep_live(d, r[4], r[0], r[1]);
}
// a group's pointer for the wave: its two words through scalar registers
__device__ __forceinline__ unsigned char* wave_ptr(const void* p, int src) {
  const uintptr_t x = (uintptr_t)p;
  return reinterpret_cast<unsigned char*>(((uintptr_t)wave_word((unsigned)(x >> 32), src) << 32) | wave_word((unsigned)x, src));
}
// one granule of four elements at p; WT: write-through (the eviction phase: in memory before publish_key)
template <int ST, bool WT> __device__ __forceinline__ void store_gran(unsigned char* p, const float4& x) {
  if constexpr (ST == TFRA_F32) {
    if (WT) store_wt16(p, *reinterpret_cast<const uint4*>(&x));
    else *reinterpret_cast<float4*>(p) = x;
  } else {
    const u64 b = to_stored4<ST>(x);
    if (WT) store_wt8(p, b);
    else *reinterpret_cast<u64*>(p) = b;
  }
}

// ---------------------------------------------------------------------------------------------
// fetch: the plan's distinct keys in gather_csr_kernel's order (row g of every output belongs to dkeys[g]).
//   stage A: the first probe line and the plan record (load_record) in flight together; find's probe (probe_find_word, plain loads):
//            nothing is claimed, no score is touched;
//   stage B: per chunk every lane issues MAXF granule loads together, unconditionally — field f of a resident row where the caller
//            wants it, else the first wanted field again (a line the wave holds already); a key that is not resident reads the
//            default row instead, which is its field 0, and takes the stored image of aux_init for the others — and with them the
//            chunk's gradient rows (sum_rows_wide), then the up-casts and the float4 stores.  A lane beyond dim in the last chunk
//            loads column 0 and stores nothing.  first_want < 0: no field is wanted, the rows are not read at all.
template <int ST, bool SUMS>
__device__ __forceinline__ void fetch_rows_wide_body(const TableView& v, int dim, const float* __restrict__ grads,
                                                     const float* __restrict__ partial, const CsrKeys& ks,
                                                     const unsigned char* __restrict__ default_row, const AuxInit& ai,
                                                     i64* __restrict__ keys_out, const RowsOut& ro, int first_want,
                                                     float* __restrict__ gsum_out, i64* __restrict__ d_count) {
  typedef typename Gran4<ST>::T GT;
  constexpr unsigned ES = ST == TFRA_F32 ? 4u : 2u;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  const unsigned ngroups = (gridDim.x * blockDim.x) >> 4;
  if (blockIdx.x == 0 && threadIdx.x == 0) *d_count = ks.d_counts[PC_OVERFLOW] ? (i64)-1 : (i64)total;
  const unsigned nf = v.n_fields;
  for (unsigned wbase = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2; wbase < total; wbase += ngroups) {
    // ---- stage A: one key per group
    const unsigned it_raw = wbase + (unsigned)(lane >> 4);
    const bool active = it_raw < total;
    const unsigned g = active ? it_raw : total - 1;
    const i64 key = ks.dkeys[g];
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    const u64 b1 = bucket1(h, b0, v.nb);
    const i64 k0 = key_line(v, b0)[sub];
    bool hot = false;
    unsigned w = 0;
    if constexpr (SUMS) w = load_record(ks, g, sub, hot);
    const i64 word = probe_find_word(v, key, b0, b1, k0, sub, gshift);
    const bool hit = word >= 0;
    const unsigned char* const row_g = hit ? word_row_ptr(v, (u64)word) : default_row;
    if (active && sub == 0) keys_out[g] = key;
    // ---- stage B: the wave, key after key
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const int src = q * 16;
      if (!wave_word((unsigned)active, src)) continue;   // the last trip's groups beyond the list: skipped by the whole wave
      const bool q_hit = wave_word((unsigned)hit, src) != 0;
      const unsigned char* const row = wave_ptr(row_g, src);
      const unsigned fstep = q_hit ? v.field_bytes : 0u;
      const size_t out0 = (size_t)(wbase + (unsigned)q) * dim;
      bool q_hot = false;
      unsigned first = 0, nsrc = 1;
      if constexpr (SUMS) {
        q_hot = wave_word((unsigned)hot, src) != 0;
        first = wave_word(w, src + 3);
        nsrc = q_hot ? wave_word(w, src + 4) : wave_word(w, src + 2);
      }
      for (int c0 = 0; c0 < dim; c0 += WIDE_COLS) {
        const bool col = c0 + lane * 4 < dim;
        const int c = col ? c0 + lane * 4 : 0;
        GT r[MAXF];
        if (first_want >= 0) {
#pragma unroll
          for (int f = 0; f < MAXF; ++f) {
            const bool want = (unsigned)f < nf && ro.field[f] != nullptr;
            r[f] = *reinterpret_cast<const GT*>(row + (unsigned)(want ? f : first_want) * fstep + (unsigned)c * ES);
          }
        }
        float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (SUMS) gg = sum_rows_wide<false>(grads, partial, q_hot, w, first, nsrc, dim, c, src, 0.f, 0.f);
        if (first_want >= 0) {
          keep5(r);
#pragma unroll
          for (int f = 0; f < MAXF; ++f) {
            if ((unsigned)f < nf && ro.field[f] != nullptr && col) {
              float4 x = up4<ST>(r[f]);
              if (f >= 1 && !q_hit) x = aux4<ST>(ai.pattern[(f - 1) & 3]);
              *reinterpret_cast<float4*>(ro.field[f] + out0 + c) = x;
            }
          }
        }
        if constexpr (SUMS) {
          if (col) *reinterpret_cast<float4*>(gsum_out + out0 + c) = gg;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// store, stage B: row i of the caller's float32 fields into the table row, by the whole wave.  Per chunk the loads of every given
// field are issued together (a field that is not given: field 0 again); each element is rounded to the storage type once, to
// nearest even (to_stored4).  is_new: the row was claimed by this call — a field the caller does not give starts at aux_init
// (the granule of AuxInit::pattern, what fill_aux_field writes word by word); on a resident row it keeps its bytes.
template <int ST, bool WT>
__device__ __forceinline__ void write_row_wide(const TableView& v, const AuxInit& ai, unsigned char* row, const RowsIn& ri, size_t i,
                                               int dim, bool is_new, int lane) {
  constexpr unsigned ES = ST == TFRA_F32 ? 4u : 2u;
  const unsigned nf = v.n_fields;
  for (int c0 = 0; c0 < dim; c0 += WIDE_COLS) {
    const bool col = c0 + lane * 4 < dim;
    const int c = col ? c0 + lane * 4 : 0;
    float4 x0, x1, x2, x3, x4;
    auto x = [&](auto F) -> float4& {
      if constexpr (F == 0) return x0; else if constexpr (F == 1) return x1; else if constexpr (F == 2) return x2;
      else if constexpr (F == 3) return x3; else return x4;
    };
    for_fields<0>([&](auto F) {
      const bool given = (unsigned)F < nf && ri.field[F] != nullptr;
      x(F) = *reinterpret_cast<const float4*>((given ? ri.field[F] : ri.field[0]) + i * (size_t)dim + c);
    });
    keep_live(x0, x1, x2, x3);
    if (!col) continue;
    for_fields<0>([&](auto F) {
      if ((unsigned)F >= nf) return;
      unsigned char* p = row + (unsigned)F * v.field_bytes + (unsigned)c * ES;
      if (ri.field[F] != nullptr) {
        store_gran<ST, WT>(p, x(F));
      } else if (F >= 1 && is_new) {
        const unsigned pat = ai.pattern[(F - 1) & 3];
        if constexpr (ST == TFRA_F32) {
          const float a = __uint_as_float(pat);
          store_gran<ST, WT>(p, make_float4(a, a, a, a));
        } else {
          const u64 b = ((u64)pat << 32) | pat;
          if (WT) store_wt8(p, b);
          else *reinterpret_cast<u64*>(p) = b;
        }
      }
    });
  }
}

// phase 1: store_rows_kernel's probes, claim, score and accounting (tfra_rows.hip), one key per group and trip.
//   stage A: the wave's four first probes in flight (with b1's lines under pf1), then locate_or_claim_from with the twin's
//            bounded / pf1 handling; the deferred flag is set for NEED_EVICT and cleared for the buffer's rows beyond the count;
//   stage B: write_row_wide<ST, false>;   stage C: update_score; the wave's accounting behind the last trip.
template <int ST>
__device__ __forceinline__ void store_rows_wide_body(const TableView& v, size_t n_buf, const i64* __restrict__ keys, const RowsIn& ri,
                                                     int dim, const AuxInit& ai, int strategy, u64 epoch, int bounded,
                                                     uint8_t* __restrict__ deferred, const long long* __restrict__ d_n) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t stride = ((size_t)gridDim.x * blockDim.x) >> 4;
  size_t n = n_buf;
  if (d_n) {   // uniform load, as find_kernel's
    const long long dn = *d_n;
    n = dn < 0 ? 0 : min(n_buf, (size_t)dn);
  }
  int fresh = 0, failed = 0;
  const bool pf1 = bounded > 1;
  for (size_t base = wave << 2; base < n_buf; base += stride) {
    // ---- stage A: one key per group
    const size_t i = base + (size_t)grp;
    const bool active = i < n;
    if (deferred && sub == 0 && !active && i < n_buf) deferred[i] = 0;
    if (base >= n) continue;   // (wave-uniform)
    const i64 key = keys[active ? i : n - 1];
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    i64 k0 = load_key_coherent(key_line(v, b0) + sub);
    i64 k1 = load_key_coherent(key_line(v, pf1 ? bucket1(h, b0, v.nb) : b0) + sub);
    i64 d0 = k0, d1 = k1;
    keep_live(k0, k1, d0, d1);
    i64 row = -1;
    bool is_new = false;
    if (active) {
      // (two calls, not one with `pf1 ? &k1 : nullptr`: a pointer chosen at run time puts k1 into scratch)
      if (pf1) row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, bounded, &k1);
      else row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, bounded);
      if (deferred && sub == 0) deferred[i] = row == NEED_EVICT;
      if (row >= 0) fresh += (is_new && sub == 0);
      else if (row != NEED_EVICT) failed += (sub == 0);
    }
    const bool go = row >= 0;
    unsigned char* const pr_g = go ? row_ptr(v, row) : nullptr;
    // ---- stage B: the wave, key after key
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const int src = q * 16;
      if (!wave_word((unsigned)go, src)) continue;   // beyond the count, deferred or failed: skipped by the whole wave
      write_row_wide<ST, false>(v, ai, wave_ptr(pr_g, src), ri, base + (size_t)q, dim, wave_word((unsigned)is_new, src) != 0, lane);
    }
    // ---- stage C: per group
    if (go) update_score(v, row, is_new, strategy, 1, epoch, sub);
  }
  wave_account(v, wave, lane, fresh, failed);
}

// phase 2 (a table at max_capacity): store_rows_evict_kernel's victim choice, lock, score and publication (tfra_rows.hip).
//   stage A: evict_and_lock for the keys phase 1 deferred (a trip without one is skipped by the whole wave);
//   stage B: write_row_wide<ST, true> — a claimed row: fields that are not given at aux_init —, write-through;
//   stage C: the score reset, update_score<true> and publish_key, in the same trip.
// A slot locked in stage A is published in stage C of the same trip, and publish_key's wait covers the whole wave's stores of
// stage B: no wave waits on another (the ordering argument of apply_csr_wide_body<.., PHASE2 = true>).
// A key that is not admitted (-1) is dropped with its whole row.
template <int ST>
__device__ __forceinline__ void store_rows_wide_evict_body(const TableView& v, size_t n, const i64* __restrict__ keys, const RowsIn& ri,
                                                           int dim, const AuxInit& ai, int strategy, u64 epoch,
                                                           const uint8_t* __restrict__ deferred) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t stride = ((size_t)gridDim.x * blockDim.x) >> 4;
  int fresh = 0, failed = 0;
  const bool lru_like = strategy == TFRA_EVICT_LRU || strategy == TFRA_EVICT_EPOCHLRU;
  const u64 in_score = 1;
  const u64 compare = strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score;
  for (size_t base = wave << 2; base < n; base += stride) {
    // ---- stage A
    const size_t i = base + (size_t)grp;
    const bool active = i < n && deferred[i];
    if (!__builtin_amdgcn_readfirstlane((int)(__ballot(active) != 0))) continue;   // nothing deferred in this wave
    i64 row = -1, key = 0;
    u64 word = 0;
    bool claimed_empty = false;
    if (active) {
      key = keys[i];
      row = evict_and_lock(v, key, compare, lru_like, sub, gshift, &word, claimed_empty);
      if (row >= 0) fresh += (claimed_empty && sub == 0);
      else if (row == -3) failed += (sub == 0);
    }
    const bool go = row >= 0;
    unsigned char* const pr_g = go ? row_ptr(v, row) : nullptr;
    // ---- stage B
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const int src = q * 16;
      if (!wave_word((unsigned)go, src)) continue;
      write_row_wide<ST, true>(v, ai, wave_ptr(pr_g, src), ri, base + (size_t)q, dim, true, lane);
    }
    // ---- stage C: the slot is LOCKED by this group: its score, then the key
    if (go) {
      if (sub == 0) store_wt8(score_word(v, word), 0);  // the slot starts a new life: scores count from zero
      update_score<true>(v, row, true, strategy, in_score, epoch, sub);
      publish_key(v, word, key, sub);
    }
  }
  wave_account(v, wave, lane, fresh, failed);
}

}  // namespace
