// GRADIENT HALF of a write-back whose ids may repeat (tfra_table_apply_planned, over a CSR plan of tfra_csr.hip): the hot sums,
// then one fused optimizer update per unique key; the same sums written out instead (tfra_reduce_by_key, tfra_plan_reduce_to);
// the one-call and the two-stream forms (tfra_table_apply_sparse, tfra_table_step_prefetch[_assign]).
// The grouped combined write-back (tfra_multi_apply_planned_combined) stands on the grouped-call frame of tfra_many.h.  A write-back's
// argument checks exist once, check_apply_planned and check_apply_combined, for every entry point that makes them; the launch
// ladders are the dispatchers of tfra_host.h (with_opt_kind, with_stored) and with_nch, for single and grouped launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_optim_device.h"
#include "tfra_plan.h"
#include "tfra_reduce_device.h"

using namespace tfra;
using namespace tfra::red;

namespace {

#ifndef TFRA_HOT_SUMS_HALVES
#define TFRA_HOT_SUMS_HALVES 1   // hot_sums_kernel: 8 rows in flight, twice (0: 16 at once, the form of rounds 2-5; A/B)
#endif

// ---------------------------------------------------------------------------------------------
// gradient half, kernel 1: one block per bin of 512 entries = 32 items of 16 entries, one 16-lane group per item.
// Runs are item-aligned (csr_bucket_kernel pads every run to whole items), so an item belongs to exactly one run or to
// none: the group loads its 16 entry words with one coalesced read, puts all 16 gradient rows in flight at once
// (unconditional loads, padding clamped to the item's first row), adds them in entry order, and the group holding the
// run's first item then adds the sums of the run's following items in item order (LDS) and writes the partial row.
// CS = CombRows (tfra_table_apply_planned_combined): the gradient of position e is formed from grads = grad_out and the entry's
// record (tfra_combine_device.h) — each lane loads the record of its own entry, the group shares it by shuffles; none: grads[e].
template <class... CS>
__device__ __forceinline__ const CombEnt* comb_ent(const CS&... cs) {
  const CombEnt* p = nullptr;
  ((p = cs.ent), ...);
  return p;
}

// The body is one function with two callers — hot_sums_kernel (one plan per launch) and hot_sums_many_kernel (a list of plans per
// launch) — so that both compile the same expressions: blk = this block's index among the nblk blocks that work on THIS plan.
template <int NCH, class... CS>
__device__ __forceinline__ void hot_sums_body(const float* __restrict__ grads, int dim,
                                              const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                              const unsigned* __restrict__ binmap,
                                              const unsigned* __restrict__ d_counts, float* __restrict__ partial,
                                              unsigned* progress, unsigned progress_val, unsigned blk, unsigned nblk, const CS... cs) {
  constexpr bool COMB = sizeof...(CS) > 0;
  constexpr int NG = NTA / 16;
  __shared__ float s_sum[NG][64];
  __shared__ unsigned char s_kind[NG + 1];   // 0 = item continues the run of the item before, 1 = first item of a run, 2 = empty item
  // tfra_table_step_prefetch: host-visible progress counter (pinned memory) — this kernel running means the
  // lookup of step `progress_val` and every earlier step of the main stream are complete
  if (progress && blk == 0 && threadIdx.x == 0)
    __hip_atomic_store(progress, progress_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, g = threadIdx.x >> 4;
  const unsigned nbins = d_counts[PC_BINS];
  for (unsigned ib = blk; ib < nbins; ib += nblk) {
    const unsigned bin = binmap[ib];
    const unsigned e = hent[(size_t)bin * SEG + threadIdx.x];          // lane `sub` holds entry `sub` of the item
    const unsigned e0 = (unsigned)__shfl((int)e, gshift);
    const bool empty = (e0 & E_SKIP) != 0, first = (e0 & E_HEAD) != 0;
    const unsigned out_row = (first && !empty && sub == 0) ? hout[(size_t)bin * 32 + g] : 0u;
    const unsigned live = (unsigned)(__ballot(!(e & E_SKIP)) >> gshift) & 0xffffu;   // entries of the item that exist
    if (sub == 0) s_kind[g] = empty ? 2 : (first ? 1 : 0);
    if (threadIdx.x == 0) s_kind[NG] = 1;
    unsigned rows[16];   // element offset of each row (< 2^18 * 256)
    float cden = 0.f, cw = 0.f;   // COMB: denominator and weight of this lane's entry
    if constexpr (COMB) {
      const CombEnt ce = comb_ent(cs...)[((e & E_SKIP) ? e0 : e) & E_POS];   // (padding: the item's first row, as below)
      cden = ce.den;
      cw = ce.w;
#pragma unroll
      for (int j = 0; j < 16; ++j) rows[j] = (unsigned)__shfl((int)ce.row, gshift + j) * (unsigned)dim;
    } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned ej = (unsigned)__shfl((int)e, gshift + j);
      rows[j] = (((live >> j) & 1u) ? (ej & E_POS) : (e0 & E_POS)) * (unsigned)dim;
    }
    }
    for (int k = 0; k < NCH; ++k) {
      const int col = k * 64 + sub * 4;
      const int cc = col < dim ? col : 0;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (TFRA_HOT_SUMS_HALVES && NCH == 1) {   // (rows of more than 64 floats keep 16 in flight: their kernels are at 122-128 registers either way)
      // 8 rows in flight, twice, instead of 16 at once: 76 registers instead of 106 => 6 waves per SIMD instead of 4 => the ~680 bins of
      // a Zipf batch (512-thread blocks) are resident in ONE round instead of two; the second batch of loads costs a trip, the second round
      // cost more: 10.0 -> 9.2 us under rocprofv3, configs[1]'s step 56.7-57.3 -> 55.6-55.7 us (A/B on one box, twice).  Same adds, same order.
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float4 x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const float4*>(grads + rows[h * 8 + j] + cc);
        keep_live(x[0], x[1], x[2], x[3]); keep_live(x[4], x[5], x[6], x[7]);
        if constexpr (COMB) {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = comb_grad4(x[j], __shfl(cden, gshift + h * 8 + j), __shfl(cw, gshift + h * 8 + j));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if ((live >> (h * 8 + j)) & 1u) { acc.x += x[j].x; acc.y += x[j].y; acc.z += x[j].z; acc.w += x[j].w; }
      }
      } else {
      float4 x[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) x[j] = *reinterpret_cast<const float4*>(grads + rows[j] + cc);   // 16 rows in flight
      keep_live(x[0], x[1], x[2], x[3]); keep_live(x[4], x[5], x[6], x[7]);
      keep_live(x[8], x[9], x[10], x[11]); keep_live(x[12], x[13], x[14], x[15]);
      if constexpr (COMB) {
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = comb_grad4(x[j], __shfl(cden, gshift + j), __shfl(cw, gshift + j));
      }
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if ((live >> j) & 1u) { acc.x += x[j].x; acc.y += x[j].y; acc.z += x[j].z; acc.w += x[j].w; }
      }
      if (k) __syncthreads();   // the owners of the previous chunk have read s_sum
      *reinterpret_cast<float4*>(&s_sum[g][sub * 4]) = acc;
      __syncthreads();
      if (first && !empty) {
        for (int g2 = g + 1; s_kind[g2] == 0; ++g2) {
          const float4 y = *reinterpret_cast<const float4*>(&s_sum[g2][sub * 4]);
          acc.x += y.x; acc.y += y.y; acc.z += y.z; acc.w += y.w;
        }
        const unsigned orow = (unsigned)__shfl((int)out_row, gshift);
        if (col < dim) *reinterpret_cast<float4*>(partial + (size_t)orow * dim + col) = acc;
      }
    }
    __syncthreads();
  }
}

template <int NCH, class... CS>
__global__ __launch_bounds__(NTA) void hot_sums_kernel(const float* __restrict__ grads, int dim,
                                                       const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                                       const unsigned* __restrict__ binmap,
                                                       const unsigned* __restrict__ d_counts, float* __restrict__ partial,
                                                       unsigned* progress, unsigned progress_val, const CS... cs) {
  hot_sums_body<NCH>(grads, dim, hent, hout, binmap, d_counts, partial, progress, progress_val, blockIdx.x, gridDim.x, cs...);
}

// The source rows of a key's sum, NB of them in flight: rows j0 .. j0+NB-1 of its list (clamped to the last one; loads issued
// together, adds in list order).  A key with few occurrences lists their batch positions in words 4.. of its record (lane i
// of the group holds word i: EVERY lane of the group must be here); a key with many lists consecutive rows of the partial
// sums.  The addresses are formed here, from the record word, not kept in an array across the kernel: with 8 pointers and
// 8 rows held per lane the update kernel needed 145 registers (3 waves per SIMD); this form needs 125 (Adam) / 109 (SGD).
// COMB (combined write-back): lanes 4.. of a key with few occurrences hold grad_out rows instead of batch positions, and the
// denominator / weight of their entry in cden / cw; each gradient row is scaled by comb_grad4 before it is added.
template <int NB, bool COMB = false>
__device__ __forceinline__ void add_rows(float4& acc, const float* __restrict__ grads, const float* __restrict__ partial, bool hot,
                                         unsigned w, unsigned first, unsigned nsrc, unsigned j0, int dim, int c, int gshift,
                                         float cden = 0.f, float cw = 0.f) {
  float4 x[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const unsigned jj = min(j0 + (unsigned)j, nsrc - 1);
    const unsigned position = (unsigned)__shfl((int)w, gshift + 4 + (int)min(jj, 7u));
    const float* q = hot ? partial + (size_t)(first + jj) * dim : grads + (size_t)position * dim;
    x[j] = *reinterpret_cast<const float4*>(q + c);
  }
  if (NB == 4) keep_live(x[0], x[1], x[2], x[3]);
  if (COMB && !hot) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int src = gshift + 4 + (int)min(min(j0 + (unsigned)j, nsrc - 1), 7u);
      x[j] = comb_grad4(x[j], __shfl(cden, src), __shfl(cw, src));
    }
  }
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (j0 + (unsigned)j < nsrc) { acc.x += x[j].x; acc.y += x[j].y; acc.z += x[j].z; acc.w += x[j].w; }
}

// the whole sum of a key; wmax = the largest list length (capped at 8) among the wave's four keys: the trip count of the
// common part is uniform across the wave, the few keys with more than 8 partial rows go on alone
template <bool COMB = false>
__device__ __forceinline__ float4 sum_rows(const float* __restrict__ grads, const float* __restrict__ partial, bool hot, unsigned w,
                                           unsigned first, unsigned nsrc, unsigned wmax, int dim, int c, int gshift,
                                           float cden = 0.f, float cw = 0.f) {
  float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
  if (wmax <= 1) add_rows<1, COMB>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, gshift, cden, cw);
  else if (wmax <= 2) add_rows<2, COMB>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, gshift, cden, cw);
  else {
    add_rows<4, COMB>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, gshift, cden, cw);
    if (wmax > 4) add_rows<4, COMB>(gg, grads, partial, hot, w, first, nsrc, 4, dim, c, gshift, cden, cw);
  }
  for (unsigned j0 = 8; j0 < nsrc; j0 += 4) add_rows<4, COMB>(gg, grads, partial, hot, w, first, nsrc, j0, dim, c, gshift, cden, cw);
  return gg;
}

// ---------------------------------------------------------------------------------------------
// gradient half, kernel 2: one 16-lane group per unique key, hot keys first (their partial lists are the longest
// chains of the kernel: started first, they finish inside the kernel's duration).
// PHASE2: bounded (Hkv) table at max_capacity — the keys flagged in `dflag` (no free slot in phase 1; one byte per key:
// a list appended through ONE atomic counter cost 4 ns per key, 260 us for a batch of new keys) replace the minimum-score
// entry of their two home buckets and start from the default row / initial slot values, exactly like
// apply_evict_kernel (tfra_optim.hip).
// (Tried: amdgpu_waves_per_eu(4) on the 145-register form — 128 VGPRs with 7 spilled: gradient half 32.5 us instead of 31.5.
// Without the pointer arrays — add_rows — it is 125 registers, 4 waves per SIMD, no spills: 28.7 us, step 57.2 instead of 59.9 us.
// Round 4: amdgpu_waves_per_eu(5, 5) on that form — 96 registers, 18 spilled for Adam: gradient half 28.7 -> 37.3 us, the step of
// configs[1] 55.4 -> 62.3 us (A/B on one box, twice).  Five waves need a kernel that NEEDS 96 registers, not one that spills to them.)
// CS = CombRows: the combined write-back (see hot_sums_kernel).
// ST: storage type of the rows (TFRA_F32 / TFRA_F16 / TFRA_BF16).  A half / bfloat16 row is read as ONE 8-byte granule per lane
// and field (4 stored elements; the group's 16 lanes = one 128-byte line), up-cast, updated in fp32 exactly like a float row,
// rounded to the storage type once (to_stored) and written back as one 8-byte write-through store per field.  A new row starts
// from the FLOAT default row and aux_init values, not from their rounded images (as apply_kernel / apply_evict_kernel do).
// Gradients and partial sums are fp32 for every ST.  The float instantiations compile the code they always did (if constexpr).
// The body is one function with two callers — apply_csr_kernel (one table per launch) and apply_csr_many_kernel (a list of tables
// per launch): blk = this block's index among the nblk blocks that work on THIS table's plan; they stand where the block index and
// the grid size of the launch stood, and nothing else differs.
template <int KIND, bool PHASE2, int ST, class... CS>
__device__ __forceinline__ void apply_csr_body(const TableView& v, OptP o, int dim, const float* __restrict__ grads,
                                               const float* __restrict__ partial, const CsrKeys& ks,
                                               const float* __restrict__ default_row, float aux0, float aux1,
                                               const ScoreP& sp, uint8_t* __restrict__ dflag, unsigned* any_deferred,
                                               unsigned use_gen, unsigned blk, unsigned nblk, const CS... cs) {
  constexpr bool COMB = sizeof...(CS) > 0;
  if (PHASE2 && *any_deferred != use_gen) return;   // phase 1 of this use deferred nothing
  constexpr int S = NSlots<KIND>::v;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  const unsigned ngroups = (nblk * blockDim.x) >> 4;
  int fresh = 0, failed = 0;
  if (o.d_lr) o.lr = *o.d_lr;
  if (!PHASE2 && blk == 0 && threadIdx.x == 0 && ks.d_counts[PC_OVERFLOW]) atomicAdd(v.err_count, ks.d_counts[PC_OVERFLOW]);  // plan overflow
  // trips are uniform per wave (the batch width below is a wave-wide maximum): a group past the end re-reads the
  // last key's records and does nothing else
  for (unsigned wbase = ((blk * blockDim.x + threadIdx.x) >> 6) << 2; wbase < total; wbase += ngroups) {
    const unsigned it_raw = wbase + (unsigned)(lane >> 4);
    const bool active = it_raw < total;
    const unsigned g = active ? it_raw : total - 1;
    if (PHASE2 && !__builtin_amdgcn_readfirstlane((int)(__ballot(active && dflag[g]) != 0))) continue;   // nothing deferred in this wave
    // two chains in flight: key -> first probe line, and keymap -> record -> source rows
    const i64 key = ks.dkeys[g];
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    i64 k0 = 0;
    if (!PHASE2) k0 = load_key_coherent(key_line(v, b0) + sub);
    bool hot;
    const unsigned w = load_record(ks, g, sub, hot);
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    const unsigned first = (unsigned)__shfl((int)w, gshift + 3);             // keys with many occurrences: first partial row
    const unsigned nsrc = hot ? (unsigned)__shfl((int)w, gshift + 4) : cnt;
    // COMB: lane 4 + j of a key with few occurrences swaps batch position j for that entry's grad_out row (+ denominator, weight)
    unsigned wsrc = w;
    float cden = 0.f, cw = 0.f;
    if constexpr (COMB) {
      if (!hot && sub >= 4 && (unsigned)(sub - 4) < cnt) {
        const CombEnt ce = comb_ent(cs...)[w];
        wsrc = ce.row; cden = ce.den; cw = ce.w;
      }
    }
    // wave-uniform batch width: 1 / 2 / 4 rows in flight (most keys of a Zipf batch occur once)
    unsigned wmax = min(nsrc, 8u);
    for (int o2 = 32; o2 >= 16; o2 >>= 1) wmax = max(wmax, (unsigned)__shfl_xor((int)wmax, o2));
    wmax = (unsigned)__builtin_amdgcn_readfirstlane((int)wmax);
    if (!active || (PHASE2 && !dflag[g])) continue;
    i64 row;
    bool is_new = false;
    u64 word = 0;
    bool claimed_empty = false;
    if (PHASE2) {
      const bool lru_like = sp.strategy == TFRA_EVICT_LRU || sp.strategy == TFRA_EVICT_EPOCHLRU;
      const u64 in_score = sp.strategy == TFRA_EVICT_EPOCHLFU ? ((sp.epoch << 32) | 1) : 1;
      row = evict_and_lock(v, key, in_score, lru_like, sub, gshift, &word, claimed_empty);
      is_new = true;
    } else {
      row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, sp.bounded);
      if (sp.bounded && sub == 0) {
        dflag[g] = row == NEED_EVICT;
        if (row == NEED_EVICT) *any_deferred = use_gen;
      }
    }
    if (row < 0) {
      failed += (sub == 0 && (PHASE2 ? row == -3 : row != NEED_EVICT));
      continue;
    }
    fresh += ((PHASE2 ? claimed_empty : is_new) && sub == 0);
    float* pr = reinterpret_cast<float*>(row_ptr(v, row));
    // (every lane of the group takes every trip — sum_rows reads the record words of the other lanes; a lane beyond the row
    // works on column 0 and stores nothing)
    if constexpr (ST != TFRA_F32) {
      typedef typename Stored<ST>::T V;
      V* sr = reinterpret_cast<V*>(pr);   // fields of dim * 2 bytes: 8-byte aligned at every c % 4 == 0 (dim % 4 == 0, rows 16-byte aligned)
      for (int c0 = 0; c0 < dim; c0 += 64) {
        const bool col = c0 + sub * 4 < dim;
        const int c = col ? c0 + sub * 4 : 0;
        // all loads unconditional and issued together (a brand-new row reads its own not yet initialised bytes and discards them)
        uint2 rp = *reinterpret_cast<const uint2*>(sr + c);
        uint2 r1 = *reinterpret_cast<const uint2*>(sr + (S >= 1 ? dim : 0) + c);
        uint2 r2 = *reinterpret_cast<const uint2*>(sr + (S >= 2 ? 2 * dim : 0) + c);
        const float4 dflt = *reinterpret_cast<const float4*>(default_row + c);
        float4 gg = sum_rows<COMB>(grads, partial, hot, COMB ? wsrc : w, first, nsrc, wmax, dim, c, gshift, cden, cw);
        uint2 dummy = rp;
        keep_live(dummy, rp, r1, r2);
        float4 p = is_new ? dflt : load_stored4<ST>(rp);
        float4 s1 = (is_new || S < 1) ? make_float4(aux0, aux0, aux0, aux0) : load_stored4<ST>(r1);
        float4 s2 = (is_new || S < 2) ? make_float4(aux1, aux1, aux1, aux1) : load_stored4<ST>(r2);
        apply_one<KIND>(o, gg.x, p.x, s1.x, s2.x);
        apply_one<KIND>(o, gg.y, p.y, s1.y, s2.y);
        apply_one<KIND>(o, gg.z, p.z, s1.z, s2.z);
        apply_one<KIND>(o, gg.w, p.w, s1.w, s2.w);
        // write-through, one rounding per element (PHASE2: in memory before publish_key)
        if (col) {
          store_wt8(sr + c, to_stored4<ST>(p));
          if (S >= 1) store_wt8(sr + dim + c, to_stored4<ST>(s1));
          if (S >= 2) store_wt8(sr + 2 * dim + c, to_stored4<ST>(s2));
        }
      }
      // aux fields the optimizer does not own (table created with more slots than it uses)
      if (is_new && (int)v.n_fields - 1 > S) {
        for (int f = S + 1; f < (int)v.n_fields; ++f) {
          const float a = f == 1 ? aux0 : aux1;
          const u64 a4 = to_stored4<ST>(make_float4(a, a, a, a));
          for (int c = sub * 4; c < dim; c += 64) store_wt8(sr + f * dim + c, a4);
        }
      }
    } else {
    for (int c0 = 0; c0 < dim; c0 += 64) {
      const bool col = c0 + sub * 4 < dim;
      const int c = col ? c0 + sub * 4 : 0;
      float4 p = *reinterpret_cast<const float4*>((is_new ? default_row : pr) + c);
      float4 s1 = *reinterpret_cast<const float4*>(pr + (S >= 1 ? dim : 0) + c);
      float4 s2 = *reinterpret_cast<const float4*>(pr + (S >= 2 ? 2 * dim : 0) + c);
      float4 gg = sum_rows<COMB>(grads, partial, hot, COMB ? wsrc : w, first, nsrc, wmax, dim, c, gshift, cden, cw);
      float4 dummy = p;
      keep_live(dummy, p, s1, s2);
      if (is_new || S < 1) s1 = make_float4(aux0, aux0, aux0, aux0);
      if (is_new || S < 2) s2 = make_float4(aux1, aux1, aux1, aux1);
      apply_one<KIND>(o, gg.x, p.x, s1.x, s2.x);
      apply_one<KIND>(o, gg.y, p.y, s1.y, s2.y);
      apply_one<KIND>(o, gg.z, p.z, s1.z, s2.z);
      apply_one<KIND>(o, gg.w, p.w, s1.w, s2.w);
      // write-through: the rows leave L2 during the kernel, not at the boundary to the next one
      if (col) {
        store_wt16(pr + c, *reinterpret_cast<uint4*>(&p));
        if (S >= 1) store_wt16(pr + dim + c, *reinterpret_cast<uint4*>(&s1));
        if (S >= 2) store_wt16(pr + 2 * dim + c, *reinterpret_cast<uint4*>(&s2));
      }
    }
    // aux fields the optimizer does not own (table created with more slots than it uses)
    if (is_new && (int)v.n_fields - 1 > S) {
      for (int f = S + 1; f < (int)v.n_fields; ++f)
        for (int c = sub; c < dim; c += 16)
          __hip_atomic_store(pr + f * dim + c, (f == 1 ? aux0 : aux1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    }
    if (PHASE2) {
      if (sub == 0) store_wt8(score_word(v, word), 0);  // the slot starts a new life
      update_score<true>(v, row, true, sp.strategy, 1, sp.epoch, sub);
      publish_key(v, word, key, sub);
    } else {
      update_score(v, row, is_new, sp.strategy, 1, sp.epoch, sub);  // one write-back = one upsert
    }
  }
  for (int off = 32; off > 0; off >>= 1) { fresh += __shfl_xor(fresh, off); failed += __shfl_xor(failed, off); }
  if (lane == 0) {
    if (fresh) size_add(v, (blk * blockDim.x + threadIdx.x) >> 6, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

template <int KIND, bool PHASE2, int ST, class... CS>
__global__ __launch_bounds__(256) void apply_csr_kernel(TableView v, OptP o, int dim, const float* __restrict__ grads,
                                                        const float* __restrict__ partial, CsrKeys ks,
                                                        const float* __restrict__ default_row, float aux0, float aux1,
                                                        ScoreP sp, uint8_t* __restrict__ dflag, unsigned* any_deferred,
                                                        unsigned use_gen, const CS... cs) {
  apply_csr_body<KIND, PHASE2, ST>(v, o, dim, grads, partial, ks, default_row, aux0, aux1, sp, dflag, any_deferred, use_gen,
                                   blockIdx.x, gridDim.x, cs...);
}

// ---- the grouped form (tfra_multi_apply_planned_combined): the combined write-backs of a LIST of tables, one sums launch per NCH
// class and one update launch per (rule, storage type) class.  What a single-table launch takes as kernel arguments is a record
// in device memory here (tfra_pool.hip: 26 tables' records do not fit the 4 KB of kernel arguments).  A class is a list of record
// indices `idx` and the blocks' prefix sums over it: the grid is the concatenation of the class's descriptors, descriptor j owning
// the blocks [prefix[j], prefix[j + 1]), and both kernels stride by THAT count.  blockIdx.x is wave-uniform, so the search, the
// index and the record are scalar loads into scalar registers, as kernel arguments are.
struct ApplyManyRec {
  TableView v;
  OptP o;
  ScoreP sp;
  CsrKeys ks;                 // (ks.hent, ks.d_counts: also the sums')
  const float* grads;         // grad_out
  float* partial;
  const float* default_row;
  const unsigned* hout;
  const unsigned* binmap;
  uint8_t* dflag;
  unsigned* any_deferred;
  const CombEnt* ent;         // this descriptor's entry records
  int dim;
  float aux0, aux1;
  unsigned use_gen;
};

template <int NCH>
__global__ __launch_bounds__(NTA) void hot_sums_many_kernel(const ApplyManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                            const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const unsigned first = prefix[d], nblk = prefix[d + 1] - first;
  const ApplyManyRec rec = recs[idx[d]];
  hot_sums_body<NCH>(rec.grads, rec.dim, rec.ks.hent, rec.hout, rec.binmap, rec.ks.d_counts, rec.partial, nullptr, 0u, blockIdx.x - first,
                     nblk, CombRows{rec.ent});
}

// PHASE2: the class's grid again; the blocks of a table that can still grow have nothing to do (the single call does not launch it)
template <int KIND, bool PHASE2, int ST>
__global__ __launch_bounds__(256) void apply_csr_many_kernel(const ApplyManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                             const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const unsigned first = prefix[d], nblk = prefix[d + 1] - first;
  const ApplyManyRec rec = recs[idx[d]];
  if (PHASE2 && !rec.sp.bounded) return;
  apply_csr_body<KIND, PHASE2, ST>(rec.v, rec.o, rec.dim, rec.grads, rec.partial, rec.ks, rec.default_row, rec.aux0, rec.aux1, rec.sp,
                                   rec.dflag, rec.any_deferred, rec.use_gen, blockIdx.x - first, nblk, CombRows{rec.ent});
}

// ---------------------------------------------------------------------------------------------
// tfra_reduce_by_key epilogue: the same per-key sums as apply_csr_kernel, written out instead of applied.
// dest != nullptr (tfra_plan_reduce_to): the sum of a key goes to row dest[p], p = the key's last batch position — the
// caller's map from batch positions to output rows (equal for all positions of a key), e.g. position -> owner-major
// index of the multi-GPU gradient route; keys_out / d_count are not written then.
__global__ __launch_bounds__(256) void gather_csr_kernel(int dim, const float* __restrict__ grads,
                                                         const float* __restrict__ partial, CsrKeys ks,
                                                         i64* __restrict__ keys_out, float* __restrict__ rows_out,
                                                         i64* __restrict__ d_count, const int* __restrict__ dest) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  const unsigned ngroups = (gridDim.x * blockDim.x) >> 4;
  if (d_count && blockIdx.x == 0 && threadIdx.x == 0) *d_count = ks.d_counts[PC_OVERFLOW] ? (i64)-1 : (i64)total;
  for (unsigned wbase = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2; wbase < total; wbase += ngroups) {
    const unsigned it_raw = wbase + (unsigned)(lane >> 4);
    const bool active = it_raw < total;
    const unsigned g = active ? it_raw : total - 1;
    bool hot;
    const unsigned w = load_record(ks, g, sub, hot);
    const i64 key = (i64)(((u64)(unsigned)__shfl((int)w, gshift + 1) << 32) | (unsigned)__shfl((int)w, gshift));
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    const unsigned first = (unsigned)__shfl((int)w, gshift + 3);
    const unsigned nsrc = hot ? (unsigned)__shfl((int)w, gshift + 4) : cnt;
    unsigned wmax = min(nsrc, 8u);
    for (int o2 = 32; o2 >= 16; o2 >>= 1) wmax = max(wmax, (unsigned)__shfl_xor((int)wmax, o2));
    wmax = (unsigned)__builtin_amdgcn_readfirstlane((int)wmax);
    if (!active) continue;
    size_t orow = g;
    if (dest) {
      unsigned lastp = (unsigned)__shfl((int)w, gshift + (hot ? 5 : 3));   // few: the last position itself; many: where it is stored
      if (hot) lastp = ks.hent[lastp];
      orow = (size_t)dest[lastp & E_POS];
    }
    for (int c0 = 0; c0 < dim; c0 += 64) {   // (every lane takes every trip: see apply_csr_kernel)
      const bool col = c0 + sub * 4 < dim;
      const int c = col ? c0 + sub * 4 : 0;
      const float4 gg = sum_rows(grads, partial, hot, w, first, nsrc, wmax, dim, c, gshift);
      if (col) *reinterpret_cast<float4*>(rows_out + orow * dim + c) = gg;
    }
    if (keys_out && sub == 0) keys_out[g] = key;
  }
}

}  // namespace

// NCH of the sums, the row's chunks of 64 floats: f(std::integral_constant<int, NCH>{}) for nch in 1..4
template <class F>
static void with_nch(int nch, F&& f) {
  switch (nch) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

template <class... CS>
static void launch_hot_sums(hipStream_t s, const tfra_sparse_plan* pl, const float* grads, unsigned bin_blocks, unsigned* progress,
                            unsigned progress_val, const CS&... cs) {
  const int dim = pl->dim;
  with_nch((dim + 63) / 64, [&](auto NCH) {
    hot_sums_kernel<NCH><<<bin_blocks, NTA, 0, s>>>(grads, dim, pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->partial, progress,
                                                    progress_val, cs...);
  });
}

// by the rule and by the rows' storage type (both checked by the caller)
template <class... CS>
static void launch_apply(Table* t, hipStream_t s, const tfra_sparse_plan* pl, int kind, const OptP& o, const float* grads,
                         const float* default_row, unsigned key_blocks, const ScoreP& sp, const CS&... cs) {
  TableView v = t->view_of(t->cur);
  const float a0 = t->opts.aux_init[0], a1 = t->opts.aux_init[1];
  const unsigned gen = ++pl->use_gen;
  // one RESIDENT grid (the kernel is grid-stride: 125 registers = 4 blocks per CU x 256 CUs): a batch's 33 K keys as 2075 blocks were two
  // rounds of dispatch plus a third of 27 blocks; 1024 blocks looping twice: configs[1] 55.2 -> 53.7 us per step (A/B on one box, twice)
  static const unsigned grid_cap = [] { const char* e = getenv("TFRA_APPLY_GRID_CAP"); return e ? (unsigned)atoi(e) : 1024u; }();
  if (grid_cap) key_blocks = std::min(key_blocks, grid_cap);
  with_opt_kind(kind, [&](auto KIND) {
    with_stored(st_index(t->opts.value_dtype), [&](auto ST) {
      apply_csr_kernel<KIND, false, ST><<<key_blocks, 256, 0, s>>>(v, o, pl->dim, grads, pl->partial, keys_of(pl), default_row, a0, a1, sp,
                                                                   pl->dflag, pl->any_deferred, gen, cs...);
      if (sp.bounded)
        apply_csr_kernel<KIND, true, ST><<<key_blocks, 256, 0, s>>>(v, o, pl->dim, grads, pl->partial, keys_of(pl), default_row, a0, a1, sp,
                                                                    pl->dflag, pl->any_deferred, gen, cs...);
    });
  });
}

// The checks of a planned write-back: apply_planned_impl's, whoever calls it, and behind check_apply_combined those of a
// descriptor of tfra_multi_apply_planned_combined.  active: the plan holds ids.
template <class AtEntry>
static Check check_apply_planned(const Table* t, const tfra_opt_params* p, const tfra_sparse_plan* pl, const float* grads,
                                 const float* param_default_row, AtEntry&& at_entry) {
  if (!t || !p || !pl) return refuse(TFRA_ERR_INVALID, "null argument");
  if (Check e = at_entry(); e.done()) return e;
  if (pl->n == 0) return nothing_to_do();
  if (!grads || !param_default_row) return refuse(TFRA_ERR_INVALID, "null buffer");
  const int dt = t->opts.value_dtype;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16 (gradients and the default row are float32)");
  if (p->kind < 0 || p->kind > TFRA_OPT_FTRL) return refuse(TFRA_ERR_INVALID, "unknown kind");
  const int need = p->kind == TFRA_OPT_SGD ? 0 : (p->kind == TFRA_OPT_ADAGRAD ? 1 : 2);
  if (t->opts.aux_fields < need) return refuse(TFRA_ERR_INVALID, "table lacks optimizer slot fields");
  if (t->opts.dim != pl->dim) return refuse(TFRA_ERR_INVALID, "the plan was built for another dim");
  if (t->opts.device != pl->device && t->opts.device >= 0) return refuse(TFRA_ERR_INVALID, "plan and table live on different devices");
  if ((((uintptr_t)grads | (uintptr_t)param_default_row) & 15)) return refuse(TFRA_ERR_UNSUPPORTED, "gradient / default buffers must be 16-B aligned");
  return Check{};
}

// comb != nullptr (tfra_table_apply_planned_combined): grads is grad_out, position e's gradient is formed from comb[e]
int tfra::apply_planned_impl(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl, const float* grads,
                              const float* param_default_row, tfra_stream_t stream, unsigned* progress, unsigned progress_val,
                             const CombEnt* comb) {
  // caller holds t->mu
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  const Check c = check_apply_planned(t, p, pl, grads, param_default_row, [&] { return Check{t->enter(s)}; });
  if (c.code) return report("apply_planned: ", c);
  if (!c.active) return TFRA_OK;
  int rc = t->prepare_insert(pl->n, s);
  if (rc) return rc;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  if (comb) launch_hot_sums(s, pl, grads, bin_blocks, progress, progress_val, CombRows{comb});
  else launch_hot_sums(s, pl, grads, bin_blocks, progress, progress_val);
  uint8_t* bounded_now;
  rc = t->bounded_flags(1, s, &bounded_now);
  if (rc) return rc;
  const ScoreP sp{t->opts.strategy, t->global_epoch, bounded_now ? (t->dense ? 2 : 1) : 0};
  OptP o{p->kind, p->lr, p->beta1, p->beta2, p->eps, p->l1, p->l2, p->lr_power, p->d_lr};
  if (comb) launch_apply(t, s, pl, p->kind, o, grads, param_default_row, key_blocks, sp, CombRows{comb});
  else launch_apply(t, s, pl, p->kind, o, grads, param_default_row, key_blocks, sp);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "apply_planned: launch failed");
  t->step_epoch();
  return TFRA_OK;
}

extern "C" int tfra_table_apply_planned(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                        const float* grads, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "apply_planned: null table");
  std::lock_guard<std::mutex> lock(t->mu);
  return apply_planned_impl(tp, p, pl, grads, param_default_row, stream, nullptr, 0);
}

// The checks tfra_table_apply_planned_combined makes before it forms the entry records (apply_planned_impl's follow behind them),
// also the first half of a descriptor's.  active: the plan holds ids.
template <class AtEntry>
static Check check_apply_combined(const Table* t, const tfra_opt_params* p, const tfra_sparse_plan* pl, const float* grad_out,
                                  const int64_t* seg, const float* weights, int combiner, size_t n_rows, const float* param_default_row,
                                  AtEntry&& at_entry) {
  if (!t || !p || !pl) return refuse(TFRA_ERR_INVALID, "null argument");
  if (combiner < 0 || combiner > 2) return refuse(TFRA_ERR_INVALID, "combiner must be 0 (sum), 1 (mean) or 2 (sqrtn)");
  if (Check e = at_entry(); e.done()) return e;
  if (pl->kind != 0 || pl->dim != t->opts.dim) return refuse(TFRA_ERR_INVALID, "the plan was built for another dim");
  if (t->opts.device != pl->device && t->opts.device >= 0) return refuse(TFRA_ERR_INVALID, "plan and table live on different devices");
  if (pl->n == 0) return nothing_to_do();
  if (!grad_out || !seg || !param_default_row) return refuse(TFRA_ERR_INVALID, "null buffer");
  if (n_rows == 0 || n_rows >= (1ULL << 30)) return refuse(TFRA_ERR_INVALID, "need 1 <= n_rows < 2^30");
  if ((((uintptr_t)grad_out | (uintptr_t)param_default_row) & 15) || ((uintptr_t)seg & 7) || ((uintptr_t)weights & 3))
    return refuse(TFRA_ERR_UNSUPPORTED, "grad_out / default buffers must be 16-B aligned");
  return Check{};
}

// The write-back of an embedding_lookup_sparse: plan over the entry ids, gradient of position e = the combiner's backward
// (tfra_combine_device.h) formed from grad_out in registers — apply_planned's kernels, reading grad_out through one more
// indirection instead of an expanded [nnz, dim] gradient.
extern "C" int tfra_table_apply_planned_combined(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                                 const float* grad_out, const int64_t* seg, const float* weights, int combiner,
                                                 size_t n_rows, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  const Check c = check_apply_combined(t, p, pl, grad_out, seg, weights, combiner, n_rows, param_default_row, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};   // the scratch below was last used on the table's previous stream
  });
  if (c.code) return report("apply_planned_combined: ", c);
  if (!c.active) return TFRA_OK;
  const size_t nnz = pl->n;
  int rc;
  if (!t->comb_ws) {
    tfra_workspace_t* w = nullptr;
    rc = tfra_workspace_create(t->device, &w);
    if (rc) return rc;
    t->comb_ws = w;
  }
  tfra_workspace_t* ws = reinterpret_cast<tfra_workspace_t*>(t->comb_ws);
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t se_b = al(2 * n_rows * sizeof(int)), den_b = al(n_rows * sizeof(float));
  rc = ws->ensure(se_b + den_b + al(nnz * sizeof(CombEnt)), s);
  if (rc) return rc;
  unsigned char* b = (unsigned char*)ws->buf;
  CombEnt* ent = reinterpret_cast<CombEnt*>(b + se_b + den_b);
  rc = comb_entries(s, nnz, seg, weights, combiner, n_rows, reinterpret_cast<int*>(b), reinterpret_cast<float*>(b + se_b), ent);
  if (rc) return rc;
  return apply_planned_impl(tp, p, pl, grad_out, param_default_row, stream, nullptr, 0, ent);
}

// ---------------------------------------------------------------------------------------------
// tfra_multi_apply_planned_combined: the call above for a LIST of tables, with launches that do not grow with the list.
namespace {

constexpr unsigned MANY_GRID_CAP = 1024;   // blocks of one grouped launch (see many_cap)

// Blocks a descriptor may own in a class of n_in_class descriptors.  The single call caps the update's grid at 1024 blocks — one
// resident round of the 125-register kernel, 4 blocks per CU x 256 CUs — and the plans' host-side grids are upper bounds (2048
// key blocks, up to 1024 bin blocks for a batch whose counts the host has not seen), mostly idle for a small batch.  The cap is
// shared: 1024 / n blocks each, so that a class of 26 descriptors is ~1014 blocks, not 26 x 1024.  A class of one descriptor has
// the single call's grid.  Both kernels stride by the descriptor's own block count, so results do not depend on it.
unsigned many_cap(unsigned blocks, unsigned n_in_class) {
  return std::max(1u, std::min(blocks, MANY_GRID_CAP / std::max(1u, n_in_class)));
}

void launch_apply_many(hipStream_t s, int st, int kind, bool phase2, unsigned grid, const ApplyManyRec* recs, const unsigned* prefix,
                       const unsigned* idx, unsigned n) {
  with_opt_kind(kind, [&](auto KIND) {
    with_stored(st, [&](auto ST) {
      if (phase2) apply_csr_many_kernel<KIND, true, ST><<<grid, 256, 0, s>>>(recs, prefix, idx, n);
      else apply_csr_many_kernel<KIND, false, ST><<<grid, 256, 0, s>>>(recs, prefix, idx, n);
    });
  });
}

void launch_hot_sums_many(hipStream_t s, int nch, unsigned grid, const ApplyManyRec* recs, const unsigned* prefix, const unsigned* idx,
                          unsigned n) {
  with_nch(nch, [&](auto NCH) { hot_sums_many_kernel<NCH><<<grid, NTA, 0, s>>>(recs, prefix, idx, n); });
}

// A descriptor's checks: the single call's (check_apply_combined, then check_apply_planned), with what only a descriptor can get
// wrong where the single call enters its table.  A plan that holds no ids is skipped there: it was built for no dim
// (tfra_sparse_plan_build), and the single call is not made with one.
Check check_apply_desc(const tfra_apply_combined_desc& d, const tfra_workspace* ws) {
  if (d.struct_size != sizeof(tfra_apply_combined_desc)) return refuse(TFRA_ERR_INVALID, "descriptor size mismatch");
  const Table* t = reinterpret_cast<const Table*>(d.table);
  Check c = check_apply_combined(t, d.opt, d.plan, d.grad_out, d.seg, d.weights, d.combiner, d.n_rows, d.param_default_row, [&] {
    if (ws->device != t->device) return refuse(TFRA_ERR_INVALID, "workspace and table live on different devices");
    return d.plan->n == 0 ? nothing_to_do() : Check{};
  });
  if (c.done()) return c;
  c = check_apply_planned(t, d.opt, d.plan, d.grad_out, d.param_default_row, [] { return Check{}; });
  if (c.done()) return c;
  const int dim = t->opts.dim;   // (hot_sums' classes: NCH 1..4)
  if (dim <= 0 || dim % 4 != 0 || dim > 64 * MAXCH) return refuse(TFRA_ERR_UNSUPPORTED, "needs dim % 4 == 0 and dim <= 256");
  return Check{};
}

}  // namespace

extern "C" int tfra_multi_apply_planned_combined(tfra_workspace_t* ws, size_t n_tables, const tfra_apply_combined_desc* descs,
                                                 uint32_t* launches_out, tfra_stream_t stream) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, "multi_apply_planned_combined: null argument");
  hipStream_t s = (hipStream_t)stream;
  const std::string who = "multi_apply_planned_combined: descriptor ";
  // every descriptor is checked before anything is enqueued and before any table is touched
  std::vector<size_t> act;   // the descriptors with work, in input order: record k belongs to descs[act[k]]
  for (size_t i = 0; i < n_tables; ++i) {
    const Check c = check_apply_desc(descs[i], ws);
    if (c.code) return report(who + std::to_string(i) + ": ", c);
    if (c.active) act.push_back(i);
  }
  // two descriptors on one table would be two writers of one key inside one launch; a plan's partial sums and flags are one use's
  for (size_t i = 0; i < n_tables; ++i)
    for (size_t j = i + 1; j < n_tables; ++j) {
      if (descs[i].table == descs[j].table)
        return set_error(TFRA_ERR_INVALID, who + std::to_string(i) + " and descriptor " + std::to_string(j) + " name the same table");
      if (descs[i].plan == descs[j].plan)
        return set_error(TFRA_ERR_INVALID, who + std::to_string(i) + " and descriptor " + std::to_string(j) + " name the same plan");
    }
  const size_t n_act = act.size();
  if (n_act == 0) return TFRA_OK;

  // classes: the sums by NCH (1..4), the update by (rule, storage type)
  constexpr int NHOT = 4, NAPP = 12;
  auto ent_blocks_of = [&](size_t k) { return (unsigned)((descs[act[k]].plan->n + 255) / 256); };
  auto den_blocks_of = [&](size_t k) { return (unsigned)((descs[act[k]].n_rows + 255) / 256); };
  std::vector<int> hot_of(n_act), app_of(n_act);
  unsigned hot_n[NHOT] = {}, app_n[NAPP] = {};
  u64 ent_blocks = 0, den_blocks = 0;
  size_t se_ints = 0, den_floats = 0, ent_recs = 0;
  for (size_t k = 0; k < n_act; ++k) {
    const tfra_apply_combined_desc& d = descs[act[k]];
    const Table* t = reinterpret_cast<const Table*>(d.table);
    hot_of[k] = (t->opts.dim + 63) / 64 - 1;
    app_of[k] = d.opt->kind * 3 + st_index(t->opts.value_dtype);
    ++hot_n[hot_of[k]];
    ++app_n[app_of[k]];
    ent_blocks += ent_blocks_of(k);
    den_blocks += den_blocks_of(k);
    se_ints += (2 * d.n_rows + 63) / 64 * 64;
    den_floats += (d.n_rows + 63) / 64 * 64;
    ent_recs += (d.plan->n + 15) / 16 * 16;
  }
  if (ent_blocks >= (1ULL << 31) || den_blocks >= (1ULL << 31))
    return set_error(TFRA_ERR_UNSUPPORTED, "multi_apply_planned_combined: too many rows in one call");

  std::vector<Table*> tabs;
  tabs.reserve(n_act);
  for (size_t i : act) tabs.push_back(reinterpret_cast<Table*>(descs[i].table));
  std::vector<std::unique_lock<std::mutex>> locks;
  int rc = lock_and_enter(std::move(tabs), s, &locks);
  if (rc) return rc;
  // capacity, as the single call prepares it: a table may grow here, so the views are taken afterwards
  std::vector<int> bounded(n_act, 0);
  bool app_evict[NAPP] = {};   // a table at max_capacity in the class: the class runs its eviction phase
  for (size_t k = 0; k < n_act; ++k) {
    Table* t = reinterpret_cast<Table*>(descs[act[k]].table);
    rc = t->prepare_insert(descs[act[k]].plan->n, s);
    if (rc) return rc;
    uint8_t* bounded_now = nullptr;
    rc = t->bounded_flags(1, s, &bounded_now);
    if (rc) return rc;
    bounded[k] = bounded_now ? (t->dense ? 2 : 1) : 0;
    app_evict[app_of[k]] = app_evict[app_of[k]] || bounded[k] != 0;
  }

  // device memory: [bounds of all rows | denominators | entry records | blob], the blob = [update records | bounds records |
  // entry-kernel records | unsigned pool: entry prefix, row prefix, then per class present its prefix and its record indices]
  const size_t se_bytes = se_ints * sizeof(int), den_bytes = den_floats * sizeof(float), ent_bytes = ent_recs * sizeof(CombEnt);
  Blob blob;
  const size_t arec_off = blob.add<ApplyManyRec>(n_act), brec_off = blob.add<BoundsRec>(n_act), crec_off = blob.add<CombManyRec>(n_act);
  const size_t pool_off = blob.add<unsigned>(2 * ClassPool::words(n_act, 1, false) + ClassPool::words(n_act, NHOT, true) +
                                             ClassPool::words(n_act, NAPP, true));
  ManyUpload up;
  rc = many_begin(ws, se_bytes + den_bytes + ent_bytes, blob.bytes(), s, &up);
  if (rc) return rc;
  unsigned char* base = (unsigned char*)ws->buf;
  int* se_base = reinterpret_cast<int*>(base);
  float* den_base = reinterpret_cast<float*>(base + se_bytes);
  CombEnt* ent_base = reinterpret_cast<CombEnt*>(base + se_bytes + den_bytes);
  ApplyManyRec* arecs = section<ApplyManyRec>(up.host, arec_off);
  BoundsRec* brecs = section<BoundsRec>(up.host, brec_off);
  CombManyRec* crecs = section<CombManyRec>(up.host, crec_off);

  std::vector<unsigned> key_blocks(n_act), bin_blocks(n_act);
  {
    size_t se_at = 0, den_at = 0, ent_at = 0;
    for (size_t k = 0; k < n_act; ++k) {
      const tfra_apply_combined_desc& d = descs[act[k]];
      Table* t = reinterpret_cast<Table*>(d.table);
      const tfra_sparse_plan* pl = d.plan;
      const tfra_opt_params* p = d.opt;
      int* se = se_base + se_at;
      float* den = den_base + den_at;
      CombEnt* ent = ent_base + ent_at;
      se_at += (2 * d.n_rows + 63) / 64 * 64;
      den_at += (d.n_rows + 63) / 64 * 64;
      ent_at += (pl->n + 15) / 16 * 16;
      brecs[k] = BoundsRec{(const i64*)d.seg, se, pl->n, d.n_rows};
      crecs[k] = CombManyRec{(const i64*)d.seg, d.weights, se, den, ent, pl->n, d.n_rows, d.combiner};
      plan_grids(pl, &key_blocks[k], &bin_blocks[k]);
      key_blocks[k] = many_cap(key_blocks[k], app_n[app_of[k]]);
      bin_blocks[k] = many_cap(bin_blocks[k], hot_n[hot_of[k]]);
      // the view: under the lock, after the capacity preparation; ++use_gen: one use of the plan
      arecs[k] = ApplyManyRec{t->view_of(t->cur), OptP{p->kind, p->lr, p->beta1, p->beta2, p->eps, p->l1, p->l2, p->lr_power, p->d_lr},
                              ScoreP{t->opts.strategy, t->global_epoch, bounded[k]}, keys_of(pl), d.grad_out, pl->partial,
                              d.param_default_row, pl->out.hout, pl->binmap, pl->dflag, pl->any_deferred, ent, pl->dim,
                              t->opts.aux_init[0], t->opts.aux_init[1], ++pl->use_gen};
    }
  }
  // the pool: the entry kernels' two prefixes over all records, then the classes, which read the records through an index
  ClassPool pool{section<unsigned>(up.host, pool_off)};
  auto all = [](size_t) { return true; };
  const ManyClass ent_cls = pool.put(n_act, false, all, ent_blocks_of), den_cls = pool.put(n_act, false, all, den_blocks_of);
  ManyClass hot_cls[NHOT], app_cls[NAPP];
  for (int c = 0; c < NHOT; ++c)
    hot_cls[c] = pool.put(n_act, true, [&](size_t k) { return hot_of[k] == c; }, [&](size_t k) { return bin_blocks[k]; });
  for (int c = 0; c < NAPP; ++c)
    app_cls[c] = pool.put(n_act, true, [&](size_t k) { return app_of[k] == c; }, [&](size_t k) { return key_blocks[k]; });

  rc = many_send(up, s, "multi_apply_planned_combined: record upload", false);
  if (rc) return rc;
  if (hipMemsetAsync(se_base, 0, se_bytes, s) != hipSuccess)   // empty rows: start = end = 0
    return set_error(TFRA_ERR_HIP, "multi_apply_planned_combined: memset");
  uint32_t launches = 0;
  const unsigned* d_pool = section<const unsigned>(up.dev, pool_off);
  rc = comb_bounds_many(s, ent_cls.grid, section<const BoundsRec>(up.dev, brec_off), d_pool + ent_cls.at, (unsigned)n_act);
  if (rc) return rc;
  rc = comb_den_ent_many(s, den_cls.grid, ent_cls.grid, section<const CombManyRec>(up.dev, crec_off), d_pool + den_cls.at,
                         d_pool + ent_cls.at, (unsigned)n_act);
  if (rc) return rc;
  launches += 3;
  const ApplyManyRec* d_arecs = section<const ApplyManyRec>(up.dev, arec_off);
  for (int c = 0; c < NHOT; ++c) {
    const ManyClass& k = hot_cls[c];
    if (!k.n) continue;
    launch_hot_sums_many(s, c + 1, k.grid, d_arecs, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
    ++launches;
  }
  for (int c = 0; c < NAPP; ++c) {
    const ManyClass& k = app_cls[c];
    if (!k.n) continue;
    launch_apply_many(s, c % 3, c / 3, false, k.grid, d_arecs, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
    ++launches;
    if (app_evict[c]) {
      launch_apply_many(s, c % 3, c / 3, true, k.grid, d_arecs, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
      ++launches;
    }
  }
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "multi_apply_planned_combined: launch failed");
  for (size_t i : act) reinterpret_cast<Table*>(descs[i].table)->step_epoch();
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

// tfra_table_apply_sparse for more ids than a plan holds (2^18).  Equal ids must still meet in ONE update, whatever
// chunk they sit in:
//   1. per chunk of 2^18 ids: unique + per-key gradient sums (tfra_reduce_by_key) into one concatenated list — a key now
//      occurs at most once per chunk, so even the hottest id of a Zipf batch is a handful of entries;
//   2. the list fits a plan: one planned write-back sums a key's entries in chunk order and applies it;
//      else the list is split by key hash (tfra_partition, mode 2) into parts that fit — a key's entries stay together,
//      the parts are disjoint key sets — and each part is written back on its own.
// A slow path (host reads of the counts, scratch allocated per call); results are deterministic, the association of the
// sums is (within chunk) + (across chunks in order).
static int apply_sparse_big(Table* t, tfra_table_t* tp, tfra_sparse_plan* pl, const tfra_opt_params* p, size_t n, const int64_t* ids,
                            const float* grads, const float* param_default_row, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int dim = t->opts.dim;
  if (!t->big_ws) {
    tfra_workspace_t* w = nullptr;
    int rc = tfra_workspace_create(t->device, &w);
    if (rc) return rc;
    t->big_ws = w;
  }
  tfra_workspace_t* ws = reinterpret_cast<tfra_workspace_t*>(t->big_ws);
  i64 *keys_cat = nullptr, *d_cnt = nullptr, *keys_part = nullptr, *d_counts = nullptr;
  float *sums_cat = nullptr, *sums_part = nullptr;
  int* perm = nullptr;
  auto cleanup = [&](int rc) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(keys_cat); (void)hipFree(d_cnt); (void)hipFree(keys_part); (void)hipFree(d_counts); (void)hipFree(sums_cat);
    (void)hipFree(sums_part); (void)hipFree(perm);
    return rc;
  };
  auto oom = [&]() { return cleanup(set_error(TFRA_ERR_OOM, "apply_sparse: scratch for a batch of more than 2^18 ids")); };
  if (hipMalloc((void**)&keys_cat, n * sizeof(i64)) != hipSuccess || hipMalloc((void**)&sums_cat, n * (size_t)dim * sizeof(float)) != hipSuccess ||
      hipMalloc((void**)&d_cnt, sizeof(i64)) != hipSuccess)
    return oom();
  size_t T = 0;
  for (size_t off = 0; off < n; off += MAX_IDS) {
    const size_t m = std::min<size_t>(MAX_IDS, n - off);
    int rc = tfra_reduce_by_key(ws, m, ids + off, dim, grads + off * (size_t)dim, (int64_t*)keys_cat + T, sums_cat + T * (size_t)dim,
                                (int64_t*)d_cnt, stream);
    if (rc) return cleanup(rc);
    i64 c = 0;
    if (hipMemcpyAsync(&c, d_cnt, sizeof(i64), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return cleanup(set_error(TFRA_ERR_HIP, "apply_sparse: count read"));
    if (c < 0) return cleanup(set_error(TFRA_ERR_FULL, "apply_sparse: a de-duplication plan overflowed"));
    T += (size_t)c;
  }
  if (T <= MAX_IDS) {
    int rc = tfra_sparse_plan_build(pl, T, (const int64_t*)keys_cat, dim, stream);
    if (!rc) rc = apply_planned_impl(tp, p, pl, sums_cat, param_default_row, stream, nullptr, 0);
    return cleanup(rc);
  }
  if (hipMalloc((void**)&keys_part, T * sizeof(i64)) != hipSuccess || hipMalloc((void**)&perm, T * sizeof(int)) != hipSuccess ||
      hipMalloc((void**)&sums_part, T * (size_t)dim * sizeof(float)) != hipSuccess)
    return oom();
  for (size_t P = (T + (MAX_IDS / 2) - 1) / (MAX_IDS / 2); P <= 2048; P *= 2) {
    (void)hipFree(d_counts); d_counts = nullptr;
    if (hipMalloc((void**)&d_counts, P * sizeof(i64)) != hipSuccess) return oom();
    int rc = tfra_partition(ws, T, nullptr, (const int64_t*)keys_cat, (int)P, 2, (int64_t*)keys_part, perm, (int64_t*)d_counts, stream);
    if (rc) return cleanup(rc);
    std::vector<i64> counts(P);
    if (hipMemcpyAsync(counts.data(), d_counts, P * sizeof(i64), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return cleanup(set_error(TFRA_ERR_HIP, "apply_sparse: count read"));
    bool fits = true;
    for (i64 c : counts) fits = fits && (size_t)c <= MAX_IDS;
    if (!fits) continue;   // a part too large (skewed hash): more parts
    rc = tfra_gather_rows(T, (size_t)dim * sizeof(float), sums_cat, perm, sums_part, stream);
    if (rc) return cleanup(rc);
    size_t off = 0;
    // ONE logical write-back: the epoch / step counters of the EPOCH* strategies advance once, not once per part (the
    // reference counts one upsert per write-back, lookup_table_op_hkv.h:528-536).  (On a bounded table at max_capacity a
    // later part may still evict keys an earlier part of the same batch inserted.)
    t->epoch_hold = true;
    for (i64 c : counts) {
      if (c > 0) {
        rc = tfra_sparse_plan_build(pl, (size_t)c, (const int64_t*)keys_part + off, dim, stream);
        if (!rc) rc = apply_planned_impl(tp, p, pl, sums_part + off * (size_t)dim, param_default_row, stream, nullptr, 0);
        if (rc) { t->epoch_hold = false; return cleanup(rc); }
      }
      off += (size_t)c;
    }
    t->epoch_hold = false;
    t->step_epoch();
    return cleanup(TFRA_OK);
  }
  return cleanup(set_error(TFRA_ERR_UNSUPPORTED, "apply_sparse: could not split the batch into parts of 2^18 ids"));
}

extern "C" int tfra_table_apply_sparse(tfra_table_t* tp, const tfra_opt_params* p, size_t n, const int64_t* ids,
                                       const float* grads, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t || !p) return set_error(TFRA_ERR_INVALID, "apply_sparse: null argument");
  if (n == 0) return TFRA_OK;
  if (!ids || !grads || !param_default_row) return set_error(TFRA_ERR_INVALID, "apply_sparse: null buffer");
  const int dt = t->opts.value_dtype;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return set_error(TFRA_ERR_UNSUPPORTED, "apply_sparse: value_dtype must be float32, float16 or bfloat16 (gradients and the default row are float32)");
  const int dim = t->opts.dim;
  if (dim % 4 != 0 || dim > 64 * MAXCH || (((uintptr_t)grads | (uintptr_t)param_default_row) & 15))
    return set_error(TFRA_ERR_UNSUPPORTED, "apply_sparse: needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers "
                                           "(use tfra_unique + tfra_segment_sum + tfra_table_apply_optimizer otherwise)");
  tfra_sparse_plan* pl;
  std::lock_guard<std::mutex> lock(t->mu);
  int rc = t->enter((hipStream_t)stream);   // orders the rebuild of the table's own plan behind its previous use
  if (rc) return rc;
  rc = own_plan(t, &pl);
  if (rc) return rc;
  if (n > MAX_IDS) return apply_sparse_big(t, tp, pl, p, n, ids, grads, param_default_row, stream);
  rc = tfra_sparse_plan_build(pl, n, ids, dim, stream);
  if (rc) return rc;
  return apply_planned_impl(tp, p, pl, grads, param_default_row, stream, nullptr, 0);
}

// unique + unsorted_segment_sum in one call = the plan + the hot sums + a gather (the reduction half of
// tfra_table_apply_sparse with the same summation tree, so routing the sums elsewhere — multi-GPU gradient
// alltoall — and applying them there gives the same bits as applying them here).
extern "C" int tfra_reduce_by_key(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const float* grads,
                                  int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !d_count) return set_error(TFRA_ERR_INVALID, "reduce_by_key: null argument");
  if (on_device(ws->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "reduce_by_key: hipSetDevice");
  if (n == 0) {
    if (hipMemsetAsync(d_count, 0, sizeof(int64_t), s) != hipSuccess) return set_error(TFRA_ERR_HIP, "reduce_by_key: memset");
    return TFRA_OK;
  }
  if (!ids || !grads || !keys_out || !rows_out) return set_error(TFRA_ERR_INVALID, "reduce_by_key: null buffer");
  if (dim <= 0 || dim % 4 != 0 || dim > 64 * MAXCH || (((uintptr_t)grads | (uintptr_t)rows_out) & 15))
    return set_error(TFRA_ERR_UNSUPPORTED, "reduce_by_key: needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers "
                                           "(use tfra_unique + tfra_segment_sum otherwise)");
  if (n > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, "reduce_by_key: at most 2^18 ids per call");
  if (!ws->plan) {
    tfra_sparse_plan* np_ = nullptr;
    int rc = tfra_sparse_plan_create(ws->device, &np_);
    if (rc) return rc;
    ws->plan = np_;
  }
  tfra_sparse_plan* pl = reinterpret_cast<tfra_sparse_plan*>(ws->plan);
  int rc = tfra_sparse_plan_build(pl, n, ids, dim, stream);
  if (rc) return rc;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  launch_hot_sums(s, pl, grads, bin_blocks, nullptr, 0);   // (pl->dim == dim)
  gather_csr_kernel<<<key_blocks, 256, 0, s>>>(dim, grads, pl->partial, keys_of(pl), (i64*)keys_out, rows_out, (i64*)d_count, nullptr);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "reduce_by_key: launch failed");
  return TFRA_OK;
}

// The per-key gradient sums of a batch whose plan was built ahead (tfra_sparse_plan_build with the table's dim, on any
// stream): hot sums + gather, the reduction half of tfra_reduce_by_key with the same summation tree, written to
// rows_out[dest[p]] where p is a position of the key.  dest [n] int32: the caller's map from batch positions to output
// rows, the same for every position of a key (e.g. position -> owner-major index of the multi-GPU gradient route, which
// is known from the ids alone).  rows_out must have a row for every value in dest; rows no key maps to are not written.
extern "C" int tfra_plan_reduce_to(const tfra_sparse_plan_t* pl, const float* grads, const int32_t* dest, float* rows_out,
                                   tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!pl) return set_error(TFRA_ERR_INVALID, "plan_reduce_to: null plan");
  if (pl->kind == 1) return set_error(TFRA_ERR_UNSUPPORTED, "plan_reduce_to: needs a plan built with the table's dim");
  if (pl->n == 0) return TFRA_OK;
  if (!grads || !dest || !rows_out) return set_error(TFRA_ERR_INVALID, "plan_reduce_to: null buffer");
  const int dim = pl->dim;
  if (dim <= 0 || (((uintptr_t)grads | (uintptr_t)rows_out) & 15))
    return set_error(TFRA_ERR_INVALID, "plan_reduce_to: the plan must have been built with the rows' dim; buffers 16-B aligned");
  if (on_device(pl->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "plan_reduce_to: hipSetDevice");
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  launch_hot_sums(s, pl, grads, bin_blocks, nullptr, 0);
  gather_csr_kernel<<<key_blocks, 256, 0, s>>>(dim, grads, pl->partial, keys_of(pl), nullptr, rows_out, nullptr, (const int*)dest);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "plan_reduce_to: launch failed");
  return TFRA_OK;
}

// ---------------------------------------------------------------------------------------------
// One training step driven from C on two streams (no Python between the launches, no graph).
//   main : lookup(ids_cur) -> write-back of batch cur (hot sums + fused update, or assign)      (plan_cur)
//   side : build plan_next from ids_next, free-running
// Cross-queue events cost ~5 us (stream wait) / ~7 us (record) each between two kernels of the main stream,
// so the two streams are ordered through two host-visible counters in pinned memory instead, and the host
// only falls back to a sync when a counter lags:
//   * table progress: written by the first block of the write-back of step s  =>  every earlier step is done.
//     plan_next's buffers were last read by step plan_next->last_used_step; the build is enqueued once the
//     progress has passed it (with >= 3 plans in rotation that is always the case unless the host is far
//     ahead of the GPU, in which case it waits here instead of in a queue);
//   * plan built: generation + counts written by the build's last kernel.  If they already show plan_cur's
//     generation the write-back is enqueued without any wait packet and with exact grids; otherwise — the host
//     got ahead of the side stream — the host waits for the side stream.
static int step_prefetch_impl(tfra_table_t* tp, const tfra_opt_params* p, tfra_sparse_plan_t* plan_cur,
                              const int64_t* ids_cur, void* rows_out, const void* find_default, const void* grads_or_values,
                              const float* param_default_row, const uint64_t* scores, tfra_sparse_plan_t* plan_next,
                              const int64_t* ids_next, size_t n_next, tfra_stream_t main_stream, tfra_stream_t side_stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t || !plan_cur) return set_error(TFRA_ERR_INVALID, "step_prefetch: null argument");
  hipStream_t ms = (hipStream_t)main_stream, ss = (hipStream_t)side_stream;
  if (ms == ss && plan_next) return set_error(TFRA_ERR_INVALID, "step_prefetch: needs two different streams");
  if (plan_next == plan_cur) return set_error(TFRA_ERR_INVALID, "step_prefetch: plan_next must differ from plan_cur");
  std::lock_guard<std::mutex> step_lock(t->step_mu);   // one driver call at a time per table
  int rc = TFRA_OK;
  if (!t->progress_host) {
    if (hipHostMalloc((void**)&t->progress_host, 64, hipHostMallocDefault) != hipSuccess) { t->progress_host = nullptr; return set_error(TFRA_ERR_OOM, "step_prefetch: hipHostMalloc"); }
    t->progress_host[0] = 0; t->progress_host[1] = 0;
  }
  const unsigned step = ++t->step_gen;
  if (plan_next) {
    if (!plan_next->host_counts) {
      if (hipHostMalloc((void**)&plan_next->host_counts, 64, hipHostMallocDefault) != hipSuccess) { plan_next->host_counts = nullptr; return set_error(TFRA_ERR_OOM, "step_prefetch: hipHostMalloc"); }
      for (unsigned i = 0; i < HC_SHIFT + PC_PUBLISHED; ++i) plan_next->host_counts[i] = 0;
    }
    if (plan_next->last_used_step) {  // the write-back that read plan_next's buffers must be over
      const unsigned need = plan_next->last_used_step + 1;
      volatile unsigned* prog = t->progress_host;
      bool ok = false;
      for (int it = 0; it < 200000 && !ok; ++it) ok = (int)(*prog - need) >= 0;   // ~ a few ms at most
      if (!ok && hipStreamSynchronize(ms) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_prefetch: sync");
    }
  }
  if (plan_cur->n && rows_out) {
    rc = tfra_table_find(tp, plan_cur->n, ids_cur, rows_out, nullptr, find_default, 0, main_stream);
    if (rc) return rc;
  }
  if (plan_next) {
    if (!p) plan_next->skip_counts_once = !(t->opts.strategy == TFRA_EVICT_LFU && !scores);   // (the next step's call passes scores or not like this one)
    rc = tfra_sparse_plan_build(plan_next, n_next, ids_next, p ? t->opts.dim : 0, side_stream);
    if (rc) return rc;
    if (!plan_next->built_ev && hipEventCreateWithFlags(&plan_next->built_ev, hipEventDisableTiming) != hipSuccess) {
      plan_next->built_ev = nullptr;
      return set_error(TFRA_ERR_HIP, "step_prefetch: event");
    }
    if (hipEventRecord(plan_next->built_ev, ss) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_prefetch: event record");
    plan_next->ev_recorded = true;   // built on the side stream: the join below applies
  }
  if (plan_cur->ev_recorded) {  // built on the side stream by an earlier call
    // complete = every block of the build has ended and its stores are in memory (the pinned counts alone do not say that)
    if (hipEventQuery(plan_cur->built_ev) != hipSuccess && hipEventSynchronize(plan_cur->built_ev) != hipSuccess)   // the wait: rare
      return set_error(TFRA_ERR_HIP, "step_prefetch: join");
    plan_cur->ev_recorded = false;
  }
  plan_cur->last_used_step = step;
  if (plan_cur->n == 0) return TFRA_OK;   // no kernel publishes this step: a later slot check falls back to a sync
  std::lock_guard<std::mutex> lock(t->mu);
  if (p) return apply_planned_impl(tp, p, plan_cur, (const float*)grads_or_values, param_default_row, main_stream, t->progress_host, step);
  return upsert_planned_impl(tp, plan_cur, grads_or_values, scores, main_stream, t->progress_host, step);
}

extern "C" int tfra_table_step_prefetch(tfra_table_t* tp, const tfra_opt_params* p, tfra_sparse_plan_t* plan_cur,
                                        const int64_t* ids_cur, void* rows_out, const void* find_default,
                                        const float* grads, const float* param_default_row,
                                        tfra_sparse_plan_t* plan_next, const int64_t* ids_next, size_t n_next,
                                        tfra_stream_t main_stream, tfra_stream_t side_stream) {
  if (!p) return set_error(TFRA_ERR_INVALID, "step_prefetch: null optimizer parameters");
  return step_prefetch_impl(tp, p, plan_cur, ids_cur, rows_out, find_default, grads, param_default_row, nullptr, plan_next, ids_next,
                            n_next, main_stream, side_stream);
}

extern "C" int tfra_table_step_prefetch_assign(tfra_table_t* tp, tfra_sparse_plan_t* plan_cur, const int64_t* ids_cur,
                                               void* rows_out, const void* find_default, const void* values,
                                               const uint64_t* scores, tfra_sparse_plan_t* plan_next,
                                               const int64_t* ids_next, size_t n_next, tfra_stream_t main_stream,
                                               tfra_stream_t side_stream) {
  return step_prefetch_impl(tp, nullptr, plan_cur, ids_cur, rows_out, find_default, values, nullptr, scores, plan_next, ids_next,
                            n_next, main_stream, side_stream);
}
