// Device side of the planned write-back for WIDE rows (tfra_apply_wide.hip): the sums of the plan's bins and the fused
// per-key update for 256 < dim <= 1024.  The twins (tfra_apply_device.h) give a key or an item to a 16-lane group, a lane owning
// four columns of every 64: for a row of 2 - 4 KB that is 4 - 16 trips of 256-byte accesses per group and a record's words held
// four times per wave.  Here the WAVE owns one row at a time — lane l owns columns k * 256 + 4 * l, k < ceil(dim / 256): an access
// is 1 KB contiguous on float rows, 512 B on half rows — and the 16-lane groups keep only what is per key: the probe, the claim, the
// record, the score.
// The plan's summation tree is kept exactly: an item's 16 entries are added in entry order from zero, a run's following items to
// its first item in item order, a key's source rows or partial rows in list order from zero.  Every addition is per column and the
// unit is built under -ffp-contract=off, so columns [a, b) of a wide result are bit for bit what the twins compute for those columns.
// Anonymous namespace: see tfra_plan_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_apply_device.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_optim_device.h"
#include "tfra_plan_device.h"
#include "tfra_reduce_device.h"

namespace {

constexpr int WIDE_COLS = 256;   // columns the wave covers per chunk: 64 lanes x 4

// a value of lane `src` (wave-uniform) in a scalar register
__device__ __forceinline__ unsigned wave_word(unsigned x, int src) { return (unsigned)__builtin_amdgcn_readfirstlane(__shfl((int)x, src)); }
__device__ __forceinline__ float wave_float(float x, int src) { return __uint_as_float(wave_word(__float_as_uint(x), src)); }

__device__ __forceinline__ void add4(float4& acc, const float4& x) { acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w; }

// ---------------------------------------------------------------------------------------------
// the sums: one 512-thread block per bin of 32 items.  A wave loads the entry words of ITS four items as the twin does (lane `sub`
// of group g holds entry `sub` of item g), then walks the four items one after the other with all 64 lanes on a chunk of 256
// columns: an item's 16 rows in flight, each 1 KB contiguous, added in entry order from zero.  The run combine goes through
// s_sum[32][256], chunk by chunk, under the twin's s_kind protocol and barriers; the wave of a run's first item adds the following
// items' sums in item order and writes the partial row.
// CS = CombRows: the gradient of entry e is comb_grad4(grad_out[row_e], den_e, w_e); each lane reads the record of its own entry,
// the wave shares it by shuffles.  grad_out is addressed with 32-bit element offsets (n_rows * dim < 2^32: checked on the host).
template <class... CS>
__device__ __forceinline__ void hot_sums_wide_body(const float* __restrict__ grads, int dim, const unsigned* __restrict__ hent,
                                                   const unsigned* __restrict__ hout, const unsigned* __restrict__ binmap,
                                                   const unsigned* __restrict__ d_counts, float* __restrict__ partial, const CS... cs) {
  constexpr bool COMB = (false || ... || std::is_same<CS, CombRows>::value);
  constexpr int NG = NTA / 16;
  __shared__ float s_sum[NG][WIDE_COLS];
  __shared__ unsigned char s_kind[NG + 1];   // 0 = item continues the run of the item before, 1 = first item of a run, 2 = empty item
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, g = threadIdx.x >> 4;
  const int g0 = (threadIdx.x >> 6) << 2;    // the wave's first item
  const unsigned nbins = d_counts[PC_BINS];
  for (unsigned ib = blockIdx.x; ib < nbins; ib += gridDim.x) {
    const unsigned bin = binmap[ib];
    const unsigned e = hent[(size_t)bin * SEG + threadIdx.x];
    const unsigned e0 = (unsigned)__shfl((int)e, gshift);
    const bool empty = (e0 & E_SKIP) != 0, first = (e0 & E_HEAD) != 0;
    const unsigned out_row = (first && !empty && sub == 0) ? hout[(size_t)bin * 32 + g] : 0u;
    const u64 live_all = __ballot(!(e & E_SKIP));   // entries that exist, of the wave's four items
    if (sub == 0) s_kind[g] = empty ? 2 : (first ? 1 : 0);
    if (threadIdx.x == 0) s_kind[NG] = 1;
    // this lane's entry: the element offset of its gradient row (padding: the item's first row, never added)
    unsigned my_row;
    float cden = 0.f, cw = 0.f;
    if constexpr (COMB) {
      const CombEnt ce = comb_ent(cs...)[((e & E_SKIP) ? e0 : e) & E_POS];
      my_row = ce.row * (unsigned)dim;
      cden = ce.den;
      cw = ce.w;
    } else {
      my_row = (((e & E_SKIP) ? e0 : e) & E_POS) * (unsigned)dim;
    }
    for (int c0 = 0; c0 < dim; c0 += WIDE_COLS) {
      const int col = c0 + lane * 4;
      const int cc = col < dim ? col : 0;
      if (c0) __syncthreads();   // the owners of the previous chunk have read s_sum
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {   // (one item at a time: 16 rows in flight and one accumulator, ~100 registers => two blocks per CU)
        const unsigned live = (unsigned)(live_all >> (q * 16)) & 0xffffu;
        if (!(live & 1u)) continue;   // an empty item (wave-uniform): nothing reads its sum
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = *reinterpret_cast<const float4*>(grads + wave_word(my_row, q * 16 + j) + cc);   // 16 rows in flight
        keep_live(x[0], x[1], x[2], x[3]); keep_live(x[4], x[5], x[6], x[7]);
        keep_live(x[8], x[9], x[10], x[11]); keep_live(x[12], x[13], x[14], x[15]);
        if constexpr (COMB) {
#pragma unroll
          for (int j = 0; j < 16; ++j) x[j] = comb_grad4(x[j], wave_float(cden, q * 16 + j), wave_float(cw, q * 16 + j));
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if ((live >> j) & 1u) add4(acc, x[j]);
        *reinterpret_cast<float4*>(&s_sum[g0 + q][lane * 4]) = acc;
      }
      __syncthreads();
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        const unsigned eq = wave_word(e0, q * 16);
        if ((eq & E_SKIP) || !(eq & E_HEAD)) continue;   // wave-uniform
        float4 a = *reinterpret_cast<const float4*>(&s_sum[g0 + q][lane * 4]);   // the run's first item: this wave's own sum
        for (int g2 = g0 + q + 1; s_kind[g2] == 0; ++g2) add4(a, *reinterpret_cast<const float4*>(&s_sum[g2][lane * 4]));
        const unsigned orow = wave_word(out_row, q * 16);
        if (col < dim) *reinterpret_cast<float4*>(partial + (size_t)orow * dim + col) = a;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// NB source rows of ONE key's sum in flight, the whole wave on a chunk: rows j0 .. j0 + NB - 1 of its list (clamped to the last;
// loads issued together, adds in list order).  src = the first lane of the key's group, whose lanes hold the record's words (lane i
// word i; COMB, a key with few occurrences: lanes 4.. hold grad_out rows and cden / cw their entries' denominator and weight).
template <int NB, bool COMB>
__device__ __forceinline__ void add_rows_wide(float4& acc, const float* __restrict__ grads, const float* __restrict__ partial, bool hot,
                                              unsigned w, unsigned first, unsigned nsrc, unsigned j0, int dim, int c, int src,
                                              float cden, float cw) {
  float4 x[NB];
  int from[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const unsigned jj = min(j0 + (unsigned)j, nsrc - 1);
    from[j] = src + 4 + (int)min(jj, 7u);
    const float* q = hot ? partial + (size_t)(first + jj) * dim : grads + (size_t)wave_word(w, from[j]) * dim;
    x[j] = *reinterpret_cast<const float4*>(q + c);
  }
  if (NB == 4) keep_live(x[0], x[1], x[2], x[3]);
  if (COMB && !hot) {
#pragma unroll
    for (int j = 0; j < NB; ++j) x[j] = comb_grad4(x[j], wave_float(cden, from[j]), wave_float(cw, from[j]));
  }
#pragma unroll
  for (int j = 0; j < NB; ++j)
    if (j0 + (unsigned)j < nsrc) add4(acc, x[j]);
}

// the whole sum of a key: 1 / 2 / 4 rows in flight by the list's length (wave-uniform: one key at a time)
template <bool COMB>
__device__ __forceinline__ float4 sum_rows_wide(const float* __restrict__ grads, const float* __restrict__ partial, bool hot, unsigned w,
                                                unsigned first, unsigned nsrc, int dim, int c, int src, float cden, float cw) {
  float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
  if (nsrc <= 1) add_rows_wide<1, COMB>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, src, cden, cw);
  else if (nsrc <= 2) add_rows_wide<2, COMB>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, src, cden, cw);
  else
    for (unsigned j0 = 0; j0 < nsrc; j0 += 4) add_rows_wide<4, COMB>(gg, grads, partial, hot, w, first, nsrc, j0, dim, c, src, cden, cw);
  return gg;
}

// ---------------------------------------------------------------------------------------------
// the update: 256 threads, grid-stride over the key list (hot keys first), four consecutive keys per wave and trip.
//   stage A, per 16-lane group (the twin's code and helpers, one key per group): the first probe line and the record in flight
//            together, COMB's swap of batch positions for grad_out rows, locate_or_claim_from — PHASE2: evict_and_lock;
//   stage B, the whole wave, key after key: everything per key comes by shuffle from its group into scalar registers; per chunk of
//            256 columns the loads of the parameter, the rule's slots and the default row are issued together with the gradient
//            rows; adds in list order, apply_one, one rounding, write-through stores;
//   stage C, per group again: the twin's tail (score, publish_key under PHASE2).
// A slot locked in stage A (PHASE2) is published in stage C of the same trip: no wave waits on another.
// ST half: 8-byte granules per lane and field, up-cast, updated in fp32, rounded once (to_stored4); a new row starts from the FLOAT
// default row and aux_init, as in the twin.
template <int KIND, bool PHASE2, int ST, class... CS>
__device__ __forceinline__ void apply_csr_wide_body(const TableView& v, OptP o, int dim, const float* __restrict__ grads,
                                                    const float* __restrict__ partial, const CsrKeys& ks,
                                                    const float* __restrict__ default_row, float aux0, float aux1, const ScoreP& sp,
                                                    uint8_t* __restrict__ dflag, unsigned* any_deferred, unsigned use_gen, const CS... cs) {
  constexpr bool COMB = (false || ... || std::is_same<CS, CombRows>::value);
  if (PHASE2 && *any_deferred != use_gen) return;   // phase 1 of this use deferred nothing
  constexpr int S = NSlots<KIND>::v;
  typedef typename Stored<ST>::T V;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  const unsigned ngroups = (gridDim.x * blockDim.x) >> 4;
  int fresh = 0, failed = 0;
  if (o.d_lr) o.lr = *o.d_lr;
  if (!PHASE2 && blockIdx.x == 0 && threadIdx.x == 0 && ks.d_counts[PC_OVERFLOW]) atomicAdd(v.err_count, ks.d_counts[PC_OVERFLOW]);  // plan overflow
  for (unsigned wbase = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2; wbase < total; wbase += ngroups) {
    // ---- stage A: one key per group
    const unsigned it_raw = wbase + (unsigned)(lane >> 4);
    const bool active = it_raw < total;
    const unsigned g = active ? it_raw : total - 1;
    if (PHASE2 && !__builtin_amdgcn_readfirstlane((int)(__ballot(active && dflag[g]) != 0))) continue;   // nothing deferred in this wave
    const i64 key = ks.dkeys[g];
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    i64 k0 = 0;
    if (!PHASE2) k0 = load_key_coherent(key_line(v, b0) + sub);
    bool hot;
    const unsigned w = load_record(ks, g, sub, hot);
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    unsigned wsrc = w;
    float cden = 0.f, cw = 0.f;
    if constexpr (COMB) {
      if (!hot && sub >= 4 && (unsigned)(sub - 4) < cnt) {
        const CombEnt ce = comb_ent(cs...)[w];
        wsrc = ce.row; cden = ce.den; cw = ce.w;
      }
    }
    i64 row = -1;
    bool is_new = false, claimed_empty = false;
    u64 word = 0;
    if (active && !(PHASE2 && !dflag[g])) {
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
      if (row < 0) failed += (sub == 0 && (PHASE2 ? row == -3 : row != NEED_EVICT));
      else fresh += ((PHASE2 ? claimed_empty : is_new) && sub == 0);
    }
    const bool go = row >= 0;
    unsigned char* const pr_g = go ? row_ptr(v, row) : nullptr;
    const unsigned pr_lo = (unsigned)(uintptr_t)pr_g, pr_hi = (unsigned)((uintptr_t)pr_g >> 32);
    // ---- stage B: the wave, key after key
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const int src = q * 16;
      if (!wave_word((unsigned)go, src)) continue;   // inactive, not deferred or failed: skipped by the whole wave
      const bool q_new = wave_word((unsigned)is_new, src) != 0, q_hot = wave_word((unsigned)hot, src) != 0;
      const unsigned first = wave_word(w, src + 3);
      const unsigned nsrc = q_hot ? wave_word(w, src + 4) : wave_word(w, src + 2);
      float* const pr = reinterpret_cast<float*>(((uintptr_t)wave_word(pr_hi, src) << 32) | wave_word(pr_lo, src));
      V* const sr = reinterpret_cast<V*>(pr);   // (half fields of dim * 2 bytes: 8-byte aligned at every c % 4 == 0)
      for (int c0 = 0; c0 < dim; c0 += WIDE_COLS) {
        const bool col = c0 + lane * 4 < dim;
        const int c = col ? c0 + lane * 4 : 0;
        float4 p, s1, s2;
        // all loads unconditional and issued together (a brand-new row reads its own not yet initialised bytes and discards them)
        if constexpr (ST != TFRA_F32) {
          uint2 rp = *reinterpret_cast<const uint2*>(sr + c);
          uint2 r1 = *reinterpret_cast<const uint2*>(sr + (S >= 1 ? dim : 0) + c);
          uint2 r2 = *reinterpret_cast<const uint2*>(sr + (S >= 2 ? 2 * dim : 0) + c);
          const float4 dflt = *reinterpret_cast<const float4*>(default_row + c);
          const float4 gg = sum_rows_wide<COMB>(grads, partial, q_hot, COMB ? wsrc : w, first, nsrc, dim, c, src, cden, cw);
          uint2 dummy = rp;
          keep_live(dummy, rp, r1, r2);
          p = q_new ? dflt : load_stored4<ST>(rp);
          s1 = (q_new || S < 1) ? make_float4(aux0, aux0, aux0, aux0) : load_stored4<ST>(r1);
          s2 = (q_new || S < 2) ? make_float4(aux1, aux1, aux1, aux1) : load_stored4<ST>(r2);
          apply_one<KIND>(o, gg.x, p.x, s1.x, s2.x);
          apply_one<KIND>(o, gg.y, p.y, s1.y, s2.y);
          apply_one<KIND>(o, gg.z, p.z, s1.z, s2.z);
          apply_one<KIND>(o, gg.w, p.w, s1.w, s2.w);
          if (col) {   // write-through, one rounding per element (PHASE2: in memory before publish_key)
            store_wt8(sr + c, to_stored4<ST>(p));
            if (S >= 1) store_wt8(sr + dim + c, to_stored4<ST>(s1));
            if (S >= 2) store_wt8(sr + 2 * dim + c, to_stored4<ST>(s2));
          }
        } else {
          p = *reinterpret_cast<const float4*>((q_new ? default_row : pr) + c);
          s1 = *reinterpret_cast<const float4*>(pr + (S >= 1 ? dim : 0) + c);
          s2 = *reinterpret_cast<const float4*>(pr + (S >= 2 ? 2 * dim : 0) + c);
          const float4 gg = sum_rows_wide<COMB>(grads, partial, q_hot, COMB ? wsrc : w, first, nsrc, dim, c, src, cden, cw);
          float4 dummy = p;
          keep_live(dummy, p, s1, s2);
          if (q_new || S < 1) s1 = make_float4(aux0, aux0, aux0, aux0);
          if (q_new || S < 2) s2 = make_float4(aux1, aux1, aux1, aux1);
          apply_one<KIND>(o, gg.x, p.x, s1.x, s2.x);
          apply_one<KIND>(o, gg.y, p.y, s1.y, s2.y);
          apply_one<KIND>(o, gg.z, p.z, s1.z, s2.z);
          apply_one<KIND>(o, gg.w, p.w, s1.w, s2.w);
          if (col) {   // write-through: the rows leave L2 during the kernel, not at the boundary to the next one
            store_wt16(pr + c, *reinterpret_cast<uint4*>(&p));
            if (S >= 1) store_wt16(pr + dim + c, *reinterpret_cast<uint4*>(&s1));
            if (S >= 2) store_wt16(pr + 2 * dim + c, *reinterpret_cast<uint4*>(&s2));
          }
        }
      }
      // aux fields the optimizer does not own (table created with more slots than it uses): aux_init, as the twin fills them
      if (q_new && (int)v.n_fields - 1 > S) {
        for (int f = S + 1; f < (int)v.n_fields; ++f) {
          const float a = f == 1 ? aux0 : aux1;
          float4 a4 = make_float4(a, a, a, a);
          for (int c = lane * 4; c < dim; c += WIDE_COLS) {
            if constexpr (ST != TFRA_F32) store_wt8(sr + f * dim + c, to_stored4<ST>(a4));
            else store_wt16(pr + f * dim + c, *reinterpret_cast<uint4*>(&a4));
          }
        }
      }
    }
    // ---- stage C: per group, the twin's tail
    if (go) {
      if (PHASE2) {
        if (sub == 0) store_wt8(score_word(v, word), 0);  // the slot starts a new life
        update_score<true>(v, row, true, sp.strategy, 1, sp.epoch, sub);
        publish_key(v, word, key, sub);
      } else {
        update_score(v, row, is_new, sp.strategy, 1, sp.epoch, sub);  // one write-back = one upsert
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { fresh += __shfl_xor(fresh, off); failed += __shfl_xor(failed, off); }
  if (lane == 0) {
    if (fresh) size_add(v, (blockIdx.x * blockDim.x + threadIdx.x) >> 6, fresh);
    if (failed) atomicAdd(v.err_count, (unsigned)failed);
  }
}

}  // namespace
