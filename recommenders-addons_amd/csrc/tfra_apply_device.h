// Device side of the GRADIENT HALF of a planned write-back, for every unit that compiles it: the body of the hot sums (hot_sums_body)
// and the body of the fused per-key update (apply_csr_body, over add_rows / sum_rows) — each ONE function, called by the
// single-table kernels (tfra_apply.hip) and by the grouped ones (tfra_apply_many.hip) — and the grouped launches' record
// (ApplyManyRec).  Anonymous namespace: see tfra_plan_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_optim_device.h"
#include "tfra_plan_device.h"
#include "tfra_reduce_device.h"

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
  auto take = [&](const auto& x) { if constexpr (std::is_same<std::decay_t<decltype(x)>, CombRows>::value) p = x.ent; };
  (take(cs), ...);   // (the pack of the update kernels may also hold the rounding's StochP)
  return p;
}

// CS = GradHalf (the *_typed write-backs and tfra_reduce_by_key_typed): the [n, dim] gradient matrix is float16 or bfloat16 and is
// read where the float one is read — a lane's four elements are ONE 8-byte load (the group's 16 lanes = one 128-byte line per 64
// columns), up-cast exactly and multiplied by the scale (one fp32 multiplication, rounded on its own: -ffp-contract=off) before
// any add, so everything behind the load sees the float matrix G32[e] = f32(g[e]) * s of the untyped call.  ONE pack type for both
// formats: is_bf16 is wave-uniform (a kernel argument), the conversion a shift or v_cvt_f32_f16 chosen by it.  *d_scale is a scalar
// load, once per wave (nullptr: 1.0f — x * 1.0f is exact, no second variant).  The `grads` argument of the kernels is unused then.
// Without one in the pack the kernels compile the code they always did (if constexpr).
struct GradHalf { const void* g; const float* d_scale; int is_bf16; };
struct GradHalfSrc { const unsigned short* g; float s; int is_bf16; };   // in the kernel: the scale already read
template <class... CS> struct HasGradHalf { static constexpr bool v = (false || ... || std::is_same<CS, GradHalf>::value); };
template <class... CS>
__device__ __forceinline__ GradHalfSrc grad_half_in(const CS&... cs) {
  GradHalfSrc r{nullptr, 1.f, 0};
  auto take = [&](const auto& x) {
    if constexpr (std::is_same<std::decay_t<decltype(x)>, GradHalf>::value) {
      r.g = reinterpret_cast<const unsigned short*>(x.g);
      r.s = x.d_scale ? *x.d_scale : 1.f;
      r.is_bf16 = x.is_bf16;
    }
  };
  (take(cs), ...);
  return r;
}
// acc += the rows of G32 that N granules of four stored gradient elements hold, in order, those that `take(j)` names: each is up-cast
// and scaled when its turn comes (never N float rows held at once).  The format's branch is wave-uniform and outside the loop.
template <int ST>
__device__ __forceinline__ void grad_half_add1(float4& acc, const uint2& r, float s) {
  float4 x = load_stored4<ST>(r);
  x.x *= s; x.y *= s; x.z *= s; x.w *= s;
  acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
}
template <int N, class Take>
__device__ __forceinline__ void grad_half_add(float4& acc, const uint2 (&r)[N], const GradHalfSrc& gh, Take&& take) {
  if (gh.is_bf16) {
#pragma unroll
    for (int j = 0; j < N; ++j) if (take(j)) grad_half_add1<TFRA_BF16>(acc, r[j], gh.s);
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) if (take(j)) grad_half_add1<TFRA_F16>(acc, r[j], gh.s);
  }
}

// The same over grad_out rows of a combined write-back (CombRows and GradHalf in one pack): granule j becomes a row of
// GO32 = f32(g) * s, THEN the entry's gradient comb_grad4(GO32 row, den, w) — ((f32(g) * s) / den) * w, each step rounded on its own —
// and is added where the float COMB arm adds it.  ent(j, den, w) shuffles entry j's denominator and weight: every lane calls it.
// ONE loop with the format selected per granule (is_bf16 is wave-uniform), not grad_half_add's two loops under a branch: with the
// combiner's divisions in it the doubled loop cost the update kernels 11 registers, and 18 of them a waves-per-SIMD class.
template <int N, class Take, class Ent>
__device__ __forceinline__ void grad_half_add_comb(float4& acc, const uint2 (&r)[N], const GradHalfSrc& gh, Take&& take, Ent&& ent) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float den, w;
    ent(j, den, w);
    float4 x = gh.is_bf16 ? load_stored4<TFRA_BF16>(r[j]) : load_stored4<TFRA_F16>(r[j]);
    x.x *= gh.s; x.y *= gh.s; x.z *= gh.s; x.w *= gh.s;
    x = comb_grad4(x, den, w);
    if (take(j)) { acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w; }
  }
}

// The body is one function with two callers — hot_sums_kernel (one plan per launch) and hot_sums_many_kernel (a list of plans per
// launch) — so that both compile the same expressions: blk = this block's index among the nblk blocks that work on THIS plan.
template <int NCH, class... CS>
__device__ __forceinline__ void hot_sums_body(const float* __restrict__ grads, int dim,
                                              const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                              const unsigned* __restrict__ binmap,
                                              const unsigned* __restrict__ d_counts, float* __restrict__ partial,
                                              unsigned* progress, unsigned progress_val, unsigned blk, unsigned nblk, const CS... cs) {
  constexpr bool COMB = (false || ... || std::is_same<CS, CombRows>::value);
  constexpr bool GH = HasGradHalf<CS...>::v;
  constexpr int NG = NTA / 16;
  const GradHalfSrc gh = grad_half_in(cs...);
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
    unsigned rows[16];   // element offset of each row (< 2^18 * 256; COMB and GH: < 2^32, checked on the host)
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
        if constexpr (GH) {
          uint2 r[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = *reinterpret_cast<const uint2*>(gh.g + rows[h * 8 + j] + cc);
          keep_live(r[0], r[1], r[2], r[3]); keep_live(r[4], r[5], r[6], r[7]);
          if constexpr (COMB)
            grad_half_add_comb(acc, r, gh, [&](int j) { return ((live >> (h * 8 + j)) & 1u) != 0; },
                               [&](int j, float& den, float& w) { den = __shfl(cden, gshift + h * 8 + j); w = __shfl(cw, gshift + h * 8 + j); });
          else
          grad_half_add(acc, r, gh, [&](int j) { return ((live >> (h * 8 + j)) & 1u) != 0; });
        } else {
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
      }
      } else if constexpr (GH) {
      uint2 r[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) r[j] = *reinterpret_cast<const uint2*>(gh.g + rows[j] + cc);   // 16 rows in flight
      keep_live(r[0], r[1], r[2], r[3]); keep_live(r[4], r[5], r[6], r[7]);
      keep_live(r[8], r[9], r[10], r[11]); keep_live(r[12], r[13], r[14], r[15]);
      if constexpr (COMB)
        grad_half_add_comb(acc, r, gh, [&](int j) { return ((live >> j) & 1u) != 0; },
                           [&](int j, float& den, float& w) { den = __shfl(cden, gshift + j); w = __shfl(cw, gshift + j); });
      else
      grad_half_add(acc, r, gh, [&](int j) { return ((live >> j) & 1u) != 0; });
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

// The source rows of a key's sum, NB of them in flight: rows j0 .. j0+NB-1 of its list (clamped to the last one; loads issued
// together, adds in list order).  A key with few occurrences lists their batch positions in words 4.. of its record (lane i
// of the group holds word i: EVERY lane of the group must be here); a key with many lists consecutive rows of the partial
// sums.  The addresses are formed here, from the record word, not kept in an array across the kernel: with 8 pointers and
// 8 rows held per lane the update kernel needed 145 registers (3 waves per SIMD); this form needs 125 (Adam) / 109 (SGD).
// COMB (combined write-back): lanes 4.. of a key with few occurrences hold grad_out rows instead of batch positions, and the
// denominator / weight of their entry in cden / cw; each gradient row is scaled by comb_grad4 before it is added.
// GH (half gradients): the `grads` arm loads 8-byte granules from gh and forms G32 from them; the `partial` arm is the float one.
// COMB and GH (the typed combined write-back): the granule is a grad_out row's; it is up-cast and scaled, then goes through comb_grad4.
// Hot keys come first in the key list, so but for one wave the branch is wave-uniform; each arm has its NB loads in flight.
template <int NB, bool COMB = false, bool GH = false>
__device__ __forceinline__ void add_rows(float4& acc, const float* __restrict__ grads, const float* __restrict__ partial, bool hot,
                                         unsigned w, unsigned first, unsigned nsrc, unsigned j0, int dim, int c, int gshift,
                                         float cden = 0.f, float cw = 0.f, const GradHalfSrc gh = GradHalfSrc{nullptr, 1.f, 0}) {
  if constexpr (GH) {
    // (each arm adds for itself, in list order: the granules are up-cast one at a time, never NB float rows held at once)
    // (hot is the group's: the shuffles of the `grads` arm find every lane of their group in it)
    // (both arms address with 32-bit element offsets from a scalar base — fewer than 2^18 rows of at most 256 elements, as rows[]
    // of the sums: with 64-bit addresses the update kernels needed 129 - 139 registers, one waves-per-SIMD class below their twins)
    if (hot) {
      float4 x[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j)
        x[j] = *reinterpret_cast<const float4*>(partial + ((first + min(j0 + (unsigned)j, nsrc - 1)) * (unsigned)dim + (unsigned)c));
      if (NB == 4) keep_live(x[0], x[1], x[2], x[3]);
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (j0 + (unsigned)j < nsrc) { acc.x += x[j].x; acc.y += x[j].y; acc.z += x[j].z; acc.w += x[j].w; }
    } else {
      uint2 r[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const unsigned position = (unsigned)__shfl((int)w, gshift + 4 + (int)min(min(j0 + (unsigned)j, nsrc - 1), 7u));
        r[j] = *reinterpret_cast<const uint2*>(gh.g + (position * (unsigned)dim + (unsigned)c));
      }
      if (NB == 4) keep_live(r[0], r[1], r[2], r[3]);
      if constexpr (COMB)   // (position = the entry's grad_out row; element offsets below 2^32: the typed call refuses n_rows * dim beyond)
        grad_half_add_comb(acc, r, gh, [&](int j) { return j0 + (unsigned)j < nsrc; }, [&](int j, float& den, float& w) {
          const int src = gshift + 4 + (int)min(min(j0 + (unsigned)j, nsrc - 1), 7u);
          den = __shfl(cden, src); w = __shfl(cw, src);
        });
      else
      grad_half_add(acc, r, gh, [&](int j) { return j0 + (unsigned)j < nsrc; });
    }
    return;
  }
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
template <bool COMB = false, bool GH = false>
__device__ __forceinline__ float4 sum_rows(const float* __restrict__ grads, const float* __restrict__ partial, bool hot, unsigned w,
                                           unsigned first, unsigned nsrc, unsigned wmax, int dim, int c, int gshift,
                                           float cden = 0.f, float cw = 0.f, const GradHalfSrc gh = GradHalfSrc{nullptr, 1.f, 0}) {
  float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
  if (wmax <= 1) add_rows<1, COMB, GH>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, gshift, cden, cw, gh);
  else if (wmax <= 2) add_rows<2, COMB, GH>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, gshift, cden, cw, gh);
  else {
    add_rows<4, COMB, GH>(gg, grads, partial, hot, w, first, nsrc, 0, dim, c, gshift, cden, cw, gh);
    if (wmax > 4) add_rows<4, COMB, GH>(gg, grads, partial, hot, w, first, nsrc, 4, dim, c, gshift, cden, cw, gh);
  }
  for (unsigned j0 = 8; j0 < nsrc; j0 += 4) add_rows<4, COMB, GH>(gg, grads, partial, hot, w, first, nsrc, j0, dim, c, gshift, cden, cw, gh);
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
// Partial sums are fp32 for every ST, gradients fp32 unless the pack holds a GradHalf (above).  The float instantiations compile
// the code they always did (if constexpr).
// A StochP in the pack (half rows of a table with TFRA_OPTION_STOCHASTIC_ROUNDING): the parameter and the slots the rule owns are
// rounded by to_stored4_sr, one hash word per lane, field and granule, formed between the rule and the store; the constant fill
// of the other fields stays nearest-even.  Without one the pack's kernels compile the code they always did.
// The body is one function with two callers — apply_csr_kernel (one table per launch) and apply_csr_many_kernel (a list of tables
// per launch): blk = this block's index among the nblk blocks that work on THIS table's plan; they stand where the block index and
// the grid size of the launch stood, and nothing else differs.
template <int KIND, bool PHASE2, int ST, class... CS>
__device__ __forceinline__ void apply_csr_body(const TableView& v, OptP o, int dim, const float* __restrict__ grads,
                                               const float* __restrict__ partial, const CsrKeys& ks,
                                               const float* __restrict__ default_row, float aux0, float aux1,
                                               const ScoreP& sp, uint8_t* __restrict__ dflag, unsigned* any_deferred,
                                               unsigned use_gen, unsigned blk, unsigned nblk, const CS... cs) {
  constexpr bool COMB = (false || ... || std::is_same<CS, CombRows>::value);
  constexpr bool STOCH = HasStoch<CS...>::v;
  constexpr bool GH = HasGradHalf<CS...>::v;
  static_assert(!STOCH || ST != TFRA_F32, "stochastic rounding is of half rows");
  const GradHalfSrc gh = grad_half_in(cs...);
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
        float4 gg = sum_rows<COMB, GH>(grads, partial, hot, COMB ? wsrc : w, first, nsrc, wmax, dim, c, gshift, cden, cw, gh);
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
        if constexpr (STOCH) {
          const u64 kb = sr_key(stoch_in(cs...), key);
          if (col) {
            store_wt8(sr + c, to_stored4_sr<ST>(p, sr_word(kb, (unsigned)c)));
            if (S >= 1) store_wt8(sr + dim + c, to_stored4_sr<ST>(s1, sr_word(kb, (unsigned)(dim + c))));
            if (S >= 2) store_wt8(sr + 2 * dim + c, to_stored4_sr<ST>(s2, sr_word(kb, (unsigned)(2 * dim + c))));
          }
        } else {
        if (col) {
          store_wt8(sr + c, to_stored4<ST>(p));
          if (S >= 1) store_wt8(sr + dim + c, to_stored4<ST>(s1));
          if (S >= 2) store_wt8(sr + 2 * dim + c, to_stored4<ST>(s2));
        }
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
      float4 gg = sum_rows<COMB, GH>(grads, partial, hot, COMB ? wsrc : w, first, nsrc, wmax, dim, c, gshift, cden, cw, gh);
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

// ---- the grouped form (tfra_multi_apply_planned_combined): the combined write-backs of a LIST of tables, one sums launch per NCH
// class and one update launch per (rule, storage type) class.  What a single-table launch takes as kernel arguments is a record
// in device memory here (tfra_pool.hip: 26 tables' records do not fit the 4 KB of kernel arguments).  A class is a list of record
// indices `idx` and the blocks' prefix sums over it: the grid is the concatenation of the class's descriptors, descriptor j owning
// the blocks [prefix[j], prefix[j + 1]), and both kernels stride by THAT count.  blockIdx.x is wave-uniform, so the search, the
// index and the record are scalar loads into scalar registers, as kernel arguments are.  (The kernels: tfra_apply_many.hip.)
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
// tfra_multi_apply_planned_combined_typed: what a descriptor with a float16 / bfloat16 grad_out adds to its ApplyManyRec, in an array
// beside the records (same index) that only the half classes' kernels read; `grads` of the record holds the half matrix's address then.
// (A record of its own: ApplyManyRec keeps its size, the float classes' kernels the code they had.)
struct GradHalfRec {
  const float* d_scale;
  int is_bf16;
};

}  // namespace
