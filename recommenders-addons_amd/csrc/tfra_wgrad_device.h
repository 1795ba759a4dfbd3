// The body of the pooled lookup's weight gradient, ONE copy for its kernels: wgrad_kernel and wgrad_ragged_kernel (tfra_wgrad.hip)
// read one table; tier_wgrad_kernel and tier_wgrad_ragged_kernel (tfra_tierwgrad.hip) read the two tables of a tier through the
// same function (its TIER axis, find_combine_row's: tfra_pool_device.h); the grouped kernels (tfra_wgrad_many.hip) call it per
// descriptor of a list.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_optim_device.h"
#include "tfra_pool.h"

namespace tfra {
namespace {

// The row r of this lane's group: its entries [b, e) are taken 16 at a time — lane j loads id and weight of entry p0 + j and hashes
// it, the next 16 loading behind this batch — and of those U at a time: U key lines in flight before any is inspected, then the U
// rows (t[NCH][U], the forward's big array) before any is used.  g[NCH] holds this lane's columns of grad_out[r, :], loaded once.
// Per entry: the lane's products, the group's reduction, s += w * d for a member; lane j keeps the raw d of entry p0 + j and the
// group stores the batch's 16 values in one coalesced store (0 for an entry that is no member).
// mean / sqrtn need s over the WHOLE row: the same group makes a second pass over its own [b, e) of dw — no rows, no probes — in
// which lane j re-reads exactly the values lane j wrote (entry b + 16 k + j both times), so program order suffices: no fence.
// Loads stay unconditional as in find_combine_row: entries past the row's end are clamped to its last entry (probed and read again,
// not used), columns past dim to column 0 (read, not added).  The probe is probe_find_word with plain loads.
// Compile-time axes beside (DT, U, NCH):
//   RAGGED  [b, e) from int64 row_splits clamped to 0 <= b <= e <= nnz, instead of the start_end ints of the bounds launch;
//   PRUNE   (with weights) an entry whose weight is not > 0 is no member: 0 out, and neither in s nor in wsum;
//   TIER    a second view, *lo, stands behind v (a tier's lower table behind its cache): an entry's row is the one v
//           holds, else the one *lo holds, else default_row.  The block is find_combine_row's (tfra_pool_device.h), statement for
//           statement: the key's hash is taken once and reduced to home buckets once per view by the lane that hashed; *lo's key
//           lines are loaded only for a U-batch in which an entry missed v — the probe's word is uniform in the group, so the
//           branch is — and all U of them at once; only the entries that missed v are probed there.  (Two copies of that block,
//           not one helper: as a __forceinline__ function it changed the code of existing kernels)  Everything
//           behind src[u] is the one-table code.
//   GHALF   grad_out is float16 or bfloat16 (the *_typed calls): the ONE difference is the load of g[NCH] — a lane's
//           four elements are one 8-byte load (the group's 16 lanes: one 128-byte line per chunk), up-cast exactly by the helpers
//           GradHalf uses (load_stored4, tfra_optim_device.h) and multiplied by the scale, one fp32 multiplication rounded on its
//           own, so that everything behind g[NCH] sees GO32[r, c] = f32(grad_out[r, c]) * s of the untyped call.  is_bf16 is
//           wave-uniform (a kernel argument or a field of the descriptor's record): ONE class for both formats.  *d_scale is read
//           once per group, before the entry loop, at a uniform address (a scalar load); nullptr: 1.0f, x * 1.0f being exact.
//           The row base is formed in 64 bits, as the float one is.  Without GHALF neither argument is read.
// An entry in no row is never visited: the memset before the launch is its 0.  (TFRA_RAGGED_FILL needs no code: a row without
// members has only pruned entries.)  Without TIER `lo` is not read.
template <int DT, int U, int NCH, bool RAGGED, bool PRUNE, bool TIER = false, bool GHALF = false>
__device__ __forceinline__ void wgrad_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                          const float* __restrict__ w, const int* __restrict__ start_end,
                                          const i64* __restrict__ row_splits, int nnz, int combiner,
                                          const unsigned char* __restrict__ default_row, const float* __restrict__ grad_out,
                                          float* dw, size_t r, const TableView* lo = nullptr, const float* d_scale = nullptr,
                                          int is_bf16 = 0) {
  static_assert(U == 4, "keep_live is written for U == 4");
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  if (r >= n_rows) return;
  int b, e;
  if constexpr (RAGGED) {
    const i64 lo_s = row_splits[r], hi_s = row_splits[r + 1];
    b = (int)min(max(lo_s, (i64)0), (i64)nnz);
    e = (int)min(max(hi_s, (i64)b), (i64)nnz);
  } else {
    b = start_end[r];
    e = start_end[n_rows + r];
  }
  if (b >= e) return;
  float wsum;
  if constexpr (PRUNE) wsum = combiner == 0 ? 0.f : comb_wsum_pruned(w, b, e, combiner);
  else wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  unsigned coff[NCH];   // this lane's byte offset inside a row, per chunk
  bool cok[NCH];
  float4 g[NCH];
  if constexpr (GHALF) {
    typedef float v4f_t __attribute__((ext_vector_type(4)));
    const float gs = d_scale ? *d_scale : 1.f;
    const unsigned short* G = reinterpret_cast<const unsigned short*>(grad_out) + r * (size_t)dim;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 64 + sub * 4;
      cok[c] = col < dim;
      coff[c] = cok[c] ? (unsigned)col * EB : 0u;
      const uint2 raw = *reinterpret_cast<const uint2*>(G + (cok[c] ? col : 0));
      float4 x = is_bf16 ? load_stored4<TFRA_BF16>(raw) : load_stored4<TFRA_F16>(raw);
      x.x *= gs; x.y *= gs; x.z *= gs; x.w *= gs;
      // The float arm's g[c] is a 16-byte load's result: four consecutive registers.  The products are placed the same way (an
      // empty asm over a 4-vector): left to itself the register allocator gave float32-row kernels up to 7 VGPRs more than their
      // float twins, three of them a waves-per-SIMD class lower (profiles/wgrad_half_isa_stats.txt).
      v4f_t q = {x.x, x.y, x.z, x.w};
      asm volatile("" : "+v"(q));
      g[c] = make_float4(q.x, q.y, q.z, q.w);
    }
  } else {
    const float* G = grad_out + r * (size_t)dim;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 64 + sub * 4;
      cok[c] = col < dim;
      coff[c] = cok[c] ? (unsigned)col * EB : 0u;
      g[c] = *reinterpret_cast<const float4*>(G + (cok[c] ? col : 0));
    }
  }
  float s = 0.f;
  const int last = e - 1;
  i64 knext = ids[min(b + sub, last)];
  float wnext = w ? w[min(b + sub, last)] : 1.f;
  for (int p0 = b; p0 < e; p0 += 16) {
    const i64 kreg = knext;
    const float wreg = wnext;
    if (p0 + 16 < e) {   // the next 16 entries, in flight behind this batch's probes and rows
      const int pn = min(p0 + 16 + sub, last);
      knext = ids[pn];
      wnext = w ? w[pn] : 1.f;
    }
    u64 hreg;
    const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
    const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
    unsigned l0reg = 0, l1reg = 0;   // (TIER) the same hash reduced by the lower table's nb
    if constexpr (TIER) {
      l0reg = __umulhi((unsigned)(hreg >> 32), (unsigned)lo->nb);
      l1reg = (unsigned)bucket1(hreg, l0reg, lo->nb);
    }
    float dmine = 0.f;   // the raw d of entry p0 + sub
    for (int q = 0; q < 16 && p0 + q < e; q += U) {
      i64 key[U], k0[U];
      unsigned b0[U], b1[U];
      float x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = gshift + q + u;
        key[u] = shfl_i64(kreg, j);
        b0[u] = (unsigned)__shfl((int)b0reg, j);
        b1[u] = (unsigned)__shfl((int)b1reg, j);
        x[u] = __shfl(wreg, j);
        k0[u] = key_line(v, b0[u])[sub];   // U probes in flight
      }
      keep_live(k0[0], k0[1], k0[2], k0[3]);
      const unsigned char* src[U];
      if constexpr (TIER) {
        bool missed[U], any_missed = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const i64 word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift);
          missed[u] = word < 0;
          any_missed = any_missed || missed[u];
          src[u] = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
        }
        if (any_missed) {   // (uniform in the group) a batch of cache hits pays nothing below
          const int j0 = gshift + q;
          i64 m0[U];
          unsigned c0[U], c1[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            c0[u] = (unsigned)__shfl((int)l0reg, j0 + u);
            c1[u] = (unsigned)__shfl((int)l1reg, j0 + u);
            m0[u] = key_line(*lo, c0[u])[sub];   // U probes in flight below
          }
          keep_live(m0[0], m0[1], m0[2], m0[3]);
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (!missed[u]) continue;
            const i64 word = probe_find_word(*lo, key[u], c0[u], c1[u], m0[u], sub, gshift);
            if (word >= 0) src[u] = word_row_ptr(*lo, (u64)word);
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const i64 word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift);
          src[u] = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
        }
      }
      Raw t[NCH][U];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int u = 0; u < U; ++u) t[c][u] = *reinterpret_cast<const Raw*>(src[u] + coff[c]);   // U rows in flight
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) keep_live(t[c][0], t[c][1], t[c][2], t[c][3]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          if (cok[c]) wgrad_dot4(d, g[c], PoolRow<DT>::widen(t[c][u]));
        d = wgrad_reduce16(d);
        bool member = p0 + q + u < e;
        if constexpr (PRUNE) member = member && x[u] > 0.f;
        if (member) wgrad_s(s, x[u], d);
        if (sub == q + u) dmine = member ? d : 0.f;
      }
    }
    if (p0 + sub < e) dw[p0 + sub] = dmine;   // one coalesced store per batch
  }
  if (combiner == 0) return;
  for (int p = b + sub; p < e; p += 16) {   // lane j re-reads what lane j wrote
    const float x = w ? w[p] : 1.f;
    const float d = dw[p];
    bool member = true;
    if constexpr (PRUNE) member = x > 0.f;
    dw[p] = member ? wgrad_finish(d, x, s, wsum, combiner) : 0.f;
  }
}

}  // namespace
}  // namespace tfra
