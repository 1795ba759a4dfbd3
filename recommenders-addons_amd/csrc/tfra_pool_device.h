// The body of the pooled lookup, ONE copy for its kernels: find_combine_kernel, find_combine_many_kernel and their ragged forms
// (tfra_pool.hip) read one table; tier_find_combine_kernel and tier_find_combine_ragged_kernel (tfra_tierpool.hip) read the two
// tables of a tier through the same function (its TIER axis).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_pool.h"

namespace tfra {
namespace {

// One 16-lane group per output row (find_wave's and seg_combine_kernel's mapping: 4 rows per wave64).  The row's entries [b, e)
// are taken 16 at a time — lane j of the group loads id and weight of entry p0 + j and hashes it, one instruction stream for 16
// keys, the next 16 loading while these are worked on — and of those U at a time: U key lines in flight before any is inspected,
// then the U rows (NCH column chunks of 64 floats each: lane `sub` holds columns 64 c + 4 sub .. + 3) before any is accumulated.
// Accumulation is strictly in entry order.  Loads stay unconditional, as in find_wave: entries past the row's end are clamped to
// its last entry (probed and read again, not accumulated), columns past dim to column 0.
// The probe is find_kernel's (probe_find_word: plain loads), so a lookup that runs beside a write-back sees what tfra_table_find sees.
// The body is one function with six callers — find_combine_kernel (one table per launch), find_combine_many_kernel (a list of
// tables per launch), their ragged forms, and the tier's two kernels — so that all compile the same expressions: r is the output
// row of this lane's group in ITS table.
// Three compile-time axes beside (DT, U, NCH):
//   RAGGED  where [b, e) comes from: the start_end ints of the bounds launch, or an int64 row_splits[n_rows + 1] (a rank-2
//           RaggedTensor's, PY/ragged_embedding_ops.py:129-442) clamped to 0 <= b <= e <= nnz — whatever row_splits holds, no
//           entry outside [0, nnz) is read.
//   SAFE    safe_embedding_lookup_sparse's semantics (PY/ragged_embedding_ops.py:414-440), by rg.flags:
//           TFRA_RAGGED_PRUNE (with weights): only the entries with weight > 0 are members — the weight sum and the accumulation
//           run over them, in entry order, as over the compacted list; a pruned entry is still probed and read (loads stay
//           unconditional), like an entry past the row's end;
//           TFRA_RAGGED_FILL: a row without members is the row of rg.fill_id (default_row on a miss), up-cast and written AS IT IS
//           (no acc += 1 * x, no scaling: a -0.0 survives).
//   TIER    a second view, *lo, stands behind v (a tier's lower table behind its cache): an entry's row is the one v
//           holds, else the one *lo holds, else default_row.  The key's hash is taken once and reduced to home buckets once per
//           view (the two tables differ in nb).  *lo's key lines are loaded only for a U-batch in which an entry missed v — the
//           probe's word is uniform in the group, so the branch is — and all U of them at once; only the entries that missed v
//           are probed there.  The fill id goes the same way.  Both probes are probe_find_word: reserved keys take its own path
//           in each view.
//   OT      the type of the output row (the typed lookups): float32, or a half type — `out` then points to 2-byte
//           elements, and the function's two stores (the FILL row, the finished accumulator) narrow their float4 to 8 B first
//           (PoolOut<OT>::narrow: round to nearest even).  Nothing in front of the two stores knows OT.
// Without RAGGED and SAFE the function is the one it was: `rg` is not read.  Without TIER `lo` is not read.  With OT float32 the
// stores are the float4 stores they were, chunk by chunk.
struct RaggedArgs {
  const i64* row_splits;
  int nnz;
  unsigned flags;
  i64 fill_id;
};
template <int DT, int U, int NCH, bool RAGGED = false, bool SAFE = false, bool TIER = false, int OT = TFRA_F32>
__device__ __forceinline__ void find_combine_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                 const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                 const unsigned char* __restrict__ default_row, float* __restrict__ out, size_t r,
                                                 const RaggedArgs& rg = RaggedArgs{}, const TableView* lo = nullptr) {
  static_assert(U == 4, "keep_live is written for U == 4");
  typedef typename PoolRow<DT>::Raw Raw;
  typedef typename PoolOut<OT>::Elem OutElem;
  typedef typename PoolOut<OT>::Vec OutVec;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  if (r >= n_rows) return;
  int b, e;
  if constexpr (RAGGED) {
    const i64 lo_s = rg.row_splits[r], hi_s = rg.row_splits[r + 1];
    b = (int)min(max(lo_s, (i64)0), (i64)rg.nnz);
    e = (int)min(max(hi_s, (i64)b), (i64)rg.nnz);
  } else {
    b = start_end[r];
    e = start_end[n_rows + r];
  }
  bool prune = false, any = false;   // (SAFE only) any: the row has a member
  if constexpr (SAFE) prune = (rg.flags & TFRA_RAGGED_PRUNE) && w;
  float wsum;
  if constexpr (SAFE) wsum = combiner == 0 ? 0.f : (prune ? comb_wsum_pruned(w, b, e, combiner) : comb_wsum(w, b, e, combiner));
  else wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  const float scale = comb_scale_of(wsum, combiner);
  unsigned coff[NCH];   // this lane's byte offset inside a row, per chunk
  bool cok[NCH];
  float4 acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 64 + sub * 4;
    cok[c] = col < dim;
    coff[c] = cok[c] ? (unsigned)col * EB : 0u;
    acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (b < e) {
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
          bool member = p0 + q + u < e;
          if constexpr (SAFE) {
            member = member && (!prune || x[u] > 0.f);
            any = any || member;
          }
          if (member) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) comb_acc4(acc[c], PoolRow<DT>::widen(t[c][u]), x[u]);
          }
        }
      }
    }
  }
  OutElem* o = reinterpret_cast<OutElem*>(out) + r * (size_t)dim;
  if constexpr (SAFE) {
    if ((rg.flags & TFRA_RAGGED_FILL) && !any) {   // (uniform in the group: every lane saw the same members)
      u64 h;
      const unsigned f0 = (unsigned)bucket0(rg.fill_id, v.nb, h);
      const unsigned f1 = (unsigned)bucket1(h, f0, v.nb);
      const i64 word = probe_find_word(v, rg.fill_id, f0, f1, key_line(v, f0)[sub], sub, gshift);
      const unsigned char* src = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
      if constexpr (TIER) {
        if (word < 0) {
          const unsigned g0 = __umulhi((unsigned)(h >> 32), (unsigned)lo->nb);
          const unsigned g1 = (unsigned)bucket1(h, g0, lo->nb);
          const i64 below = probe_find_word(*lo, rg.fill_id, g0, g1, key_line(*lo, g0)[sub], sub, gshift);
          if (below >= 0) src = word_row_ptr(*lo, (u64)below);
        }
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (cok[c])
          *reinterpret_cast<OutVec*>(o + c * 64 + sub * 4) = PoolOut<OT>::narrow(PoolRow<DT>::widen(*reinterpret_cast<const Raw*>(src + coff[c])));
      return;
    }
  }
  if constexpr (OT == TFRA_F32) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (cok[c]) *reinterpret_cast<float4*>(o + c * 64 + sub * 4) = comb_finish4(acc[c], wsum, scale, combiner);
  } else {
    // every chunk finished and packed before the first store: narrowing chunk by chunk between the stores took the safe ragged
    // NCH = 2 kernels from the twins' 79 VGPRs to 81, 6 to 5 waves per SIMD (profiles/typed_lookup_isa_stats.txt)
    OutVec fin[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) fin[c] = PoolOut<OT>::narrow(comb_finish4(acc[c], wsum, scale, combiner));
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (cok[c]) *reinterpret_cast<OutVec*>(o + c * 64 + sub * 4) = fin[c];
  }
}

}  // namespace
}  // namespace tfra
