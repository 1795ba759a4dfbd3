// The bodies of the pooled lookup and of its weight gradient for WIDE rows, 256 < dim <= 1024 (tfra_pool_wide.hip): ONE
// wave64 per output row, four rows per 256-thread block, where find_combine_row / wgrad_row (tfra_pool_device.h, tfra_wgrad_device.h)
// give a row to one 16-lane group whose lanes hold NCH <= 4 chunks of 64 columns.  A group that held 16 chunks per lane would keep
// t[16][4] float4 in flight — 256 VGPRs — and cover 256 bytes of a 4 KB row per load instruction; so the row belongs to a wave here,
// and the two kernels split that wave differently, because their arithmetic allows different things.
//
// Both take a row's entries [b, e) 64 at a time — lane j loads id and weight of entry p0 + j and hashes it, the next 64 loading
// behind this batch — and of those FOUR at a time: group k (lanes 16 k .. 16 k + 15) probes entry p0 + q + k with probe_find_word,
// whose sub / gshift arguments make it a per-group function, so four key lines are in flight, one per group.  The key lines of the
// NEXT four entries are loaded before this four's rows are used (inside a batch of 64), so a probe's latency hides behind the row
// reads in front of it.  Loads stay unconditional as in the twins: an entry past the row's end is clamped to its last entry
// (probed and read again, a member of nothing), a column at or beyond dim to column 0 (read, neither added nor stored);
// row_splits is clamped to 0 <= b <= e <= nnz.  No LDS: what the groups resolve goes round by __shfl.
// The results are the twins' expressions in the twins' order (comb_wsum / comb_acc4 / comb_finish4; wgrad_dot4 / wgrad_reduce16 /
// wgrad_s / wgrad_finish, under -ffp-contract=off), which at these widths only the op chain evaluates today: unique, tfra_table_find
// and tfra_sparse_segment_combine[_backprop_weights].  Bit for bit those.
// Not here: typed outputs, a half grad_out, tiers, the grouped *_many calls, long-row blocks at wide dims.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_pool.h"
#include "tfra_pool_device.h"
#include "tfra_pool_long_device.h"

namespace tfra {
namespace {

constexpr int WIDE_THREADS = 256;   // four waves, one output row each
constexpr int WIDE_ROWS = WIDE_THREADS / 64;

// What a wave keeps of the four entries whose probe is under way: lane L of group k holds entry p0 + q + k's key, home buckets and
// word L of its first key line (the load in flight until wide_resolve inspects it).
struct WideProbe {
  i64 key, k0;
  unsigned b0, b1;
};
// start the probes of the four entries q .. q + 3 of a batch from what the batch's lanes hold (kreg: the id; b0reg, b1reg: its buckets)
__device__ __forceinline__ void wide_issue(const TableView& v, i64 kreg, unsigned b0reg, unsigned b1reg, int q, int grp, int sub,
                                           WideProbe& pr) {
  const int j = q + grp;
  pr.key = shfl_i64(kreg, j);
  pr.b0 = (unsigned)__shfl((int)b0reg, j);
  pr.b1 = (unsigned)__shfl((int)b1reg, j);
  pr.k0 = key_line(v, pr.b0)[sub];
}
// finish this group's probe: its entry's row, default_row on a miss
__device__ __forceinline__ const unsigned char* wide_resolve(const TableView& v, const WideProbe& pr, int sub, int gshift,
                                                             const unsigned char* __restrict__ default_row) {
  const i64 word = probe_find_word(v, pr.key, pr.b0, pr.b1, pr.k0, sub, gshift);
  return word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
}
__device__ __forceinline__ const unsigned char* shfl_ptr(const unsigned char* p, int src) {
  return reinterpret_cast<const unsigned char*>((uintptr_t)shfl_i64((i64)(uintptr_t)p, src));
}

// ---- the forward: the wave split over COLUMNS ---------------------------------------------------------------------------------------
// NCW = ceil(dim / 256) chunks of 256 columns; lane L holds columns 256 c + 4 L .. + 3 of chunk c, so a row load is one contiguous
// 1 KB (float32 rows) or 512 B (half rows) per instruction and the accumulator is acc[NCW] float4.  Accumulation is elementwise,
// so ANY column mapping gives the twin's bits: that is why the wave may be split this way here.  The four row pointers the groups
// resolved go to all 64 lanes from lanes 0, 16, 32 and 48; then t[NCW][4] is loaded — at most 16 float4, 64 VGPRs —, the next four
// probes are started, and the adds run in entry order u = 0 .. 3, for members only.  PRUNE and FILL are find_combine_row's: the
// weight sum and the adds run over the entries with weight > 0; a row without members is the row of fill_id (default_row on a
// miss), up-cast and written AS IT IS.  `any` is uniform in the wave: every lane saw the same members.
template <int DT, int NCW, bool RAGGED, bool SAFE>
__device__ __forceinline__ void find_combine_wide_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                      const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                      const unsigned char* __restrict__ default_row, float* __restrict__ out,
                                                      size_t r, const RaggedArgs& rg) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  if (r >= n_rows) return;   // (the whole wave)
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, r, b, e);
  bool prune = false, any = false;   // (SAFE only) any: the row has a member
  if constexpr (SAFE) prune = (rg.flags & TFRA_RAGGED_PRUNE) && w;
  float wsum;
  if constexpr (SAFE) wsum = combiner == 0 ? 0.f : (prune ? comb_wsum_pruned(w, b, e, combiner) : comb_wsum(w, b, e, combiner));
  else wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  const float scale = comb_scale_of(wsum, combiner);
  unsigned coff[NCW];   // this lane's byte offset inside a row, per chunk
  bool cok[NCW];
  float4 acc[NCW];
#pragma unroll
  for (int c = 0; c < NCW; ++c) {
    const int col = c * 256 + lane * 4;
    cok[c] = col < dim;
    coff[c] = cok[c] ? (unsigned)col * EB : 0u;
    acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (b < e) {
    const int last = e - 1;
    i64 knext = ids[min(b + lane, last)];
    float wnext = w ? w[min(b + lane, last)] : 1.f;
    for (int p0 = b; p0 < e; p0 += 64) {
      const i64 kreg = knext;
      const float wreg = wnext;
      if (p0 + 64 < e) {   // the next 64 entries, in flight behind this batch's probes and rows
        const int pn = min(p0 + 64 + lane, last);
        knext = ids[pn];
        wnext = w ? w[pn] : 1.f;
      }
      u64 hreg;
      const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
      const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
      const int nq = min(64, e - p0);
      WideProbe pr;
      wide_issue(v, kreg, b0reg, b1reg, 0, grp, sub, pr);
      for (int q = 0; q < nq; q += 4) {
        const unsigned char* mine = wide_resolve(v, pr, sub, gshift, default_row);
        const unsigned char* src[4];
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          src[u] = shfl_ptr(mine, 16 * u);
          x[u] = __shfl(wreg, q + u);
        }
        Raw t[NCW][4];
#pragma unroll
        for (int c = 0; c < NCW; ++c) {
#pragma unroll
          for (int u = 0; u < 4; ++u) t[c][u] = *reinterpret_cast<const Raw*>(src[u] + coff[c]);   // 4 NCW row loads in flight
        }
        if (q + 4 < nq) wide_issue(v, kreg, b0reg, b1reg, q + 4, grp, sub, pr);   // the next four key lines behind them
#pragma unroll
        for (int c = 0; c < NCW; ++c) keep_live(t[c][0], t[c][1], t[c][2], t[c][3]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          bool member = p0 + q + u < e;
          if constexpr (SAFE) {
            member = member && (!prune || x[u] > 0.f);
            any = any || member;
          }
          if (member) {
#pragma unroll
            for (int c = 0; c < NCW; ++c)
              if (cok[c]) comb_acc4(acc[c], PoolRow<DT>::widen(t[c][u]), x[u]);
          }
        }
      }
    }
  }
  float* o = out + r * (size_t)dim;
  if constexpr (SAFE) {
    if ((rg.flags & TFRA_RAGGED_FILL) && !any) {   // every group probes fill_id and finds the same row
      u64 h;
      const unsigned f0 = (unsigned)bucket0(rg.fill_id, v.nb, h);
      const unsigned f1 = (unsigned)bucket1(h, f0, v.nb);
      const i64 word = probe_find_word(v, rg.fill_id, f0, f1, key_line(v, f0)[sub], sub, gshift);
      const unsigned char* src = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
#pragma unroll
      for (int c = 0; c < NCW; ++c)
        if (cok[c]) *reinterpret_cast<float4*>(o + c * 256 + lane * 4) = PoolRow<DT>::widen(*reinterpret_cast<const Raw*>(src + coff[c]));
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < NCW; ++c)
    if (cok[c]) *reinterpret_cast<float4*>(o + c * 256 + lane * 4) = comb_finish4(acc[c], wsum, scale, combiner);
}

// ---- the weight gradient: the wave split over ENTRIES -----------------------------------------------------------------------------
// The dot product's order is pinned to the 16-lane mapping of tfra_combine_device.h — lane `sub` adds its products over chunks of 64
// columns, ascending, then wgrad_reduce16 —, so the columns cannot be dealt out over 64 lanes.  Instead every group keeps its own
// copy of g: grad_out[r, :] in the 16-lane mapping, NCH = 4 NCW <= 16 float4 per lane, loaded once.  Group k owns entry p0 + q + k
// outright: it probes it and streams its row four chunks at a time, the next four loading while these are multiplied (d needs no
// more than the current chunks), so four entries' rows are read in parallel per wave.  The four d then go to all lanes from lanes
// 0, 16, 32 and 48 and every lane runs wgrad_s for u = 0 .. 3 in entry order: s is the twin's.  Lane j keeps the raw d of entry
// p0 + j (0 for a non-member) and the wave stores a batch's 64 values in one coalesced store.  mean / sqrtn make the twin's second
// pass over the wave's own [b, e): lane j re-reads what lane j wrote (entry b + 64 i + j both times), so program order suffices.
template <int DT, int NCW, bool RAGGED, bool PRUNE>
__device__ __forceinline__ void wgrad_wide_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                               const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                               const unsigned char* __restrict__ default_row, const float* __restrict__ grad_out,
                                               float* dw, size_t r, const RaggedArgs& rg) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;
  constexpr int NCH = 4 * NCW;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  if (r >= n_rows) return;   // (the whole wave)
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, r, b, e);
  if (b >= e) return;
  float wsum;
  if constexpr (PRUNE) wsum = combiner == 0 ? 0.f : comb_wsum_pruned(w, b, e, combiner);
  else wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  float4 g[NCH];
  const float* G = grad_out + r * (size_t)dim;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 64 + sub * 4;
    g[c] = *reinterpret_cast<const float4*>(G + (col < dim ? col : 0));
  }
  float s = 0.f;
  const int last = e - 1;
  i64 knext = ids[min(b + lane, last)];
  float wnext = w ? w[min(b + lane, last)] : 1.f;
  for (int p0 = b; p0 < e; p0 += 64) {
    const i64 kreg = knext;
    const float wreg = wnext;
    if (p0 + 64 < e) {
      const int pn = min(p0 + 64 + lane, last);
      knext = ids[pn];
      wnext = w ? w[pn] : 1.f;
    }
    u64 hreg;
    const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
    const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
    const int nq = min(64, e - p0);
    float dmine = 0.f;   // the raw d of entry p0 + lane
    WideProbe pr;
    wide_issue(v, kreg, b0reg, b1reg, 0, grp, sub, pr);
    for (int q = 0; q < nq; q += 4) {
      const unsigned char* src = wide_resolve(v, pr, sub, gshift, default_row);   // this group's entry: p0 + q + grp
      Raw t[2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = i * 64 + sub * 4;
        t[0][i] = *reinterpret_cast<const Raw*>(src + (col < dim ? (unsigned)col * EB : 0u));
      }
      if (q + 4 < nq) wide_issue(v, kreg, b0reg, b1reg, q + 4, grp, sub, pr);   // the next four key lines behind the row's head
      float d = 0.f;
#pragma unroll
      for (int cb = 0; cb < NCW; ++cb) {
        if (cb + 1 < NCW) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int col = ((cb + 1) * 4 + i) * 64 + sub * 4;
            t[(cb + 1) & 1][i] = *reinterpret_cast<const Raw*>(src + (col < dim ? (unsigned)col * EB : 0u));
          }
        }
        keep_live(t[cb & 1][0], t[cb & 1][1], t[cb & 1][2], t[cb & 1][3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = cb * 4 + i;
          if (c * 64 + sub * 4 < dim) wgrad_dot4(d, g[c], PoolRow<DT>::widen(t[cb & 1][i]));
        }
      }
      d = wgrad_reduce16(d);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float du = __shfl(d, 16 * u), xu = __shfl(wreg, q + u);
        bool member = p0 + q + u < e;
        if constexpr (PRUNE) member = member && xu > 0.f;
        if (member) wgrad_s(s, xu, du);
        if (lane == q + u) dmine = member ? du : 0.f;
      }
    }
    if (p0 + lane < e) dw[p0 + lane] = dmine;   // one coalesced store per batch
  }
  if (combiner == 0) return;
  for (int p = b + lane; p < e; p += 64) {   // lane j re-reads what lane j wrote
    const float x = w ? w[p] : 1.f;
    const float d = dw[p];
    bool member = true;
    if constexpr (PRUNE) member = x > 0.f;
    dw[p] = member ? wgrad_finish(d, x, s, wsum, combiner) : 0.f;
  }
}

}  // namespace
}  // namespace tfra
