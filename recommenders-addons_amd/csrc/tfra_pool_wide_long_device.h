// The bodies of the pooled lookup and of its weight gradient for LONG WIDE rows: 256 < dim <= 1024 and a few hundred entries per
// row (tfra_pool_wide_long.hip).  find_combine_wide_row / wgrad_wide_row (tfra_pool_wide_device.h) give an output row
// to ONE wave64, which keeps four key lines and 4 NCW row loads in flight and spends three quarters of its cycles waiting for them;
// a batch of 512 rows of 256 entries puts 512 waves on a chip of 1024 SIMDs.  Here a row belongs to a BLOCK.  The long form of
// dim <= 256 (tfra_pool_long_device.h) does not carry over: its 16 KiB slab of up-cast rows is sized for NCH <= 4, and its 16-lane
// column mapping is the wrong one at these widths.  The only LDS here is sixteen words per window: what the groups resolved.
//
// The entries of a row [b, e) come as in the wave form: every wave loads the same batch of entries — lane j holds id, weight and
// home buckets of entry p0 + j — and takes what it needs from its own lanes, so ids and weights need no LDS.  Inside a batch the
// block takes a WINDOW of entries at a time, one entry per 16-lane group of the block: group k of wave c probes entry 4 c + k of
// the window with wide_issue / wide_resolve as they stand, and the next window's probes start before this window's rows are used.
// What a group resolved goes to a double-buffered LDS array, one __syncthreads() per window: array (n + 1) & 1 was last read in
// window n - 1, which every wave left before any passed the barrier of window n.  Every wave of a block runs the same windows (b, e
// and the weights are the block's), so the barriers are uniform.  Loads stay unconditional: an entry past the row's end is clamped
// to its last entry, a column at or beyond dim to column 0; row_splits is clamped to 0 <= b <= e <= nnz.
// The results are the wave forms' expressions in the wave forms' order, so the op chain's, bit for bit.
// Not here: typed outputs, a half grad_out, tiers, the grouped *_many calls, a mixed short / long dispatch at wide dims.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_pool.h"
#include "tfra_pool_device.h"
#include "tfra_pool_long_device.h"
#include "tfra_pool_wide_device.h"

namespace tfra {
namespace {

constexpr int WIDE_LONG_GROUPS = 16;   // the most 16-lane groups a block has: the entries of its largest window

// What lane `src` of this wave holds, for a `src` that is the same in every lane (a window's index): one v_readlane per word, and the
// result is the wave's, not a lane's — a row pointer taken this way is a scalar base for the row loads behind it.
__device__ __forceinline__ unsigned wave_word(unsigned x, int src) { return (unsigned)__builtin_amdgcn_readlane((int)x, src); }
__device__ __forceinline__ float wave_float(float x, int src) { return __uint_as_float(wave_word(__float_as_uint(x), src)); }
__device__ __forceinline__ const unsigned char* wave_ptr(u64 p, int src) {
  const u64 lo = wave_word((unsigned)p, src), hi = wave_word((unsigned)(p >> 32), src);
  return reinterpret_cast<const unsigned char*>((uintptr_t)(hi << 32 | lo));
}

// ---- the forward: a wave per 256-column CHUNK --------------------------------------------------------------------------------------
// 64 NCW threads, NCW = ceil(dim / 256).  Wave c owns chunk c for the whole row: lane L holds columns 256 c + 4 L .. + 3 in ONE
// float4 accumulator, where the wave form has acc[NCW].  Accumulation is elementwise and a column is still summed in entry order
// by one lane, so the bits are the wave form's.  A window is W = 4 NCW entries (8, 12 or 16), a batch the largest multiple of W
// that is at most 64 (64, 60, 64).  Behind the barrier every wave loads ITS chunk of all W rows before it uses the first — at most
// 16 Raw per lane, the budget of the wave form's t[NCW][4], and NCW times as many rows in flight per output row —, starts the next
// window's probes and adds in entry order u = 0 .. W - 1, members only.  PRUNE, FILL, `any` and wsum are find_combine_wide_row's;
// every wave sees every weight, so `any` and wsum are the same in all of them, and a row without members has fill_id probed by
// each wave and its chunk written as it is.
template <int DT, int NCW, bool RAGGED, bool SAFE>
__device__ __forceinline__ void find_combine_wide_long_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                           const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                           const unsigned char* __restrict__ default_row, float* __restrict__ out,
                                                           size_t r, const RaggedArgs& rg) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  constexpr int W = 4 * NCW, BATCH = 64 / W * W;
  static_assert(W <= WIDE_LONG_GROUPS && W % 4 == 0, "a window gives every group of the block one entry");
  __shared__ u64 rows[2][WIDE_LONG_GROUPS];   // the row pointers of a window, in entry order
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4, c = threadIdx.x >> 6;
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, r, b, e);
  bool prune = false, any = false;   // (SAFE only) any: the row has a member
  if constexpr (SAFE) prune = (rg.flags & TFRA_RAGGED_PRUNE) && w;
  float wsum;
  if constexpr (SAFE) wsum = combiner == 0 ? 0.f : (prune ? comb_wsum_pruned(w, b, e, combiner) : comb_wsum(w, b, e, combiner));
  else wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  const float scale = comb_scale_of(wsum, combiner);
  const int col = c * 256 + lane * 4;
  const bool cok = col < dim;
  const unsigned coff = cok ? (unsigned)col * EB : 0u;   // this lane's byte offset inside a row
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (b < e) {
    const int last = e - 1;
    int buf = 0;
    i64 knext = ids[min(b + lane, last)];
    float wnext = w ? w[min(b + lane, last)] : 1.f;
    for (int p0 = b; p0 < e; p0 += BATCH) {
      const i64 kreg = knext;
      const float wreg = wnext;
      if (p0 + BATCH < e) {   // the next batch, in flight behind this batch's probes and rows
        const int pn = min(p0 + BATCH + lane, last);
        knext = ids[pn];
        wnext = w ? w[pn] : 1.f;
      }
      u64 hreg;
      const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
      const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
      const int nq = min(BATCH, e - p0);
      WideProbe pr;
      wide_issue(v, kreg, b0reg, b1reg, 4 * c, grp, sub, pr);
      for (int q = 0; q < nq; q += W) {
        const unsigned char* mine = wide_resolve(v, pr, sub, gshift, default_row);   // entry p0 + q + 4 c + grp
        if (sub == 0) rows[buf][4 * c + grp] = (u64)(uintptr_t)mine;
        __syncthreads();
        const u64 window = rows[buf][sub];   // lane u < W: the row of entry p0 + q + u
        buf ^= 1;
        Raw t[W];
        float x[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
          t[u] = *reinterpret_cast<const Raw*>(wave_ptr(window, u) + coff);   // W row loads in flight
          x[u] = wave_float(wreg, q + u);
        }
        if (q + W < nq) wide_issue(v, kreg, b0reg, b1reg, q + W + 4 * c, grp, sub, pr);   // the next window's key lines behind them
#pragma unroll
        for (int u = 0; u < W; u += 4) keep_live(t[u], t[u + 1], t[u + 2], t[u + 3]);
#pragma unroll
        for (int u = 0; u < W; ++u) {
          bool member = p0 + q + u < e;
          if constexpr (SAFE) {
            member = member && (!prune || x[u] > 0.f);
            any = any || member;
          }
          if (member && cok) comb_acc4(acc, PoolRow<DT>::widen(t[u]), x[u]);
        }
      }
    }
  }
  float* o = out + r * (size_t)dim + col;
  if constexpr (SAFE) {
    if ((rg.flags & TFRA_RAGGED_FILL) && !any) {   // every group of every wave probes fill_id and finds the same row
      u64 h;
      const unsigned f0 = (unsigned)bucket0(rg.fill_id, v.nb, h);
      const unsigned f1 = (unsigned)bucket1(h, f0, v.nb);
      const i64 word = probe_find_word(v, rg.fill_id, f0, f1, key_line(v, f0)[sub], sub, gshift);
      const unsigned char* src = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
      if (cok) *reinterpret_cast<float4*>(o) = PoolRow<DT>::widen(*reinterpret_cast<const Raw*>(src + coff));
      return;
    }
  }
  if (cok) *reinterpret_cast<float4*>(o) = comb_finish4(acc, wsum, scale, combiner);
}

// ---- the weight gradient: a 16-lane group per ENTRY -------------------------------------------------------------------------------
// The dot product's order is pinned to the 16-lane mapping (wgrad_dot4 over chunks of 64 columns ascending, then wgrad_reduce16), so
// the block is split over entries as wgrad_wide_row splits its wave: 256 threads, sixteen groups, a window of sixteen entries.
// Every group keeps its copy of grad_out[r, :] (NCH = 4 NCW float4 per lane), probes its entry — group k of wave c has entry
// 4 c + k of the window — and streams its row four chunks at a time through two buffers: wgrad_wide_row's inner loop, statement for
// statement.  The sixteen reduced d go to the double-buffered LDS array, and behind the barrier EVERY wave runs wgrad_s over the
// window in entry order, members only: s is the wave form's and the same in every wave, and so is what lane j keeps, the raw d of
// entry p0 + j.  No wave reads what another wave stored to global memory: wave 0 alone stores each batch (one coalesced store) and
// makes the mean / sqrtn second pass, lane j re-reading what lane j wrote, as the wave form does; the other waves are done at the
// last window.
template <int DT, int NCW, bool RAGGED, bool PRUNE>
__device__ __forceinline__ void wgrad_wide_long_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                    const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                    const unsigned char* __restrict__ default_row, const float* __restrict__ grad_out,
                                                    float* dw, size_t r, const RaggedArgs& rg) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;
  constexpr int NCH = 4 * NCW, W = WIDE_LONG_GROUPS;
  __shared__ float ds[2][W];   // the d of a window's entries, in entry order
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4, wave = threadIdx.x >> 6;
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, r, b, e);
  if (b >= e) return;   // (the whole block)
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
  int buf = 0;
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
    wide_issue(v, kreg, b0reg, b1reg, 4 * wave, grp, sub, pr);
    for (int q = 0; q < nq; q += W) {
      const unsigned char* src = wide_resolve(v, pr, sub, gshift, default_row);   // this group's entry: p0 + q + 4 wave + grp
      Raw t[2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = i * 64 + sub * 4;
        t[0][i] = *reinterpret_cast<const Raw*>(src + (col < dim ? (unsigned)col * EB : 0u));
      }
      if (q + W < nq) wide_issue(v, kreg, b0reg, b1reg, q + W + 4 * wave, grp, sub, pr);   // the next window's key lines behind the row's head
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
      if (sub == 0) ds[buf][4 * wave + grp] = d;
      __syncthreads();
      const float window = ds[buf][sub];   // lane u: the d of entry p0 + q + u
      buf ^= 1;
#pragma unroll
      for (int u = 0; u < W; ++u) {
        const float du = wave_float(window, u), xu = wave_float(wreg, q + u);
        bool member = p0 + q + u < e;
        if constexpr (PRUNE) member = member && xu > 0.f;
        if (member) wgrad_s(s, xu, du);
        if (lane == q + u) dmine = member ? du : 0.f;
      }
    }
    if (wave == 0 && p0 + lane < e) dw[p0 + lane] = dmine;   // one coalesced store per batch
  }
  if (combiner == 0 || wave != 0) return;
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
