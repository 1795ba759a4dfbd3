// The bodies of the pooled lookup and of its weight gradient for MIXED row lengths (tfra_pool_mixed.hip): one
// 256-thread block owns 16 CONSECUTIVE output rows r0 .. r0 + 15.  A row shorter than long_from entries is walked by one 16-lane
// group, exactly as the twins walk it (find_combine_row, wgrad_row: called here, so the code is theirs); a row of long_from entries
// or more is done by the whole block, the way the long forms do it (tfra_pool_long_device.h: the 16 groups probe and read
// DIFFERENT entries of a window at the same time, and only the adds stay serial, in entry order).  A heavy-tailed sequence feature
// — most rows a handful of ids, a few of them hundreds — thus runs each population of rows in the shape that suits it, in one
// launch, where the twins leave one group walking a long row alone and the long forms idle 15 groups on a short one.
//
// The block's course:
//   1. classify   lane `sub` of EVERY group loads the bounds of row r0 + sub (long_bounds, the row index clamped to n_rows - 1 so
//                 that the load stays unconditional; a row at or past n_rows has length 0), and a ballot cut to the group's 16
//                 lanes gives the 16-bit mask of the rows with e - b >= long_from.  No LDS, no barrier.
//   2. short rows group g walks row r0 + g with the twin's function if its bit is clear (a row past n_rows returns there at once).
//   3. long rows  for each set bit, ascending, the whole block does that row; every thread of the block runs every iteration.
// THE MASK IS UNIFORM IN THE BLOCK BY CONSTRUCTION: all 16 groups load the same 16 pairs of bounds, from memory that nothing
// writes during the launch, and compare with the same long_from.  Every barrier below hangs on that: the loop over the mask's bits
// and each window loop inside it have the same trip counts in all four waves.  (The mask goes through readfirstlane, so that the
// compiler sees a wave-uniform loop as well.)  Keep it that way: nothing a lane alone knows may enter the mask or a trip count.
// Inside a long row no path leaves early — the long forms `return` on the FILL path and on an empty row, which is right for a block
// that owns one row and wrong here — and a barrier closes each long row, so that the next one finds LDS free.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_pool.h"
#include "tfra_pool_device.h"
#include "tfra_pool_long_device.h"
#include "tfra_wgrad_device.h"

namespace tfra {
namespace {

constexpr int MIXED_ROWS = 16;   // output rows per block: one per group

// Step 1: the mask of this block's long rows, the same value in every lane of the block.
template <bool RAGGED>
__device__ __forceinline__ unsigned mixed_long_mask(size_t n_rows, const int* __restrict__ start_end, const RaggedArgs& rg, size_t r0,
                                                    unsigned long_from, int sub, int gshift) {
  const size_t rr = r0 + (size_t)sub;
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, min(rr, n_rows - 1), b, e);   // (n_rows > 0: the host launches no block otherwise)
  const bool is_long = rr < n_rows && (unsigned)(e - b) >= long_from;
  const unsigned mask = (unsigned)(__ballot(is_long) >> gshift) & 0xffffu;
  return (unsigned)__builtin_amdgcn_readfirstlane((int)mask);
}

// ---- the forward ------------------------------------------------------------------------------------------------------------------------
// LDS of a block, shared by its long rows one after the other.  ONE slab of a window (16 KiB whatever the class), where the long
// form has two: 16 KiB + 512 B + 8 B = 16 904 B per block lets nine blocks share a CU's 160 KiB, more than the eight waves a SIMD
// can hold, so LDS is never what limits a batch of short rows that does not touch it — with the long form's 33 800 B it would be
// (four blocks per CU).  The price is a second barrier per window: park, barrier, sum, barrier.  The row loads of window k + 1
// are still issued before window k is summed and are parked behind it, so their latency hides behind the adds as before.
struct MixedSlab {
  float4 slab[LONG_SLAB_VEC];
  float wts[LONG_WMAX];
  unsigned mem[LONG_WMAX];
  float row_wsum;
  unsigned row_any;
};

// One long row r with the entries [b, e), e - b >= 1, by the whole block: find_combine_long_row's windows, parking, entry-order adds
// into one register accumulator per thread, thread 0's weight sum, group 0's FILL probe — with one slab and with every thread
// reaching every barrier.
template <int DT, int NCH, bool SAFE>
__device__ __forceinline__ void find_combine_mixed_long_row(const TableView& v, int dim, const i64* __restrict__ ids,
                                                            const float* __restrict__ w, int combiner,
                                                            const unsigned char* __restrict__ default_row, float* __restrict__ out,
                                                            size_t r, int b, int e, const RaggedArgs& rg, MixedSlab& L) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  constexpr int W = 64 / NCH, U = W / 16, ROWV = 16 * NCH;   // entries per window and per group; float4 per slab entry
  static_assert(W * ROWV == LONG_SLAB_VEC && W <= LONG_WMAX, "the slab holds one window");
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15, gshift = lane & 48, g = tid >> 4;
  bool prune = false;
  if constexpr (SAFE) prune = (rg.flags & TFRA_RAGGED_PRUNE) && w;
  unsigned coff[NCH];   // this lane's byte offset inside a row, per chunk
  bool cok[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 64 + sub * 4;
    cok[c] = col < dim;
    coff[c] = cok[c] ? (unsigned)col * EB : 0u;
  }
  const int n = e - b, last = e - 1, nwin = (n + W - 1) / W;   // (uniform in the block: b and e are)
  const bool summer = tid * 4 < dim;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float wsum = 0.f;   // (thread 0)
  bool any = false;   // the row has a member
  Raw t[NCH][U];
  float x[U];
  i64 knext;
  float wnext;
  long_window_ids<U>(ids, w, b, last, g, sub, knext, wnext);
  {
    const i64 kreg = knext;
    const float wreg = wnext;
    if (nwin > 1) long_window_ids<U>(ids, w, b + W, last, g, sub, knext, wnext);
    long_window_rows<DT, NCH, U>(v, kreg, wreg, default_row, coff, sub, gshift, t, x);
  }
  for (int k = 0; k < nwin; ++k) {
    // park the group's entries of window k (rows in t, weights in x): the slab is free, the barrier below the last sum closed it
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = g * U + u;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (cok[c]) L.slab[i * ROWV + c * 16 + sub] = PoolRow<DT>::widen(t[c][u]);
      if (sub == 0) {
        bool member = k * W + i < n;
        if constexpr (SAFE) member = member && (!prune || x[u] > 0.f);
        L.wts[i] = x[u];
        L.mem[i] = member ? 1u : 0u;
      }
    }
    __syncthreads();
    if (k + 1 < nwin) {   // (uniform in the block) the next window's rows, in flight behind this window's adds
      const i64 kreg = knext;
      const float wreg = wnext;
      if (k + 2 < nwin) long_window_ids<U>(ids, w, b + (k + 2) * W, last, g, sub, knext, wnext);
      long_window_rows<DT, NCH, U>(v, kreg, wreg, default_row, coff, sub, gshift, t, x);
    }
    if (summer) {
      const int cnt = min(W, n - k * W);
      for (int i = 0; i < cnt; ++i) {
        if (!L.mem[i]) continue;   // (the same word for every thread)
        const float xi = L.wts[i];
        comb_acc4(acc, L.slab[i * ROWV + tid], xi);
        any = true;
        if (tid == 0 && combiner != 0) wsum += combiner == 2 ? xi * xi : xi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    L.row_wsum = wsum;
    L.row_any = any ? 1u : 0u;
  }
  __syncthreads();
  wsum = L.row_wsum;
  float* o = out + r * (size_t)dim;
  bool filled = false;
  if constexpr (SAFE) filled = (rg.flags & TFRA_RAGGED_FILL) && !L.row_any;
  if (filled) {
    if (tid < 16) {   // group 0 probes and copies; the others wait at the barrier below
      u64 h;
      const unsigned f0 = (unsigned)bucket0(rg.fill_id, v.nb, h);
      const unsigned f1 = (unsigned)bucket1(h, f0, v.nb);
      const i64 word = probe_find_word(v, rg.fill_id, f0, f1, key_line(v, f0)[sub], sub, gshift);
      const unsigned char* src = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (cok[c]) *reinterpret_cast<float4*>(o + c * 64 + sub * 4) = PoolRow<DT>::widen(*reinterpret_cast<const Raw*>(src + coff[c]));
    }
  } else {
    const float scale = comb_scale_of(wsum, combiner);
    if (summer) *reinterpret_cast<float4*>(o + tid * 4) = comb_finish4(acc, wsum, scale, combiner);
  }
  __syncthreads();   // row_wsum and row_any are read: the block's next long row may write LDS
}

template <int DT, int NCH, bool RAGGED, bool SAFE>
__device__ __forceinline__ void find_combine_mixed_block(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                         const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                         const unsigned char* __restrict__ default_row, float* __restrict__ out,
                                                         unsigned long_from, const RaggedArgs& rg) {
  __shared__ MixedSlab L;
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15, gshift = lane & 48, g = tid >> 4;
  const size_t r0 = (size_t)blockIdx.x * MIXED_ROWS;
  unsigned mask = mixed_long_mask<RAGGED>(n_rows, start_end, rg, r0, long_from, sub, gshift);
  if (!((mask >> g) & 1u))
    find_combine_row<DT, 4, NCH, RAGGED, SAFE>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out, r0 + (size_t)g, rg);
  while (mask) {   // (uniform in the block)
    const int j = __ffs((int)mask) - 1;
    mask &= mask - 1;
    int b, e;
    long_bounds<RAGGED>(n_rows, start_end, rg, r0 + (size_t)j, b, e);   // (a set bit is a row below n_rows)
    find_combine_mixed_long_row<DT, NCH, SAFE>(v, dim, ids, w, combiner, default_row, out, r0 + (size_t)j, b, e, rg, L);
  }
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------------
// wgrad_long_row for one of a block's long rows: the groups form d_p of their entries in tfra_combine_device.h's one order and park
// d_p and w_p (the first LONG_PARK entries in LDS, a longer row's rest in dw_out), thread 0 forms s and the weight sum in entry
// order, all 256 threads write wgrad_finish.  LDS per block: 2 x 8 KiB + 8 B, as there: nine blocks per CU.
struct MixedPark {
  float4 dpark[LONG_PARK / 4];
  float4 wpark[LONG_PARK / 4];
  float row_s, row_wsum;
};

template <int DT, int NCH, bool PRUNE>
__device__ __forceinline__ void wgrad_mixed_long_row(const TableView& v, int dim, const i64* __restrict__ ids, const float* __restrict__ w,
                                                     int combiner, const unsigned char* __restrict__ default_row,
                                                     const float* __restrict__ grad_out, float* dw, size_t r, int b, int e, MixedPark& L) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;
  constexpr int W = 64 / NCH, U = W / 16;
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15, gshift = lane & 48, g = tid >> 4;
  unsigned coff[NCH];
  bool cok[NCH];
  float4 go[NCH];
  const float* G = grad_out + r * (size_t)dim;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 64 + sub * 4;
    cok[c] = col < dim;
    coff[c] = cok[c] ? (unsigned)col * EB : 0u;
    go[c] = *reinterpret_cast<const float4*>(G + (cok[c] ? col : 0));
  }
  const int n = e - b, last = e - 1, nwin = (n + W - 1) / W;   // (uniform in the block)
  float* dp = reinterpret_cast<float*>(L.dpark);
  float* wp = reinterpret_cast<float*>(L.wpark);
  i64 knext;
  float wnext;
  long_window_ids<U>(ids, w, b, last, g, sub, knext, wnext);
  for (int k = 0; k < nwin; ++k) {
    const i64 kreg = knext;
    const float wreg = wnext;
    if (k + 1 < nwin) long_window_ids<U>(ids, w, b + (k + 1) * W, last, g, sub, knext, wnext);
    Raw t[NCH][U];
    float x[U];
    long_window_rows<DT, NCH, U>(v, kreg, wreg, default_row, coff, sub, gshift, t, x);
#pragma unroll
    for (int c = 0; c < NCH; ++c) live_n<U>(t[c]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (cok[c]) wgrad_dot4(d, go[c], PoolRow<DT>::widen(t[c][u]));
      d = wgrad_reduce16(d);
      const int i = k * W + g * U + u;   // the entry's place in the row
      if (sub == 0 && i < n) {
        if (i < LONG_PARK) {
          dp[i] = d;
          wp[i] = x[u];
        } else {
          dw[b + i] = d;
        }
      }
    }
  }
  __syncthreads();
  float s = 0.f, wsum = 0.f;
  if (combiner != 0) {   // (uniform in the block: a kernel argument)
    if (tid == 0) {
      const int np = min(n, LONG_PARK);
      for (int i0 = 0; i0 < np; i0 += 4) {
        const float4 d4 = L.dpark[i0 >> 2], x4 = L.wpark[i0 >> 2];
        const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, xx[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bool member = i0 + j < np;
          if constexpr (PRUNE) member = member && xx[j] > 0.f;
          if (member) {
            wgrad_s(s, xx[j], dd[j]);
            wsum += combiner == 2 ? xx[j] * xx[j] : xx[j];
          }
        }
      }
      for (int i = LONG_PARK; i < n; ++i) {   // a row longer than the park: its rest from global memory
        const float xi = w ? w[b + i] : 1.f, d = dw[b + i];
        bool member = true;
        if constexpr (PRUNE) member = xi > 0.f;
        if (member) {
          wgrad_s(s, xi, d);
          wsum += combiner == 2 ? xi * xi : xi;
        }
      }
      L.row_s = s;
      L.row_wsum = wsum;
    }
    __syncthreads();
    s = L.row_s;
    wsum = L.row_wsum;
  }
  for (int i = tid; i < n; i += LONG_THREADS) {
    const float xi = i < LONG_PARK ? wp[i] : (w ? w[b + i] : 1.f);
    const float d = i < LONG_PARK ? dp[i] : dw[b + i];
    bool member = true;
    if constexpr (PRUNE) member = xi > 0.f;
    dw[b + i] = member ? wgrad_finish(d, xi, s, wsum, combiner) : 0.f;
  }
  __syncthreads();   // the park, row_s and row_wsum are read: the block's next long row may write LDS
}

template <int DT, int NCH, bool RAGGED, bool PRUNE>
__device__ __forceinline__ void wgrad_mixed_block(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                  const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                  const unsigned char* __restrict__ default_row, const float* __restrict__ grad_out,
                                                  float* dw, unsigned long_from, const RaggedArgs& rg) {
  __shared__ MixedPark L;
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15, gshift = lane & 48, g = tid >> 4;
  const size_t r0 = (size_t)blockIdx.x * MIXED_ROWS;
  unsigned mask = mixed_long_mask<RAGGED>(n_rows, start_end, rg, r0, long_from, sub, gshift);
  if (!((mask >> g) & 1u))
    wgrad_row<DT, 4, NCH, RAGGED, PRUNE>(v, n_rows, dim, ids, w, start_end, rg.row_splits, rg.nnz, combiner, default_row, grad_out, dw,
                                         r0 + (size_t)g);
  while (mask) {   // (uniform in the block)
    const int j = __ffs((int)mask) - 1;
    mask &= mask - 1;
    int b, e;
    long_bounds<RAGGED>(n_rows, start_end, rg, r0 + (size_t)j, b, e);   // (a set bit is a row below n_rows)
    wgrad_mixed_long_row<DT, NCH, PRUNE>(v, dim, ids, w, combiner, default_row, grad_out, dw, r0 + (size_t)j, b, e, L);
  }
}

}  // namespace
}  // namespace tfra
