// The bodies of the pooled lookup and of its weight gradient for LONG rows (tfra_pool_long.hip): ONE 256-thread block
// per output row, where find_combine_row / wgrad_row (tfra_pool_device.h, tfra_wgrad_device.h) give a row to one 16-lane group.
// The twins walk a row's entries serially, U probes and U row reads at a time, which suits the 1 - 30 ids of a categorical
// feature; a history of a few hundred ids leaves 16 lanes waiting on one latency after the other.  The time does not go into the
// adds — it goes into the probes and the row reads, and those are independent per entry — so here the block's 16 groups probe and
// read DIFFERENT entries of the row at the same time, and only the adds stay serial: in entry order, with the twins' expressions
// (comb_acc, comb_wsum's statement, wgrad_dot4 / wgrad_reduce16 / wgrad_s / wgrad_finish, under -ffp-contract=off), so the results
// equal the twins' bit for bit.
//
// A row's entries [b, e) are taken in WINDOWS of W = 64 / NCH entries (64 for dim <= 64, 32 for dim <= 128, 16 above): group g of
// the block owns the U = W / 16 entries g U .. g U + U - 1 of a window.  For them it does what find_combine_row does for a U-batch:
// lane j < U loads id and weight of entry j and hashes it, the group takes key, home buckets and weight by shuffle, reads
// key_line(...)[sub] of all U entries before it inspects any, runs probe_find_word, and reads word_row_ptr / default_row for all U
// entries and all NCH chunks (lane `sub` holds columns 64 c + 4 sub .. + 3 of chunk c) before any is used.  Loads stay
// unconditional: an entry past the row's end is clamped to the row's last entry (probed and read again, a member of nothing), a
// column past dim to column 0.  The ids and weights of the NEXT window are loaded behind this window's key lines.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_pool.h"
#include "tfra_pool_device.h"

namespace tfra {
namespace {

// keep_live (tfra_device.h) for U = 1, 2 or 4 values: one empty asm that takes them all, so that every load of a batch is issued
// before the first is waited for
__device__ __forceinline__ void live1(i64& a) { asm volatile("" : "+v"(a)); }
__device__ __forceinline__ void live1(uint2& a) { asm volatile("" : "+v"(a.x), "+v"(a.y)); }
__device__ __forceinline__ void live1(float4& a) { asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w)); }
__device__ __forceinline__ void live2(i64& a, i64& b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void live2(uint2& a, uint2& b) { asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(b.x), "+v"(b.y)); }
__device__ __forceinline__ void live2(float4& a, float4& b) {
  asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w));
}
template <int U, class T>
__device__ __forceinline__ void live_n(T (&a)[U]) {
  static_assert(U == 1 || U == 2 || U == 4, "a window gives a group 1, 2 or 4 entries");
  if constexpr (U == 4) keep_live(a[0], a[1], a[2], a[3]);
  else if constexpr (U == 2) live2(a[0], a[1]);
  else live1(a[0]);
}

constexpr int LONG_THREADS = 256;     // 16 groups of 16 lanes
constexpr int LONG_SLAB_VEC = 1024;   // float4 per slab: W entries of 16 NCH float4 — 16 KiB whatever the class
constexpr int LONG_WMAX = 64;

// where row r's entries lie: find_combine_row's two sources, statement for statement
template <bool RAGGED>
__device__ __forceinline__ void long_bounds(size_t n_rows, const int* __restrict__ start_end, const RaggedArgs& rg, size_t r, int& b,
                                            int& e) {
  if constexpr (RAGGED) {
    const i64 lo_s = rg.row_splits[r], hi_s = rg.row_splits[r + 1];
    b = (int)min(max(lo_s, (i64)0), (i64)rg.nnz);
    e = (int)min(max(hi_s, (i64)b), (i64)rg.nnz);
  } else {
    b = start_end[r];
    e = start_end[n_rows + r];
  }
}

// this lane's id and weight of a window whose first entry is pw: lane j of group g holds entry pw + g U + (j mod U), clamped
template <int U>
__device__ __forceinline__ void long_window_ids(const i64* __restrict__ ids, const float* __restrict__ w, int pw, int last, int g,
                                                int sub, i64& k, float& x) {
  const int p = min(pw + g * U + (sub & (U - 1)), last);
  k = ids[p];
  x = w ? w[p] : 1.f;
}

// The group's U entries of one window, from the ids the lanes hold (kreg, wreg): their weights x[u] and their rows t[c][u], the
// loads of which are all issued when this returns and none waited for.
template <int DT, int NCH, int U>
__device__ __forceinline__ void long_window_rows(const TableView& v, i64 kreg, float wreg, const unsigned char* __restrict__ default_row,
                                                 const unsigned (&coff)[NCH], int sub, int gshift,
                                                 typename PoolRow<DT>::Raw (&t)[NCH][U], float (&x)[U]) {
  typedef typename PoolRow<DT>::Raw Raw;
  u64 hreg;
  const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
  const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
  i64 key[U], k0[U];
  unsigned b0[U], b1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = gshift + u;
    key[u] = shfl_i64(kreg, j);
    b0[u] = (unsigned)__shfl((int)b0reg, j);
    b1[u] = (unsigned)__shfl((int)b1reg, j);
    x[u] = __shfl(wreg, j);
    k0[u] = key_line(v, b0[u])[sub];   // U probes in flight
  }
  live_n<U>(k0);
  const unsigned char* src[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const i64 word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift);
    src[u] = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int u = 0; u < U; ++u) t[c][u] = *reinterpret_cast<const Raw*>(src[u] + coff[c]);   // NCH U row loads in flight
  }
}

// ---- the forward ------------------------------------------------------------------------------------------------------------------------
// A window's rows are up-cast (PoolRow<DT>::widen: exact) and parked in an LDS slab, [entry][64 NCH] floats, each entry's weight and
// member bit beside it.  Behind the barrier the threads t < dim / 4 — thread 16 c + sub owns the columns 64 c + 4 sub .. + 3,
// find_combine_row's mapping — walk the slab IN ENTRY ORDER and apply comb_acc4 to ONE register accumulator that lives across the
// windows, for the members only: positions below e, and under TFRA_RAGGED_PRUNE the weights > 0.  Thread 0 alone forms the weight
// sum as the weights pass, with comb_wsum's statement over the members (comb_wsum_pruned's under PRUNE: the same members).
// Two slabs: the loads of window k + 1 are issued BEFORE window k is summed and stored behind it, so one barrier per window
// suffices — slab (k + 1) & 1 was last read in iteration k - 1, which the barrier at its end closed.
// LDS per block: 2 x 16 KiB of slabs + 2 x 64 x (4 + 4) B of weights and member words + 8 B = 33 800 B: four blocks per CU.
// The row's end is find_combine_row's: comb_scale_of, comb_finish4; under TFRA_RAGGED_FILL a row without members is the row of
// fill_id (default_row on a miss), probed by group 0 and written as it is.
template <int DT, int NCH, bool RAGGED, bool SAFE>
__device__ __forceinline__ void find_combine_long_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                      const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                      const unsigned char* __restrict__ default_row, float* __restrict__ out,
                                                      size_t r, const RaggedArgs& rg) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  constexpr int W = 64 / NCH, U = W / 16, ROWV = 16 * NCH;   // entries per window and per group; float4 per slab entry
  static_assert(W * ROWV == LONG_SLAB_VEC && W <= LONG_WMAX, "a slab holds one window");
  __shared__ float4 slab[2][LONG_SLAB_VEC];
  __shared__ float wts[2][LONG_WMAX];
  __shared__ unsigned mem[2][LONG_WMAX];
  __shared__ float row_wsum;
  __shared__ unsigned row_any;
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15, gshift = lane & 48, g = tid >> 4;
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, r, b, e);
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
  const int n = e - b, last = e - 1, nwin = (n + W - 1) / W;
  const bool summer = tid * 4 < dim;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float wsum = 0.f;   // (thread 0)
  bool any = false;   // the row has a member
  Raw t[NCH][U];
  float x[U];
  i64 knext = 0;
  float wnext = 1.f;
  // park the group's entries of the window that starts at pw (rows in t, weights in x) in slab `buf`
  auto park = [&](int buf, int pw) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = g * U + u;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (cok[c]) slab[buf][i * ROWV + c * 16 + sub] = PoolRow<DT>::widen(t[c][u]);
      if (sub == 0) {
        bool member = pw + i < e;
        if constexpr (SAFE) member = member && (!prune || x[u] > 0.f);
        wts[buf][i] = x[u];
        mem[buf][i] = member ? 1u : 0u;
      }
    }
  };
  if (nwin > 0) {
    long_window_ids<U>(ids, w, b, last, g, sub, knext, wnext);
    const i64 kreg = knext;
    const float wreg = wnext;
    if (nwin > 1) long_window_ids<U>(ids, w, b + W, last, g, sub, knext, wnext);
    long_window_rows<DT, NCH, U>(v, kreg, wreg, default_row, coff, sub, gshift, t, x);
    park(0, b);
  }
  __syncthreads();
  for (int k = 0; k < nwin; ++k) {
    const bool more = k + 1 < nwin;   // (uniform in the block)
    if (more) {
      const i64 kreg = knext;
      const float wreg = wnext;
      if (k + 2 < nwin) long_window_ids<U>(ids, w, b + (k + 2) * W, last, g, sub, knext, wnext);
      long_window_rows<DT, NCH, U>(v, kreg, wreg, default_row, coff, sub, gshift, t, x);
    }
    if (summer) {
      const int buf = k & 1, cnt = min(W, n - k * W);
      for (int i = 0; i < cnt; ++i) {
        if (!mem[buf][i]) continue;   // (the same word for every thread)
        const float xi = wts[buf][i];
        comb_acc4(acc, slab[buf][i * ROWV + tid], xi);
        any = true;
        if (tid == 0 && combiner != 0) wsum += combiner == 2 ? xi * xi : xi;
      }
    }
    if (more) park((k + 1) & 1, b + (k + 1) * W);
    __syncthreads();
  }
  if (tid == 0) {
    row_wsum = wsum;
    row_any = any ? 1u : 0u;
  }
  __syncthreads();
  wsum = row_wsum;
  float* o = out + r * (size_t)dim;
  if constexpr (SAFE) {
    if ((rg.flags & TFRA_RAGGED_FILL) && !row_any) {
      if (tid >= 16) return;   // group 0 probes and copies
      u64 h;
      const unsigned f0 = (unsigned)bucket0(rg.fill_id, v.nb, h);
      const unsigned f1 = (unsigned)bucket1(h, f0, v.nb);
      const i64 word = probe_find_word(v, rg.fill_id, f0, f1, key_line(v, f0)[sub], sub, gshift);
      const unsigned char* src = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (cok[c]) *reinterpret_cast<float4*>(o + c * 64 + sub * 4) = PoolRow<DT>::widen(*reinterpret_cast<const Raw*>(src + coff[c]));
      return;
    }
  }
  const float scale = comb_scale_of(wsum, combiner);
  if (summer) *reinterpret_cast<float4*>(o + tid * 4) = comb_finish4(acc, wsum, scale, combiner);
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------------
// The same block per row and the same windows.  Every lane holds its columns of grad_out[r, :] (g[NCH], the 16 groups alike); a
// group forms d_p of its U entries in the ONE order of tfra_combine_device.h — d = 0, wgrad_dot4 over the chunks ascending (a
// column at or beyond dim adds nothing), wgrad_reduce16 — and its lane 0 parks the raw d_p and w_p: in LDS for the first
// LONG_PARK entries of the row, and for a longer row's rest d_p in dw_out itself (w_p is read again from w).
// mean / sqrtn: thread 0 then forms s (wgrad_s) and W / S (comb_wsum's statement) over the members in entry order, four parked
// entries per LDS read; all threads write dw_p = wgrad_finish(d_p, w_p, s, wsum), 0 for an entry that is no member (pruned by
// weight).  sum: dw_p = d_p, no second walk.  LDS per block: 2 x 8 KiB + 8 B.
constexpr int LONG_PARK = 2048;
template <int DT, int NCH, bool RAGGED, bool PRUNE>
__device__ __forceinline__ void wgrad_long_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                               const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                               const unsigned char* __restrict__ default_row, const float* __restrict__ grad_out,
                                               float* dw, size_t r, const RaggedArgs& rg) {
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;
  constexpr int W = 64 / NCH, U = W / 16;
  __shared__ float4 dpark[LONG_PARK / 4];
  __shared__ float4 wpark[LONG_PARK / 4];
  __shared__ float row_s, row_wsum;
  const int tid = threadIdx.x, lane = tid & 63, sub = lane & 15, gshift = lane & 48, g = tid >> 4;
  int b, e;
  long_bounds<RAGGED>(n_rows, start_end, rg, r, b, e);
  if (b >= e) return;   // (the whole block)
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
  const int n = e - b, last = e - 1, nwin = (n + W - 1) / W;
  float* dp = reinterpret_cast<float*>(dpark);
  float* wp = reinterpret_cast<float*>(wpark);
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
  if (combiner != 0) {
    if (tid == 0) {
      const int np = min(n, LONG_PARK);
      for (int i0 = 0; i0 < np; i0 += 4) {
        const float4 d4 = dpark[i0 >> 2], x4 = wpark[i0 >> 2];
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
      row_s = s;
      row_wsum = wsum;
    }
    __syncthreads();
    s = row_s;
    wsum = row_wsum;
  }
  for (int i = tid; i < n; i += LONG_THREADS) {
    const float xi = i < LONG_PARK ? wp[i] : (w ? w[b + i] : 1.f);
    const float d = i < LONG_PARK ? dp[i] : dw[b + i];
    bool member = true;
    if constexpr (PRUNE) member = xi > 0.f;
    dw[b + i] = member ? wgrad_finish(d, xi, s, wsum, combiner) : 0.f;
  }
}

}  // namespace
}  // namespace tfra
