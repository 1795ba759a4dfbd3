// The backward of the sparse segment combiner of embedding_lookup_sparse (PY/dynamic_embedding_ops.py:218-291: gather,
// *= weights, segment_sum, then / sum w (mean) or / sqrt(sum w^2) (sqrtn)).  For entry e of row r = seg[e] with weight w_e
// (1 without weights) and incoming gradient G[r,:]:
//   g_e = (G[r] / den_r) * w_e,   den_r = 1 (sum) | sum_{seg = r} w (mean) | sqrt(sum_{seg = r} w^2) (sqrtn)
// in fp32 and in TF's order: the divide's gradient first, then the multiply's (G / 1 == G exactly, so sum needs no branch).
// A row whose weight sum is 0 gives g_e = 0, the forward's convention (seg_combine_kernel, tfra_combine.hip).
//
// Every kernel that forms g_e — tfra_sparse_segment_combine_backprop (written out) and the combined write-back of
// tfra_table_apply_planned_combined (formed in registers from grad_out, tfra_apply_device.h) — reads the same per-entry record and
// calls comb_grad4, so the two routes agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "tfra_device.h"

namespace tfra {

// one 16-B load per entry: the grad_out row, its denominator, the entry's weight
struct CombEnt {
  unsigned row;
  float den;
  float w;
  unsigned pad;
};

// kernel argument of the combined write-back: position e of the plan has gradient comb_grad4(grads[ent[e].row], ent[e].den, ent[e].w)
struct CombRows {
  const CombEnt* ent;
};

// the weight sum of a row's members [b, e) in input order: sum w (sum, mean) | sum w^2 (sqrtn).  ONE loop for the forward
// (seg_combine_kernel, find_combine_kernel) and the backward (comb_den)
__device__ __forceinline__ float comb_wsum(const float* __restrict__ w, int b, int e, int combiner) {
  float s = 0.f;
  for (int p = b; p < e; ++p) { const float x = w ? w[p] : 1.f; s += combiner == 2 ? x * x : x; }
  return s;
}

// comb_wsum over the members that safe_embedding_lookup_sparse keeps (PY/dynamic_embedding_ops.py:374-376, `_prune_invalid_weights`:
// weight > 0, so a NaN weight is no member), in input order: the sum comb_wsum gives for the compacted list, bit for bit.  w != NULL.
__device__ __forceinline__ float comb_wsum_pruned(const float* __restrict__ w, int b, int e, int combiner) {
  float s = 0.f;
  for (int p = b; p < e; ++p) { const float x = w[p]; if (x > 0.f) s += combiner == 2 ? x * x : x; }
  return s;
}

// den_r over the row's members [b, e)
__device__ __forceinline__ float comb_den(const float* __restrict__ w, int b, int e, int combiner) {
  if (combiner == 0) return 1.f;
  const float s = comb_wsum(w, b, e, combiner);
  return combiner == 2 ? sqrtf(s) : s;
}

// ---- the forward's two steps, shared by seg_combine_kernel (tfra_combine.hip: rows from a [U, dim] tensor) and find_combine_kernel
// (tfra_pool.hip: rows straight from the table), so that both compile the same expressions and agree bit for bit ------------------
// one member: acc += v * x
__device__ __forceinline__ void comb_acc(float& acc, float v, float x) { acc += v * x; }
__device__ __forceinline__ void comb_acc4(float4& acc, float4 v, float x) {
  comb_acc(acc.x, v.x, x); comb_acc(acc.y, v.y, x); comb_acc(acc.z, v.z, x); comb_acc(acc.w, v.w, x);
}
// the row's end: wsum = comb_wsum of the row; sum: acc as it is | mean: acc / wsum | sqrtn: acc / sqrt(wsum); 0 when wsum == 0
__device__ __forceinline__ float comb_scale_of(float wsum, int combiner) { return combiner == 2 ? sqrtf(wsum) : (combiner == 1 ? wsum : 1.f); }
__device__ __forceinline__ float comb_finish(float acc, float wsum, float scale, int combiner) {
  if (combiner == 0) return acc;
  return wsum != 0.f ? acc / scale : 0.f;
}
__device__ __forceinline__ float4 comb_finish4(float4 acc, float wsum, float scale, int combiner) {
  return make_float4(comb_finish(acc.x, wsum, scale, combiner), comb_finish(acc.y, wsum, scale, combiner),
                     comb_finish(acc.z, wsum, scale, combiner), comb_finish(acc.w, wsum, scale, combiner));
}

__device__ __forceinline__ float comb_grad(float g, float den, float w) { return den != 0.f ? (g / den) * w : 0.f; }

__device__ __forceinline__ float4 comb_grad4(float4 g, float den, float w) {
  return make_float4(comb_grad(g.x, den, w), comb_grad(g.y, den, w), comb_grad(g.z, den, w), comb_grad(g.w, den, w));
}

// ---- the gradient with respect to the WEIGHTS (sp_weights of embedding_lookup_sparse) ----------------------------------------------
// The forward is out = A / den with A = sum_p w_p x_p over the row's members and den = 1 (sum) | W = sum w (mean) | sqrt(S),
// S = sum w^2 (sqrtn).  With G = grad_out[r, :], d_p = sum_c G[c] x_p[c] and s = sum_p w_p d_p (members in entry order):
//   sum    dw_p = d_p
//   mean   dw_p = (d_p - s / W) / W
//   sqrtn  dw_p = (d_p - (s / S) * w_p) / sqrtf(S)
// W / S is the forward's comb_wsum / comb_wsum_pruned (the same loop); mean / sqrtn with W / S == 0 give 0 for every entry of the
// row; an entry that is no member (pruned by weight, or in no row) gets exactly 0 and enters neither s nor W / S.
// ONE evaluation order, for every kernel that forms dw (wgrad_*_kernel in tfra_wgrad.hip: rows straight from the table;
// seg_combine_wgrad_kernel in tfra_combine.hip: rows from a [U, dim] tensor), so that the routes agree bit for bit:
//   - lane `sub` of the row's 16-lane group holds the columns 64 c + 4 sub .. + 3 of chunk c (find_combine_row's mapping);
//   - it starts from d = 0 and adds its products G[col] * x[col] one by one, chunks ascending, components x, y, z, w inside a
//     chunk (wgrad_dot4 / wgrad_dot1); a column at or beyond dim adds nothing (the add is skipped, not fed a zero);
//   - the 16 partial sums are reduced by __shfl_xor with offsets 8, 4, 2, 1 (wgrad_reduce16: every lane ends with the same bits);
//   - s starts from 0 and adds w_p * d_p per member in entry order (wgrad_s).
// The library is built with -ffp-contract=off: every product is rounded before it is added.
__device__ __forceinline__ void wgrad_dot1(float& d, float g, float x) { d += g * x; }
__device__ __forceinline__ void wgrad_dot4(float& d, float4 g, float4 x) {
  wgrad_dot1(d, g.x, x.x); wgrad_dot1(d, g.y, x.y); wgrad_dot1(d, g.z, x.z); wgrad_dot1(d, g.w, x.w);
}
__device__ __forceinline__ float wgrad_reduce16(float d) {
  d += __shfl_xor(d, 8);
  d += __shfl_xor(d, 4);
  d += __shfl_xor(d, 2);
  d += __shfl_xor(d, 1);
  return d;
}
__device__ __forceinline__ void wgrad_s(float& s, float w, float d) { s += w * d; }
// a member's dw from its raw d_p, its weight, the row's s and wsum (= W | S)
__device__ __forceinline__ float wgrad_finish(float d, float w, float s, float wsum, int combiner) {
  if (combiner == 0) return d;
  if (!(wsum != 0.f)) return 0.f;
  if (combiner == 1) return (d - s / wsum) / wsum;
  return (d - (s / wsum) * w) / sqrtf(wsum);
}

// The bodies of comb_den_kernel / comb_ent_kernel (tfra_combine.hip), one function each with two callers: the single-table kernels
// and the grouped ones (comb_den_many_kernel / comb_ent_many_kernel), which find r / p inside THEIR descriptor
__device__ __forceinline__ void comb_den_row(size_t r, size_t n_rows, const int* __restrict__ start_end, const float* __restrict__ w,
                                             int combiner, float* __restrict__ den) {
  if (r < n_rows) den[r] = comb_den(w, start_end[r], start_end[n_rows + r], combiner);
}
__device__ __forceinline__ void comb_ent_one(size_t p, size_t nnz, const i64* __restrict__ seg, const float* __restrict__ w,
                                             const float* __restrict__ den, size_t n_rows, CombEnt* __restrict__ ent) {
  if (p >= nnz) return;
  const i64 s = seg[p];
  const bool ok = s >= 0 && (size_t)s < n_rows;
  ent[p] = CombEnt{ok ? (unsigned)s : 0u, ok ? den[s] : 0.f, w ? w[p] : 1.f, 0u};
}

// The per-entry records of one batch (tfra_combine.hip): ent[e] = {seg[e], den_{seg[e]}, w_e}; an entry whose row lies outside
// [0, n_rows) gets {0, 0, w} (gradient 0, as the forward ignores it).  seg ascending; se: scratch of 2 n_rows ints, den: of
// n_rows floats.  n_rows >= 1.
int comb_entries(hipStream_t s, size_t nnz, const int64_t* seg, const float* weights, int combiner, size_t n_rows, int* se,
                 float* den, CombEnt* ent);

// se[r] / se[n_rows + r] = first / one-past-last entry of row r (seg ascending; entries outside [0, n_rows) are in no row; a row
// without entries: 0, 0).  se: 2 n_rows ints.  A memset and one launch (tfra_combine.hip).
int comb_bounds(hipStream_t s, size_t nnz, const int64_t* seg, size_t n_rows, int* se);

}  // namespace tfra
