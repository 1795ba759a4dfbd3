// The sparse segment combiner over a [U, dim] tensor of rows — the chain behind embedding_lookup_sparse
// (PY/dynamic_embedding_ops.py:120-293): forward, the gradient of the entries and the gradient of the weights — and the
// tfra::comb_* helpers (row bounds, per-entry records) that tfra_pool.hip, tfra_wgrad.hip and the grouped write-back call.
// The arithmetic is tfra_combine_device.h's.  Stream-ordered, no host sync, results deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_frontend.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_optim_device.h"

using namespace tfra;

namespace {

// ------------------------------------ sparse segment combiner -----------------------------------
__global__ void seg64_bounds_kernel(size_t n, const i64* __restrict__ seg, int* start_end, size_t n_rows) {
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  i64 s = seg[p];
  if (s < 0 || (size_t)s >= n_rows) return;
  if (p == 0 || seg[p - 1] != s) start_end[s] = (int)p;
  if (p == n - 1 || seg[p + 1] != s) start_end[n_rows + s] = (int)p + 1;
}

// one 16-lane group per output row; members in input order, 4 row loads in flight
template <bool VEC4>
__global__ __launch_bounds__(256) void seg_combine_kernel(size_t n_rows, int dim, const float* __restrict__ rows,
                                                          const int* __restrict__ idx, const float* __restrict__ w,
                                                          const int* __restrict__ start_end, int combiner,
                                                          float* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const size_t r = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  if (r >= n_rows) return;
  const int b = start_end[r], e = start_end[n_rows + r];
  const float wsum = comb_wsum(w, b, e, combiner);
  const float scale = comb_scale_of(wsum, combiner);
  float* o = out + r * (size_t)dim;
  if (VEC4) {
    for (int c = sub * 4; c < dim; c += 64) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int p = b; p < e; ++p) {
        const float x = w ? w[p] : 1.f;
        const float4 v = *reinterpret_cast<const float4*>(rows + (size_t)idx[p] * dim + c);
        comb_acc4(acc, v, x);
      }
      *reinterpret_cast<float4*>(o + c) = comb_finish4(acc, wsum, scale, combiner);
    }
  } else {
    for (int c = sub; c < dim; c += 16) {
      float acc = 0.f;
      for (int p = b; p < e; ++p) comb_acc(acc, rows[(size_t)idx[p] * dim + c], w ? w[p] : 1.f);
      o[c] = comb_finish(acc, wsum, scale, combiner);
    }
  }
}

// The gradient of seg_combine_kernel's WEIGHTS (tfra_combine_device.h: wgrad_*; the chain twin of wgrad_kernel, tfra_wgrad.hip):
// the same 16-lane group per output row and the same column-to-lane mapping — lane `sub` adds its products over the columns
// 64 c + 4 sub .. + 3, chunks ascending — then the group's reduction and s += w * d in entry order.  The lane (p - b) & 15 stores
// the raw d of entry p; for mean / sqrtn the group then walks its own [b, e) of dw again, lane j re-reading what lane j wrote.
template <bool VEC4>
__global__ __launch_bounds__(256) void seg_combine_wgrad_kernel(size_t n_rows, int dim, const float* __restrict__ rows,
                                                                const int* __restrict__ idx, const float* __restrict__ w,
                                                                const int* __restrict__ start_end, int combiner,
                                                                const float* __restrict__ grad_out, float* dw) {
  const int sub = threadIdx.x & 15;
  const size_t r = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  if (r >= n_rows) return;
  const int b = start_end[r], e = start_end[n_rows + r];
  if (b >= e) return;
  const float wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  const float* G = grad_out + r * (size_t)dim;
  float s = 0.f;
  for (int p = b; p < e; ++p) {
    const float x = w ? w[p] : 1.f;
    const float* row = rows + (size_t)idx[p] * dim;
    float d = 0.f;
    for (int c = sub * 4; c < dim; c += 64) {
      if (VEC4) {
        wgrad_dot4(d, *reinterpret_cast<const float4*>(G + c), *reinterpret_cast<const float4*>(row + c));
      } else {
        for (int k = c; k < c + 4 && k < dim; ++k) wgrad_dot1(d, G[k], row[k]);
      }
    }
    d = wgrad_reduce16(d);
    wgrad_s(s, x, d);
    if (sub == ((p - b) & 15)) dw[p] = d;
  }
  if (combiner == 0) return;
  for (int p = b + sub; p < e; p += 16) dw[p] = wgrad_finish(dw[p], w ? w[p] : 1.f, s, wsum, combiner);
}

// The same over a float16 / bfloat16 grad_out (tfra_sparse_segment_combine_backprop_weights_typed): the body above
// with GO32[r, c] = f32(grad_out[r, c]) * s formed at its load of G and nothing else changed — a second kernel and not a template
// axis of the first, whose name and code stay as they are.  VEC4: one 8-byte load per lane and chunk, up-cast by load_stored4 (the
// helpers GradHalf uses); otherwise element by element (load_stored), any dim and 2-byte aligned rows.  is_bf16 is a kernel
// argument (wave-uniform), *d_scale is read once per group at a uniform address; nullptr: 1.0f.
template <bool VEC4>
__global__ __launch_bounds__(256) void seg_combine_wgrad_half_kernel(size_t n_rows, int dim, const float* __restrict__ rows,
                                                                     const int* __restrict__ idx, const float* __restrict__ w,
                                                                     const int* __restrict__ start_end, int combiner,
                                                                     const unsigned short* __restrict__ grad_out, float* dw,
                                                                     const float* __restrict__ d_scale, int is_bf16) {
  const int sub = threadIdx.x & 15;
  const size_t r = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  if (r >= n_rows) return;
  const int b = start_end[r], e = start_end[n_rows + r];
  if (b >= e) return;
  const float wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  const float gs = d_scale ? *d_scale : 1.f;
  const unsigned short* G = grad_out + r * (size_t)dim;
  float s = 0.f;
  for (int p = b; p < e; ++p) {
    const float x = w ? w[p] : 1.f;
    const float* row = rows + (size_t)idx[p] * dim;
    float d = 0.f;
    for (int c = sub * 4; c < dim; c += 64) {
      if (VEC4) {
        const uint2 raw = *reinterpret_cast<const uint2*>(G + c);
        float4 g = is_bf16 ? load_stored4<TFRA_BF16>(raw) : load_stored4<TFRA_F16>(raw);
        g.x *= gs; g.y *= gs; g.z *= gs; g.w *= gs;
        wgrad_dot4(d, g, *reinterpret_cast<const float4*>(row + c));
      } else {
        for (int k = c; k < c + 4 && k < dim; ++k) {
          const float g = (is_bf16 ? bits_to_float<TFRA_BF16>(G[k]) : bits_to_float<TFRA_F16>(G[k])) * gs;
          wgrad_dot1(d, g, row[k]);
        }
      }
    }
    d = wgrad_reduce16(d);
    wgrad_s(s, x, d);
    if (sub == ((p - b) & 15)) dw[p] = d;
  }
  if (combiner == 0) return;
  for (int p = b + sub; p < e; p += 16) dw[p] = wgrad_finish(dw[p], w ? w[p] : 1.f, s, wsum, combiner);
}

// ------------------------------------ combiner backward (tfra_combine_device.h) -----------------
__global__ void comb_den_kernel(size_t n_rows, const int* __restrict__ start_end, const float* __restrict__ w, int combiner,
                                float* __restrict__ den) {
  comb_den_row((size_t)blockIdx.x * blockDim.x + threadIdx.x, n_rows, start_end, w, combiner, den);
}

__global__ void comb_ent_kernel(size_t nnz, const i64* __restrict__ seg, const float* __restrict__ w, const float* __restrict__ den,
                                size_t n_rows, CombEnt* __restrict__ ent) {
  comb_ent_one((size_t)blockIdx.x * blockDim.x + threadIdx.x, nnz, seg, w, den, n_rows, ent);
}

// the two over a list (tfra_multi_apply_planned_combined): descriptor d owns ceil(n_rows / 256) blocks of the first and
// ceil(nnz / 256) blocks of the second, and r / p count ITS rows / entries
__global__ __launch_bounds__(256) void comb_den_many_kernel(const CombManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                            unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const CombManyRec rec = recs[d];
  comb_den_row((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x, rec.n_rows, rec.se, rec.w, rec.combiner, rec.den);
}

__global__ __launch_bounds__(256) void comb_ent_many_kernel(const CombManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                            unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const CombManyRec rec = recs[d];
  comb_ent_one((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x, rec.nnz, rec.seg, rec.w, rec.den, rec.n_rows, rec.ent);
}

// entry_grads[e, :] = comb_grad(grad_out[row_e, :], den_e, w_e); VEC4: one float4 per thread
template <bool VEC4>
__global__ __launch_bounds__(256) void comb_backprop_kernel(size_t nnz, int dim, const float* __restrict__ g,
                                                            const CombEnt* __restrict__ ent, float* __restrict__ out) {
  const size_t per = VEC4 ? (size_t)(dim / 4) : (size_t)dim;
  const size_t total = nnz * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i / per, c = i - e * per;
    const CombEnt ce = ent[e];
    if (VEC4) {
      const float4 x = *reinterpret_cast<const float4*>(g + (size_t)ce.row * dim + c * 4);
      *reinterpret_cast<float4*>(out + e * dim + c * 4) = comb_grad4(x, ce.den, ce.w);
    } else {
      out[e * dim + c] = comb_grad(g[(size_t)ce.row * dim + c], ce.den, ce.w);
    }
  }
}

// the head the forward and the weight gradient share: the rows' bounds in the workspace, one 16-lane group per output row
int comb_rows_head(tfra_workspace* ws, hipStream_t s, size_t nnz, const int64_t* seg, size_t n_rows, int*& se, dim3& grid) {
  int rc = carve(ws, s, [&](Carver& c) { se = c.take<int>(2 * n_rows); });
  if (rc) return rc;
  grid = dim3((unsigned)((n_rows * 16 + 255) / 256));
  return comb_bounds(s, nnz, seg, n_rows, se);
}

}  // namespace

extern "C" {

int tfra_sparse_segment_combine(tfra_workspace_t* ws, size_t nnz, int dim, const float* rows, const int32_t* idx,
                                const int64_t* seg, const float* weights, int combiner, size_t n_rows, float* out,
                                tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !out || dim <= 0 || combiner < 0 || combiner > 2) return set_error(TFRA_ERR_INVALID, "segment_combine: bad argument");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (n_rows == 0) return TFRA_OK;
  if (nnz && (!rows || !idx || !seg)) return set_error(TFRA_ERR_INVALID, "segment_combine: null buffer");
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return set_error(TFRA_ERR_INVALID, "segment_combine: too large");
  int* se;
  dim3 grid;
  int rc = comb_rows_head(ws, s, nnz, seg, n_rows, se, grid);
  if (rc) return rc;
  bool vec4 = dim % 4 == 0 && (((uintptr_t)rows | (uintptr_t)out) % 16 == 0);
  if (vec4) seg_combine_kernel<true><<<grid, 256, 0, s>>>(n_rows, dim, rows, idx, weights, se, combiner, out);
  else seg_combine_kernel<false><<<grid, 256, 0, s>>>(n_rows, dim, rows, idx, weights, se, combiner, out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_sparse_segment_combine_backprop(tfra_workspace_t* ws, size_t nnz, int dim, const float* grad_out, const int64_t* seg,
                                         const float* weights, int combiner, size_t n_rows, float* entry_grads_out,
                                         tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || dim <= 0 || combiner < 0 || combiner > 2) return set_error(TFRA_ERR_INVALID, "segment_combine_backprop: bad argument");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (nnz == 0) return TFRA_OK;
  if (!grad_out || !seg || !entry_grads_out) return set_error(TFRA_ERR_INVALID, "segment_combine_backprop: null buffer");
  if (n_rows == 0) return set_error(TFRA_ERR_INVALID, "segment_combine_backprop: entries but no rows");
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return set_error(TFRA_ERR_INVALID, "segment_combine_backprop: too large");
  if (((uintptr_t)seg & 7) || ((uintptr_t)weights & 3) || (((uintptr_t)grad_out | (uintptr_t)entry_grads_out) & 3))
    return set_error(TFRA_ERR_UNSUPPORTED, "segment_combine_backprop: misaligned buffer");
  int* se;
  float* den;
  CombEnt* ent;
  int rc = carve(ws, s, [&](Carver& c) {
    se = c.take<int>(2 * n_rows);
    den = c.take<float>(n_rows);
    ent = c.take<CombEnt>(nnz);
  });
  if (rc) return rc;
  rc = comb_entries(s, nnz, seg, weights, combiner, n_rows, se, den, ent);
  if (rc) return rc;
  const bool vec4 = dim % 4 == 0 && (((uintptr_t)grad_out | (uintptr_t)entry_grads_out) & 15) == 0;
  const size_t work = nnz * (size_t)(vec4 ? dim / 4 : dim);
  const unsigned grid = (unsigned)std::min<size_t>((work + 255) / 256, 8192);
  if (vec4) comb_backprop_kernel<true><<<grid, 256, 0, s>>>(nnz, dim, grad_out, ent, entry_grads_out);
  else comb_backprop_kernel<false><<<grid, 256, 0, s>>>(nnz, dim, grad_out, ent, entry_grads_out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

// tfra_sparse_segment_combine_backprop_weights (hg == nullptr) and its typed twin over a half grad_out (hg, checked by
// check_typed: not NULL, 8-byte aligned; grad_out is not read then): one function, `who` names the caller in the refusals
static int seg_combine_wgrad_impl(const std::string& who, tfra_workspace_t* ws, size_t nnz, int dim, const float* rows, const int32_t* idx,
                                  const float* grad_out, const tfra_grads* hg, const int64_t* seg, const float* weights, int combiner,
                                  size_t n_rows, float* dw_out, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || dim <= 0 || combiner < 0 || combiner > 2) return set_error(TFRA_ERR_INVALID, who + ": bad argument");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (nnz == 0) return TFRA_OK;
  if (!rows || !idx || !seg || !dw_out || (n_rows && !grad_out && !hg)) return set_error(TFRA_ERR_INVALID, who + ": null buffer");
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return set_error(TFRA_ERR_INVALID, who + ": too large");
  if (((uintptr_t)seg & 7) || (((uintptr_t)weights | (uintptr_t)idx | (uintptr_t)rows | (uintptr_t)grad_out | (uintptr_t)dw_out) & 3))
    return set_error(TFRA_ERR_UNSUPPORTED, who + ": misaligned buffer");
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries in no row: 0
  if (n_rows == 0) return TFRA_OK;
  int* se;
  dim3 grid;
  int rc = comb_rows_head(ws, s, nnz, seg, n_rows, se, grid);
  if (rc) return rc;
  if (hg) {   // the vector arm: rows as the twin wants them, the half matrix 8-byte aligned (check_typed) and dim % 4 == 0
    const unsigned short* g = (const unsigned short*)hg->grads;
    const int bf = hg->dtype == TFRA_BF16;
    if (dim % 4 == 0 && (uintptr_t)rows % 16 == 0)
      seg_combine_wgrad_half_kernel<true><<<grid, 256, 0, s>>>(n_rows, dim, rows, idx, weights, se, combiner, g, dw_out, hg->d_scale, bf);
    else
      seg_combine_wgrad_half_kernel<false><<<grid, 256, 0, s>>>(n_rows, dim, rows, idx, weights, se, combiner, g, dw_out, hg->d_scale, bf);
    HIP_TRY(hipGetLastError());
    return TFRA_OK;
  }
  const bool vec4 = dim % 4 == 0 && (((uintptr_t)rows | (uintptr_t)grad_out) % 16 == 0);
  if (vec4) seg_combine_wgrad_kernel<true><<<grid, 256, 0, s>>>(n_rows, dim, rows, idx, weights, se, combiner, grad_out, dw_out);
  else seg_combine_wgrad_kernel<false><<<grid, 256, 0, s>>>(n_rows, dim, rows, idx, weights, se, combiner, grad_out, dw_out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_sparse_segment_combine_backprop_weights(tfra_workspace_t* ws, size_t nnz, int dim, const float* rows, const int32_t* idx,
                                                 const float* grad_out, const int64_t* seg, const float* weights, int combiner,
                                                 size_t n_rows, float* dw_out, tfra_stream_t stream) {
  return seg_combine_wgrad_impl("segment_combine_backprop_weights", ws, nnz, dim, rows, idx, grad_out, nullptr, seg, weights, combiner,
                                n_rows, dw_out, stream);
}

int tfra_sparse_segment_combine_backprop_weights_typed(tfra_workspace_t* ws, size_t nnz, int dim, const float* rows, const int32_t* idx,
                                                       const tfra_grads* grad_out, const int64_t* seg, const float* weights,
                                                       int combiner, size_t n_rows, float* dw_out, tfra_stream_t stream) {
  bool forward;
  if (const Check c = check_typed(grad_out, &forward); c.code) return report("segment_combine_backprop_weights_typed: ", c);
  if (forward)
    return tfra_sparse_segment_combine_backprop_weights(ws, nnz, dim, rows, idx, (const float*)grad_out->grads, seg, weights, combiner,
                                                        n_rows, dw_out, stream);
  return seg_combine_wgrad_impl("segment_combine_backprop_weights_typed", ws, nnz, dim, rows, idx, nullptr, grad_out, seg, weights,
                                combiner, n_rows, dw_out, stream);
}

}  // extern "C"

namespace tfra {
int comb_bounds(hipStream_t s, size_t nnz, const int64_t* seg, size_t n_rows, int* se) {
  HIP_TRY(hipMemsetAsync(se, 0, 2 * n_rows * sizeof(int), s));  // empty rows: start = end = 0
  if (nnz) seg64_bounds_kernel<<<(unsigned)((nnz + 255) / 256), 256, 0, s>>>(nnz, (const i64*)seg, se, n_rows);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int comb_entries(hipStream_t s, size_t nnz, const int64_t* seg, const float* weights, int combiner, size_t n_rows, int* se,
                 float* den, CombEnt* ent) {
  int rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  comb_den_kernel<<<(unsigned)((n_rows + 255) / 256), 256, 0, s>>>(n_rows, se, weights, combiner, den);
  comb_ent_kernel<<<(unsigned)((nnz + 255) / 256), 256, 0, s>>>(nnz, (const i64*)seg, weights, den, n_rows, ent);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int comb_den_ent_many(hipStream_t s, unsigned den_grid, unsigned ent_grid, const CombManyRec* recs, const unsigned* den_prefix,
                      const unsigned* ent_prefix, unsigned n) {
  comb_den_many_kernel<<<den_grid, 256, 0, s>>>(recs, den_prefix, n);
  comb_ent_many_kernel<<<ent_grid, 256, 0, s>>>(recs, ent_prefix, n);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
}  // namespace tfra
