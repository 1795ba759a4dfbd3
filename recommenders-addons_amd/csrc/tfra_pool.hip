// Pooled lookup: the forward of embedding_lookup_sparse / safe_embedding_lookup_sparse straight from the table
// (tfra_table_find_combine).  The reference runs it as an op chain (PY/dynamic_embedding_ops.py:120-293):
//   tf.unique(ids)                                  :218-221   (a [U] tensor, idx[nnz], a host-visible count)
//   embedding_lookup(params, unique ids)            :223-231   (a [U, dim] tensor)
//   gather(idx) * weights, segment_sum, / sum w | / sqrt(sum w^2)   :233-291   (a [nnz, dim] tensor between them)
// A read needs no de-duplication (repeats of a hot id hit the cache), so here one 16-lane group per OUTPUT ROW walks the row's
// entries in input order, probes the table once per entry and accumulates w * row in registers: neither tensor exists and
// nothing is counted on the host.  The arithmetic is tfra_combine_device.h's, the code seg_combine_kernel (tfra_frontend.hip)
// compiles, in the same order, so the result equals tfra_table_find + tfra_sparse_segment_combine bit for bit.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"

using namespace tfra;

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return set_error(_e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP,                \
                       std::string(#expr) + ": " + hipGetErrorString(_e));                    \
  } while (0)

namespace {

// four elements of a row as float32: a 16-B load of a float32 row, an 8-B load of a half row up-cast exactly
template <int DT> struct PoolRow;
template <> struct PoolRow<TFRA_F32> {
  typedef float4 Raw;
  static __device__ __forceinline__ float4 widen(float4 x) { return x; }
};
template <> struct PoolRow<TFRA_F16> {
  typedef uint2 Raw;
  static __device__ __forceinline__ float h(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ float4 widen(uint2 x) {
    return make_float4(h((unsigned short)x.x), h((unsigned short)(x.x >> 16)), h((unsigned short)x.y), h((unsigned short)(x.y >> 16)));
  }
};
template <> struct PoolRow<TFRA_BF16> {
  typedef uint2 Raw;
  static __device__ __forceinline__ float4 widen(uint2 x) {
    return make_float4(bf16_to_f32((unsigned short)x.x), bf16_to_f32((unsigned short)(x.x >> 16)), bf16_to_f32((unsigned short)x.y),
                       bf16_to_f32((unsigned short)(x.y >> 16)));
  }
};

// One 16-lane group per output row (find_wave's and seg_combine_kernel's mapping: 4 rows per wave64).  The row's entries [b, e)
// are taken 16 at a time — lane j of the group loads id and weight of entry p0 + j and hashes it, one instruction stream for 16
// keys, the next 16 loading while these are worked on — and of those U at a time: U key lines in flight before any is inspected,
// then the U rows (NCH column chunks of 64 floats each: lane `sub` holds columns 64 c + 4 sub .. + 3) before any is accumulated.
// Accumulation is strictly in entry order.  Loads stay unconditional, as in find_wave: entries past the row's end are clamped to
// its last entry (probed and read again, not accumulated), columns past dim to column 0.
// The probe is find_kernel's (probe_find_word: plain loads), so a lookup that runs beside a write-back sees what tfra_table_find sees.
template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void find_combine_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                           const float* __restrict__ w, const int* __restrict__ start_end,
                                                           int combiner, const unsigned char* __restrict__ default_row,
                                                           float* __restrict__ out) {
  static_assert(U == 4, "keep_live is written for U == 4");
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t r = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  if (r >= n_rows) return;
  const int b = start_end[r], e = start_end[n_rows + r];
  const float wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
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
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const i64 word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift);
          src[u] = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
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
          if (p0 + q + u < e) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) comb_acc4(acc[c], PoolRow<DT>::widen(t[c][u]), x[u]);
          }
        }
      }
    }
  }
  float* o = out + r * (size_t)dim;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (cok[c]) *reinterpret_cast<float4*>(o + c * 64 + sub * 4) = comb_finish4(acc[c], wsum, scale, combiner);
}

template <int DT>
void launch_find_combine(hipStream_t s, const TableView& v, size_t n_rows, int dim, const i64* ids, const float* w, const int* se,
                         int combiner, const unsigned char* d, float* out) {
  constexpr int U = 4;
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  if (dim <= 64) find_combine_kernel<DT, U, 1><<<grid, 256, 0, s>>>(v, n_rows, dim, ids, w, se, combiner, d, out);
  else if (dim <= 128) find_combine_kernel<DT, U, 2><<<grid, 256, 0, s>>>(v, n_rows, dim, ids, w, se, combiner, d, out);
  else find_combine_kernel<DT, U, 4><<<grid, 256, 0, s>>>(v, n_rows, dim, ids, w, se, combiner, d, out);
}

}  // namespace

extern "C" int tfra_table_find_combine(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                       const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                       tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "find_combine: null table");
  if (!ws || combiner < 0 || combiner > 2) return set_error(TFRA_ERR_INVALID, "find_combine: bad argument");
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(t->mu);
  int rc = t->enter(s);
  if (rc) return rc;
  if (ws->device != t->device) return set_error(TFRA_ERR_INVALID, "find_combine: workspace and table live on different devices");
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: value_dtype must be float32, float16 or bfloat16");
  if (dim % 4 != 0 || dim > 256)
    return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: needs dim % 4 == 0 and dim <= 256 (use tfra_unique + tfra_table_find + "
                                           "tfra_sparse_segment_combine otherwise)");
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: too large (nnz < 2^31, n_rows < 2^30)");
  if ((((uintptr_t)out | (uintptr_t)default_row) & 15) || ((uintptr_t)ids & 7) || ((uintptr_t)seg & 7) || ((uintptr_t)weights & 3))
    return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: misaligned buffer (out and default_row: 16 bytes)");
  if (n_rows == 0) return TFRA_OK;
  if (!out) return set_error(TFRA_ERR_INVALID, "find_combine: null out");
  if (nnz == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * sizeof(float), s));
    return TFRA_OK;
  }
  if (!ids || !seg || !default_row) return set_error(TFRA_ERR_INVALID, "find_combine: null buffer");
  rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  const TableView v = t->view_of(t->cur);
  const i64* k = (const i64*)ids;
  const unsigned char* d = (const unsigned char*)default_row;
  if (dt == TFRA_F32) launch_find_combine<TFRA_F32>(s, v, n_rows, dim, k, weights, se, combiner, d, out);
  else if (dt == TFRA_F16) launch_find_combine<TFRA_F16>(s, v, n_rows, dim, k, weights, se, combiner, d, out);
  else launch_find_combine<TFRA_BF16>(s, v, n_rows, dim, k, weights, se, combiner, d, out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
