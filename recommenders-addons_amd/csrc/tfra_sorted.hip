// The two front-end ops that sort (the only includer of rocprim among the front-end units):
//   tfra_segment_sum    unsorted_segment_sum of grads   PY/dynamic_embedding_optimizer.py:177-190
//   tfra_select_lowest  the k keys of lowest status, ties in input order
// Stream-ordered, counts stay on the device (no host sync), results deterministic.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_frontend.h"
#include "tfra_host.h"

using namespace tfra;

namespace {

// ------------------------------------ segment sum ---------------------------------------------
__global__ void iota_kernel(int* p, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (int)i;
}

__global__ void widen_i32_kernel(const int* __restrict__ in, i64* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}

// seg_sorted ascending (stable => member indices ascending inside a segment).  One 16-lane group
// per segment walks its members in index order: out[seg,:] = sum_i in[i,:], ONE fp32 add per
// element per member, i.e. exactly the order of a sequential CPU unsorted_segment_sum
// (bit-exact vs the oracle).

__global__ void seg_bounds_kernel(size_t n, const int* __restrict__ seg_sorted, int* seg_start, size_t max_segments) {
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  int s = seg_sorted[p];
  if ((size_t)s >= max_segments) return;
  if (p == 0 || seg_sorted[p - 1] != s) seg_start[s] = (int)p;
  if (p == n - 1 || seg_sorted[p + 1] != s) seg_start[max_segments + s] = (int)p + 1;  // end
}

template <bool VEC4>
__global__ __launch_bounds__(256) void seg_sum_kernel(size_t nseg_cap, const i64* __restrict__ d_nseg, int dim,
                                                      const float* __restrict__ in, const int* __restrict__ member,
                                                      const int* __restrict__ seg_start, float* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const size_t g = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  size_t nseg = (size_t)*d_nseg;
  if (nseg > nseg_cap) nseg = nseg_cap;
  if (g >= nseg) return;
  int b = seg_start[g], e = seg_start[nseg_cap + g];
  float* o = out + g * (size_t)dim;
  if (VEC4) {
    for (int c = sub * 4; c < dim; c += 64) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int p = b; p < e; ++p) {
        float4 x = *reinterpret_cast<const float4*>(in + (size_t)member[p] * dim + c);
        acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
      }
      *reinterpret_cast<float4*>(o + c) = acc;
    }
  } else {
    for (int c = sub; c < dim; c += 16) {
      float acc = 0.f;
      for (int p = b; p < e; ++p) acc += in[(size_t)member[p] * dim + c];
      o[c] = acc;
    }
  }
}

}  // namespace

extern "C" {

int tfra_segment_sum(tfra_workspace_t* ws, size_t n, int dim, const float* in, const int32_t* idx,
                     const int64_t* d_num_segments, size_t max_segments, float* out, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !d_num_segments || !out || dim <= 0) return set_error(TFRA_ERR_INVALID, "segment_sum: bad argument");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (max_segments == 0) return TFRA_OK;
  if (n == 0) { HIP_TRY(hipMemsetAsync(out, 0, max_segments * (size_t)dim * sizeof(float), s)); return TFRA_OK; }
  if (!in || !idx) return set_error(TFRA_ERR_INVALID, "segment_sum: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "segment_sum: too many rows");
  unsigned bits = 1;
  while ((1ULL << bits) < max_segments && bits < 32) ++bits;
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs((void*)nullptr, tmp_bytes, (const int*)idx, (int*)nullptr, (const int*)nullptr,
                                    (int*)nullptr, n, 0u, bits, s));
  int *iota, *seg_sorted, *member, *seg_start;
  void* tmp;
  int rc = carve(ws, s, [&](Carver& c) {
    iota = c.take<int>(n);
    seg_sorted = c.take<int>(n);
    member = c.take<int>(n);
    seg_start = c.take<int>(2 * max_segments);
    tmp = c.take<unsigned char>(tmp_bytes);
  });
  if (rc) return rc;
  iota_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(iota, n);
  HIP_TRY(hipMemsetAsync(seg_start, 0, 2 * max_segments * sizeof(int), s));  // empty segments: start=end=0
  HIP_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const int*)idx, seg_sorted, (const int*)iota, member, n, 0u, bits, s));
  seg_bounds_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, seg_sorted, seg_start, max_segments);
  dim3 grid((unsigned)((max_segments * 16 + 255) / 256));
  bool vec4 = (dim % 4 == 0) && (((uintptr_t)in | (uintptr_t)out) % 16 == 0);
  if (vec4) seg_sum_kernel<true><<<grid, 256, 0, s>>>(max_segments, (const i64*)d_num_segments, dim, in, member, seg_start, out);
  else seg_sum_kernel<false><<<grid, 256, 0, s>>>(max_segments, (const i64*)d_num_segments, dim, in, member, seg_start, out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_select_lowest(tfra_workspace_t* ws, size_t n, const int64_t* keys, const void* status, int status_dtype,
                       size_t k, int64_t* keys_out, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || (status_dtype != TFRA_I32 && status_dtype != TFRA_I64) || k > n)
    return set_error(TFRA_ERR_INVALID, "select_lowest: bad argument (status int32/int64, k <= n)");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (k == 0) return TFRA_OK;
  if (!keys || !status || !keys_out) return set_error(TFRA_ERR_INVALID, "select_lowest: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "select_lowest: too many keys");
  size_t tmp_bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs((void*)nullptr, tmp_bytes, (const i64*)nullptr, (i64*)nullptr, (const i64*)nullptr,
                                    (i64*)nullptr, n, 0u, 64u, s));
  i64 *wide, *st_sorted, *k_sorted;
  void* tmp;
  int rc = carve(ws, s, [&](Carver& c) {
    wide = c.take<i64>(n);
    st_sorted = c.take<i64>(n);
    k_sorted = c.take<i64>(n);
    tmp = c.take<unsigned char>(tmp_bytes);
  });
  if (rc) return rc;
  const i64* st = (const i64*)status;
  if (status_dtype == TFRA_I32) {
    widen_i32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((const int*)status, wide, n);
    st = wide;
  }
  // stable LSD radix sort, ascending, signed: equal statuses keep their input order
  HIP_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, st, st_sorted, (const i64*)keys, k_sorted, n, 0u, 64u, s));
  HIP_TRY(hipMemcpyAsync(keys_out, k_sorted, k * sizeof(i64), hipMemcpyDeviceToDevice, s));
  return TFRA_OK;
}

}  // extern "C"
