// Front-end helpers that bracket the table ops in the reference, one unit per concern:
//   tfra_unique        tf.unique                      PY/dynamic_embedding_ops.py:99                    tfra_unique.hip
//   tfra_gather_rows   tf.gather(unique_rows, idx)    PY/dynamic_embedding_ops.py:111                   here
//   tfra_segment_sum   unsorted_segment_sum of grads  PY/dynamic_embedding_optimizer.py:177-190         tfra_sorted.hip
//   tfra_partition     default_partition_fn + dynamic_partition  PY/dynamic_embedding_variable.py:131-197  tfra_partition.hip
//   tfra_scatter_rows  dynamic_stitch                 PY/dynamic_embedding_variable.py:157-162          here
// and the sparse segment combiner in tfra_combine.hip.  This unit keeps the workspace's life, the int32 <-> int64 key
// conversion and the row gather / scatter.
// All stream-ordered, counts stay on the device (no host sync), results deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"

using namespace tfra;

namespace {

// ------------------------------------ int32 <-> int64 keys ------------------------------------
__global__ __launch_bounds__(256) void widen_keys_kernel(size_t n, const int* __restrict__ in, i64* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (i64)in[i];
}
__global__ __launch_bounds__(256) void narrow_keys_kernel(size_t n, const i64* __restrict__ in, int* __restrict__ out, i64* overflow) {
  unsigned bad = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const i64 k = in[i];
    out[i] = (int)k;
    bad += (i64)(int)k != k;
  }
  if (overflow && bad) atomicAdd(reinterpret_cast<unsigned long long*>(overflow), (unsigned long long)bad);
}

// ------------------------------------ row gather / scatter ------------------------------------
template <int G, bool SCATTER>
__global__ __launch_bounds__(256) void move_rows_kernel(size_t n, unsigned row_bytes, const unsigned char* __restrict__ in,
                                                        const int* __restrict__ idx, unsigned char* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const size_t i = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  if (i >= n) return;
  size_t j = (size_t)idx[i];
  const unsigned char* src = in + (SCATTER ? i : j) * (size_t)row_bytes;
  unsigned char* dst = out + (SCATTER ? j : i) * (size_t)row_bytes;
  copy_bytes16<G>(dst, src, row_bytes, sub);
}

// gather of 16-byte-granule rows with U rows of a 16-lane group in flight (the row -> position gather behind a lookup of de-duplicated
// ids moves B rows: one row per group was one dependent idx -> row -> store chain per group, 9-13 us for 131 072 rows of 256 B)
template <int U, bool NT = false>
__global__ __launch_bounds__(256) void gather_rows16_kernel(size_t n, unsigned row_bytes, const unsigned char* __restrict__ in,
                                                            const int* __restrict__ idx, unsigned char* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const size_t base = ((((size_t)blockIdx.x * 256) + threadIdx.x) >> 4) * U;
  if (base >= n) return;
  size_t j[U];
#pragma unroll
  for (int u = 0; u < U; ++u) j[u] = base + u < n ? (size_t)idx[base + u] : 0;
  for (unsigned off = (unsigned)sub * 16u; off < row_bytes; off += 256u) {
    uint4 t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = *reinterpret_cast<const uint4*>(in + j[u] * (size_t)row_bytes + off);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u < n) {
        if (NT) {
          typedef unsigned v4u __attribute__((ext_vector_type(4)));
          v4u x = {t[u].x, t[u].y, t[u].z, t[u].w};
          __builtin_nontemporal_store(x, reinterpret_cast<v4u*>(out + (base + u) * (size_t)row_bytes + off));
        }
        else *reinterpret_cast<uint4*>(out + (base + u) * (size_t)row_bytes + off) = t[u];
      }
  }
}

template <bool SCATTER>
int move_rows(size_t n, size_t row_bytes, const void* in, const int32_t* idx, void* out, hipStream_t s) {
  if (n == 0) return TFRA_OK;
  if (!in || !idx || !out) return set_error(TFRA_ERR_INVALID, "gather/scatter: null buffer");
  const int g = granule_of(row_bytes, in, out);
  dim3 grid((unsigned)((n * 16 + 255) / 256)), block(256);
  const unsigned char* i8 = (const unsigned char*)in;
  unsigned char* o8 = (unsigned char*)out;
  unsigned rb = (unsigned)row_bytes;
  if (!SCATTER && g == 16 && n >= 4096) {
    // non-temporal stores: the output (B rows: tens of MB) is not read again by this kernel and does not fit the caches — 9.8 -> 8.5 us for
    // 131 072 rows of 256 B (scripts/mb_gather.py; 8 rows in flight instead of 4: no change)
    gather_rows16_kernel<4, true><<<(unsigned)(((n + 3) / 4 * 16 + 255) / 256), block, 0, s>>>(n, rb, i8, idx, o8);
    HIP_TRY(hipGetLastError());
    return TFRA_OK;
  }
  with_granule(g, [&](auto G) { move_rows_kernel<G, SCATTER><<<grid, block, 0, s>>>(n, rb, i8, idx, o8); });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

}  // namespace

extern "C" {

int tfra_workspace_create(int device, tfra_workspace_t** out) {
  if (!out) return set_error(TFRA_ERR_INVALID, "null out");
  tfra_workspace* ws = new tfra_workspace();
  if (device < 0 && hipGetDevice(&device) != hipSuccess) { delete ws; return set_error(TFRA_ERR_HIP, "no HIP device"); }
  ws->device = device;
  *out = ws;
  return TFRA_OK;
}

int tfra_workspace_destroy(tfra_workspace_t* ws) {
  if (!ws) return TFRA_OK;
  (void)hipSetDevice(ws->device);
  if (ws->buf) { (void)hipDeviceSynchronize(); (void)hipFree(ws->buf); }
  if (ws->unq_buf) { (void)hipDeviceSynchronize(); (void)hipFree(ws->unq_buf); }
  if (ws->unq_ev) (void)hipEventDestroy(ws->unq_ev);
  if (ws->unqm_buf) { (void)hipDeviceSynchronize(); (void)hipFree(ws->unqm_buf); }
  if (ws->unqm_ev) (void)hipEventDestroy(ws->unqm_ev);
  if (ws->h_err) { (void)hipDeviceSynchronize(); (void)hipHostFree(ws->h_err); }
  tfra::destroy_workspace_plan(ws->plan);
  tfra::destroy_workspace_plan(ws->uplan);
  tfra::destroy_workspace_many(ws->many);
  delete ws;
  return TFRA_OK;
}

int tfra_keys_widen_i32(size_t n, const int32_t* keys_in, int64_t* keys_out, tfra_stream_t stream) {
  if (n == 0) return TFRA_OK;
  if (!keys_in || !keys_out) return set_error(TFRA_ERR_INVALID, "keys_widen_i32: null buffer");
  widen_keys_kernel<<<(unsigned)std::min<size_t>(4096, (n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n, keys_in, (i64*)keys_out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_keys_narrow_i32(size_t n, const int64_t* keys_in, int32_t* keys_out, int64_t* d_overflow, tfra_stream_t stream) {
  if (d_overflow) HIP_TRY(hipMemsetAsync(d_overflow, 0, sizeof(int64_t), (hipStream_t)stream));
  if (n == 0) return TFRA_OK;
  if (!keys_in || !keys_out) return set_error(TFRA_ERR_INVALID, "keys_narrow_i32: null buffer");
  narrow_keys_kernel<<<(unsigned)std::min<size_t>(4096, (n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n, (const i64*)keys_in, keys_out, (i64*)d_overflow);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_gather_rows(size_t n, size_t row_bytes, const void* rows, const int32_t* idx, void* out, tfra_stream_t stream) {
  return move_rows<false>(n, row_bytes, rows, idx, out, (hipStream_t)stream);
}

int tfra_scatter_rows(size_t n, size_t row_bytes, const void* in, const int32_t* perm, void* out, tfra_stream_t stream) {
  return move_rows<true>(n, row_bytes, in, perm, out, (hipStream_t)stream);
}

}  // extern "C"
