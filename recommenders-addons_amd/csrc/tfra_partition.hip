// tfra_partition / tfra_partition_by_owner: default_partition_fn + dynamic_partition
// (PY/dynamic_embedding_variable.py:131-197) — a stable split of the keys by owner shard, the owner computed from the key
// or given by the caller.  Stream-ordered, the per-shard counts stay on the device, results deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_frontend.h"
#include "tfra_host.h"

using namespace tfra;

namespace {

// ------------------------------------ partition ------------------------------------------------
__device__ __forceinline__ int owner_of(i64 key, int num, int mode) {
  if (mode == 0) return (int)(key & 0x7fffffff) % num;
  if (mode == 1) { i64 m = key % num; return (int)(m < 0 ? m + num : m); }
  return (int)__umul64hi(fmix64((u64)key), (u64)num);
}

// pass 1: per-tile (256 ids) histogram -> hist[tile][shard]
__global__ __launch_bounds__(256) void part_hist_kernel(size_t n, const i64* __restrict__ d_n, const i64* __restrict__ keys,
                                                        const int* __restrict__ owner, int num, int mode, int* hist) {
  extern __shared__ int cnt[];
  if (d_n) n = (size_t)min((i64)n, max(*d_n, (i64)0));
  for (int s = threadIdx.x; s < num; s += 256) cnt[s] = 0;
  __syncthreads();
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    // caller-computed partitions outside [0, num) are DISCARDED, like the reference's GPU DynamicPartition
    // (T/dynamic_partition_op_test.py:221-283; its CPU kernel raises instead)
    const int o = owner ? owner[i] : owner_of(keys[i], num, mode);
    if ((unsigned)o < (unsigned)num) atomicAdd(&cnt[o], 1);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < num; s += 256) hist[(size_t)blockIdx.x * num + s] = cnt[s];
}

// pass 2 (single block): shard-major exclusive scan over (shard, tile); totals -> d_counts
__global__ __launch_bounds__(1024) void part_scan_kernel(int* hist, size_t tiles, int num, i64* d_counts) {
  __shared__ int sh[1024];
  __shared__ long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int s = 0; s < num; ++s) {
    long long start = carry;
    __syncthreads();
    for (size_t base = 0; base < tiles; base += 1024) {
      size_t tix = base + threadIdx.x;
      int v = tix < tiles ? hist[tix * num + s] : 0;
      sh[threadIdx.x] = v;
      __syncthreads();
      for (int o = 1; o < 1024; o <<= 1) {
        int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
      }
      int incl = sh[threadIdx.x];
      if (tix < tiles) hist[tix * num + s] = (int)(carry + incl - v);
      __syncthreads();
      if (threadIdx.x == 1023) carry += incl;
      __syncthreads();
    }
    if (threadIdx.x == 0) d_counts[s] = carry - start;
    __syncthreads();
  }
}

// pass 3: stable scatter.  Rank inside the tile = (same-owner ids in earlier waves) + (same-owner
// ids in lower lanes of this wave), found with a ballot per distinct owner present in the wave.
__global__ __launch_bounds__(256) void part_scatter_kernel(size_t n, const i64* __restrict__ d_n, const i64* __restrict__ keys,
                                                           const int* __restrict__ owner, int num, int mode,
                                                           const int* __restrict__ hist, i64* keys_out, int* perm_out) {
  extern __shared__ int wcnt[];  // [4][num]
  if (d_n) n = (size_t)min((i64)n, max(*d_n, (i64)0));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int s = threadIdx.x; s < 4 * num; s += 256) wcnt[s] = 0;
  __syncthreads();
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = i < n;
  i64 key = (ok && keys) ? keys[i] : 0;
  int own = ok ? (owner ? owner[i] : owner_of(key, num, mode)) : -1;
  if ((unsigned)own >= (unsigned)num) own = -1;  // out of range: discarded
  ok = own >= 0;
  int rank = 0;
  u64 todo = __ballot(ok);
  while (todo) {
    int leader = __ffsll((unsigned long long)todo) - 1;
    int o = __shfl(own, leader);
    u64 m = __ballot(own == o);
    if (own == o) rank = __popcll(m & ((1ULL << lane) - 1));
    if (lane == leader) wcnt[w * num + o] = __popcll(m);
    todo &= ~m;
  }
  __syncthreads();
  if (ok) {
    int before = 0;
    for (int k = 0; k < w; ++k) before += wcnt[k * num + own];
    size_t pos = (size_t)hist[(size_t)blockIdx.x * num + own] + before + rank;
    if (keys_out) keys_out[pos] = key;
    perm_out[pos] = (int)i;
  }
}

// the frame behind both entry points (arguments checked, n > 0): histogram per tile of 256, shard-major scan, stable scatter
int launch_partition(tfra_workspace* ws, hipStream_t s, size_t n, const i64* d_n, const i64* keys, const int* owner, int num_shards,
                     int mode, i64* keys_out, int* perm_out, i64* d_counts) {
  const size_t tiles = (n + 255) / 256;
  int* hist;
  int rc = carve(ws, s, [&](Carver& c) { hist = c.take<int>(tiles * num_shards); });
  if (rc) return rc;
  part_hist_kernel<<<(unsigned)tiles, 256, num_shards * sizeof(int), s>>>(n, d_n, keys, owner, num_shards, mode, hist);
  part_scan_kernel<<<1, 1024, 0, s>>>(hist, tiles, num_shards, d_counts);
  part_scatter_kernel<<<(unsigned)tiles, 256, 4 * num_shards * sizeof(int), s>>>(n, d_n, keys, owner, num_shards, mode, hist, keys_out,
                                                                                  perm_out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

}  // namespace

extern "C" {

int tfra_partition(tfra_workspace_t* ws, size_t n, const int64_t* d_n, const int64_t* keys, int num_shards, int mode,
                   int64_t* keys_out, int32_t* perm_out, int64_t* d_counts, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !d_counts || num_shards <= 0 || num_shards > 2048 || mode < 0 || mode > 2)
    return set_error(TFRA_ERR_INVALID, "partition: bad argument (1 <= num_shards <= 2048, mode in 0..2)");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (n == 0) { HIP_TRY(hipMemsetAsync(d_counts, 0, num_shards * sizeof(int64_t), s)); return TFRA_OK; }
  if (!keys || !keys_out || !perm_out) return set_error(TFRA_ERR_INVALID, "partition: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "partition: too many keys");
  return launch_partition(ws, s, n, (const i64*)d_n, (const i64*)keys, nullptr, num_shards, mode, (i64*)keys_out, perm_out, (i64*)d_counts);
}

int tfra_partition_by_owner(tfra_workspace_t* ws, size_t n, const int32_t* owner, int num_shards, int32_t* perm_out,
                            int64_t* d_counts, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !d_counts || num_shards <= 0 || num_shards > 2048)
    return set_error(TFRA_ERR_INVALID, "partition_by_owner: bad argument (1 <= num_shards <= 2048)");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (n == 0) { HIP_TRY(hipMemsetAsync(d_counts, 0, num_shards * sizeof(int64_t), s)); return TFRA_OK; }
  if (!owner || !perm_out) return set_error(TFRA_ERR_INVALID, "partition_by_owner: null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, "partition_by_owner: too many keys");
  return launch_partition(ws, s, n, nullptr, nullptr, owner, num_shards, 0, nullptr, perm_out, (i64*)d_counts);
}

}  // extern "C"
