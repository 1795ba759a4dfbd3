// tfra_unique: tf.unique (PY/dynamic_embedding_ops.py:99) — the distinct ids in order of first occurrence and, per id, its
// index among them.  Two implementations over one open-addressing scratch set: three launches over two persistent,
// self-emptying sets up to 2^20 ids (unique_fast), six launches over the workspace's scratch above.  Stream-ordered, the
// count stays on the device, the result is deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_frontend.h"
#include "tfra_host.h"
#include "tfra_unique_device.h"

using namespace tfra;

namespace {

// ------------------------------------ unique --------------------------------------------------
__global__ void unq_fill_kernel(i64* hkeys, int* hfirst, size_t cap1) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap1; i += (size_t)gridDim.x * blockDim.x) {
    hkeys[i] = EMPTY_KEY;
    hfirst[i] = 0x7fffffff;
  }
}

// scratch open-addressing set: CAS the id in, remember the smallest input index per distinct id; a block's equal ids are grouped in
// LDS first (unq_group_in_block, tfra_unique_device.h)
__global__ __launch_bounds__(UNQ_INS) void unq_insert_kernel(size_t n, const i64* __restrict__ ids, i64* hkeys, int* hfirst,
                                                             int* slot_of, size_t cap) {
  __shared__ i64 l_id[UNQ_INS];
  __shared__ unsigned l_own[UNQ_LCAP];   // 0 = free, else (claiming thread + 1)
  __shared__ int l_first[UNQ_LCAP];      // smallest thread index of the group
  __shared__ int l_slot[UNQ_LCAP];       // the group's slot in the global set
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * UNQ_INS + t;
  const bool ok = i < n;
  const i64 id = ok ? ids[i] : 0;
  const unsigned h = unq_group_in_block(t, ok, id, l_id, l_own, l_first);
  if (ok && l_first[h] == t) {  // first position of its id in this block
    size_t s;
    if (id == EMPTY_KEY) {
      s = cap;  // side slot for the sentinel value itself
    } else {
      s = fmix64((u64)id) & (cap - 1);
      for (;;) {
        i64 cur = load_key_coherent(&hkeys[s]);
        if (cur == id) break;
        if (cur == EMPTY_KEY) {
          i64 old = (i64)atomicCAS((u64*)&hkeys[s], (u64)EMPTY_KEY, (u64)id);
          if (old == EMPTY_KEY || old == id) break;
        }
        s = (s + 1) & (cap - 1);
      }
    }
    atomicMin(&hfirst[s], (int)i);
    l_slot[h] = (int)s;
  }
  __syncthreads();
  if (ok) slot_of[i] = l_slot[h];
}

__device__ __forceinline__ int block_sum_256(int v, int* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(256) void unq_count_kernel(size_t n, const int* __restrict__ hfirst,
                                                        const int* __restrict__ slot_of, int* block_counts) {
  __shared__ int sh[4];
  size_t base = (size_t)blockIdx.x * UNQ_TILE + threadIdx.x * UNQ_ITEMS;
  int c = 0;
#pragma unroll
  for (int k = 0; k < UNQ_ITEMS; ++k) {
    size_t i = base + k;
    if (i < n) c += hfirst[slot_of[i]] == (int)i;
  }
  int t = block_sum_256(c, sh);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = t;
}

// single-block exclusive scan of per-tile counts (in place) + grand total
__global__ __launch_bounds__(1024) void scan_counts_kernel(int* counts, size_t m, i64* total_out) {
  __shared__ int sh[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (size_t base = 0; base < m; base += 1024) {
    size_t i = base + threadIdx.x;
    int v = i < m ? counts[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += add;
      __syncthreads();
    }
    int incl = sh[threadIdx.x];
    if (i < m) counts[i] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += incl;
    __syncthreads();
  }
  if (threadIdx.x == 0 && total_out) *total_out = carry;
}

__global__ __launch_bounds__(256) void unq_scatter_kernel(size_t n, const i64* __restrict__ ids,
                                                          const int* __restrict__ hfirst, const int* __restrict__ slot_of,
                                                          const int* __restrict__ block_off, i64* unique_out, int* hrank) {
  __shared__ int wsum[4];
  size_t base = (size_t)blockIdx.x * UNQ_TILE + threadIdx.x * UNQ_ITEMS;
  int flag[UNQ_ITEMS];
  const int excl = unq_flags_scan(n, base, hfirst, slot_of, flag, wsum);
  int pos = block_off[blockIdx.x] + excl;
#pragma unroll
  for (int k = 0; k < UNQ_ITEMS; ++k) {
    if (flag[k]) {
      size_t i = base + k;
      unique_out[pos] = ids[i];
      hrank[slot_of[i]] = pos;
      ++pos;
    }
  }
}

__global__ void unq_idx_kernel(size_t n, const int* __restrict__ slot_of, const int* __restrict__ hrank, int* idx_out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) idx_out[i] = hrank[slot_of[i]];
}

// ---- tfra_unique in three launches (n <= 2^20) ------------------------------------------------------------------
// The six launches above (fill, insert, count, scan, scatter, idx) cost 34 us for 131 072 ids, most of it launch latency.
//   unq2_insert   as unq_insert_kernel, into one of TWO persistent sets; the thread whose compare-and-swap installed a
//                 key appends its slot to the set's used list, and the slots the OTHER set used in the previous call are
//                 emptied on the way (no fill kernel);
//   unq2_scatter  per tile of 1024 ids: first-occurrence flags, tile count published with the call's generation, the
//                 tile's offset = sum of the earlier tiles' counts, read as they appear (decoupled look-back: tile j only
//                 waits for tiles < j, and the hardware dispatches the blocks of a grid in index order, so whatever a
//                 waiting tile needs is already resident or finished — this does NOT rely on the whole grid being
//                 co-resident, other streams may hold CUs), then the scatter of unq_scatter_kernel; the last tile writes the total;
//   unq_idx_kernel.
// (UnqSet: tfra_unique_device.h; here hkeys / hfirst / hrank are [cap + 1])
__global__ __launch_bounds__(UNQ_INS) void unq2_insert_kernel(size_t n, const i64* __restrict__ ids, UnqSet cur, UnqSet old, int* slot_of,
                                                              size_t cap) {
  __shared__ i64 l_id[UNQ_INS];
  __shared__ unsigned l_own[UNQ_LCAP];
  __shared__ int l_first[UNQ_LCAP];
  __shared__ int l_slot[UNQ_LCAP];
  __shared__ unsigned s_n, s_base;
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * UNQ_INS + t;
  const unsigned n_old = *old.nused;
  const bool ok = i < n;
  const i64 id = ok ? ids[i] : 0;
  const unsigned h = unq_group_in_block(t, ok, id, l_id, l_own, l_first, &s_n);
  bool mine = false;
  unsigned myslot = 0, myidx = 0;
  if (ok && l_first[h] == t) {  // first position of its id in this block
    size_t sl;
    if (id == EMPTY_KEY) {
      sl = cap;  // side slot for the sentinel value itself
      mine = atomicMin(&cur.hfirst[sl], (int)i) == 0x7fffffff;
    } else {
      sl = fmix64((u64)id) & (cap - 1);
      for (;;) {
        const i64 was = (i64)atomicCAS((u64*)&cur.hkeys[sl], (u64)EMPTY_KEY, (u64)id);
        if (was == EMPTY_KEY) { mine = true; break; }
        if (was == id) break;
        sl = (sl + 1) & (cap - 1);
      }
      atomicMin(&cur.hfirst[sl], (int)i);
    }
    l_slot[h] = (int)sl;
    myslot = (unsigned)sl;
    if (mine) myidx = atomicAdd(&s_n, 1u);
  }
  __syncthreads();
  if (ok) slot_of[i] = l_slot[h];
  if (t == 0) s_base = s_n ? atomicAdd(cur.nused, s_n) : 0u;
  __syncthreads();
  if (mine) cur.used[s_base + myidx] = myslot;
  // the other set: empty the slots its last call used
  for (size_t k = (size_t)blockIdx.x * UNQ_INS + t; k < n_old; k += (size_t)gridDim.x * UNQ_INS) {
    const unsigned sl = old.used[k];
    old.hkeys[sl] = EMPTY_KEY;
    old.hfirst[sl] = 0x7fffffff;
  }
}

__global__ __launch_bounds__(256) void unq2_scatter_kernel(size_t n, const i64* __restrict__ ids, UnqSet cur, UnqSet old,
                                                           const int* __restrict__ slot_of, unsigned long long* agg, unsigned gen,
                                                           i64* unique_out, i64* total_out) {
  __shared__ int wsum[4];
  __shared__ int s_off;
  const size_t base = (size_t)blockIdx.x * UNQ_TILE + threadIdx.x * UNQ_ITEMS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int flag[UNQ_ITEMS];
  const int excl = unq_flags_scan(n, base, cur.hfirst, slot_of, flag, wsum);
  const int tile_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (threadIdx.x == 0)   // publish this tile's count under the call's generation
    __hip_atomic_store(agg + blockIdx.x, ((unsigned long long)gen << 32) | (unsigned)tile_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // offset = counts of the earlier tiles, read as they appear (wave 0: 64 tiles per sweep)
  if (w == 0) {
    int sum = 0;
    for (unsigned j0 = 0; j0 < blockIdx.x; j0 += 64) {
      const unsigned j = j0 + (unsigned)lane;
      if (j < blockIdx.x) {
        unsigned long long v;
        do { v = __hip_atomic_load(agg + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((unsigned)(v >> 32) != gen);
        sum += (int)(unsigned)v;
      }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) s_off = sum;
  }
  __syncthreads();
  int pos = s_off + excl;
#pragma unroll
  for (int k = 0; k < UNQ_ITEMS; ++k) {
    if (flag[k]) {
      const size_t i = base + k;
      unique_out[pos] = ids[i];
      cur.hrank[slot_of[i]] = pos;
      ++pos;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    if (total_out) *total_out = (i64)(s_off + tile_total);
    *old.nused = 0;   // the other set is empty again (unq2_insert_kernel of this call emptied it): its next call counts from zero
  }
}

// the persistent buffer of unique_fast: [256 B: the two sets' nused] [set 0] [set 1] [slot_of: nmax ints] [agg: a word per tile];
// a set: hkeys | hfirst | hrank (cap + 1 each) | used (nmax)
struct UnqLayout {
  size_t hfirst, hrank, used, per, slot_of, agg, bytes;
  UnqLayout(size_t cap, size_t nmax) {
    hfirst = align_up((cap + 1) * 8);
    hrank = hfirst + align_up((cap + 1) * 4);
    used = hrank + align_up((cap + 1) * 4);
    per = used + align_up(nmax * 4);
    slot_of = 256 + 2 * per;
    agg = slot_of + align_up(nmax * 4);
    bytes = agg + align_up(((nmax + UNQ_TILE - 1) / UNQ_TILE) * 8);
  }
  UnqSet set_of(void* buf, unsigned p) const {
    unsigned char* w = (unsigned char*)buf + 256 + (size_t)p * per;
    return UnqSet{(i64*)w, (int*)(w + hfirst), (int*)(w + hrank), (unsigned*)(w + used), (unsigned*)buf + p};
  }
};

// tfra_unique for n <= 2^20 ids: three launches over two persistent, self-emptying sets (see unq2_insert_kernel)
int unique_fast(tfra_workspace* ws, size_t n, const i64* ids, i64* unique_out, int32_t* idx_out, i64* d_num_unique, hipStream_t s) {
  const size_t tiles = (n + UNQ_TILE - 1) / UNQ_TILE;
  if (ws->unq_nmax < n) {
    if (ws->unq_buf) {
      if (hipStreamSynchronize(s) != hipSuccess || hipFree(ws->unq_buf) != hipSuccess) return set_error(TFRA_ERR_HIP, "unique: free failed");
      ws->unq_buf = nullptr; ws->unq_nmax = 0;
    }
    const size_t nmax = std::max<size_t>(n, 4096);
    size_t cap = 1024;
    while (cap < 2 * nmax) cap <<= 1;
    const UnqLayout L(cap, nmax);
    hipError_t e = hipMalloc(&ws->unq_buf, L.bytes);
    if (e != hipSuccess) { ws->unq_buf = nullptr; return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, "unique: hipMalloc failed"); }
    HIP_TRY(hipMemsetAsync(ws->unq_buf, 0, L.bytes, s));
    ws->unq_cap = cap; ws->unq_nmax = nmax; ws->unq_parity = 1; ws->unq_gen = 0;
    for (unsigned p = 0; p < 2; ++p) {   // both sets start empty
      const UnqSet u = L.set_of(ws->unq_buf, p);
      unq_fill_kernel<<<(unsigned)std::min<size_t>(2048, (cap + 256) / 256), 256, 0, s>>>(u.hkeys, u.hfirst, cap + 1);
    }
  }
  // The two sets, their parity and generation are STATE of the workspace: calls must reach them in one order.  Same stream:
  // stream order.  Another stream than the last call's: wait for that call (the Python layer keeps one workspace per stream,
  // so this only triggers for callers of the C ABI that share a workspace across streams).
  if (ws->unq_stream_set && ws->unq_stream != s) {
    if (!ws->unq_ev) HIP_TRY(hipEventCreateWithFlags(&ws->unq_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ws->unq_ev, ws->unq_stream));
    HIP_TRY(hipStreamWaitEvent(s, ws->unq_ev, 0));
  }
  ws->unq_stream = s; ws->unq_stream_set = true;
  const size_t cap = ws->unq_cap;
  const UnqLayout L(cap, ws->unq_nmax);
  const unsigned p = ws->unq_parity ^ 1u;
  const UnqSet cur = L.set_of(ws->unq_buf, p), old = L.set_of(ws->unq_buf, p ^ 1u);
  int* slot_of = (int*)((unsigned char*)ws->unq_buf + L.slot_of);
  unsigned long long* agg = (unsigned long long*)((unsigned char*)ws->unq_buf + L.agg);
  if (++ws->unq_gen == 0) ws->unq_gen = 1;   // (tile counts of an earlier call carry another generation)
  unq2_insert_kernel<<<(unsigned)((n + UNQ_INS - 1) / UNQ_INS), UNQ_INS, 0, s>>>(n, ids, cur, old, slot_of, cap);
  unq2_scatter_kernel<<<(unsigned)tiles, 256, 0, s>>>(n, ids, cur, old, slot_of, agg, ws->unq_gen, unique_out, d_num_unique);
  unq_idx_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, slot_of, cur.hrank, idx_out);
  HIP_TRY(hipGetLastError());
  ws->unq_parity = p;
  return TFRA_OK;
}

}  // namespace

extern "C" int tfra_unique(tfra_workspace_t* ws, size_t n, const int64_t* ids, int64_t* unique_out, int32_t* idx_out,
                           int64_t* d_num_unique, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!ws || !d_num_unique) return set_error(TFRA_ERR_INVALID, "unique: null argument");
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));
  if (n == 0) { HIP_TRY(hipMemsetAsync(d_num_unique, 0, sizeof(int64_t), s)); return TFRA_OK; }
  if (!ids || !unique_out || !idx_out) return set_error(TFRA_ERR_INVALID, "unique: null buffer");
  if (n >= (1ULL << 30)) return set_error(TFRA_ERR_INVALID, "unique: more than 2^30 ids per call");
  if (n <= ((size_t)1 << 20)) return unique_fast(ws, n, (const i64*)ids, (i64*)unique_out, idx_out, (i64*)d_num_unique, s);
  size_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  const size_t tiles = (n + UNQ_TILE - 1) / UNQ_TILE;
  i64* hkeys;
  int *hfirst, *hrank, *slot_of, *bcnt;
  int rc = carve(ws, s, [&](Carver& c) {
    hkeys = c.take<i64>(cap + 1);
    hfirst = c.take<int>(cap + 1);
    hrank = c.take<int>(cap + 1);
    slot_of = c.take<int>(n);
    bcnt = c.take<int>(tiles);
  });
  if (rc) return rc;
  unq_fill_kernel<<<(unsigned)std::min<size_t>(2048, (cap + 256) / 256), 256, 0, s>>>(hkeys, hfirst, cap + 1);
  unq_insert_kernel<<<(unsigned)((n + UNQ_INS - 1) / UNQ_INS), UNQ_INS, 0, s>>>(n, (const i64*)ids, hkeys, hfirst, slot_of, cap);
  unq_count_kernel<<<(unsigned)tiles, 256, 0, s>>>(n, hfirst, slot_of, bcnt);
  scan_counts_kernel<<<1, 1024, 0, s>>>(bcnt, tiles, (i64*)d_num_unique);
  unq_scatter_kernel<<<(unsigned)tiles, 256, 0, s>>>(n, (const i64*)ids, hfirst, slot_of, bcnt, (i64*)unique_out, hrank);
  unq_idx_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, slot_of, hrank, idx_out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
