// Scans over a window of the table's slots (tfra_table.hip): export_batch, the score-filtered export_batch_if / erase_if
//  and the slot census.
#include <hip/hip_runtime.h>

#include "tfra_host.h"

using namespace tfra;

// introspection (tests, tools): counts of empty / locked / live key slots and of flagged buckets
__global__ void slot_census_kernel(TableView v, u64* out) {
  u64 e = 0, l = 0, live = 0, f0 = 0, f1 = 0;
  const size_t total = v.nb * 16;
  for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (size_t)gridDim.x * blockDim.x) {
    const i64 k = *key_word(v, w);
    if ((w & 15) == 15) { f0 += ((u64)k & META_OVF0) != 0; f1 += ((u64)k & META_OVF1) != 0; }
    else if (k == EMPTY_KEY) ++e;
    else if (k == LOCKED_KEY) ++l;
    else ++live;
  }
  if (e) atomicAdd(out + 0, e);
  if (l) atomicAdd(out + 1, l);
  if (live) atomicAdd(out + 2, live);
  if (f0) atomicAdd(out + 3, f0);
  if (f1) atomicAdd(out + 4, f1);
}

// ---- export_batch: slots [offset, offset+n) -> compact (key,row,score) at *counter ----------
// One block = 64 buckets; one returned atomic per block (not per wave) reserves the output run.
template <int G>
__global__ __launch_bounds__(256) void export_kernel(TableView v, u64 first_bucket, u64 last_bucket,
                                                     u64 lo, u64 hi, u64* counter, i64* __restrict__ keys_out,
                                                     unsigned char* __restrict__ vals_out,
                                                     u64* __restrict__ scores_out) {
  __shared__ unsigned cnt[64];
  __shared__ u64 base_s;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const int grp_in_block = threadIdx.x >> 4;  // 0..15
  i64 k[4];
  unsigned live[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    u64 b = first_bucket + (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    bool ok = b < last_bucket;
    k[it] = ok ? key_line(v, b)[sub] : EMPTY_KEY;
    u64 slot = b * SLOTS + sub;
    bool l = ok && sub < SLOTS && k[it] != EMPTY_KEY && k[it] != LOCKED_KEY && slot >= lo && slot < hi;
    live[it] = (unsigned)(__ballot(l) >> gshift) & 0x7fffu;
    if (sub == 0) cnt[it * 16 + grp_in_block] = __popc(live[it]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int i = 0; i < 64; ++i) { unsigned c = cnt[i]; cnt[i] = run; run += c; }
    base_s = run ? atomicAdd(counter, (u64)run) : 0;
  }
  __syncthreads();
  const u64 base = base_s;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    u64 b = first_bucket + (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    u64 pos0 = base + cnt[it * 16 + grp_in_block];
    unsigned m = live[it];
    if (m & (1u << sub)) {
      u64 pos = pos0 + __popc(m & ((1u << sub) - 1));
      keys_out[pos] = k[it];
      if (scores_out) scores_out[pos] = has_scores(v) ? score_line(v, b)[sub] : 0;
    }
    if (vals_out) {
      unsigned r = 0;
      while (m) {
        int s = __ffs(m) - 1;
        m &= m - 1;
        copy_bytes16<G>(vals_out + (pos0 + r) * (size_t)v.field_bytes,
                        row_at(v, b, (unsigned)s), v.field_bytes, sub);
        ++r;
      }
    }
  }
}

// the two side rows (keys INT64_MIN, INT64_MIN+1) are slots nb*15 and nb*15+1
__global__ void export_reserved_kernel(TableView v, u64 lo, u64 hi, u64* counter, i64* keys_out,
                                       unsigned char* vals_out, u64* scores_out) {
  for (int r = 0; r < NUM_RESERVED; ++r) {
    u64 slot = v.nb * SLOTS + r;
    if (slot < lo || slot >= hi || !v.reserved_present[r]) continue;
    __shared__ u64 pos_s;
    if (threadIdx.x == 0) pos_s = atomicAdd(counter, 1ULL);
    __syncthreads();
    u64 pos = pos_s;
    if (threadIdx.x == 0) { keys_out[pos] = EMPTY_KEY + r; if (scores_out) scores_out[pos] = ~0ULL; }
    if (vals_out)
      for (unsigned off = threadIdx.x; off < v.field_bytes; off += blockDim.x)
        vals_out[pos * (size_t)v.field_bytes + off] = row_ptr(v, (i64)slot)[off];
    __syncthreads();
  }
}

// ---- score-filtered scans: export_if / erase_if ----------------------------
// pred: tfra_score_pred (uniform: a scalar select).  The side rows count as score ~0: every GE, no LT.
__device__ __forceinline__ bool score_pred(int pred, u64 score, u64 threshold) {
  return pred == TFRA_SCORE_LT ? score < threshold : score >= threshold;
}
// keep_live over the key lines and the score lines of a block's four buckets: all eight loads are issued before the first wait
__device__ __forceinline__ void keep_live8(i64 (&a)[4], i64 (&b)[4]) {
  asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}

// export_kernel's shape (64 buckets per block, one returned atomic per block) over live && pred(score) && slot in [lo, hi).
// The block's run is reserved whatever `cap` is, so *counter ends as the number of matches; an entry at a position >= cap is
// not written (key, score, row alike).  keys_out == NULL: count only.  Tail buckets are clamped, not skipped, so that the
// loads stay unconditional (see find_wave).
template <int G>
__global__ __launch_bounds__(256) void export_if_kernel(TableView v, u64 first_bucket, u64 last_bucket, u64 lo, u64 hi,
                                                        int pred, u64 threshold, u64 cap, u64* counter,
                                                        i64* __restrict__ keys_out, unsigned char* __restrict__ vals_out,
                                                        u64* __restrict__ scores_out) {
  __shared__ unsigned cnt[64];
  __shared__ u64 base_s;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const int grp_in_block = threadIdx.x >> 4;  // 0..15
  i64 k[4], sc[4];
  unsigned match[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const u64 b = first_bucket + (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    const u64 bc = b < last_bucket ? b : last_bucket - 1;
    k[it] = key_line(v, bc)[sub];
    sc[it] = (i64)score_line(v, bc)[sub];
  }
  keep_live8(k, sc);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const u64 b = first_bucket + (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    const u64 slot = b * SLOTS + sub;
    const bool m = b < last_bucket && sub < SLOTS && k[it] != EMPTY_KEY && k[it] != LOCKED_KEY &&
                   score_pred(pred, (u64)sc[it], threshold) && slot >= lo && slot < hi;
    match[it] = (unsigned)(__ballot(m) >> gshift) & 0x7fffu;
    if (sub == 0) cnt[it * 16 + grp_in_block] = __popc(match[it]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int i = 0; i < 64; ++i) { unsigned c = cnt[i]; cnt[i] = run; run += c; }
    base_s = run ? atomicAdd(counter, (u64)run) : 0;
  }
  if (!keys_out) return;
  __syncthreads();
  const u64 base = base_s;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const u64 b = first_bucket + (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    const u64 pos0 = base + cnt[it * 16 + grp_in_block];
    unsigned m = match[it];
    if (m & (1u << sub)) {
      const u64 pos = pos0 + __popc(m & ((1u << sub) - 1));
      if (pos < cap) {
        keys_out[pos] = k[it];
        if (scores_out) scores_out[pos] = (u64)sc[it];
      }
    }
    if (vals_out) {
      unsigned r = 0;
      while (m && pos0 + r < cap) {
        const int s = __ffs(m) - 1;
        m &= m - 1;
        copy_bytes16<G>(vals_out + (pos0 + r) * (size_t)v.field_bytes, row_at(v, b, (unsigned)s), v.field_bytes, sub);
        ++r;
      }
    }
  }
}

// the two side rows under the same predicate and cap rule
__global__ void export_reserved_if_kernel(TableView v, u64 lo, u64 hi, int pred, u64 threshold, u64 cap, u64* counter,
                                          i64* keys_out, unsigned char* vals_out, u64* scores_out) {
  if (!score_pred(pred, ~0ULL, threshold)) return;
  for (int r = 0; r < NUM_RESERVED; ++r) {
    u64 slot = v.nb * SLOTS + r;
    if (slot < lo || slot >= hi || !v.reserved_present[r]) continue;
    __shared__ u64 pos_s;
    if (threadIdx.x == 0) pos_s = atomicAdd(counter, 1ULL);
    __syncthreads();
    u64 pos = pos_s;
    if (keys_out && pos < cap) {
      if (threadIdx.x == 0) { keys_out[pos] = EMPTY_KEY + r; if (scores_out) scores_out[pos] = ~0ULL; }
      if (vals_out)
        for (unsigned off = threadIdx.x; off < v.field_bytes; off += blockDim.x)
          vals_out[pos * (size_t)v.field_bytes + off] = row_ptr(v, (i64)slot)[off];
    }
    __syncthreads();
  }
}

// The same scan over the whole table; every matching slot is emptied as erase_kernel empties it (CAS key -> EMPTY_KEY, then
// the score word to 0; the overflow flags are monotone, so nothing else is needed).  One size_add per wave, one atomicAdd
// per block into `erased` (optional).  Block 0 clears the matching side rows through reserved_present.
__global__ __launch_bounds__(256) void erase_if_kernel(TableView v, int pred, u64 threshold, u64* erased) {
  __shared__ int wave_gone[4];
  const int lane = threadIdx.x & 63, sub = lane & 15;
  const int grp_in_block = threadIdx.x >> 4;  // 0..15
  i64 k[4], sc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const u64 b = (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    const u64 bc = b < v.nb ? b : v.nb - 1;
    k[it] = key_line(v, bc)[sub];
    sc[it] = (i64)score_line(v, bc)[sub];
  }
  keep_live8(k, sc);
  int gone = 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const u64 b = (u64)blockIdx.x * 64 + it * 16 + grp_in_block;
    if (b < v.nb && sub < SLOTS && k[it] != EMPTY_KEY && k[it] != LOCKED_KEY && score_pred(pred, (u64)sc[it], threshold)) {
      if (atomicCAS((u64*)(key_line(v, b) + sub), (u64)k[it], (u64)EMPTY_KEY) == (u64)k[it]) {
        score_line(v, b)[sub] = 0;
        ++gone;
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < NUM_RESERVED && score_pred(pred, ~0ULL, threshold))
    gone += atomicExch(&v.reserved_present[threadIdx.x], 0u) != 0;
  for (int o = 32; o > 0; o >>= 1) gone += __shfl_xor(gone, o);
  if (lane == 0) {
    if (gone) size_add(v, (u64)blockIdx.x * 4 + (threadIdx.x >> 6), -(long long)gone);
    wave_gone[threadIdx.x >> 6] = gone;
  }
  if (!erased) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = wave_gone[0] + wave_gone[1] + wave_gone[2] + wave_gone[3];
    if (total) atomicAdd(erased, (u64)total);
  }
}

int tfra::score_filter_check(const Table* t, int pred, const char* fn) {
  if (!t) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null table");
  if (pred != TFRA_SCORE_GE && pred != TFRA_SCORE_LT)
    return set_error(TFRA_ERR_INVALID, std::string(fn) + ": unknown predicate " + std::to_string(pred) + " (TFRA_SCORE_GE | TFRA_SCORE_LT)");
  if (t->opts.strategy < 0)
    return set_error(TFRA_ERR_UNSUPPORTED, std::string(fn) + ": the table keeps no scores (strategy TFRA_EVICT_NONE)");
  return TFRA_OK;
}

// Slots [offset, offset + n) of `v` as the export kernels take them: the buckets [first_bucket, last_bucket) that hold one, a block per 64
// of them (grid == 0: side rows only; hi > total: the side rows are in the window).  false: an empty window, the call returns TFRA_OK.
struct ScanWindow { u64 lo, hi, total, first_bucket, last_bucket; unsigned grid; };
static bool scan_window(const TableView& v, size_t offset, size_t n, ScanWindow* w) {
  const u64 lo = offset, hi = offset + n, total = v.nb * SLOTS;
  if (n == 0 || lo >= total + NUM_RESERVED) return false;
  const u64 fb = lo / SLOTS, lb = std::min<u64>(v.nb, (std::min<u64>(hi, total) + SLOTS - 1) / SLOTS);
  *w = ScanWindow{lo, hi, total, fb, lb, lb > fb ? (unsigned)((lb - fb + 63) / 64) : 0u};
  return true;
}

extern "C" int tfra_table_slot_census(tfra_table_t* tp, uint64_t* out5, tfra_stream_t stream) {
  TABLE_ENTER();
  if (!out5) return set_error(TFRA_ERR_INVALID, "slot_census: null out");
  u64* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 5 * sizeof(u64)));
  HIP_TRY(hipMemsetAsync(d, 0, 5 * sizeof(u64), s));
  slot_census_kernel<<<2048, 256, 0, s>>>(t->view_of(t->cur), d);
  HIP_TRY(hipMemcpyAsync(out5, d, 5 * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipFree(d));
  return TFRA_OK;
}

extern "C" int tfra_table_export_batch(tfra_table_t* tp, size_t n, size_t offset, size_t* d_counter, int64_t* keys,
                                       void* values, uint64_t* scores, tfra_stream_t stream) {
  TABLE_ENTER();
  if (!d_counter || !keys) return set_error(TFRA_ERR_INVALID, "export: null buffer");
  const TableView v = t->view_of(t->cur);
  ScanWindow w;
  if (!scan_window(v, offset, n, &w)) return TFRA_OK;
  int g = granule_of(t->field_bytes, values, nullptr);
  u64* c = (u64*)d_counter;
  unsigned char* vo = (unsigned char*)values;
  if (w.grid)
    with_granule(g, [&](auto G) { export_kernel<G><<<w.grid, 256, 0, s>>>(v, w.first_bucket, w.last_bucket, w.lo, w.hi, c, (i64*)keys, vo, (u64*)scores); });
  if (w.hi > w.total)
    export_reserved_kernel<<<1, 64, 0, s>>>(v, w.lo, w.hi, c, (i64*)keys, vo, (u64*)scores);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

extern "C" int tfra_table_export_batch_if(tfra_table_t* tp, int pred, uint64_t threshold, size_t n, size_t offset, size_t* d_counter,
                                          size_t cap, int64_t* keys, void* values, uint64_t* scores, tfra_stream_t stream) {
  {
    int rc = score_filter_check(reinterpret_cast<Table*>(tp), pred, "tfra_table_export_batch_if");
    if (rc) return rc;
  }
  if (!d_counter) return set_error(TFRA_ERR_INVALID, "tfra_table_export_batch_if: null counter");
  if (!keys && (values || scores))
    return set_error(TFRA_ERR_INVALID, "tfra_table_export_batch_if: keys == NULL (count only) takes no values and no scores");
  TABLE_ENTER();
  const TableView v = t->view_of(t->cur);
  ScanWindow w;
  if (!scan_window(v, offset, n, &w)) return TFRA_OK;
  int g = granule_of(t->field_bytes, values, nullptr);
  u64* c = (u64*)d_counter;
  unsigned char* vo = (unsigned char*)values;
  if (w.grid)
    with_granule(g, [&](auto G) {
      export_if_kernel<G><<<w.grid, 256, 0, s>>>(v, w.first_bucket, w.last_bucket, w.lo, w.hi, pred, (u64)threshold, (u64)cap, c, (i64*)keys, vo, (u64*)scores);
    });
  if (w.hi > w.total)
    export_reserved_if_kernel<<<1, 64, 0, s>>>(v, w.lo, w.hi, pred, (u64)threshold, (u64)cap, c, (i64*)keys, vo, (u64*)scores);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

extern "C" int tfra_table_erase_if(tfra_table_t* tp, int pred, uint64_t threshold, size_t* d_erased, tfra_stream_t stream) {
  {
    int rc = score_filter_check(reinterpret_cast<Table*>(tp), pred, "tfra_table_erase_if");
    if (rc) return rc;
  }
  TABLE_ENTER();
  TableView v = t->view_of(t->cur);
  erase_if_kernel<<<(unsigned)((v.nb + 63) / 64), 256, 0, s>>>(v, pred, (u64)threshold, (u64*)d_erased);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
