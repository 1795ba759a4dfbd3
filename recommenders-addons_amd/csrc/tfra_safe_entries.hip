// The entry lists of safe sparse lookups: tfra_multi_safe_entries builds, for a LIST of safe lookups, the kept list
// (the entries that survive pruning by weight, in input order) and the entry list (the kept entries and one entry per row left
// without any, in row order) on the device, and leaves both counts per list there.  One record upload, then at most five launches,
// whatever the list's length:
//   keep       (lists that prune)  per tile of 1024 entries: every entry's member flag and in-tile exclusive member prefix, the
//                                  tile's member count
//   keep scan  (lists that prune)  one block per list: the tile counts to exclusive offsets, the total behind them
//   rows       per tile of 1024 rows: lb(r) and lb(r + 1), K(lb(r)), the member-less flag and its in-tile exclusive prefix,
//              the tile's count of member-less rows
//   row scan   one block per list: those tile counts to exclusive offsets; writes d_counts
//   scatter    one thread per entry and one per row: members to kept position K(p) and entry position K(p) + E(row), the
//              filler of a member-less row r to K(lb(r)) + E(r)
// K(p) = members before p, E(r) = member-less rows before r, lb(r) = the first p with row >= r.  A list that does not prune has
// K(p) = clamp(p, lb(0), lb(n_rows)) - lb(0) in closed form and skips the first two launches.
// No block waits for another: the scans over tile counts are launches of their own.  Every write position is below the buffer's
// length for ANY rows / splits: K(p) <= p, E(r) <= r, lb(r) <= nnz, and a member's row is checked against n_rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_frontend.h"
#include "tfra_host.h"
#include "tfra_many.h"

using namespace tfra;

namespace {

constexpr unsigned SE_B = 256;                  // threads of a block
constexpr unsigned SE_R = 4;                    // rounds: a thread's entries (rows) are tile + k * SE_B + t — every round coalesced
constexpr unsigned SE_T = SE_B * SE_R;          // a tile
constexpr unsigned SE_FLAG = 0x80000000u;       // top bit of a kpre / rpre word: member / member-less
constexpr unsigned SE_MASK = 0x7fffffffu;
constexpr size_t SE_MAX_LIST = (size_t)1 << 31;    // nnz + n_rows of one list stays below
constexpr size_t SE_MAX_TOTAL = (size_t)1 << 24;   // entries plus rows of a call

// One list.  flags holds TFRA_SAFE_PRUNE only where the list has weights and entries: its K comes from kpre / ktile.
struct SafeRec {
  const i64* rows;   // ascending row ids [nnz], or (RAGGED) row_splits [n_rows + 1]
  const i64* ids;
  const float* w;
  i64 fill_id;
  i64* kept_ids; i64* kept_rows; float* kept_w;
  i64* ent_ids; i64* ent_rows; float* ent_w;
  i64* counts;
  unsigned* kpre;    // [nnz]             member flag | in-tile exclusive member prefix     (PRUNE)
  unsigned* ktile;   // [entry tiles + 1] members per tile -> exclusive offsets, the total  (PRUNE)
  unsigned* rpre;    // [n_rows]          member-less flag | in-tile exclusive prefix
  unsigned* rk;      // [n_rows]          K(lb(r))
  unsigned* rtile;   // [row tiles + 1]   member-less rows per tile -> exclusive offsets, the total
  unsigned nnz, n_rows, flags;
};

__device__ __forceinline__ unsigned se_tiles(unsigned n) { return (n + SE_T - 1) / SE_T; }

// lb(row), row in [0, n_rows]: the first p with row(p) >= row, in [0, nnz]
__device__ __forceinline__ unsigned se_lb(const SafeRec& r, unsigned row) {
  if (r.flags & TFRA_SAFE_RAGGED) {
    const i64 s = r.rows[row];
    return s < 0 ? 0u : s > (i64)r.nnz ? r.nnz : (unsigned)s;
  }
  unsigned lo = 0, hi = r.nnz;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (r.rows[mid] < (i64)row) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the row of entry p when it lies in [0, n_rows), else -1
__device__ __forceinline__ i64 se_row(const SafeRec& r, unsigned p) {
  if (!(r.flags & TFRA_SAFE_RAGGED)) {
    const i64 v = r.rows[p];
    return (v >= 0 && v < (i64)r.n_rows) ? v : -1;
  }
  if ((i64)p < r.rows[0]) return -1;
  unsigned lo = 0, hi = r.n_rows;   // how many of row_splits[1 .. n_rows] are <= p
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (r.rows[1 + mid] <= (i64)p) lo = mid + 1; else hi = mid;
  }
  return lo < r.n_rows ? (i64)lo : -1;
}

// lb(0) and lb(n_rows) of a list that does not prune, hi >= lo whatever the rows hold: threads 0 and 1, then the block
__device__ __forceinline__ void se_range(const SafeRec& r, unsigned* s_lohi) {
  if (!(r.flags & TFRA_SAFE_PRUNE) && threadIdx.x < 2) s_lohi[threadIdx.x] = se_lb(r, threadIdx.x ? r.n_rows : 0u);
  __syncthreads();
}

// K(x), x in [0, nnz]; <= x
__device__ __forceinline__ unsigned se_K(const SafeRec& r, unsigned lo, unsigned hi, unsigned x) {
  if (r.flags & TFRA_SAFE_PRUNE) return x < r.nnz ? r.ktile[x / SE_T] + (r.kpre[x] & SE_MASK) : r.ktile[se_tiles(r.nnz)];
  hi = max(hi, lo);
  return min(max(x, lo), hi) - lo;
}

// The tile's flags f[k] (position tile + k * SE_B + t) to their exclusive prefix in position order; returns the tile's count.
__device__ __forceinline__ unsigned se_tile_scan(const bool (&f)[SE_R], unsigned (&excl)[SE_R], unsigned (*wsum)[4]) {
  const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k) {
    const unsigned long long m = __ballot(f[k]);
    excl[k] = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[k][w] = (unsigned)__popcll(m);
  }
  __syncthreads();
  unsigned run = 0;
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k)
#pragma unroll
    for (unsigned ww = 0; ww < 4; ++ww) {
      if (ww == w) excl[k] += run;
      run += wsum[k][ww];
    }
  return run;
}

// a[0 .. nt) to its exclusive prefix sums by one block; returns the total (every thread)
__device__ __forceinline__ unsigned se_scan_tiles(unsigned* a, unsigned nt, unsigned* lds) {
  const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned run = 0;
  for (unsigned base = 0; base < nt; base += SE_B) {
    const unsigned i = base + threadIdx.x;
    const unsigned v = i < nt ? a[i] : 0u;
    unsigned x = v;
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    unsigned woff = 0, tot = 0;
#pragma unroll
    for (unsigned ww = 0; ww < 4; ++ww) {
      if (ww < w) woff += lds[ww];
      tot += lds[ww];
    }
    if (i < nt) a[i] = run + woff + x - v;
    run += tot;
    __syncthreads();
  }
  return run;
}

// keep: a pruning list owns ceil(nnz / SE_T) blocks
__global__ __launch_bounds__(SE_B) void se_keep_kernel(const SafeRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                       const unsigned* __restrict__ idx, unsigned n) {
  __shared__ unsigned wsum[SE_R][4];
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const SafeRec r = recs[idx[d]];
  const unsigned tile = blockIdx.x - prefix[d];
  bool f[SE_R];
  unsigned ex[SE_R];
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k) {
    const unsigned p = tile * SE_T + k * SE_B + threadIdx.x;
    f[k] = p < r.nnz && r.w[p] > 0.0f && se_row(r, p) >= 0;
  }
  const unsigned total = se_tile_scan(f, ex, wsum);
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k) {
    const unsigned p = tile * SE_T + k * SE_B + threadIdx.x;
    if (p < r.nnz) r.kpre[p] = ex[k] | (f[k] ? SE_FLAG : 0u);
  }
  if (threadIdx.x == 0) r.ktile[tile] = total;
}

// keep scan: one block per pruning list
__global__ __launch_bounds__(SE_B) void se_keep_scan_kernel(const SafeRec* __restrict__ recs, const unsigned* __restrict__ idx) {
  __shared__ unsigned lds[4];
  const SafeRec r = recs[idx[blockIdx.x]];
  const unsigned nt = se_tiles(r.nnz);
  const unsigned total = se_scan_tiles(r.ktile, nt, lds);
  if (threadIdx.x == 0) r.ktile[nt] = total;
}

// rows: a list with rows owns ceil(n_rows / SE_T) blocks
__global__ __launch_bounds__(SE_B) void se_rows_kernel(const SafeRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                       const unsigned* __restrict__ idx, unsigned n) {
  __shared__ unsigned wsum[SE_R][4];
  __shared__ unsigned s_lohi[2];
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const SafeRec r = recs[idx[d]];
  const unsigned tile = blockIdx.x - prefix[d];
  se_range(r, s_lohi);
  const unsigned lo = s_lohi[0], hi = s_lohi[1];   // (read only where the list does not prune)
  bool f[SE_R];
  unsigned ex[SE_R], kb[SE_R];
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k) {
    const unsigned row = tile * SE_T + k * SE_B + threadIdx.x;
    f[k] = false; kb[k] = 0;
    if (row < r.n_rows) {
      kb[k] = se_K(r, lo, hi, se_lb(r, row));
      f[k] = se_K(r, lo, hi, se_lb(r, row + 1)) <= kb[k];
    }
  }
  const unsigned total = se_tile_scan(f, ex, wsum);
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k) {
    const unsigned row = tile * SE_T + k * SE_B + threadIdx.x;
    if (row < r.n_rows) {
      r.rpre[row] = ex[k] | (f[k] ? SE_FLAG : 0u);
      r.rk[row] = kb[k];
    }
  }
  if (threadIdx.x == 0) r.rtile[tile] = total;
}

// row scan: one block per list of the call, the lists without rows included; writes both counts
__global__ __launch_bounds__(SE_B) void se_row_scan_kernel(const SafeRec* __restrict__ recs) {
  __shared__ unsigned lds[4];
  __shared__ unsigned s_lohi[2];
  const SafeRec r = recs[blockIdx.x];
  if (r.n_rows == 0) {
    if (threadIdx.x == 0) { r.counts[0] = 0; r.counts[1] = 0; }
    return;
  }
  se_range(r, s_lohi);
  const unsigned nt = se_tiles(r.n_rows);
  const unsigned fillers = se_scan_tiles(r.rtile, nt, lds);
  if (threadIdx.x == 0) {
    r.rtile[nt] = fillers;
    const unsigned kept = se_K(r, s_lohi[0], s_lohi[1], r.nnz);
    r.counts[0] = (i64)kept;
    r.counts[1] = (i64)kept + (i64)fillers;
  }
}

// scatter: a list owns ceil(nnz / SE_T) entry tiles and, where it wants its entry list, ceil(n_rows / SE_T) row tiles behind them
__global__ __launch_bounds__(SE_B) void se_scatter_kernel(const SafeRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                          const unsigned* __restrict__ idx, unsigned n) {
  __shared__ unsigned s_lohi[2];
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const SafeRec r = recs[idx[d]];
  const unsigned j = blockIdx.x - prefix[d], nte = se_tiles(r.nnz);
  const unsigned cap = r.nnz + r.n_rows;   // (the guards below never bite: see the head of this file)
  if (j >= nte) {   // a row tile: the fillers
    const unsigned rt = j - nte;
    const unsigned off = r.rtile[rt];
    const bool fill = r.flags & TFRA_SAFE_FILL;
#pragma unroll
    for (unsigned k = 0; k < SE_R; ++k) {
      const unsigned row = rt * SE_T + k * SE_B + threadIdx.x;
      if (row >= r.n_rows) continue;
      const unsigned v = r.rpre[row];
      if (!(v & SE_FLAG)) continue;
      const unsigned pos = r.rk[row] + off + (v & SE_MASK);
      if (pos >= cap) continue;
      r.ent_ids[pos] = fill ? r.fill_id : 0;
      r.ent_rows[pos] = (i64)row;
      if (r.ent_w) r.ent_w[pos] = fill ? 1.0f : 0.0f;
    }
    return;
  }
  se_range(r, s_lohi);
  const unsigned lo = s_lohi[0], hi = s_lohi[1];
  const bool prune = r.flags & TFRA_SAFE_PRUNE;
  const unsigned koff = prune ? r.ktile[j] : 0u;
#pragma unroll
  for (unsigned k = 0; k < SE_R; ++k) {
    const unsigned p = j * SE_T + k * SE_B + threadIdx.x;
    if (p >= r.nnz) continue;
    unsigned K;
    if (prune) {
      const unsigned v = r.kpre[p];
      if (!(v & SE_FLAG)) continue;
      K = koff + (v & SE_MASK);
    } else {
      K = se_K(r, lo, hi, p);
    }
    const i64 row = se_row(r, p);
    if (row < 0 || K >= r.nnz) continue;
    const i64 id = r.ids[p];
    const float wv = r.w ? r.w[p] : 1.0f;
    if (r.kept_ids) {
      r.kept_ids[K] = id;
      r.kept_rows[K] = row;
      if (r.w) r.kept_w[K] = wv;
    }
    if (r.ent_ids) {
      const unsigned pos = K + r.rtile[(unsigned)row / SE_T] + (r.rpre[row] & SE_MASK);
      if (pos >= cap) continue;
      r.ent_ids[pos] = id;
      r.ent_rows[pos] = row;
      if (r.ent_w) r.ent_w[pos] = wv;
    }
  }
}

struct OutRange {
  uintptr_t lo, hi;
  size_t desc;
};

// where a list's scratch lies in the call's front of the workspace (bytes from its start)
struct SafeScratch {
  size_t kpre, ktile, rpre, rk, rtile;
};

}  // namespace

extern "C" int tfra_multi_safe_entries(tfra_workspace_t* ws, size_t n_lists, const tfra_safe_entries_desc* descs,
                                       uint32_t* launches_out, tfra_stream_t stream) {
  const std::string who = "multi_safe_entries";
  if (launches_out) *launches_out = 0;
  if (n_lists == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and nothing is written
  std::vector<OutRange> ranges;
  std::vector<SafeScratch> at(n_lists);
  std::vector<unsigned> flags(n_lists);
  size_t total = 0, front = 0;
  auto take = [&front](size_t words) { const size_t o = front; front += align_up(words * sizeof(unsigned)); return o; };
  for (size_t i = 0; i < n_lists; ++i) {
    const tfra_safe_entries_desc& d = descs[i];
    const std::string at_i = who + ": descriptor " + std::to_string(i) + ": ";
    if (d.struct_size != sizeof(tfra_safe_entries_desc)) return set_error(TFRA_ERR_INVALID, at_i + "descriptor size mismatch");
    if (d.flags & ~(TFRA_SAFE_PRUNE | TFRA_SAFE_FILL | TFRA_SAFE_RAGGED)) return set_error(TFRA_ERR_INVALID, at_i + "unknown flag bits");
    if (!d.d_counts) return set_error(TFRA_ERR_INVALID, at_i + "null d_counts");
    const bool kept = d.kept_ids || d.kept_rows || d.kept_weights, ent = d.entry_ids || d.entry_rows || d.entry_weights;
    if (kept && (!d.kept_ids || !d.kept_rows || (d.weights && !d.kept_weights)))
      return set_error(TFRA_ERR_INVALID, at_i + "kept_ids, kept_rows and kept_weights go together");
    if (ent && (!d.entry_ids || !d.entry_rows)) return set_error(TFRA_ERR_INVALID, at_i + "entry_ids and entry_rows go together");
    if (d.n_rows >= SE_MAX_LIST || d.nnz >= SE_MAX_LIST || d.nnz + d.n_rows >= SE_MAX_LIST)
      return set_error(TFRA_ERR_UNSUPPORTED, at_i + "nnz + n_rows >= 2^31");
    if (d.n_rows && (d.nnz || (d.flags & TFRA_SAFE_RAGGED)) && !d.rows) return set_error(TFRA_ERR_INVALID, at_i + "null rows");
    if (d.n_rows && d.nnz && (kept || ent) && !d.ids) return set_error(TFRA_ERR_INVALID, at_i + "null ids");
    const void* p8[] = {d.rows, d.ids, d.kept_ids, d.kept_rows, d.entry_ids, d.entry_rows, d.d_counts};
    for (const void* p : p8)
      if ((uintptr_t)p % 8) return set_error(TFRA_ERR_INVALID, at_i + "an int64 buffer is not 8-byte aligned");
    const void* p4[] = {d.weights, d.kept_weights, d.entry_weights};
    for (const void* p : p4)
      if ((uintptr_t)p % 4) return set_error(TFRA_ERR_INVALID, at_i + "a float buffer is not 4-byte aligned");
    total += d.nnz + d.n_rows;
    if (total > SE_MAX_TOTAL) return set_error(TFRA_ERR_UNSUPPORTED, at_i + "the lists total more than 2^24 entries plus rows");
    auto range = [&](const void* p, size_t bytes) {
      if (p && bytes) ranges.push_back({(uintptr_t)p, (uintptr_t)p + bytes, i});
    };
    range(d.d_counts, 2 * sizeof(int64_t));
    range(d.kept_ids, d.nnz * sizeof(int64_t));
    range(d.kept_rows, d.nnz * sizeof(int64_t));
    range(d.weights ? d.kept_weights : nullptr, d.nnz * sizeof(float));
    range(d.entry_ids, (d.nnz + d.n_rows) * sizeof(int64_t));
    range(d.entry_rows, (d.nnz + d.n_rows) * sizeof(int64_t));
    range(d.entry_weights, (d.nnz + d.n_rows) * sizeof(float));
    // (K of a list without weights or without entries is the closed form)
    flags[i] = d.flags & ~((d.weights && d.nnz && d.n_rows) ? 0u : (unsigned)TFRA_SAFE_PRUNE);
    if (d.n_rows) {
      const size_t nte = (d.nnz + SE_T - 1) / SE_T, ntr = (d.n_rows + SE_T - 1) / SE_T;
      if (flags[i] & TFRA_SAFE_PRUNE) { at[i].kpre = take(d.nnz); at[i].ktile = take(nte + 1); }
      at[i].rpre = take(d.n_rows); at[i].rk = take(d.n_rows); at[i].rtile = take(ntr + 1);
    }
  }
  // every list's outputs are written by blocks of their own with nothing ordered between them: no two output ranges may meet
  std::sort(ranges.begin(), ranges.end(), [](const OutRange& a, const OutRange& b) { return a.lo < b.lo; });
  for (size_t k = 1, top = 0; k < ranges.size(); ++k) {   // top: the range that reaches furthest so far
    if (ranges[k].lo < ranges[top].hi)
      return set_error(TFRA_ERR_INVALID, who + ": descriptor " + std::to_string(std::max(ranges[k].desc, ranges[top].desc)) +
                                             ": an output range overlaps one of descriptor " +
                                             std::to_string(std::min(ranges[k].desc, ranges[top].desc)));
    if (ranges[k].hi > ranges[top].hi) top = k;
  }
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));

  Blob blob;
  const size_t rec_off = blob.add<SafeRec>(n_lists);
  const size_t cls_off = blob.add<unsigned>(3 * ClassPool::words(n_lists, 1, true));   // (a list may stand in all three classes)
  ManyUpload up;
  if (int rc = many_begin(ws, front, blob.bytes(), s, &up)) return rc;
  unsigned char* scratch = (unsigned char*)ws->buf;
  SafeRec* recs = section<SafeRec>(up.host, rec_off);
  for (size_t i = 0; i < n_lists; ++i) {
    const tfra_safe_entries_desc& d = descs[i];
    SafeRec r{};
    r.rows = (const i64*)d.rows; r.ids = (const i64*)d.ids; r.w = d.weights; r.fill_id = d.fill_id;
    r.kept_ids = (i64*)d.kept_ids; r.kept_rows = (i64*)d.kept_rows; r.kept_w = d.kept_weights;
    r.ent_ids = (i64*)d.entry_ids; r.ent_rows = (i64*)d.entry_rows; r.ent_w = d.entry_weights;
    r.counts = (i64*)d.d_counts;
    r.nnz = (unsigned)d.nnz; r.n_rows = (unsigned)d.n_rows; r.flags = flags[i];
    if (d.n_rows) {
      if (flags[i] & TFRA_SAFE_PRUNE) { r.kpre = (unsigned*)(scratch + at[i].kpre); r.ktile = (unsigned*)(scratch + at[i].ktile); }
      r.rpre = (unsigned*)(scratch + at[i].rpre); r.rk = (unsigned*)(scratch + at[i].rk); r.rtile = (unsigned*)(scratch + at[i].rtile);
    }
    recs[i] = r;
  }
  auto tiles = [](size_t n) { return (unsigned)((n + SE_T - 1) / SE_T); };
  ClassPool pool{section<unsigned>(up.host, cls_off)};
  const ManyClass c_keep = pool.put(n_lists, true, [&](size_t k) { return (flags[k] & TFRA_SAFE_PRUNE) != 0; },
                                    [&](size_t k) { return tiles(descs[k].nnz); });
  const ManyClass c_rows = pool.put(n_lists, true, [&](size_t k) { return descs[k].n_rows != 0; },
                                    [&](size_t k) { return tiles(descs[k].n_rows); });
  auto scat_blocks = [&](size_t k) {
    const tfra_safe_entries_desc& d = descs[k];
    if (!d.n_rows) return 0u;
    return d.entry_ids ? tiles(d.nnz) + tiles(d.n_rows) : d.kept_ids ? tiles(d.nnz) : 0u;
  };
  const ManyClass c_scat = pool.put(n_lists, true, [&](size_t k) { return scat_blocks(k) != 0; }, scat_blocks);
  if (int rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true)) return rc;

  const SafeRec* drecs = section<const SafeRec>(up.dev, rec_off);
  const unsigned* dcls = section<const unsigned>(up.dev, cls_off);
  uint32_t launches = 0;
  if (c_keep.n) {
    const unsigned* pre = dcls + c_keep.at;
    se_keep_kernel<<<c_keep.grid, SE_B, 0, s>>>(drecs, pre, pre + c_keep.n + 1, c_keep.n);
    se_keep_scan_kernel<<<c_keep.n, SE_B, 0, s>>>(drecs, pre + c_keep.n + 1);
    launches += 2;
  }
  if (c_rows.n) {
    const unsigned* pre = dcls + c_rows.at;
    se_rows_kernel<<<c_rows.grid, SE_B, 0, s>>>(drecs, pre, pre + c_rows.n + 1, c_rows.n);
    ++launches;
  }
  se_row_scan_kernel<<<(unsigned)n_lists, SE_B, 0, s>>>(drecs);
  ++launches;
  if (c_scat.n) {
    const unsigned* pre = dcls + c_scat.at;
    se_scatter_kernel<<<c_scat.grid, SE_B, 0, s>>>(drecs, pre, pre + c_scat.n + 1, c_scat.n);
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}
