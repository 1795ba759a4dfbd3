// The pooling lists of a field-wise embedding: tfra_field_entries orders a dense [n_rows, per_row] block of ids by
// (sample, slot, input position) and writes the n_rows * nslots + 1 split points of the segments sample * nslots + slot — what the
// pooled lookups, the combined write-back and the weight gradient want in front of them — in ONE launch:
//   count    every wave owns a contiguous stretch of its sample's positions and walks it in chunks of 64; the lanes of a chunk
//            that hold the same slot find each other by one ballot per slot bit, and the lowest of them adds their number to the
//            wave's own count of that slot in LDS
//   scan     the sample's first wave turns the counts into exclusive starts, per slot and then per wave, and writes the sample's
//            nslots splits (the block of the last sample also the closing one)
//   scatter  the waves walk their stretches again: an entry goes to start(wave, slot) + the lanes below it in its match, and the
//            lowest lane of a match moves the start on
// A sample with up to 64 entries takes one wave (4 samples to a block), up to 128 two, else four.  The sort is local to a sample, so
// no block waits for another, nothing is scanned across blocks and there is no workspace.  The order is STABLE: stretches, chunks and
// lanes are all in position order.  A slot outside [0, nslots) is clamped before it is looked at and counted in d_bad.  Every write
// position is sample * per_row + rank with rank checked against per_row, the splits' index is below n_rows * nslots + 1 by
// construction: no write leaves its buffer whatever `slots` holds (or becomes between the two walks).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tfra_mi355x.h"
#include "tfra_host.h"

using namespace tfra;

namespace {

constexpr unsigned FE_B = 256;                    // threads of a block: 4 waves
constexpr unsigned FE_W = FE_B / 64;
constexpr size_t FE_MAX_N = (size_t)1 << 31;      // ids, and samples, stay below
static_assert(TFRA_FIELD_ENTRIES_MAX_SLOTS * FE_W * sizeof(unsigned) <= 32768, "the waves' counts of a block at the cap: 32 KiB of LDS");

struct FieldArgs {
  const i64* ids;
  const i64* slots;
  i64* entry_ids;
  i64* row_splits;
  int* entry_pos;
  i64* entry_seg;
  i64* d_bad;
  unsigned n_rows, per_row, nslots;
  unsigned wps;      // waves per sample: 1, 2 or 4
  unsigned stretch;  // positions of a wave, a multiple of 64
  unsigned bits;     // bits of nslots - 1
};

// the slot of a position, clamped into [0, nslots)
__device__ __forceinline__ unsigned fe_slot(i64 v, unsigned nslots, bool* bad) {
  *bad = v < 0 || v >= (i64)nslots;
  return v < 0 ? 0u : v >= (i64)nslots ? nslots - 1u : (unsigned)v;
}

// the lanes of the wave that are `live` and hold the same slot as this one (every lane of the wave calls it)
__device__ __forceinline__ unsigned long long fe_match(bool live, unsigned slot, unsigned bits) {
  unsigned long long m = __ballot(live);
  for (unsigned b = 0; b < bits; ++b) {
    const bool one = (slot >> b) & 1u;
    const unsigned long long bm = __ballot(one);
    m &= one ? bm : ~bm;
  }
  return m;
}

__global__ __launch_bounds__(FE_B) void field_entries_kernel(const FieldArgs a) {
  extern __shared__ unsigned fe_lds[];   // [FE_W][nslots]: a wave's counts, then its starts
  const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned ws = w / a.wps, wi = w % a.wps;          // the sample of this wave within the block, the wave within the sample
  const size_t sample = (size_t)blockIdx.x * (FE_W / a.wps) + ws;
  const bool have = sample < a.n_rows;
  volatile unsigned* mine = fe_lds + w * a.nslots;
  for (unsigned f = lane; f < a.nslots; f += 64) mine[f] = 0;
  // (a wave's LDS accesses complete in program order, and `mine` is this wave's alone until the barrier)
  const size_t base = sample * a.per_row;
  const unsigned lo = wi * a.stretch;
  const unsigned hi = have ? min(a.per_row, lo + a.stretch) : 0u;
  unsigned n_bad = 0;
  for (unsigned c = lo; c < hi; c += 64) {
    const unsigned p = c + lane;
    const bool live = p < hi;
    bool bad = false;
    const unsigned slot = fe_slot(live ? a.slots[base + p] : 0, a.nslots, &bad);
    n_bad += (unsigned)__popcll(__ballot(live && bad));
    const unsigned long long m = fe_match(live, slot, a.bits);
    if (live && !(m & below)) mine[slot] += (unsigned)__popcll(m);
  }
  if (a.d_bad && lane == 0 && n_bad) atomicAdd((unsigned long long*)a.d_bad, (unsigned long long)n_bad);
  __syncthreads();
  if (have && wi == 0) {   // counts -> starts, by the sample's first wave; `run`: the entries of the slots below this round's
    volatile unsigned* cnt = fe_lds + w * a.nslots;   // (wave wi of the sample: cnt + wi * nslots)
    unsigned run = 0;
    for (unsigned f0 = 0; f0 < a.nslots; f0 += 64) {
      const unsigned f = f0 + lane;
      unsigned c[FE_W], tot = 0;
#pragma unroll
      for (unsigned k = 0; k < FE_W; ++k) {
        c[k] = (k < a.wps && f < a.nslots) ? cnt[k * a.nslots + f] : 0u;
        tot += c[k];
      }
      unsigned x = tot;
#pragma unroll
      for (unsigned o = 1; o < 64; o <<= 1) {
        const unsigned y = __shfl_up(x, o);
        if (lane >= o) x += y;
      }
      unsigned start = run + x - tot;
      run += __shfl(x, 63);
      if (f < a.nslots) {
        a.row_splits[sample * a.nslots + f] = (i64)(base + start);
#pragma unroll
        for (unsigned k = 0; k < FE_W; ++k)
          if (k < a.wps) { cnt[k * a.nslots + f] = start; start += c[k]; }
      }
    }
    if (sample == (size_t)a.n_rows - 1 && lane == 0) a.row_splits[(size_t)a.n_rows * a.nslots] = (i64)((size_t)a.n_rows * a.per_row);
  }
  __syncthreads();
  for (unsigned c = lo; c < hi; c += 64) {
    const unsigned p = c + lane;
    const bool live = p < hi;
    bool bad = false;
    const unsigned slot = fe_slot(live ? a.slots[base + p] : 0, a.nslots, &bad);
    const unsigned long long m = fe_match(live, slot, a.bits);
    const unsigned before = (unsigned)__popcll(m & below);
    unsigned rank = 0;
    if (live) {
      rank = mine[slot] + before;
      if (before == 0) mine[slot] = rank + (unsigned)__popcll(m);
    }
    if (live && rank < a.per_row) {
      a.entry_ids[base + rank] = a.ids[base + p];
      if (a.entry_pos) a.entry_pos[base + rank] = (int)(base + p);
      if (a.entry_seg) a.entry_seg[base + rank] = (i64)(sample * a.nslots + slot);
    }
  }
}

struct Range {
  uintptr_t lo, hi;
};

}  // namespace

extern "C" int tfra_field_entries(size_t n_rows, size_t per_row, size_t nslots, const int64_t* ids, const int64_t* slots,
                                  int64_t* entry_ids, int64_t* row_splits, int32_t* entry_pos, int64_t* entry_seg,
                                  int64_t* d_bad, tfra_stream_t stream) {
  const std::string who = "field_entries: ";
  if (n_rows == 0) return TFRA_OK;
  // every check runs before anything is enqueued: a refused call writes nothing
  if (nslots == 0) return set_error(TFRA_ERR_INVALID, who + "nslots == 0");
  if (!row_splits) return set_error(TFRA_ERR_INVALID, who + "null row_splits");
  if (per_row && (!ids || !slots || !entry_ids)) return set_error(TFRA_ERR_INVALID, who + "null ids, slots or entry_ids");
  if (nslots > TFRA_FIELD_ENTRIES_MAX_SLOTS)
    return set_error(TFRA_ERR_UNSUPPORTED, who + "nslots " + std::to_string(nslots) + " exceeds " + std::to_string(TFRA_FIELD_ENTRIES_MAX_SLOTS));
  if (n_rows >= FE_MAX_N || per_row >= FE_MAX_N || n_rows * per_row >= FE_MAX_N)
    return set_error(TFRA_ERR_UNSUPPORTED, who + "n_rows * per_row >= 2^31");
  const size_t n = n_rows * per_row;
  const void* p8[] = {ids, slots, entry_ids, row_splits, entry_seg, d_bad};
  for (const void* p : p8)
    if ((uintptr_t)p % 8) return set_error(TFRA_ERR_INVALID, who + "an int64 buffer is not 8-byte aligned");
  if ((uintptr_t)entry_pos % 4) return set_error(TFRA_ERR_INVALID, who + "entry_pos is not 4-byte aligned");
  // the blocks write their samples' outputs with nothing ordered between them, and read ids and slots twice: no output may meet
  // another output or an input (ids and slots may be one buffer)
  Range r[7];
  unsigned n_in = 0, n_r = 0;
  auto range = [&](const void* p, size_t bytes) {
    if (p && bytes) r[n_r++] = {(uintptr_t)p, (uintptr_t)p + bytes};
  };
  range(ids, n * sizeof(int64_t));
  range(slots, n * sizeof(int64_t));
  n_in = n_r;
  range(entry_ids, n * sizeof(int64_t));
  range(row_splits, (n_rows * nslots + 1) * sizeof(int64_t));
  range(entry_pos, n * sizeof(int32_t));
  range(entry_seg, n * sizeof(int64_t));
  range(d_bad, sizeof(int64_t));
  for (unsigned i = n_in; i < n_r; ++i)
    for (unsigned j = 0; j < i; ++j)
      if (r[i].lo < r[j].hi && r[j].lo < r[i].hi) return set_error(TFRA_ERR_INVALID, who + "an output overlaps another buffer of the call");

  FieldArgs a{};
  a.ids = (const i64*)ids; a.slots = (const i64*)slots;
  a.entry_ids = (i64*)entry_ids; a.row_splits = (i64*)row_splits; a.entry_pos = entry_pos; a.entry_seg = (i64*)entry_seg;
  a.d_bad = (i64*)d_bad;
  a.n_rows = (unsigned)n_rows; a.per_row = (unsigned)per_row; a.nslots = (unsigned)nslots;
  a.wps = per_row <= 64 ? 1u : per_row <= 128 ? 2u : FE_W;
  const size_t share = (per_row + a.wps - 1) / a.wps;
  a.stretch = (unsigned)((share + 63) / 64 * 64);
  a.bits = 0;
  while (((size_t)1 << a.bits) < nslots) ++a.bits;
  const size_t per_block = FE_W / a.wps;
  const unsigned grid = (unsigned)((n_rows + per_block - 1) / per_block);
  field_entries_kernel<<<grid, FE_B, FE_W * nslots * sizeof(unsigned), (hipStream_t)stream>>>(a);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
