// The read side of a tier: tfra_table_find_missed — find that also lists its misses —, tfra_table_assign — a write
// that only hits — and tfra_table_contains.  All three are find_wave (tfra_device.h: 16 lanes per key, U = 4 keys in flight per
// group) with one of its Tier* extras; what is new here is the append of the miss list.
#include <hip/hip_runtime.h>

#include "tfra_host.h"

using namespace tfra;

// 64-key tiles (four waves each) that ONE block of find_missed_kernel covers — a block of 256 * TIER_TILES threads — and so the keys
// behind one atomicAdd on the miss counter: 64 * TIER_TILES.  Adds to one address serialise (DESIGN §4 measured ~150 M/s), so
// B = 131 072 keys cost 2048 / TIER_TILES adds.  The tiles of a block run side by side, not one after the other: the launch has
// find_kernel's waves in flight whatever the value.  The value kept is the one scripts/mb_find_missed.py measured best
// (profiles/find_missed_mb.jsonl); a build with -DTFRA_TIER_TILES=N tries another.
#ifndef TFRA_TIER_TILES
#define TFRA_TIER_TILES 4
#endif
constexpr int TIER_TILES = TFRA_TIER_TILES;
static_assert(TIER_TILES == 1 || TIER_TILES == 2 || TIER_TILES == 4, "a block has at most 1024 threads");

// Where the miss list goes (tfra_table_export_batch_if's counter and cap rules).
struct MissOut {
  u64* counter;    // device size_t, advanced by every miss whatever cap is; null: no list
  u64 cap;         // pairs at positions >= cap are not written
  i64* keys;       // may be null
  int* idx;        // may be null
  u64* scores;     // find_missed's scores_out: may be null
};

__device__ __forceinline__ size_t served(size_t n, const long long* d_n) {   // min(n, *d_n), a negative count = 0 (find_kernel's)
  if (!d_n) return n;
  const long long dn = *d_n;
  return dn < 0 ? 0 : min(n, (size_t)dn);
}

// ---- find_missed ----------------------------------------------------------------------------------------------------------------
// A block is TILES tiles of 64 keys, one wave per 16 keys, all through find_wave at once; each wave leaves its 16-bit miss mask in
// LDS.  Then ONE wave scans the 4 * TILES counts, ONE lane takes the block's range with ONE atomicAdd (none when the block has no
// miss), and every wave stores its pairs at the base it was given: plain vector stores, behind every load group of the lookup.
template <int G, int U, bool PF1, int TILES>
__global__ __launch_bounds__(256 * TILES) void find_missed_kernel(TableView v, size_t n, const i64* __restrict__ keys, unsigned char* __restrict__ out,
                                                                  uint8_t* __restrict__ exists, const unsigned char* __restrict__ defaults, int full,
                                                                  const long long* __restrict__ d_n, MissOut mo) {
  constexpr int NW = 4 * TILES;   // waves per block
  __shared__ unsigned s_mask[NW];
  __shared__ u64 s_base[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned wave = blockIdx.x * NW + w;
  TierMissed x{mo.scores, 0u};
  find_wave<G, U, G == 16, PF1, TierMissed>(v, served(n, d_n), keys, out, exists, defaults, full, 0u, wave, &x);
  if (!mo.counter) return;   // (uniform) find plus scores
  if (lane == 0) s_mask[w] = x.miss;
  __syncthreads();
  if (w == 0) {
    const unsigned c = lane < NW ? (unsigned)__popc(s_mask[lane]) : 0u;
    unsigned incl = c;
#pragma unroll
    for (int o = 1; o < NW; o <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, o);
      if (lane >= o) incl += up;
    }
    const unsigned total = (unsigned)__shfl((int)incl, NW - 1);
    u64 b = 0;
    if (lane == 0 && total) b = atomicAdd(mo.counter, (u64)total);
    b = (u64)shfl_i64((i64)b, 0);
    if (lane < NW) s_base[lane] = b + (incl - c);
  }
  __syncthreads();
  if (!mo.keys && !mo.idx) return;   // count only
  if (lane >= 16 || !((x.miss >> lane) & 1u)) return;
  const unsigned i = wave * 16 + lane;   // (a bit is only set for i < n)
  const u64 p = s_base[w] + (unsigned)__popc(x.miss & ((1u << lane) - 1u));
  if (p >= mo.cap) return;
  if (mo.keys) mo.keys[p] = keys[i];
  if (mo.idx) mo.idx[p] = (int)i;
}

// ---- assign: values[i] into the row of every resident key, the score touched as on an assign; absent keys change nothing ----------
template <int G, int U, bool PF1>
__global__ __launch_bounds__(256) void assign_kernel(TableView v, size_t n, const i64* __restrict__ keys, const unsigned char* __restrict__ vals,
                                                     const u64* __restrict__ scores, uint8_t* __restrict__ found, int strategy, u64 epoch,
                                                     const long long* __restrict__ d_n) {
  TierAssign x{scores, strategy, epoch};
  find_wave<G, U, false, PF1, TierAssign>(v, served(n, d_n), keys, nullptr, found, vals, 1, 0u, blockIdx.x * 4 + (threadIdx.x >> 6), &x);
}

// ---- contains: the probe alone ----------------------------------------------------------------------------------------------------
template <int U, bool PF1>
__global__ __launch_bounds__(256) void contains_kernel(TableView v, size_t n, const i64* __restrict__ keys, uint8_t* __restrict__ exists,
                                                       const long long* __restrict__ d_n) {
  find_wave<16, U, false, PF1, TierContains>(v, served(n, d_n), keys, nullptr, exists, nullptr, 0, 0u, blockIdx.x * 4 + (threadIdx.x >> 6));
}

// =============================== host side ==========================================================================================

// The refusals the three calls share, in this order: the table (by the caller), then the buffers, then the count.
static int tier_check(const char* fn, size_t n, bool buffers) {
  if (!buffers) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null buffer");
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": more than 2^31-1 keys per call");
  return TFRA_OK;
}
static unsigned blocks_of(size_t n, int tiles) { return (unsigned)((n + 64 * (size_t)tiles - 1) / (64 * (size_t)tiles)); }

extern "C" {

int tfra_table_find_missed(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, void* values, uint8_t* exists,
                           uint64_t* scores_out, const void* defaults, int default_is_full, size_t* d_missed_counter, size_t cap,
                           int64_t* missed_keys, int32_t* missed_indices, tfra_stream_t stream) {
  const char* fn = "tfra_table_find_missed";
  if (!tp) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null table");
  if (n == 0) return TFRA_OK;
  if (int rc = tier_check(fn, n, keys && (defaults || !values))) return rc;
  if (!d_missed_counter && (missed_keys || missed_indices))
    return set_error(TFRA_ERR_INVALID, std::string(fn) + ": a miss list needs its counter (d_missed_counter == NULL)");
  TABLE_ENTER();
  const TableView v = t->view_of(t->cur);
  const int g = values ? granule_of(t->field_bytes, values, defaults) : 16;
  constexpr int U = 4;
  const dim3 grid(blocks_of(n, TIER_TILES)), block(256 * TIER_TILES);
  const i64* k = (const i64*)keys;
  unsigned char* o = (unsigned char*)values;
  const unsigned char* d = (const unsigned char*)defaults;
  const long long* dn = (const long long*)d_n;
  const MissOut mo{(u64*)d_missed_counter, (u64)cap, (i64*)missed_keys, (int*)missed_indices, (u64*)scores_out};
  with_granule(g, [&](auto G) {
    if constexpr (G == 16) {   // a dense table: both home-bucket lines of a key in flight together, as find does
      if (t->dense) { find_missed_kernel<16, U, true, TIER_TILES><<<grid, block, 0, s>>>(v, n, k, o, exists, d, default_is_full, dn, mo); return; }
    }
    find_missed_kernel<G, U, false, TIER_TILES><<<grid, block, 0, s>>>(v, n, k, o, exists, d, default_is_full, dn, mo);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_table_assign(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const void* values, const uint64_t* scores,
                      uint8_t* found, tfra_stream_t stream) {
  const char* fn = "tfra_table_assign";
  if (!tp) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null table");
  if (n == 0) return TFRA_OK;
  if (int rc = tier_check(fn, n, keys && values)) return rc;
  TABLE_ENTER();
  const TableView v = t->view_of(t->cur);
  const int g = granule_of(t->field_bytes, values, nullptr);
  constexpr int U = 4;
  const dim3 grid(blocks_of(n, 1)), block(256);
  const i64* k = (const i64*)keys;
  const unsigned char* vals = (const unsigned char*)values;
  const u64* sc = (const u64*)scores;
  const long long* dn = (const long long*)d_n;
  const int strat = t->opts.strategy;
  const u64 epoch = t->global_epoch;
  with_granule(g, [&](auto G) {
    if constexpr (G == 16) {
      if (t->dense) { assign_kernel<16, U, true><<<grid, block, 0, s>>>(v, n, k, vals, sc, found, strat, epoch, dn); return; }
    }
    assign_kernel<G, U, false><<<grid, block, 0, s>>>(v, n, k, vals, sc, found, strat, epoch, dn);
  });
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}

int tfra_table_contains(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, uint8_t* exists, tfra_stream_t stream) {
  const char* fn = "tfra_table_contains";
  if (!tp) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null table");
  if (n == 0) return TFRA_OK;
  if (int rc = tier_check(fn, n, keys && exists)) return rc;
  TABLE_ENTER();
  const TableView v = t->view_of(t->cur);
  constexpr int U = 4;
  const dim3 grid(blocks_of(n, 1)), block(256);
  const long long* dn = (const long long*)d_n;
  if (t->dense) contains_kernel<U, true><<<grid, block, 0, s>>>(v, n, (const i64*)keys, exists, dn);
  else contains_kernel<U, false><<<grid, block, 0, s>>>(v, n, (const i64*)keys, exists, dn);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

}  // extern "C"
