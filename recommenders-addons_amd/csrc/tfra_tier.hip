// The read side of a tier: tfra_table_find_missed — find that also lists its misses —, tfra_table_assign — a write
// that only hits — and tfra_table_contains.  All three are find_wave (tfra_device.h: 16 lanes per key, U = 4 keys in flight per
// group) with one of its Tier* extras; what is new here is the append of the miss list.  The tier driver (tfra_tierstep.hip, DESIGN
// §4.20) launches find_missed through launch_find_missed (tfra_tier.h), with the touching instance find_missed_touch_kernel.
#include <hip/hip_runtime.h>

#include "tfra_host.h"
#include "tfra_tier.h"
#include "tfra_tier_device.h"

using namespace tfra;

// ---- find_missed: the body is find_missed_body (tfra_tier_device.h), on the block index of the launch ------------------------------
// The kernels of the body: find_missed_kernel under the name and with the code it had, and the touching instance.
template <int G, int U, bool PF1, int TILES>
__global__ __launch_bounds__(256 * TILES) void find_missed_kernel(TableView v, size_t n, const i64* __restrict__ keys, unsigned char* __restrict__ out,
                                                                  uint8_t* __restrict__ exists, const unsigned char* __restrict__ defaults, int full,
                                                                  const long long* __restrict__ d_n, MissOut mo) {
  find_missed_body<G, U, PF1, TILES>(v, n, keys, out, exists, defaults, full, d_n, mo, TierMissed{mo.scores, 0u}, blockIdx.x);
}
template <int G, int U, bool PF1, int TILES>
__global__ __launch_bounds__(256 * TILES) void find_missed_touch_kernel(TableView v, size_t n, const i64* __restrict__ keys, unsigned char* __restrict__ out,
                                                                        uint8_t* __restrict__ exists, const unsigned char* __restrict__ defaults, int full,
                                                                        const long long* __restrict__ d_n, MissOut mo, int strategy, u64 epoch) {
  find_missed_body<G, U, PF1, TILES>(v, n, keys, out, exists, defaults, full, d_n, mo, TierMissedTouch{mo.scores, 0u, strategy, epoch}, blockIdx.x);
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

void launch_find_missed(Table* t, hipStream_t s, size_t n, const long long* dn, const i64* k, unsigned char* o, uint8_t* exists,
                        const unsigned char* d, int full, const MissOut& mo, bool touch) {
  const TableView v = t->view_of(t->cur);
  const int g = o ? granule_of(t->field_bytes, o, d) : 16;
  constexpr int U = 4;
  const dim3 grid(blocks_of(n, TIER_TILES)), block(256 * TIER_TILES);
  const int strat = t->opts.strategy;
  const u64 epoch = t->global_epoch;
  with_granule(g, [&](auto G) {
    if constexpr (G == 16) {   // a dense table: both home-bucket lines of a key in flight together, as find does
      if (t->dense) {
        if (touch) find_missed_touch_kernel<16, U, true, TIER_TILES><<<grid, block, 0, s>>>(v, n, k, o, exists, d, full, dn, mo, strat, epoch);
        else find_missed_kernel<16, U, true, TIER_TILES><<<grid, block, 0, s>>>(v, n, k, o, exists, d, full, dn, mo);
        return;
      }
    }
    if (touch) find_missed_touch_kernel<G, U, false, TIER_TILES><<<grid, block, 0, s>>>(v, n, k, o, exists, d, full, dn, mo, strat, epoch);
    else find_missed_kernel<G, U, false, TIER_TILES><<<grid, block, 0, s>>>(v, n, k, o, exists, d, full, dn, mo);
  });
}

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
  const MissOut mo{(u64*)d_missed_counter, (u64)cap, (i64*)missed_keys, (int*)missed_indices, (u64*)scores_out};
  launch_find_missed(t, s, n, (const long long*)d_n, (const i64*)keys, (unsigned char*)values, exists, (const unsigned char*)defaults,
                     default_is_full, mo, false);
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
