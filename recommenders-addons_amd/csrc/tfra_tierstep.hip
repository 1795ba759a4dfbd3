// The tier driver: an upper table — a bounded LRU cache at max_capacity — in front of a lower table that never
// forgets, driven as ONE stream-ordered chain with no host read: tfra_tier_find, tfra_tier_find_or_insert, tfra_tier_insert.
// (Many tiers' find_or_insert in one chain: tfra_multi_tier_find_or_insert, tfra_tierstep_many.hip, DESIGN §4.25.  find_or_insert
// over the distinct keys of a write-back plan: tfra_tier_find_or_insert_planned, tfra_tierplan.hip)
// Whole co-located rows move between the tiers, so a key that goes down and comes up again keeps its slot vectors.
// The launches of a find_or_insert: tier_begin_kernel; find_missed_touch_kernel on the upper table (launch_find_missed,
// tfra_tier.hip); tier_fetch_kernel on the lower table (here); the locked whole-row upsert into the upper table, its phase 2
// capturing (insert_counted, tfra_upsert.hip); the same upsert of what was displaced into the lower table; with TFRA_TIER_VERIFY
// a count-only find_missed_kernel on the upper table.
#include <hip/hip_runtime.h>

#include <new>

#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_tier.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;

// One thread, in place of a memset: the previous call's two counters go into the statistics and start from zero.
__global__ void tier_begin_kernel(u64* w) {
  w[TS_CALLS] += 1;
  w[TS_MISSED] += w[TC_MISSED];
  w[TS_DEMOTED] += w[TC_DOWN];
  w[TC_MISSED] = 0;
  w[TC_DOWN] = 0;
}

// ---- step 2: the lower table's lookup of the miss list ----------------------------------------------------------------------------
// find_wave with TierFetch: the embedding of listed key j goes to out[pos_of[j]].  With a stage, the whole row goes to stage row j: a
// hit's as the lower table stores it, a never-seen key's as [its default row | slot vectors at aux_init] — what an upsert would have
// left for it.  The block's hits are counted with ONE add (none when it has no hit).
// (A TWIN, tier_fetch_body in tfra_tierstep_many.hip, runs this on a block index local to a descriptor of the grouped admission:
// as a call of a shared body this kernel lost its code — by-value structs went to LDS — DESIGN §4.25.  A fix here belongs there too.)
template <int G, int U, bool PF1, int TILES>
__global__ __launch_bounds__(256 * TILES) void tier_fetch_kernel(TableView v, FetchIO io, AuxInit ai) {
  constexpr int NW = 4 * TILES;
  __shared__ unsigned s_hits[NW];
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4, w = threadIdx.x >> 6;
  const unsigned wave = blockIdx.x * NW + w;
  const size_t n = min(io.cap, (size_t)*io.d_count);   // uniform
  TierFetch x;
  x.pos_of = io.pos_of;
  x.where = io.where;
  find_wave<G, U, G == 16, PF1, TierFetch>(v, n, io.keys, io.out, nullptr, io.defaults, io.full, 0u, wave, &x);
  unsigned hits = 0;
  if ((size_t)wave * (4 * U) < n) {   // (the waves find_wave served: x.word / x.pos are set)
    const unsigned whole = v.n_fields * v.field_bytes;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t j = (size_t)wave * (4 * U) + (unsigned)(u * 4 + grp);
      const bool valid = j < n;   // (a clamped tail position is not a key)
      const bool hit = valid && x.word[u] >= 0;
      hits += (unsigned)__popcll(__ballot(hit && sub == 0));
      if (!io.stage || !valid) continue;
      unsigned char* srow = io.stage + j * whole;
      if (hit) {
        copy_bytes16<G>(srow, word_row_ptr(v, (u64)x.word[u]), whole, sub);
      } else {
        copy_bytes16<G>(srow, io.defaults + (io.full ? (size_t)x.pos[u] * v.field_bytes : 0), v.field_bytes, sub);
        for (unsigned f = 1; f < v.n_fields; ++f)
          fill_aux_field(srow + f * v.field_bytes, v.field_bytes, ai.pattern[(f - 1) & 3], ai.elem_bytes, G >= 4 && (v.field_bytes & 3) == 0, sub);
      }
    }
  }
  if (lane == 0) s_hits[w] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) total += s_hits[i];
    if (total) atomicAdd(io.lower_hits, (u64)total);
  }
}

// =============================== host side ==========================================================================================

void tier_begin(tfra_tier* tier, hipStream_t s) { tier_begin_kernel<<<1, 1, 0, s>>>(tier->words); }

void launch_fetch(Table* lower, hipStream_t s, size_t n, const FetchIO& io, const AuxInit& ai) {
  const TableView v = lower->view_of(lower->cur);
  int g = granule_of(lower->field_bytes, io.out, io.defaults);
  if (io.stage) g = std::min(g, granule_of(lower->field_bytes, io.stage, nullptr));
  constexpr int U = 4;
  const dim3 grid(blocks_of(n, TIER_TILES)), block(256 * TIER_TILES);
  with_granule(g, [&](auto G) {
    if constexpr (G == 16) {
      if (lower->dense) { tier_fetch_kernel<16, U, true, TIER_TILES><<<grid, block, 0, s>>>(v, io, ai); return; }
    }
    tier_fetch_kernel<G, U, false, TIER_TILES><<<grid, block, 0, s>>>(v, io, ai);
  });
}

// The head of every call on a tier: the refusals that need no device (here), then the driver's lock and both tables' (TierEntry and
// tier_enter: tfra_tier.h).
static int tier_check(const char* fn, const tfra_tier* tier, size_t n, bool buffers) {
  if (!buffers) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null buffer");
  if (n > tier->max_batch) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": more keys than the tier's max_batch");
  return TFRA_OK;
}

// steps 3 and 4: `values` into the upper table, what that displaces as whole rows into the lower one
int tier_put(tfra_tier* tier, hipStream_t s, size_t n, const long long* d_n, const i64* keys, const unsigned char* values, bool whole_in) {
  const EvictOut eo{tier->words + TC_DOWN, (u64)tier->max_batch, tier->down_keys, tier->down_rows, tier->down_scores, tier->whole};
  if (int rc = insert_counted(tier->upper, s, n, d_n, keys, values, nullptr, whole_in, &eo)) return rc;
  return insert_counted(tier->lower, s, n, (const long long*)(tier->words + TC_DOWN), tier->down_keys, tier->down_rows, nullptr, true, nullptr);
}

extern "C" {

int tfra_tier_create(tfra_table_t* up, tfra_table_t* lo, size_t max_batch, tfra_tier_t** out) {
  const char* fn = "tfra_tier_create: ";
  if (!up || !lo || !out) return set_error(TFRA_ERR_INVALID, std::string(fn) + "null table or out");
  Table* upper = reinterpret_cast<Table*>(up);
  Table* lower = reinterpret_cast<Table*>(lo);
  if (upper == lower) return set_error(TFRA_ERR_INVALID, std::string(fn) + "upper and lower are the same table");
  if (upper->device != lower->device || upper->opts.value_dtype != lower->opts.value_dtype || upper->opts.dim != lower->opts.dim ||
      upper->opts.aux_fields != lower->opts.aux_fields)
    return set_error(TFRA_ERR_INVALID, std::string(fn) + "the tables differ in device, value dtype, dim or aux_fields");
  if (upper->opts.strategy != TFRA_EVICT_LRU && upper->opts.strategy != TFRA_EVICT_EPOCHLRU)
    return set_error(TFRA_ERR_UNSUPPORTED, std::string(fn) + "the upper table must be LRU or EPOCHLRU (every key of a lookup must be admitted)");
  if (lower->opts.strategy != TFRA_EVICT_NONE)
    return set_error(TFRA_ERR_UNSUPPORTED, std::string(fn) + "the lower table must be TFRA_EVICT_NONE (the bottom must not forget)");
  if (max_batch == 0 || max_batch >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, std::string(fn) + "max_batch must be in [1, 2^31)");
  if (on_device(upper->device) != hipSuccess) return set_error(TFRA_ERR_HIP, std::string(fn) + "hipSetDevice failed");
  tfra_tier* t = new (std::nothrow) tfra_tier();
  if (!t) return set_error(TFRA_ERR_OOM, std::string(fn) + "out of host memory");
  t->upper = upper;
  t->lower = lower;
  t->max_batch = max_batch;
  t->fb = upper->field_bytes;
  t->whole = upper->field_bytes * (1u + (unsigned)upper->opts.aux_fields);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_words = 0, o_mk = al(TIER_WORDS * 8), o_mi = o_mk + al(max_batch * 8), o_mr = o_mi + al(max_batch * 4),
               o_up = o_mr + al(max_batch * 4), o_dk = o_up + al(max_batch * t->whole), o_dr = o_dk + al(max_batch * 8), o_ds = o_dr + al(max_batch * t->whole),
               total = o_ds + al(max_batch * 8);
  hipError_t e = hipMalloc((void**)&t->block, total);
  if (e == hipSuccess) e = hipMemset(t->block, 0, al(TIER_WORDS * 8));
  if (e != hipSuccess) {
    if (t->block) (void)hipFree(t->block);
    delete t;
    return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, std::string(fn) + "staging: " + hipGetErrorString(e));
  }
  t->words = (u64*)(t->block + o_words);
  t->miss_keys = (i64*)(t->block + o_mk);
  t->miss_idx = (int*)(t->block + o_mi);
  t->miss_rec = (int*)(t->block + o_mr);
  t->up_rows = t->block + o_up;
  t->down_keys = (i64*)(t->block + o_dk);
  t->down_rows = t->block + o_dr;
  t->down_scores = (u64*)(t->block + o_ds);
  *out = t;
  return TFRA_OK;
}

int tfra_tier_destroy(tfra_tier_t* tier) {
  if (!tier) return TFRA_OK;
  (void)hipSetDevice(tier->upper->device);
  (void)hipDeviceSynchronize();   // a queued call may still use the staging
  (void)hipFree(tier->block);
  delete tier;
  return TFRA_OK;
}

int tfra_tier_find(tfra_tier_t* tier, size_t n, const int64_t* d_n, const int64_t* keys, void* values, uint8_t* where,
                   const void* defaults, int default_is_full, tfra_stream_t stream) {
  const char* fn = "tfra_tier_find";
  if (!tier) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null tier");
  if (n == 0) return TFRA_OK;
  if (int rc = tier_check(fn, tier, n, keys && values && defaults)) return rc;
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  if (int rc = tier_enter(tier, s, &entry)) return rc;
  tier_begin_kernel<<<1, 1, 0, s>>>(tier->words);
  const MissOut mo{tier->words + TC_MISSED, (u64)tier->max_batch, tier->miss_keys, tier->miss_idx, nullptr};
  launch_find_missed(tier->upper, s, n, (const long long*)d_n, (const i64*)keys, (unsigned char*)values, where, (const unsigned char*)defaults,
                     default_is_full, mo, false);
  const FetchIO io{tier->miss_keys, tier->miss_idx, tier->words + TC_MISSED, std::min(n, tier->max_batch), (unsigned char*)values, where,
                   (const unsigned char*)defaults, default_is_full, nullptr, tier->words + TS_LOWER_HITS};
  launch_fetch(tier->lower, s, n, io, tier->upper->aux);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_tier_find_or_insert(tfra_tier_t* tier, size_t n, const int64_t* d_n, const int64_t* keys, const void* init_values,
                             int init_is_full, void* values_out, uint8_t* where, uint32_t flags, tfra_stream_t stream) {
  const Check c = check_tier_find_or_insert(tier, n, keys, init_values, flags);
  if (c.done()) return report("tfra_tier_find_or_insert: ", c);
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  if (int rc = tier_enter(tier, s, &entry)) return rc;
  const long long* dn = (const long long*)d_n;
  const i64* k = (const i64*)keys;
  const unsigned char* init = (const unsigned char*)init_values;
  tier_begin_kernel<<<1, 1, 0, s>>>(tier->words);
  // 1. the upper table: rows and `where` of the hits, their scores touched; the misses to the list
  const MissOut mo{tier->words + TC_MISSED, (u64)tier->max_batch, tier->miss_keys, tier->miss_idx, nullptr};
  launch_find_missed(tier->upper, s, n, dn, k, (unsigned char*)values_out, where, init, init_is_full, mo, true);
  // 2. the lower table: the whole row of every listed key, or the row a never-seen key starts with
  const FetchIO io{tier->miss_keys, tier->miss_idx, tier->words + TC_MISSED, std::min(n, tier->max_batch), (unsigned char*)values_out, where,
                   init, init_is_full, tier->up_rows, tier->words + TS_LOWER_HITS};
  launch_fetch(tier->lower, s, n, io, tier->upper->aux);
  HIP_TRY(hipGetLastError());
  // 3. + 4. up they go; what they displace goes down
  if (int rc = tier_put(tier, s, n, (const long long*)(tier->words + TC_MISSED), tier->miss_keys, tier->up_rows, true)) return rc;
  // 5. how many keys of the batch are NOT resident now (a batch that saturates its own home buckets)
  if (flags & TFRA_TIER_VERIFY) {
    const MissOut count{tier->words + TS_NOT_RESIDENT, 0, nullptr, nullptr, nullptr};
    launch_find_missed(tier->upper, s, n, dn, k, nullptr, nullptr, nullptr, 0, count, false);
    HIP_TRY(hipGetLastError());
  }
  return TFRA_OK;
}

int tfra_tier_insert(tfra_tier_t* tier, size_t n, const int64_t* d_n, const int64_t* keys, const void* values, tfra_stream_t stream) {
  const char* fn = "tfra_tier_insert";
  if (!tier) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null tier");
  if (n == 0) return TFRA_OK;
  if (int rc = tier_check(fn, tier, n, keys && values)) return rc;
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  if (int rc = tier_enter(tier, s, &entry)) return rc;
  tier_begin_kernel<<<1, 1, 0, s>>>(tier->words);
  return tier_put(tier, s, n, (const long long*)d_n, (const i64*)keys, (const unsigned char*)values, false);
}

int tfra_tier_stats(tfra_tier_t* tier, uint64_t* out8, tfra_stream_t stream) {
  const char* fn = "tfra_tier_stats";
  if (!tier) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null tier");
  if (!out8) return set_error(TFRA_ERR_INVALID, std::string(fn) + ": null buffer");
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  if (int rc = tier_enter(tier, s, &entry)) return rc;
  uint64_t w[TIER_WORDS];
  HIP_TRY(hipMemcpyAsync(w, tier->words, sizeof(w), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < TS_WORDS; ++i) out8[i] = w[i];
  out8[TS_MISSED] += w[TC_MISSED];   // the call still pending
  out8[TS_DEMOTED] += w[TC_DOWN];
  return TFRA_OK;
}

}  // extern "C"
