// The typed accumulate of the table (tfra_table.hip): tfra_table_accum_or_assign.  Unique keys run the locked kernel and, on a table
// at max_capacity, tfra_upsert.hip's eviction phase (evict_phase, tfra_upsert.h); keys that repeat are sorted first (rocprim: the
// only unit of the family that needs it).  (Unique keys on a table that is large for the batch take the ownership pass instead.)
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "tfra_host.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;

// ---- typed accumulate: row[j] += delta[j], one add per element (ValueArray::operator+=) ----

template <int DT>
__device__ __forceinline__ void row_add(unsigned char* row, const unsigned char* delta, unsigned dim, int sub) {
  for (unsigned j = sub; j < dim; j += 16) {
    if (DT == TFRA_F32) reinterpret_cast<float*>(row)[j] += reinterpret_cast<const float*>(delta)[j];
    else if (DT == TFRA_F64) reinterpret_cast<double*>(row)[j] += reinterpret_cast<const double*>(delta)[j];
    else if (DT == TFRA_I8) reinterpret_cast<signed char*>(row)[j] = (signed char)(reinterpret_cast<signed char*>(row)[j] + reinterpret_cast<const signed char*>(delta)[j]);
    else if (DT == TFRA_I32) reinterpret_cast<unsigned*>(row)[j] += reinterpret_cast<const unsigned*>(delta)[j];
    else if (DT == TFRA_I64) reinterpret_cast<u64*>(row)[j] += reinterpret_cast<const u64*>(delta)[j];
    else if (DT == TFRA_F16) {
      _Float16 a = reinterpret_cast<_Float16*>(row)[j], b = reinterpret_cast<const _Float16*>(delta)[j];
      reinterpret_cast<_Float16*>(row)[j] = (_Float16)((float)a + (float)b);
    } else {
      unsigned short* r = reinterpret_cast<unsigned short*>(row);
      r[j] = f32_to_bf16(bf16_to_f32(r[j]) + bf16_to_f32(reinterpret_cast<const unsigned short*>(delta)[j]));
    }
  }
}

// ---- accum_or_assign.  ROUND >= 0: duplicate-safe mode, processes only the occurrence that is
// currently first-in-line for its key (election word), see host loop. -------------------------
// one (key, values-or-delta, exists) triple: absent & !exists -> insert, present & exists -> row += delta, else nothing
template <int DT, int G>
__device__ __forceinline__ void accum_one(const TableView& v, size_t i, const i64* __restrict__ keys,
                                          const unsigned char* __restrict__ vod, const uint8_t* __restrict__ exists,
                                          const u64* __restrict__ scores, unsigned dim, const AuxInit& ai, int strategy, u64 epoch,
                                          uint8_t* __restrict__ deferred, int bounded_mode, int sub, int gshift, int& fresh,
                                          int& failed) {
  const i64 key = keys[i];
  const bool ex = exists[i] != 0;
  const unsigned char* src = vod + i * (size_t)v.field_bytes;
  if (!ex) {
    bool is_new;
    i64 row;
    if (deferred) {  // bounded table at max_capacity: keys without a free slot evict in phase 2
      u64 h;
      const u64 b0 = bucket0(key, v.nb, h);
      const i64 k0 = load_key_coherent(key_line(v, b0) + sub);
      row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, bounded_mode);
      if (sub == 0) deferred[i] = row == NEED_EVICT;
    } else {
      row = locate_or_claim(v, key, sub, gshift, is_new);
    }
    if (row < 0) failed += (sub == 0 && row != NEED_EVICT);
    else if (is_new) {
      copy_bytes16<G>(row_ptr(v, row), src, v.field_bytes, sub);
      if (v.n_fields > 1) init_aux_fields(v, ai, row, sub, 0);
      update_score(v, row, true, strategy, scores ? scores[i] : 1, epoch, sub);
      fresh += (sub == 0);
    }  // present & !exists: dropped
  } else {
    i64 row = probe_find<true>(v, key, sub, gshift);
    if (row >= 0) {
      row_add<DT>(row_ptr(v, row), src, dim, sub);
      update_score(v, row, false, strategy, scores ? scores[i] : 1, epoch, sub);
    }  // absent & exists: dropped
    if (deferred && sub == 0) deferred[i] = 0;
  }
}

template <int DT, int G>
__global__ __launch_bounds__(256) void accum_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                    const unsigned char* __restrict__ vod,
                                                    const uint8_t* __restrict__ exists,
                                                    const u64* __restrict__ scores, unsigned dim,
                                                    AuxInit ai, int strategy, u64 epoch,
                                                    uint8_t* __restrict__ deferred, int bounded_mode) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t g = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  const size_t wave = g >> 2;
  int fresh = 0, failed = 0;
  if (g < n) accum_one<DT, G>(v, g, keys, vod, exists, scores, dim, ai, strategy, epoch, deferred, bounded_mode, sub, gshift, fresh, failed);
  wave_account(v, wave, lane, fresh, failed);
}

// Keys that repeat within one call: the reference applies the triples one after the other in index order
// (LaunchTensorsAccum on one thread; accumrase_fn, cuckoohash_map.hh:619-633), and the outcome of an occurrence depends
// on the ones before it (an insert makes the key present for the next).  The (key, index) pairs arrive sorted by key
// (stable radix sort: indices ascend within a key); the group of a key's FIRST sorted position walks the key's
// occurrences in index order, every step through memory (a key that repeats thousands of times is one long chain —
// exact, not fast: TFRA de-duplicates before accum, PY/dynamic_embedding_variable.py:1377-1378).
template <int DT, int G>
__global__ __launch_bounds__(256) void accum_segments_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                             const unsigned char* __restrict__ vod,
                                                             const uint8_t* __restrict__ exists, const u64* __restrict__ scores,
                                                             unsigned dim, AuxInit ai, int strategy, u64 epoch,
                                                             const u64* __restrict__ sorted_keys, const unsigned* __restrict__ sorted_idx) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t p = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  int fresh = 0, failed = 0;
  if (p < n) {
    const u64 k = sorted_keys[p];
    if (p == 0 || sorted_keys[p - 1] != k) {
      for (size_t q = p; q < n && sorted_keys[q] == k; ++q) {
        accum_one<DT, G>(v, (size_t)sorted_idx[q], keys, vod, exists, scores, dim, ai, strategy, epoch, nullptr, 0, sub, gshift, fresh, failed);
        __threadfence_block();   // the next occurrence reads what this one wrote (other lanes of the group, same row)
      }
    }
  }
  wave_account(v, p >> 2, lane, fresh, failed);
}

__global__ void iota_u32_kernel(unsigned* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (unsigned)i;
}

static void launch_accum(int dt, int g, dim3 grid, hipStream_t s, TableView v, size_t n, const i64* k, const unsigned char* vod,
                         const uint8_t* ex, const u64* sc, unsigned dim, AuxInit ai, int strat, u64 epoch,
                         const u64* sorted_keys, const unsigned* sorted_idx, uint8_t* deferred, int bmode) {
  with_dtype(dt, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    with_granule(g, [&](auto G) {
      if (sorted_keys) accum_segments_kernel<DT, G><<<grid, 256, 0, s>>>(v, n, k, vod, ex, sc, dim, ai, strat, epoch, sorted_keys, sorted_idx);
      else accum_kernel<DT, G><<<grid, 256, 0, s>>>(v, n, k, vod, ex, sc, dim, ai, strat, epoch, deferred, bmode);
    });
  });
}

extern "C" int tfra_table_accum_or_assign(tfra_table_t* tp, size_t n, const int64_t* keys, const void* vod,
                                          const uint8_t* exists, const uint64_t* scores, uint32_t flags, tfra_stream_t stream) {
  TABLE_ENTER();
  if (n == 0) return TFRA_OK;
  int rc = check_batch("accum: ", n, keys && vod && exists);
  if (rc) return rc;
  rc = t->prepare_insert(n, s);
  if (rc) return rc;
  int g = granule_of(t->field_bytes, vod, nullptr);
  TableView v = t->view_of(t->cur);
  const i64* k = (const i64*)keys;
  if (flags & TFRA_FLAG_UNIQUE_KEYS) {
    // unique keys (what TFRA hands the op: PY/dynamic_embedding_variable.py:1377-1378): the single pass with bucket ownership,
    // as tfra_table_insert_or_assign does, whenever the batch is small for the table; else the locked kernels
    bool taken = false;
    rc = own_upsert_unique(t, s, n, k, vod, (const u64*)scores, &taken, exists);
    if (rc) return rc;
    if (taken) return TFRA_OK;   // (TableWrapper::accum does not step the epoch: lookup_table_op_hkv.h:539-546)
    dim3 grid((unsigned)((n * 16 + 255) / 256));
    uint8_t* deferred;
    rc = t->bounded_flags(n, s, &deferred);
    if (rc) return rc;
    launch_accum(t->opts.value_dtype, g, grid, s, v, n, k, (const unsigned char*)vod, exists, (const u64*)scores,
                 (unsigned)t->opts.dim, t->aux, t->opts.strategy, t->global_epoch, nullptr, nullptr, deferred,
                 bounded_mode(t, deferred != nullptr));
    // phase 2: the absent keys that found no free slot replace a minimum-score entry
    if (deferred) evict_phase(t, s, v, g, n, k, (const unsigned char*)vod, (const u64*)scores, 0, deferred);
    HIP_TRY(hipGetLastError());
    return TFRA_OK;
  }
  {
    uint8_t* bounded_now;
    rc = t->bounded_flags(1, s, &bounded_now);
    if (rc) return rc;
    if (bounded_now)
      return set_error(TFRA_ERR_UNSUPPORTED, "accum: a bounded (Hkv) table at max_capacity needs TFRA_FLAG_UNIQUE_KEYS "
                                             "(HKV's unique-keys contract) so that eviction is well defined");
  }
  // Duplicate-safe mode: the reference applies the triples sequentially in index order (LaunchTensorsAccum on one
  // thread).  All on the device, no host copy and no synchronisation: a stable radix sort of (key, index) groups the
  // occurrences of a key with their indices ascending, and accum_segments_kernel walks each group in that order.
  {
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs((void*)nullptr, tmp_bytes, (const u64*)nullptr, (u64*)nullptr, (const unsigned*)nullptr,
                                      (unsigned*)nullptr, n, 0u, 64u, s));
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    rc = t->ensure_scratch(al(n * 8) + 2 * al(n * 4) + al(tmp_bytes), s);
    if (rc) return rc;
    t->apply_P = 0;  // scratch head is overwritten below
    unsigned char* w = (unsigned char*)t->scratch;
    u64* sorted_keys = (u64*)w; w += al(n * 8);
    unsigned* iota = (unsigned*)w; w += al(n * 4);
    unsigned* sorted_idx = (unsigned*)w; w += al(n * 4);
    void* tmp = w;
    iota_u32_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(iota, n);
    HIP_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, (const u64*)keys, sorted_keys, (const unsigned*)iota, sorted_idx, n, 0u, 64u, s));
    dim3 grid((unsigned)((n * 16 + 255) / 256));
    launch_accum(t->opts.value_dtype, g, grid, s, v, n, k, (const unsigned char*)vod, exists, (const u64*)scores,
                 (unsigned)t->opts.dim, t->aux, t->opts.strategy, t->global_epoch, sorted_keys, sorted_idx, nullptr, 0);
  }
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
