// MI355X (gfx950) dynamic-embedding table: kernels + C ABI (include/tfra_mi355x.h).
//
// Replaces, behind TFRA's own op surface, what `gpu::TableWrapper` gets from HierarchicalKV
// (R/kernels/lookup_impl/lookup_table_op_hkv.h:515-756) with results defined by the
// reference's CPU table (R/kernels/cuckoo_hashtable_op.cc, lib/cuckoo/cuckoohash_map.hh).
// Work mapping everywhere: 16 lanes per key (one 128-B bucket line per probe, one 16-B
// granule per lane per row step), 4 keys per wave64, U independent keys in flight per group.
// Growth and storage: tfra_grow.hip; the locked upsert family: tfra_upsert.hip, tfra_find_insert.hip, tfra_accum.hip; the slot-window scans: tfra_scan.hip.
#include <hip/hip_runtime.h>

#include <cstring>

#include "tfra_host.h"   // (with it: the C ABI header, tfra_device.h, <algorithm>, <mutex>, <string>)

using namespace tfra;

// =============================== kernels ====================================================

// ---- find (+ fused default fill, + exists) -------------------------------------------------
// (the work of a wave — 16 keys — is find_wave, tfra_device.h; PF1: both home-bucket lines of a key in flight together)
template <int G, int U, bool WT = (G == 16), bool PF1 = false>
__global__ __launch_bounds__(256) void find_kernel(TableView v, size_t n, const i64* __restrict__ keys,
                                                   unsigned char* __restrict__ out,
                                                   uint8_t* __restrict__ exists,
                                                   const unsigned char* __restrict__ defaults,
                                                   int full, unsigned field_off, const long long* __restrict__ d_n = nullptr) {
  if (d_n) {   // tfra_table_find_n: the key count lives on the device (n = the buffers' length)
    const long long dn = *d_n;
    n = dn < 0 ? 0 : min(n, (size_t)dn);
  }
  find_wave<G, U, WT, PF1>(v, n, keys, out, exists, defaults, full, field_off, (blockIdx.x * blockDim.x + threadIdx.x) >> 6);
}

// ---- erase ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void erase_kernel(TableView v, size_t n, const i64* __restrict__ keys) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t g = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  int gone = 0;
  if (g < n) {
    i64 key = keys[g];
    if (is_reserved_key(key)) {
      if (sub == 0) gone = atomicExch(&v.reserved_present[reserved_index(key)], 0u) != 0;
    } else {
      i64 row = probe_find<true>(v, key, sub, gshift);
      if (row >= 0 && sub == 0) {
        u64 wb; unsigned ws; split_row((u64)row, wb, ws);
        u64 w = wb * 16 + ws;
        // CAS so that duplicate keys in one call decrement the size once
        gone = atomicCAS((u64*)key_word(v, w), (u64)key, (u64)EMPTY_KEY) == (u64)key;
        if (gone && has_scores(v)) *score_word(v, w) = 0;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) gone += __shfl_xor(gone, o);
  if (lane == 0 && gone) size_add(v, g >> 2, -(long long)gone);
}

// ---- clear / fill ---------------------------------------------------------------------------
__global__ void clear_kernel(TableView v, int reset_counters) {
  size_t total = v.nb * 16;
  for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (size_t)gridDim.x * blockDim.x) {
    *key_word(v, w) = ((w & 15) == 15) ? 0 : EMPTY_KEY;
    if (has_scores(v)) *score_word(v, w) = 0;
  }
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!reset_counters) return;
  if (t < SIZE_SHARDS) v.size_shards[t * SIZE_SHARD_STRIDE] = 0;
  if (t < NUM_RESERVED) v.reserved_present[t] = 0;
  if (t == 0) { *v.err_count = 0; *const_cast<unsigned*>(v.dense_flag) = 0; }
}

__global__ void fill_i32_kernel(int* p, size_t n, int val) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = val;
}

__global__ void size_kernel(TableView v, i64* out) {
  __shared__ long long part[SIZE_SHARDS];
  part[threadIdx.x] = (long long)v.size_shards[threadIdx.x * SIZE_SHARD_STRIDE];
  __syncthreads();
  for (int s = SIZE_SHARDS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = part[0];
}

// =============================== host side ==================================================

static size_t dtype_size(int dt) {
  switch (dt) {
    case TFRA_F32: case TFRA_I32: return 4;
    case TFRA_F16: case TFRA_BF16: return 2;
    case TFRA_I8: return 1;
    case TFRA_I64: case TFRA_F64: return 8;
    default: return 0;
  }
}

static unsigned short host_f2h(float f) {
  _Float16 h = (_Float16)f;
  unsigned short u;
  memcpy(&u, &h, 2);
  return u;
}
static unsigned short host_f2b(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

static AuxInitPod make_aux_init(const tfra_table_opts& o) {   // elem_bytes = sizeof(V); pattern[f] = aux_init[f] as V, replicated to 32 bits
  AuxInitPod ai;
  ai.elem_bytes = (unsigned)dtype_size(o.value_dtype);
  for (int f = 0; f < 4; ++f) {
    float x = o.aux_init[f];
    unsigned pat = 0;
    switch (o.value_dtype) {
      case TFRA_F32: memcpy(&pat, &x, 4); break;
      case TFRA_I32: { int v = (int)x; memcpy(&pat, &v, 4); } break;
      case TFRA_F16: { unsigned short h = host_f2h(x); pat = h | ((unsigned)h << 16); } break;
      case TFRA_BF16: { unsigned short h = host_f2b(x); pat = h | ((unsigned)h << 16); } break;
      case TFRA_I8: { unsigned char c = (unsigned char)(signed char)x; pat = c * 0x01010101u; } break;
      default: pat = 0; break;  // 8-byte types: aux fields start at 0
    }
    ai.pattern[f] = pat;
  }
  return ai;
}

namespace tfra {

thread_local std::string g_last_error;
int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

void* Table::dalloc(size_t bytes, hipStream_t s) {
  if (alloc.alloc) return alloc.alloc(alloc.user, 0, bytes, (tfra_stream_t)s);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  return p;
}
void Table::dfree(void* p, hipStream_t s) {
  if (!p) return;
  if (alloc.alloc) alloc.free(alloc.user, 0, p, (tfra_stream_t)s);
  else (void)hipFree(p);
}

TableView Table::view_of(const Storage& st) const {
  TableView v;
  v.base = st.base; v.nb = st.nb;
  v.hdr = hdr_bytes();
  v.bucket_stride = bucket_stride();
  v.field_bytes = field_bytes; v.row_stride = row_stride; v.n_fields = 1 + opts.aux_fields;
  v.reserved_present = reserved_present; v.size_shards = size_shards; v.winner = winner;
  v.err_count = err_count;
  v.dense_flag = d_dense;
  return v;
}

// serialise against work queued on another stream (the reference blocks on a per-table mutex and
// a stream sync per op, R/kernels/hkv_hashtable_op_gpu.cu.cc:192-213; here: event chaining).
int Table::enter(hipStream_t s) {
  if (on_device(device) != hipSuccess) return set_error(TFRA_ERR_HIP, "hipSetDevice failed");
  if (has_last && s != last_stream && !capture_safe) {
    HIP_TRY(hipEventRecord(chain_event, last_stream));
    HIP_TRY(hipStreamWaitEvent(s, chain_event, 0));
  }
  last_stream = s;
  has_last = true;
  return TFRA_OK;
}

int Table::read_size(hipStream_t s, size_t* out) {
  enqueue_size(d_scalar, s);
  HIP_TRY(hipMemcpyAsync(h_scalar, d_scalar, sizeof(i64), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  i64 v = *h_scalar;
  *out = v < 0 ? 0 : (size_t)v;
  size_ub = *out;
  return TFRA_OK;
}

int Table::check_errors(hipStream_t s) {
  unsigned e = 0;
  HIP_TRY(hipMemcpyAsync(h_scalar, err_count, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  memcpy(&e, h_scalar, sizeof(unsigned));
  if (e) {
    HIP_TRY(hipMemsetAsync(err_count, 0, sizeof(unsigned), s));
    return set_error(TFRA_ERR_FULL, std::to_string(e) + " keys could not be placed: table full at max_capacity (or a write-back plan overflowed)");
  }
  return TFRA_OK;
}

// bucket-owner tags of the ownership-based write-backs: 4 B per bucket, zeroed; rebuilt after a rehash
unsigned* Table::ensure_own_tags(hipStream_t s) {
  if (no_owner_tags) return nullptr;
  if (own_tags && own_tags_nb == cur.nb) return own_tags;
  if (own_tags) { (void)hipStreamSynchronize(s); dfree(own_tags, s); own_tags = nullptr; }
  own_tags = (unsigned*)dalloc(cur.nb * sizeof(unsigned), s);
  if (!own_tags) { g_last_error.clear(); return nullptr; }
  if (hipMemsetAsync(own_tags, 0, cur.nb * sizeof(unsigned), s) != hipSuccess) { dfree(own_tags, s); own_tags = nullptr; return nullptr; }
  own_tags_nb = cur.nb;
  own_gen = 0;
  return own_tags;
}

int Table::ensure_winner(hipStream_t s) {
  size_t need = cur.nb * SLOTS + NUM_RESERVED;
  if (winner && winner_len >= need) return TFRA_OK;
  dfree(winner, s);
  winner = (int*)dalloc(need * sizeof(int), s);
  if (!winner) return set_error(TFRA_ERR_OOM, "winner scratch allocation failed");
  winner_len = need;
  fill_i32_kernel<<<2048, 256, 0, s>>>(winner, need, -1);
  return TFRA_OK;
}

// Hkv flavour at max_capacity (the table cannot grow): *out = the per-key phase-2 flag buffer of a
// two-phase (place, then evict) write; nullptr while the table can still grow or is unbounded.
int Table::bounded_flags(size_t n, hipStream_t s, uint8_t** out) {
  *out = nullptr;
  if (!at_max_capacity()) return TFRA_OK;
  if (evict_flags_cap < n) {
    if (evict_flags) { HIP_TRY(hipStreamSynchronize(s)); dfree(evict_flags, s); }
    evict_flags = (uint8_t*)dalloc(n, s);
    if (!evict_flags) { evict_flags_cap = 0; return set_error(TFRA_ERR_OOM, "eviction flag buffer allocation failed"); }
    evict_flags_cap = n;
  }
  *out = evict_flags;
  return TFRA_OK;
}

int Table::ensure_scratch(size_t bytes, hipStream_t s) {
  if (scratch_bytes >= bytes) return TFRA_OK;
  apply_P = 0;  // the armed cursor area of tfra_table_apply_sparse does not survive a reallocation
  if (scratch) { HIP_TRY(hipStreamSynchronize(s)); dfree(scratch, s); }
  size_t want = std::max(bytes, scratch_bytes * 2);
  scratch = dalloc(want, s);
  if (!scratch) { scratch_bytes = 0; return set_error(TFRA_ERR_OOM, "scratch allocation failed"); }
  scratch_bytes = want;
  return TFRA_OK;
}

void Table::enqueue_clear(const Storage& st, bool reset_counters, hipStream_t s) { clear_kernel<<<2048, 256, 0, s>>>(view_of(st), reset_counters ? 1 : 0); }
void Table::enqueue_size(i64* d_out, hipStream_t s) { size_kernel<<<1, SIZE_SHARDS, 0, s>>>(view_of(cur), d_out); }

}  // namespace tfra

static int find_impl(Table* t, hipStream_t s, int field, size_t n, const int64_t* keys, void* values,
                     uint8_t* exists, const void* defaults, int full, const int64_t* d_n = nullptr) {
  if (n == 0) return TFRA_OK;
  if (!keys || !values || !defaults) return set_error(TFRA_ERR_INVALID, "find: null buffer");
  if (n >= (1ULL << 32)) return set_error(TFRA_ERR_INVALID, "find: more than 2^32-1 keys per call");
  if (field < 0 || field > t->opts.aux_fields) return set_error(TFRA_ERR_INVALID, "find: bad field");
  TableView v = t->view_of(t->cur);
  unsigned fo = field * t->field_bytes;
  int g = granule_of(t->field_bytes, values, defaults);
  if (fo) g = std::min(g, granule_of(fo, nullptr, nullptr));
  constexpr int U = 4;
  size_t waves = (n + 4 * U - 1) / (4 * U);
  dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const i64* k = (const i64*)keys;
  unsigned char* o = (unsigned char*)values;
  const unsigned char* d = (const unsigned char*)defaults;
  const long long* dn = (const long long*)d_n;
  with_granule(g, [&](auto G) {
    if constexpr (G == 16) {   // a dense table: both home-bucket lines of a key in flight together (PF1)
      if (t->dense) { find_kernel<16, U, true, true><<<grid, block, 0, s>>>(v, n, k, o, exists, d, full, fo, dn); return; }
    }
    find_kernel<G, U><<<grid, block, 0, s>>>(v, n, k, o, exists, d, full, fo, dn);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

// ------------------------------------ C ABI --------------------------------------------------
extern "C" {

const char* tfra_last_error(void) { return g_last_error.c_str(); }
int tfra_abi_version(void) { return TFRA_ABI_VERSION; }

int tfra_table_create(const tfra_table_opts* o, const tfra_allocator* alloc, tfra_table_t** out) {
  if (!o || !out) return set_error(TFRA_ERR_INVALID, "null argument");
  if (o->struct_size != sizeof(tfra_table_opts)) return set_error(TFRA_ERR_INVALID, "tfra_table_opts size mismatch (ABI)");
  size_t es = dtype_size(o->value_dtype);
  if (!es) return set_error(TFRA_ERR_INVALID, "unsupported value_dtype");
  if (o->dim <= 0) return set_error(TFRA_ERR_INVALID, "dim must be positive");
  if (o->aux_fields < 0 || o->aux_fields > 4) return set_error(TFRA_ERR_INVALID, "aux_fields must be in [0,4]");
  if (o->strategy < -1 || o->strategy > 4) return set_error(TFRA_ERR_INVALID, "unknown eviction strategy");
  Table* t = new Table();
  t->opts = *o;
  if (alloc) t->alloc = *alloc;
  int dev = o->device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) { delete t; return set_error(TFRA_ERR_HIP, "no HIP device"); }
  t->device = dev;
  if (hipSetDevice(dev) != hipSuccess) { delete t; return set_error(TFRA_ERR_HIP, "hipSetDevice failed"); }
  // hkv_hashtable_op_gpu.cu.cc:121-133: init 0 -> default, max < init -> max = init
  if (t->opts.init_capacity == 0) t->opts.init_capacity = t->opts.max_capacity ? (1ULL << 20) : 8192;
  if (t->opts.max_capacity && t->opts.max_capacity < t->opts.init_capacity) t->opts.max_capacity = t->opts.init_capacity;
  if (t->opts.max_load_factor <= 0.f || t->opts.max_load_factor > 1.f)
    t->opts.max_load_factor = t->opts.max_capacity ? 0.5f : 0.75f;
  t->field_bytes = (unsigned)(o->dim * es);
  t->row_stride = (unsigned)(((size_t)t->field_bytes * (1 + o->aux_fields) + 15) / 16 * 16);
  t->aux = make_aux_init(t->opts);
  hipStream_t s = nullptr;
  auto fail = [&](int rc) { tfra_table_destroy(reinterpret_cast<tfra_table_t*>(t)); return rc; };
  size_t ctr_bytes = (SIZE_SHARDS * SIZE_SHARD_STRIDE) * sizeof(u64);
  t->size_shards = (u64*)t->dalloc(ctr_bytes, s);
  t->reserved_present = (unsigned*)t->dalloc(64, s);  // [0,1] sentinel-key presence | +8 err_count | +10 dense flag | +12 two i64 scalars
  if (!t->size_shards || !t->reserved_present) return fail(set_error(TFRA_ERR_OOM, "counter allocation failed"));
  t->err_count = t->reserved_present + 8;
  t->d_dense = t->reserved_present + 10;
  t->d_scalar = (i64*)(t->reserved_present + 12);
  if (hipHostMalloc((void**)&t->h_scalar, 64) != hipSuccess) return fail(set_error(TFRA_ERR_OOM, "pinned scalar"));
  if (hipHostMalloc((void**)&t->own_stats_host, 64) != hipSuccess) { t->own_stats_host = nullptr; return fail(set_error(TFRA_ERR_OOM, "pinned sample words")); }
  t->own_stats_host[0] = t->own_stats_host[1] = 0;   // (allocated here, not at the first write-back: that one may run under stream capture)
  if (hipEventCreateWithFlags(&t->chain_event, hipEventDisableTiming) != hipSuccess) return fail(set_error(TFRA_ERR_HIP, "event"));
  if (hipEventCreateWithFlags(&t->size_event, hipEventDisableTiming) != hipSuccess) return fail(set_error(TFRA_ERR_HIP, "event"));
  t->h_size = t->h_scalar + 4;
  u64 nb = std::max<u64>(2, (u64)((double)t->opts.init_capacity / t->opts.max_load_factor / SLOTS) + 1);
  nb = t->lattice_nb(nb);   // bounded tables: slots <= max_capacity, and doublings end exactly there
  int rc = t->alloc_storage(nb, &t->cur, s);
  if (rc) return fail(rc);
  t->enqueue_clear(t->cur, true, s);
  if (hipStreamSynchronize(s) != hipSuccess) return fail(set_error(TFRA_ERR_HIP, "clear failed"));
  *out = reinterpret_cast<tfra_table_t*>(t);
  return TFRA_OK;
}

int tfra_table_destroy(tfra_table_t* tp) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return TFRA_OK;
  (void)hipSetDevice(t->device);
  (void)hipDeviceSynchronize();
  hipStream_t s = nullptr;
  destroy_own_plan(t);
  t->free_storage(t->cur, s);
  t->dfree(t->size_shards, s); t->dfree(t->reserved_present, s);
  t->dfree(t->winner, s); t->dfree(t->scratch, s); t->dfree(t->evict_flags, s); t->dfree(t->own_tags, s); t->dfree(t->own_ws, s);
  if (t->progress_host) (void)hipHostFree(t->progress_host);
  if (t->own_stats_host) (void)hipHostFree(t->own_stats_host);
  if (t->h_scalar) (void)hipHostFree(t->h_scalar);
  if (t->chain_event) (void)hipEventDestroy(t->chain_event);
  if (t->size_event) (void)hipEventDestroy(t->size_event);
  delete t;
  return TFRA_OK;
}

int tfra_table_find(tfra_table_t* tp, size_t n, const int64_t* keys, void* values, uint8_t* exists,
                    const void* defaults, int default_is_full, tfra_stream_t stream) {
  TABLE_ENTER();
  return find_impl(t, s, 0, n, keys, values, exists, defaults, default_is_full);
}

int tfra_table_find_n(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, void* values, uint8_t* exists,
                      const void* defaults, int default_is_full, tfra_stream_t stream) {
  TABLE_ENTER();
  if (!d_n) return set_error(TFRA_ERR_INVALID, "find_n: null count");
  return find_impl(t, s, 0, n, keys, values, exists, defaults, default_is_full, d_n);
}

int tfra_table_find_field(tfra_table_t* tp, int field, size_t n, const int64_t* keys, void* values,
                          uint8_t* exists, const void* defaults, int default_is_full, tfra_stream_t stream) {
  TABLE_ENTER();
  return find_impl(t, s, field, n, keys, values, exists, defaults, default_is_full);
}

int tfra_table_erase(tfra_table_t* tp, size_t n, const int64_t* keys, tfra_stream_t stream) {
  TABLE_ENTER();
  if (n == 0) return TFRA_OK;
  if (!keys) return set_error(TFRA_ERR_INVALID, "erase: null keys");
  erase_kernel<<<(unsigned)((n * 16 + 255) / 256), 256, 0, s>>>(t->view_of(t->cur), n, (const i64*)keys);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_table_clear(tfra_table_t* tp, tfra_stream_t stream) {
  TABLE_ENTER();
  t->enqueue_clear(t->cur, true, s);
  HIP_TRY(hipGetLastError());
  t->size_ub = 0;
  t->size_pending = false;
  t->n_since_read = 0;
  t->dense = false;
  return TFRA_OK;
}

int tfra_table_size(tfra_table_t* tp, size_t* out, tfra_stream_t stream) {
  TABLE_ENTER();
  if (!out) return set_error(TFRA_ERR_INVALID, "size: null out");
  int rc = t->read_size(s, out);
  if (rc) return rc;
  return t->check_errors(s);
}

int tfra_table_size_to_device(tfra_table_t* tp, int64_t* d_out, tfra_stream_t stream) {
  TABLE_ENTER();
  if (!d_out) return set_error(TFRA_ERR_INVALID, "size: null out");
  t->enqueue_size((i64*)d_out, s);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

int tfra_table_check_errors(tfra_table_t* tp, tfra_stream_t stream) {
  TABLE_ENTER();
  return t->check_errors(s);
}

int tfra_table_capacity(tfra_table_t* tp, size_t* out) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t || !out) return set_error(TFRA_ERR_INVALID, "capacity: null argument");
  std::lock_guard<std::mutex> lock(t->mu);
  *out = t->cur.nb * SLOTS + NUM_RESERVED;
  return TFRA_OK;
}

int tfra_table_set_option(tfra_table_t* tp, int option, int64_t value) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "null table");
  std::lock_guard<std::mutex> lock(t->mu);
  if (option == TFRA_OPTION_CAPTURE_SAFE) { t->capture_safe = value != 0; return TFRA_OK; }
  if (option == TFRA_OPTION_NO_OWNER_TAGS) { t->no_owner_tags = value != 0; return TFRA_OK; }
  if (option == TFRA_OPTION_KEY_BYTES_ON_DISK) {
    if (value != 4 && value != 8) return set_error(TFRA_ERR_INVALID, "TFRA_OPTION_KEY_BYTES_ON_DISK: 4 or 8");
    t->key_file_bytes = (int)value;
    return TFRA_OK;
  }
  if (option == TFRA_OPTION_STOCHASTIC_ROUNDING) {
    if (value != 0 && t->opts.value_dtype != TFRA_F16 && t->opts.value_dtype != TFRA_BF16)
      return set_error(TFRA_ERR_UNSUPPORTED, "set_option: TFRA_OPTION_STOCHASTIC_ROUNDING needs a float16 or bfloat16 table");
    t->sr_seed = (uint64_t)value;
    t->sr_call = 0;
    return TFRA_OK;
  }
  return set_error(TFRA_ERR_INVALID, "unknown option");
}

int tfra_table_set_global_epoch(tfra_table_t* tp, uint64_t epoch) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "null table");
  std::lock_guard<std::mutex> lock(t->mu);
  t->global_epoch = epoch;
  return TFRA_OK;
}

}  // extern "C"
