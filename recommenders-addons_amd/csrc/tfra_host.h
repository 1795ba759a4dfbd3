// Host-side table object behind the opaque tfra_table_t handle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_optim_device.h"

namespace tfra {

extern thread_local std::string g_last_error;
int set_error(int code, const std::string& msg);

// HIP_TRY_AS: the error text names `what` instead of the expression
#define HIP_TRY_AS(what, expr)                                                                \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return set_error(_e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP,                \
                       std::string(what) + ": " + hipGetErrorString(_e));                     \
  } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(#expr, expr)

// Makes `device` the calling thread's device: hipSuccess, or why it could not.  hipSetDevice costs tens of microseconds on
// ROCm 7.2 — more than the find kernel itself — so it is only issued when the calling thread is on another device.  (The
// destroy paths' unconditional hipSetDevice is another thing: they cannot report a failure and do not care for the cost.)
static inline hipError_t on_device(int device) {
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur == device) return hipSuccess;
  return hipSetDevice(device);
}

// head of a C entry point of the table units (tfra_table / tfra_grow / tfra_upsert / tfra_find_insert / tfra_accum / tfra_scan .hip): handle `tp`, `stream`
#define TABLE_ENTER()                                         \
  Table* t = reinterpret_cast<Table*>(tp);                    \
  if (!t) return set_error(TFRA_ERR_INVALID, "null table");   \
  hipStream_t s = (hipStream_t)stream;                        \
  std::lock_guard<std::mutex> lock(t->mu);                    \
  { int _rc = t->enter(s); if (_rc) return _rc; }

struct Storage {
  unsigned char* base = nullptr;  // nb bucket blocks [key line | score line | 15 rows] + 2 side rows
  u64 nb = 0;
  // big tables: physical memory mapped chunk by chunk into ONE reserved virtual range (hipMemAddressReserve / hipMemMap),
  // so that growth maps more memory behind the table and splits the buckets in place (Table::grow_in_place)
  bool vmm = false;
  size_t va_bytes = 0, mapped = 0, chunk_bytes = 0;   // every chunk has the same size (see vmm_map_more)
  std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> chunks;
};

struct AuxInitPod {
  unsigned elem_bytes;
  unsigned pattern[4];
};

struct Table {
  tfra_table_opts opts{};
  tfra_allocator alloc{nullptr, nullptr, nullptr};
  int device = 0;
  unsigned field_bytes = 0, row_stride = 0;
  Storage cur;
  u64* size_shards = nullptr;
  unsigned* reserved_present = nullptr;  // [2] + err_count + d_scalar in one 64-B block
  unsigned* err_count = nullptr;
  unsigned* d_dense = nullptr;  // TableView::dense_flag
  i64* d_scalar = nullptr;
  i64* h_scalar = nullptr;  // pinned
  unsigned* progress_host = nullptr;  // tfra_table_step_prefetch: pinned progress counter of the main stream
  unsigned* own_stats_host = nullptr; // pinned: [0] keys that were NOT plain hits, [1] keys looked at — a sample (every 16th wave) of the last
                                      // ownership write-back of a SET plan that has ended: picks the pass's form for the next one (launch_own)
  unsigned step_gen = 0;
  std::mutex step_mu;
  uint8_t* evict_flags = nullptr;  // phase-2 flags of a fused write-back on a bounded table
  size_t evict_flags_cap = 0;
  int* winner = nullptr;
  size_t winner_len = 0;
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  void* own_plan = nullptr;  // tfra_sparse_plan of the one-call write-backs (tfra_table_apply_sparse / upsert_sparse)
  void* big_ws = nullptr;    // tfra_workspace of tfra_table_apply_sparse with more than 2^18 ids
  void* comb_ws = nullptr;   // tfra_workspace of tfra_table_apply_planned_combined (the entries' combiner records)
  unsigned* own_tags = nullptr;  // [nb] bucket-owner tags (upsert_own_kernel), allocated on first use
  u64 own_tags_nb = 0;
  unsigned own_gen = 0;      // bucket-owner tag of the last ownership-based write-back (upsert_own_kernel)
  void* own_ws = nullptr;    // scratch of the ownership pass over a caller's unique keys (own_upsert_unique): counters | items | flags
  size_t own_ws_bytes = 0;
  unsigned own_ws_uses = 0;
  unsigned apply_P = 0;      // bucket count the cursor area at the head of `scratch` is armed for (0 = not armed)
  AuxInitPod aux{};
  // host bookkeeping
  std::mutex mu;
  size_t size_ub = 0;  // upper bound of the live-key count (exact after read_size)
  hipStream_t last_stream = nullptr;
  bool has_last = false;
  hipEvent_t chain_event = nullptr;
  hipEvent_t size_event = nullptr;  // async size refresh (prepare_insert)
  bool size_pending = false;
  size_t n_since_read = 0;
  i64* h_size = nullptr;  // pinned, inside the h_scalar block
  bool growth_blocked = false;
  bool dense = false;        // a table that cannot grow any more holds > 60 % of its slots (async size reads)
  bool capture_safe = false;  // TFRA_OPTION_CAPTURE_SAFE
  bool no_owner_tags = false; // TFRA_OPTION_NO_OWNER_TAGS
  int key_file_bytes = 8;     // TFRA_OPTION_KEY_BYTES_ON_DISK
  uint64_t global_epoch = 0;
  int64_t curr_step = 1;
  bool epoch_hold = false;   // see step_epoch
  uint64_t sr_seed = 0;      // TFRA_OPTION_STOCHASTIC_ROUNDING: 0 = off (nearest even), else the seed of the half rows' rounding bits
  uint64_t sr_call = 0;      // fused write-backs since the option was set (step_writeback): the call index of the next one
  int n_rehash = 0;

  void* dalloc(size_t bytes, hipStream_t s);
  void dfree(void* p, hipStream_t s);
  int alloc_storage(u64 nb, Storage* st, hipStream_t s);
  TableView view_of(const Storage& st) const;
  int enter(hipStream_t s);
  int read_size(hipStream_t s, size_t* out);
  int check_errors(hipStream_t s);
  int ensure_winner(hipStream_t s);
  unsigned* ensure_own_tags(hipStream_t s);
  int ensure_scratch(size_t bytes, hipStream_t s);
  int grow(u64 min_nb, hipStream_t s);
  u64 lattice_nb(u64 min_nb) const;
  bool at_max_capacity() const;
  int grow_in_place(u64 min_nb, hipStream_t s);   // TFRA_ERR_UNSUPPORTED: not possible here, copy instead
  void free_storage(Storage& st, hipStream_t s);
  int n_split = 0;                                // in-place growths so far
  int prepare_insert(size_t n, hipStream_t s);
  int poll_density(size_t n, hipStream_t s);
  int bounded_flags(size_t n, hipStream_t s, uint8_t** out);
  void enqueue_clear(const Storage& st, bool reset_counters, hipStream_t s);   // clear_kernel <<<2048, 256>>> (tfra_table.hip)
  void enqueue_size(i64* d_out, hipStream_t s);                                // size_kernel <<<1, SIZE_SHARDS>>> of `cur`
  // geometry: a bucket block is [key line | score line (scored tables) | SLOTS rows]; the side rows follow the last block
  unsigned hdr_bytes() const { return opts.strategy >= 0 ? 256u : 128u; }
  size_t bucket_stride() const { return (size_t)hdr_bytes() + (size_t)SLOTS * row_stride; }
  size_t storage_bytes(u64 nb) const { return nb * bucket_stride() + (size_t)NUM_RESERVED * row_stride; }
  u64 max_nb() const { return std::max<u64>(2, opts.max_capacity / SLOTS); }   // (max_capacity == 0, unbounded: the caller's case)
  void step_epoch() {   // one upsert, or one fused write-back, is one step of the epoch strategies (lookup_table_op_hkv.h:528-536)
    if (epoch_hold) return;   // one logical write-back issued as several launches (apply_sparse_big): stepped once by the caller
    if (opts.strategy != TFRA_EVICT_EPOCHLRU && opts.strategy != TFRA_EVICT_EPOCHLFU) return;
    curr_step += 1;
    if (opts.step_per_epoch > 0 && curr_step > opts.step_per_epoch) { global_epoch += 1; curr_step = 1; }
  }
  // behind a FUSED OPTIMIZER write-back that passed its checks and had work to do: step_epoch, and one call of the stochastic
  // rounding's random stream (held like the epoch while one logical write-back is issued in parts)
  void step_writeback() {
    step_epoch();
    if (!epoch_hold) sr_call += 1;
  }
  bool stochastic() const { return sr_seed != 0; }
  StochP stoch_of() const { return StochP{sr_mix64(sr_seed + sr_call * SR_GAMMA)}; }   // `a` of this call (tfra_optim_device.h)
};

// The kernels' forms of a caller's optimizer parameters and of the table's score state.  at_capacity: whether Table::bounded_flags
// handed out flag bytes (a bounded table that cannot grow any more: the write-back runs its eviction phase); 2 = such a table is
// also dense (locate_or_claim_from).
static inline OptP opt_of(const tfra_opt_params* p) {
  return OptP{p->kind, p->lr, p->beta1, p->beta2, p->eps, p->l1, p->l2, p->lr_power, p->d_lr};
}
static inline int bounded_mode(const Table* t, bool at_capacity) { return at_capacity ? (t->dense ? 2 : 1) : 0; }
static inline ScoreP score_of(const Table* t, const uint8_t* flags) {
  return ScoreP{t->opts.strategy, t->global_epoch, bounded_mode(t, flags != nullptr)};
}

// Scratch of ONE call: the device and pinned allocations made through it live until the holder goes out of scope.  Its destructor
// synchronises the call's stream once — a copy or a kernel queued there may still use the memory — and frees them, on every way
// out of the function.  false: the allocation failed (the pointer is null, the caller reports it in its own words).
struct Scratch {
  hipStream_t s;
  std::vector<std::pair<void*, bool>> held;   // (pointer, pinned)
  explicit Scratch(hipStream_t stream) : s(stream) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  template <class T>
  bool take(T** p, size_t bytes, bool pinned) {
    *p = nullptr;
    if ((pinned ? hipHostMalloc((void**)p, bytes, hipHostMallocDefault) : hipMalloc((void**)p, bytes)) != hipSuccess) { *p = nullptr; return false; }
    held.emplace_back(*p, pinned);
    return true;
  }
  template <class T> bool device(T** p, size_t bytes) { return take(p, bytes, false); }
  template <class T> bool pinned(T** p, size_t bytes) { return take(p, bytes, true); }
  ~Scratch() {
    if (!held.empty()) (void)hipStreamSynchronize(s);
    for (auto& h : held) (void)(h.second ? hipHostFree(h.first) : hipFree(h.first));
  }
};

// Argument check shared by the score-filtered calls (tfra_scan.hip): TFRA_ERR_INVALID for a null table or an unknown predicate,
// TFRA_ERR_UNSUPPORTED for a table without a score line; the message names `fn`.  Enqueues nothing.
int score_filter_check(const Table* t, int pred, const char* fn);
void destroy_own_plan(Table* t);   // tfra_csr.hip
// insert_or_assign of UNIQUE keys as one ownership pass (tfra_own.hip); *taken = false: not applicable, run the locked kernels
int own_upsert_unique(Table* t, hipStream_t s, size_t n, const i64* keys, const void* values, const u64* scores, bool* taken,
                      const uint8_t* accum_exists = nullptr, const int64_t* d_n = nullptr);   // accum_exists: insert_or_accum instead of an assign
void destroy_workspace_plan(void* plan);   // tfra_csr.hip
void destroy_workspace_many(void* stage);  // tfra_pool.hip

// Copy granule of rows of `bytes` bytes between two buffers: the largest power of two <= 16 that divides the row size and both
// addresses (a null pointer divides everything).
static inline int granule_of(size_t bytes, const void* a, const void* b) {
  size_t x = bytes | (size_t)(uintptr_t)a | (size_t)(uintptr_t)b | 16;
  int g = (int)(x & (~x + 1));
  return g > 16 ? 16 : g;
}
// f(std::integral_constant<int, G>{}) for the granule G in {16, 8, 4, 2, 1} that g selects (anything else: 1): one launch ladder
// for the kernels templated on their granule
template <class F>
static inline void with_granule(int g, F&& f) {
  switch (g) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{}); break;
  }
}

// f(std::integral_constant<int, DT>{}) for the value dtype DT (tfra_dtype) that dt selects (anything else: TFRA_F64)
template <class F>
static inline void with_dtype(int dt, F&& f) {
  switch (dt) {
    case TFRA_F32: f(std::integral_constant<int, TFRA_F32>{}); break;
    case TFRA_F16: f(std::integral_constant<int, TFRA_F16>{}); break;
    case TFRA_BF16: f(std::integral_constant<int, TFRA_BF16>{}); break;
    case TFRA_I8: f(std::integral_constant<int, TFRA_I8>{}); break;
    case TFRA_I32: f(std::integral_constant<int, TFRA_I32>{}); break;
    case TFRA_I64: f(std::integral_constant<int, TFRA_I64>{}); break;
    default: f(std::integral_constant<int, TFRA_F64>{}); break;
  }
}

// The fused kernels' storage types as an index: 0 float32, 1 float16, 2 bfloat16 (the caller has refused every other dtype)
static inline int st_index(int dtype) { return dtype == TFRA_F16 ? 1 : dtype == TFRA_BF16 ? 2 : 0; }
// One launch ladder per template axis (as with_granule), for single-table and grouped launchers alike: storage type, rule
template <class F>
static inline void with_stored(int st, F&& f) {
  switch (st) {
    case 1: f(std::integral_constant<int, TFRA_F16>{}); break;
    case 2: f(std::integral_constant<int, TFRA_BF16>{}); break;
    default: f(std::integral_constant<int, TFRA_F32>{}); break;
  }
}
template <class F>
static inline void with_opt_kind(int kind, F&& f) {
  switch (kind) {
    case TFRA_OPT_SGD: f(std::integral_constant<int, TFRA_OPT_SGD>{}); break;
    case TFRA_OPT_ADAM: f(std::integral_constant<int, TFRA_OPT_ADAM>{}); break;
    case TFRA_OPT_ADAGRAD: f(std::integral_constant<int, TFRA_OPT_ADAGRAD>{}); break;
    case TFRA_OPT_MOMENTUM: f(std::integral_constant<int, TFRA_OPT_MOMENTUM>{}); break;
    case TFRA_OPT_NESTEROV: f(std::integral_constant<int, TFRA_OPT_NESTEROV>{}); break;
    case TFRA_OPT_RMSPROP: f(std::integral_constant<int, TFRA_OPT_RMSPROP>{}); break;
    default: f(std::integral_constant<int, TFRA_OPT_FTRL>{}); break;   // (the callers have refused every kind that is not one of the seven)
  }
}

}  // namespace tfra

// Scratch of the front-end ops (tfra_workspace_create): one growing device buffer per caller stream.
struct tfra_workspace {
  int device = 0;
  void* buf = nullptr;
  size_t bytes = 0;
  void* plan = nullptr;   // tfra_sparse_plan of tfra_reduce_by_key
  void* uplan = nullptr;  // tfra_sparse_plan of tfra_unique_unordered and tfra_table_find_unique (tfra::workspace_uplan)
  unsigned* h_err = nullptr;   // pinned: polls of the one-launch unique that timed out (reported by the NEXT tfra_unique_unordered call)
  // tfra_unique (up to 2^20 ids): two persistent hash sets that alternate and empty each other (no fill kernel per call)
  void* unq_buf = nullptr;
  size_t unq_cap = 0, unq_nmax = 0;
  unsigned unq_parity = 0, unq_gen = 0;
  // the sets persist from call to call: a call on ANOTHER stream than the previous one is ordered behind it by an event
  hipStream_t unq_stream = nullptr;
  bool unq_stream_set = false;
  hipEvent_t unq_ev = nullptr;
  // tfra_multi_unique (tfra_unique_many.hip): the same state once more, of its own — two sets of unqm_slots slots that the call's
  // lists share as sub-sets, room for unqm_nmax ids and unqm_tiles scatter tiles in all; tfra_unique's sets above are not touched by it
  void* unqm_buf = nullptr;
  size_t unqm_slots = 0, unqm_nmax = 0, unqm_tiles = 0;
  unsigned unqm_parity = 0, unqm_gen = 0;
  hipStream_t unqm_stream = nullptr;
  bool unqm_stream_set = false;
  hipEvent_t unqm_ev = nullptr;
  void* many = nullptr;   // pinned staging ring of the grouped calls' descriptor records (ManyStage, tfra_many.h)
  int ensure(size_t need, hipStream_t s) {
    if (need <= bytes) return TFRA_OK;
    if (buf) {
      if (hipStreamSynchronize(s) != hipSuccess || hipFree(buf) != hipSuccess) return tfra::set_error(TFRA_ERR_HIP, "workspace: free failed");
      buf = nullptr; bytes = 0;
    }
    size_t want = need > ((size_t)1 << 20) ? need : ((size_t)1 << 20);
    hipError_t e = hipMalloc(&buf, want);
    if (e != hipSuccess) { buf = nullptr; return tfra::set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, "workspace: hipMalloc failed"); }
    bytes = want;
    return TFRA_OK;
  }
};

namespace tfra {
// The helper object an owner (a table, a workspace) keeps in a void* slot, created on `device` on first use: a workspace, a plan.
// A create call that fails has recorded its own error; the slot stays null.
static inline int workspace_in(void** slot, int device, tfra_workspace_t** out) {
  if (!*slot) {
    tfra_workspace_t* w = nullptr;
    int rc = tfra_workspace_create(device, &w);
    if (rc) return rc;
    *slot = w;
  }
  *out = reinterpret_cast<tfra_workspace_t*>(*slot);
  return TFRA_OK;
}
static inline int plan_in(void** slot, int device, tfra_sparse_plan_t** out) {
  if (!*slot) {
    tfra_sparse_plan_t* pl = nullptr;
    int rc = tfra_sparse_plan_create(device, &pl);
    if (rc) return rc;
    *slot = pl;
  }
  *out = reinterpret_cast<tfra_sparse_plan_t*>(*slot);
  return TFRA_OK;
}
// The workspace's plan object of tfra_unique_unordered / tfra_table_find_unique
static inline int workspace_uplan(tfra_workspace* ws, tfra_sparse_plan_t** out) { return plan_in(&ws->uplan, ws->device, out); }
}  // namespace tfra
