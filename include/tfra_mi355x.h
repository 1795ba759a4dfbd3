/* tfra_mi355x.h — C ABI of the MI355X-native dynamic-embedding table engine.
 *
 * This is the drop-in boundary: exactly the surface TFRA's GPU adapter
 * (`gpu::TableWrapper<K,V>`) needs from its storage engine, plus the fused extras that
 * replace multi-op sequences of the reference.  Plain pointers and sizes only; all device
 * pointers are HIP device pointers on the table's device; `stream` is a `hipStream_t`
 * passed as `void*`.  Every entry point returns 0 on success or a negative tfra_status and
 * never throws; `tfra_last_error()` returns a thread-local message.  All table operations
 * are STREAM-ORDERED and do not synchronise the host unless documented.
 *
 * Reference files (R = /root/reference/tensorflow_recommenders_addons/dynamic_embedding/core):
 *   R/kernels/lookup_impl/lookup_table_op_hkv.h   gpu::TableWrapper  (what calls the engine)
 *   R/kernels/hkv_hashtable_op_gpu.cu.cc          HkvHashTableOfTensorsGpu (TF op kernels)
 *   R/kernels/cuckoo_hashtable_op.cc              CuckooHashTableOfTensors (CPU semantics =
 *                                                 the result oracle)
 *   R/ops/hkv_hashtable_ops.cc                    op names / attrs
 */
#ifndef TFRA_MI355X_H_
#define TFRA_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFRA_ABI_VERSION 1

typedef struct tfra_table tfra_table_t;
typedef void* tfra_stream_t; /* hipStream_t */

typedef enum {
  TFRA_OK = 0,
  TFRA_ERR_INVALID = -1,   /* bad argument / shape / dtype (TF: InvalidArgument)          */
  TFRA_ERR_OOM = -2,       /* allocation failed                                            */
  TFRA_ERR_HIP = -3,       /* HIP runtime error (TF: Internal)                             */
  TFRA_ERR_FULL = -4,      /* table at max_capacity and key could not be placed            */
  TFRA_ERR_IO = -5,        /* KV-file save/load failed                                     */
  TFRA_ERR_UNSUPPORTED = -6
} tfra_status;

/* value dtypes registered for the GPU ops: K=int64 x V in {float, int8, int32, int64, half,
 * bfloat16} (R/kernels/hkv_hashtable_op_gpu.cu.cc:1133-1138); double is the CPU table's extra
 * (R/kernels/cuckoo_hashtable_op.cc:995-1014). */
typedef enum {
  TFRA_F32 = 0, TFRA_F16 = 1, TFRA_BF16 = 2, TFRA_I8 = 3, TFRA_I32 = 4, TFRA_I64 = 5, TFRA_F64 = 6
} tfra_dtype;

/* eviction strategy enum 0..4 as in R/kernels/lookup_impl/lookup_table_op_hkv.h:454-475 and
 * PY/dynamic_embedding_creator.py:141-146; -1 = never evict (libcuckoo semantics: grow). */
typedef enum {
  TFRA_EVICT_NONE = -1, TFRA_EVICT_LRU = 0, TFRA_EVICT_LFU = 1, TFRA_EVICT_EPOCHLRU = 2,
  TFRA_EVICT_EPOCHLFU = 3, TFRA_EVICT_CUSTOMIZED = 4
} tfra_evict_strategy;

/* Mirrors TableWrapperInitOptions (R/kernels/lookup_impl/lookup_table_op_hkv.h:304-315) and
 * the creator-op attrs (R/ops/hkv_hashtable_ops.cc:318-339).  POD, versioned by struct_size. */
typedef struct {
  uint32_t struct_size;           /* = sizeof(tfra_table_opts)                               */
  int32_t value_dtype;            /* tfra_dtype                                              */
  int32_t dim;                    /* value_shape[0]                                          */
  int32_t aux_fields;             /* S co-located per-key state vectors of `dim` elements
                                     (optimizer slots m,v / accum,linear); 0 for a plain table */
  uint64_t init_capacity;         /* attr init_capacity / init_size; 0 -> 1 Mi
                                     (hkv_hashtable_op_gpu.cu.cc:53) or 8192 for cuckoo flavour */
  uint64_t max_capacity;          /* attr max_capacity; 0 = unbounded (libcuckoo flavour)   */
  uint64_t max_hbm_for_vectors;   /* accepted for attr parity and ignored; two tiers: tfra_tier_* */
  float max_load_factor;          /* growth trigger; 0 -> 0.5 like lookup_table_op_hkv.h:449
                                     when max_capacity>0, 0.75 for the unbounded flavour     */
  int32_t strategy;               /* tfra_evict_strategy                                     */
  int64_t step_per_epoch;         /* EPOCH* strategies (lookup_table_op_hkv.h:528-536)       */
  int32_t reserved_key_start_bit; /* accepted for attr parity: this engine stores EVERY int64
                                     key (libcuckoo parity), nothing is reserved             */
  int32_t device;                 /* HIP device ordinal; -1 = current                        */
  float aux_init[4];              /* initial value of every element of aux field f + 1 of a newly inserted key,
                                     converted to value_dtype once at create: F32 as is; F16 and BF16 rounded
                                     to nearest even; I32 and I8 truncated toward zero; I64 and F64 tables
                                     IGNORE it: their aux fields start at 0                  */
} tfra_table_opts;

/* Allocation bridge = TFOrDefaultAllocator (lookup_table_op_hkv.h:329-426): lets the host
 * framework own the bytes.  NULL -> hipMalloc/hipFree. kind: 0 device, 1 pinned host, 2 host. */
typedef struct {
  void* (*alloc)(void* user, int kind, size_t bytes, tfra_stream_t stream);
  void (*free)(void* user, int kind, void* ptr, tfra_stream_t stream);
  void* user;
} tfra_allocator;

/* flags for insert / accum */
#define TFRA_FLAG_UNIQUE_KEYS 1u /* caller guarantees no duplicate keys in this call (HKV's
                                    contract, PY/dynamic_embedding_variable.py:1377-1378):
                                    single-pass fast path. Without it duplicates resolve like the
                                    single-threaded reference: the LAST occurrence wins.        */

const char* tfra_last_error(void);
int tfra_abi_version(void);

/* -- lifetime: HashTableGpuOp / ResourceMgr own one handle per (shard, variable)
 *    (R/kernels/cuckoo_hashtable_op_gpu.h:43-139); init = lookup_table_op_hkv.h:435-520 ------ */
int tfra_table_create(const tfra_table_opts* opts, const tfra_allocator* alloc, tfra_table_t** out);
int tfra_table_destroy(tfra_table_t* t);

/* -- find = TableWrapper::get (lookup_table_op_hkv.h:719-732) with the default pre-fill FUSED:
 *    values[i,:] = hit ? row : (default_is_full ? defaults[i,:] : defaults[0,:]);
 *    exists[i] (may be NULL) = hit.  Duplicate keys allowed.  Never inserts.
 *    Result oracle: TableWrapperOptimized::find (lookup_table_op_cpu.h:188-217).           */
int tfra_table_find(tfra_table_t* t, size_t n, const int64_t* keys, void* values, uint8_t* exists,
                    const void* defaults, int default_is_full, tfra_stream_t stream);

/* -- insert_or_assign = TableWrapper::upsert (lookup_table_op_hkv.h:522-537); scores NULL or
 *    [n] (HkvHashTableInsert's `scores` input, empty tensor -> NULL).  Advances the epoch
 *    counter for EPOCH* strategies.  Oracle: LaunchTensorsInsert (cuckoo_hashtable_op.cc:111).
 *    With TFRA_FLAG_UNIQUE_KEYS (what the Insert op passes: HKV's contract) the call is ONE pass
 *    with bucket ownership over the caller's keys (the kernels of tfra_table_upsert_planned, no
 *    plan); a bulk load — so many keys for the table's size that most would collide on a home
 *    bucket — and calls without the flag take the locked kernels.  Same results either way.
 *    A bounded (Hkv) table at max_capacity: a key that finds neither itself nor an empty slot replaces the minimum-score
 *    entry among the 30 slots of its two home buckets (ties: the first home bucket before the second; an empty slot before
 *    any victim).  LFU / EPOCHLFU / CUSTOMIZED admit the key only if its compare score (the caller's score; EPOCHLFU:
 *    epoch << 32 | score) is >= that minimum — else it is dropped, no error, nothing changes.  The replaced slot starts a new
 *    life: the new key's LFU count is its own score, aux fields are at aux_init.  Without TFRA_FLAG_UNIQUE_KEYS the call (and
 *    tfra_table_accum_or_assign) returns TFRA_ERR_UNSUPPORTED there and changes nothing.  (tests/test_gpu_eviction.py)      */
int tfra_table_insert_or_assign(tfra_table_t* t, size_t n, const int64_t* keys, const void* values,
                                const uint64_t* scores, uint32_t flags, tfra_stream_t stream);

/* -- The same two ops with the key COUNT on the device: n = the length of the buffers, *d_n (a device int64, or pinned host
 *    memory the device can read) = the number of keys in them; min(n, *d_n) keys are looked up / written.  For the chain
 *    tfra_unique_unordered -> Find -> gather -> Insert of embedding_lookup (python/ops/dynamic_embedding_ops.py:99-117), where the
 *    count is only the SHAPE of tf.unique's output: the host reads it while these calls already run.  insert_or_assign_n takes
 *    unique keys (TFRA_FLAG_UNIQUE_KEYS semantics, the Insert op's contract) through the single-pass write-back and returns
 *    TFRA_ERR_UNSUPPORTED when that pass cannot take the call (owner tags off, a bulk load): read the count and call the plain
 *    entry point then.  A growing table sizes itself by n, the upper bound.                                                    */
int tfra_table_find_n(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys, void* values, uint8_t* exists,
                      const void* defaults, int default_is_full, tfra_stream_t stream);
int tfra_table_insert_or_assign_n(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys, const void* values,
                                  const uint64_t* scores, tfra_stream_t stream);

/* -- insert_and_evict (HierarchicalKV's insert_and_evict): an insert that hands back what it displaces, for a host or SSD tier
 *    below HBM, eviction metrics, or re-admission with the old row.
 *    The write is tfra_table_insert_or_assign(t, n, keys, values, scores, TFRA_FLAG_UNIQUE_KEYS, stream): unique keys, the
 *    embedding field, the same epoch stepping, the same victim and admission rule, a new life for the replaced slot; the table
 *    ends as that call would leave it.
 *    Reported: EVERY entry that leaves the table because of this call is appended at *d_evicted_counter as a triple
 *    (key, row, score): the row in the table's value dtype with the bytes it held when it left, the score the uint64
 *    tfra_table_export_batch would have reported for it at that moment.  A key that is NOT admitted (LFU / EPOCHLFU /
 *    CUSTOMIZED, compare score below the minimum of its home buckets) is reported too, as (the key, the caller's row, its
 *    compare score — EPOCHLFU: epoch << 32 | score): nothing the caller handed in or had resident is lost.  A key that takes
 *    an empty slot reports nothing; a key that cannot be placed at all counts in tfra_table_check_errors as for
 *    insert_or_assign and is not reported.  Whatever the order in which the keys of the call arrive:
 *    {resident before} U {keys} = {resident after} + {reported}, every reported key exactly once, and a reported key that
 *    was one of `keys` carries the row of `values`.
 *    flags: TFRA_EVICT_WHOLE_ROWS — evicted_values rows are the whole co-located row, (1 + aux_fields) * dim elements
 *    (embedding, then the slot vectors, as stored; a key that was not admitted has its slot vectors at aux_init); without
 *    it rows of dim elements.  Unknown bits: TFRA_ERR_INVALID.
 *    Counter and cap are tfra_table_export_batch_if's: *d_evicted_counter (device size_t, the caller zeroes it) is advanced
 *    by every reported entry whatever cap is; an entry whose position is >= cap is not written — key, row and score alike;
 *    cap = n always suffices.  evicted_keys == NULL: count only (evicted_values and evicted_scores must be NULL too, else
 *    TFRA_ERR_INVALID).  evicted_values and evicted_scores may each be NULL.  The output order is unspecified.
 *    A table that is not at max_capacity (still growing, or TFRA_EVICT_NONE) displaces nothing: the call IS that
 *    insert_or_assign, the counter and the output buffers are not touched (evicted_scores may be non-NULL).
 *    At max_capacity the call always takes the locked two-phase kernels (phase 2 captures); the single ownership pass that
 *    insert_or_assign prefers for small batches does not capture.  Same table either way.
 *    Refused before anything is enqueued, tfra_last_error() naming the function: a NULL table, keys, values or counter,
 *    n >= 2^31 (TFRA_ERR_INVALID).  n == 0: TFRA_OK, nothing touched.  Synchronises nothing; usable under
 *    TFRA_OPTION_CAPTURE_SAFE as tfra_table_insert_or_assign is.  (tests/test_gpu_insert_and_evict.py)                      */
#define TFRA_EVICT_WHOLE_ROWS 1u
int tfra_table_insert_and_evict(tfra_table_t* t, size_t n, const int64_t* keys, const void* values,
                                const uint64_t* scores, uint32_t flags, size_t* d_evicted_counter, size_t cap,
                                int64_t* evicted_keys, void* evicted_values, uint64_t* evicted_scores,
                                tfra_stream_t stream);

/* -- find_or_insert (HierarchicalKV's find_or_insert): the lookup of a training step.  A key that is resident is READ; a key
 *    that is not is admitted with the row the caller drew for it, and that row is returned.  After the call every key of the
 *    batch that could be placed is resident with the row the caller saw, so the step's write-back only ever hits.
 *    keys: unique within the call (HKV's contract, what TFRA_FLAG_UNIQUE_KEYS names).  d_n: NULL, or the key count as in
 *    tfra_table_find_n (a device int64, or pinned host memory the device can read): min(n, *d_n) keys are served, entries of
 *    values_out / found beyond the count are left as they are; a growing table sizes itself by n, the upper bound.
 *    init_values: [n, dim] when init_is_full, else one row [dim], in the table's value dtype (tfra_table_find's defaults /
 *    default_is_full).  scores: NULL or [n], as for tfra_table_insert_or_assign.  values_out ([n, dim]) may be NULL (admit
 *    only); found ([n]) may be NULL.
 *    A HIT: values_out[i] = the resident embedding row, found[i] = 1.  The row and the slot vectors are not written; the
 *    score is touched as insert_or_assign touches it on an assign (LRU: the clock, LFU: += score, CUSTOMIZED: the caller's).
 *    A MISS: the key is written exactly as tfra_table_insert_or_assign(.., TFRA_FLAG_UNIQUE_KEYS) would write (key, init row,
 *    score): below max_capacity or on a growing table into an empty slot with the slot vectors at aux_init; at max_capacity
 *    with the same victim and admission rule, the slot starting a new life.  values_out[i] = the init row and found[i] = 0,
 *    whether the key was placed, was not admitted, or could not be placed (that one counts in tfra_table_check_errors).
 *    The table ends as tfra_table_insert_or_assign(keys, found ? resident row : init row, scores, TFRA_FLAG_UNIQUE_KEYS) on
 *    the locked kernels would leave it: keys, rows, slot vectors, scores; the epoch steps once per call.  A key of the batch
 *    may be displaced by a later key of the same batch only where that call would displace it; the row returned for it is
 *    still the one it had.
 *    The call always takes the locked two-phase kernels (phase 1 finds or claims and copies, phase 2 — at max_capacity only —
 *    evicts for the keys that found no empty slot); the single ownership pass does not serve it.  Every value dtype, every dim.
 *    Refused before anything is enqueued, tfra_last_error() naming the function: a NULL table, keys or init_values,
 *    n >= 2^31 (TFRA_ERR_INVALID).  n == 0: TFRA_OK, nothing touched.  Synchronises nothing; under TFRA_OPTION_CAPTURE_SAFE it
 *    behaves as tfra_table_insert_or_assign does.  (tests/test_gpu_find_or_insert.py)                                        */
int tfra_table_find_or_insert(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys,
                              const void* init_values, int init_is_full, const uint64_t* scores,
                              void* values_out, uint8_t* found, tfra_stream_t stream);

/* -- The read side of a tier: a table that stands in front of something slower (insert_and_evict above is its write side).
 *    All three calls: d_n is NULL, or the key count as in tfra_table_find_n (a device int64, or pinned host memory the device
 *    can read): min(n, *d_n) keys are served, a negative count means 0, and entries of the outputs beyond the count are left
 *    as they are.  Refused before anything is enqueued, tfra_last_error() naming the function: a NULL table, NULL keys, NULL
 *    exists for contains, NULL values for assign, NULL defaults with non-NULL values, n >= 2^31 (TFRA_ERR_INVALID).  n == 0:
 *    TFRA_OK, nothing touched.  They synchronise nothing, never grow the table, and are usable under
 *    TFRA_OPTION_CAPTURE_SAFE as tfra_table_find is.  (tests/test_gpu_find_missed.py, test_gpu_assign.py, test_gpu_tier_loop.py)
 *
 *    find_missed (HierarchicalKV's find(n, keys, values, missed_keys, missed_indices, missed_size, scores)): tfra_table_find that
 *    also lists its misses.  values and exists are byte for byte what tfra_table_find writes for the same arguments (the
 *    embedding field, duplicate keys, one default row or [n, dim] defaults, every value dtype and dim); it never inserts and
 *    never writes the table, an LRU score is not touched.  values may be NULL: the call lists misses only, defaults is not
 *    read.  scores_out: NULL or [n]; a hit's entry is the uint64 tfra_table_export_batch would report for that key now (a table
 *    without scores: 0; a reserved key: ~0), a miss's is 0.
 *    Reported: every missed batch position i is appended at *d_missed_counter as the pair (keys[i], (int32_t)i); a missing key
 *    that repeats is reported at every one of its positions, unique keys give a unique list.  The two arrays are
 *    index-aligned; the order is unspecified.  Counter and cap are tfra_table_export_batch_if's: the counter (device size_t,
 *    the caller zeroes it, the call continues from its value) advances by every miss whatever cap is; a pair whose position is
 *    >= cap is not written, key and index alike; cap = n always suffices from a zeroed counter.  missed_keys and
 *    missed_indices may each be NULL (both: count only).  d_missed_counter == NULL requires both NULL (else TFRA_ERR_INVALID):
 *    the call is then find plus scores.
 *    *d_missed_counter is 8 bytes: it can be handed unchanged as d_n to tfra_table_find_n, tfra_table_insert_or_assign_n or
 *    tfra_table_find_or_insert on another table (the lower tier), with missed_keys as their keys — no host read in between.
 *    The counter takes ONE atomic add per block of the launch that has a miss, not one per miss.
 *
 *    assign (HierarchicalKV's assign): a write that only hits.  keys: unique within the call (what TFRA_FLAG_UNIQUE_KEYS names;
 *    with repeats the row a repeated key ends with is unspecified).  A resident key gets values[i] in its embedding field, its
 *    score is touched exactly as tfra_table_insert_or_assign touches it on an assign (scores ? scores[i] : 1), its slot vectors
 *    are not written, found[i] = 1.  A key that is not resident changes nothing — it is not claimed, not evicted for, not
 *    counted in tfra_table_check_errors — and found[i] = 0: the caller sends it to the tier that holds it.  The size and the
 *    slot census are unchanged; the epoch steps once per call, as for insert_or_assign.  Both reserved keys are served.
 *    found may be NULL.
 *
 *    contains (HierarchicalKV's contains): exists[i] is tfra_table_find's byte; one probe per key, no row is read, nothing is
 *    written.                                                                                                               */
int tfra_table_find_missed(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys,
                           void* values, uint8_t* exists, uint64_t* scores_out,
                           const void* defaults, int default_is_full,
                           size_t* d_missed_counter, size_t cap, int64_t* missed_keys, int32_t* missed_indices,
                           tfra_stream_t stream);
int tfra_table_assign(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys, const void* values,
                      const uint64_t* scores, uint8_t* found, tfra_stream_t stream);
int tfra_table_contains(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys, uint8_t* exists,
                        tfra_stream_t stream);

/* -- insert_and_evict_n: tfra_table_insert_and_evict with the key count on the device and, on request, whole rows in.
 *    The contract is tfra_table_insert_and_evict's over min(n, *d_n) keys.  d_n is as in tfra_table_find_n (NULL: n; a negative
 *    count: 0): nothing beyond the count is read as a key or written, scratch and growth are sized by n.  The call always takes
 *    the locked two-phase kernels; off max_capacity it displaces nothing and leaves the counter alone, like its parent.
 *    flags: TFRA_EVICT_WHOLE_ROWS as above, and TFRA_INSERT_WHOLE_ROWS — `values` rows are (1 + aux_fields) * dim elements, the
 *    embedding, then the slot vectors, as stored.  The slot vectors are then written from the caller's row in every case (a key
 *    that takes an empty slot, a key that replaces a victim, a key that was already resident) and aux_init is not applied; under
 *    TFRA_EVICT_WHOLE_ROWS a key that is not admitted is reported with the caller's whole row.  Without the flag the bytes
 *    written are exactly tfra_table_insert_and_evict's.  Unknown bits: TFRA_ERR_INVALID.
 *    Refused before anything is enqueued, tfra_last_error() naming the function: the parent's cases.
 *    (tests/test_gpu_insert_and_evict_n.py)                                                                                   */
#define TFRA_INSERT_WHOLE_ROWS 2u
int tfra_table_insert_and_evict_n(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys, const void* values,
                                  const uint64_t* scores, uint32_t flags, size_t* d_evicted_counter, size_t cap,
                                  int64_t* evicted_keys, void* evicted_values, uint64_t* evicted_scores, tfra_stream_t stream);

/* -- The tier driver: `upper`, a bounded LRU / EPOCHLRU table (a cache in HBM), in front of `lower`, a TFRA_EVICT_NONE table that
 *    holds everything.  Every call is ONE stream-ordered chain of launches on both tables with no host read, and moves WHOLE
 *    co-located rows between them: a key that is demoted and later promoted comes back with its slot vectors.
 *    The invariant, after every call, for every key ever written through the tier: if upper contains it, upper holds its newest
 *    whole row; otherwise lower holds it.  The tier is inclusive: a promoted key keeps a stale copy below, upper wins, a demotion
 *    overwrites the stale copy.  (Writes that go to either table directly are the caller's to keep consistent with this.)
 *    create refuses, naming itself: tables that differ in device, value dtype, dim or aux_fields, upper == lower, max_batch == 0
 *    or >= 2^31 (TFRA_ERR_INVALID); an upper strategy other than LRU / EPOCHLRU — every key must be admitted — and a lower
 *    strategy other than TFRA_EVICT_NONE — the bottom must not forget — (TFRA_ERR_UNSUPPORTED).  The driver owns staging for
 *    max_batch keys; it must be destroyed before its tables (destroy waits for the device).
 *    All calls: d_n as in tfra_table_find_n; n > max_batch, a NULL tier or a NULL required buffer: TFRA_ERR_INVALID naming the
 *    function, nothing enqueued; n == 0: TFRA_OK, nothing touched.  Both tables are locked as the grouped calls lock several
 *    tables (one global order), so a tier call and a plain call on either table from another thread do not deadlock.
 *
 *    tfra_tier_find: a read.  Duplicates are served at every position, nothing moves, nothing is written to either table, no score
 *    is touched.  values[i] = the row upper holds, else the row lower holds, else the default (defaults / default_is_full as in
 *    tfra_table_find); where[i] (may be NULL) = 1 (upper), 2 (lower) or 0 (neither).
 *
 *    tfra_tier_find_or_insert: the lookup of a training step.  keys are unique.  values_out (may be NULL) and where (may be NULL)
 *    as for tfra_tier_find, a never-seen key's row being its init row (init_values / init_is_full as in
 *    tfra_table_find_or_insert).  Afterwards every key of the batch is resident in upper with its whole row — a key from below
 *    with the slot vectors it had there, a never-seen key with slot vectors at upper's aux_init — and its score is the newest:
 *    the hits are touched before the misses are promoted, so the batch does not evict its own keys.  What the promotion
 *    displaces goes to lower as whole rows.
 *    The saturation limit: a batch that fills both home buckets of one of its own keys with its own keys (30 slots) cannot keep
 *    that key in upper; its row is then below and the invariant holds, but a fused write-back of the step would not find it
 *    resident and restart it from the default row — the same limit as a key "not resident at write-back time".  And that
 *    write-back inserts the key into upper directly: at max_capacity it evicts another resident key OUTSIDE the tier, whose
 *    newest whole row is not demoted and is lost (lower keeps at most a stale copy) — the invariant breaks for that victim.
 *    It takes a batch built for the purpose; a caller that cannot rule one out checks not_resident before writing back.  With
 *    TFRA_TIER_VERIFY the call counts the batch keys that are not resident at its end into the statistics (not_resident).
 *
 *    tfra_tier_insert: upsert of embedding rows (unique keys) into upper, as tfra_table_insert_and_evict writes them (a new key's
 *    slot vectors start at aux_init); what it displaces goes to lower as whole rows.
 *
 *    tfra_tier_stats: out8 = {calls, missed, lower_hits, demoted, not_resident, 0, 0, 0}, cumulative, the call still pending
 *    included.  The one call that reads on the host (it waits for the stream).
 *    (tests/test_gpu_tier_driver.py)                                                                                          */
typedef struct tfra_tier tfra_tier_t;
#define TFRA_TIER_VERIFY 1u
int tfra_tier_create(tfra_table_t* upper, tfra_table_t* lower, size_t max_batch, tfra_tier_t** out);
int tfra_tier_destroy(tfra_tier_t* tier);
int tfra_tier_find(tfra_tier_t* tier, size_t n, const int64_t* d_n, const int64_t* keys, void* values, uint8_t* where,
                   const void* defaults, int default_is_full, tfra_stream_t stream);
int tfra_tier_find_or_insert(tfra_tier_t* tier, size_t n, const int64_t* d_n, const int64_t* keys, const void* init_values,
                             int init_is_full, void* values_out, uint8_t* where, uint32_t flags, tfra_stream_t stream);
int tfra_tier_insert(tfra_tier_t* tier, size_t n, const int64_t* d_n, const int64_t* keys, const void* values, tfra_stream_t stream);
int tfra_tier_stats(tfra_tier_t* tier, uint64_t* out8, tfra_stream_t stream);

/* -- accum_or_assign = TableWrapper::accum (lookup_table_op_hkv.h:539-546):
 *    absent & !exists -> insert row; present & exists -> row += delta (element order 0..dim-1,
 *    one add each); otherwise no-op.  Oracle: accumrase_fn (lib/cuckoo/cuckoohash_map.hh:619). */
int tfra_table_accum_or_assign(tfra_table_t* t, size_t n, const int64_t* keys,
                               const void* values_or_deltas, const uint8_t* exists,
                               const uint64_t* scores, uint32_t flags, tfra_stream_t stream);

/* -- erase / clear / size / capacity (lookup_table_op_hkv.h:745-756) ---------------------- */
int tfra_table_erase(tfra_table_t* t, size_t n, const int64_t* keys, tfra_stream_t stream);
int tfra_table_clear(tfra_table_t* t, tfra_stream_t stream);
/* host result: synchronises `stream` (HkvHashTableOfTensorsGpu::size, :162-170) */
int tfra_table_size(tfra_table_t* t, size_t* out, tfra_stream_t stream);
/* device scalar result, no host sync (size_i64, :172-179) */
int tfra_table_size_to_device(tfra_table_t* t, int64_t* d_out, tfra_stream_t stream);
/* Keys the device could not place since the last check (table full at max_capacity with nothing evictable, rehash
 * failure, a write-back plan whose internal capacity overflowed): returns TFRA_ERR_FULL with the count in
 * tfra_last_error() and clears the counter; TFRA_OK when there were none.  Synchronises `stream`.  tfra_table_size
 * performs the same check; the stream-ordered entry points never read the counter themselves. */
int tfra_table_check_errors(tfra_table_t* t, tfra_stream_t stream);
/* number of slots export_batch scans (= value to loop `offset` up to) */
int tfra_table_capacity(tfra_table_t* t, size_t* out);
/* Growth so far (introspection): out4 = {growths, of which in place, storage is a mapped address range (0/1), bytes
 * mapped}.  Tables of TFRA_VMM_THRESHOLD_MB (env, default 4096) or more live in a reserved virtual address range and grow
 * by mapping more memory behind the table and splitting every bucket into its children where it is — peak memory = the
 * new size; smaller tables, and tables on a caller-supplied allocator, grow by copying (old + new coexist). */
int tfra_table_growth_stats(tfra_table_t* t, uint64_t* out4);
/* introspection (tests, tools): out5 = {empty key slots, slots locked by an eviction in progress (0 whenever no
 * call is running), live key slots, buckets with the OVF0 flag, buckets with the OVF1 flag}.  Host buffer;
 * synchronises `stream`. */
int tfra_table_slot_census(tfra_table_t* t, uint64_t* out5, tfra_stream_t stream);
/* grow (rehash) so that at least `min_slots` slots exist; no-op if already that large */
int tfra_table_reserve(tfra_table_t* t, size_t min_slots, tfra_stream_t stream);

/* -- export_batch(n, offset, d_counter, keys, values, scores) (lookup_table_op_hkv.h:548-594):
 *    scans slots [offset, offset+n) and appends live (key, row[, score]) triples at
 *    *d_counter (device size_t, caller zeroes it), order unspecified.  values/scores may be
 *    NULL.  Output buffers must hold every live entry of the range.                        */
int tfra_table_export_batch(tfra_table_t* t, size_t n, size_t offset, size_t* d_counter,
                            int64_t* keys, void* values, uint64_t* scores, tfra_stream_t stream);

/* -- score-filtered scans (HierarchicalKV's export_batch_if / size_if / erase_if) for tables with a score line, i.e. every
 *    eviction strategy but TFRA_EVICT_NONE.  pred(score, threshold): TFRA_SCORE_GE = score >= threshold, TFRA_SCORE_LT =
 *    score < threshold, on the uint64 score export_batch reports (LRU: device clock; EPOCHLRU / EPOCHLFU: epoch << 32 | low
 *    word; LFU: count; CUSTOMIZED: the caller's).  The two reserved keys (side rows) count as score ~0: they match every GE
 *    and no LT.  All three calls: a table without scores returns TFRA_ERR_UNSUPPORTED, an unknown pred TFRA_ERR_INVALID, both
 *    before anything is enqueued (no counter is touched, no file created); tfra_last_error() names the function.  Like
 *    export_batch they are ordered against writers of the table by the caller.                                          */
typedef enum { TFRA_SCORE_GE = 0, TFRA_SCORE_LT = 1 } tfra_score_pred;
/* export_batch over the matching entries: n, offset, the slot numbering (reserved keys at nb*15 and nb*15+1) and the
 * unspecified order are tfra_table_export_batch's.  *d_counter (caller zeroes it) is advanced by EVERY match of the range
 * whatever cap is; an entry whose output position is >= cap is not written — key, row and score alike — so buffers of cap
 * entries are never overrun.  keys == NULL: count only (values and scores must be NULL too, else TFRA_ERR_INVALID; cap is
 * ignored, no row is read).                                                                                            */
int tfra_table_export_batch_if(tfra_table_t* t, int pred, uint64_t threshold, size_t n, size_t offset,
                               size_t* d_counter, size_t cap, int64_t* keys, void* values, uint64_t* scores,
                               tfra_stream_t stream);
/* Erases every matching entry of the whole table (one scan of the key and score lines; rows are not touched) and adds
 * their number to *d_erased (device size_t, may be NULL).  Synchronises nothing; safe under TFRA_OPTION_CAPTURE_SAFE
 * as tfra_table_erase is.                                                                                              */
int tfra_table_erase_if(tfra_table_t* t, int pred, uint64_t threshold, size_t* d_erased /* may be NULL; += */,
                        tfra_stream_t stream);
/* tfra_table_save_field for the matching entries only: the same `<prefix>-keys` / `<prefix>-values` files, byte format,
 * `append` and TFRA_OPTION_KEY_BYTES_ON_DISK key width, written window by window (buffer_keys slots per window, so a
 * window never holds more than buffer_keys matches; the cap is a guard).  field == 0 is the embedding.  No `-scores` file
 * is written: the reference's loader reads none (lookup_table_op_hkv.h:596-600), so a loaded key starts from the score its
 * insert gives it.  The files merge over a base through tfra_table_load, which does not clear.  A delta does not record
 * erased keys.                                                                                                         */
int tfra_table_save_if(tfra_table_t* t, int field, int pred, uint64_t threshold, const char* prefix,
                       size_t buffer_keys, int append, tfra_stream_t stream, size_t* n_saved);

/* -- run-time options.  TFRA_OPTION_CAPTURE_SAFE = 1 makes every table entry point safe to call
 *    while `stream` is being captured into a hipGraph (no host synchronisation, no event
 *    record/query, no growth): the caller guarantees capacity (tfra_table_reserve beforehand) and
 *    keeps using ONE stream.  Scratch buffers must have been sized by an identical warm-up call.
 *    TFRA_OPTION_NO_OWNER_TAGS = 1 makes the planned write-backs take the general two-kernel path
 *    (the one used when the 4 B/bucket owner-tag array cannot be allocated); same results.      */
typedef enum {
  TFRA_OPTION_CAPTURE_SAFE = 1,
  TFRA_OPTION_NO_OWNER_TAGS = 2,
  TFRA_OPTION_KEY_BYTES_ON_DISK = 3,
  TFRA_OPTION_STOCHASTIC_ROUNDING = 4
} tfra_option;
/*    TFRA_OPTION_KEY_BYTES_ON_DISK = 4 | 8 (default 8): the width of a key in `<prefix>-keys` files.  4 = tables whose OP-LEVEL key type
 *    is int32 (the reference's (int32, float) GPU kernels, K/cuckoo_hashtable_op_gpu.cu.cc:1058: its files hold raw int32 keys): save
 *    narrows, load widens (sign-extending); a key outside the int32 range fails the save.
 *    TFRA_OPTION_STOCHASTIC_ROUNDING = 0 (default, off) | a 64-bit seed: every FUSED OPTIMIZER write-back of a float16 / bfloat16 table
 *    (tfra_table_apply_optimizer / _apply_sparse / _apply_planned / _apply_planned_combined, the prefetch steps, tfra_route_apply, and the
 *    table's member of tfra_multi_apply_planned_combined, which is served by the single call's launches) rounds what the rule produced
 *    — the parameter and every slot vector the rule owns — stochastically instead of to nearest even.  With lo = x rounded toward zero
 *    onto the storage grid (continued by one step past its largest finite value, stored as infinity), hi the next grid value away
 *    from zero and F = 65536 (|x| - |lo|) / (|hi| - |lo|), the result is hi iff 65536 - r <= F, r the element's 16 random bits; a
 *    representable value, an infinity, a NaN and |x| at or beyond the continued step are stored as with the option off.  The bits are
 *    a pure function of (seed, call, key, element): with mix64 the splitmix64 finalizer and GAMMA = 0x9E3779B97F4A7C15,
 *      a = mix64(seed + call * GAMMA), b = mix64(a ^ key), e = field * dim + column, w = mix64(b + ((e >> 2) + 1) * GAMMA),
 *      r = (w >> 16 (e & 3)) & 0xffff.
 *    `call` is the table's count of fused write-backs that passed their checks and had work to do (one logical write-back issued in
 *    parts is one call); setting the option, to any value, sets it to 0.  The constant aux_init fill of fields the rule does not own,
 *    tfra_table_insert_or_accum, the upserts and every copy of a row keep nearest-even / the bits they are given.  A non-zero value on a
 *    table of another value type, and a fused write-back on a table that also has TFRA_OPTION_CAPTURE_SAFE (a replayed graph would
 *    reuse one call index), fail with TFRA_ERR_UNSUPPORTED before anything is enqueued.  (tests/test_gpu_stochastic_rounding.py) */
int tfra_table_set_option(tfra_table_t* t, int option, int64_t value);

/* -- set_global_epoch (lookup_table_op_hkv.h:499,507,533) --------------------------------- */
int tfra_table_set_global_epoch(tfra_table_t* t, uint64_t epoch);

/* -- KV files: <prefix>-keys (raw int64[]) and <prefix>-values (raw V[n*dim]), native endian
 *    (cuckoo_hashtable_op.cc:310-505; lookup_table_op_hkv.h:602-717).  buffer_keys = keys per
 *    I/O chunk.  load does NOT clear (the GPU op clears first, the CPU op does not).       */
int tfra_table_save(tfra_table_t* t, const char* prefix, size_t buffer_keys, int append,
                    tfra_stream_t stream, size_t* n_saved);
int tfra_table_load(tfra_table_t* t, const char* prefix, size_t buffer_keys, tfra_stream_t stream,
                    size_t* n_loaded);

/* ============================ fused extras (beyond HKV's surface) ========================= */

/* Field access for tables created with aux_fields > 0: same as find / insert_or_assign but on
 * state vector `field` (0 = the embedding itself).  Lets `<param>/<opt>/<slot>` variables of
 * create_slots (PY/dynamic_embedding_optimizer.py:870-958) be views of one physical table.
 * tfra_table_insert_field with field != 0: a resident key gets field `field` replaced and nothing else touched.  A key that
 * is NOT resident is created: field `field` = the value, field 0 = zeros (the engine holds no default row to give it) and
 * the other aux fields = aux_init.  Repeated keys without TFRA_FLAG_UNIQUE_KEYS: the last occurrence wins.  A field insert
 * never evicts: on a bounded table at max_capacity an absent key is created where its home buckets have a free slot, and
 * is dropped and counted (tfra_table_check_errors reports exactly these keys) where they have none; no resident row
 * changes either way.  The flag is accepted there with or without unique keys.  (tests/test_gpu_aux_fields.py)          */
int tfra_table_find_field(tfra_table_t* t, int field, size_t n, const int64_t* keys, void* values,
                          uint8_t* exists, const void* defaults, int default_is_full,
                          tfra_stream_t stream);
int tfra_table_insert_field(tfra_table_t* t, int field, size_t n, const int64_t* keys,
                            const void* values, uint32_t flags, tfra_stream_t stream);
/* KV files of one state vector: the reference checkpoints every slot variable of create_slots as its own table
 * (`<param>/<opt>/<slot>` -> `<param>_<opt>_<slot>_mht_<i>of<N>-keys/-values`); here the slot is field `field` of the
 * parameter's rows.  Same format as tfra_table_save / _load (field 0 = the embedding itself).  Load the embedding
 * first: tfra_table_load_field of an aux field creates a key that is not resident yet like tfra_table_insert_field does,
 * with field 0 = zeros and the other aux fields = aux_init, not with the parameter's default row (the engine has none). */
int tfra_table_save_field(tfra_table_t* t, int field, const char* prefix, size_t buffer_keys, int append,
                          tfra_stream_t stream, size_t* n_saved);
int tfra_table_load_field(tfra_table_t* t, int field, const char* prefix, size_t buffer_keys, tfra_stream_t stream,
                          size_t* n_loaded);

/* Fused sparse optimizer write-back: replaces (1+S) finds + dense apply + (1+S) upserts
 * (PY/dynamic_embedding_optimizer.py:165-204) with one pass over rows laid out [p|slot..].
 * keys [n] UNIQUE (use tfra_segment_sum first), grads [n,dim] fp32.  Missing keys are inserted
 * with p = param_defaults (full [n,dim] or broadcast [dim], like find) and slots = aux_init.
 * Requires aux_fields >= the optimizer's slot count.  value_dtype F32, F16 or BF16, here and in the planned / sparse forms
 * below (gradients and defaults are float32 — half gradients: the *_typed calls — and the rule runs in fp32 on the up-cast row and slots and the
 * results are rounded to the storage type once, to nearest even — or stochastically, on a table with
 * TFRA_OPTION_STOCHASTIC_ROUNDING; a new row starts from the float32 default row and aux_init values, not from their
 * rounded images).                                                                            */
typedef enum {
  TFRA_OPT_SGD = 0, TFRA_OPT_ADAM = 1, TFRA_OPT_ADAGRAD = 2, TFRA_OPT_FTRL = 3,
  TFRA_OPT_MOMENTUM = 4, TFRA_OPT_NESTEROV = 5, TFRA_OPT_RMSPROP = 6
} tfra_opt_kind;
/* The three later kinds use the fields the struct already has (it has no size field, so it does not grow; ABI version 1):
 *   MOMENTUM / NESTEROV (ResourceApplyMomentum, use_nesterov = false / true): lr, beta1 = momentum.  One slot: field 1 = accum,
 *     aux_init[0] = 0.   accum = accum * beta1 + g;  p -= accum * lr   |   p -= g * lr + accum * (beta1 * lr)
 *   RMSPROP (ResourceApplyRMSProp, non-centered): lr, beta1 = momentum, eps, and beta2 = 1 - rho — ALREADY SUBTRACTED by the
 *     caller, in double, and rounded to float once: (float)(1.0 - rho).  That is the constant TF's kernel and the oracle multiply
 *     by; 1.f - (float)rho is another float for rho = 0.9.  Two slots: field 1 = ms (aux_init[0] = initial_rms), field 2 = mom
 *     (aux_init[1] = 0).   ms += (g * g - ms) * beta2;  mom = mom * beta1 + (g * lr) / sqrt(ms + eps);  p -= mom
 * d_lr overrides lr for these as for the others (Nesterov's beta1 * lr is formed in the kernel, from the lr in force).
 * Every call below that takes a tfra_opt_params accepts all seven kinds on all of its paths and refuses any other value. */
typedef struct {
  int32_t kind;     /* tfra_opt_kind */
  float lr;         /* Adam: pass lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the host (global step) */
  float beta1, beta2, eps;          /* Adam; Adagrad: eps<0 -> TF1 rule (no eps); Momentum / Nesterov / RMSProp: see above */
  float l1, l2, lr_power;           /* FTRL                                                  */
  const float* d_lr;                /* optional DEVICE scalar overriding `lr` (read by the kernel):
                                       lets a captured hipGraph follow a learning-rate schedule /
                                       Adam's per-step lr_t without re-capturing                */
} tfra_opt_params;
/* d_n: optional DEVICE int64 scalar; when non-NULL only the first min(n, *d_n) keys are applied,
 * so a caller can chain tfra_unique -> tfra_segment_sum -> apply without reading the unique count
 * on the host (n is then the buffer length).
 * Scores, here and in the sparse / planned / combined forms below: one write-back is one upsert with score 1 — LFU counts + 1,
 * a CUSTOMIZED score BECOMES 1, EPOCHLFU epoch << 32 | (count + 1).  On a bounded table at max_capacity the keys that hit or find
 * an empty slot are written first, then every other key replaces the minimum-score entry of its two home buckets as
 * tfra_table_insert_or_assign does, with compare score 1 (EPOCHLFU: epoch << 32 | 1), and starts from the default row and
 * aux_init; a key that is not admitted is dropped WITH its gradient, no error.  (tests/test_gpu_eviction.py) */
int tfra_table_apply_optimizer(tfra_table_t* t, const tfra_opt_params* p, size_t n,
                               const int64_t* keys, const float* grads, const void* param_defaults,
                               int default_is_full, const int64_t* d_n, tfra_stream_t stream);

/* The whole backward half of a training step: ids [n] MAY repeat (a raw Zipf batch); gradients of equal
 * ids are summed in a fixed order (deterministic; ids occurring <= 8 times in the batch: strictly in batch order),
 * then one fused update per unique key as above.  = _resource_apply_sparse_duplicate_indices + the write-back
 * sequence (PY/dynamic_embedding_optimizer.py:165-204).  param_default_row: [dim] fp32, used for unseen keys.
 * Requires float32, float16 or bfloat16 values, dim % 4 == 0, dim <= 256.  On a table that is not evicting, the bytes are those of
 * tfra_reduce_by_key + tfra_table_apply_optimizer (same summation tree, same rule, one rounding).  More than 2^18 (262 144) ids per call take a slower path (chunk-wise
 * sums, then every key once; host reads of the counts, scratch allocated per call) with the same result up to the
 * association of the sums. */
int tfra_table_apply_sparse(tfra_table_t* t, const tfra_opt_params* p, size_t n, const int64_t* ids,
                            const float* grads, const float* param_default_row, tfra_stream_t stream);

/* insert_or_assign of a batch whose keys MAY repeat — the LAST occurrence wins, like the reference's sequential
 * LaunchTensorsInsert (K/cuckoo_hashtable_op.cc:104-140) — de-duplicated on the device, also on a bounded (Hkv)
 * table running at max_capacity (eviction needs one writer per key).  values [n,dim] of the table's dtype;
 * scores [n] or NULL (the last occurrence's score; LFU without scores counts the occurrences).  More than 2^18 ids are
 * written chunk after chunk on the stream. */
int tfra_table_upsert_sparse(tfra_table_t* t, size_t n, const int64_t* ids, const void* values,
                             const uint64_t* scores, tfra_stream_t stream);

/* The two calls above split at the point where gradients / values are needed.  Which ids repeat, in which order
 * their gradients are summed and which unique keys the step writes depends on the ids alone, and the ids of a step
 * are known at lookup time (PY/embedding_weights.py keeps them in the TrainableWrapper) or earlier (input
 * pipeline).  tfra_sparse_plan_build does that id-only half on ANY stream — next to the lookup of the same ids, or
 * while the previous step still runs: the batch as CSR-by-key (unique keys, and per key its batch positions in
 * ascending order; keys with many occurrences pre-split into runs of <= 512) — and tfra_table_apply_planned /
 * tfra_table_upsert_planned do the rest when the gradients / values exist.  Results are bit-identical to the
 * one-call forms.  The caller orders build and use (event / same stream) and keeps `plan` untouched until the
 * work using it has finished; a plan can be rebuilt for the next batch afterwards (it owns its device buffers:
 * ~ (90 + dim/2) B per id + 12 MB).  dim: the table's dim, or 0 for a plan only used by upsert_planned: an
 * assign needs the LAST position and the count of every distinct id, not the list of its positions, and such a
 * plan is built by ONE kernel (LDS de-duplication per 1024 ids + a global hash set with atomic max; ~21 MB).
 * A plan object is not internally locked: one thread builds / consumes it at a time (different plans and
 * different tables are independent).                                                                  */
typedef struct tfra_sparse_plan tfra_sparse_plan_t;
int tfra_sparse_plan_create(int device, tfra_sparse_plan_t** out);
int tfra_sparse_plan_destroy(tfra_sparse_plan_t* plan);
int tfra_sparse_plan_build(tfra_sparse_plan_t* plan, size_t n, const int64_t* ids, int dim, tfra_stream_t stream);
int tfra_table_apply_planned(tfra_table_t* t, const tfra_opt_params* p, const tfra_sparse_plan_t* plan,
                             const float* grads, const float* param_default_row, tfra_stream_t stream);
int tfra_table_upsert_planned(tfra_table_t* t, const tfra_sparse_plan_t* plan, const void* values,
                              const uint64_t* scores, tfra_stream_t stream);
/* -- find_or_insert over a write-back plan: the lookup of a training step whose ids repeat, served from the plan the step's
 *    write-back uses anyway — one de-duplication per step.
 *    plan: a CSR plan (tfra_sparse_plan_build with the table's dim) over a batch of n ids that may repeat; n is the plan's id
 *    count.  The keys served are the plan's distinct keys; their count stays on the device, nothing is read on the host and
 *    nothing is synchronised.  L(k) = the last batch position of key k.
 *    The table effect is tfra_table_find_or_insert's over the distinct keys, with the init row of k = init_values[L(k)] when
 *    init_is_full ([n, dim], one row per batch POSITION), else the one row [dim]; score of k = scores[L(k)] (scores: NULL or
 *    [n], per position; NULL as there).  The table ends as that call leaves it: keys, rows, slot vectors at aux_init for
 *    admitted keys, scores touched once per KEY (not per occurrence), one epoch step, the same victim and admission rule at
 *    max_capacity.  The result does not depend on the plan's internal key order.
 *    rows_out [n, dim] (the table's value dtype, required), found [n] (may be NULL): for EVERY batch position p of key k,
 *    rows_out[p] = the row tfra_table_find_or_insert returns for k and found[p] its flag — the resident row on a hit, the
 *    init row on a miss, whether the key was placed, not admitted or unplaceable.  All positions of a key get identical bits.
 *    Limits, as the planned write-back's: float32 / float16 / bfloat16 rows, dim % 4 == 0, dim <= 256, rows_out and
 *    init_values 16-byte aligned.
 *    Refused before anything is enqueued, tfra_last_error() naming the function: a NULL table, plan, init_values or rows_out,
 *    a plan never built, a plan whose dim is not the table's (TFRA_ERR_INVALID); an assign-only plan (dim 0), a dtype, dim
 *    or alignment outside the limits (TFRA_ERR_UNSUPPORTED).
 *    A plan whose build latched errors adds them to the table's error counter (tfra_table_check_errors), as the planned
 *    write-backs do; the positions of the keys the plan lost are left as they are.
 *    The plan stays the write-back's plan: a later tfra_table_apply_planned, _apply_planned_combined or _upsert_planned of it
 *    does what it would have done.  (The call uses plan scratch those calls overwrite anyway; records, bins, count words and
 *    ownership counters are not written.)  Usable under TFRA_OPTION_CAPTURE_SAFE as tfra_table_find_or_insert is.
 *    (tests/test_gpu_find_or_insert_planned.py)                                                                          */
int tfra_table_find_or_insert_planned(tfra_table_t* t, const tfra_sparse_plan_t* plan,
                                      const void* init_values, int init_is_full, const uint64_t* scores,
                                      void* rows_out, uint8_t* found, tfra_stream_t stream);
/* The same over a TIER (tfra_tier_create) -- tfra_tier_find_or_insert over a write-back plan: the lookup of a training step whose ids repeat, de-duplicated ONCE.  The keys
 *    served are the DISTINCT keys of `plan`, a built CSR plan (tfra_sparse_plan_build with the tables' dim) of at most max_batch
 *    ids; the call relates to tfra_tier_find_or_insert as tfra_table_find_or_insert_planned relates to tfra_table_find_or_insert:
 *    a key's init row is init_values[L(k)], L(k) its LAST batch position (init_is_full == 0: row 0), and the key's row and its
 *    `where` byte (1 = was in upper, 2 = came from lower, 0 = never seen) are written to EVERY batch position of the key.
 *    rows_out ([plan n, dim]) and where ([plan n]) may each be NULL; both NULL is the admit-only form (nothing is handed back, the
 *    two launches that spread rows to positions are not enqueued).  The tier carries no caller scores, so there is no `scores`.
 *    Afterwards every distinct key of the plan is resident in upper with its whole row (a never-seen key: [init row | aux_init
 *    slots]), what the promotion displaced is below as whole rows; the hits are touched before the promotion; the statistics move
 *    as for tfra_tier_find_or_insert, counted per distinct key; TFRA_TIER_VERIFY counts the distinct keys not resident at the end.
 *    The plan is left untouched and serves tfra_table_apply_planned / _apply_planned_combined / _upsert_planned on the upper table
 *    afterwards.  Nothing is read on the host; a plan overflow word goes to the upper table's error counter.
 *    Refused before anything is enqueued, tfra_last_error() naming the function: a NULL tier, plan or init_values, unknown flag
 *    bits, a plan that was never built, more ids in the plan than max_batch, a plan of another dim or device (TFRA_ERR_INVALID);
 *    an assign-only (SET) plan, a value dtype other than float32 / float16 / bfloat16, dim % 4 != 0, dim > 256, init_values or
 *    rows_out not 16-byte aligned (TFRA_ERR_UNSUPPORTED).  The saturation limit of tfra_tier_find_or_insert holds unchanged.
 *    (tests/test_gpu_tier_planned.py)                                                                                          */
int tfra_tier_find_or_insert_planned(tfra_tier_t* tier, const tfra_sparse_plan_t* plan, const void* init_values,
                                     int init_is_full, void* rows_out, uint8_t* where, uint32_t flags, tfra_stream_t stream);
/* The write-back of an embedding_lookup_sparse (gradient with respect to its combined output): the contract of
 * tfra_table_apply_planned, with `plan` built over the ENTRY ids (the sparse input's values, repeats included) and the
 * gradient of plan position e = the combiner's backward of entry e, formed from grad_out[n_rows, dim] in registers
 * (never written out): g_e = (grad_out[seg[e]] / den) * w_e, den = 1 (sum) | sum of the row's weights (mean) |
 * sqrt(sum of their squares) (sqrtn), 0 when that sum is 0 (see tfra_sparse_segment_combine_backprop).  seg[nnz]
 * ascending, weights[nnz] or NULL (=> 1), combiner 0 sum, 1 mean, 2 sqrtn.  Bit-identical to
 * tfra_table_apply_sparse(ids, tfra_sparse_segment_combine_backprop(grad_out, ...)).  float32 / float16 / bfloat16 tables, dim % 4 == 0,
 * dim <= 256, grad_out / default row 16-B aligned. */
int tfra_table_apply_planned_combined(tfra_table_t* t, const tfra_opt_params* p, const tfra_sparse_plan_t* plan,
                                      const float* grad_out, const int64_t* seg, const float* weights, int combiner,
                                      size_t n_rows, const float* param_default_row, tfra_stream_t stream);
/* Introspection (tests, tools): counts[6] = {keys with > 8 occurrences, other keys, partial sums, 512-entry bins,
 * entries of the other keys, build errors}; when keys != NULL also the CSR itself, keys with > 8 occurrences first:
 * keys[i], cnt[i], and positions[] = the batch positions of key 0, of key 1, ... each ascending (cap = length of
 * keys/cnt, positions holds n).  A plan built with dim 0 keeps no positions list: counts = {0, distinct keys, 0, 0, 0, 0},
 * keys / cnt in no particular order, positions must be NULL.  Host buffers; synchronises `stream`. */
int tfra_sparse_plan_read(const tfra_sparse_plan_t* plan, uint32_t* counts, int64_t* keys, uint32_t* cnt,
                          uint32_t* positions, size_t cap, tfra_stream_t stream);

/* One whole training step of a single table on two streams, driven from C (what a TF executor does
 * between the ops of one session.run, without the host framework in the loop):
 *   main : rows_out = find(ids_cur) [n = plan_cur's id count; skipped when rows_out is NULL; rows_out and find_default
 *          have the table's value type, grads and param_default_row are float32]
 *          -> tfra_table_apply_planned(plan_cur, grads)            (tfra_table_step_prefetch)
 *          or tfra_table_upsert_planned(plan_cur, values, scores)  (tfra_table_step_prefetch_assign)
 *   side : tfra_sparse_plan_build(plan_next, ids_next), free-running; plan_next may be NULL (last step).
 * plan_cur must have been built from ids_cur (by an earlier call as its plan_next, or by
 * tfra_sparse_plan_build on main_stream).  ids_next must be complete in memory when the call is made (the side
 * stream does not wait for the main stream).  The streams are ordered inside, normally without any
 * cross-queue event: rotate >= 3 plans (4 recommended) so that plan_next's buffers — last read by the
 * step that used it as plan_cur — are idle when it is rebuilt; with fewer the call waits on the host.  */
int tfra_table_step_prefetch(tfra_table_t* t, const tfra_opt_params* p, tfra_sparse_plan_t* plan_cur,
                             const int64_t* ids_cur, void* rows_out, const void* find_default,
                             const float* grads, const float* param_default_row,
                             tfra_sparse_plan_t* plan_next, const int64_t* ids_next, size_t n_next,
                             tfra_stream_t main_stream, tfra_stream_t side_stream);
int tfra_table_step_prefetch_assign(tfra_table_t* t, tfra_sparse_plan_t* plan_cur, const int64_t* ids_cur,
                                    void* rows_out, const void* find_default, const void* values,
                                    const uint64_t* scores, tfra_sparse_plan_t* plan_next,
                                    const int64_t* ids_next, size_t n_next, tfra_stream_t main_stream,
                                    tfra_stream_t side_stream);

/* Many tables on one GPU (BASELINE configs[4]: 26 embedding tables): the step of every table — the arguments of
 * tfra_table_step_prefetch (opt != NULL: grads_or_values = float gradients) or tfra_table_step_prefetch_assign (opt ==
 * NULL: grads_or_values = rows of the table's dtype) — issued from a pool of `n_workers` host threads (0 = 4), tables
 * dealt out dynamically.  Give the tables of one call disjoint stream pairs (or a few pairs round-robin) so that their
 * launches and kernels overlap; the call returns when every step has been ENQUEUED (like the single-table form it does
 * not wait for the GPU).  The first error of any table is returned.  In TensorFlow this is the inter-op thread pool
 * running the per-table op sequences of one session.run. */
typedef struct {
  uint32_t struct_size;              /* = sizeof(tfra_step_desc) */
  uint32_t reserved;
  tfra_table_t* table;
  const tfra_opt_params* opt;
  tfra_sparse_plan_t* plan_cur;
  const int64_t* ids_cur;
  void* rows_out;
  const void* find_default;
  const void* grads_or_values;
  const float* param_default_row;
  const uint64_t* scores;
  tfra_sparse_plan_t* plan_next;
  const int64_t* ids_next;
  size_t n_next;
  tfra_stream_t main_stream;
  tfra_stream_t side_stream;
} tfra_step_desc;
int tfra_multi_step_prefetch(size_t n_tables, const tfra_step_desc* descs, int n_workers);

/* -- the overlapped step: lookup of batch i+1 in ONE launch with the write-back of batch i ------------------------------
 * Replaces, for a training loop that alternates Find and Insert on one table, the pair of ops
 *   HkvHashTableOfTensorsGpu::Find   (K/hkv_hashtable_op_gpu.cu.cc:182-213  -> lookup_table_op_hkv.h:719-756 get)
 *   HkvHashTableOfTensorsGpu::Insert (K/hkv_hashtable_op_gpu.cu.cc:253-290  -> lookup_table_op_hkv.h:522-537 upsert)
 * with results IDENTICAL to running them one after the other (Insert exclusive, Find shared: lookup i+1 sees update i).
 * The driver defers the write-back of a batch to the NEXT call and runs it in the same kernel as that call's lookup; ids the
 * two batches share are served from `values_prev` (the rows being written), everything else from the table; an entry the
 * write-back would evict although this lookup looks for it is evicted after the lookup and the lookup's output corrected
 * (csrc/tfra_step_impl.h).  Ids may repeat (the last occurrence wins).  ONE launch per step on ONE stream, nothing
 * waits on the host: steps can be enqueued any number ahead (tfra_table_steps_overlap).  NOT for hipGraph capture: a launch
 * carries host-side rotating state (which of two counter sets the previous launch's tail zeroed, the plan rotation, the
 * ownership generation); a replayed launch would reuse counters nobody zeroed.  TFRA_OPTION_CAPTURE_SAFE tables take the
 * sequential path inside the same entry points.
 *
 *   tfra_table_step_overlap(d, n, ids, rows_out, exists_out, defaults, default_is_full, values_prev, scores_prev,
 *                           n_next, ids_next, n_next2, ids_next2, stream)
 *     rows_out[n, dim] / exists_out[n] (optional) = Find(ids) with the default fill of tfra_table_find;
 *     values_prev [n_prev, dim] = the rows to assign to the ids of the PREVIOUS call (NULL on the first call / after a
 *       flush); they must stay unchanged until this call's work has run;
 *     ids_next / n_next and ids_next2 / n_next2 (optional) = the ids of the next call and of the one after it, as an input
 *       pipeline knows them: the de-duplication plan of a batch is built over TWO launches without atomics (its distinct ids
 *       are scattered into per-window segments by the launch two calls ahead, its table is built by the launch one call ahead).
 *       With ids_next only, the plan of the next batch is built by a launch of its own in front of the step (round 3's plan
 *       kernel); with neither, by the next call in front of ITS step.  ids must stay valid until their batch has been written
 *       back (the call after the one that looked them up).  An announced batch is recognised by (address, length) when its
 *       own call comes: from announcement to write-back its buffer must stay UNMODIFIED (a ring of id buffers needs at least
 *       four entries when ids_next2 is used); a batch that was announced but is never stepped is forgotten by the next call.
 *   tfra_table_step_overlap_flush(d, values_prev, scores_prev, stream) writes the last batch back: call it before the table
 *     is used through any other entry point.
 * Tables or calls the overlap does not cover (LFU / EPOCHLFU / CUSTOMIZED scores — a key may be refused —, caller scores, optimizer slots, rows
 * that are not multiples of 16 bytes) run the same sequence one op after the other inside the same entry points. */
typedef struct tfra_step_driver tfra_step_driver_t;
int tfra_step_driver_create(tfra_table_t* t, tfra_step_driver_t** out);
int tfra_step_driver_destroy(tfra_step_driver_t* d);
int tfra_table_step_overlap(tfra_step_driver_t* d, size_t n, const int64_t* ids, void* rows_out, uint8_t* exists_out,
                            const void* defaults, int default_is_full, const void* values_prev, const uint64_t* scores_prev,
                            size_t n_next, const int64_t* ids_next, size_t n_next2, const int64_t* ids_next2, tfra_stream_t stream);
int tfra_table_step_overlap_flush(tfra_step_driver_t* d, const void* values_prev, const uint64_t* scores_prev, tfra_stream_t stream);
/* `count` consecutive steps from ONE host call (the arguments of tfra_table_step_overlap per step). */
typedef struct {
  uint32_t struct_size;              /* = sizeof(tfra_overlap_step) */
  int32_t default_is_full;
  size_t n;
  const int64_t* ids;
  void* rows_out;
  uint8_t* exists_out;
  const void* defaults;
  const void* values_prev;
  const uint64_t* scores_prev;
  size_t n_next;
  const int64_t* ids_next;
  size_t n_next2;
  const int64_t* ids_next2;
} tfra_overlap_step;
int tfra_table_steps_overlap(tfra_step_driver_t* d, size_t count, const tfra_overlap_step* steps, tfra_stream_t stream);
/* measurement: HIP events around the launch of each of the next `steps` overlapped steps; _kernel_times waits for them and
 * returns the average duration of the step launch in microseconds (rest_kernel_us: a second launch no longer exists, ~0) */
int tfra_step_driver_time_kernels(tfra_step_driver_t* d, size_t steps);
int tfra_step_driver_kernel_times(tfra_step_driver_t* d, double* step_kernel_us, double* rest_kernel_us, size_t* steps);
/* tuning builds (TFRA_STEP_VARIANT & 16): per-role time stamps of the last launches, out[64][6][4], see csrc/tfra_step_impl.h */
int tfra_step_driver_timing(tfra_step_driver_t* d, uint64_t* out);
/* steps taken overlapped / one op after the other so far; whether a write-back is pending; device_counts[3] (optional,
 * synchronises the device) = {evictions the pass deferred because the next lookup wanted the victim, victims the remainder
 * pass noted, output rows it rewrote with the default row} */
int tfra_step_driver_stats(const tfra_step_driver_t* d, uint64_t* overlapped, uint64_t* sequential, int* pending,
                           uint32_t* device_counts, uint32_t* why_sequential, uint64_t* plans_built);
/* lookups whose positions had been sorted one launch ahead (the MAP role of csrc/tfra_step_impl.h: the next batch's positions probed
 * in this batch's plan and packed by where their row comes from — needs ids_next): such a lookup reads no plan entry and, for the
 * positions served from the rows being written, no table line */
int tfra_step_driver_lookups_listed(const tfra_step_driver_t* d, uint64_t* out);
/* plans_built[2] (optional): plans of a next batch built inside the step launch (from pairs scattered one launch earlier: ids
 * known TWO batches ahead) / built by a launch of their own in front of the step (ids known one batch ahead only, or not at all) */
/* why_sequential (optional): why the last step that ran one op after the other did — 1 empty batch, 2 a buffer or the row
 * size is not a multiple of 16 bytes, 4 no owner tags, 8 optimizer slots / a strategy that may refuse a key / caller scores, 16 and 32
 * (round 5: the table can still grow / is not yet dense) are no longer reasons unless TFRA_STEP_GROWING=0, 64 the
 * previous batch was empty, 128 TFRA_OPTION_CAPTURE_SAFE */

/* -- front-end helpers (N1/N3 rows of SURVEY.md §8f) ------------------------------------- */

/* Scratch for unique/partition; grows on demand, reusable across calls on one stream.
 * A workspace serves ONE call at a time and ONE stream: it is not internally locked (unlike a table), growing it frees the
 * buffer the previous call's kernels were given (after a synchronise of the CURRENT call's stream only), and the persistent
 * sets of tfra_unique / tfra_multi_unique alternate by a parity that a call flips on the host.  Two host threads must therefore
 * never be inside the library with the same workspace — a caller with several threads keeps one workspace per thread and stream,
 * or a lock of its own around every call it hands the workspace to (the table calls that take one included: the table's lock
 * does not cover the workspace).  tfra_unique and tfra_multi_unique alone tolerate a change of stream between two calls (they
 * chain the new stream behind the previous one with an event); every other workspace call assumes the stream of the last one. */
typedef struct tfra_workspace tfra_workspace_t;
int tfra_workspace_create(int device, tfra_workspace_t** out);
int tfra_workspace_destroy(tfra_workspace_t* ws);

/* tf.unique: unique_out[0..*d_num_unique) in order of first occurrence, idx_out[i] = position of
 * ids[i] in unique_out (PY/dynamic_embedding_ops.py:99; PY/shadow_embedding_ops.py:316).
 * d_num_unique is a device int64 scalar (no host sync). */
int tfra_unique(tfra_workspace_t* ws, size_t n, const int64_t* ids, int64_t* unique_out,
                int32_t* idx_out, int64_t* d_num_unique, tfra_stream_t stream);
/* The same without tf.unique's first-occurrence ORDER (unique_out in no particular order, idx_out consistent with it): what
 * embedding_lookup needs of tf.unique (PY/dynamic_embedding_ops.py:99-117 — the distinct ids feed Find / Insert, the inverse
 * index the gather; the order is not observable there).  Two launches instead of three; n <= 2^18.  d_num_unique may be
 * device-visible pinned host memory: the count then reaches the host without a copy. */
int tfra_unique_unordered(tfra_workspace_t* ws, size_t n, const int64_t* ids, int64_t* unique_out,
                          int32_t* idx_out, int64_t* d_num_unique, tfra_stream_t stream);

/* tfra_unique of a LIST of id lists as ONE stream-ordered chain: for descriptor d, unique_out[0 .. *d_num_unique),
 * idx_out and *d_num_unique hold exactly what tfra_unique(ws, n, ids, unique_out, idx_out, d_num_unique, stream) writes — the
 * distinct ids in order of first occurrence, the position of every id among them, the count on the device.  The lists are
 * independent: an id that stands in two lists is distinct in each.  unique_out[*d_num_unique .. n) is unspecified.  Deterministic.
 * Enqueues: one upload of the records (the workspace's ring of pinned, event-guarded slots), then one insert launch over all lists'
 * ids, one scatter launch over all lists' tiles (it writes every list's count, 0 for a list with n == 0, whose other pointers may
 * be NULL) and one index launch, which is left out when no descriptor has an idx_out: 3 launches, or 2, whatever n_lists.
 * *launches_out (optional, host): the kernel launches enqueued; 0 when the call is refused or has nothing to do.
 * Every check runs before anything is enqueued: a refused call writes nothing.  TFRA_ERR_INVALID, naming the descriptor: a
 * struct_size other than sizeof, flags != 0, d_num_unique NULL, ids or unique_out NULL where n > 0, a list longer than 2^20 ids,
 * lists that total more than 2^22 ids, output ranges (unique_out, idx_out, d_num_unique) of different descriptors that overlap.
 * The same ids may stand in several descriptors.  The call keeps persistent sets of its own in the workspace, apart from
 * tfra_unique's: the two may be interleaved freely.  Synchronises nothing.  Not for stream capture.
 *                                                                                        (tests/test_gpu_unique_many.py) */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_unique_desc) */
  uint32_t flags;            /* 0 */
  size_t n;                  /* ids in this list; 0 is allowed */
  const int64_t* ids;        /* [n] */
  int64_t* unique_out;       /* [n] */
  int32_t* idx_out;          /* [n], or NULL: this list's inverse index is not wanted */
  int64_t* d_num_unique;     /* device int64 scalar */
} tfra_unique_desc;
int tfra_multi_unique(tfra_workspace_t* ws, size_t n_lists, const tfra_unique_desc* descs, uint32_t* launches_out /* optional, host */,
                      tfra_stream_t stream);

/* The entry lists of a LIST of safe sparse lookups, built on the device as ONE stream-ordered chain: what the
 * training form of safe_embedding_lookup_sparse hands its wrapper.  A descriptor is one lookup: nnz entries (ids[p], weights[p]) of
 * n_rows rows; the row of entry p is rows[p] (ascending), or with TFRA_SAFE_RAGGED the r with rows[r] <= p < rows[r + 1]
 * (rows = row_splits [n_rows + 1], non-decreasing).  Entry p is a MEMBER when its row lies in [0, n_rows) and — TFRA_SAFE_PRUNE
 * with weights given — weights[p] > 0 (a NaN is no member); an entry whose row lies outside is in neither list.
 *   kept list:  the members in input order, (ids[p], row, weights[p]); kept_weights is not written when weights == NULL.
 *   entry list: sorted by row; a row with members contributes them in input order with weight weights ? weights[p] : 1.0f, a row
 *               without members ONE entry (fill_id, r, 1.0f) with TFRA_SAFE_FILL, else (0, r, 0.0f).
 *   d_counts:   the kept count and the entry count, always written (n_rows == 0: both 0; nnz == 0: the entry list is the fillers).
 * Nothing at or beyond a count is specified, and nothing is ever written outside [0, nnz) of the kept buffers or
 * [0, nnz + n_rows) of the entry buffers — also where rows are not ascending or splits not non-decreasing, whose lists are then
 * unspecified.  The kept group is kept_ids and kept_rows, with kept_weights where weights are given: all or none.  The entry
 * group is entry_ids and entry_rows, entry_weights optional.  Neither group: the counts alone.  Deterministic.
 * Enqueues: one upload of the records (the workspace's ring of pinned, event-guarded slots), then per tile of 1024 the members'
 * counts and their scan for the lists that prune, the rows' bounds and member-less flags, their scan (it writes d_counts) and the
 * scatter: at most 5 launches, 3 when no list prunes, whatever n_lists; no block waits for another; scratch is the workspace's.
 * *launches_out (optional, host): the kernel launches enqueued; 0 when the call is refused or n_lists == 0 (TFRA_OK).
 * Every check runs before anything is enqueued: a refused call writes nothing.  TFRA_ERR_INVALID, naming the descriptor: a
 * struct_size other than sizeof, unknown flag bits, d_counts NULL, rows NULL where n_rows > 0 and (nnz > 0 or RAGGED), ids NULL
 * where n_rows > 0, nnz > 0 and a group is given, a half-given group, an int64 buffer that is not 8-byte or a float buffer that
 * is not 4-byte aligned, output ranges (the groups' buffers, d_counts) that overlap; descs NULL with n_lists > 0.
 * TFRA_ERR_UNSUPPORTED: nnz + n_rows >= 2^31 in one list, more than 2^24 entries plus rows in all lists.
 * Synchronises nothing.                                                                 (tests/test_gpu_safe_entries.py) */
#define TFRA_SAFE_PRUNE  1u  /* with weights: an entry is a member only if weights[p] > 0 (NaN: no member) */
#define TFRA_SAFE_FILL   2u  /* an empty row's entry is (fill_id, weight 1); without the flag (0, weight 0) */
#define TFRA_SAFE_RAGGED 4u  /* rows = row_splits [n_rows + 1] instead of ascending row ids [nnz] */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_safe_entries_desc) */
  uint32_t flags;            /* TFRA_SAFE_* */
  size_t n_rows;
  size_t nnz;
  const int64_t* rows;       /* [nnz] ascending row ids, or (RAGGED) row_splits [n_rows + 1] */
  const int64_t* ids;        /* [nnz] */
  const float* weights;      /* [nnz], or NULL */
  int64_t fill_id;
  int64_t* kept_ids;         /* [nnz] */
  int64_t* kept_rows;        /* [nnz] */
  float* kept_weights;       /* [nnz] */
  int64_t* entry_ids;        /* [nnz + n_rows] */
  int64_t* entry_rows;       /* [nnz + n_rows] */
  float* entry_weights;      /* [nnz + n_rows], or NULL */
  int64_t* d_counts;         /* device int64[2]: kept count, entry count */
} tfra_safe_entries_desc;
int tfra_multi_safe_entries(tfra_workspace_t* ws, size_t n_lists, const tfra_safe_entries_desc* descs,
                            uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The pooling lists of a field-wise embedding, built on the device in ONE launch: what FieldWiseEmbedding hands the
 * ragged pooled lookup.  ids and slots are dense row-major blocks [n_rows * per_row]: sample b owns the positions
 * [b * per_row, (b + 1) * per_row), and slots[p] in [0, nslots) is the field of ids[p].  With n = n_rows * per_row:
 *   entry_ids  [n]: the ids ordered by (sample, slot, input position) — STABLE: within one (sample, slot) the input order is kept.
 *   row_splits [n_rows * nslots + 1]: row_splits[b * nslots + f] = b * per_row + the number of sample b's entries with slot < f;
 *              the last element is n.  Segment b * nslots + f owns the entries [row_splits[s], row_splits[s + 1]).
 *   entry_pos  [n] int32, optional (NULL): the input position p of every entry.
 *   entry_seg  [n], optional (NULL): b * nslots + slot of every entry — the ascending `seg` of the combined write-back.
 *   d_bad      device int64, optional (NULL): += the number of slots outside [0, nslots).  Such a slot is a caller error: it is
 *              clamped into range (below 0 to 0, else to nslots - 1) and counted, never used as an index.
 * Nothing is ever written outside [0, n) of the entry buffers or outside row_splits' n_rows * nslots + 1 elements, whatever slots
 * holds.  Deterministic.  n_rows == 0: TFRA_OK, nothing is looked at or written.  per_row == 0: every split is 0 (ids, slots and
 * the entry buffers may be NULL).
 * Enqueues ONE kernel on `stream`, on the calling thread's current device: a sample is sorted by one, two or four waves of one block
 * (up to 64, up to 128, more entries) with the per-slot counts in LDS, the rank inside a chunk of 64 from wave64 ballots in
 * position order; no workspace, no memset, no host read, no block waits for another, plain vector stores (d_bad: one atomic add per
 * wave that saw a bad slot).
 * Every check runs before anything is enqueued: a refused call writes nothing.  TFRA_ERR_INVALID: nslots == 0, row_splits NULL,
 * ids, slots or entry_ids NULL where per_row > 0, an int64 buffer that is not 8-byte aligned or entry_pos not 4-byte aligned, an
 * output that overlaps another output or an input (ids and slots may be one buffer).  TFRA_ERR_UNSUPPORTED:
 * nslots > TFRA_FIELD_ENTRIES_MAX_SLOTS, n_rows * per_row >= 2^31 (or either factor).  The cap is the LDS budget: four waves' counts
 * of 4 bytes per slot, 32 KiB at the cap — half of what a block gets without opting in, and five blocks to a CU.
 * Synchronises nothing.                                                                 (tests/test_gpu_field_entries.py) */
#define TFRA_FIELD_ENTRIES_MAX_SLOTS 2048u
int tfra_field_entries(size_t n_rows, size_t per_row, size_t nslots, const int64_t* ids, const int64_t* slots, int64_t* entry_ids,
                       int64_t* row_splits, int32_t* entry_pos /* optional */, int64_t* entry_seg /* optional */,
                       int64_t* d_bad /* optional */, tfra_stream_t stream);

/* Find of all n ids AND tfra_unique_unordered of the same ids in ONE launch — the forward half of embedding_lookup as the fused TF op
 * TFRA>HkvHashTableEmbeddingLookup issues it (tf_ops/fused_ops_rocm.cc; PY/dynamic_embedding_ops.py:99-117 needs the rows of every id,
 * the distinct ids and the inverse index for the backward pass).  rows_out / exists / defaults / default_is_full as tfra_table_find,
 * unique_out / idx_out / d_num_unique as tfra_unique_unordered (n <= 2^18); the same results as the two calls one after the other (which
 * is what runs for rows that are not 16-byte granules). */
int tfra_table_find_unique(tfra_table_t* t, tfra_workspace_t* ws, size_t n, const int64_t* ids, void* rows_out, uint8_t* exists,
                           const void* defaults, int default_is_full, int64_t* unique_out, int32_t* idx_out,
                           int64_t* d_num_unique, tfra_stream_t stream);

/* out[idx[i],:] += in[i,:] in index order per segment is NOT guaranteed; sums are accumulated in
 * fp32 with a fixed tree per segment => deterministic. out is [num_segments, dim], zeroed here. */
int tfra_segment_sum(tfra_workspace_t* ws, size_t n, int dim, const float* in, const int32_t* idx,
                     const int64_t* d_num_segments, size_t max_segments, float* out,
                     tfra_stream_t stream);

/* tf.unique + unsorted_segment_sum in one call, parallel per key and order-fixed (the reduction half of
 * tfra_table_apply_sparse, same summation tree: PY/dynamic_embedding_optimizer.py:177-190): keys_out[0..*d_count) =
 * the distinct ids (unspecified order, may differ between calls), rows_out[i,:] = sum of the rows of `in` whose
 * id is keys_out[i] (bit-reproducible per key; ids occurring <= 8 times: strictly in input order).  keys_out [n],
 * rows_out [n,dim]; fp32, dim % 4 == 0, dim <= 256, n <= 2^18.  *d_count = -1 if an internal capacity overflowed
 * (pathological hash skew).  Unlike tfra_segment_sum the cost does not grow with the multiplicity of the hottest id. */
int tfra_reduce_by_key(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const float* in,
                       int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream);

/* -- Half-precision gradients: the three calls that read an [n, dim] gradient matrix, taking it as the dense part
 *    of a bfloat16 / float16 model hands it back, with the loss scale undone on the way.  Additive; ABI version 1.
 *    Contract: each call equals its untyped twin (tfra_table_apply_sparse, tfra_table_apply_planned, tfra_reduce_by_key) given
 *    the float32 matrix  G32[e] = f32(grads[e]) * s.
 *      f32() is the exact up-cast: subnormals are kept, a NaN stays a NaN.
 *      s = *d_scale, read by the kernels on the stream (a GradScaler's inverse scale; nothing is read on the host).  The product
 *      is ONE float32 multiplication, rounded on its own (the library is built with -ffp-contract=off).  d_scale == NULL: the
 *      result equals s = 1.
 *    Everything behind G32 is the twin's: the summation order of repeated ids, partial sums in float32, the rule and the rounding
 *    (stochastic included), scores, phase 2 on a full bounded table, the epoch step, the plan's error latch, capture-safety.
 *    tfra_table_apply_sparse_typed beyond 2^18 ids takes the twin's slower path; its first stage is the typed reduce, chunk by
 *    chunk, and the rest is unchanged, the sums being float32.
 *    dtype == TFRA_F32 with d_scale == NULL forwards to the untyped function: the same code, the same launches.
 *    Refused before anything is enqueued (tfra_last_error() names the function):
 *      TFRA_ERR_INVALID      a NULL g or g->grads; reserved != 0; a dtype other than the three
 *      TFRA_ERR_UNSUPPORTED  half gradients that are not 8-byte aligned; a float32 matrix with a scale (loss scaling belongs to
 *                            float16)
 *      and everything the twin checks, with the twin's codes.
 *    The combined write-backs are typed too: tfra_table_apply_planned_combined_typed below and
 *    tfra_multi_apply_planned_combined_typed (with the grouped calls).  Their contract is the same sentence over grad_out:
 *      A typed combined call equals its untyped twin given the float32 matrix  GO32[r] = f32(grad_out[r]) * s,  bit for bit.
 *    The product is formed BEFORE the combiner's backward: entry e's gradient is ((f32(g) * s) / den) * w, in that order, each
 *    step rounded on its own.  Everything behind GO32 is the twin's: the entry records, the denominators, the summation order of
 *    repeated ids, float32 partial sums, the rule and the rounding (stochastic included), scores, phase 2, the epoch step, the
 *    plan's error latch.  The refusals are those above, raised before anything is enqueued, and what the twin checks (half grad_out
 *    8-byte aligned instead of 16).  Addressing: the kernels address a half grad_out with 32-bit ELEMENT offsets, so a typed call
 *    on halves refuses n_rows * dim >= 2^32 with TFRA_ERR_UNSUPPORTED (the twin's n_rows < 2^30 holds besides); it does not widen
 *    the addresses.
 *    The weight-gradient calls are typed too: the seven *_backprop_weights_typed calls, declared behind their
 *    twins below.  Their contract is the same sentence over grad_out, with GO32[r, c] = f32(grad_out[r, c]) * s formed BEFORE the
 *    dot product d_p = sum_c GO32[r, c] * x_p[c]; dw_out stays float32.
 *    Not typed: tfra_table_apply_optimizer, the step drivers and tfra_sparse_segment_combine_backprop: they take float32. */
typedef struct {
  const void*  grads;    /* [n, dim] row-major in `dtype`; float32: 16-byte aligned, halves: 8-byte aligned */
  int32_t      dtype;    /* TFRA_F32 | TFRA_F16 | TFRA_BF16 */
  int32_t      reserved; /* must be 0 */
  const float* d_scale;  /* optional DEVICE float scalar, read by the kernels; NULL = no scaling */
} tfra_grads;            /* 24 bytes */
int tfra_table_apply_sparse_typed(tfra_table_t* t, const tfra_opt_params* p, size_t n, const int64_t* ids,
                                  const tfra_grads* g, const float* param_default_row, tfra_stream_t stream);
int tfra_table_apply_planned_typed(tfra_table_t* t, const tfra_opt_params* p, const tfra_sparse_plan_t* plan,
                                   const tfra_grads* g, const float* param_default_row, tfra_stream_t stream);
int tfra_reduce_by_key_typed(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const tfra_grads* g,
                             int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream);
/* tfra_table_apply_planned_combined with grad_out [n_rows, dim] as a tfra_grads.  TFRA_F32 with a NULL scale forwards to it. */
int tfra_table_apply_planned_combined_typed(tfra_table_t* t, const tfra_opt_params* p, const tfra_sparse_plan_t* plan,
                                            const tfra_grads* grad_out, const int64_t* seg, const float* weights /* may be NULL */,
                                            int combiner, size_t n_rows, const float* param_default_row, tfra_stream_t stream);

/* -- Whole rows out and back: the two table calls of a dense rule that has no fused write-back
 *    (optimizers.Generic with whole_rows=True).  The rows are co-located [p | slot 1 | ..]: a key's whole row is read with one
 *    probe and written with one probe.  Additive; ABI version 1. */
typedef struct {
  uint32_t struct_size;   /* = sizeof(tfra_row_fields) = 48 */
  int32_t  n_fields;      /* must equal 1 + the table's aux_fields (1..5) */
  float*   field[5];      /* field[f]: [n, dim] float32, row-major, 16-byte aligned, or NULL; entries >= n_fields must be NULL */
} tfra_row_fields;

/* tfra_table_fetch_planned: a READ over a built CSR plan of the table's dim (tfra_sparse_plan_build); U = its distinct keys.
 *      *d_count      = U, or -1 when the plan overflowed, exactly as tfra_reduce_by_key reports it
 *      keys_out[j]   j < U: the plan's distinct keys in the plan's key order — the order tfra_reduce_by_key over the same ids
 *                    writes; unspecified, but the same j indexes every output of this call
 *      gsum_out[j,:] bit for bit the row tfra_reduce_by_key_typed(ids, g) writes for that key (the same hot sums, the same
 *                    summation tree).  g: the record of the typed calls.  g == NULL requires gsum_out == NULL: the call then
 *                    fetches rows only and enqueues no sums launch
 *      rows_out->field[f][j,:] = the exact float32 up-cast of what tfra_table_find_field(t, f, key, defaults, 0) returns, where
 *                    defaults is `default_row` for f == 0 (ONE row in the table's value dtype, as tfra_table_find takes it) and
 *                    the table's stored image of aux_init[f - 1] for f >= 1: a resident key gives its stored fields, a key that
 *                    is not resident [default_row | aux_init ..].  A NULL field[f] is not read and not written
 *    Rows at or beyond U are left as they are.  The call never inserts, touches no score, changes no size and counts no error:
 *    find's probe (plain loads; both reserved key values are served), one probe per key, one read per wanted field.
 *    Launches: the hot-sums launch when g is given, then ONE fetch launch; nothing is read on the host.
 *    Limits: float32 / float16 / bfloat16 tables; dim % 4 == 0, dim <= 256; default_row, gsum_out and every field 16-byte aligned
 *    (a half default_row: 8-byte); a plan of at most 2^18 ids.
 *    Refused before anything is enqueued (tfra_last_error() names the function):
 *      TFRA_ERR_INVALID      a NULL t, plan, keys_out, rows_out, d_count or default_row; a wrong struct_size or n_fields, a
 *                            non-NULL entry beyond n_fields; a plan never built, or of another dim or device; gsum_out without g
 *                            or g without gsum_out; whatever the typed calls refuse for g, with their codes
 *      TFRA_ERR_UNSUPPORTED  an assign-only (SET) plan, another value dtype, the dim limits, a misaligned buffer
 *    A plan of 0 ids sets *d_count = 0 and does nothing else. */
int tfra_table_fetch_planned(tfra_table_t* t, const tfra_sparse_plan_t* plan, const tfra_grads* g,
                             const void* default_row, int64_t* keys_out, const tfra_row_fields* rows_out,
                             float* gsum_out, int64_t* d_count, tfra_stream_t stream);

/* tfra_table_store_rows: the write that goes with it — a unique-keys upsert of whole rows given as float32 fields.
 *    keys are UNIQUE within the call; d_n as in tfra_table_find_n (NULL: n; a negative count: 0).  field[0] must be non-NULL.
 *    Every element is rounded to the table's value dtype ONCE, to nearest even: a NaN stays a NaN, overflow goes to infinity.
 *    Nearest even also on a table with TFRA_OPTION_STOCHASTIC_ROUNDING (upserts keep nearest-even).
 *      a resident key: every field with a non-NULL pointer is replaced, a NULL field keeps its bytes
 *      a key that takes an empty slot or replaces a victim: non-NULL fields from the caller, NULL fields at aux_init
 *    The table ends with the keys and field bytes this sequence leaves, wherever that sequence places every key:
 *      tfra_table_insert_or_assign(keys, to_dtype(field[0]), NULL, TFRA_FLAG_UNIQUE_KEYS), then
 *      tfra_table_insert_field(f, keys, to_dtype(field[f]), TFRA_FLAG_UNIQUE_KEYS) for each non-NULL f >= 1
 *    with two differences:
 *      - scores and the epoch move as for ONE insert_or_assign with scores == NULL, not 1 + S times
 *      - on a bounded table at max_capacity the victim and admission rule is insert_or_assign's, applied once: a key that is
 *        not admitted is dropped with its whole row and no error, where the sequence's field inserts would count one
 *    One probe per key.  At most two launches: phase 1, and phase 2 only at max_capacity (the locked two-phase route of
 *    tfra_table_insert_and_evict_n, without capture).  Under TFRA_OPTION_CAPTURE_SAFE it behaves as insert_or_assign does.
 *    Limits and refusals as the fetch's: value dtypes, dim, alignment (TFRA_ERR_UNSUPPORTED); n < 2^31, a NULL t / keys / rows /
 *    field[0], the record's checks (TFRA_ERR_INVALID).  n == 0 returns TFRA_OK and touches nothing. */
int tfra_table_store_rows(tfra_table_t* t, size_t n, const int64_t* d_n, const int64_t* keys,
                          const tfra_row_fields* rows, tfra_stream_t stream);

/* The reduction half of tfra_reduce_by_key for a batch whose plan was built AHEAD (tfra_sparse_plan_build with dim = the
 * rows' dim, any stream): rows_out[dest[p], :] = sum of the rows of `grads` whose id equals ids[p] (same summation tree,
 * bit-reproducible).  dest [n] int32 maps batch positions to output rows and must be equal for all positions of one id —
 * e.g. position -> owner-major index of the multi-GPU gradient route, which depends on the ids alone and is computed
 * one batch ahead together with the plan (PY/shadow_embedding_ops.py:397-447 does unique + partition at lookup time). */
int tfra_plan_reduce_to(const tfra_sparse_plan_t* plan, const float* grads, const int32_t* dest, float* rows_out,
                        tfra_stream_t stream);

/* The distinct ids of a built plan in place of tfra_unique, for a caller that needs them grouped by owner (the multi-GPU
 * route; PY/shadow_embedding_ops.py:316,397-422 does unique then dynamic_partition):
 *   tfra_plan_partition   = tfra_partition over the plan's distinct keys (order unspecified): keys_out owner-major,
 *                           perm_out[j] = the plan's index of the key in owner-major row j, d_counts[num_shards];
 *   tfra_plan_positions_to: dest_out[p] = j for every batch position p whose id is the key of owner-major row j —
 *                           the position -> row map for tfra_gather_rows (lookup) and tfra_plan_reduce_to (gradients). */
int tfra_plan_partition(const tfra_sparse_plan_t* plan, tfra_workspace_t* ws, int num_shards, int mode,
                        int64_t* keys_out, int32_t* perm_out, int64_t* d_counts, tfra_stream_t stream);
int tfra_plan_positions_to(const tfra_sparse_plan_t* plan, const int32_t* perm, int32_t* dest_out, tfra_stream_t stream);

/* int32 <-> int64 keys on the device (sign-extending / truncating): the engine's keys are int64; a caller whose op-level key type is
 * int32 (K/cuckoo_hashtable_op_gpu.cu.cc:1058 REGISTER_KERNEL(int32, float)) widens in front of every table call and narrows the keys
 * an export returns.  tfra_keys_narrow_i32 counts the keys that do not fit into *d_overflow (device int64, may be NULL). */
int tfra_keys_widen_i32(size_t n, const int32_t* keys_in, int64_t* keys_out, tfra_stream_t stream);
int tfra_keys_narrow_i32(size_t n, const int64_t* keys_in, int32_t* keys_out, int64_t* d_overflow, tfra_stream_t stream);

/* out[i,:] = rows[idx[i],:] (tf.gather after unique). row_bytes = dim*sizeof(V). */
int tfra_gather_rows(size_t n, size_t row_bytes, const void* rows, const int32_t* idx, void* out,
                     tfra_stream_t stream);

/* embedding_lookup_sparse combiner (PY/dynamic_embedding_ops.py:224-291; SparseSegmentSum/Mean/SqrtN,
 * K/segment_reduction_ops_gpu.cu.cc:30-60): out[r,:] = combine_{i : seg[i]==r} w[i] * rows[idx[i],:]
 * with seg ASCENDING (SparseTensor row ids), weights NULL => 1.  combiner 0 sum, 1 mean (/ sum w),
 * 2 sqrtn (/ sqrt(sum w^2)); empty rows -> 0.  rows/out fp32; members are added in input order. */
int tfra_sparse_segment_combine(tfra_workspace_t* ws, size_t nnz, int dim, const float* rows,
                                const int32_t* idx, const int64_t* seg, const float* weights, int combiner,
                                size_t n_rows, float* out, tfra_stream_t stream);
/* Its backward (TF's SparseSegment{Sum,Mean,SqrtN}Grad together with the weights multiply, PY/dynamic_embedding_ops.py:
 * 218-291): entry_grads_out[e,:] = (grad_out[seg[e],:] / den) * w[e] in fp32, in that order, den = 1 (sum) |
 * sum_{seg==r} w (mean) | sqrt(sum_{seg==r} w^2) (sqrtn); a row whose weight sum is 0 gives 0 (as the forward), an
 * entry whose row lies outside [0, n_rows) gives 0.  seg ascending, weights NULL => 1, n_rows >= 1 when nnz > 0.
 * Chained with tfra_segment_sum(idx) it is the gradient of the lookup's unique rows. */
int tfra_sparse_segment_combine_backprop(tfra_workspace_t* ws, size_t nnz, int dim, const float* grad_out,
                                         const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                         float* entry_grads_out, tfra_stream_t stream);
/* The gradient of tfra_sparse_segment_combine with respect to its WEIGHTS: dw_out[p] = d loss / d weights[p], float32 [nnz],
 * from grad_out = d loss / d out [n_rows, dim] and x_p = rows[idx[p],:] — the formulas, conventions and evaluation order of
 * tfra_table_find_combine_backprop_weights below (same device functions, same column-to-lane mapping: where both apply, the
 * bits are equal).  Any dim > 0, as the forward.  seg ascending; weights NULL = all 1; an entry whose row lies outside
 * [0, n_rows) gets 0.  Enqueues the bounds step, one memset of dw_out and one launch.  nnz == 0: TFRA_OK. */
int tfra_sparse_segment_combine_backprop_weights(tfra_workspace_t* ws, size_t nnz, int dim, const float* rows,
                                                 const int32_t* idx, const float* grad_out, const int64_t* seg,
                                                 const float* weights, int combiner, size_t n_rows, float* dw_out,
                                                 tfra_stream_t stream);

/* pooled lookup = embedding_lookup_sparse's forward (PY/dynamic_embedding_ops.py:120-293) without its intermediates:
 * out[r,:] = combine over {p : seg[p] == r}, in input order, of w_p * (hit(ids[p]) ? row(ids[p]) : default_row), float32.
 * seg ascending.  Entries with seg outside [0, n_rows) are ignored.  A row without entries gives zeros.
 * mean / sqrtn: a row whose weight sum is 0 gives zeros.  weights NULL = all 1.  combiner 0 sum | 1 mean | 2 sqrtn.
 * default_row: one row in the table's value dtype.  Never inserts.  Duplicate and reserved ids are as in tfra_table_find.
 * Two launches (the rows' bounds, then one probe + row read per entry accumulated in registers); no unique pass, no [nnz, dim]
 * or [U, dim] tensor, nothing read on the host.  Bit-identical to tfra_table_find(ids -> rows, default_is_full = 0) followed by
 * tfra_sparse_segment_combine(float32(rows), idx = 0..nnz-1, seg, weights, combiner).
 * float32 / float16 / bfloat16 tables (half rows are up-cast exactly), dim % 4 == 0, dim <= 256, out and default_row 16-byte
 * aligned, nnz < 2^31, n_rows < 2^30: anything else returns TFRA_ERR_UNSUPPORTED and writes nothing.  nnz == 0 zero-fills out. */
int tfra_table_find_combine(tfra_table_t* t, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                            const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                            tfra_stream_t stream);

/* The pooled lookups of MANY tables in one call (a 26-table model's forward is 26 tfra_table_find_combine calls = 78 enqueues
 * otherwise): descs[i].out is bit-identical to tfra_table_find_combine(table, ws, nnz, ids, seg, weights, combiner, n_rows,
 * default_row, out, stream) — the same device code runs — and every rule of that call holds per descriptor (seg ascending,
 * entries outside [0, n_rows) ignored, empty rows zeros, reserved and duplicate ids, never inserts, the dtype / dim / alignment /
 * size limits).  n_rows == 0: the descriptor is skipped.  nnz == 0: its out is zero-filled.  n_tables == 0: TFRA_OK.
 * All descriptors are checked BEFORE anything is enqueued: if one fails, the call returns the code the single call returns for it
 * (TFRA_ERR_UNSUPPORTED / TFRA_ERR_INVALID; the message names the descriptor's index) and no out of any descriptor is written.
 * A wrong struct_size, a table on another device than ws, or descs == NULL with n_tables > 0: TFRA_ERR_INVALID.
 * The same table may appear in several descriptors (two features sharing one table); each distinct table is locked once, in
 * address order, and ordered behind its last stream once.  The tables' storage is looked at at call time: a table that grew
 * between two calls is read where it is now.
 * Enqueues, whatever n_tables: one upload of the descriptors' records (from a ring of pinned slots, each guarded by an event, so
 * that calls may follow each other with no host synchronisation; the stream is never waited for once ws has its size), one
 * memset of all rows' bounds, one bounds launch over all descriptors' entries and one combine launch per (value dtype, NCH)
 * class in the list — NCH = 1 for dim <= 64, 2 for dim <= 128, 4 otherwise: at most 9.  *launches_out (optional, host): the
 * kernel launches enqueued = the bounds launch (when any nnz > 0) + the combine launches.  Not for stream capture. */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;
  size_t nnz; const int64_t* ids; const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows; const void* default_row; float* out;                         /* out [n_rows, table dim] float32 */
} tfra_find_combine_desc;
int tfra_multi_find_combine(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_desc* descs,
                            uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The pooled lookup over a rank-2 RaggedTensor (PY/ragged_embedding_ops.py:129-260, embedding_lookup_sparse) with the semantics of
 * its safe form (PY/ragged_embedding_ops.py:263-442, safe_embedding_lookup_sparse) on request: row r combines the entries
 * [row_splits[r], row_splits[r + 1]) of ids / weights, in input order, as tfra_table_find_combine combines the entries with
 * seg == r — the same device code, so the result is bit-identical to that call on the row ids the splits stand for.
 * row_splits: int64 [n_rows + 1] on the device, 8-byte aligned.  Its CONTENT is not validated (that would need a host read):
 * the kernel uses b = clamp(row_splits[r], 0, nnz), e = clamp(row_splits[r + 1], b, nnz), so a negative, decreasing or too large
 * value gives an empty or shortened row and never a read outside ids / weights.
 * flags:
 *   TFRA_RAGGED_PRUNE  (:414-416; ignored when weights == NULL) an entry is a member of its row only if weights[p] > 0 — a NaN
 *                      weight is no member, as under math_ops.greater.  The weight sum and the accumulation run over the members
 *                      only, in entry order: the bits are those of the compacted list.  Ids are never pruned.
 *   TFRA_RAGGED_FILL   (:417-440) a row without members is the row stored under fill_id (any int64, the reserved key values
 *                      included), default_row on a miss, up-cast to float32 and written as it is (a -0.0 survives).
 *                      Without the flag such a row is zeros.
 * ONE kernel launch and nothing else (no workspace, no memset, no bounds launch); nnz == 0 without FILL is one memset of out,
 * with FILL the kernel runs and every row is the fill row.  The limits of tfra_table_find_combine hold (float32 / float16 /
 * bfloat16, dim % 4 == 0, dim <= 256, out and default_row 16-byte aligned, nnz < 2^31, n_rows < 2^30: TFRA_ERR_UNSUPPORTED);
 * unknown flag bits, a NULL row_splits with n_rows > 0: TFRA_ERR_INVALID.  n_rows == 0: TFRA_OK, nothing written.  Never inserts. */
#define TFRA_RAGGED_PRUNE 1u
#define TFRA_RAGGED_FILL  2u
int tfra_table_find_combine_ragged(tfra_table_t* t, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                   const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                   int64_t fill_id, const void* default_row, float* out, tfra_stream_t stream);

/* The two pooled lookups over a TIER (tfra_tier_create): tfra_table_find_combine and tfra_table_find_combine_ragged with the row of
 * an entry taken from both tables — the row upper holds, else the row lower holds, else default_row; upper wins, as in
 * tfra_tier_find.  The fill id of TFRA_RAGGED_FILL is looked up the same way, and the reserved key values are served in both tables.
 * Every rule of the one-table calls holds, with their codes and wording, checked on the upper table (both tables of a tier have its
 * value dtype, dim and device): the limits (float32 / float16 / bfloat16, dim % 4 == 0, dim <= 256, out and default_row 16-byte
 * aligned, nnz < 2^31, n_rows < 2^30), seg ascending, row_splits clamped and never validated, PRUNE / FILL, the zero rows, and the
 * launches — the tuple form is the bounds launch plus ONE combine launch, the ragged form ONE launch.
 * These calls are READS: nothing moves between the tables, nothing is written to either, no score is touched and the tier's
 * statistics do not change.  They use none of the tier's staging, so nnz is NOT limited by max_batch.  A key that is only below
 * costs its group one more key line; a batch of U = 4 entries that all hit upper reads nothing of lower.
 * Bit-identical to tfra_tier_find (default_is_full = 0) of ids followed by tfra_sparse_segment_combine over float32(rows) and
 * idx = 0..nnz-1, and to tfra_table_find_combine on one table that holds the same newest rows.
 * A NULL tier: TFRA_ERR_INVALID, nothing enqueued.  Never inserts, never promotes: a training step admits its ids first
 * (tfra_tier_find_or_insert with values_out == NULL).                                    (tests/test_gpu_tier_pooled.py) */
int tfra_tier_find_combine(tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                           const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                           tfra_stream_t stream);
int tfra_tier_find_combine_ragged(tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                  const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                  int64_t fill_id, const void* default_row, float* out, tfra_stream_t stream);

/* The gradient of the pooled lookup's WEIGHTS over a tier: tfra_table_find_combine_backprop_weights and
 * tfra_table_find_combine_ragged_backprop_weights (below), with the tier in the place of the table and the row of an entry taken
 * from both tables as in tfra_tier_find_combine.  dw_out[p] is what tfra_table_find_combine_backprop_weights gives on ONE table
 * that holds every key's newest row: upper wins, a stale copy below a promoted key is never read, a key in neither table is
 * default_row.  Bit-identical to that call, and to tfra_tier_find (default_is_full = 0) of ids followed by
 * tfra_sparse_segment_combine_backprop_weights over float32(rows) and idx = 0..nnz-1.  The ragged form's PRUNE and FILL are the
 * one-table ragged call's: a pruned entry and every entry of a row without members get exactly 0 (fill_id is not looked up, in
 * either table); row_splits is clamped and never validated; overlapping rows as described there.
 * Every rule of the one-table calls holds, with their codes and wording, checked on the upper table, grad_out in the place of out
 * (16-byte aligned), dw_out 4-byte aligned and non-NULL when nnz > 0.  nnz == 0 or n_rows == 0: TFRA_OK (with nnz > 0 and no rows,
 * dw_out is zeroed).  A NULL tier: TFRA_ERR_INVALID.  After any refusal nothing has been enqueued.
 * These calls are READS, as the tier's pooled lookups are: nothing moves between the tables, nothing is written to either, no
 * score is touched, tfra_tier_stats does not change, none of the tier's staging is used and nnz is NOT limited by max_batch.
 * Enqueues what the one-table calls enqueue: the tuple form the bounds step, one memset of dw_out and ONE launch; the ragged form
 * one memset and ONE launch.  A batch of U = 4 entries that all hit upper reads nothing of lower.
 *                                                                                   (tests/test_gpu_tier_weight_grad.py) */
int tfra_tier_find_combine_backprop_weights(tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                            const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                            const void* default_row, const float* grad_out, float* dw_out,
                                            tfra_stream_t stream);
int tfra_tier_find_combine_ragged_backprop_weights(tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                   const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                   int64_t fill_id, const void* default_row, const float* grad_out,
                                                   float* dw_out, tfra_stream_t stream);

/* The ragged pooled lookups of MANY tables in one call (the multi-hot features of a many-table model: the Keras layers call
 * PY/ragged_embedding_ops.py:263-442 once per feature): descs[i].out is bit-identical to tfra_table_find_combine_ragged of the
 * descriptor's fields — the same device code runs — and every rule of that call holds per descriptor.  n_rows == 0: the
 * descriptor is skipped.  n_tables == 0: TFRA_OK.  The same table may appear in several descriptors.
 * All descriptors are checked BEFORE anything is enqueued: if one fails, the call returns the code the single call returns for it
 * (the message names the descriptor's index) and no out of any descriptor is written.  A wrong struct_size, a non-zero
 * `reserved`, a table on another device than ws, or descs == NULL with n_tables > 0: TFRA_ERR_INVALID.
 * Locks, the tables' storage and the upload are those of tfra_multi_find_combine (shared ring of pinned slots in ws).
 * Enqueues, whatever n_tables: one upload of the descriptors' records and one launch per (value dtype, NCH, safe-or-not) class
 * in the list — safe: the descriptor's flags change something (FILL, or PRUNE with weights) — at most 18; no memset, no bounds
 * launch.  *launches_out (optional, host): the kernel launches enqueued.  Not for stream capture. */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_ragged_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;
  size_t n_rows; const int64_t* row_splits;                                   /* [n_rows + 1] */
  size_t nnz; const int64_t* ids; const float* weights;                       /* weights may be NULL */
  uint32_t flags; uint32_t reserved;                                          /* TFRA_RAGGED_*; reserved = 0 */
  int64_t fill_id; const void* default_row; float* out;                       /* out [n_rows, table dim] float32 */
} tfra_find_combine_ragged_desc;
int tfra_multi_find_combine_ragged(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_ragged_desc* descs,
                                   uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The two grouped pooled lookups over a list whose members are TIERS or plain tables (a many-table model keeps its big tables
 * tiered and its small ones plain, and one call reads all of them): tfra_multi_find_combine / tfra_multi_find_combine_ragged with
 * a descriptor that names exactly ONE of table / tier.  descs[i].out is bit-identical to the single call on that descriptor — the
 * same device function runs: a descriptor that names a tier matches tfra_tier_find_combine / tfra_tier_find_combine_ragged (upper
 * wins, else lower, else default_row; the fill id is looked up the same way), one that names a table matches
 * tfra_table_find_combine / tfra_table_find_combine_ragged.  Every rule of the single calls holds per descriptor, with their codes
 * and wording, checked on the table or on the tier's upper table.  n_rows == 0: the descriptor is skipped.  nnz == 0: its out is
 * zero-filled (ragged form with FILL: the kernel runs and every row is the fill row).  n_tables == 0: TFRA_OK.
 * All descriptors are checked BEFORE anything is enqueued: if one fails, the call returns the single call's code, the message is
 * "multi_tier_find_combine[_ragged]: descriptor <i>: ..." and no out of any descriptor is written.  Both of table / tier set,
 * neither of them set, a wrong struct_size, a non-zero `reserved`, a table on another device than ws, or descs == NULL with
 * n_tables > 0: TFRA_ERR_INVALID.
 * These calls are READS, as the single tier calls are: nothing moves between the tables, nothing is written to any of them, no
 * score is touched, tfra_tier_stats does not change, no tier's staging is used and nnz is not limited by max_batch.  So the same
 * tier and the same table may stand in several descriptors, and a table may be named directly in one descriptor while it is the
 * upper or lower table of a tier in another.
 * Locks: each distinct tier's own mutex once, in address order, before any table lock; then every distinct table of the call
 * (plain ones, uppers, lowers) once, in the global order of tfra_multi_find_combine — the hierarchy of the single tier calls.  The
 * tables' storage is looked at under the locks: a lower table that grew between two calls is read where it is now.
 * Enqueues, whatever n_tables: one upload of the records (the ring of pinned, event-guarded slots in ws that
 * tfra_multi_find_combine uses: calls may follow each other with no host wait); the tuple form then one memset of all rows'
 * bounds, ONE bounds launch over all descriptors, tiered or not, and one combine launch per (tiered or not, value dtype, NCH)
 * class in the list, at most 18; the ragged form one launch per (tiered or not, value dtype, NCH, safe or not) class, at most 36,
 * no memset and no bounds launch.  The plain classes run the kernels of tfra_multi_find_combine[_ragged].  *launches_out
 * (optional, host): the kernel launches enqueued.  Not for stream capture.  A training step admits its tiers' ids first, all
 * tiers in one chain with tfra_multi_tier_find_or_insert (below): what these calls collapse is the read.
 *                                                                                         (tests/test_gpu_tier_pooled_many.py) */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_tier_find_combine_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;       /* exactly ONE of table / tier is non-NULL */
  tfra_tier_t*  tier;
  size_t nnz; const int64_t* ids; const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows; const void* default_row; float* out;                         /* out [n_rows, dim] float32 */
} tfra_tier_find_combine_desc;
int tfra_multi_tier_find_combine(tfra_workspace_t* ws, size_t n_tables, const tfra_tier_find_combine_desc* descs,
                                 uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_tier_find_combine_ragged_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;       /* exactly ONE of table / tier is non-NULL */
  tfra_tier_t*  tier;
  size_t n_rows; const int64_t* row_splits;                                   /* [n_rows + 1] */
  size_t nnz; const int64_t* ids; const float* weights;                       /* weights may be NULL */
  uint32_t flags; uint32_t reserved;                                          /* TFRA_RAGGED_*; reserved = 0 */
  int64_t fill_id; const void* default_row; float* out;                       /* out [n_rows, dim] float32 */
} tfra_tier_find_combine_ragged_desc;
int tfra_multi_tier_find_combine_ragged(tfra_workspace_t* ws, size_t n_tables, const tfra_tier_find_combine_ragged_desc* descs,
                                        uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The grouped ADMISSION over tiers: tfra_tier_find_or_insert of a LIST of tiers as one stream-ordered chain (a model with 26 tiered
 * features otherwise enqueues 26 chains of 6 launches in front of a grouped read of 3).  Per descriptor the call IS
 * tfra_tier_find_or_insert on that descriptor: values_out and where, the invariant (afterwards every batch key is resident in the
 * upper table with its whole row, what the promotion displaced is in the lower table as whole rows), the touch of the hits before
 * the promotion, and the statistics (calls + 1, missed, lower_hits, demoted, not_resident under TFRA_TIER_VERIFY) are the same;
 * the same device code runs (stages 2 to 4 as twins of the single kernels).  n == 0: the descriptor is skipped and its tier counts
 * no call.  n_tiers == 0: TFRA_OK.
 * Refusals, ALL before anything is enqueued — a refused list leaves every table, every statistic and every output of every
 * descriptor untouched: the single call's rules with its codes and wording, prefixed "multi_tier_find_or_insert: descriptor <i>: "
 * (a NULL tier, NULL keys or init_values, n > max_batch, unknown flag bits); and, TFRA_ERR_INVALID: a wrong struct_size, a
 * non-zero `reserved`, descs == NULL with n_tiers > 0 (or a NULL ws), a tier on another device than ws, the same tier in two
 * descriptors, and any table standing twice in the call in ANY role (two tiers over one lower table; one tier's lower table
 * being another's upper table).  This call WRITES: the read calls' "may stand in several descriptors" does not carry over — a
 * block of a launch touches only its own descriptor's tables and staging.  (Descriptors with n == 0 are not looked at for this.)
 * Locks: each tier's own mutex once, in address order, then every upper and lower table once in the global order, as
 * tfra_multi_tier_find_combine.
 * Host work first: for ALL members, before the first grouped launch, both tables make room for the batch (a table may grow or
 * enqueue a size read, as in the single call) and an upper table at max_capacity sets up its phase-2 flags; the epoch is read
 * then and stepped per table after the enqueue.  If this fails part-way (a lower table's growth runs out of memory), earlier
 * tables may have grown, but no row and no statistic has changed.
 * Enqueues: one upload of the records (the workspace's ring of pinned, event-guarded slots), then each stage of the single chain
 * once per launch class — the template instance and host mode the single call would have picked: 1 launch for all tiers'
 * begin; find_missed_touch over the upper tables (copy granule 16 / 8 / 4 / 2 / 1 of row and buffers, 16 also with a dense
 * table's second home bucket in flight: at most 6); the fetch over the lower tables (at most 6); the whole-row upsert into the
 * upper tables (per granule, at most 5), for the members at max_capacity its capturing phase 2 (at most 5); the upsert of what
 * was displaced into the lower tables (at most 5); for TFRA_TIER_VERIFY members the count-only find_missed (at most 2).  At most
 * 30 launches whatever n_tiers; a list of 16-byte-aligned float32 tiers whose uppers are full is one class per stage: 6 launches,
 * 7 with TFRA_TIER_VERIFY.  *launches_out (optional, host): the kernel launches enqueued.  Not for stream capture.
 *                                                                                          (tests/test_gpu_tier_admit_many.py) */
typedef struct {
  uint32_t struct_size;            /* = sizeof(tfra_tier_find_or_insert_desc) */
  uint32_t flags;                  /* TFRA_TIER_VERIFY or 0 */
  tfra_tier_t* tier;
  size_t n; const int64_t* d_n;    /* d_n may be NULL; as tfra_tier_find_or_insert */
  const int64_t* keys;             /* unique */
  const void* init_values; int32_t init_is_full; uint32_t reserved;   /* reserved = 0 */
  void* values_out; uint8_t* where;                                   /* both may be NULL (admission only) */
} tfra_tier_find_or_insert_desc;
int tfra_multi_tier_find_or_insert(tfra_workspace_t* ws, size_t n_tiers, const tfra_tier_find_or_insert_desc* descs,
                                   uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The grouped admitting lookup of PLAIN tables: tfra_table_find_or_insert of a LIST of tables as one stream-ordered chain (a model
 * with 26 random-initializer features otherwise enqueues 26 admissions in front of a grouped read of 3).  Per descriptor the call
 * IS tfra_table_find_or_insert on that descriptor: values_out and found are the same and the table ends the same (keys, rows,
 * slot vectors at aux_init, scores; the epoch steps once per table), with the same victim and admission rule at max_capacity;
 * min(n, *d_n) keys are served and outputs beyond the count are left as they are; the same device code runs (both phases as twins
 * of the single call's kernels).  n == 0: the descriptor is skipped and its table's epoch does not step.  n_tables == 0: TFRA_OK.
 * Refusals, ALL before anything is enqueued — a refused list leaves every table and every output of every descriptor untouched:
 * the single call's rules with its codes and wording, prefixed "multi_find_or_insert: descriptor <i>: " (a NULL table, NULL keys
 * or init_values, n >= 2^31); and, TFRA_ERR_INVALID: a wrong struct_size, non-zero `flags` or `reserved`, descs == NULL with
 * n_tables > 0 or a NULL ws ("null argument": checked without a device, *launches_out = 0), a table on another device than ws,
 * and the same table in two descriptors.  This call WRITES: a block of a launch touches only its own descriptor's table, buffers
 * and scratch.  (Descriptors with n == 0 are not looked at for this.)
 * Locks: every table once, in the global order of the grouped calls.
 * Host work first: for ALL members, before the first grouped launch, the table makes room for the batch (it may grow or enqueue a
 * size read, as in the single call) and a table at max_capacity sets up its phase-2 flags (and, for one shared init row without
 * values_out, its spill rows); the epoch is read then and stepped per table after the enqueue.  If this fails part-way (a
 * growth runs out of memory), earlier tables may have grown, but no row has changed.
 * Enqueues: one upload of the records (the workspace's ring of pinned, event-guarded slots), then phase 1 once per copy-granule
 * class (16 / 8 / 4 / 2 / 1 of row, init rows and values_out) present in the list, and phase 2 once per granule class among the
 * members at max_capacity.  At most 10 launches whatever n_tables; a list of 16-byte-aligned float32 growing tables takes 1, with
 * full bounded members 2.  *launches_out (optional, host): the kernel launches enqueued.  Synchronises nothing.  Not for stream
 * capture.                                                                              (tests/test_gpu_find_or_insert_many.py) */
typedef struct {
  uint32_t struct_size;            /* = sizeof(tfra_find_or_insert_desc) */
  uint32_t flags;                  /* 0 */
  tfra_table_t* table;
  size_t n; const int64_t* d_n;    /* d_n may be NULL; as tfra_table_find_or_insert */
  const int64_t* keys;             /* unique */
  const void* init_values; int32_t init_is_full; uint32_t reserved;   /* reserved = 0 */
  const uint64_t* scores;          /* NULL or [n] */
  void* values_out; uint8_t* found;                                   /* both may be NULL (admission only) */
} tfra_find_or_insert_desc;
int tfra_multi_find_or_insert(tfra_workspace_t* ws, size_t n_tables, const tfra_find_or_insert_desc* descs,
                              uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The gradient of the pooled lookup with respect to its WEIGHTS (sp_weights of embedding_lookup_sparse; the reference gets it
 * from TensorFlow's autodiff of `embeddings *= weights`, segment_sum and the divide, PY/dynamic_embedding_ops.py:233-291):
 * dw_out[p] = d loss / d weights[p], float32 [nnz], for grad_out = d loss / d out, float32 [n_rows, dim].
 * For row r with members p (weights w_p, rows x_p read as float32: half rows up-cast exactly, default_row on a miss, as in the
 * forward), G = grad_out[r,:], d_p = sum_c G[c] x_p[c], s = sum_p w_p d_p and wsum = sum w (mean) | sum w^2 (sqrtn), the
 * forward's sum:
 *   sum    dw_p = d_p
 *   mean   dw_p = (d_p - s / wsum) / wsum
 *   sqrtn  dw_p = (d_p - (s / wsum) * w_p) / sqrtf(wsum)
 * mean / sqrtn with wsum == 0: every entry of the row gets 0.  An entry with seg outside [0, n_rows) gets 0.  weights NULL = all
 * 1; the gradient with respect to those implicit ones is still written.  seg ascending.
 * Order (csrc/tfra_combine_device.h): lane `sub` of the row's 16-lane group holds the columns 64 c + 4 sub .. + 3; it adds its
 * products over chunks ascending, components x, y, z, w; the group reduces by xor-shuffles with offsets 8, 4, 2, 1; columns at
 * or beyond dim add nothing; s adds w_p * d_p in entry order.  Bit-identical to tfra_table_find(ids -> rows) followed by
 * tfra_sparse_segment_combine_backprop_weights(float32(rows), idx = 0..nnz-1, ...).
 * Enqueues the forward's bounds step (a memset and a launch), one memset of dw_out and one launch (one probe and one row read
 * per entry; mean / sqrtn re-read the row's own [b, e) range of dw_out once — the table's rows are read once, the forward's out
 * is not an input).  Never inserts, touches no score; the table's storage is read where it is at call time, behind the table's
 * last stream.  Limits and refusals are tfra_table_find_combine's, with grad_out in the place of out: float32 / float16 /
 * bfloat16 tables, dim % 4 == 0, dim <= 256, grad_out and default_row 16-byte aligned, nnz < 2^31, n_rows < 2^30: anything else
 * returns TFRA_ERR_UNSUPPORTED and writes nothing; a bad combiner or a NULL buffer: TFRA_ERR_INVALID.  nnz == 0: TFRA_OK. */
int tfra_table_find_combine_backprop_weights(tfra_table_t* t, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                             const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                             const void* default_row, const float* grad_out, float* dw_out,
                                             tfra_stream_t stream);

/* The same gradient for the ragged call (tfra_table_find_combine_ragged): row r owns the entries [b, e) with
 * b = clamp(row_splits[r], 0, nnz), e = clamp(row_splits[r + 1], b, nnz); an entry outside that cover gets 0, and nothing
 * outside ids / weights / dw_out [0, nnz) is read or written whatever row_splits holds.  Bit-identical to
 * tfra_table_find_combine_backprop_weights on the row ids the splits stand for.
 * TFRA_RAGGED_PRUNE (ignored when weights == NULL): an entry whose weight is not > 0 (NaN included) is no member: it gets
 * exactly 0 and enters neither s nor wsum; the members' values are those of the compacted list, bit for bit.
 * TFRA_RAGGED_FILL: a row without members yields the fill row, which does not depend on the weights: its entries get 0 (they
 * are all pruned; fill_id is not looked up).
 * Overlapping rows: a row_splits that decreases can make two rows claim the same entries.  Both rows' groups then write those
 * entries of dw_out, in both passes and without ordering between them: such an entry ends as one row's value or a mix of the
 * two.  Entries that exactly one row claims are that row's, and nothing outside [0, nnz) is touched.
 * Enqueues one memset of dw_out and ONE launch; no workspace.  Limits and refusals are tfra_table_find_combine_ragged's, with
 * grad_out in the place of out; unknown flag bits: TFRA_ERR_INVALID.  nnz == 0: TFRA_OK. */
int tfra_table_find_combine_ragged_backprop_weights(tfra_table_t* t, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                    const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                    int64_t fill_id, const void* default_row, const float* grad_out,
                                                    float* dw_out, tfra_stream_t stream);

/* The weight gradients of MANY pooled lookups in one call (a model with 26 weighted sparse features asks for 26 of them per step:
 * ~100 enqueues for 26 small kernels otherwise).  A descriptor names exactly ONE of table / tier, as tfra_tier_find_combine_desc
 * does; descs[i].dw_out is bit-identical to the single call on that descriptor — the same device function runs:
 * tfra_table_find_combine[_ragged]_backprop_weights for a table, tfra_tier_find_combine[_ragged]_backprop_weights for a tier
 * (upper wins, else lower, else default_row).  Every rule of the single calls holds per descriptor, with their codes and wording,
 * checked on the table or on the tier's upper table: an entry in no row (tuple form) or outside the clamped cover of row_splits
 * (ragged form) gets 0; PRUNE applies only with weights, FILL changes nothing and fill_id is not looked at.
 * nnz == 0: nothing is written for the descriptor.  n_rows == 0 (nnz > 0): its dw_out is zero-filled.  n_tables == 0: TFRA_OK.
 * All descriptors are checked BEFORE anything is enqueued: if one fails, the call returns the single call's code, the message is
 * "multi_find_combine[_ragged]_backprop_weights: descriptor <i>: ..." and no dw_out of any descriptor is written.  Both of
 * table / tier set, neither of them set, a wrong struct_size, a non-zero `reserved`, a table on another device than ws, or
 * descs == NULL with n_tables > 0: TFRA_ERR_INVALID.
 * These calls are READS: no table is written, no score is touched, nothing moves between tiers, tfra_tier_stats does not change,
 * no tier's staging is used and nnz is not limited by max_batch.  So the same table or tier may stand in several descriptors, and
 * a table may be named directly in one descriptor while it is the upper or lower table of a tier in another.  The dw_out ranges
 * of different descriptors must NOT overlap (not checked: the descriptors' rows run side by side in one launch).
 * Locks and storage as in tfra_multi_tier_find_combine: each distinct tier's mutex once, in address order, then every distinct
 * table once in the global order; the views are taken under the locks.
 * Enqueues, whatever n_tables: one upload of the records (the workspace's ring of pinned slots); the tuple form one memset of all
 * rows' bounds; then ONE launch that zero-fills every dw_out (a descriptor owns ceil(nnz / 256) blocks of it) — in the tuple form
 * the same launch writes all rows' bounds —; then one gradient launch per (tiered or not, value dtype, NCH) class in the list, at
 * most 18; the ragged form per (tiered or not, value dtype, NCH, pruning or not) class, at most 36 — pruning: TFRA_RAGGED_PRUNE
 * with weights.
 * *launches_out (optional, host): the kernel launches enqueued =
 *     (1 if any descriptor has nnz > 0, else 0) + (the distinct classes among the descriptors with nnz > 0 and n_rows > 0).
 * Not for stream capture.                                                                  (tests/test_gpu_wgrad_many.py) */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_wgrad_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;       /* exactly ONE of table / tier is non-NULL */
  tfra_tier_t*  tier;
  size_t nnz; const int64_t* ids; const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows; const void* default_row;
  const float* grad_out;     /* [n_rows, dim] float32, 16-byte aligned */
  float* dw_out;             /* [nnz] float32 */
} tfra_find_combine_wgrad_desc;
int tfra_multi_find_combine_backprop_weights(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_wgrad_desc* descs,
                                             uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_ragged_wgrad_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;       /* exactly ONE of table / tier is non-NULL */
  tfra_tier_t*  tier;
  size_t n_rows; const int64_t* row_splits;                                   /* [n_rows + 1] */
  size_t nnz; const int64_t* ids; const float* weights;                       /* weights may be NULL */
  uint32_t flags; uint32_t reserved;                                          /* TFRA_RAGGED_*; reserved = 0 */
  int64_t fill_id; const void* default_row;                                   /* fill_id is ignored */
  const float* grad_out;     /* [n_rows, dim] float32, 16-byte aligned */
  float* dw_out;             /* [nnz] float32 */
} tfra_find_combine_ragged_wgrad_desc;
int tfra_multi_find_combine_ragged_backprop_weights(tfra_workspace_t* ws, size_t n_tables,
                                                    const tfra_find_combine_ragged_wgrad_desc* descs,
                                                    uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* -- Half-precision grad_out in the weight gradients: the seven calls above that read grad_out [n_rows, dim], taking
 *    it as a tfra_grads record (with the half-precision gradients, above) — the float16 / bfloat16 matrix a half model hands to
 *    tfra_table_apply_planned_combined_typed serves the weight gradient as it is, with no conversion pass.  Additive; ABI version 1.
 *    Contract: a typed weight-gradient call equals its untyped twin, bit for bit, given the float32 matrix
 *        GO32[r, c] = f32(grad_out[r, c]) * s
 *    with f32() and s as defined for tfra_grads: the up-cast is exact (subnormals kept, a NaN stays a NaN), s = *d_scale is read by
 *    the kernel on the stream, the product is ONE float32 multiplication rounded on its own, d_scale == NULL equals s = 1.  The
 *    product is formed BEFORE the dot product: d_p = sum_c GO32[r, c] * x_p[c], in the column order documented for the twin.
 *    Everything behind GO32 is the twin's: the probe, default_row on a miss, the tier's row source, PRUNE / FILL, the clamping of
 *    row_splits, the second pass of mean / sqrtn, the memsets and the bounds step, the locks, the launches' shapes and number.
 *    dw_out stays float32 [nnz].
 *    dtype == TFRA_F32 with d_scale == NULL forwards to the untyped function: the same code, the same launches.
 *    Refused before anything is enqueued and before the table or tier handle is looked at, dw_out untouched (tfra_last_error()
 *    begins as the twin's messages begin, with _typed appended to the name):
 *      TFRA_ERR_INVALID      a NULL grad_out or grad_out->grads; reserved != 0; a dtype other than the three
 *      TFRA_ERR_UNSUPPORTED  half gradients that are not 8-byte aligned; a float32 matrix with a scale
 *    then everything the twin checks, with the twin's codes and wording; a half grad_out needs 8-byte alignment where the float
 *    one needs 16 (with dim % 4 == 0 every row then is 8-byte aligned, odd rows at dim 4 included).
 *    Size limits: none beyond the twin's.  The row base grad_out + r * dim is formed in 64 bits, as the float one is: the
 *    n_rows * dim < 2^32 rule of the typed combined write-backs does NOT apply here.
 *    tfra_sparse_segment_combine_backprop_weights_typed keeps "any dim > 0": its vector arm runs when dim % 4 == 0 and rows is
 *    16-byte aligned (the half matrix is 8-byte aligned by the record's check), its element-wise arm otherwise (rows of the half
 *    matrix then start at 2-byte multiples); both give the twin's bits, and the bits of the pooled calls where both apply.
 *                                                         (tests/test_wgrad_half_abi.py, tests/test_gpu_wgrad_half.py) */
int tfra_table_find_combine_backprop_weights_typed(tfra_table_t* t, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                   const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                   const void* default_row, const tfra_grads* grad_out, float* dw_out,
                                                   tfra_stream_t stream);
int tfra_table_find_combine_ragged_backprop_weights_typed(tfra_table_t* t, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                          const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                          int64_t fill_id, const void* default_row, const tfra_grads* grad_out,
                                                          float* dw_out, tfra_stream_t stream);
int tfra_tier_find_combine_backprop_weights_typed(tfra_tier_t* tier, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                  const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                  const void* default_row, const tfra_grads* grad_out, float* dw_out,
                                                  tfra_stream_t stream);
int tfra_tier_find_combine_ragged_backprop_weights_typed(tfra_tier_t* tier, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                         const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                                         int64_t fill_id, const void* default_row, const tfra_grads* grad_out,
                                                         float* dw_out, tfra_stream_t stream);
int tfra_sparse_segment_combine_backprop_weights_typed(tfra_workspace_t* ws, size_t nnz, int dim, const float* rows,
                                                       const int32_t* idx, const tfra_grads* grad_out, const int64_t* seg,
                                                       const float* weights, int combiner, size_t n_rows, float* dw_out,
                                                       tfra_stream_t stream);
/* The grouped forms: tfra_multi_find_combine[_ragged]_backprop_weights with each descriptor's grad_out as a tfra_grads record.
 * descs[i].dw_out is bit-identical to the single typed call on the descriptor.  Descriptors of all three formats, with and without
 * a scale, may stand in one list; each record is checked as the single typed call checks it, before the descriptor's table or tier
 * is looked at, every descriptor before anything is enqueued; a refused list writes nothing and the message names the
 * descriptor's index ("multi_find_combine[_ragged]_backprop_weights_typed: descriptor <i>: ...").  A list whose descriptors are
 * all float32 without a scale runs the untyped call's code and launches — with ONE difference in what it accepts: a record's
 * `grads` must not be NULL, whatever n_rows is (the single typed calls' "null gradients"), where the untyped grouped call takes
 * a NULL grad_out for a descriptor without rows.  Everything else is the untyped grouped call's; the zero-fill / bounds launch
 * is unchanged.
 * Float-or-half is one more axis of the launch classes (float16 and bfloat16 share a launch: the format is a wave-uniform value
 * beside the descriptor's record).  *launches_out (optional, host): the kernel launches enqueued =
 *     (1 if any descriptor has nnz > 0, else 0)
 *     + (the distinct (tiered or not, value dtype, NCH[, pruning or not], float-or-half) classes among the descriptors with
 *        nnz > 0 and n_rows > 0):  at most 36 in the tuple form, 72 in the ragged form.
 * A list that is all half or all float has the untyped call's count.                      (tests/test_gpu_wgrad_half_many.py) */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_wgrad_typed_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;       /* exactly ONE of table / tier is non-NULL */
  tfra_tier_t*  tier;
  size_t nnz; const int64_t* ids; const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows; const void* default_row;
  tfra_grads grad_out;       /* [n_rows, dim] in grad_out.dtype, with its optional device scale */
  float* dw_out;             /* [nnz] float32 */
} tfra_find_combine_wgrad_typed_desc;
int tfra_multi_find_combine_backprop_weights_typed(tfra_workspace_t* ws, size_t n_tables,
                                                   const tfra_find_combine_wgrad_typed_desc* descs,
                                                   uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_ragged_wgrad_typed_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;       /* exactly ONE of table / tier is non-NULL */
  tfra_tier_t*  tier;
  size_t n_rows; const int64_t* row_splits;                                   /* [n_rows + 1] */
  size_t nnz; const int64_t* ids; const float* weights;                       /* weights may be NULL */
  uint32_t flags; uint32_t reserved;                                          /* TFRA_RAGGED_*; reserved = 0 */
  int64_t fill_id; const void* default_row;                                   /* fill_id is ignored */
  tfra_grads grad_out;       /* [n_rows, dim] in grad_out.dtype, with its optional device scale */
  float* dw_out;             /* [nnz] float32 */
} tfra_find_combine_ragged_wgrad_typed_desc;
int tfra_multi_find_combine_ragged_backprop_weights_typed(tfra_workspace_t* ws, size_t n_tables,
                                                          const tfra_find_combine_ragged_wgrad_typed_desc* descs,
                                                          uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The combined write-backs of MANY tables in one call (a 26-table model's backward is 26 tfra_table_apply_planned_combined calls =
 * ~160 enqueues otherwise): table i ends bit-identical to tfra_table_apply_planned_combined(table, opt, plan, grad_out, seg,
 * weights, combiner, n_rows, param_default_row, stream) — the same device code runs — and every rule of that call holds per
 * descriptor (float32 / float16 / bfloat16 rows, dim % 4 == 0, dim <= 256, grad_out / default row 16-B aligned, the rule's slot
 * fields, plan built over the table's ENTRY ids with the table's dim on the table's device, 1 <= n_rows < 2^30; opt->d_lr is
 * honoured per descriptor).  A descriptor whose plan holds 0 ids is skipped.  n_tables == 0: TFRA_OK.
 * All descriptors are checked BEFORE anything is enqueued and before any table is touched: if one fails, the call returns the code
 * the single call returns for it (the message names the descriptor's index) and no table or slot is changed.  A wrong
 * struct_size, descs == NULL with n_tables > 0, or a table on another device than ws: TFRA_ERR_INVALID.
 * A table or a plan may appear in at most ONE descriptor (two descriptors on one table would be two writers of one key inside one
 * launch): TFRA_ERR_INVALID otherwise, the message names both indices.  (tfra_multi_find_combine allows repeats: it only reads.)
 * The tables are locked once each, in address order, and ordered behind their last stream once each; then each table's capacity
 * is prepared as the single call prepares it (a table may grow here; this part stays per table and may enqueue its own small
 * size reads); the tables' storage is looked at after that, and the epoch strategies count one write-back per table.
 * Enqueues after that, whatever n_tables: one upload of the descriptors' records (the workspace's ring of pinned, event-guarded
 * slots, shared with tfra_multi_find_combine: calls may follow each other with no host synchronisation, and the stream is never
 * waited for once ws has its size), one memset, one bounds launch, one denominator launch and one entry-record launch over all
 * descriptors, one sums launch per NCH class in the list (NCH = ceil(dim / 64): 1..4), one update launch per (rule, storage
 * type) class in the list, and one eviction-phase launch per such class that holds a table at max_capacity.  The scratch of all
 * descriptors (bounds, denominators, entry records) lives in ws; partial sums stay in each plan.
 * *launches_out (optional, host): the kernel launches enqueued =
 *   3 + (NCH classes present) + ((rule, storage type) classes present) + ((rule, storage type) classes with a table at max_capacity),
 * 0 when no descriptor has ids.  26 growing float32 tables of dims 16 / 32 / 64 / 128 with one rule: 3 + 2 + 1 = 6.
 * A descriptor whose table has TFRA_OPTION_STOCHASTIC_ROUNDING on is checked with the others and then served by the single call's
 * launches, on the same stream, behind the grouped ones (the grouped kernels round to nearest even); *launches_out counts the
 * grouped launches only.
 * The plans are built per plan (tfra_sparse_plan_build) or by tfra_multi_sparse_plan_build below.  Not for stream capture. */
typedef struct {
  uint32_t struct_size;              /* = sizeof(tfra_apply_combined_desc) */
  int32_t  combiner;                 /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;
  const tfra_opt_params* opt;        /* per descriptor; usually the same for all */
  const tfra_sparse_plan_t* plan;    /* CSR plan built over this table's ENTRY ids (tfra_sparse_plan_build, dim = table dim) */
  const float* grad_out;             /* [n_rows, dim] float32 */
  const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows;
  const float* param_default_row;    /* [dim] float32 */
} tfra_apply_combined_desc;
int tfra_multi_apply_planned_combined(tfra_workspace_t* ws, size_t n_tables, const tfra_apply_combined_desc* descs,
                                      uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The same with each descriptor's grad_out as a tfra_grads record — half-precision gradients, above: table i ends bit-identical to
 * tfra_table_apply_planned_combined_typed on its descriptor.  Descriptors of all three formats, with and without a scale, may
 * stand in one list; each is checked as the single typed call checks it, all of them before anything is enqueued, and a refused
 * list writes nothing (the message names the descriptor's index).  Everything else is tfra_multi_apply_planned_combined's.
 * The format is one more axis of the launch classes, with two values — float32, or half (float16 and bfloat16 share a launch:
 * the format is a wave-uniform value in the descriptor's record).
 * *launches_out (optional, host): the kernel launches enqueued =
 *   3 + ((NCH, float-or-half) classes present) + ((rule, storage type, float-or-half) classes present)
 *     + ((rule, storage type, float-or-half) classes with a table at max_capacity),
 * 0 when no descriptor has ids.  A list that is all half or all float has the untyped call's count (26 growing float32 tables of
 * dims 16 / 32 / 64 / 128 with one rule: 6); with one float32 descriptor of dim 16 among 25 bfloat16 ones: 3 + 3 + 2 = 8.
 * A descriptor whose table rounds stochastically is served by tfra_table_apply_planned_combined_typed behind the grouped launches. */
typedef struct {
  uint32_t struct_size;              /* = sizeof(tfra_apply_combined_typed_desc) */
  int32_t  combiner;                 /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;
  const tfra_opt_params* opt;
  const tfra_sparse_plan_t* plan;
  tfra_grads grad_out;               /* [n_rows, dim] in grad_out.dtype, with its optional device scale */
  const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows;
  const float* param_default_row;    /* [dim] float32 */
} tfra_apply_combined_typed_desc;    /* 88 bytes */
int tfra_multi_apply_planned_combined_typed(tfra_workspace_t* ws, size_t n_tables, const tfra_apply_combined_typed_desc* descs,
                                            uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* The CSR plans of MANY batches in one call (a 26-table model's write-back plans are 26 tfra_sparse_plan_build calls = 78 launches
 * otherwise): descs[i].plan ends as tfra_sparse_plan_build(plan, n, ids, dim, stream) leaves it — the same device code runs, with
 * the same arithmetic and placement rules: the CSR's content per key (tfra_sparse_plan_read) and every write-back through the plan
 * are bit-identical; where a key's records land inside the plan's buffers differs from run to run, as between two single builds.
 * Every rule of that call holds per descriptor (dim % 4 == 0, dim <= 256, at most 2^18 ids, ids complete in memory in stream
 * order, the caller orders build and use).  n == 0: the plan is left empty and takes no blocks.  n_plans == 0: TFRA_OK.
 * All descriptors are checked BEFORE any plan is touched: if one fails, the call returns the code the single call returns for it
 * (the message names the descriptor's index, then the single call's text), nothing is enqueued and every plan of the list still
 * holds its previous build.  Only a descriptor can get these wrong: a wrong struct_size, a plan on another device than ws, or
 * descs == NULL with n_plans > 0: TFRA_ERR_INVALID; dim == 0 (the assign-only plan is one kernel already): TFRA_ERR_UNSUPPORTED;
 * the same plan in two descriptors: TFRA_ERR_INVALID, the message names both indices.
 * Everything that can fail for memory or that synchronises comes before the first enqueue as well: a plan that outgrew its buffer
 * is reallocated there (hipDeviceSynchronize + hipFree + hipMalloc, as in the single call), and ws takes its size.
 * Enqueues after that, whatever n_plans: per plan that is new, was reallocated or whose number of merge buckets changed, the
 * memsets the single call enqueues for it (none in the steady state); one upload of the plans' records (the workspace's ring of
 * pinned, event-guarded slots, shared with the other grouped calls); one tile launch and one scatter launch over all plans' tiles
 * (512 ids each) and one merge-bucket launch per pass size present in the list (512, or 1024 for a plan of more than 131072 ids).
 * *launches_out (optional, host): the kernel launches enqueued = 2 + (pass sizes present): 3 for any list whose plans hold at most
 * 131072 ids each, 0 when no descriptor has ids.  ws must be a workspace of the stream's own (the ring and the records are its
 * state): a build on a side stream next to another grouped call on the main stream uses two workspaces.  Not for stream capture. */
typedef struct { uint32_t struct_size; tfra_sparse_plan_t* plan; size_t n; const int64_t* ids; int dim; } tfra_plan_build_desc;
int tfra_multi_sparse_plan_build(tfra_workspace_t* ws, size_t n_plans, const tfra_plan_build_desc* descs,
                                 uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

/* default_partition_fn(PY/dynamic_embedding_variable.py:165-197) + dynamic_partition in one
 * pass: owner[i] = mode 0: (key & 0x7fffffff) % num_shards (CUDA-build branch)
 *                  mode 1: floor_mod(key, num_shards)       (CPU-build branch)
 *                  mode 2: fmix64(key) % num_shards         (opt-in, Zipf-balanced)
 * Produces owner-major keys_out, perm_out (original index of each output element, i.e. the
 * dynamic_partition of range(n)) and d_counts[num_shards] (device int64).
 * d_n: optional DEVICE int64 scalar; when non-NULL only the first min(n, *d_n) keys are partitioned
 * (chains after tfra_unique without reading the unique count on the host).                  */
int tfra_partition(tfra_workspace_t* ws, size_t n, const int64_t* d_n, const int64_t* keys, int num_shards,
                   int mode, int64_t* keys_out, int32_t* perm_out, int64_t* d_counts, tfra_stream_t stream);

/* Same, for a caller-computed owner[i] in [0,num_shards) (custom `partitioner=` functions,
 * PY/dynamic_embedding_variable.py:484-500): only perm_out and d_counts are produced. */
int tfra_partition_by_owner(tfra_workspace_t* ws, size_t n, const int32_t* owner, int num_shards,
                            int32_t* perm_out, int64_t* d_counts, tfra_stream_t stream);

/* dynamic_stitch for one flat permutation: out[perm[i],:] = in[i,:]. */
int tfra_scatter_rows(size_t n, size_t row_bytes, const void* in, const int32_t* perm, void* out,
                      tfra_stream_t stream);

/* Size restriction (PY/restrict_policies.py:205-230,332-358 do export -> top_k(-status)
 * -> gather -> remove in Python): keys_out[0..k) = the k keys with the LOWEST status (timestamp or
 * frequency), ties resolved in input order (stable).  status_dtype TFRA_I32 or TFRA_I64; k <= n.
 * Feed keys_out to tfra_table_erase of the parameter table and of the status table.            */
int tfra_select_lowest(tfra_workspace_t* ws, size_t n, const int64_t* keys, const void* status,
                       int status_dtype, size_t k, int64_t* keys_out, tfra_stream_t stream);

/* -- multi-GPU routed step issued from C (the route of HvdAllToAllEmbedding,
 *    PY/shadow_embedding_ops.py:397-447 / DE/python/keras/layers/embedding.py:545-594, prepared ahead of the step).
 *
 *    A transport moves peer-major device buffers between the ranks of one job: send_bytes[r] bytes go to rank r,
 *    recv_bytes[r] bytes arrive from it (an alltoallv), enqueued on `stream`.  channel 0 carries rows and gradients
 *    (the critical path of a step), channel 1 the counts and ids of later batches; the two never wait for each other.
 *    Every rank issues the same sequence of calls.  tfra_rccl_transport_* is the RCCL one (grouped ncclSend/ncclRecv
 *    over xGMI, one communicator per channel; librccl is dlopen()ed from `librccl_path`, the copy the host framework
 *    already loaded); tests plug a host-staged transport into the same driver.                                       */
typedef struct {
  void* ctx;
  int rank, world;
  int (*alltoallv)(void* ctx, int channel, const void* send, const size_t* send_bytes, void* recv,
                   const size_t* recv_bytes, tfra_stream_t stream);
  /* optional (NULL: the driver issues two alltoallv): TWO independent alltoallv as ONE exchange — the RCCL transport groups all their
   * sends / recvs into one ncclGroup, one kernel instead of two (the count exchange of one batch with the id exchange of another) */
  int (*alltoallv2)(void* ctx, int channel, const void* send_a, const size_t* send_bytes_a, void* recv_a, const size_t* recv_bytes_a,
                    const void* send_b, const size_t* send_bytes_b, void* recv_b, const size_t* recv_bytes_b, tfra_stream_t stream);
} tfra_transport;
#define TFRA_RCCL_ID_BYTES 128
int tfra_rccl_unique_id(const char* librccl_path, void* id_out /* TFRA_RCCL_ID_BYTES, host */);
/* ids: 2 x TFRA_RCCL_ID_BYTES (one per channel), made by rank 0 and distributed by the caller; call on every rank */
int tfra_rccl_transport_create(const char* librccl_path, const void* ids, int rank, int world, int device,
                               tfra_transport* out);
int tfra_rccl_transport_destroy(tfra_transport* tr);
/* ranks of the transport's communicators as RCCL itself reports them (ncclCommCount, both channels) */
int tfra_rccl_transport_ranks(const tfra_transport* tr, int* out);

/*    The driver.  feed() hands a batch to the id-only half of the route, which runs ahead of the step on the driver's
 *    own streams: the de-duplication plan of the batch and its distinct ids grouped by owner (a helper thread launches
 *    these), the count exchange, the split sizes on their way to pinned memory, the id exchange, the position ->
 *    returned-row map and the plan of the ids this rank serves.  A batch moves one stage per step, so keep THREE batches
 *    fed ahead of the one being looked up and nothing ever waits (fewer works too: the missing stages then run, and
 *    stall, inside lookup).  Every collective is issued by the calling thread at points that depend on the call
 *    sequence alone, so all ranks issue them in the same order.
 *      lookup : rows_out[i,:] = row of ids[i] of the OLDEST fed batch (owner's find, default row for missing keys,
 *               alltoall of the rows, one gather)
 *      apply  : gradient rows of that batch -> per-key sums in owner-major order -> alltoall -> fused sparse update at
 *               the owner (tfra_table_apply_planned: sums the <= world parts of a key in a fixed order); retires it
 *    transport NULL: one rank, buffers are copied on the device.  fp32 rows, dim % 4 == 0, dim <= 256, batches of at
 *    most max_batch <= 2^18 ids; the ids a rank serves per batch must not exceed 2^18.  One caller thread.
 *    flags: TFRA_ROUTE_NO_THREAD = everything is issued by the calling thread.                                      */
#define TFRA_ROUTE_NO_THREAD 1u
typedef struct tfra_route tfra_route_t;
int tfra_route_create(tfra_table_t* table, const tfra_transport* transport, int partition_mode, size_t max_batch,
                      uint32_t flags, tfra_route_t** out);
int tfra_route_destroy(tfra_route_t* r);
int tfra_route_feed(tfra_route_t* r, size_t n, const int64_t* d_ids, int ids_ready, tfra_stream_t stream);
int tfra_route_lookup(tfra_route_t* r, float* d_rows_out, const float* default_row, tfra_stream_t stream);
int tfra_route_apply(tfra_route_t* r, const tfra_opt_params* p, const float* d_grads, const float* param_default_row,
                     tfra_stream_t stream);
/* ids this rank serves for the oldest fed batch (device pointer valid until its apply; waits for the split sizes) */
int tfra_route_served_ids(tfra_route_t* r, const int64_t** d_ids, size_t* n, size_t* n_distinct_local);

/* -- the metric's step on a hash-sharded table: lookup(B) + insert_or_assign(B) with ids / rows / values routed ---------------
 *    (csrc/tfra_aroute.hip).  Replaces, for a table sharded over the GPUs of one node, the reference's sequence
 *      lookup : HvdAllToAllEmbedding.__alltoall_embedding_lookup__  (PY/shadow_embedding_ops.py:397-447: unique -> partition ->
 *               hvd.alltoall(ids) -> local Find -> hvd.alltoall(rows) -> stitch)
 *      insert : Variable.upsert on a sharded Variable            (PY/dynamic_embedding_variable.py:772-800: keys AND values
 *               partitioned by owner, one Insert per shard; the last occurrence of a repeated key wins)
 *    with TWO launches per batch (route plan: insert + emit) for everything that depends on the ids alone (de-duplication, grouping by owner, last positions,
 *    position -> row map: runs ahead, on the driver's own streams, followed by the count exchange, the one host read of the split
 *    sizes and the id exchange) and, per step on the caller's stream: gather(values at the last positions) -> alltoall(values) ->
 *    tfra_table_step_overlap at the owner (lookup of the ids it serves for THIS batch + write-back of the rows it received for the
 *    PREVIOUS one, one launch) -> alltoall(rows) -> gather(rows -> positions).
 *    Results = ONE table that sees, per step, lookup(every rank's ids) and then insert_or_assign(rank 0's batch, rank 1's, ...):
 *    a key written by several ranks in one step keeps the highest rank's last occurrence; lookup i+1 sees every write of step i.
 *      feed  : announce a batch (ids must stay valid and unchanged until the batch has been written back).  A batch moves one
 *              stage of its route per step: keep FIVE batches fed ahead of the one being looked up and nothing waits on the
 *              host (fewer works too: the missing stages then run, and stall, inside step; the owner's overlapped step then
 *              builds its de-duplication plans by launches of their own).  At most six.
 *      step  : rows_out[i,:] = row of ids[i] of the OLDEST fed batch not yet looked up (default_row for missing keys: one row);
 *              values_prev [n_prev, dim] = the rows to assign to the ids of the batch the PREVIOUS step looked up (NULL on the
 *              first step / after a flush); they must stay unchanged until this call's work has run.
 *      flush : writes the last looked-up batch back.  Call it before the table is used through any other entry point.
 *    transport NULL: one rank (device copies where the alltoalls would be).  Any value type; batches of at most max_batch <= 2^18
 *    ids, at most 2^18 ids served per rank and batch, at most 64 ranks.  Every rank issues the same call sequence; one caller thread.
 *    stats out6: steps, host stalls on split sizes, owner steps taken overlapped / one op after the other, distinct ids of the last
 *    batch looked up, ids this rank served for it. */
typedef struct tfra_assign_route tfra_assign_route_t;
int tfra_assign_route_create(tfra_table_t* table, const tfra_transport* transport, int partition_mode, size_t max_batch,
                             tfra_assign_route_t** out);
int tfra_assign_route_destroy(tfra_assign_route_t* r);
int tfra_assign_route_feed(tfra_assign_route_t* r, size_t n, const int64_t* d_ids, int ids_ready, tfra_stream_t stream);
int tfra_assign_route_step(tfra_assign_route_t* r, void* d_rows_out, const void* default_row, const void* values_prev,
                           tfra_stream_t stream);
int tfra_assign_route_flush(tfra_assign_route_t* r, const void* values_prev, tfra_stream_t stream);
int tfra_assign_route_stats(const tfra_assign_route_t* r, uint64_t* out6);
/* measurement: tfra_step_driver_time_kernels / _kernel_times of the owner's step driver (the step launch of the next `steps` steps) */
int tfra_assign_route_time_kernels(tfra_assign_route_t* r, size_t steps);
int tfra_assign_route_kernel_times(tfra_assign_route_t* r, double* step_kernel_us, size_t* steps);

/* -- Half-precision OUTPUTS of the lookups: the forward counterpart of tfra_grads.  A bfloat16 / float16 model over
 *    a float32 master table gets its activations in its own type from the lookup's kernel, and a half table feeding a float32 model
 *    gets float32, with no conversion pass behind the call.  Additive; ABI version 1.
 *    Contract: a typed call equals its untyped twin (tfra_table_find / tfra_table_find_n, tfra_table_find_combine,
 *    tfra_table_find_combine_ragged, tfra_multi_find_combine, tfra_multi_find_combine_ragged) followed by the elementwise
 *    conversion of the twin's output to `dtype`, bit for bit.
 *      f32() of a half value is the exact up-cast: subnormals are kept, a NaN stays a NaN.
 *      float32 -> float16 / bfloat16 is round to nearest even: ties go to even, the result is infinity beyond the largest finite
 *      value, results in the subnormal range are kept, a NaN stays a NaN.  bfloat16 is the library's f32_to_bf16 (a NaN keeps its
 *      upper 16 bits and gets bit 6 set); float16 is the hardware conversion (the _Float16 cast).
 *      A half table read out in the OTHER half type goes through float32: exact up-cast, then the rounding above.
 *      defaults / default_row stay in the TABLE's value dtype, as in the twins, and are converted the same way.
 *    Everything in front of the conversion is the twin's: the probe (plain loads, reserved keys), exists, the clamping of
 *    row_splits, PRUNE / FILL (the fill row is converted as it is: a -0.0 survives), entries in no row, zero rows, the accumulation
 *    order, float32 accumulators, nnz == 0, and the launches: a typed call enqueues what its twin enqueues.
 *    tfra_table_find_typed with dtype == the table's value dtype forwards to tfra_table_find / tfra_table_find_n, and a pooled call
 *    with dtype == TFRA_F32 forwards to its twin: the same code, the same launches.
 *    Limits: the pooled calls keep their twins' (float32 / float16 / bfloat16 tables, dim % 4 == 0, dim <= 256).  tfra_table_find_typed
 *    takes on the same limits (its conversion works on 4-element granules) and serves field 0 only; d_n may be NULL (the count is n).
 *    A half output is addressed with the twin's size_t row offsets: no new size limit.
 *    Refused before anything is enqueued (tfra_last_error() names the function and, in the grouped calls, the descriptor's index;
 *    nothing is written to any output):
 *      TFRA_ERR_INVALID      a NULL record, or NULL rows with rows to write; reserved != 0; a dtype other than the three; a wrong
 *                            struct_size
 *      TFRA_ERR_UNSUPPORTED  rows misaligned (float32: 16 bytes, halves: 8 bytes); the dim / value dtype limits
 *      and everything the twin checks, with the twin's codes and wording (a find's defaults must be aligned as its rows are read:
 *      float32 tables 16 bytes, half tables 8).
 *    Not typed: the tier calls (tfra_tier_*), tfra_table_find_field, tfra_table_find_unique, the find_or_insert family, the step
 *    drivers and the routes: they write the table's value dtype (the pooled ones float32). */
typedef struct {
  void*   rows;      /* [n, dim] row-major in `dtype`; float32: 16-byte aligned, halves: 8-byte aligned */
  int32_t dtype;     /* TFRA_F32 | TFRA_F16 | TFRA_BF16 */
  int32_t reserved;  /* must be 0 */
} tfra_rows_out;     /* 16 bytes */
int tfra_table_find_typed(tfra_table_t* t, size_t n, const int64_t* d_n /* may be NULL */, const int64_t* keys,
                          const tfra_rows_out* out, uint8_t* exists, const void* defaults, int default_is_full,
                          tfra_stream_t stream);
int tfra_table_find_combine_typed(tfra_table_t* t, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                  const float* weights, int combiner, size_t n_rows, const void* default_row,
                                  const tfra_rows_out* out, tfra_stream_t stream);
int tfra_table_find_combine_ragged_typed(tfra_table_t* t, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                         const int64_t* ids, const float* weights, int combiner, uint32_t flags,
                                         int64_t fill_id, const void* default_row, const tfra_rows_out* out,
                                         tfra_stream_t stream);
/* The grouped forms: tfra_multi_find_combine / tfra_multi_find_combine_ragged over plain tables, each descriptor with an output
 * record of its own.  The output type is one more launch-class axis — (value dtype, NCH, out dtype[, safe or not]) — so a list
 * with ONE output type keeps the twin's launch count. */
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_typed_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;
  size_t nnz; const int64_t* ids; const int64_t* seg; const float* weights;   /* weights may be NULL */
  size_t n_rows; const void* default_row; tfra_rows_out out;                  /* out.rows [n_rows, table dim] in out.dtype */
} tfra_find_combine_typed_desc;
int tfra_multi_find_combine_typed(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_typed_desc* descs,
                                  uint32_t* launches_out /* optional, host */, tfra_stream_t stream);
typedef struct {
  uint32_t struct_size;      /* = sizeof(tfra_find_combine_ragged_typed_desc) */
  int32_t  combiner;         /* 0 sum | 1 mean | 2 sqrtn */
  tfra_table_t* table;
  size_t n_rows; const int64_t* row_splits;                                   /* [n_rows + 1] */
  size_t nnz; const int64_t* ids; const float* weights;                       /* weights may be NULL */
  uint32_t flags; uint32_t reserved;                                          /* TFRA_RAGGED_*; reserved = 0 */
  int64_t fill_id; const void* default_row; tfra_rows_out out;                /* out.rows [n_rows, table dim] in out.dtype */
} tfra_find_combine_ragged_typed_desc;
int tfra_multi_find_combine_ragged_typed(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_ragged_typed_desc* descs,
                                         uint32_t* launches_out /* optional, host */, tfra_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TFRA_MI355X_H_ */
