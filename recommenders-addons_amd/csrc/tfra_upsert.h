// What the three units of the locked upsert family (tfra_upsert.hip, tfra_find_insert.hip, tfra_accum.hip) share on the host, ONE
// copy each: the entry check of a batch call, the scratch of the eviction phase, and that phase's launch.  The first two are
// file-local in each unit (static), as the frames of tfra_apply.h.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "tfra_host.h"
#include "tfra_upsert_device.h"

// The refusals every batch call of the family makes, in the order every one of them makes them: a null buffer, the call's own checks
// (`more`, which records its own error), then the key count.  `who` is the call's prefix of both texts ("insert: ", ...);
// who_count: the prefix of the count's text where it is another.
struct NoMoreChecks { int operator()() const { return TFRA_OK; } };
template <class More = NoMoreChecks>
static int check_batch(const char* who, size_t n, bool buffers, More&& more = More{}, const char* who_count = nullptr) {
  if (!buffers) return set_error(TFRA_ERR_INVALID, std::string(who) + "null buffer");
  if (int rc = more()) return rc;
  if (n >= (1ULL << 31)) return set_error(TFRA_ERR_INVALID, std::string(who_count ? who_count : who) + "more than 2^31-1 keys per call");
  return TFRA_OK;
}

// Scratch of a two-phase call on a table at max_capacity, carved out of t->scratch in this order, each part 256-B aligned:
// [n] phase-2 flags | [n] per-key scores (want_scores) | [n, spill_row_bytes] rows phase 2 reads instead of the caller's (0: none).
// Takes the scratch head, so the armed cursor area is given up (apply_P).
// The table has a SECOND flag buffer, Table::bounded_flags: accum_or_assign and the fused write-backs keep their flags there,
// because the ownership pass they may run first, and the cursor area a write-back arms, live at the head of t->scratch.
struct EvictScratch {
  uint8_t* deferred = nullptr;
  u64* key_scores = nullptr;
  unsigned char* spill = nullptr;
};
static int carve_evict_scratch(Table* t, hipStream_t s, size_t n, bool want_scores, size_t spill_row_bytes, EvictScratch* es) {
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t score_bytes = want_scores ? al(n * 8) : 0;
  int rc = t->ensure_scratch(al(n) + score_bytes + n * spill_row_bytes, s);
  if (rc) return rc;
  t->apply_P = 0;
  unsigned char* w = (unsigned char*)t->scratch;
  es->deferred = w;
  if (want_scores) es->key_scores = (u64*)(w + al(n));
  if (spill_row_bytes) es->spill = w + al(n) + score_bytes;
  return TFRA_OK;
}

// Phase 2 of a bounded-table upsert, the ONE launch of insert_evict_kernel (tfra_upsert.hip): the keys whose flag in `deferred` is
// set replace the minimum-score entry of their home buckets by row i of src_rows and scores[i] (null: 1).  g: the copy granule of
// table row and src_rows.  eo: the capturing instance (tfra_table_insert_and_evict), one granule for the output rows too.
// whole_in (with eo only): src_rows are whole co-located rows, written and reported as such (TFRA_INSERT_WHOLE_ROWS).
// (Hidden: shared by the library's units, not one of its dynamic symbols.)
__attribute__((visibility("hidden"))) void evict_phase(Table* t, hipStream_t s, const TableView& v, int g, size_t n, const i64* keys, const unsigned char* src_rows,
                 const u64* scores, unsigned field, const uint8_t* deferred, const EvictOut* eo = nullptr, bool whole_in = false);

// The body of tfra_table_insert_and_evict_n behind its argument checks, for a caller that holds the table's lock and has entered it
// on s (the call itself; the tier driver, tfra_tierstep.hip): the locked two-phase upsert of min(n, *d_n) unique keys (d_n null: n).
// whole_in: `values` rows are whole co-located rows.  eo: looked at on a table at max_capacity only; null there: nothing is
// reported (whole rows are only written by the capturing instance: whole_in without eo is refused there).
__attribute__((visibility("hidden"))) int insert_counted(Table* t, hipStream_t s, size_t n, const long long* d_n, const i64* keys, const unsigned char* values,
                   const u64* scores, bool whole_in, const EvictOut* eo);
