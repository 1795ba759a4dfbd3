// The write-back plan object (tfra_sparse_plan_t) and the host helpers the units of the write-back share:
//   tfra_csr.hip      the CSR plan (gradients): its builders, the object's life, tfra_sparse_plan_read, the route helpers
//   tfra_setplan.hip  the SET plan (assign-only): its builders, and the unique / find+unique ops built on it
//   tfra_apply.hip    the gradient half: hot sums + the fused optimizer update (device bodies: tfra_apply_device.h, checks: tfra_apply.h)
//   tfra_apply_many.hip  the grouped combined write-back (tfra_multi_apply_planned_combined)
//   tfra_prefetch.hip the two-stream look-ahead driver (tfra_table_step_prefetch[_assign]); no kernel of its own
//   tfra_own.hip      the assign half: the ownership pass + its remainder
//   tfra_step.hip     the overlapped step's driver (its kernel: tfra_step_impl.h)
//   tfra_find_insert.hip  find_or_insert over a CSR plan's keys (tfra_table_find_or_insert_planned)
//   tfra_tierplan.hip  the same over a tier (tfra_tier_find_or_insert_planned)
//   tfra_rows.hip     whole rows and gradient sums of a CSR plan's keys (tfra_table_fetch_planned)
// The object holds types of tfra_plan_device.h (anonymous namespace): every unit includes the same definitions, so it has one
// layout.  A helper shared across units cannot take or return such a type (its linkage would be internal): the shared ones below
// take the plan object, pointers and scalars; keys_of, which returns one, is defined here for each unit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_host.h"
#include "tfra_own_device.h"
#include "tfra_plan_device.h"

// ---------------------------------------------------------------------------------------------
struct tfra_sparse_plan {
  int device = 0;
  void* buf = nullptr;
  size_t bytes = 0;
  // layout of the last build
  size_t n = 0, npad = 0, ntiles = 0;
  unsigned P = 0, cm = 0;
  int dim = 0;
  unsigned* cursors = nullptr;
  CsrDesc ds{};
  CsrOut out{};
  unsigned* tile_entries = nullptr;
  unsigned short* run_start = nullptr;
  unsigned* tile_len = nullptr;
  uint4* drec = nullptr;
  unsigned* keymap = nullptr;
  i64* dkeys = nullptr;
  unsigned* binmap = nullptr;
  unsigned* d_counts = nullptr;     // the control words of the last build (PC_*, tfra_plan_device.h): the CSR buffer's, or set_counts
  uint8_t* dflag = nullptr;
  size_t dflag_len = 0;
  OwnItem* slow_items = nullptr;   // [SLOW_CAP] left-over keys of the ownership pass of a write-back (self-contained items)
  unsigned* any_deferred = nullptr;   // = use_gen of the last write-back that deferred a key to its eviction phase
  mutable unsigned use_gen = 0;
  mutable unsigned ups_uses[2] = {0, 0};   // upsert_planned uses of the CSR buffer / of the SET buffer: the parity selects the left-over
                                           // counter set of THAT buffer (each buffer has its own two sets and its own flag bytes: a plan
                                           // object rebuilt with dim > 0, then dim 0, then dim > 0 again must find its CSR buffer's sets
                                           // where its last CSR use left them)
  float* partial = nullptr;
  int* prow_dest = nullptr;        // [partial rows] scratch of tfra_plan_positions_to
  bool armed = false;              // cursors/counters are zero (re-armed by the last kernel of the previous build)
  unsigned* host_counts = nullptr; // pinned copy of a CSR build's published words (HC_*, tfra_plan_device.h)
  unsigned gen = 0;                // generation of the last enqueued build
  bool ev_recorded = false;        // the last build ran on a side stream (tfra_table_step_prefetch)
  unsigned last_used_step = 0;     // last step whose write-back read this plan
  hipEvent_t built_ev = nullptr;   // recorded behind a build on a side stream (tfra_table_step_prefetch): complete = the plan is in memory
  // SET plan (dim 0): its own buffer; two tables alternate (setplan_kernel)
  int kind = 0;                    // 0 CSR, 1 SET
  void* setbuf = nullptr;
  size_t set_cap = 0;              // ids the set buffer was sized for
  unsigned set_m2 = 0;
  SetTab set_tab[2]{};
  unsigned set_parity = 0;         // table of the last build
  unsigned* set_counts = nullptr;  // the control words of the set buffer (PC_* and SC_*, tfra_plan_device.h)
  unsigned set_use[2] = {0, 0};    // uses of each table so far
  bool built_counts = true;        // the last build counted occurrences
  bool skip_counts_once = false;   // the NEXT build need not count occurrences (set by the table's own drivers for tables whose
                                   // scores do not read them; a build through the public entry point always counts)
  uint8_t* set_dflag = nullptr;
  OwnItem* set_items = nullptr;
  // the overlapped step (tfra_step_impl.h) builds a SET plan in two launches without atomics: launch 1 scatters every tile's
  // distinct (id, last position) pairs into per-window segments, launch 2 builds each window of the table from its segments
  void* segbuf = nullptr;
  size_t seg_cap_ids = 0;          // ids the scatter buffers were sized for
  SetEnt* seg_pairs = nullptr;     // [windows][tiles][SEG_CAP]
  unsigned* seg_cnt = nullptr;     // [windows][tiles]
  SetEnt* ovf_pairs = nullptr;     // pairs that did not fit their segment (an adversarial batch): appended with an atomic
  unsigned* ovf_cnt = nullptr;
  unsigned* ucnt = nullptr;        // [windows <= 256] distinct keys per window of the last list-less build (the step launch's BUILD role)
  unsigned seg_tiles = 0;          // tiles of the last scatter
  unsigned scat_use = 0;           // scatters into this object so far (its two overflow counters alternate)
  const int64_t* scat_ids = nullptr;   // the batch whose pairs the segments hold (nullptr: none)
  size_t scat_n = 0;
  unsigned char tab_state[2] = {0, 0}; // what each table holds (TAB_*; the build rules: setplan_prepare, tfra_setplan.hip)
  bool ever_built = false;         // a build call has reached this object (n == 0 since: a batch of 0 ids, not "never built")
};
enum : unsigned char { TAB_EMPTY = 0, TAB_LISTED = 1, TAB_LISTLESS = 2 };

namespace tfra {

// ---- tfra_setplan.hip
// The SET plan of a batch (dim 0) on stream s; counts: also the occurrences of every id (see setplan_kernel)
int setplan_build(tfra_sparse_plan* pl, size_t n, const int64_t* ids, hipStream_t s, bool counts);
// A build without the dense list, made by the overlapped step's launch: the scatter buffers for n ids, then the bookkeeping of
// the build launch (the object's other table takes the build: pl->set_tab[pl->set_parity] afterwards)
int setplan_prepare_listless(tfra_sparse_plan* pl, size_t n, hipStream_t s);
void setplan_take_listless(tfra_sparse_plan* pl, size_t n);
// n SET entries (SetEnt) set free, with one small launch on stream s
void setplan_fill_empty(void* ent, size_t n, hipStream_t s);

// ---- tfra_csr.hip
void plan_grids(const tfra_sparse_plan* pl, unsigned* key_blocks, unsigned* bin_blocks);
int own_plan(Table* t, tfra_sparse_plan** out);

// ---- tfra_apply.hip (callers: tfra_prefetch.hip, and the unit itself)
int apply_planned_impl(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl, const float* grads,
                       const float* param_default_row, tfra_stream_t stream, unsigned* progress, unsigned progress_val,
                       const CombEnt* comb = nullptr, const tfra_grads* hg = nullptr);
// the hot sums of a plan, as tfra_reduce_by_key launches them (hg: a checked half matrix, else `grads`); caller: tfra_rows.hip
void hot_sums_launch(hipStream_t s, const tfra_sparse_plan_t* pl, const float* grads, const tfra_grads* hg, unsigned bin_blocks);

// ---- tfra_own.hip
// Host half of an ownership write-back of a plan's keys: everything but the launches (upsert_planned_impl launches the pair
// upsert_own_kernel + upsert_rest_kernel, the overlapped step puts the pass into its one launch).
struct OwnLaunch {
  OwnArgs a;
  OwnCtrs* ctr; OwnCtrs* next_ctr;
  unsigned og;            // bucket-owner generation of this launch (0: no owner tags)
  unsigned key_blocks;    // the plan's keys / 16, as far as the host knows them
  unsigned rem_blocks;    // grid of the remainder pass
  bool simple;
  int g;                  // copy granule
};
int own_prepare(Table* t, const tfra_sparse_plan_t* pl, const void* values, const uint64_t* scores, hipStream_t s,
                const unsigned* progress, OwnLaunch* L);
int upsert_planned_impl(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const void* values, const uint64_t* scores,
                        tfra_stream_t stream, unsigned* progress, unsigned progress_val);

}  // namespace tfra

static inline CsrKeys keys_of(const tfra_sparse_plan* pl) {
  if (pl->kind == 1) {
    // a SET use block is laid out as the head of a CSR d_counts block on purpose (tfra_plan_device.h): d_counts = the block of
    // the table's current use, in which tb.count is word SC_USE_COUNT
    const SetTab& tb = pl->set_tab[pl->set_parity];
    return CsrKeys{nullptr, nullptr, nullptr, nullptr, nullptr, tb.count - SC_USE_COUNT, tb.ukeys, tb.uslot, tb.ent};
  }
  return CsrKeys{pl->keymap, pl->dkeys, pl->out.crec, pl->out.hrec, pl->out.hent, pl->d_counts, nullptr, nullptr, nullptr};
}
