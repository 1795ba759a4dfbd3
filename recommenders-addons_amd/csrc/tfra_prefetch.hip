// The two-stream look-ahead driver (tfra_table_step_prefetch[_assign]): one training step driven from C, the next batch's plan
// built on a side stream meanwhile.  It launches no kernel of its own: the lookup is tfra_table_find, the plan tfra_sparse_plan_build,
// the write-back apply_planned_impl (tfra_apply.hip) or upsert_planned_impl (tfra_own.hip).  tfra_multi.hip drives several tables
// through these calls.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/tfra_mi355x.h"
#include "tfra_host.h"
#include "tfra_plan.h"

using namespace tfra;

// A pinned block of `bytes` bytes in *slot on first use, zeroed.  false: no memory, and *slot stays null.
static bool pinned_on_first_use(unsigned** slot, size_t bytes) {
  if (*slot) return true;
  if (hipHostMalloc((void**)slot, bytes, hipHostMallocDefault) != hipSuccess) { *slot = nullptr; return false; }
  memset(*slot, 0, bytes);
  return true;
}

// ---------------------------------------------------------------------------------------------
// One training step driven from C on two streams (no Python between the launches, no graph).
//   main : lookup(ids_cur) -> write-back of batch cur (hot sums + fused update, or assign)      (plan_cur)
//   side : build plan_next from ids_next, free-running
// Cross-queue events cost ~5 us (stream wait) / ~7 us (record) each between two kernels of the main stream,
// so the two streams are ordered through two host-visible counters in pinned memory instead, and the host
// only falls back to a sync when a counter lags:
//   * table progress: written by the first block of the write-back of step s  =>  every earlier step is done.
//     plan_next's buffers were last read by step plan_next->last_used_step; the build is enqueued once the
//     progress has passed it (with >= 3 plans in rotation that is always the case unless the host is far
//     ahead of the GPU, in which case it waits here instead of in a queue);
//   * plan built: generation + counts written by the build's last kernel.  If they already show plan_cur's
//     generation the write-back is enqueued without any wait packet and with exact grids; otherwise — the host
//     got ahead of the side stream — the host waits for the side stream.
static int step_prefetch_impl(tfra_table_t* tp, const tfra_opt_params* p, tfra_sparse_plan_t* plan_cur,
                              const int64_t* ids_cur, void* rows_out, const void* find_default, const void* grads_or_values,
                              const float* param_default_row, const uint64_t* scores, tfra_sparse_plan_t* plan_next,
                              const int64_t* ids_next, size_t n_next, tfra_stream_t main_stream, tfra_stream_t side_stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t || !plan_cur) return set_error(TFRA_ERR_INVALID, "step_prefetch: null argument");
  hipStream_t ms = (hipStream_t)main_stream, ss = (hipStream_t)side_stream;
  if (ms == ss && plan_next) return set_error(TFRA_ERR_INVALID, "step_prefetch: needs two different streams");
  if (plan_next == plan_cur) return set_error(TFRA_ERR_INVALID, "step_prefetch: plan_next must differ from plan_cur");
  std::lock_guard<std::mutex> step_lock(t->step_mu);   // one driver call at a time per table
  int rc = TFRA_OK;
  if (p && t->stochastic() && t->capture_safe)   // the write-back would refuse it (check_rounding) behind the lookup: refuse in front
    return set_error(TFRA_ERR_UNSUPPORTED, "step_prefetch: TFRA_OPTION_STOCHASTIC_ROUNDING and TFRA_OPTION_CAPTURE_SAFE are both set "
                                           "(a replayed graph would reuse one call index)");
  if (!pinned_on_first_use(&t->progress_host, 64)) return set_error(TFRA_ERR_OOM, "step_prefetch: hipHostMalloc");
  const unsigned step = ++t->step_gen;
  if (plan_next) {
    // (all 16 words: the build publishes HC_SHIFT + PC_PUBLISHED of them)
    if (!pinned_on_first_use(&plan_next->host_counts, 64)) return set_error(TFRA_ERR_OOM, "step_prefetch: hipHostMalloc");
    if (plan_next->last_used_step) {  // the write-back that read plan_next's buffers must be over
      const unsigned need = plan_next->last_used_step + 1;
      volatile unsigned* prog = t->progress_host;
      bool ok = false;
      for (int it = 0; it < 200000 && !ok; ++it) ok = (int)(*prog - need) >= 0;   // ~ a few ms at most
      if (!ok && hipStreamSynchronize(ms) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_prefetch: sync");
    }
  }
  if (plan_cur->n && rows_out) {
    rc = tfra_table_find(tp, plan_cur->n, ids_cur, rows_out, nullptr, find_default, 0, main_stream);
    if (rc) return rc;
  }
  if (plan_next) {
    if (!p) plan_next->skip_counts_once = !(t->opts.strategy == TFRA_EVICT_LFU && !scores);   // (the next step's call passes scores or not like this one)
    rc = tfra_sparse_plan_build(plan_next, n_next, ids_next, p ? t->opts.dim : 0, side_stream);
    if (rc) return rc;
    if (!plan_next->built_ev && hipEventCreateWithFlags(&plan_next->built_ev, hipEventDisableTiming) != hipSuccess) {
      plan_next->built_ev = nullptr;
      return set_error(TFRA_ERR_HIP, "step_prefetch: event");
    }
    if (hipEventRecord(plan_next->built_ev, ss) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_prefetch: event record");
    plan_next->ev_recorded = true;   // built on the side stream: the join below applies
  }
  if (plan_cur->ev_recorded) {  // built on the side stream by an earlier call
    // complete = every block of the build has ended and its stores are in memory (the pinned counts alone do not say that)
    if (hipEventQuery(plan_cur->built_ev) != hipSuccess && hipEventSynchronize(plan_cur->built_ev) != hipSuccess)   // the wait: rare
      return set_error(TFRA_ERR_HIP, "step_prefetch: join");
    plan_cur->ev_recorded = false;
  }
  plan_cur->last_used_step = step;
  if (plan_cur->n == 0) return TFRA_OK;   // no kernel publishes this step: a later slot check falls back to a sync
  std::lock_guard<std::mutex> lock(t->mu);
  if (p) return apply_planned_impl(tp, p, plan_cur, (const float*)grads_or_values, param_default_row, main_stream, t->progress_host, step);
  return upsert_planned_impl(tp, plan_cur, grads_or_values, scores, main_stream, t->progress_host, step);
}

extern "C" int tfra_table_step_prefetch(tfra_table_t* tp, const tfra_opt_params* p, tfra_sparse_plan_t* plan_cur,
                                        const int64_t* ids_cur, void* rows_out, const void* find_default,
                                        const float* grads, const float* param_default_row,
                                        tfra_sparse_plan_t* plan_next, const int64_t* ids_next, size_t n_next,
                                        tfra_stream_t main_stream, tfra_stream_t side_stream) {
  if (!p) return set_error(TFRA_ERR_INVALID, "step_prefetch: null optimizer parameters");
  return step_prefetch_impl(tp, p, plan_cur, ids_cur, rows_out, find_default, grads, param_default_row, nullptr, plan_next, ids_next,
                            n_next, main_stream, side_stream);
}

extern "C" int tfra_table_step_prefetch_assign(tfra_table_t* tp, tfra_sparse_plan_t* plan_cur, const int64_t* ids_cur,
                                               void* rows_out, const void* find_default, const void* values,
                                               const uint64_t* scores, tfra_sparse_plan_t* plan_next,
                                               const int64_t* ids_next, size_t n_next, tfra_stream_t main_stream,
                                               tfra_stream_t side_stream) {
  return step_prefetch_impl(tp, nullptr, plan_cur, ids_cur, rows_out, find_default, values, nullptr, scores, plan_next, ids_next,
                            n_next, main_stream, side_stream);
}

