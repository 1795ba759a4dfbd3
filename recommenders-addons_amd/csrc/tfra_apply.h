// What the single-table write-backs (tfra_apply.hip) and the grouped one (tfra_apply_many.hip) share on the host, ONE copy each:
// the sums' launch ladder by row width (with_nch) and the argument checks of a planned and of a combined write-back
// (check_apply_planned, check_apply_combined), which the single call and every descriptor of the grouped call run.
// File-local in each unit (static), as keys_of of tfra_plan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_plan.h"

// NCH of the sums, the row's chunks of 64 floats: f(std::integral_constant<int, NCH>{}) for nch in 1..4
template <class F>
static void with_nch(int nch, F&& f) {
  switch (nch) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// A fused write-back of a table that rounds stochastically takes one call index of the random stream, on the host: a captured
// graph would replay that one index.  Every fused write-back refuses the pair before it enqueues anything.
static Check check_rounding(const Table* t) {
  if (t->stochastic() && t->capture_safe)
    return refuse(TFRA_ERR_UNSUPPORTED, "TFRA_OPTION_STOCHASTIC_ROUNDING and TFRA_OPTION_CAPTURE_SAFE are both set (a replayed graph would reuse one call index)");
  return Check{};
}

// (What a tfra_grads itself must satisfy, check_typed, stands in tfra_many.h beside Check: the typed weight gradients use it too.)

// The checks of a planned write-back: apply_planned_impl's, whoever calls it, and behind check_apply_combined those of a
// descriptor of tfra_multi_apply_planned_combined.  active: the plan holds ids.  grad_mask: 15 for a float gradient matrix, 7 for
// the float16 / bfloat16 one of the *_typed calls.
template <class AtEntry>
static Check check_apply_planned(const Table* t, const tfra_opt_params* p, const tfra_sparse_plan* pl, const void* grads,
                                 const float* param_default_row, AtEntry&& at_entry, unsigned grad_mask = 15u) {
  if (!t || !p || !pl) return refuse(TFRA_ERR_INVALID, "null argument");
  if (Check e = check_rounding(t); e.done()) return e;
  if (Check e = at_entry(); e.done()) return e;
  if (pl->n == 0) return nothing_to_do();
  if (!grads || !param_default_row) return refuse(TFRA_ERR_INVALID, "null buffer");
  const int dt = t->opts.value_dtype;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16 (the default row is float32)");
  if (p->kind < 0 || p->kind > TFRA_OPT_RMSPROP) return refuse(TFRA_ERR_INVALID, "unknown kind");
  const int need = opt_slots(p->kind);
  if (t->opts.aux_fields < need) return refuse(TFRA_ERR_INVALID, "table lacks optimizer slot fields");
  if (t->opts.dim != pl->dim) return refuse(TFRA_ERR_INVALID, "the plan was built for another dim");
  if (t->opts.device != pl->device && t->opts.device >= 0) return refuse(TFRA_ERR_INVALID, "plan and table live on different devices");
  if (((uintptr_t)grads & grad_mask) || ((uintptr_t)param_default_row & 15))
    return refuse(TFRA_ERR_UNSUPPORTED, grad_mask == 15u ? "gradient / default buffers must be 16-B aligned"
                                                         : "half gradients must be 8-B aligned, the default row 16-B");
  return Check{};
}

// The checks tfra_table_apply_planned_combined makes before it forms the entry records (apply_planned_impl's follow behind them),
// also the first half of a descriptor's.  active: the plan holds ids.  grad_mask: 15 for a float grad_out, 7 for the float16 /
// bfloat16 one of the *_combined_typed calls, whose kernels address grad_out with 32-bit element offsets: n_rows * dim < 2^32 then.
template <class AtEntry>
static Check check_apply_combined(const Table* t, const tfra_opt_params* p, const tfra_sparse_plan* pl, const void* grad_out,
                                  const int64_t* seg, const float* weights, int combiner, size_t n_rows, const float* param_default_row,
                                  AtEntry&& at_entry, unsigned grad_mask = 15u) {
  if (!t || !p || !pl) return refuse(TFRA_ERR_INVALID, "null argument");
  if (combiner < 0 || combiner > 2) return refuse(TFRA_ERR_INVALID, "combiner must be 0 (sum), 1 (mean) or 2 (sqrtn)");
  if (Check e = check_rounding(t); e.done()) return e;
  if (Check e = at_entry(); e.done()) return e;
  if (pl->kind != 0 || pl->dim != t->opts.dim) return refuse(TFRA_ERR_INVALID, "the plan was built for another dim");
  if (t->opts.device != pl->device && t->opts.device >= 0) return refuse(TFRA_ERR_INVALID, "plan and table live on different devices");
  if (pl->n == 0) return nothing_to_do();
  if (!grad_out || !seg || !param_default_row) return refuse(TFRA_ERR_INVALID, "null buffer");
  if (n_rows == 0 || n_rows >= (1ULL << 30)) return refuse(TFRA_ERR_INVALID, "need 1 <= n_rows < 2^30");
  if (grad_mask != 15u && (unsigned long long)n_rows * (unsigned long long)t->opts.dim >= (1ULL << 32))
    return refuse(TFRA_ERR_UNSUPPORTED, "half grad_out is addressed with 32-bit element offsets: need n_rows * dim < 2^32");
  if (((uintptr_t)grad_out & grad_mask) || ((uintptr_t)param_default_row & 15) || ((uintptr_t)seg & 7) || ((uintptr_t)weights & 3))
    return refuse(TFRA_ERR_UNSUPPORTED, grad_mask == 15u ? "grad_out / default buffers must be 16-B aligned"
                                                         : "half grad_out must be 8-B aligned, the default row 16-B");
  return Check{};
}
