// The planned sparse write-back for WIDE rows: tfra_table_apply_planned_wide, tfra_table_apply_planned_combined_wide
// and tfra_table_apply_sparse_wide, for float32, float16 and bfloat16 tables with dim % 4 == 0 and 256 < dim <= 1024 and float32
// gradients.  (Their plan build, tfra_sparse_plan_build_wide, stands beside its twin in tfra_csr.hip: one host part, the width rule a
// parameter.)  The twins (tfra_apply.hip) stop at dim 256 — a template cap of their 16-lanes-per-key kernels, nothing in the plan:
// a wide variable trained through unique + segment_sum + apply_optimizer, and its embedding_lookup_sparse through an expanded
// [nnz, dim] gradient besides.  Here one wave owns a row (the bodies and why the bits are the twins': tfra_apply_wide_device.h).
// Each call runs its twin's checks (tfra_apply.h) in its twin's order with the width rule exchanged, and enqueues in its twin's
// shape: sums launch, update launch, and on a bounded table the eviction phase's launch.
// Not provided in this form: half gradients and a scale (tfra_grads), stochastic rounding, more than 2^18 ids, the reduce / fetch /
// store calls of a plan, the grouped *_many forms, the step drivers, tiers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_apply.h"
#include "tfra_apply_wide_device.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_plan.h"

using namespace tfra;
using namespace tfra::red;

namespace {

// the sums (hot_sums_wide_body): one block per bin, the grid strides over the plan's bins
template <class... CS>
__global__ __launch_bounds__(NTA) void hot_sums_wide_kernel(const float* __restrict__ grads, int dim, const unsigned* __restrict__ hent,
                                                            const unsigned* __restrict__ hout, const unsigned* __restrict__ binmap,
                                                            const unsigned* __restrict__ d_counts, float* __restrict__ partial,
                                                            const CS... cs) {
  hot_sums_wide_body(grads, dim, hent, hout, binmap, d_counts, partial, cs...);
}

// the update (apply_csr_wide_body): one wave per key, four keys per wave and trip; PHASE2: the eviction phase of a table at max_capacity
template <int KIND, bool PHASE2, int ST, class... CS>
__global__ __launch_bounds__(256) void apply_csr_wide_kernel(TableView v, OptP o, int dim, const float* __restrict__ grads,
                                                             const float* __restrict__ partial, CsrKeys ks,
                                                             const float* __restrict__ default_row, float aux0, float aux1, ScoreP sp,
                                                             uint8_t* __restrict__ dflag, unsigned* any_deferred, unsigned use_gen,
                                                             const CS... cs) {
  apply_csr_wide_body<KIND, PHASE2, ST>(v, o, dim, grads, partial, ks, default_row, aux0, aux1, sp, dflag, any_deferred, use_gen, cs...);
}

// by the rule and by the rows' storage type (both checked by the caller)
template <class... CS>
void launch_apply_wide(Table* t, hipStream_t s, const tfra_sparse_plan* pl, int kind, const OptP& o, const float* grads,
                       const float* default_row, unsigned key_blocks, const ScoreP& sp, const CS&... cs) {
  const TableView v = t->view_of(t->cur);
  const float a0 = t->opts.aux_init[0], a1 = t->opts.aux_init[1];
  const unsigned gen = ++pl->use_gen;
  key_blocks = std::min(key_blocks, 1024u);   // one resident grid, as the twin's (the kernel is grid-stride)
  with_opt_kind(kind, [&](auto KIND) {
    with_stored(st_index(t->opts.value_dtype), [&](auto ST) {
      apply_csr_wide_kernel<KIND, false, ST><<<key_blocks, 256, 0, s>>>(v, o, pl->dim, grads, pl->partial, keys_of(pl), default_row, a0, a1,
                                                                        sp, pl->dflag, pl->any_deferred, gen, cs...);
      if (sp.bounded)
        apply_csr_wide_kernel<KIND, true, ST><<<key_blocks, 256, 0, s>>>(v, o, pl->dim, grads, pl->partial, keys_of(pl), default_row, a0,
                                                                         a1, sp, pl->dflag, pl->any_deferred, gen, cs...);
    });
  });
}

// apply_planned_impl (tfra_apply.hip) for a wide table; comb != nullptr: grads is grad_out, position e's gradient is formed from
// comb[e].  The caller holds t->mu.
int apply_planned_wide_impl(const char* who, const char* twin, Table* t, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                            const float* grads, const float* param_default_row, hipStream_t s, const CombEnt* comb) {
  const Check c = check_apply_planned(t, p, pl, grads, param_default_row, [&] { return Check{t->enter(s)}; }, 15u, twin);
  if (c.code) return report(who, c);
  if (!c.active) return TFRA_OK;
  int rc = t->prepare_insert(pl->n, s);
  if (rc) return rc;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  // (key_blocks counts 16 lanes per key; a wave takes four keys per trip here as there, so the grid is the twin's)
  const int dim = pl->dim;
  if (comb) hot_sums_wide_kernel<<<bin_blocks, NTA, 0, s>>>(grads, dim, pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->partial, CombRows{comb});
  else hot_sums_wide_kernel<<<bin_blocks, NTA, 0, s>>>(grads, dim, pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->partial);
  uint8_t* bounded_now;
  rc = t->bounded_flags(1, s, &bounded_now);
  if (rc) return rc;
  const ScoreP sp = score_of(t, bounded_now);
  const OptP o = opt_of(p);
  if (comb) launch_apply_wide(t, s, pl, p->kind, o, grads, param_default_row, key_blocks, sp, CombRows{comb});
  else launch_apply_wide(t, s, pl, p->kind, o, grads, param_default_row, key_blocks, sp);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, std::string(who) + "launch failed");
  t->step_writeback();
  return TFRA_OK;
}

}  // namespace

extern "C" int tfra_table_apply_planned_wide(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl, const float* grads,
                                             const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "apply_planned_wide: null table");
  std::lock_guard<std::mutex> lock(t->mu);
  return apply_planned_wide_impl("apply_planned_wide: ", "tfra_table_apply_planned", t, p, pl, grads, param_default_row, (hipStream_t)stream,
                                 nullptr);
}

// The write-back of an embedding_lookup_sparse over a wide table: the entry records as the twin forms them (comb_entries), then the
// wide kernels reading grad_out through them — the expanded [nnz, dim] gradient is never formed.
extern "C" int tfra_table_apply_planned_combined_wide(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                                      const float* grad_out, const int64_t* seg, const float* weights, int combiner,
                                                      size_t n_rows, const float* param_default_row, tfra_stream_t stream) {
  const char* who = "apply_planned_combined_wide: ";
  const char* twin = "tfra_table_apply_planned_combined";
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  const Check c = check_apply_combined(t, p, pl, grad_out, seg, weights, combiner, n_rows, param_default_row, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};   // the scratch below was last used on the table's previous stream
  }, 15u, twin);
  if (c.code) return report(who, c);
  if (!c.active) return TFRA_OK;
  const size_t nnz = pl->n;
  tfra_workspace_t* ws;
  int rc = workspace_in(&t->comb_ws, t->device, &ws);
  if (rc) return rc;
  auto al = [](size_t x) { return (x + 255) / 256 * 256; };
  const size_t se_b = al(2 * n_rows * sizeof(int)), den_b = al(n_rows * sizeof(float));
  rc = ws->ensure(se_b + den_b + al(nnz * sizeof(CombEnt)), s);
  if (rc) return rc;
  unsigned char* b = (unsigned char*)ws->buf;
  CombEnt* ent = reinterpret_cast<CombEnt*>(b + se_b + den_b);
  rc = comb_entries(s, nnz, seg, weights, combiner, n_rows, reinterpret_cast<int*>(b), reinterpret_cast<float*>(b + se_b), ent);
  if (rc) return rc;
  return apply_planned_wide_impl(who, twin, t, p, pl, grad_out, param_default_row, s, ent);
}

// plan build into the table's own plan + the planned write-back, as tfra_table_apply_sparse; at most 2^18 ids (no chunked path)
extern "C" int tfra_table_apply_sparse_wide(tfra_table_t* tp, const tfra_opt_params* p, size_t n, const int64_t* ids, const float* grads,
                                            const float* param_default_row, tfra_stream_t stream) {
  const char* twin = "tfra_table_apply_sparse";
  Table* t = reinterpret_cast<Table*>(tp);
  const std::string pre = "apply_sparse_wide: ";
  if (!t || !p) return set_error(TFRA_ERR_INVALID, pre + "null argument");
  if (n == 0) return TFRA_OK;
  if (!ids || !grads || !param_default_row) return set_error(TFRA_ERR_INVALID, pre + "null buffer");
  const int dt = t->opts.value_dtype;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return set_error(TFRA_ERR_UNSUPPORTED, pre + "value_dtype must be float32, float16 or bfloat16 (the default row is float32)");
  const int dim = t->opts.dim;
  if (!wide_apply_dim(dim)) return report(pre, refuse_wide_dim(twin));
  if (((uintptr_t)grads & 15) || ((uintptr_t)param_default_row & 15))
    return set_error(TFRA_ERR_UNSUPPORTED, pre + "gradient / default buffers must be 16-B aligned");
  if (n > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, pre + "at most 2^18 ids per call");
  tfra_sparse_plan* pl;
  std::lock_guard<std::mutex> lock(t->mu);
  if (const Check c = check_rounding(t, true); c.code) return report(pre, c);   // (before the plan build is enqueued)
  int rc = t->enter((hipStream_t)stream);   // orders the rebuild of the table's own plan behind its previous use
  if (rc) return rc;
  rc = own_plan(t, &pl);
  if (rc) return rc;
  rc = tfra_sparse_plan_build_wide(pl, n, ids, dim, stream);
  if (rc) return rc;
  return apply_planned_wide_impl(pre.c_str(), twin, t, p, pl, grads, param_default_row, (hipStream_t)stream, nullptr);
}
