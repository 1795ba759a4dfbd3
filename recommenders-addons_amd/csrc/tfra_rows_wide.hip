// Whole rows out and back for WIDE rows: tfra_table_fetch_planned_wide and tfra_table_store_rows_wide, the two
// table calls of a dense update rule that has no fused write-back (optimizers.Generic with whole_rows=True) on a float32, float16
// or bfloat16 table with dim % 4 == 0 and 256 < dim <= 1024.  The twins (tfra_rows.hip) stop at dim 256 — a template cap of their
// 16-lanes-per-key kernels: such a variable trained through unique + segment_sum, 1 + S finds and 1 + S upserts.  Here one wave
// owns a row (the bodies: tfra_rows_wide_device.h); the plan is tfra_sparse_plan_build_wide's, the sums are the wide write-back's.
// Each call runs its twin's checks in its twin's order with its twin's codes, the width rule exchanged (tfra_apply.h), and
// enqueues in its twin's shape: the fetch a sums launch when gradients are given and ONE fetch launch, the store phase 1 and on a
// table at max_capacity the eviction phase's launch.
// Not provided in this form: half gradients and a scale (tfra_grads), more than 2^18 ids in a plan, tfra_reduce_by_key, tiers.
// Kernels instantiated here: rows_hot_sums_wide_kernel, fetch_rows_wide_kernel<ST, SUMS>, store_rows_wide_kernel<ST>,
// store_rows_wide_evict_kernel<ST>.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_apply.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_plan.h"
#include "tfra_rows_wide_device.h"
#include "tfra_upsert.h"

using namespace tfra;
using namespace tfra::red;

static_assert(sizeof(tfra_row_fields) == 48, "tfra_row_fields is 48 bytes (ABI)");

namespace {

// the sums in front of a fetch with gradients (hot_sums_wide_body): one block per bin, the grid strides over the plan's bins
__global__ __launch_bounds__(NTA) void rows_hot_sums_wide_kernel(const float* __restrict__ grads, int dim, const unsigned* __restrict__ hent,
                                                                 const unsigned* __restrict__ hout, const unsigned* __restrict__ binmap,
                                                                 const unsigned* __restrict__ d_counts, float* __restrict__ partial) {
  hot_sums_wide_body(grads, dim, hent, hout, binmap, d_counts, partial);
}

template <int ST, bool SUMS>
__global__ __launch_bounds__(256) void fetch_rows_wide_kernel(TableView v, int dim, const float* __restrict__ grads,
                                                              const float* __restrict__ partial, CsrKeys ks,
                                                              const unsigned char* __restrict__ default_row, AuxInit ai,
                                                              i64* __restrict__ keys_out, RowsOut ro, int first_want,
                                                              float* __restrict__ gsum_out, i64* __restrict__ d_count) {
  fetch_rows_wide_body<ST, SUMS>(v, dim, grads, partial, ks, default_row, ai, keys_out, ro, first_want, gsum_out, d_count);
}

template <int ST>
__global__ __launch_bounds__(256) void store_rows_wide_kernel(TableView v, size_t n_buf, const i64* __restrict__ keys, RowsIn ri, int dim,
                                                              AuxInit ai, int strategy, u64 epoch, int bounded,
                                                              uint8_t* __restrict__ deferred, const long long* __restrict__ d_n) {
  store_rows_wide_body<ST>(v, n_buf, keys, ri, dim, ai, strategy, epoch, bounded, deferred, d_n);
}

template <int ST>
__global__ __launch_bounds__(256) void store_rows_wide_evict_kernel(TableView v, size_t n, const i64* __restrict__ keys, RowsIn ri, int dim,
                                                                    AuxInit ai, int strategy, u64 epoch,
                                                                    const uint8_t* __restrict__ deferred) {
  store_rows_wide_evict_body<ST>(v, n, keys, ri, dim, ai, strategy, epoch, deferred);
}

constexpr unsigned MAX_BLOCKS = 2048;   // one resident grid (the kernels are grid-stride)

// ---- host: the twins' checks (check_fields / check_table of tfra_rows.hip), the width rule exchanged ----
Check check_fields(const tfra_row_fields* r, bool need_field0) {
  if (r->struct_size != sizeof(tfra_row_fields)) return refuse(TFRA_ERR_INVALID, "tfra_row_fields size mismatch (ABI)");
  if (r->n_fields < 1 || r->n_fields > MAXF) return refuse(TFRA_ERR_INVALID, "tfra_row_fields.n_fields must be 1 + the table's aux_fields (1..5)");
  for (int f = r->n_fields; f < MAXF; ++f)
    if (r->field[f]) return refuse(TFRA_ERR_INVALID, "tfra_row_fields.field entries at or beyond n_fields must be NULL");
  if (need_field0 && !r->field[0]) return refuse(TFRA_ERR_INVALID, "field[0] must not be NULL");
  for (int f = 0; f < r->n_fields; ++f)
    if ((uintptr_t)r->field[f] & 15) return refuse(TFRA_ERR_UNSUPPORTED, "every field must be 16-B aligned");
  return Check{};
}
Check check_table(const Table* t, const tfra_row_fields* r, const char* twin) {
  const int dt = t->opts.value_dtype;
  if (r->n_fields != 1 + t->opts.aux_fields) return refuse(TFRA_ERR_INVALID, "tfra_row_fields.n_fields must be 1 + the table's aux_fields");
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16");
  if (!wide_apply_dim(t->opts.dim)) return refuse_wide_dim(twin);
  return Check{};
}

}  // namespace

extern "C" int tfra_table_fetch_planned_wide(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const tfra_grads* g, const void* default_row,
                                             int64_t* keys_out, const tfra_row_fields* rows_out, float* gsum_out, int64_t* d_count,
                                             tfra_stream_t stream) {
  const std::string who = "tfra_table_fetch_planned_wide: ";
  if (!tp || !pl || !keys_out || !rows_out || !d_count || !default_row) return set_error(TFRA_ERR_INVALID, who + "null argument");
  if (const Check c = check_fields(rows_out, false); c.code) return report(who, c);
  if ((g != nullptr) != (gsum_out != nullptr)) return set_error(TFRA_ERR_INVALID, who + "gradients and gsum_out go together (both, or both NULL)");
  if (g) {
    bool forward = false;
    if (const Check c = check_typed(g, &forward); c.code) return report(who, c);
    if (!forward)
      return set_error(TFRA_ERR_UNSUPPORTED, who + "wide rows take float32 gradients without a scale (half gradients are up-cast by the caller)");
    if ((uintptr_t)g->grads & 15) return set_error(TFRA_ERR_UNSUPPORTED, who + "float32 gradients must be 16-B aligned");
    if ((uintptr_t)gsum_out & 15) return set_error(TFRA_ERR_UNSUPPORTED, who + "gsum_out must be 16-B aligned");
  }
  {
    const Table* tc = reinterpret_cast<const Table*>(tp);
    if (const Check c = check_table(tc, rows_out, "tfra_table_fetch_planned"); c.code) return report(who, c);
    if ((uintptr_t)default_row & (tc->opts.value_dtype == TFRA_F32 ? 15 : 7))
      return set_error(TFRA_ERR_UNSUPPORTED, who + "default_row must be 16-B aligned (a half row: 8-B)");
    if (pl->n == 0 && !pl->ever_built) return set_error(TFRA_ERR_INVALID, who + "no built plan");
    if (pl->n && pl->kind == 1)
      return set_error(TFRA_ERR_UNSUPPORTED, who + "needs a plan built with the table's dim (an assign-only plan keeps no positions)");
    if (pl->n && pl->dim != tc->opts.dim) return set_error(TFRA_ERR_INVALID, who + "the plan was built for another dim");
    if (tc->opts.device != pl->device && tc->opts.device >= 0) return set_error(TFRA_ERR_INVALID, who + "plan and table live on different devices");
    if (pl->n > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, who + "at most 2^18 ids per plan");
  }
  TABLE_ENTER();
  if (pl->n == 0) {
    if (hipMemsetAsync(d_count, 0, sizeof(int64_t), s) != hipSuccess) return set_error(TFRA_ERR_HIP, who + "memset");
    return TFRA_OK;
  }
  const int dim = t->opts.dim;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  // (key_blocks counts 16 lanes per key; a wave takes four keys per trip here as there, so the grid is the twin's)
  key_blocks = std::min(key_blocks, MAX_BLOCKS);
  RowsOut ro{};
  int first_want = -1;
  for (int f = 0; f < rows_out->n_fields; ++f) {
    ro.field[f] = rows_out->field[f];
    if (ro.field[f] && first_want < 0) first_want = f;
  }
  const TableView v = t->view_of(t->cur);
  const CsrKeys ks = keys_of(pl);
  const unsigned char* dr = (const unsigned char*)default_row;
  const float* grads = g ? (const float*)g->grads : nullptr;
  if (g) rows_hot_sums_wide_kernel<<<bin_blocks, NTA, 0, s>>>(grads, dim, pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->partial);
  with_stored(st_index(t->opts.value_dtype), [&](auto ST) {
    if (!g)
      fetch_rows_wide_kernel<ST, false><<<key_blocks, 256, 0, s>>>(v, dim, nullptr, pl->partial, ks, dr, t->aux, (i64*)keys_out, ro,
                                                                    first_want, nullptr, (i64*)d_count);
    else
      fetch_rows_wide_kernel<ST, true><<<key_blocks, 256, 0, s>>>(v, dim, grads, pl->partial, ks, dr, t->aux, (i64*)keys_out, ro,
                                                                   first_want, gsum_out, (i64*)d_count);
  });
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, who + "launch failed");
  return TFRA_OK;
}

extern "C" int tfra_table_store_rows_wide(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const tfra_row_fields* rows,
                                          tfra_stream_t stream) {
  const std::string who = "tfra_table_store_rows_wide: ";
  if (!tp) return set_error(TFRA_ERR_INVALID, who + "null table");
  if (n == 0) return TFRA_OK;
  if (int rc = check_batch(who.c_str(), n, keys && rows, [&] {
        if (const Check c = check_fields(rows, true); c.code) return report(who, c);
        if (const Check c = check_table(reinterpret_cast<const Table*>(tp), rows, "tfra_table_store_rows"); c.code) return report(who, c);
        return (int)TFRA_OK;
      }))
    return rc;
  TABLE_ENTER();
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys: a growing table may grow a call early)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const int strat = t->opts.strategy, dim = t->opts.dim;
  const size_t blocks = (n + 15) / 16;   // four keys per wave and trip, four waves per block
  const dim3 grid((unsigned)std::min<size_t>(blocks, MAX_BLOCKS)), block(256);
  const bool bounded = t->at_max_capacity();
  EvictScratch es;
  if (bounded) {
    rc = carve_evict_scratch(t, s, n, false, 0, &es);
    if (rc) return rc;
  }
  RowsIn ri{};
  for (int f = 0; f < rows->n_fields; ++f) ri.field[f] = rows->field[f];
  const TableView v = t->view_of(t->cur);
  const int bd = bounded_mode(t, bounded);
  with_stored(st_index(t->opts.value_dtype), [&](auto ST) {
    store_rows_wide_kernel<ST><<<grid, block, 0, s>>>(v, n, (const i64*)keys, ri, dim, t->aux, strat, epoch, bd, es.deferred, (const long long*)d_n);
    if (bounded)
      store_rows_wide_evict_kernel<ST><<<grid, block, 0, s>>>(v, n, (const i64*)keys, ri, dim, t->aux, strat, epoch, es.deferred);
  });
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}
