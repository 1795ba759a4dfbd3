// The admitting lookups of the table: tfra_table_find_or_insert, and tfra_table_find_or_insert_planned, the
// same lookup over the distinct keys of a write-back plan (tfra_plan.h).  Phase 1 is insert_unique_kernel<G, U, true>
// (tfra_upsert_device.h; instantiated here and nowhere else) or the planned pair find_plan_keys_kernel / find_plan_bins_kernel
// (the latter, and GroupRow: tfra_find_insert_device.h, shared with tfra_tierplan.hip); phase 2 of a table at max_capacity is
// tfra_upsert.hip's (evict_phase, tfra_upsert.h).
#include <hip/hip_runtime.h>

#include "tfra_find_insert.h"
#include "tfra_find_insert_device.h"
#include "tfra_host.h"
#include "tfra_plan.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;

// find_or_insert: always the locked two-phase route, as insert_and_evict; the ownership pass does not serve it.
extern "C" int tfra_table_find_or_insert(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const void* init_values,
                                         int init_is_full, const uint64_t* scores, void* values_out, uint8_t* found,
                                         tfra_stream_t stream) {
  {   // (the grouped call, tfra_find_insert_many.hip, runs the same checks per descriptor)
    const Check c = check_find_or_insert(tp, n, keys, init_values);
    if (c.done()) return report("tfra_table_find_or_insert: ", c);
  }
  TABLE_ENTER();
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys when d_n is given)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const unsigned fb = t->field_bytes;
  const int g = granule_of(fb, init_values, values_out);
  const i64* k = (const i64*)keys;
  const unsigned char* init = (const unsigned char*)init_values;
  const u64* sc = (const u64*)scores;
  const int strat = t->opts.strategy;
  constexpr int U = 4;
  const size_t waves = (n + 4 * U - 1) / (4 * U);
  dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  const bool bounded = t->at_max_capacity();
  EvictScratch es;
  FindOut fo{(unsigned char*)values_out, found, nullptr, (const long long*)d_n, init_is_full != 0};
  const unsigned char* src2 = init;   // phase 2 reads row i of its source
  if (bounded) {
    rc = carve_evict_scratch(t, s, n, false, !init_is_full && !values_out ? fb : 0, &es);
    if (rc) return rc;
    fo.spill = es.spill;
    if (!init_is_full) src2 = fo.spill ? fo.spill : fo.vals;   // a deferred key's init row is in values_out[i] after phase 1
  }
  TableView v = t->view_of(t->cur);
  const int bd = bounded_mode(t, bounded);
  with_granule(g, [&](auto G) { insert_unique_kernel<G, U, true><<<grid, block, 0, s>>>(v, n, k, init, sc, 0, t->aux, strat, epoch, bd, es.deferred, fo); });
  if (bounded) evict_phase(t, s, v, g, n, k, src2, sc, 0, es.deferred);
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}

// ---- find_or_insert over a write-back plan: the keys are the CSR plan's distinct keys, every batch position of a
// key gets its row.  Key k's init row and score are those of its LAST batch position L(k), so the outcome does not depend on
// the order the plan holds its keys in.

// What the planned instance reads per batch position and where its rows go.
struct PlanFindIO {
  const unsigned char* init;  // [n, field_bytes] when full, else one row
  const u64* scores;          // null, or [n] per batch position
  unsigned char* rows;        // [n, field_bytes]
  uint8_t* found;             // [n]; may be null
  int full;
  unsigned n;                 // the plan's id count: rows of `rows`, upper bound of its keys
  // a table at max_capacity: phase 2 (insert_evict_kernel) reads entry g of dense per-KEY arrays
  uint8_t* deferred;          // [n] flags; null off max_capacity
  unsigned char* spill;       // [n, field_bytes]: a deferred key's init row
  u64* key_scores;            // [n]: its score; null when scores is
};

// Key launch: one 16-lane group per plan key (grid-stride, bounded by the count on the device).  Probe, score and the per-wave
// size / error accounting are insert_unique_kernel<G, U, true>'s; the row then goes to every position of a key with at most
// DIRECT occurrences, and to position L(k) of a key whose positions sit in the bins (find_plan_bins_kernel copies it on from there).
template <int G>
__global__ __launch_bounds__(256) void find_plan_keys_kernel(TableView v, CsrKeys ks, PlanFindIO io, AuxInit ai, int strategy, u64 epoch,
                                                             int bounded, int* __restrict__ prow_dest) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = min(ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD], io.n);
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
  const unsigned ngroups = nthreads >> 4;
  if (blockIdx.x == 0 && threadIdx.x == 0 && ks.d_counts[PC_OVERFLOW]) atomicAdd(v.err_count, ks.d_counts[PC_OVERFLOW]);  // plan overflow
  // phase 2 walks all n entries: the flags of the entries beyond the count say "not deferred"
  if (io.deferred)
    for (unsigned i = total + tid; i < io.n; i += nthreads) io.deferred[i] = 0;
  const unsigned fb = v.field_bytes;
  const bool pf1 = bounded > 1;  // table near capacity: both home buckets' lines in flight together
  int fresh = 0, failed = 0;
  for (unsigned g = tid >> 4; g < total; g += ngroups) {
    bool many;
    const unsigned w = load_record(ks, g, sub, many);
    const i64 key = (i64)(((u64)(unsigned)__shfl((int)w, gshift + 1) << 32) | (unsigned)__shfl((int)w, gshift));
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    const i64 k0 = load_key_coherent(key_line(v, b0) + sub);
    const i64 k1 = load_key_coherent(key_line(v, pf1 ? bucket1(h, b0, v.nb) : b0) + sub);  // (same line again: an L2 hit)
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    unsigned lastp = (unsigned)__shfl((int)w, gshift + (many ? 5 : 3));   // few: the last position itself; many: where it is stored
    if (many) lastp = ks.hent[lastp];
    lastp &= E_POS;
    if (lastp >= io.n) continue;   // (no record of a completed build says so)
    const unsigned char* init = io.init + (io.full ? (size_t)lastp * fb : 0);
    const u64 in_score = io.scores ? io.scores[lastp] : 1;
    bool is_new;
    const i64 row = locate_or_claim_from(v, key, h, b0, k0, sub, gshift, is_new, bounded, pf1 ? &k1 : nullptr);
    const bool hit = row >= 0 && !is_new;
    GroupRow<G> r;
    r.load(hit ? row_ptr(v, row) : init, fb, sub);
    if (io.deferred && sub == 0) io.deferred[g] = row == NEED_EVICT;
    if (!hit) {
      if (row >= 0) {
        r.store(row_ptr(v, row), fb, sub);
        if (v.n_fields > 1) init_aux_fields(v, ai, row, sub, 0);
      } else if (row == NEED_EVICT && io.spill) {
        r.store(io.spill + (size_t)g * fb, fb, sub);
        if (io.key_scores && sub == 0) io.key_scores[g] = in_score;
      }
    }
    if (row >= 0) {
      update_score(v, row, is_new, strategy, in_score, epoch, sub);
      fresh += (is_new && sub == 0);
    } else if (row != NEED_EVICT) {
      failed += (sub == 0);
    }
    if (many) {
      r.store(io.rows + (size_t)lastp * fb, fb, sub);
      if (io.found && sub == 0) io.found[lastp] = hit;
      const unsigned first = (unsigned)__shfl((int)w, gshift + 3), nsrc = (unsigned)__shfl((int)w, gshift + 4);
      for (unsigned t = sub; t < nsrc; t += 16) prow_dest[first + t] = (int)lastp;
    } else {
      for (unsigned e = 0; e < min(cnt, (unsigned)DIRECT); ++e) {
        const unsigned p = (unsigned)__shfl((int)w, gshift + 4 + (int)e);
        if (p >= io.n) continue;
        r.store(io.rows + (size_t)p * fb, fb, sub);
        if (io.found && sub == 0) io.found[p] = hit;
      }
    }
  }
  wave_account(v, tid >> 6, lane, fresh, failed);
}

extern "C" int tfra_table_find_or_insert_planned(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const void* init_values,
                                                 int init_is_full, const uint64_t* scores, void* rows_out, uint8_t* found,
                                                 tfra_stream_t stream) {
  const char* who = "tfra_table_find_or_insert_planned: ";
  if (!tp) return set_error(TFRA_ERR_INVALID, std::string(who) + "null table");
  if (!pl) return set_error(TFRA_ERR_INVALID, std::string(who) + "null plan");
  if (!init_values || !rows_out) return set_error(TFRA_ERR_INVALID, std::string(who) + "null buffer");
  if (pl->n == 0) return set_error(TFRA_ERR_INVALID, std::string(who) + "no built plan");
  if (pl->kind == 1)
    return set_error(TFRA_ERR_UNSUPPORTED, std::string(who) + "needs a plan built with the table's dim (an assign-only plan keeps no positions)");
  {
    const Table* tc = reinterpret_cast<const Table*>(tp);
    const int dt = tc->opts.value_dtype, dim = tc->opts.dim;
    if (pl->dim != dim) return set_error(TFRA_ERR_INVALID, std::string(who) + "the plan was built for another dim");
    if (tc->opts.device != pl->device && tc->opts.device >= 0)
      return set_error(TFRA_ERR_INVALID, std::string(who) + "plan and table live on different devices");
    if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
      return set_error(TFRA_ERR_UNSUPPORTED, std::string(who) + "value_dtype must be float32, float16 or bfloat16");
    if (dim % 4 != 0 || dim > 256 || (((uintptr_t)init_values | (uintptr_t)rows_out) & 15))
      return set_error(TFRA_ERR_UNSUPPORTED, std::string(who) + "needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers");
  }
  TABLE_ENTER();
  const size_t n = pl->n;
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const unsigned fb = t->field_bytes;
  const int g = granule_of(fb, init_values, rows_out) >= 16 ? 16 : 8;   // (dim % 4 == 0: rows of at least 8 bytes, at most 1024)
  const int strat = t->opts.strategy;
  const bool bounded = t->at_max_capacity();
  PlanFindIO io{(const unsigned char*)init_values, (const u64*)scores, (unsigned char*)rows_out, found, init_is_full != 0, (unsigned)n,
                nullptr, nullptr, nullptr};
  if (bounded) {
    EvictScratch es;
    rc = carve_evict_scratch(t, s, n, scores != nullptr, fb, &es);
    if (rc) return rc;
    io.deferred = es.deferred;
    io.key_scores = es.key_scores;
    io.spill = es.spill;
  }
  TableView v = t->view_of(t->cur);
  const int bd = bounded_mode(t, bounded);
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  const CsrKeys ks = keys_of(pl);
  auto launch = [&](auto G) {
    find_plan_keys_kernel<G><<<key_blocks, 256, 0, s>>>(v, ks, io, t->aux, strat, epoch, bd, pl->prow_dest);
    // (always launched: the host does not know the bin count; without bins it does nothing)
    find_plan_bins_kernel<G><<<bin_blocks, NTA, 0, s>>>(pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->prow_dest, io.rows, found, fb,
                                                        (unsigned)n);
  };
  if (g == 16) launch(std::integral_constant<int, 16>{});
  else launch(std::integral_constant<int, 8>{});
  // phase 2 over the plan's dense keys: flags, rows and scores by key index
  if (bounded) evict_phase(t, s, v, g, n, pl->dkeys, io.spill, io.key_scores, 0, io.deferred);
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}
