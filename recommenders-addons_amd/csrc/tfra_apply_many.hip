// tfra_multi_apply_planned_combined: the combined write-back (tfra_table_apply_planned_combined, tfra_apply.hip) for a LIST of tables,
// with launches that do not grow with the list.  Its two kernels call the bodies the single call's kernels call, and read what
// those take as arguments from a record (ApplyManyRec: tfra_apply_device.h); a descriptor's checks are the single call's
// (tfra_apply.h).  The host side stands on the grouped-call frame of tfra_many.h: check, classify, lock, lay out, fill, send, launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_apply.h"
#include "tfra_apply_device.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_optim_device.h"
#include "tfra_plan.h"
#include "tfra_reduce_device.h"

using namespace tfra;
using namespace tfra::red;

namespace {

// the sums of one NCH class: block -> descriptor -> record (scalar loads), then the single call's body
template <int NCH>
__global__ __launch_bounds__(NTA) void hot_sums_many_kernel(const ApplyManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                            const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const unsigned first = prefix[d], nblk = prefix[d + 1] - first;
  const ApplyManyRec rec = recs[idx[d]];
  hot_sums_body<NCH>(rec.grads, rec.dim, rec.ks.hent, rec.hout, rec.binmap, rec.ks.d_counts, rec.partial, nullptr, 0u, blockIdx.x - first,
                     nblk, CombRows{rec.ent});
}

// PHASE2: the class's grid again; the blocks of a table that can still grow have nothing to do (the single call does not launch it)
template <int KIND, bool PHASE2, int ST>
__global__ __launch_bounds__(256) void apply_csr_many_kernel(const ApplyManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                             const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const unsigned first = prefix[d], nblk = prefix[d + 1] - first;
  const ApplyManyRec rec = recs[idx[d]];
  if (PHASE2 && !rec.sp.bounded) return;
  apply_csr_body<KIND, PHASE2, ST>(rec.v, rec.o, rec.dim, rec.grads, rec.partial, rec.ks, rec.default_row, rec.aux0, rec.aux1, rec.sp,
                                   rec.dflag, rec.any_deferred, rec.use_gen, blockIdx.x - first, nblk, CombRows{rec.ent});
}

// The half classes of tfra_multi_apply_planned_combined_typed: the same two kernels over descriptors whose grad_out is float16 /
// bfloat16 — rec.grads is the half matrix's address, hrecs[i] the scale's address and the format (wave-uniform, as GradHalf wants it).
template <int NCH>
__global__ __launch_bounds__(NTA) void hot_sums_many_half_kernel(const ApplyManyRec* __restrict__ recs, const GradHalfRec* __restrict__ hrecs,
                                                                 const unsigned* __restrict__ prefix, const unsigned* __restrict__ idx,
                                                                 unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const unsigned first = prefix[d], nblk = prefix[d + 1] - first;
  const ApplyManyRec rec = recs[idx[d]];
  const GradHalfRec h = hrecs[idx[d]];
  hot_sums_body<NCH>(nullptr, rec.dim, rec.ks.hent, rec.hout, rec.binmap, rec.ks.d_counts, rec.partial, nullptr, 0u, blockIdx.x - first,
                     nblk, CombRows{rec.ent}, GradHalf{rec.grads, h.d_scale, h.is_bf16});
}

template <int KIND, bool PHASE2, int ST>
__global__ __launch_bounds__(256) void apply_csr_many_half_kernel(const ApplyManyRec* __restrict__ recs, const GradHalfRec* __restrict__ hrecs,
                                                                  const unsigned* __restrict__ prefix, const unsigned* __restrict__ idx,
                                                                  unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const unsigned first = prefix[d], nblk = prefix[d + 1] - first;
  const ApplyManyRec rec = recs[idx[d]];
  const GradHalfRec h = hrecs[idx[d]];
  if (PHASE2 && !rec.sp.bounded) return;
  apply_csr_body<KIND, PHASE2, ST>(rec.v, rec.o, rec.dim, nullptr, rec.partial, rec.ks, rec.default_row, rec.aux0, rec.aux1, rec.sp,
                                   rec.dflag, rec.any_deferred, rec.use_gen, blockIdx.x - first, nblk, CombRows{rec.ent},
                                   GradHalf{rec.grads, h.d_scale, h.is_bf16});
}

constexpr unsigned MANY_GRID_CAP = 1024;   // blocks of one grouped launch (see many_cap)

// Blocks a descriptor may own in a class of n_in_class descriptors.  The single call caps the update's grid at 1024 blocks — one
// resident round of the 125-register kernel, 4 blocks per CU x 256 CUs — and the plans' host-side grids are upper bounds (2048
// key blocks, up to 1024 bin blocks for a batch whose counts the host has not seen), mostly idle for a small batch.  The cap is
// shared: 1024 / n blocks each, so that a class of 26 descriptors is ~1014 blocks, not 26 x 1024.  A class of one descriptor has
// the single call's grid.  Both kernels stride by the descriptor's own block count, so results do not depend on it.
unsigned many_cap(unsigned blocks, unsigned n_in_class) {
  return std::max(1u, std::min(blocks, MANY_GRID_CAP / std::max(1u, n_in_class)));
}

// hrecs != nullptr: a half class
void launch_apply_many(hipStream_t s, int st, int kind, bool phase2, unsigned grid, const ApplyManyRec* recs, const GradHalfRec* hrecs,
                       const unsigned* prefix, const unsigned* idx, unsigned n) {
  with_opt_kind(kind, [&](auto KIND) {
    with_stored(st, [&](auto ST) {
      if (hrecs) {
        if (phase2) apply_csr_many_half_kernel<KIND, true, ST><<<grid, 256, 0, s>>>(recs, hrecs, prefix, idx, n);
        else apply_csr_many_half_kernel<KIND, false, ST><<<grid, 256, 0, s>>>(recs, hrecs, prefix, idx, n);
      } else if (phase2) apply_csr_many_kernel<KIND, true, ST><<<grid, 256, 0, s>>>(recs, prefix, idx, n);
      else apply_csr_many_kernel<KIND, false, ST><<<grid, 256, 0, s>>>(recs, prefix, idx, n);
    });
  });
}

void launch_hot_sums_many(hipStream_t s, int nch, unsigned grid, const ApplyManyRec* recs, const GradHalfRec* hrecs, const unsigned* prefix,
                          const unsigned* idx, unsigned n) {
  with_nch(nch, [&](auto NCH) {
    if (hrecs) hot_sums_many_half_kernel<NCH><<<grid, NTA, 0, s>>>(recs, hrecs, prefix, idx, n);
    else hot_sums_many_kernel<NCH><<<grid, NTA, 0, s>>>(recs, prefix, idx, n);
  });
}

// What the two descriptor types differ in: where grad_out stands, and (typed) its format and scale.
const void* grad_ptr(const tfra_apply_combined_desc& d) { return d.grad_out; }
const void* grad_ptr(const tfra_apply_combined_typed_desc& d) { return d.grad_out.grads; }
const tfra_grads* half_grads(const tfra_apply_combined_desc&) { return nullptr; }
const tfra_grads* half_grads(const tfra_apply_combined_typed_desc& d) { return d.grad_out.dtype == TFRA_F32 ? nullptr : &d.grad_out; }
Check check_grads(const tfra_apply_combined_desc&) { return Check{}; }
Check check_grads(const tfra_apply_combined_typed_desc& d) { bool forward; return check_typed(&d.grad_out, &forward); }
int single_call(const tfra_apply_combined_desc& d, tfra_stream_t stream) {
  return tfra_table_apply_planned_combined(d.table, d.opt, d.plan, d.grad_out, d.seg, d.weights, d.combiner, d.n_rows, d.param_default_row,
                                           stream);
}
int single_call(const tfra_apply_combined_typed_desc& d, tfra_stream_t stream) {
  return tfra_table_apply_planned_combined_typed(d.table, d.opt, d.plan, &d.grad_out, d.seg, d.weights, d.combiner, d.n_rows,
                                                 d.param_default_row, stream);
}

// A descriptor's checks: the single call's (check_apply_combined, then check_apply_planned), with what only a descriptor can get
// wrong where the single call enters its table.  A plan that holds no ids is skipped there: it was built for no dim
// (tfra_sparse_plan_build), and the single call is not made with one.
template <class Desc>
Check check_apply_desc(const Desc& d, const tfra_workspace* ws) {
  if (d.struct_size != sizeof(Desc)) return refuse(TFRA_ERR_INVALID, "descriptor size mismatch");
  if (Check g = check_grads(d); g.done()) return g;   // (typed: what a tfra_grads itself must satisfy)
  const unsigned grad_mask = half_grads(d) ? 7u : 15u;
  const Table* t = reinterpret_cast<const Table*>(d.table);
  Check c = check_apply_combined(t, d.opt, d.plan, grad_ptr(d), d.seg, d.weights, d.combiner, d.n_rows, d.param_default_row, [&] {
    if (ws->device != t->device) return refuse(TFRA_ERR_INVALID, "workspace and table live on different devices");
    return d.plan->n == 0 ? nothing_to_do() : Check{};
  }, grad_mask);
  if (c.done()) return c;
  c = check_apply_planned(t, d.opt, d.plan, grad_ptr(d), d.param_default_row, [] { return Check{}; }, grad_mask);
  if (c.done()) return c;
  const int dim = t->opts.dim;   // (hot_sums' classes: NCH 1..4)
  if (dim <= 0 || dim % 4 != 0 || dim > 64 * MAXCH) return refuse(TFRA_ERR_UNSUPPORTED, "needs dim % 4 == 0 and dim <= 256");
  return Check{};
}

// A descriptor's slices of the call's three front buffers, in elements: the rows' bounds (int), their denominators (float), the
// entry records (CombEnt).  What sizes the buffers also walks them.
struct Slices { size_t se, den, ent; };
template <class Desc>
Slices slices_of(const Desc& d) {
  return Slices{(2 * d.n_rows + 63) / 64 * 64, (d.n_rows + 63) / 64 * 64, (d.plan->n + 15) / 16 * 16};
}

template <class Desc>
int apply_grouped(const std::string& fn, tfra_workspace_t* ws, const Desc* descs, const std::vector<size_t>& act, uint32_t* launches_out,
                  hipStream_t s);

// tfra_multi_apply_planned_combined (Desc = tfra_apply_combined_desc) and its typed twin (tfra_apply_combined_typed_desc): one frame
template <class Desc>
int multi_apply_impl(const std::string& fn, tfra_workspace_t* ws, size_t n_tables, const Desc* descs, uint32_t* launches_out,
                     tfra_stream_t stream) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, fn + ": null argument");
  hipStream_t s = (hipStream_t)stream;
  const std::string who = fn + ": descriptor ";
  // every descriptor is checked before anything is enqueued and before any table is touched
  std::vector<size_t> act;   // the descriptors with work, in input order: record k belongs to descs[act[k]]
  for (size_t i = 0; i < n_tables; ++i) {
    const Check c = check_apply_desc(descs[i], ws);
    if (c.code) return report(who + std::to_string(i) + ": ", c);
    if (c.active) act.push_back(i);
  }
  // two descriptors on one table would be two writers of one key inside one launch; a plan's partial sums and flags are one use's
  for (size_t i = 0; i < n_tables; ++i)
    for (size_t j = i + 1; j < n_tables; ++j) {
      if (descs[i].table == descs[j].table)
        return set_error(TFRA_ERR_INVALID, who + std::to_string(i) + " and descriptor " + std::to_string(j) + " name the same table");
      if (descs[i].plan == descs[j].plan)
        return set_error(TFRA_ERR_INVALID, who + std::to_string(i) + " and descriptor " + std::to_string(j) + " name the same plan");
    }
  // members whose table rounds stochastically (TFRA_OPTION_STOCHASTIC_ROUNDING): the grouped kernels have no rounding axis, so the
  // single call's launches serve them, on the same stream, behind the grouped ones (whose table locks are released by then)
  std::vector<size_t> grouped, single;
  for (size_t i : act) (reinterpret_cast<const Table*>(descs[i].table)->stochastic() ? single : grouped).push_back(i);
  if (!grouped.empty()) {
    const int rc = apply_grouped(fn, ws, descs, grouped, launches_out, s);
    if (rc) return rc;
  }
  for (size_t i : single) {
    const int rc = single_call(descs[i], stream);
    if (rc) return rc;
  }
  return TFRA_OK;
}

}  // namespace

extern "C" int tfra_multi_apply_planned_combined(tfra_workspace_t* ws, size_t n_tables, const tfra_apply_combined_desc* descs,
                                                 uint32_t* launches_out, tfra_stream_t stream) {
  return multi_apply_impl("multi_apply_planned_combined", ws, n_tables, descs, launches_out, stream);
}

extern "C" int tfra_multi_apply_planned_combined_typed(tfra_workspace_t* ws, size_t n_tables, const tfra_apply_combined_typed_desc* descs,
                                                       uint32_t* launches_out, tfra_stream_t stream) {
  return multi_apply_impl("multi_apply_planned_combined_typed", ws, n_tables, descs, launches_out, stream);
}

namespace {

// the grouped launches over act, the checked descriptors with work whose tables round to nearest even
template <class Desc>
int apply_grouped(const std::string& fn, tfra_workspace_t* ws, const Desc* descs, const std::vector<size_t>& act, uint32_t* launches_out,
                  hipStream_t s) {
  const size_t n_act = act.size();

  // classes: the sums by (NCH 1..4, float or half grad_out), the update by (rule, storage type, float or half grad_out); the half
  // classes stand behind the float ones, and the untyped call has none: its class counts are what they were
  constexpr bool TYPED = std::is_same<Desc, tfra_apply_combined_typed_desc>::value;
  constexpr int NHOT1 = 4, NAPP1 = (TFRA_OPT_RMSPROP + 1) * 3;   // (check_apply_planned has refused every other kind)
  constexpr int NHOT = (TYPED ? 2 : 1) * NHOT1, NAPP = (TYPED ? 2 : 1) * NAPP1;
  auto ent_blocks_of = [&](size_t k) { return (unsigned)((descs[act[k]].plan->n + 255) / 256); };
  auto den_blocks_of = [&](size_t k) { return (unsigned)((descs[act[k]].n_rows + 255) / 256); };
  std::vector<int> hot_of(n_act), app_of(n_act);
  unsigned hot_n[NHOT] = {}, app_n[NAPP] = {};
  u64 ent_blocks = 0, den_blocks = 0;
  size_t se_ints = 0, den_floats = 0, ent_recs = 0;
  for (size_t k = 0; k < n_act; ++k) {
    const Desc& d = descs[act[k]];
    const Table* t = reinterpret_cast<const Table*>(d.table);
    const bool half = half_grads(d) != nullptr;
    hot_of[k] = (t->opts.dim + 63) / 64 - 1 + (half ? NHOT1 : 0);
    app_of[k] = d.opt->kind * 3 + st_index(t->opts.value_dtype) + (half ? NAPP1 : 0);
    ++hot_n[hot_of[k]];
    ++app_n[app_of[k]];
    ent_blocks += ent_blocks_of(k);
    den_blocks += den_blocks_of(k);
    const Slices sl = slices_of(d);
    se_ints += sl.se;
    den_floats += sl.den;
    ent_recs += sl.ent;
  }
  if (ent_blocks >= (1ULL << 31) || den_blocks >= (1ULL << 31))
    return set_error(TFRA_ERR_UNSUPPORTED, fn + ": too many rows in one call");

  std::vector<Table*> tabs;
  tabs.reserve(n_act);
  for (size_t i : act) tabs.push_back(reinterpret_cast<Table*>(descs[i].table));
  std::vector<std::unique_lock<std::mutex>> locks;
  int rc = lock_and_enter(std::move(tabs), s, &locks);
  if (rc) return rc;
  // capacity, as the single call prepares it: a table may grow here, so the views are taken afterwards
  std::vector<ScoreP> score(n_act);
  bool app_evict[NAPP] = {};   // a table at max_capacity in the class: the class runs its eviction phase
  for (size_t k = 0; k < n_act; ++k) {
    Table* t = reinterpret_cast<Table*>(descs[act[k]].table);
    rc = t->prepare_insert(descs[act[k]].plan->n, s);
    if (rc) return rc;
    uint8_t* bounded_now = nullptr;
    rc = t->bounded_flags(1, s, &bounded_now);
    if (rc) return rc;
    score[k] = score_of(t, bounded_now);
    app_evict[app_of[k]] = app_evict[app_of[k]] || score[k].bounded != 0;
  }

  // device memory: [bounds of all rows | denominators | entry records | blob], the blob = [update records | bounds records |
  // entry-kernel records | unsigned pool: entry prefix, row prefix, then per class present its prefix and its record indices]
  const size_t se_bytes = se_ints * sizeof(int), den_bytes = den_floats * sizeof(float), ent_bytes = ent_recs * sizeof(CombEnt);
  Blob blob;
  const size_t arec_off = blob.add<ApplyManyRec>(n_act), brec_off = blob.add<BoundsRec>(n_act), crec_off = blob.add<CombManyRec>(n_act);
  const size_t hrec_off = TYPED ? blob.add<GradHalfRec>(n_act) : 0;
  const size_t pool_off = blob.add<unsigned>(2 * ClassPool::words(n_act, 1, false) + ClassPool::words(n_act, NHOT, true) +
                                             ClassPool::words(n_act, NAPP, true));
  ManyUpload up;
  rc = many_begin(ws, se_bytes + den_bytes + ent_bytes, blob.bytes(), s, &up);
  if (rc) return rc;
  unsigned char* base = (unsigned char*)ws->buf;
  int* se_base = reinterpret_cast<int*>(base);
  float* den_base = reinterpret_cast<float*>(base + se_bytes);
  CombEnt* ent_base = reinterpret_cast<CombEnt*>(base + se_bytes + den_bytes);
  ApplyManyRec* arecs = section<ApplyManyRec>(up.host, arec_off);
  BoundsRec* brecs = section<BoundsRec>(up.host, brec_off);
  CombManyRec* crecs = section<CombManyRec>(up.host, crec_off);
  GradHalfRec* hrecs = TYPED ? section<GradHalfRec>(up.host, hrec_off) : nullptr;

  std::vector<unsigned> key_blocks(n_act), bin_blocks(n_act);
  {
    size_t se_at = 0, den_at = 0, ent_at = 0;
    for (size_t k = 0; k < n_act; ++k) {
      const Desc& d = descs[act[k]];
      Table* t = reinterpret_cast<Table*>(d.table);
      const tfra_sparse_plan* pl = d.plan;
      if (const tfra_grads* hg = half_grads(d)) hrecs[k] = GradHalfRec{hg->d_scale, hg->dtype == TFRA_BF16};
      else if (TYPED) hrecs[k] = GradHalfRec{nullptr, 0};
      int* se = se_base + se_at;
      float* den = den_base + den_at;
      CombEnt* ent = ent_base + ent_at;
      const Slices sl = slices_of(d);
      se_at += sl.se;
      den_at += sl.den;
      ent_at += sl.ent;
      brecs[k] = BoundsRec{(const i64*)d.seg, se, pl->n, d.n_rows};
      crecs[k] = CombManyRec{(const i64*)d.seg, d.weights, se, den, ent, pl->n, d.n_rows, d.combiner};
      plan_grids(pl, &key_blocks[k], &bin_blocks[k]);
      key_blocks[k] = many_cap(key_blocks[k], app_n[app_of[k]]);
      bin_blocks[k] = many_cap(bin_blocks[k], hot_n[hot_of[k]]);
      // the view: under the lock, after the capacity preparation; ++use_gen: one use of the plan
      arecs[k] = ApplyManyRec{t->view_of(t->cur), opt_of(d.opt), score[k], keys_of(pl), (const float*)grad_ptr(d), pl->partial, d.param_default_row,
                              pl->out.hout, pl->binmap, pl->dflag, pl->any_deferred, ent, pl->dim, t->opts.aux_init[0],
                              t->opts.aux_init[1], ++pl->use_gen};
    }
  }
  // the pool: the entry kernels' two prefixes over all records, then the classes, which read the records through an index
  ClassPool pool{section<unsigned>(up.host, pool_off)};
  auto all = [](size_t) { return true; };
  const ManyClass ent_cls = pool.put(n_act, false, all, ent_blocks_of), den_cls = pool.put(n_act, false, all, den_blocks_of);
  ManyClass hot_cls[NHOT], app_cls[NAPP];
  for (int c = 0; c < NHOT; ++c)
    hot_cls[c] = pool.put(n_act, true, [&](size_t k) { return hot_of[k] == c; }, [&](size_t k) { return bin_blocks[k]; });
  for (int c = 0; c < NAPP; ++c)
    app_cls[c] = pool.put(n_act, true, [&](size_t k) { return app_of[k] == c; }, [&](size_t k) { return key_blocks[k]; });

  rc = many_send(up, s, (fn + ": record upload").c_str(), false);
  if (rc) return rc;
  if (hipMemsetAsync(se_base, 0, se_bytes, s) != hipSuccess)   // empty rows: start = end = 0
    return set_error(TFRA_ERR_HIP, fn + ": memset");
  uint32_t launches = 0;
  const unsigned* d_pool = section<const unsigned>(up.dev, pool_off);
  rc = comb_bounds_many(s, ent_cls.grid, section<const BoundsRec>(up.dev, brec_off), d_pool + ent_cls.at, (unsigned)n_act);
  if (rc) return rc;
  rc = comb_den_ent_many(s, den_cls.grid, ent_cls.grid, section<const CombManyRec>(up.dev, crec_off), d_pool + den_cls.at,
                         d_pool + ent_cls.at, (unsigned)n_act);
  if (rc) return rc;
  launches += 3;
  const ApplyManyRec* d_arecs = section<const ApplyManyRec>(up.dev, arec_off);
  const GradHalfRec* d_hrecs = TYPED ? section<const GradHalfRec>(up.dev, hrec_off) : nullptr;
  for (int c = 0; c < NHOT; ++c) {
    const ManyClass& k = hot_cls[c];
    if (!k.n) continue;
    launch_hot_sums_many(s, c % NHOT1 + 1, k.grid, d_arecs, c >= NHOT1 ? d_hrecs : nullptr, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
    ++launches;
  }
  for (int c = 0; c < NAPP; ++c) {
    const ManyClass& k = app_cls[c];
    if (!k.n) continue;
    const GradHalfRec* hr = c >= NAPP1 ? d_hrecs : nullptr;
    launch_apply_many(s, c % 3, c % NAPP1 / 3, false, k.grid, d_arecs, hr, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
    ++launches;
    if (app_evict[c]) {
      launch_apply_many(s, c % 3, c % NAPP1 / 3, true, k.grid, d_arecs, hr, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
      ++launches;
    }
  }
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, fn + ": launch failed");
  for (size_t i : act) reinterpret_cast<Table*>(descs[i].table)->step_writeback();
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

}  // namespace

