// GRADIENT HALF of a write-back whose ids may repeat (tfra_table_apply_planned, over a CSR plan of tfra_csr.hip): the hot sums,
// then one fused optimizer update per unique key (their bodies: tfra_apply_device.h); the same sums written out instead
// (tfra_reduce_by_key, tfra_plan_reduce_to); the combined form (tfra_table_apply_planned_combined) and the one-call form
// (tfra_table_apply_sparse); the *_typed forms of the calls that read an [n, dim] gradient matrix or grad_out, for float16 / bfloat16
// gradients (GradHalf in the kernels' pack).  The grouped combined write-back is tfra_apply_many.hip, the two-stream look-ahead driver
// tfra_prefetch.hip.  A write-back's argument checks exist once (tfra_apply.h); the launch ladders are the dispatchers of
// tfra_host.h (with_opt_kind, with_stored) and with_nch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
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

// gradient half, kernel 1 (hot_sums_body): one block per bin, the grid strides over the plan's bins
template <int NCH, class... CS>
__global__ __launch_bounds__(NTA) void hot_sums_kernel(const float* __restrict__ grads, int dim,
                                                       const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                                       const unsigned* __restrict__ binmap,
                                                       const unsigned* __restrict__ d_counts, float* __restrict__ partial,
                                                       unsigned* progress, unsigned progress_val, const CS... cs) {
  hot_sums_body<NCH>(grads, dim, hent, hout, binmap, d_counts, partial, progress, progress_val, blockIdx.x, gridDim.x, cs...);
}

// gradient half, kernel 2 (apply_csr_body): one 16-lane group per unique key; PHASE2: the eviction phase of a table at max_capacity
template <int KIND, bool PHASE2, int ST, class... CS>
__global__ __launch_bounds__(256) void apply_csr_kernel(TableView v, OptP o, int dim, const float* __restrict__ grads,
                                                        const float* __restrict__ partial, CsrKeys ks,
                                                        const float* __restrict__ default_row, float aux0, float aux1,
                                                        ScoreP sp, uint8_t* __restrict__ dflag, unsigned* any_deferred,
                                                        unsigned use_gen, const CS... cs) {
  apply_csr_body<KIND, PHASE2, ST>(v, o, dim, grads, partial, ks, default_row, aux0, aux1, sp, dflag, any_deferred, use_gen,
                                   blockIdx.x, gridDim.x, cs...);
}

// ---------------------------------------------------------------------------------------------
// tfra_reduce_by_key epilogue: the same per-key sums as apply_csr_kernel, written out instead of applied.
// dest != nullptr (tfra_plan_reduce_to): the sum of a key goes to row dest[p], p = the key's last batch position — the
// caller's map from batch positions to output rows (equal for all positions of a key), e.g. position -> owner-major
// index of the multi-GPU gradient route; keys_out / d_count are not written then.
// CS = GradHalf (tfra_reduce_by_key_typed): the gradient matrix is float16 / bfloat16, read through sum_rows as the update reads
// it; `grads` is not read then.
template <class... CS>
__global__ __launch_bounds__(256) void gather_csr_kernel(int dim, const float* __restrict__ grads,
                                                         const float* __restrict__ partial, CsrKeys ks,
                                                         i64* __restrict__ keys_out, float* __restrict__ rows_out,
                                                         i64* __restrict__ d_count, const int* __restrict__ dest, const CS... cs) {
  constexpr bool GH = HasGradHalf<CS...>::v;
  const GradHalfSrc gh = grad_half_in(cs...);
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  const unsigned ngroups = (gridDim.x * blockDim.x) >> 4;
  if (d_count && blockIdx.x == 0 && threadIdx.x == 0) *d_count = ks.d_counts[PC_OVERFLOW] ? (i64)-1 : (i64)total;
  for (unsigned wbase = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2; wbase < total; wbase += ngroups) {
    const unsigned it_raw = wbase + (unsigned)(lane >> 4);
    const bool active = it_raw < total;
    const unsigned g = active ? it_raw : total - 1;
    bool hot;
    const unsigned w = load_record(ks, g, sub, hot);
    const i64 key = (i64)(((u64)(unsigned)__shfl((int)w, gshift + 1) << 32) | (unsigned)__shfl((int)w, gshift));
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    const unsigned first = (unsigned)__shfl((int)w, gshift + 3);
    const unsigned nsrc = hot ? (unsigned)__shfl((int)w, gshift + 4) : cnt;
    unsigned wmax = min(nsrc, 8u);
    for (int o2 = 32; o2 >= 16; o2 >>= 1) wmax = max(wmax, (unsigned)__shfl_xor((int)wmax, o2));
    wmax = (unsigned)__builtin_amdgcn_readfirstlane((int)wmax);
    if (!active) continue;
    size_t orow = g;
    if (dest) {
      unsigned lastp = (unsigned)__shfl((int)w, gshift + (hot ? 5 : 3));   // few: the last position itself; many: where it is stored
      if (hot) lastp = ks.hent[lastp];
      orow = (size_t)dest[lastp & E_POS];
    }
    for (int c0 = 0; c0 < dim; c0 += 64) {   // (every lane takes every trip: see apply_csr_kernel)
      const bool col = c0 + sub * 4 < dim;
      const int c = col ? c0 + sub * 4 : 0;
      const float4 gg = sum_rows<false, GH>(grads, partial, hot, w, first, nsrc, wmax, dim, c, gshift, 0.f, 0.f, gh);
      if (col) *reinterpret_cast<float4*>(rows_out + orow * dim + c) = gg;
    }
    if (keys_out && sub == 0) keys_out[g] = key;
  }
}

}  // namespace

template <class... CS>
static void launch_hot_sums(hipStream_t s, const tfra_sparse_plan* pl, const float* grads, unsigned bin_blocks, unsigned* progress,
                            unsigned progress_val, const CS&... cs) {
  const int dim = pl->dim;
  with_nch((dim + 63) / 64, [&](auto NCH) {
    hot_sums_kernel<NCH><<<bin_blocks, NTA, 0, s>>>(grads, dim, pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->partial, progress,
                                                    progress_val, cs...);
  });
}

// by the rule and by the rows' storage type (both checked by the caller)
template <class... CS>
static void launch_apply(Table* t, hipStream_t s, const tfra_sparse_plan* pl, int kind, const OptP& o, const float* grads,
                         const float* default_row, unsigned key_blocks, const ScoreP& sp, const CS&... cs) {
  TableView v = t->view_of(t->cur);
  const float a0 = t->opts.aux_init[0], a1 = t->opts.aux_init[1];
  const unsigned gen = ++pl->use_gen;
  // one RESIDENT grid (the kernel is grid-stride: 125 registers = 4 blocks per CU x 256 CUs): a batch's 33 K keys as 2075 blocks were two
  // rounds of dispatch plus a third of 27 blocks; 1024 blocks looping twice: configs[1] 55.2 -> 53.7 us per step (A/B on one box, twice)
  static const unsigned grid_cap = [] { const char* e = getenv("TFRA_APPLY_GRID_CAP"); return e ? (unsigned)atoi(e) : 1024u; }();
  if (grid_cap) key_blocks = std::min(key_blocks, grid_cap);
  // xs: the caller's pack, and behind it the rounding's StochP for the half rows of a table that rounds stochastically
  auto launch = [&](auto KIND, auto ST, const auto&... xs) {
    apply_csr_kernel<KIND, false, ST><<<key_blocks, 256, 0, s>>>(v, o, pl->dim, grads, pl->partial, keys_of(pl), default_row, a0, a1, sp,
                                                                 pl->dflag, pl->any_deferred, gen, xs...);
    if (sp.bounded)
      apply_csr_kernel<KIND, true, ST><<<key_blocks, 256, 0, s>>>(v, o, pl->dim, grads, pl->partial, keys_of(pl), default_row, a0, a1, sp,
                                                                  pl->dflag, pl->any_deferred, gen, xs...);
  };
  with_opt_kind(kind, [&](auto KIND) {
    with_stored(st_index(t->opts.value_dtype), [&](auto ST) {
      if constexpr (decltype(ST)::value != TFRA_F32) {
        if (t->stochastic()) { launch(KIND, ST, cs..., t->stoch_of()); return; }
      }
      launch(KIND, ST, cs...);
    });
  });
}

// the kernels' pack member of a half gradient matrix (hg: checked by check_typed)
static GradHalf half_of(const tfra_grads* hg) { return GradHalf{hg->grads, hg->d_scale, hg->dtype == TFRA_BF16}; }

// comb != nullptr (tfra_table_apply_planned_combined): grads is grad_out, position e's gradient is formed from comb[e]
// hg != nullptr (the *_typed calls): the gradient matrix is hg's, float16 or bfloat16; grads is not read
// both (tfra_table_apply_planned_combined_typed): hg is grad_out, a row of it is up-cast and scaled before comb[e] is applied
int tfra::apply_planned_impl(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl, const float* grads,
                              const float* param_default_row, tfra_stream_t stream, unsigned* progress, unsigned progress_val,
                             const CombEnt* comb, const tfra_grads* hg) {
  // caller holds t->mu
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  const Check c = check_apply_planned(t, p, pl, hg ? hg->grads : (const void*)grads, param_default_row,
                                      [&] { return Check{t->enter(s)}; }, hg ? 7u : 15u);
  if (c.code) return report(hg ? (comb ? "apply_planned_combined_typed: " : "apply_planned_typed: ") : "apply_planned: ", c);
  if (!c.active) return TFRA_OK;
  int rc = t->prepare_insert(pl->n, s);
  if (rc) return rc;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  if (comb && hg) launch_hot_sums(s, pl, nullptr, bin_blocks, progress, progress_val, CombRows{comb}, half_of(hg));
  else if (comb) launch_hot_sums(s, pl, grads, bin_blocks, progress, progress_val, CombRows{comb});
  else if (hg) launch_hot_sums(s, pl, nullptr, bin_blocks, progress, progress_val, half_of(hg));
  else launch_hot_sums(s, pl, grads, bin_blocks, progress, progress_val);
  uint8_t* bounded_now;
  rc = t->bounded_flags(1, s, &bounded_now);
  if (rc) return rc;
  const ScoreP sp = score_of(t, bounded_now);
  const OptP o = opt_of(p);
  if (comb && hg) launch_apply(t, s, pl, p->kind, o, nullptr, param_default_row, key_blocks, sp, CombRows{comb}, half_of(hg));
  else if (comb) launch_apply(t, s, pl, p->kind, o, grads, param_default_row, key_blocks, sp, CombRows{comb});
  else if (hg) launch_apply(t, s, pl, p->kind, o, nullptr, param_default_row, key_blocks, sp, half_of(hg));
  else launch_apply(t, s, pl, p->kind, o, grads, param_default_row, key_blocks, sp);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "apply_planned: launch failed");
  t->step_writeback();
  return TFRA_OK;
}

extern "C" int tfra_table_apply_planned(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                        const float* grads, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "apply_planned: null table");
  std::lock_guard<std::mutex> lock(t->mu);
  return apply_planned_impl(tp, p, pl, grads, param_default_row, stream, nullptr, 0);
}

// ---- the *_typed calls: the gradient matrix as the caller's dense part left it (tfra_grads).  A typed call equals its untyped
// twin on G32[e] = f32(grads[e]) * *d_scale; the kernels form G32 in registers (GradHalf, tfra_apply_device.h).
// (What a tfra_grads itself must satisfy, before anything is enqueued: check_typed, tfra_apply.h.)

extern "C" int tfra_table_apply_planned_typed(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                              const tfra_grads* g, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "apply_planned_typed: null table");
  bool forward;
  if (const Check c = check_typed(g, &forward); c.code) return report("apply_planned_typed: ", c);
  if (forward) return tfra_table_apply_planned(tp, p, pl, (const float*)g->grads, param_default_row, stream);
  std::lock_guard<std::mutex> lock(t->mu);
  return apply_planned_impl(tp, p, pl, nullptr, param_default_row, stream, nullptr, 0, nullptr, g);
}

// The write-back of an embedding_lookup_sparse: plan over the entry ids, gradient of position e = the combiner's backward
// (tfra_combine_device.h) formed from grad_out in registers — apply_planned's kernels, reading grad_out through one more
// indirection instead of an expanded [nnz, dim] gradient.
// (hg != nullptr: tfra_table_apply_planned_combined_typed on a half grad_out, checked by check_typed; grad_out is not read then)
static int apply_combined_impl(const char* who, tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                               const float* grad_out, const tfra_grads* hg, const int64_t* seg, const float* weights, int combiner,
                               size_t n_rows, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  const Check c = check_apply_combined(t, p, pl, hg ? hg->grads : (const void*)grad_out, seg, weights, combiner, n_rows, param_default_row, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};   // the scratch below was last used on the table's previous stream
  }, hg ? 7u : 15u);
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
  return apply_planned_impl(tp, p, pl, grad_out, param_default_row, stream, nullptr, 0, ent, hg);
}

extern "C" int tfra_table_apply_planned_combined(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                                 const float* grad_out, const int64_t* seg, const float* weights, int combiner,
                                                 size_t n_rows, const float* param_default_row, tfra_stream_t stream) {
  return apply_combined_impl("apply_planned_combined: ", tp, p, pl, grad_out, nullptr, seg, weights, combiner, n_rows, param_default_row,
                             stream);
}

// The typed form: grad_out as the dense part left it.  Equals the untyped call on GO32[r] = f32(grad_out[r]) * *d_scale; the kernels
// form GO32 in registers, in front of comb_grad4 (CombRows and GradHalf in one pack).
extern "C" int tfra_table_apply_planned_combined_typed(tfra_table_t* tp, const tfra_opt_params* p, const tfra_sparse_plan_t* pl,
                                                       const tfra_grads* grad_out, const int64_t* seg, const float* weights,
                                                       int combiner, size_t n_rows, const float* param_default_row,
                                                       tfra_stream_t stream) {
  bool forward;
  if (const Check c = check_typed(grad_out, &forward); c.code) return report("apply_planned_combined_typed: ", c);
  if (forward)
    return tfra_table_apply_planned_combined(tp, p, pl, (const float*)grad_out->grads, seg, weights, combiner, n_rows, param_default_row,
                                             stream);
  return apply_combined_impl("apply_planned_combined_typed: ", tp, p, pl, nullptr, grad_out, seg, weights, combiner, n_rows,
                             param_default_row, stream);
}

// tfra_table_apply_sparse for more ids than a plan holds (2^18).  Equal ids must still meet in ONE update, whatever
// chunk they sit in:
//   1. per chunk of 2^18 ids: unique + per-key gradient sums (tfra_reduce_by_key) into one concatenated list — a key now
//      occurs at most once per chunk, so even the hottest id of a Zipf batch is a handful of entries;
//   2. the list fits a plan: one planned write-back sums a key's entries in chunk order and applies it;
//      else the list is split by key hash (tfra_partition, mode 2) into parts that fit — a key's entries stay together,
//      the parts are disjoint key sets — and each part is written back on its own.
// A slow path (host reads of the counts, scratch allocated per call); results are deterministic, the association of the
// sums is (within chunk) + (across chunks in order).
// hg != nullptr (tfra_table_apply_sparse_typed): stage 1 is the typed reduce; the sums are float, the rest is unchanged.
static int reduce_by_key_impl(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const float* grads, const tfra_grads* hg,
                              int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream);
static int apply_sparse_big(Table* t, tfra_table_t* tp, tfra_sparse_plan* pl, const tfra_opt_params* p, size_t n, const int64_t* ids,
                            const float* grads, const tfra_grads* hg, const float* param_default_row, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int dim = t->opts.dim;
  tfra_workspace_t* ws;
  if (int rc = workspace_in(&t->big_ws, t->device, &ws)) return rc;
  i64 *keys_cat, *d_cnt, *keys_part;
  float *sums_cat, *sums_part;
  int* perm;
  Scratch scratch(s);   // (freed behind a synchronisation of s, on every way out)
  auto oom = [] { return set_error(TFRA_ERR_OOM, "apply_sparse: scratch for a batch of more than 2^18 ids"); };
  if (!scratch.device(&keys_cat, n * sizeof(i64)) || !scratch.device(&sums_cat, n * (size_t)dim * sizeof(float)) ||
      !scratch.device(&d_cnt, sizeof(i64)))
    return oom();
  size_t T = 0;
  for (size_t off = 0; off < n; off += MAX_IDS) {
    const size_t m = std::min<size_t>(MAX_IDS, n - off);
    tfra_grads part;   // (rows of dim % 4 == 0 halves: a chunk's matrix is 8-B aligned as the whole is)
    if (hg) { part = *hg; part.grads = (const unsigned short*)hg->grads + off * (size_t)dim; }
    int rc = reduce_by_key_impl(ws, m, ids + off, dim, hg ? nullptr : grads + off * (size_t)dim, hg ? &part : nullptr,
                                (int64_t*)keys_cat + T, sums_cat + T * (size_t)dim, (int64_t*)d_cnt, stream);
    if (rc) return rc;
    i64 c = 0;
    if (hipMemcpyAsync(&c, d_cnt, sizeof(i64), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return set_error(TFRA_ERR_HIP, "apply_sparse: count read");
    if (c < 0) return set_error(TFRA_ERR_FULL, "apply_sparse: a de-duplication plan overflowed");
    T += (size_t)c;
  }
  if (T <= MAX_IDS) {
    int rc = tfra_sparse_plan_build(pl, T, (const int64_t*)keys_cat, dim, stream);
    if (!rc) rc = apply_planned_impl(tp, p, pl, sums_cat, param_default_row, stream, nullptr, 0);
    return rc;
  }
  if (!scratch.device(&keys_part, T * sizeof(i64)) || !scratch.device(&perm, T * sizeof(int)) ||
      !scratch.device(&sums_part, T * (size_t)dim * sizeof(float)))
    return oom();
  for (size_t P = (T + (MAX_IDS / 2) - 1) / (MAX_IDS / 2); P <= 2048; P *= 2) {
    Scratch per_attempt(s);   // the parts' counts: as many as THIS attempt has parts
    i64* d_counts;
    if (!per_attempt.device(&d_counts, P * sizeof(i64))) return oom();
    int rc = tfra_partition(ws, T, nullptr, (const int64_t*)keys_cat, (int)P, 2, (int64_t*)keys_part, perm, (int64_t*)d_counts, stream);
    if (rc) return rc;
    std::vector<i64> counts(P);
    if (hipMemcpyAsync(counts.data(), d_counts, P * sizeof(i64), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return set_error(TFRA_ERR_HIP, "apply_sparse: count read");
    bool fits = true;
    for (i64 c : counts) fits = fits && (size_t)c <= MAX_IDS;
    if (!fits) continue;   // a part too large (skewed hash): more parts
    rc = tfra_gather_rows(T, (size_t)dim * sizeof(float), sums_cat, perm, sums_part, stream);
    if (rc) return rc;
    size_t off = 0;
    // ONE logical write-back: the epoch / step counters of the EPOCH* strategies advance once, not once per part (the
    // reference counts one upsert per write-back, lookup_table_op_hkv.h:528-536).  (On a bounded table at max_capacity a
    // later part may still evict keys an earlier part of the same batch inserted.)
    t->epoch_hold = true;
    for (i64 c : counts) {
      if (c > 0) {
        rc = tfra_sparse_plan_build(pl, (size_t)c, (const int64_t*)keys_part + off, dim, stream);
        if (!rc) rc = apply_planned_impl(tp, p, pl, sums_part + off * (size_t)dim, param_default_row, stream, nullptr, 0);
        if (rc) { t->epoch_hold = false; return rc; }
      }
      off += (size_t)c;
    }
    t->epoch_hold = false;
    t->step_writeback();
    return TFRA_OK;
  }
  return set_error(TFRA_ERR_UNSUPPORTED, "apply_sparse: could not split the batch into parts of 2^18 ids");
}

// tfra_table_apply_sparse (hg == nullptr) and tfra_table_apply_sparse_typed on half gradients (hg, checked by check_typed; grads
// is not read then): one function, `who` names the caller in the refusals
static int apply_sparse_impl(const char* who, tfra_table_t* tp, const tfra_opt_params* p, size_t n, const int64_t* ids, const float* grads,
                             const tfra_grads* hg, const float* param_default_row, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  const std::string pre = std::string(who) + ": ";
  if (!t || !p) return set_error(TFRA_ERR_INVALID, (pre + "null argument").c_str());
  if (n == 0) return TFRA_OK;
  const void* gsrc = hg ? hg->grads : (const void*)grads;
  if (!ids || !gsrc || !param_default_row) return set_error(TFRA_ERR_INVALID, (pre + "null buffer").c_str());
  const int dt = t->opts.value_dtype;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return set_error(TFRA_ERR_UNSUPPORTED, (pre + "value_dtype must be float32, float16 or bfloat16 (the default row is float32)").c_str());
  const int dim = t->opts.dim;
  if (dim % 4 != 0 || dim > 64 * MAXCH || ((uintptr_t)gsrc & (hg ? 7 : 15)) || ((uintptr_t)param_default_row & 15))
    return set_error(TFRA_ERR_UNSUPPORTED, (pre + "needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers (half gradients: 8-B) "
                                                  "(use tfra_unique + tfra_segment_sum + tfra_table_apply_optimizer otherwise)").c_str());
  tfra_sparse_plan* pl;
  std::lock_guard<std::mutex> lock(t->mu);
  if (const Check c = check_rounding(t); c.code) return report(pre.c_str(), c);   // (before the plan build is enqueued)
  int rc = t->enter((hipStream_t)stream);   // orders the rebuild of the table's own plan behind its previous use
  if (rc) return rc;
  rc = own_plan(t, &pl);
  if (rc) return rc;
  if (n > MAX_IDS) return apply_sparse_big(t, tp, pl, p, n, ids, grads, hg, param_default_row, stream);
  rc = tfra_sparse_plan_build(pl, n, ids, dim, stream);
  if (rc) return rc;
  return apply_planned_impl(tp, p, pl, grads, param_default_row, stream, nullptr, 0, nullptr, hg);
}

extern "C" int tfra_table_apply_sparse(tfra_table_t* tp, const tfra_opt_params* p, size_t n, const int64_t* ids,
                                       const float* grads, const float* param_default_row, tfra_stream_t stream) {
  return apply_sparse_impl("apply_sparse", tp, p, n, ids, grads, nullptr, param_default_row, stream);
}

extern "C" int tfra_table_apply_sparse_typed(tfra_table_t* tp, const tfra_opt_params* p, size_t n, const int64_t* ids,
                                             const tfra_grads* g, const float* param_default_row, tfra_stream_t stream) {
  bool forward;
  if (const Check c = check_typed(g, &forward); c.code) return report("apply_sparse_typed: ", c);
  if (forward) return tfra_table_apply_sparse(tp, p, n, ids, (const float*)g->grads, param_default_row, stream);
  return apply_sparse_impl("apply_sparse_typed", tp, p, n, ids, nullptr, g, param_default_row, stream);
}

// unique + unsorted_segment_sum in one call = the plan + the hot sums + a gather (the reduction half of
// tfra_table_apply_sparse with the same summation tree, so routing the sums elsewhere — multi-GPU gradient
// alltoall — and applying them there gives the same bits as applying them here).
// (hg != nullptr: tfra_reduce_by_key_typed on half gradients, checked by check_typed; grads is not read then)
static int reduce_by_key_impl(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const float* grads, const tfra_grads* hg,
                              int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const std::string pre = hg ? "reduce_by_key_typed: " : "reduce_by_key: ";
  if (!ws || !d_count) return set_error(TFRA_ERR_INVALID, (pre + "null argument").c_str());
  if (on_device(ws->device) != hipSuccess) return set_error(TFRA_ERR_HIP, (pre + "hipSetDevice").c_str());
  if (n == 0) {
    if (hipMemsetAsync(d_count, 0, sizeof(int64_t), s) != hipSuccess) return set_error(TFRA_ERR_HIP, (pre + "memset").c_str());
    return TFRA_OK;
  }
  const void* gsrc = hg ? hg->grads : (const void*)grads;
  if (!ids || !gsrc || !keys_out || !rows_out) return set_error(TFRA_ERR_INVALID, (pre + "null buffer").c_str());
  if (dim <= 0 || dim % 4 != 0 || dim > 64 * MAXCH || ((uintptr_t)gsrc & (hg ? 7 : 15)) || ((uintptr_t)rows_out & 15))
    return set_error(TFRA_ERR_UNSUPPORTED, (pre + "needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers (half gradients: 8-B) "
                                                  "(use tfra_unique + tfra_segment_sum otherwise)").c_str());
  if (n > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, (pre + "at most 2^18 ids per call").c_str());
  tfra_sparse_plan* pl;
  int rc = plan_in(&ws->plan, ws->device, &pl);
  if (rc) return rc;
  rc = tfra_sparse_plan_build(pl, n, ids, dim, stream);
  if (rc) return rc;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  if (hg) {
    launch_hot_sums(s, pl, nullptr, bin_blocks, nullptr, 0, half_of(hg));
    gather_csr_kernel<<<key_blocks, 256, 0, s>>>(dim, nullptr, pl->partial, keys_of(pl), (i64*)keys_out, rows_out, (i64*)d_count, nullptr,
                                                 half_of(hg));
  } else {
    launch_hot_sums(s, pl, grads, bin_blocks, nullptr, 0);   // (pl->dim == dim)
    gather_csr_kernel<<<key_blocks, 256, 0, s>>>(dim, grads, pl->partial, keys_of(pl), (i64*)keys_out, rows_out, (i64*)d_count, nullptr);
  }
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, (pre + "launch failed").c_str());
  return TFRA_OK;
}

extern "C" int tfra_reduce_by_key(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const float* grads,
                                  int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream) {
  return reduce_by_key_impl(ws, n, ids, dim, grads, nullptr, keys_out, rows_out, d_count, stream);
}

extern "C" int tfra_reduce_by_key_typed(tfra_workspace_t* ws, size_t n, const int64_t* ids, int dim, const tfra_grads* g,
                                        int64_t* keys_out, float* rows_out, int64_t* d_count, tfra_stream_t stream) {
  bool forward;
  if (const Check c = check_typed(g, &forward); c.code) return report("reduce_by_key_typed: ", c);
  if (forward) return tfra_reduce_by_key(ws, n, ids, dim, (const float*)g->grads, keys_out, rows_out, d_count, stream);
  return reduce_by_key_impl(ws, n, ids, dim, nullptr, g, keys_out, rows_out, d_count, stream);
}

// The per-key gradient sums of a batch whose plan was built ahead (tfra_sparse_plan_build with the table's dim, on any
// stream): hot sums + gather, the reduction half of tfra_reduce_by_key with the same summation tree, written to
// rows_out[dest[p]] where p is a position of the key.  dest [n] int32: the caller's map from batch positions to output
// rows, the same for every position of a key (e.g. position -> owner-major index of the multi-GPU gradient route, which
// is known from the ids alone).  rows_out must have a row for every value in dest; rows no key maps to are not written.
extern "C" int tfra_plan_reduce_to(const tfra_sparse_plan_t* pl, const float* grads, const int32_t* dest, float* rows_out,
                                   tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!pl) return set_error(TFRA_ERR_INVALID, "plan_reduce_to: null plan");
  if (pl->kind == 1) return set_error(TFRA_ERR_UNSUPPORTED, "plan_reduce_to: needs a plan built with the table's dim");
  if (pl->n == 0) return TFRA_OK;
  if (!grads || !dest || !rows_out) return set_error(TFRA_ERR_INVALID, "plan_reduce_to: null buffer");
  const int dim = pl->dim;
  if (dim <= 0 || (((uintptr_t)grads | (uintptr_t)rows_out) & 15))
    return set_error(TFRA_ERR_INVALID, "plan_reduce_to: the plan must have been built with the rows' dim; buffers 16-B aligned");
  if (on_device(pl->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "plan_reduce_to: hipSetDevice");
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  launch_hot_sums(s, pl, grads, bin_blocks, nullptr, 0);
  gather_csr_kernel<<<key_blocks, 256, 0, s>>>(dim, grads, pl->partial, keys_of(pl), nullptr, rows_out, nullptr, (const int*)dest);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "plan_reduce_to: launch failed");
  return TFRA_OK;
}

// The hot sums of a plan for a unit that has no sums kernel of its own (tfra_rows.hip): the launch tfra_reduce_by_key makes, over
// the float matrix `grads` or, hg != nullptr (checked by check_typed), over hg's half matrix.
void tfra::hot_sums_launch(hipStream_t s, const tfra_sparse_plan_t* pl, const float* grads, const tfra_grads* hg, unsigned bin_blocks) {
  if (hg) launch_hot_sums(s, pl, nullptr, bin_blocks, nullptr, 0, half_of(hg));
  else launch_hot_sums(s, pl, grads, bin_blocks, nullptr, 0);
}
