// Whole rows out and back: the two table calls of a dense update rule that has no fused write-back
// (optimizers.Generic with whole_rows=True).
//   tfra_table_fetch_planned  a READ over a CSR plan's distinct keys: one probe per key, its co-located fields up-cast to float32
//                             field tensors, and next to them the per-key gradient sums of tfra_reduce_by_key — gather_csr_kernel's
//                             loop (tfra_apply.hip) with find's probe and a whole-row read added.  The hot sums are tfra_apply.hip's
//                             launch (hot_sums_launch).
//   tfra_table_store_rows     the unique-keys upsert of whole rows given as float32 fields: insert_counted_kernel<G, U, true> and
//                             insert_evict_body<G, false, false> (tfra_upsert.hip) with the source rounded on the way in and the
//                             NULL-field rule.  Both are TWINS of those bodies — their probes, claim, score and accounting are
//                             repeated here so that the kernels of tfra_upsert.hip keep their code; a fix there belongs here too.
// Kernels instantiated here: fetch_rows_kernel<ST, SUMS, [GradHalf]>, store_rows_kernel<ST, U>, store_rows_evict_kernel<ST>.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_apply.h"
#include "tfra_apply_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_optim_device.h"
#include "tfra_plan.h"
#include "tfra_upsert.h"
#include "tfra_upsert_device.h"

using namespace tfra;
using namespace tfra::red;

static_assert(sizeof(tfra_row_fields) == 48, "tfra_row_fields is 48 bytes (ABI)");

namespace {

constexpr int MAXF = 5;   // fields of a row: the embedding and up to four slot vectors
struct RowsOut { float* field[MAXF]; };
struct RowsIn { const float* field[MAXF]; };

// Four stored elements of a row as ONE granule per lane: 16 bytes of a float row, 8 of a half one (the group's 16 lanes = 64 columns)
template <int ST> struct Gran4 { typedef uint2 T; };
template <> struct Gran4<TFRA_F32> { typedef float4 T; };
template <int ST> __device__ __forceinline__ float4 up4(const typename Gran4<ST>::T& r) {
  if constexpr (ST == TFRA_F32) return r;
  else return load_stored4<ST>(r);
}
// aux_init[f - 1] as the table stores it (AuxInit::pattern), up-cast
template <int ST> __device__ __forceinline__ float4 aux4(unsigned pat) {
  float a;
  if constexpr (ST == TFRA_F32) a = __uint_as_float(pat);
  else a = bits_to_float<ST>(pat & 0xffffu);
  return make_float4(a, a, a, a);
}
// fn(std::integral_constant<int, F>{}) for the fields F = FIRST .. MAXF - 1: the field index is a constant in every use, so the
// records of field pointers and the aux patterns stay kernel arguments in scalar registers (a loop the compiler does not unroll
// indexes them with a variable, and the record goes to scratch)
template <int FIRST, class Fn> __device__ __forceinline__ void for_fields(Fn&& fn) {
  if constexpr (FIRST < MAXF) { fn(std::integral_constant<int, FIRST>{}); for_fields<FIRST + 1>(fn); }
}
template <int ST> __device__ __forceinline__ void keep5(typename Gran4<ST>::T (&r)[MAXF]) {
  keep_live(r[0], r[1], r[2], r[3]);
  typename Gran4<ST>::T d = r[4];
  keep_live(d, r[4], r[0], r[1]);
}

// ---- fetch: one 16-lane group per distinct key of the plan, as gather_csr_kernel visits them (the same g, so the same row of
// every output).  Two chains in flight, as in apply_csr_body: key -> key line -> row, and keymap -> record -> gradient rows.
// The probe is find_kernel's (probe_find_word, plain loads): nothing is claimed, no score is touched.
// Per 64 columns every lane issues MAXF granule loads together, unconditionally: field f of a resident row where the caller wants
// it, else the first wanted field again (a line the group holds already); a key that is not resident reads the default row
// instead, which is its field 0, and takes the stored image of aux_init for the others.  A lane beyond dim works on column 0 and
// stores nothing.  first_want < 0: no field is wanted, the rows are not read at all.
// SUMS: gsum_out gets gather_csr_kernel's sums (sum_rows: the same tree); CS = GradHalf: over a half gradient matrix.
template <int ST, bool SUMS, class... CS>
__global__ __launch_bounds__(256) void fetch_rows_kernel(TableView v, int dim, const float* __restrict__ grads,
                                                         const float* __restrict__ partial, CsrKeys ks,
                                                         const unsigned char* __restrict__ default_row, AuxInit ai,
                                                         i64* __restrict__ keys_out, RowsOut ro, int first_want,
                                                         float* __restrict__ gsum_out, i64* __restrict__ d_count, const CS... cs) {
  constexpr bool GH = HasGradHalf<CS...>::v;
  typedef typename Gran4<ST>::T GT;
  constexpr unsigned ES = ST == TFRA_F32 ? 4u : 2u;
  const GradHalfSrc gh = grad_half_in(cs...);
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  const unsigned ngroups = (gridDim.x * blockDim.x) >> 4;
  if (blockIdx.x == 0 && threadIdx.x == 0) *d_count = ks.d_counts[PC_OVERFLOW] ? (i64)-1 : (i64)total;
  const unsigned nf = v.n_fields;
  for (unsigned wbase = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2; wbase < total; wbase += ngroups) {
    const unsigned it_raw = wbase + (unsigned)(lane >> 4);
    const bool active = it_raw < total;
    const unsigned g = active ? it_raw : total - 1;
    const i64 key = ks.dkeys[g];
    u64 h;
    const u64 b0 = bucket0(key, v.nb, h);
    const u64 b1 = bucket1(h, b0, v.nb);
    const i64 k0 = key_line(v, b0)[sub];
    bool hot = false;
    unsigned w = 0, first = 0, nsrc = 1, wmax = 1;
    if constexpr (SUMS) {
      w = load_record(ks, g, sub, hot);
      const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
      first = (unsigned)__shfl((int)w, gshift + 3);
      nsrc = hot ? (unsigned)__shfl((int)w, gshift + 4) : cnt;
      wmax = min(nsrc, 8u);
      for (int o2 = 32; o2 >= 16; o2 >>= 1) wmax = max(wmax, (unsigned)__shfl_xor((int)wmax, o2));
      wmax = (unsigned)__builtin_amdgcn_readfirstlane((int)wmax);
    }
    if (!active) continue;
    const i64 word = probe_find_word(v, key, b0, b1, k0, sub, gshift);
    const bool hit = word >= 0;
    const unsigned char* row = hit ? word_row_ptr(v, (u64)word) : default_row;
    const unsigned fstep = hit ? v.field_bytes : 0u;
    for (int c0 = 0; c0 < dim; c0 += 64) {   // (every lane takes every trip: sum_rows reads the record words of the other lanes)
      const bool col = c0 + sub * 4 < dim;
      const int c = col ? c0 + sub * 4 : 0;
      GT r[MAXF];
      if (first_want >= 0) {
#pragma unroll
        for (int f = 0; f < MAXF; ++f) {
          const bool want = (unsigned)f < nf && ro.field[f] != nullptr;
          r[f] = *reinterpret_cast<const GT*>(row + (unsigned)(want ? f : first_want) * fstep + (unsigned)c * ES);
        }
      }
      float4 gg = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (SUMS) gg = sum_rows<false, GH>(grads, partial, hot, w, first, nsrc, wmax, dim, c, gshift, 0.f, 0.f, gh);
      if (first_want >= 0) {
        keep5<ST>(r);
#pragma unroll
        for (int f = 0; f < MAXF; ++f) {
          if ((unsigned)f < nf && ro.field[f] != nullptr && col) {
            float4 x = up4<ST>(r[f]);
            if (f >= 1 && !hit) x = aux4<ST>(ai.pattern[(f - 1) & 3]);
            *reinterpret_cast<float4*>(ro.field[f] + (size_t)g * dim + c) = x;
          }
        }
      }
      if constexpr (SUMS) {
        if (col) *reinterpret_cast<float4*>(gsum_out + (size_t)g * dim + c) = gg;
      }
    }
    if (sub == 0) keys_out[g] = key;
  }
}

// ---- store: a row of the table from the caller's float32 fields, by the row's 16-lane group.  Per 64 columns the loads of all
// given fields are issued together; each element is rounded to the storage type once, to nearest even (to_stored4).
// is_new: the row was claimed by this call — a field the caller does not give starts at aux_init; on a resident row it keeps its bytes.
// WT: write-through stores (the eviction path: the row must be in memory before the key is published, see publish_key).
template <int ST, bool WT>
__device__ __forceinline__ void write_row(const TableView& v, const AuxInit& ai, unsigned char* row, const RowsIn& ri, size_t i,
                                          int dim, bool is_new, int sub) {
  constexpr unsigned ES = ST == TFRA_F32 ? 4u : 2u;
  const unsigned nf = v.n_fields;
  for (int c = sub * 4; c < dim; c += 64) {
    float4 x0, x1, x2, x3, x4;
    auto x = [&](auto F) -> float4& {
      if constexpr (F == 0) return x0; else if constexpr (F == 1) return x1; else if constexpr (F == 2) return x2;
      else if constexpr (F == 3) return x3; else return x4;
    };
    for_fields<0>([&](auto F) {
      const bool given = (unsigned)F < nf && ri.field[F] != nullptr;
      x(F) = *reinterpret_cast<const float4*>((given ? ri.field[F] : ri.field[0]) + i * (size_t)dim + c);
    });
    keep_live(x0, x1, x2, x3);
    for_fields<0>([&](auto F) {
      if ((unsigned)F < nf && ri.field[F] != nullptr) {
        unsigned char* p = row + (unsigned)F * v.field_bytes + (unsigned)c * ES;
        if constexpr (ST == TFRA_F32) {
          if (WT) store_wt16(p, *reinterpret_cast<uint4*>(&x(F)));
          else *reinterpret_cast<float4*>(p) = x(F);
        } else {
          const u64 b = to_stored4<ST>(x(F));
          if (WT) store_wt8(p, b);
          else *reinterpret_cast<u64*>(p) = b;
        }
      }
    });
  }
  if (is_new) {
    for_fields<1>([&](auto F) {
      if ((unsigned)F < nf && ri.field[F] == nullptr)
        fill_aux_field<WT>(row + (unsigned)F * v.field_bytes, v.field_bytes, ai.pattern[(F - 1) & 3], ai.elem_bytes, true, sub);
    });
  }
}

// phase 1: insert_counted_kernel<G, U, true>'s probes, claim, score and accounting (tfra_upsert.hip), the row from float32 fields
template <int ST, int U>
__global__ __launch_bounds__(256) void store_rows_kernel(TableView v, size_t n_buf, const i64* __restrict__ keys, RowsIn ri, int dim,
                                                         AuxInit ai, int strategy, u64 epoch, int bounded,
                                                         uint8_t* __restrict__ deferred, const long long* __restrict__ d_n) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = lane >> 4;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  constexpr int KPW = 4 * U;
  const size_t base = wave * KPW;
  size_t n = n_buf;
  if (d_n) {   // uniform load, as find_kernel's
    const long long dn = *d_n;
    n = dn < 0 ? 0 : min(n_buf, (size_t)dn);
  }
  if (deferred && lane < KPW && base + lane >= n && base + lane < n_buf) deferred[base + lane] = 0;
  if (base >= n) return;
  const size_t last = n - 1;
  i64 kreg = keys[min(base + (size_t)(lane & (KPW - 1)), last)];
  int fresh = 0, failed = 0;
  i64 key[U], k0[U], k1[U];
  u64 h[U], b0[U];
  const bool pf1 = bounded > 1;
#pragma unroll
  for (int u = 0; u < U; ++u) {  // U first probes in flight (unconditional, tail clamped)
    key[u] = shfl_i64(kreg, u * 4 + grp);
    b0[u] = bucket0(key[u], v.nb, h[u]);
    k0[u] = load_key_coherent(key_line(v, b0[u]) + sub);
    k1[u] = load_key_coherent(key_line(v, pf1 ? bucket1(h[u], b0[u], v.nb) : b0[u]) + sub);
  }
  static_assert(U == 4, "keep_live is written for U == 4");
  keep_live(k0[0], k0[1], k0[2], k0[3]);
  keep_live(k1[0], k1[1], k1[2], k1[3]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t i = base + (size_t)(u * 4 + grp);
    if (i >= n) continue;
    bool is_new;
    const i64 row = locate_or_claim_from(v, key[u], h[u], b0[u], k0[u], sub, gshift, is_new, bounded, pf1 ? &k1[u] : nullptr);
    if (deferred && sub == 0) deferred[i] = row == NEED_EVICT;
    if (row >= 0) {
      write_row<ST, false>(v, ai, row_ptr(v, row), ri, i, dim, is_new, sub);
      update_score(v, row, is_new, strategy, 1, epoch, sub);
      fresh += (is_new && sub == 0);
    } else if (row != NEED_EVICT) {
      failed += (sub == 0);
    }
  }
  wave_account(v, wave, lane, fresh, failed);
}

// phase 2 (a table at max_capacity): insert_evict_body<G, false, false>'s victim choice, lock, score and publication
// (tfra_upsert.hip), the row from float32 fields.  A key that is not admitted (-1) is dropped with its whole row.
template <int ST>
__global__ __launch_bounds__(256) void store_rows_evict_kernel(TableView v, size_t n, const i64* __restrict__ keys, RowsIn ri, int dim,
                                                               AuxInit ai, int strategy, u64 epoch,
                                                               const uint8_t* __restrict__ deferred) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const size_t i = (((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4);
  int fresh = 0, failed = 0;
  const bool lru_like = strategy == TFRA_EVICT_LRU || strategy == TFRA_EVICT_EPOCHLRU;
  const bool active = i < n && deferred[i];
  if (active) {
    const i64 key = keys[i];
    const u64 in_score = 1;
    const u64 compare = strategy == TFRA_EVICT_EPOCHLFU ? ((epoch << 32) | in_score) : in_score;
    u64 word = 0;
    bool claimed_empty = false;
    const i64 row = evict_and_lock(v, key, compare, lru_like, sub, gshift, &word, claimed_empty);
    if (row >= 0) {
      // the slot is LOCKED by this group: the row (a claimed row: fields that are not given at aux_init), its score, then the key
      write_row<ST, true>(v, ai, row_ptr(v, row), ri, i, dim, true, sub);
      if (sub == 0) store_wt8(score_word(v, word), 0);  // the slot starts a new life: scores count from zero
      update_score<true>(v, row, true, strategy, in_score, epoch, sub);
      publish_key(v, word, key, sub);
      fresh = (claimed_empty && sub == 0);
    } else if (row == -3) {
      failed = (sub == 0);
    }
  }
  wave_account(v, i >> 2, lane, fresh, failed);
}

// ---- host: what both calls check of a tfra_row_fields before they look at the table (nothing of it needs a device) ----
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
// ... and of the table: its value dtype, its dim, and the record's field count
Check check_table(const Table* t, const tfra_row_fields* r) {
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (r->n_fields != 1 + t->opts.aux_fields) return refuse(TFRA_ERR_INVALID, "tfra_row_fields.n_fields must be 1 + the table's aux_fields");
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16");
  if (dim % 4 != 0 || dim > 64 * MAXCH) return refuse(TFRA_ERR_UNSUPPORTED, "needs dim % 4 == 0 and dim <= 256");
  return Check{};
}

}  // namespace

extern "C" int tfra_table_fetch_planned(tfra_table_t* tp, const tfra_sparse_plan_t* pl, const tfra_grads* g, const void* default_row,
                                        int64_t* keys_out, const tfra_row_fields* rows_out, float* gsum_out, int64_t* d_count,
                                        tfra_stream_t stream) {
  const std::string who = "tfra_table_fetch_planned: ";
  if (!tp || !pl || !keys_out || !rows_out || !d_count || !default_row) return set_error(TFRA_ERR_INVALID, who + "null argument");
  if (const Check c = check_fields(rows_out, false); c.code) return report(who, c);
  if ((g != nullptr) != (gsum_out != nullptr)) return set_error(TFRA_ERR_INVALID, who + "gradients and gsum_out go together (both, or both NULL)");
  bool forward = false;
  if (g) {
    if (const Check c = check_typed(g, &forward); c.code) return report(who, c);
    if (forward && ((uintptr_t)g->grads & 15)) return set_error(TFRA_ERR_UNSUPPORTED, who + "float32 gradients must be 16-B aligned");
    if ((uintptr_t)gsum_out & 15) return set_error(TFRA_ERR_UNSUPPORTED, who + "gsum_out must be 16-B aligned");
  }
  {
    const Table* tc = reinterpret_cast<const Table*>(tp);
    if (const Check c = check_table(tc, rows_out); c.code) return report(who, c);
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
  key_blocks = std::min(key_blocks, 2048u);   // (the kernel is grid-stride)
  RowsOut ro{};
  int first_want = -1;
  for (int f = 0; f < rows_out->n_fields; ++f) {
    ro.field[f] = rows_out->field[f];
    if (ro.field[f] && first_want < 0) first_want = f;
  }
  const TableView v = t->view_of(t->cur);
  const CsrKeys ks = keys_of(pl);
  const unsigned char* dr = (const unsigned char*)default_row;
  const float* grads = forward ? (const float*)g->grads : nullptr;
  if (g) hot_sums_launch(s, pl, grads, forward ? nullptr : g, bin_blocks);
  with_stored(st_index(t->opts.value_dtype), [&](auto ST) {
    if (!g)
      fetch_rows_kernel<ST, false><<<key_blocks, 256, 0, s>>>(v, dim, nullptr, pl->partial, ks, dr, t->aux, (i64*)keys_out, ro, first_want,
                                                               nullptr, (i64*)d_count);
    else if (forward)
      fetch_rows_kernel<ST, true><<<key_blocks, 256, 0, s>>>(v, dim, grads, pl->partial, ks, dr, t->aux, (i64*)keys_out, ro, first_want,
                                                              gsum_out, (i64*)d_count);
    else
      fetch_rows_kernel<ST, true><<<key_blocks, 256, 0, s>>>(v, dim, nullptr, pl->partial, ks, dr, t->aux, (i64*)keys_out, ro, first_want,
                                                              gsum_out, (i64*)d_count, GradHalf{g->grads, g->d_scale, g->dtype == TFRA_BF16});
  });
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, who + "launch failed");
  return TFRA_OK;
}

extern "C" int tfra_table_store_rows(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const tfra_row_fields* rows,
                                     tfra_stream_t stream) {
  const std::string who = "tfra_table_store_rows: ";
  if (!tp) return set_error(TFRA_ERR_INVALID, who + "null table");
  if (n == 0) return TFRA_OK;
  if (int rc = check_batch(who.c_str(), n, keys && rows, [&] {
        if (const Check c = check_fields(rows, true); c.code) return report(who, c);
        if (const Check c = check_table(reinterpret_cast<const Table*>(tp), rows); c.code) return report(who, c);
        return (int)TFRA_OK;
      }))
    return rc;
  TABLE_ENTER();
  int rc = t->prepare_insert(n, s);   // (n is an upper bound of the keys: a growing table may grow a call early)
  if (rc) return rc;
  const u64 epoch = t->global_epoch;
  const int strat = t->opts.strategy, dim = t->opts.dim;
  constexpr int U = 4;
  const size_t waves = (n + 4 * U - 1) / (4 * U);
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
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
    store_rows_kernel<ST, U><<<grid, block, 0, s>>>(v, n, (const i64*)keys, ri, dim, t->aux, strat, epoch, bd, es.deferred, (const long long*)d_n);
    if (bounded)
      store_rows_evict_kernel<ST><<<dim3((unsigned)((n * 16 + 255) / 256)), block, 0, s>>>(v, n, (const i64*)keys, ri, dim, t->aux, strat, epoch,
                                                                                          es.deferred);
  });
  HIP_TRY(hipGetLastError());
  t->step_epoch();
  return TFRA_OK;
}
