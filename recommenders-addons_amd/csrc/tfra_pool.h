// What the pooled lookups (tfra_pool.hip; typed: tfra_pool_typed.hip; long rows: tfra_pool_long.hip; wide rows, with their weight
// gradients: tfra_pool_wide.hip; over a tier: tfra_tierpool.hip)
// and the gradients of their weights (tfra_wgrad.hip; over a tier: tfra_tierwgrad.hip; over a list: tfra_wgrad_many.hip) share, ONE
// copy each: the up-cast of a stored row (PoolRow), the launch ladders by value dtype and row width (with_pool_class,
// with_ragged_class), the argument checks of the tuple and the ragged call (check_find_combine, check_find_combine_ragged;
// check_dw_out for the gradient's output) and, at the end, the host frame of every SINGLE call: four function templates (forward
// and weight gradient, tuple and ragged) over an owner (TableOwner here, TierOwner in tfra_tier.h) and the unit's launch.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"

namespace tfra {
int comb_bounds(hipStream_t s, size_t nnz, const int64_t* seg, size_t n_rows, int* se);   // tfra_combine.hip (tfra_combine_device.h)

namespace {

// four elements of a row as float32: a 16-B load of a float32 row, an 8-B load of a half row up-cast exactly
template <int DT> struct PoolRow;
template <> struct PoolRow<TFRA_F32> {
  typedef float4 Raw;
  static __device__ __forceinline__ float4 widen(float4 x) { return x; }
};
template <> struct PoolRow<TFRA_F16> {
  typedef uint2 Raw;
  static __device__ __forceinline__ float h(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ float4 widen(uint2 x) {
    return make_float4(h((unsigned short)x.x), h((unsigned short)(x.x >> 16)), h((unsigned short)x.y), h((unsigned short)(x.y >> 16)));
  }
};
template <> struct PoolRow<TFRA_BF16> {
  typedef uint2 Raw;
  static __device__ __forceinline__ float4 widen(uint2 x) {
    return make_float4(bf16_to_f32((unsigned short)x.x), bf16_to_f32((unsigned short)(x.x >> 16)), bf16_to_f32((unsigned short)x.y),
                       bf16_to_f32((unsigned short)(x.y >> 16)));
  }
};

// four float32 as an output row's elements (the typed lookups): themselves, or rounded to nearest even to a half
// type and packed into 8 B — float16 by the _Float16 cast add2_f16 uses, bfloat16 by f32_to_bf16 (tfra_device.h)
template <int OT> struct PoolOut;
template <> struct PoolOut<TFRA_F32> {
  typedef float Elem;
  typedef float4 Vec;
  static __device__ __forceinline__ float4 narrow(float4 x) { return x; }
};
template <> struct PoolOut<TFRA_F16> {
  typedef unsigned short Elem;
  typedef uint2 Vec;
  static __device__ __forceinline__ unsigned h(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ uint2 narrow(float4 x) { return make_uint2(h(x.x) | (h(x.y) << 16), h(x.z) | (h(x.w) << 16)); }
};
template <> struct PoolOut<TFRA_BF16> {
  typedef unsigned short Elem;
  typedef uint2 Vec;
  static __device__ __forceinline__ uint2 narrow(float4 x) {
    return make_uint2((unsigned)f32_to_bf16(x.x) | ((unsigned)f32_to_bf16(x.y) << 16),
                      (unsigned)f32_to_bf16(x.z) | ((unsigned)f32_to_bf16(x.w) << 16));
  }
};

// NCH by the row width: 1 (dim <= 64), 2 (<= 128) or 4 column chunks; f(std::integral_constant<int, NCH>{}) for the index
int nch_index(int dim) { return dim <= 64 ? 0 : dim <= 128 ? 1 : 2; }
template <class F>
void with_nch(int index, F&& f) {
  switch (index) {
    case 0: f(std::integral_constant<int, 1>{}); break;
    case 1: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
// launch(DT, U, NCH) for a table's storage type index and NCH index: the one ladder of the single and the grouped launch
template <class F>
void with_pool_class(int st, int nch, F&& launch) {
  with_stored(st, [&](auto DT) { with_nch(nch, [&](auto NCH) { launch(DT, std::integral_constant<int, 4>{}, NCH); }); });
}

// The checks of a pooled lookup, for tfra_table_find_combine and for each descriptor of tfra_multi_find_combine.
// active: there are rows to write.
const char* const NEEDS_DIM = "needs dim % 4 == 0 and dim <= 256";
// The row widths a pooled call serves, as a rule: its refusal's words, or nullptr.  narrow_dims is the rule of every call but the
// wide-row ones (tfra_pool_wide.hip), which bring wide_dims; an owner names another rule than narrow_dims as Owner::DIMS (dims_of).
typedef const char* (*DimRule)(int dim);
const char* narrow_dims(int dim) { return dim % 4 != 0 || dim > 256 ? NEEDS_DIM : nullptr; }
const char* const NEEDS_WIDE_DIM =
    "needs dim % 4 == 0 and 256 < dim <= 1024 (dim <= 256: tfra_table_find_combine, its ragged form and their *_backprop_weights forms)";
const char* wide_dims(int dim) { return dim % 4 != 0 || dim <= 256 || dim > 1024 ? NEEDS_WIDE_DIM : nullptr; }
template <class Owner> constexpr auto dims_of(int) -> decltype(Owner::DIMS) { return Owner::DIMS; }
template <class Owner> constexpr DimRule dims_of(long) { return narrow_dims; }
template <class AtEntry>
Check check_find_combine(const Table* t, const tfra_workspace* ws, size_t nnz, const void* ids, const void* seg, const float* weights,
                         int combiner, size_t n_rows, const void* default_row, const float* out, AtEntry&& at_entry,
                         DimRule dims = narrow_dims) {
  if (!t) return refuse(TFRA_ERR_INVALID, "null table");
  if (!ws || combiner < 0 || combiner > 2) return refuse(TFRA_ERR_INVALID, "bad argument");
  if (Check e = at_entry(); e.done()) return e;
  if (ws->device != t->device) return refuse(TFRA_ERR_INVALID, "workspace and table live on different devices");
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16");
  if (const char* m = dims(dim)) return refuse(TFRA_ERR_UNSUPPORTED, m);
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return refuse(TFRA_ERR_UNSUPPORTED, "too large (nnz < 2^31, n_rows < 2^30)");
  if ((((uintptr_t)out | (uintptr_t)default_row) & 15) || ((uintptr_t)ids & 7) || ((uintptr_t)seg & 7) || ((uintptr_t)weights & 3))
    return refuse(TFRA_ERR_UNSUPPORTED, "misaligned buffer (out and default_row: 16 bytes)");
  if (n_rows == 0) return nothing_to_do();
  if (!out) return refuse(TFRA_ERR_INVALID, "null out");
  if (nnz && (!ids || !seg || !default_row)) return refuse(TFRA_ERR_INVALID, "null buffer");
  return Check{};
}

// The checks of a ragged pooled lookup, for tfra_table_find_combine_ragged and for each descriptor of tfra_multi_find_combine_ragged:
// check_find_combine's codes and wording for table, dtype, dim, size and alignment, and what only the ragged form can get wrong.
// ws: the grouped call's workspace; the single call needs none (NULL).  row_splits' CONTENT is not looked at: the kernel clamps it.
template <class AtEntry>
Check check_find_combine_ragged(const Table* t, const tfra_workspace* ws, size_t n_rows, const void* row_splits, size_t nnz, const void* ids,
                                const float* weights, int combiner, uint32_t flags, uint32_t reserved, const void* default_row,
                                const float* out, AtEntry&& at_entry, DimRule dims = narrow_dims) {
  if (!t) return refuse(TFRA_ERR_INVALID, "null table");
  if (combiner < 0 || combiner > 2) return refuse(TFRA_ERR_INVALID, "bad argument");
  if (flags & ~(TFRA_RAGGED_PRUNE | TFRA_RAGGED_FILL)) return refuse(TFRA_ERR_INVALID, "unknown flag bits (TFRA_RAGGED_PRUNE | TFRA_RAGGED_FILL)");
  if (reserved) return refuse(TFRA_ERR_INVALID, "reserved must be 0");
  if (Check e = at_entry(); e.done()) return e;
  if (ws && ws->device != t->device) return refuse(TFRA_ERR_INVALID, "workspace and table live on different devices");
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16");
  if (const char* m = dims(dim)) return refuse(TFRA_ERR_UNSUPPORTED, m);
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return refuse(TFRA_ERR_UNSUPPORTED, "too large (nnz < 2^31, n_rows < 2^30)");
  if ((((uintptr_t)out | (uintptr_t)default_row) & 15) || ((uintptr_t)ids & 7) || ((uintptr_t)weights & 3))
    return refuse(TFRA_ERR_UNSUPPORTED, "misaligned buffer (out and default_row: 16 bytes)");
  if ((uintptr_t)row_splits & 7) return refuse(TFRA_ERR_UNSUPPORTED, "misaligned row_splits (8 bytes)");
  if (n_rows == 0) return nothing_to_do();
  if (!out) return refuse(TFRA_ERR_INVALID, "null out");
  if (!row_splits) return refuse(TFRA_ERR_INVALID, "null row_splits");
  if ((nnz && !ids) || ((nnz || (flags & TFRA_RAGGED_FILL)) && !default_row)) return refuse(TFRA_ERR_INVALID, "null buffer");
  return Check{};
}
// what only the weight-gradient calls can get wrong, behind the forward's checks: dw_out
Check check_dw_out(size_t nnz, const float* dw_out) {
  if (nnz && !dw_out) return refuse(TFRA_ERR_INVALID, "null dw_out");
  if ((uintptr_t)dw_out & 3) return refuse(TFRA_ERR_UNSUPPORTED, "misaligned dw_out (4 bytes)");
  return Check{};
}
// what only a typed lookup can get wrong (tfra_rows_out), in front of its twin's checks.  NULL rows are left to the twin ("null
// out", behind its n_rows == 0): out_for_twin() is what the twin's checks look at in the place of its float* out — a half matrix
// needs 8 bytes where the twin asks 16, and that has been decided here.
Check check_rows_out(const tfra_rows_out* o) {
  if (!o) return refuse(TFRA_ERR_INVALID, "null out record");
  if (o->reserved) return refuse(TFRA_ERR_INVALID, "out.reserved must be 0");
  if (o->dtype != TFRA_F32 && o->dtype != TFRA_F16 && o->dtype != TFRA_BF16)
    return refuse(TFRA_ERR_INVALID, "out.dtype must be TFRA_F32, TFRA_F16 or TFRA_BF16");
  if ((uintptr_t)o->rows & (o->dtype == TFRA_F32 ? 15 : 7))
    return refuse(TFRA_ERR_UNSUPPORTED, "misaligned out.rows (float32: 16 bytes, halves: 8 bytes)");
  return Check{};
}
const float* out_for_twin(const tfra_rows_out& o) { return reinterpret_cast<const float*>((uintptr_t)o.rows & ~(uintptr_t)15); }
// The same for a half grad_out of the typed weight gradients (tfra_grads, checked by check_typed: 8-byte aligned, not NULL): what the
// twin's checks look at in the place of its float* grad_out.
const float* grads_for_twin(const tfra_grads& g) { return reinterpret_cast<const float*>((uintptr_t)g.grads & ~(uintptr_t)15); }
// whether the flags change anything: the SAFE kernels run only then
bool ragged_safe(uint32_t flags, const float* weights) { return (flags & TFRA_RAGGED_FILL) || ((flags & TFRA_RAGGED_PRUNE) && weights); }
// launch(DT, U, NCH, SAFE): with_pool_class with the ragged forms' fourth axis
template <class F>
void with_ragged_class(int st, int nch, bool safe, F&& launch) {
  with_pool_class(st, nch, [&](auto DT, auto U, auto NCH) {
    if (safe) launch(DT, U, NCH, std::true_type{});
    else launch(DT, U, NCH, std::false_type{});
  });
}

// ---- the host frames of the SINGLE pooled calls -------------------------------------------------------------------------------------
// A call is: refuse a missing owner, run the form's checks (which enter the owner where the single call locks), append the owner's
// hint to NEEDS_DIM, report behind the entry point's name, take the early returns, (tuple forms) lay the rows' bounds into the
// workspace, launch, hipGetLastError.  That is written here once per form; an entry point names itself, its owner and its operands
// and writes its launch.  The launch runs after the owner is entered and takes the table views itself: a table that grew since
// the last call has another one.  What differs between the callers comes in through the owner and the launch alone.
//
// An owner is what a call enters and whose table the checks run on.  It holds its locks for as long as the frame runs and carries:
//   present()      a refusal in the owner's words where there is nothing to enter, in front of everything else;
//   table()        the table the checks run on;
//   enter(s)       lock and enter on s;
//   FORWARD_HINT, GRADIENT_HINT   what NEEDS_DIM advises instead;
//   DIMS           (optional) the row widths its calls serve, where not narrow_dims: WideOwner, whose refusal carries its own advice;
//   OUT_IS_GRAD    behind the entry point's name, the prefix of the forward's checks where grad_out stands in the place of out.
struct TableOwner {
  static constexpr const char* FORWARD_HINT = " (use tfra_unique + tfra_table_find + tfra_sparse_segment_combine otherwise)";
  static constexpr const char* GRADIENT_HINT = " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  static constexpr const char* OUT_IS_GRAD = " (out = grad_out): ";
  Table* t;
  std::unique_lock<std::mutex> lock;
  explicit TableOwner(tfra_table_t* tp) : t(reinterpret_cast<Table*>(tp)) {}
  Check present() const { return Check{}; }   // a NULL table is the checks' "null table"
  Table* table() const { return t; }
  int enter(hipStream_t s) {
    lock = std::unique_lock<std::mutex>(t->mu);
    return t->enter(s);
  }
};

// the owner of the wide-row calls (tfra_pool_wide.hip): a table, entered as TableOwner enters it, with 256 < dim <= 1024
struct WideOwner : TableOwner {
  static constexpr DimRule DIMS = wide_dims;
  using TableOwner::TableOwner;
};

// the bounds of a tuple call's rows, [2 * n_rows] ints at the head of the workspace (comb_bounds: a memset and one launch)
int pooled_bounds(tfra_workspace* ws, hipStream_t s, size_t nnz, const int64_t* seg, size_t n_rows, int** se) {
  if (int rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s)) return rc;
  *se = (int*)ws->buf;
  return comb_bounds(s, nnz, seg, n_rows, *se);
}

// The forward frames.  out_checked: what the twin's checks look at (out, or out_for_twin(*out)); out and elem: the address the
// nnz == 0 shortcut zeroes and the bytes of an output element (4, or 2 for half outputs: +0.0 is all-zero bits in every type).
// launch(se) / launch(): the unit's kernel over the rows' bounds / over row_splits.
template <class Owner, class Launch>
int find_combine_call(const char* who, Owner owner, tfra_workspace* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                      const float* weights, int combiner, size_t n_rows, const void* default_row, const float* out_checked, void* out,
                      size_t elem, hipStream_t s, Launch&& launch) {
  if (const Check e = owner.present(); e.code) return report(std::string(who) + ": ", e);
  Check c = check_find_combine(owner.table(), ws, nnz, ids, seg, weights, combiner, n_rows, default_row, out_checked,
                               [&] { return Check{owner.enter(s)}; }, dims_of<Owner>(0));
  if (c.msg == NEEDS_DIM) c.msg += Owner::FORWARD_HINT;
  if (c.code) return report(std::string(who) + ": ", c);
  if (!c.active) return TFRA_OK;
  if (nnz == 0) {
    const int dim = owner.table()->opts.dim;
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * elem, s));
    return TFRA_OK;
  }
  int* se;
  if (int rc = pooled_bounds(ws, s, nnz, seg, n_rows, &se)) return rc;
  launch(se);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

template <class Owner, class Launch>
int find_combine_ragged_call(const char* who, Owner owner, size_t n_rows, const int64_t* row_splits, size_t nnz, const int64_t* ids,
                             const float* weights, int combiner, uint32_t flags, const void* default_row, const float* out_checked,
                             void* out, size_t elem, hipStream_t s, Launch&& launch) {
  if (const Check e = owner.present(); e.code) return report(std::string(who) + ": ", e);
  Check c = check_find_combine_ragged(owner.table(), nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row,
                                      out_checked, [&] { return Check{owner.enter(s)}; }, dims_of<Owner>(0));
  if (c.msg == NEEDS_DIM) c.msg += Owner::FORWARD_HINT;
  if (c.code) return report(std::string(who) + ": ", c);
  if (!c.active) return TFRA_OK;
  if (nnz == 0 && !(flags & TFRA_RAGGED_FILL)) {
    const int dim = owner.table()->opts.dim;
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * elem, s));
    return TFRA_OK;
  }
  launch();
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

// The weight-gradient frames: the forward's checks with grad_checked (grad_out, or grads_for_twin(*hg)) in the place of out, then
// dw_out.  No entry: nothing is written.  Otherwise dw_out is zeroed FIRST — an entry in no row, or outside the clamped cover of
// row_splits, gets 0 — and a call without rows ends there.
template <class Owner, class Launch>
int find_combine_wgrad_call(const char* who, Owner owner, tfra_workspace* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                            const float* weights, int combiner, size_t n_rows, const void* default_row, const float* grad_checked,
                            float* dw_out, hipStream_t s, Launch&& launch) {
  if (const Check e = owner.present(); e.code) return report(std::string(who) + ": ", e);
  Check c = check_find_combine(owner.table(), ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grad_checked,
                               [&] { return Check{owner.enter(s)}; }, dims_of<Owner>(0));
  if (c.msg == NEEDS_DIM) c.msg += Owner::GRADIENT_HINT;
  if (c.code) return report(std::string(who) + Owner::OUT_IS_GRAD, c);
  if (const Check d = check_dw_out(nnz, dw_out); d.code) return report(std::string(who) + ": ", d);
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));
  if (!c.active) return TFRA_OK;
  int* se;
  if (int rc = pooled_bounds(ws, s, nnz, seg, n_rows, &se)) return rc;
  launch(se);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

template <class Owner, class Launch>
int find_combine_ragged_wgrad_call(const char* who, Owner owner, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                   const int64_t* ids, const float* weights, int combiner, uint32_t flags, const void* default_row,
                                   const float* grad_checked, float* dw_out, hipStream_t s, Launch&& launch) {
  if (const Check e = owner.present(); e.code) return report(std::string(who) + ": ", e);
  Check c = check_find_combine_ragged(owner.table(), nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row,
                                      grad_checked, [&] { return Check{owner.enter(s)}; }, dims_of<Owner>(0));
  if (c.msg == NEEDS_DIM) c.msg += Owner::GRADIENT_HINT;
  if (c.code) return report(std::string(who) + Owner::OUT_IS_GRAD, c);
  if (const Check d = check_dw_out(nnz, dw_out); d.code) return report(std::string(who) + ": ", d);
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));
  if (!c.active) return TFRA_OK;
  launch();
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
// what the weight gradients' ragged ladder takes as its fourth axis: PRUNE.  FILL changes nothing (a row that takes the fill row has
// no members: its entries are 0 whatever fill_id holds), and PRUNE without weights neither.
bool wgrad_prune(uint32_t flags, const float* weights) { return (flags & TFRA_RAGGED_PRUNE) && weights; }

}  // namespace
}  // namespace tfra
