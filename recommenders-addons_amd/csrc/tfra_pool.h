// What the pooled lookup (tfra_pool.hip; over a tier: tfra_tierpool.hip) and the gradient of its weights (tfra_wgrad.hip; over a tier: tfra_tierwgrad.hip; over a list: tfra_wgrad_many.hip) share, ONE copy each: the up-cast of a
// stored row (PoolRow), the launch ladders by value dtype and row width (with_pool_class, with_ragged_class) and the argument checks
// of the tuple and the ragged call (check_find_combine, check_find_combine_ragged; check_dw_out for the gradient's output).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"

namespace tfra {
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
template <class AtEntry>
Check check_find_combine(const Table* t, const tfra_workspace* ws, size_t nnz, const void* ids, const void* seg, const float* weights,
                         int combiner, size_t n_rows, const void* default_row, const float* out, AtEntry&& at_entry) {
  if (!t) return refuse(TFRA_ERR_INVALID, "null table");
  if (!ws || combiner < 0 || combiner > 2) return refuse(TFRA_ERR_INVALID, "bad argument");
  if (Check e = at_entry(); e.done()) return e;
  if (ws->device != t->device) return refuse(TFRA_ERR_INVALID, "workspace and table live on different devices");
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16");
  if (dim % 4 != 0 || dim > 256) return refuse(TFRA_ERR_UNSUPPORTED, NEEDS_DIM);
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
                                const float* out, AtEntry&& at_entry) {
  if (!t) return refuse(TFRA_ERR_INVALID, "null table");
  if (combiner < 0 || combiner > 2) return refuse(TFRA_ERR_INVALID, "bad argument");
  if (flags & ~(TFRA_RAGGED_PRUNE | TFRA_RAGGED_FILL)) return refuse(TFRA_ERR_INVALID, "unknown flag bits (TFRA_RAGGED_PRUNE | TFRA_RAGGED_FILL)");
  if (reserved) return refuse(TFRA_ERR_INVALID, "reserved must be 0");
  if (Check e = at_entry(); e.done()) return e;
  if (ws && ws->device != t->device) return refuse(TFRA_ERR_INVALID, "workspace and table live on different devices");
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) return refuse(TFRA_ERR_UNSUPPORTED, "value_dtype must be float32, float16 or bfloat16");
  if (dim % 4 != 0 || dim > 256) return refuse(TFRA_ERR_UNSUPPORTED, NEEDS_DIM);
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

}  // namespace
}  // namespace tfra
