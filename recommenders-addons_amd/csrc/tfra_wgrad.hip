// The gradient of the pooled lookup with respect to its WEIGHTS, straight from the table (tfra_table_find_combine_backprop_weights
// and its ragged form).  The reference gets it from TensorFlow's autodiff of `embeddings *= weights`, segment_sum and the divide
// (PY/dynamic_embedding_ops.py:233-291), which needs the [nnz, dim] rows the pooled lookup was built to avoid.  Here the launch has
// the forward's shape (find_combine_row, tfra_pool.hip): one 16-lane group per OUTPUT ROW, one probe and one row read per entry, the
// row's incoming gradient held in registers where the forward holds its accumulator, and [nnz] floats out.
// The arithmetic and its ONE evaluation order are tfra_combine_device.h's (wgrad_dot4, wgrad_reduce16, wgrad_s, wgrad_finish), the
// code seg_combine_wgrad_kernel (tfra_combine.hip: rows from a [U, dim] tensor) compiles, so the two routes agree bit for bit.
// The argument checks and the launch ladders are the forward's (tfra_pool.h).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"

using namespace tfra;

namespace {

// The row r of this lane's group: its entries [b, e) are taken 16 at a time — lane j loads id and weight of entry p0 + j and hashes
// it, the next 16 loading behind this batch — and of those U at a time: U key lines in flight before any is inspected, then the U
// rows (t[NCH][U], the forward's big array) before any is used.  g[NCH] holds this lane's columns of grad_out[r, :], loaded once.
// Per entry: the lane's products, the group's reduction, s += w * d for a member; lane j keeps the raw d of entry p0 + j and the
// group stores the batch's 16 values in one coalesced store (0 for an entry that is no member).
// mean / sqrtn need s over the WHOLE row: the same group makes a second pass over its own [b, e) of dw — no rows, no probes — in
// which lane j re-reads exactly the values lane j wrote (entry b + 16 k + j both times), so program order suffices: no fence.
// Loads stay unconditional as in find_combine_row: entries past the row's end are clamped to its last entry (probed and read again,
// not used), columns past dim to column 0 (read, not added).  The probe is probe_find_word with plain loads.
// Compile-time axes beside (DT, U, NCH):
//   RAGGED  [b, e) from int64 row_splits clamped to 0 <= b <= e <= nnz, instead of the start_end ints of the bounds launch;
//   PRUNE   (with weights) an entry whose weight is not > 0 is no member: 0 out, and neither in s nor in wsum.
// An entry in no row is never visited: the memset before the launch is its 0.  (TFRA_RAGGED_FILL needs no code: a row without
// members has only pruned entries.)
template <int DT, int U, int NCH, bool RAGGED, bool PRUNE>
__device__ __forceinline__ void wgrad_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                          const float* __restrict__ w, const int* __restrict__ start_end,
                                          const i64* __restrict__ row_splits, int nnz, int combiner,
                                          const unsigned char* __restrict__ default_row, const float* __restrict__ grad_out,
                                          float* dw, size_t r) {
  static_assert(U == 4, "keep_live is written for U == 4");
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  if (r >= n_rows) return;
  int b, e;
  if constexpr (RAGGED) {
    const i64 lo = row_splits[r], hi = row_splits[r + 1];
    b = (int)min(max(lo, (i64)0), (i64)nnz);
    e = (int)min(max(hi, (i64)b), (i64)nnz);
  } else {
    b = start_end[r];
    e = start_end[n_rows + r];
  }
  if (b >= e) return;
  float wsum;
  if constexpr (PRUNE) wsum = combiner == 0 ? 0.f : comb_wsum_pruned(w, b, e, combiner);
  else wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  unsigned coff[NCH];   // this lane's byte offset inside a row, per chunk
  bool cok[NCH];
  float4 g[NCH];
  const float* G = grad_out + r * (size_t)dim;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 64 + sub * 4;
    cok[c] = col < dim;
    coff[c] = cok[c] ? (unsigned)col * EB : 0u;
    g[c] = *reinterpret_cast<const float4*>(G + (cok[c] ? col : 0));
  }
  float s = 0.f;
  const int last = e - 1;
  i64 knext = ids[min(b + sub, last)];
  float wnext = w ? w[min(b + sub, last)] : 1.f;
  for (int p0 = b; p0 < e; p0 += 16) {
    const i64 kreg = knext;
    const float wreg = wnext;
    if (p0 + 16 < e) {   // the next 16 entries, in flight behind this batch's probes and rows
      const int pn = min(p0 + 16 + sub, last);
      knext = ids[pn];
      wnext = w ? w[pn] : 1.f;
    }
    u64 hreg;
    const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
    const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
    float dmine = 0.f;   // the raw d of entry p0 + sub
    for (int q = 0; q < 16 && p0 + q < e; q += U) {
      i64 key[U], k0[U];
      unsigned b0[U], b1[U];
      float x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = gshift + q + u;
        key[u] = shfl_i64(kreg, j);
        b0[u] = (unsigned)__shfl((int)b0reg, j);
        b1[u] = (unsigned)__shfl((int)b1reg, j);
        x[u] = __shfl(wreg, j);
        k0[u] = key_line(v, b0[u])[sub];   // U probes in flight
      }
      keep_live(k0[0], k0[1], k0[2], k0[3]);
      const unsigned char* src[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const i64 word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift);
        src[u] = word >= 0 ? word_row_ptr(v, (u64)word) : default_row;
      }
      Raw t[NCH][U];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int u = 0; u < U; ++u) t[c][u] = *reinterpret_cast<const Raw*>(src[u] + coff[c]);   // U rows in flight
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) keep_live(t[c][0], t[c][1], t[c][2], t[c][3]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
          if (cok[c]) wgrad_dot4(d, g[c], PoolRow<DT>::widen(t[c][u]));
        d = wgrad_reduce16(d);
        bool member = p0 + q + u < e;
        if constexpr (PRUNE) member = member && x[u] > 0.f;
        if (member) wgrad_s(s, x[u], d);
        if (sub == q + u) dmine = member ? d : 0.f;
      }
    }
    if (p0 + sub < e) dw[p0 + sub] = dmine;   // one coalesced store per batch
  }
  if (combiner == 0) return;
  for (int p = b + sub; p < e; p += 16) {   // lane j re-reads what lane j wrote
    const float x = w ? w[p] : 1.f;
    const float d = dw[p];
    bool member = true;
    if constexpr (PRUNE) member = x > 0.f;
    dw[p] = member ? wgrad_finish(d, x, s, wsum, combiner) : 0.f;
  }
}

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void wgrad_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                    const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                    const unsigned char* __restrict__ default_row,
                                                    const float* __restrict__ grad_out, float* dw) {
  wgrad_row<DT, U, NCH, false, false>(v, n_rows, dim, ids, w, start_end, nullptr, 0, combiner, default_row, grad_out, dw,
                                      ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

template <int DT, int U, int NCH, bool PRUNE>
__global__ __launch_bounds__(256) void wgrad_ragged_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                           const float* __restrict__ w, const i64* __restrict__ row_splits, int nnz,
                                                           int combiner, const unsigned char* __restrict__ default_row,
                                                           const float* __restrict__ grad_out, float* dw) {
  wgrad_row<DT, U, NCH, true, PRUNE>(v, n_rows, dim, ids, w, nullptr, row_splits, nnz, combiner, default_row, grad_out, dw,
                                     ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

// what only these calls can get wrong, behind the forward's checks: dw_out
Check check_dw_out(size_t nnz, const float* dw_out) {
  if (nnz && !dw_out) return refuse(TFRA_ERR_INVALID, "null dw_out");
  if ((uintptr_t)dw_out & 3) return refuse(TFRA_ERR_UNSUPPORTED, "misaligned dw_out (4 bytes)");
  return Check{};
}

}  // namespace

extern "C" int tfra_table_find_combine_backprop_weights(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids,
                                                        const int64_t* seg, const float* weights, int combiner, size_t n_rows,
                                                        const void* default_row, const float* grad_out, float* dw_out,
                                                        tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine(t, ws, nnz, ids, seg, weights, combiner, n_rows, default_row, grad_out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report("find_combine_backprop_weights (out = grad_out): ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report("find_combine_backprop_weights: ", d);
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries in no row: 0
  if (!c.active) return TFRA_OK;                                // (no rows)
  const int dim = t->opts.dim;
  int rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  with_pool_class(st_index(t->opts.value_dtype), nch_index(dim), [&](auto DT, auto U, auto NCH) {
    wgrad_kernel<DT, U, NCH><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, se, combiner,
                                                        (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

extern "C" int tfra_table_find_combine_ragged_backprop_weights(tfra_table_t* tp, size_t n_rows, const int64_t* row_splits, size_t nnz,
                                                               const int64_t* ids, const float* weights, int combiner,
                                                               uint32_t flags, int64_t fill_id, const void* default_row,
                                                               const float* grad_out, float* dw_out, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  hipStream_t s = (hipStream_t)stream;
  std::unique_lock<std::mutex> lock;
  Check c = check_find_combine_ragged(t, nullptr, n_rows, row_splits, nnz, ids, weights, combiner, flags, 0, default_row, grad_out, [&] {
    lock = std::unique_lock<std::mutex>(t->mu);
    return Check{t->enter(s)};
  });
  if (c.msg == NEEDS_DIM) c.msg += " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)";
  if (c.code) return report("find_combine_ragged_backprop_weights (out = grad_out): ", c);
  if (Check d = check_dw_out(nnz, dw_out); d.code) return report("find_combine_ragged_backprop_weights: ", d);
  (void)fill_id;   // a row that takes the fill row has no members: its entries are 0 whatever fill_id holds
  if (nnz == 0) return TFRA_OK;
  HIP_TRY(hipMemsetAsync(dw_out, 0, nnz * sizeof(float), s));   // entries outside the clamped cover: 0
  if (!c.active) return TFRA_OK;                                // (no rows)
  const int dim = t->opts.dim;
  const TableView v = t->view_of(t->cur);
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  // the ladder's fourth axis is PRUNE here: FILL changes nothing, and PRUNE without weights neither
  with_ragged_class(st_index(t->opts.value_dtype), nch_index(dim), (flags & TFRA_RAGGED_PRUNE) && weights,
                    [&](auto DT, auto U, auto NCH, auto PRUNE) {
    wgrad_ragged_kernel<DT, U, NCH, PRUNE><<<grid, 256, 0, s>>>(v, n_rows, dim, (const i64*)ids, weights, (const i64*)row_splits, (int)nnz,
                                                                    combiner, (const unsigned char*)default_row, grad_out, dw_out);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
