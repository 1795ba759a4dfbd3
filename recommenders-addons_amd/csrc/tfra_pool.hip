// Pooled lookup: the forward of embedding_lookup_sparse / safe_embedding_lookup_sparse straight from the table
// (tfra_table_find_combine).  The reference runs it as an op chain (PY/dynamic_embedding_ops.py:120-293):
//   tf.unique(ids)                                  :218-221   (a [U] tensor, idx[nnz], a host-visible count)
//   embedding_lookup(params, unique ids)            :223-231   (a [U, dim] tensor)
//   gather(idx) * weights, segment_sum, / sum w | / sqrt(sum w^2)   :233-291   (a [nnz, dim] tensor between them)
// A read needs no de-duplication (repeats of a hot id hit the cache), so here one 16-lane group per OUTPUT ROW walks the row's
// entries in input order, probes the table once per entry and accumulates w * row in registers: neither tensor exists and
// nothing is counted on the host.  The arithmetic is tfra_combine_device.h's, the code seg_combine_kernel (tfra_frontend.hip)
// compiles, in the same order, so the result equals tfra_table_find + tfra_sparse_segment_combine bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"

using namespace tfra;

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return set_error(_e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP,                \
                       std::string(#expr) + ": " + hipGetErrorString(_e));                    \
  } while (0)

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

// One 16-lane group per output row (find_wave's and seg_combine_kernel's mapping: 4 rows per wave64).  The row's entries [b, e)
// are taken 16 at a time — lane j of the group loads id and weight of entry p0 + j and hashes it, one instruction stream for 16
// keys, the next 16 loading while these are worked on — and of those U at a time: U key lines in flight before any is inspected,
// then the U rows (NCH column chunks of 64 floats each: lane `sub` holds columns 64 c + 4 sub .. + 3) before any is accumulated.
// Accumulation is strictly in entry order.  Loads stay unconditional, as in find_wave: entries past the row's end are clamped to
// its last entry (probed and read again, not accumulated), columns past dim to column 0.
// The probe is find_kernel's (probe_find_word: plain loads), so a lookup that runs beside a write-back sees what tfra_table_find sees.
// The body is one function with two callers — find_combine_kernel (one table per launch) and find_combine_many_kernel (a list of
// tables per launch) — so that both compile the same expressions: r is the output row of this lane's group in ITS table.
template <int DT, int U, int NCH>
__device__ __forceinline__ void find_combine_row(const TableView& v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                 const float* __restrict__ w, const int* __restrict__ start_end, int combiner,
                                                 const unsigned char* __restrict__ default_row, float* __restrict__ out, size_t r) {
  static_assert(U == 4, "keep_live is written for U == 4");
  typedef typename PoolRow<DT>::Raw Raw;
  constexpr unsigned EB = DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  if (r >= n_rows) return;
  const int b = start_end[r], e = start_end[n_rows + r];
  const float wsum = combiner == 0 ? 0.f : comb_wsum(w, b, e, combiner);
  const float scale = comb_scale_of(wsum, combiner);
  unsigned coff[NCH];   // this lane's byte offset inside a row, per chunk
  bool cok[NCH];
  float4 acc[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 64 + sub * 4;
    cok[c] = col < dim;
    coff[c] = cok[c] ? (unsigned)col * EB : 0u;
    acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (b < e) {
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
          if (p0 + q + u < e) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) comb_acc4(acc[c], PoolRow<DT>::widen(t[c][u]), x[u]);
          }
        }
      }
    }
  }
  float* o = out + r * (size_t)dim;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (cok[c]) *reinterpret_cast<float4*>(o + c * 64 + sub * 4) = comb_finish4(acc[c], wsum, scale, combiner);
}

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void find_combine_kernel(TableView v, size_t n_rows, int dim, const i64* __restrict__ ids,
                                                           const float* __restrict__ w, const int* __restrict__ start_end,
                                                           int combiner, const unsigned char* __restrict__ default_row,
                                                           float* __restrict__ out) {
  find_combine_row<DT, U, NCH>(v, n_rows, dim, ids, w, start_end, combiner, default_row, out,
                               ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4);
}

// ---- the grouped form (tfra_multi_find_combine): the lookups of a LIST of tables in one launch per (value dtype, NCH) class ------
// What a single-table launch takes as kernel arguments is a record in device memory here (26 tables' records do not fit the 4 KB
// of kernel arguments: a TableView alone is 80 B).  The grid is the concatenation of the class's descriptors, descriptor d owning
// the blocks [prefix[d], prefix[d + 1]) = ceil(n_rows * 16 / 256) blocks, so that a block never straddles two descriptors.
struct ManyRec {
  TableView v;
  size_t n_rows;
  const i64* ids;
  const float* w;
  const int* se;
  const unsigned char* default_row;
  float* out;
  int dim;
  int combiner;
};
// (BoundsRec, the record of the bounds launch, and many_desc_of, the search that takes a block to its descriptor: tfra_many.h)

template <int DT, int U, int NCH>
__global__ __launch_bounds__(256) void find_combine_many_kernel(const ManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                                unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const ManyRec rec = recs[d];
  find_combine_row<DT, U, NCH>(rec.v, rec.n_rows, rec.dim, rec.ids, rec.w, rec.se, rec.combiner, rec.default_row, rec.out,
                               ((size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x) >> 4);
}

// seg64_bounds_kernel (tfra_frontend.hip) over a list: descriptor d owns ceil(nnz / 256) blocks and p counts ITS entries, so the
// neighbours p - 1 / p + 1 are never read across a descriptor's end.  se zeroed before (empty rows: 0, 0).
__global__ __launch_bounds__(256) void seg64_bounds_many_kernel(const BoundsRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                                unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const BoundsRec rec = recs[d];
  const size_t p = (size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x;
  if (p >= rec.nnz) return;
  const i64 s = rec.seg[p];
  if (s < 0 || (size_t)s >= rec.n_rows) return;
  if (p == 0 || rec.seg[p - 1] != s) rec.se[s] = (int)p;
  if (p == rec.nnz - 1 || rec.seg[p + 1] != s) rec.se[rec.n_rows + s] = (int)p + 1;
}

template <int DT>
void launch_find_combine_many(hipStream_t s, int nch, unsigned grid, const ManyRec* recs, const unsigned* prefix, unsigned n) {
  constexpr int U = 4;
  if (nch == 0) find_combine_many_kernel<DT, U, 1><<<grid, 256, 0, s>>>(recs, prefix, n);
  else if (nch == 1) find_combine_many_kernel<DT, U, 2><<<grid, 256, 0, s>>>(recs, prefix, n);
  else find_combine_many_kernel<DT, U, 4><<<grid, 256, 0, s>>>(recs, prefix, n);
}

// (the records reach the device through the workspace's pinned staging ring: ManyStage, tfra_many.h)

// the single call's checks of one descriptor, in its order and with its codes; *active: the descriptor has rows to write
int check_desc(const tfra_find_combine_desc& d, const tfra_workspace* ws, bool* active, std::string* msg) {
  *active = false;
  if (d.struct_size != sizeof(tfra_find_combine_desc)) { *msg = "descriptor size mismatch"; return TFRA_ERR_INVALID; }
  const Table* t = reinterpret_cast<const Table*>(d.table);
  if (!t) { *msg = "null table"; return TFRA_ERR_INVALID; }
  if (d.combiner < 0 || d.combiner > 2) { *msg = "bad argument"; return TFRA_ERR_INVALID; }
  if (ws->device != t->device) { *msg = "workspace and table live on different devices"; return TFRA_ERR_INVALID; }
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16) { *msg = "value_dtype must be float32, float16 or bfloat16"; return TFRA_ERR_UNSUPPORTED; }
  if (dim % 4 != 0 || dim > 256) { *msg = "needs dim % 4 == 0 and dim <= 256"; return TFRA_ERR_UNSUPPORTED; }
  if (d.nnz >= (1ULL << 31) || d.n_rows >= (1ULL << 30)) { *msg = "too large (nnz < 2^31, n_rows < 2^30)"; return TFRA_ERR_UNSUPPORTED; }
  if ((((uintptr_t)d.out | (uintptr_t)d.default_row) & 15) || ((uintptr_t)d.ids & 7) || ((uintptr_t)d.seg & 7) || ((uintptr_t)d.weights & 3)) {
    *msg = "misaligned buffer (out and default_row: 16 bytes)";
    return TFRA_ERR_UNSUPPORTED;
  }
  if (d.n_rows == 0) return TFRA_OK;
  if (!d.out) { *msg = "null out"; return TFRA_ERR_INVALID; }
  if (d.nnz && (!d.ids || !d.seg || !d.default_row)) { *msg = "null buffer"; return TFRA_ERR_INVALID; }
  *active = true;
  return TFRA_OK;
}

template <int DT>
void launch_find_combine(hipStream_t s, const TableView& v, size_t n_rows, int dim, const i64* ids, const float* w, const int* se,
                         int combiner, const unsigned char* d, float* out) {
  constexpr int U = 4;
  const unsigned grid = (unsigned)((n_rows * 16 + 255) / 256);
  if (dim <= 64) find_combine_kernel<DT, U, 1><<<grid, 256, 0, s>>>(v, n_rows, dim, ids, w, se, combiner, d, out);
  else if (dim <= 128) find_combine_kernel<DT, U, 2><<<grid, 256, 0, s>>>(v, n_rows, dim, ids, w, se, combiner, d, out);
  else find_combine_kernel<DT, U, 4><<<grid, 256, 0, s>>>(v, n_rows, dim, ids, w, se, combiner, d, out);
}

}  // namespace

extern "C" int tfra_table_find_combine(tfra_table_t* tp, tfra_workspace_t* ws, size_t nnz, const int64_t* ids, const int64_t* seg,
                                       const float* weights, int combiner, size_t n_rows, const void* default_row, float* out,
                                       tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "find_combine: null table");
  if (!ws || combiner < 0 || combiner > 2) return set_error(TFRA_ERR_INVALID, "find_combine: bad argument");
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(t->mu);
  int rc = t->enter(s);
  if (rc) return rc;
  if (ws->device != t->device) return set_error(TFRA_ERR_INVALID, "find_combine: workspace and table live on different devices");
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: value_dtype must be float32, float16 or bfloat16");
  if (dim % 4 != 0 || dim > 256)
    return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: needs dim % 4 == 0 and dim <= 256 (use tfra_unique + tfra_table_find + "
                                           "tfra_sparse_segment_combine otherwise)");
  if (nnz >= (1ULL << 31) || n_rows >= (1ULL << 30)) return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: too large (nnz < 2^31, n_rows < 2^30)");
  if ((((uintptr_t)out | (uintptr_t)default_row) & 15) || ((uintptr_t)ids & 7) || ((uintptr_t)seg & 7) || ((uintptr_t)weights & 3))
    return set_error(TFRA_ERR_UNSUPPORTED, "find_combine: misaligned buffer (out and default_row: 16 bytes)");
  if (n_rows == 0) return TFRA_OK;
  if (!out) return set_error(TFRA_ERR_INVALID, "find_combine: null out");
  if (nnz == 0) {
    HIP_TRY(hipMemsetAsync(out, 0, n_rows * (size_t)dim * sizeof(float), s));
    return TFRA_OK;
  }
  if (!ids || !seg || !default_row) return set_error(TFRA_ERR_INVALID, "find_combine: null buffer");
  rc = ws->ensure((2 * n_rows * sizeof(int) + 255) / 256 * 256, s);
  if (rc) return rc;
  int* se = (int*)ws->buf;
  rc = comb_bounds(s, nnz, seg, n_rows, se);
  if (rc) return rc;
  const TableView v = t->view_of(t->cur);
  const i64* k = (const i64*)ids;
  const unsigned char* d = (const unsigned char*)default_row;
  if (dt == TFRA_F32) launch_find_combine<TFRA_F32>(s, v, n_rows, dim, k, weights, se, combiner, d, out);
  else if (dt == TFRA_F16) launch_find_combine<TFRA_F16>(s, v, n_rows, dim, k, weights, se, combiner, d, out);
  else launch_find_combine<TFRA_BF16>(s, v, n_rows, dim, k, weights, se, combiner, d, out);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

namespace tfra {
int comb_bounds_many(hipStream_t s, unsigned grid, const BoundsRec* recs, const unsigned* prefix, unsigned n) {
  seg64_bounds_many_kernel<<<grid, 256, 0, s>>>(recs, prefix, n);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

void destroy_workspace_many(void* p) {
  ManyStage* st = reinterpret_cast<ManyStage*>(p);
  if (!st) return;
  for (int i = 0; i < ManyStage::RING; ++i) {
    if (st->pending[i]) (void)hipEventSynchronize(st->ev[i]);
    if (st->ev[i]) (void)hipEventDestroy(st->ev[i]);
  }
  if (st->host) (void)hipHostFree(st->host);
  delete st;
}
}  // namespace tfra

extern "C" int tfra_multi_find_combine(tfra_workspace_t* ws, size_t n_tables, const tfra_find_combine_desc* descs,
                                       uint32_t* launches_out, tfra_stream_t stream) {
  if (launches_out) *launches_out = 0;
  if (n_tables == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, "multi_find_combine: null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and no out is written
  constexpr int NCLASS = 9;   // (float32 | float16 | bfloat16) x (NCH 1 | 2 | 4)
  std::vector<int> cls(n_tables, -1);
  size_t n_act = 0, n_bnd = 0, total_rows = 0;
  for (size_t i = 0; i < n_tables; ++i) {
    bool active = false;
    std::string msg;
    const int rc = check_desc(descs[i], ws, &active, &msg);
    if (rc) return set_error(rc, "multi_find_combine: descriptor " + std::to_string(i) + ": " + msg);
    if (!active) continue;
    const Table* t = reinterpret_cast<const Table*>(descs[i].table);
    const int dt = t->opts.value_dtype, dim = t->opts.dim;
    cls[i] = (dt == TFRA_F32 ? 0 : dt == TFRA_F16 ? 1 : 2) * 3 + (dim <= 64 ? 0 : dim <= 128 ? 1 : 2);
    ++n_act;
    n_bnd += descs[i].nnz ? 1 : 0;
    total_rows += descs[i].n_rows;
  }
  if (n_act == 0) return TFRA_OK;
  // the records' order: class by class, input order inside a class
  std::vector<size_t> order;
  order.reserve(n_act);
  size_t cls_first[NCLASS + 1];
  u64 cls_blocks[NCLASS], bnd_blocks = 0;
  for (int c = 0; c < NCLASS; ++c) {
    cls_first[c] = order.size();
    cls_blocks[c] = 0;
    for (size_t i = 0; i < n_tables; ++i)
      if (cls[i] == c) { order.push_back(i); cls_blocks[c] += (descs[i].n_rows * 16 + 255) / 256; }
    if (cls_blocks[c] >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, "multi_find_combine: too many rows in one call");
  }
  cls_first[NCLASS] = order.size();
  for (size_t i = 0; i < n_tables; ++i)
    if (cls[i] >= 0) bnd_blocks += (descs[i].nnz + 255) / 256;
  if (bnd_blocks >= (1ULL << 31)) return set_error(TFRA_ERR_UNSUPPORTED, "multi_find_combine: too many entries in one call");

  // each distinct table locked once, in one global order (by address): two threads with overlapping lists cannot deadlock
  std::vector<Table*> tabs;
  tabs.reserve(n_act);
  for (size_t i : order) tabs.push_back(reinterpret_cast<Table*>(descs[i].table));
  std::sort(tabs.begin(), tabs.end(), std::less<Table*>());
  tabs.erase(std::unique(tabs.begin(), tabs.end()), tabs.end());
  std::vector<std::unique_lock<std::mutex>> locks;
  locks.reserve(tabs.size());
  for (Table* t : tabs) locks.emplace_back(t->mu);
  for (Table* t : tabs) {
    const int rc = t->enter(s);
    if (rc) return rc;
  }

  // device memory: [bounds of all rows | records | per-class block prefixes | bounds records | their block prefix]
  const size_t se_bytes = (2 * total_rows * sizeof(int) + 255) / 256 * 256;
  const size_t rec_off = 0, cpre_off = (n_act * sizeof(ManyRec) + 15) / 16 * 16;
  const size_t brec_off = (cpre_off + (n_act + NCLASS) * sizeof(unsigned) + 15) / 16 * 16;
  const size_t bpre_off = brec_off + n_bnd * sizeof(BoundsRec);
  const size_t blob_bytes = (bpre_off + (n_bnd + 1) * sizeof(unsigned) + 255) / 256 * 256;
  int rc = ws->ensure(se_bytes + blob_bytes, s);
  if (rc) return rc;
  ManyStage* stage = many_stage_of(ws);
  unsigned char* h = nullptr;
  int slot = 0;
  rc = stage->take(blob_bytes, &h, &slot);
  if (rc) return rc;
  int* se_base = (int*)ws->buf;
  unsigned char* d_blob = (unsigned char*)ws->buf + se_bytes;
  ManyRec* recs = reinterpret_cast<ManyRec*>(h + rec_off);
  unsigned* cpre = reinterpret_cast<unsigned*>(h + cpre_off);
  BoundsRec* brecs = reinterpret_cast<BoundsRec*>(h + brec_off);
  unsigned* bpre = reinterpret_cast<unsigned*>(h + bpre_off);
  // the views are taken here, under the locks: a table that grew since the last call has another one
  std::vector<size_t> se_off(n_tables, 0);
  {
    size_t off = 0;
    for (size_t i = 0; i < n_tables; ++i)
      if (cls[i] >= 0) { se_off[i] = off; off += 2 * descs[i].n_rows; }
  }
  size_t cpre_at[NCLASS];
  {
    size_t k = 0, pre = 0;
    for (int c = 0; c < NCLASS; ++c) {
      cpre_at[c] = pre;
      if (cls_first[c] == cls_first[c + 1]) continue;
      unsigned blocks = 0;
      for (size_t j = cls_first[c]; j < cls_first[c + 1]; ++j, ++k) {
        const tfra_find_combine_desc& d = descs[order[j]];
        Table* t = reinterpret_cast<Table*>(d.table);
        ManyRec& r = recs[k];
        r.v = t->view_of(t->cur);
        r.n_rows = d.n_rows;
        r.ids = (const i64*)d.ids;
        r.w = d.weights;
        r.se = se_base + se_off[order[j]];
        r.default_row = (const unsigned char*)d.default_row;
        r.out = d.out;
        r.dim = t->opts.dim;
        r.combiner = d.combiner;
        cpre[pre++] = blocks;
        blocks += (unsigned)((d.n_rows * 16 + 255) / 256);
      }
      cpre[pre++] = blocks;
    }
  }
  {
    size_t k = 0;
    unsigned blocks = 0;
    for (size_t i = 0; i < n_tables; ++i) {
      if (cls[i] < 0 || descs[i].nnz == 0) continue;
      brecs[k].seg = (const i64*)descs[i].seg;
      brecs[k].se = se_base + se_off[i];
      brecs[k].nnz = descs[i].nnz;
      brecs[k].n_rows = descs[i].n_rows;
      bpre[k++] = blocks;
      blocks += (unsigned)((descs[i].nnz + 255) / 256);
    }
    bpre[k] = blocks;
  }
  HIP_TRY(hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s));
  rc = stage->sent(slot, s);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(se_base, 0, 2 * total_rows * sizeof(int), s));   // empty rows (and every row of an nnz == 0 descriptor): 0, 0
  uint32_t launches = 0;
  if (n_bnd) {
    seg64_bounds_many_kernel<<<(unsigned)bnd_blocks, 256, 0, s>>>(reinterpret_cast<const BoundsRec*>(d_blob + brec_off),
                                                                  reinterpret_cast<const unsigned*>(d_blob + bpre_off), (unsigned)n_bnd);
    ++launches;
  }
  for (int c = 0; c < NCLASS; ++c) {
    const unsigned n = (unsigned)(cls_first[c + 1] - cls_first[c]);
    if (!n) continue;
    const ManyRec* r = reinterpret_cast<const ManyRec*>(d_blob + rec_off) + cls_first[c];
    const unsigned* p = reinterpret_cast<const unsigned*>(d_blob + cpre_off) + cpre_at[c];
    const unsigned grid = (unsigned)cls_blocks[c];
    if (c / 3 == 0) launch_find_combine_many<TFRA_F32>(s, c % 3, grid, r, p, n);
    else if (c / 3 == 1) launch_find_combine_many<TFRA_F16>(s, c % 3, grid, r, p, n);
    else launch_find_combine_many<TFRA_BF16>(s, c % 3, grid, r, p, n);
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}
