// tfra_table_find_typed: tfra_table_find / tfra_table_find_n with the rows written in another type than the table stores — a
// float32 master table read out as bfloat16 / float16 activations, a half table read out as float32.  The result is
// the twin's followed by the elementwise conversion, bit for bit, and the torch conversion pass behind the lookup is gone: the
// [n, dim] matrix is written once, in the type its reader wants.
// The kernel is find_wave's shape (tfra_device.h) with the copy loop converting: 16 lanes per key, U = 4 keys per group, one lane
// per key for the hash, unconditional loads with the tail clamped, the probe of find_kernel (probe_find_word: plain loads).  It is
// a kernel of its own and not one more axis of find_wave: seven kernels share that function, and none of them may move.
// The up-cast and the rounding are PoolRow / PoolOut (tfra_pool.h), the ones the pooled lookups' typed forms use.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_pool.h"

using namespace tfra;

namespace {

// One wave serves 16 keys (4 per 16-lane group).  A lane's granule is FOUR ELEMENTS, whatever the two types are: lane `sub` reads
// columns 64 c + 4 sub .. + 3 of the stored row (16 B of a float32 row, 8 B of a half row), widens them to float32, narrows them to
// OUT_DT and stores 16 B or 8 B — the U rows of a group in flight before the first is converted.  dim % 4 == 0 (the host checks).
template <int IN_DT, int OUT_DT, bool PF1>
__global__ __launch_bounds__(256) void find_cast_kernel(TableView v, size_t n, int dim, const i64* __restrict__ keys,
                                                        unsigned char* __restrict__ out, uint8_t* __restrict__ exists,
                                                        const unsigned char* __restrict__ defaults, int full,
                                                        const long long* __restrict__ d_n) {
  static_assert(IN_DT != OUT_DT, "the same type on both sides is tfra_table_find");
  constexpr int U = 4;
  typedef typename PoolRow<IN_DT>::Raw Raw;
  typedef typename PoolOut<OUT_DT>::Vec Vec;
  constexpr unsigned EI = IN_DT == TFRA_F32 ? 4u : 2u, EO = OUT_DT == TFRA_F32 ? 4u : 2u;   // bytes per element
  if (d_n) {   // uniform load, as find_kernel's: the key count lives on the device (n = the buffers' length)
    const long long dn = *d_n;
    n = dn < 0 ? 0 : min(n, (size_t)dn);
  }
  const unsigned wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const int grp = lane >> 4;
  constexpr int KPW = 4 * U;
  const unsigned base = wave * KPW;   // n < 2^32 (the host checks)
  if (base >= n) return;
  const unsigned last = (unsigned)n - 1;
  const i64 kreg = keys[min(base + (unsigned)(lane & (KPW - 1)), last)];   // one lane per key for the hash (find_wave)
  u64 hreg;
  const unsigned b0reg = (unsigned)bucket0(kreg, v.nb, hreg);
  const unsigned b1reg = (unsigned)bucket1(hreg, b0reg, v.nb);
  i64 key[U];
  unsigned b0[U], b1[U], idx[U];
  i64 k0[U], k1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * 4 + grp;
    key[u] = shfl_i64(kreg, j);
    b0[u] = (unsigned)__shfl((int)b0reg, j);
    b1[u] = (unsigned)__shfl((int)b1reg, j);
    idx[u] = min(base + (unsigned)j, last);
    k0[u] = key_line(v, b0[u])[sub];  // U probes in flight
    k1[u] = PF1 ? key_line(v, b1[u])[sub] : 0;
  }
  keep_live(k0[0], k0[1], k0[2], k0[3]);
  if (PF1) keep_live(k1[0], k1[1], k1[2], k1[3]);
  const unsigned char* src[U];
  unsigned char* dst[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const i64 word = probe_find_word(v, key[u], b0[u], b1[u], k0[u], sub, gshift, PF1 ? &k1[u] : nullptr);
    if (exists && sub == 0) exists[idx[u]] = word >= 0;
    src[u] = word >= 0 ? word_row_ptr(v, (u64)word) : defaults + (full ? (u64)idx[u] * (u64)v.field_bytes : 0);
    dst[u] = out + (u64)idx[u] * (u64)((unsigned)dim * EO);
  }
  for (unsigned col = sub * 4; col < (unsigned)dim; col += 64) {
    Raw tmp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) tmp[u] = *reinterpret_cast<const Raw*>(src[u] + col * EI);  // U rows in flight
    keep_live(tmp[0], tmp[1], tmp[2], tmp[3]);
#pragma unroll
    for (int u = 0; u < U; ++u) {  // clamped tail: same bytes twice
      Vec x = PoolOut<OUT_DT>::narrow(PoolRow<IN_DT>::widen(tmp[u]));
      if constexpr (OUT_DT == TFRA_F32) store_wt16(dst[u] + col * EO, *reinterpret_cast<uint4*>(&x));   // find_kernel's write-through
      else *reinterpret_cast<Vec*>(dst[u] + col * EO) = x;
    }
  }
}

// launch(IN_DT, OUT_DT) for two different storage type indices (st_index)
template <class F>
void with_cast_pair(int in, int out, F&& launch) {
  with_stored(in, [&](auto IN) {
    with_stored(out, [&](auto OUT) {
      if constexpr (decltype(IN)::value != decltype(OUT)::value) launch(IN, OUT);
    });
  });
}

}  // namespace

extern "C" int tfra_table_find_typed(tfra_table_t* tp, size_t n, const int64_t* d_n, const int64_t* keys, const tfra_rows_out* out,
                                     uint8_t* exists, const void* defaults, int default_is_full, tfra_stream_t stream) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t) return set_error(TFRA_ERR_INVALID, "null table");
  if (Check c = check_rows_out(out); c.code) return report("find_typed: ", c);
  if (out->dtype == t->opts.value_dtype)   // the table's own type: the untyped call, its code and its launches
    return d_n ? tfra_table_find_n(tp, n, d_n, keys, out->rows, exists, defaults, default_is_full, stream)
               : tfra_table_find(tp, n, keys, out->rows, exists, defaults, default_is_full, stream);
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(t->mu);
  if (int rc = t->enter(s)) return rc;
  const int dt = t->opts.value_dtype, dim = t->opts.dim;
  if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
    return set_error(TFRA_ERR_UNSUPPORTED, "find_typed: value_dtype must be float32, float16 or bfloat16");
  if (dim % 4 != 0 || dim > 256) return set_error(TFRA_ERR_UNSUPPORTED, std::string("find_typed: ") + NEEDS_DIM);
  if (n == 0) return TFRA_OK;
  if (!keys || !out->rows || !defaults) return set_error(TFRA_ERR_INVALID, "find_typed: null buffer");
  if (n >= (1ULL << 32)) return set_error(TFRA_ERR_INVALID, "find_typed: more than 2^32-1 keys per call");
  if ((uintptr_t)defaults & (dt == TFRA_F32 ? 15 : 7))
    return set_error(TFRA_ERR_UNSUPPORTED, "find_typed: misaligned defaults (float32 tables: 16 bytes, half tables: 8)");
  const TableView v = t->view_of(t->cur);
  const size_t waves = (n + 15) / 16;
  const unsigned grid = (unsigned)((waves + 3) / 4);
  const bool pf1 = t->dense;   // find_impl's rule: a dense table puts both home-bucket lines of a key in flight together
  with_cast_pair(st_index(dt), st_index(out->dtype), [&](auto IN, auto OUT) {
    if (pf1)
      find_cast_kernel<IN, OUT, true><<<grid, 256, 0, s>>>(v, n, dim, (const i64*)keys, (unsigned char*)out->rows, exists,
                                                             (const unsigned char*)defaults, default_is_full, (const long long*)d_n);
    else
      find_cast_kernel<IN, OUT, false><<<grid, 256, 0, s>>>(v, n, dim, (const i64*)keys, (unsigned char*)out->rows, exists,
                                                              (const unsigned char*)defaults, default_is_full, (const long long*)d_n);
  });
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}
