// The grouped de-duplication: tfra_multi_unique, the tfra_unique (tfra_unique.hip) of a LIST of id lists as ONE
// stream-ordered chain: one record upload, one insert launch over all lists' ids, one scatter launch over all lists' tiles, one
// index launch for the lists that want their inverse index — 3 launches, or 2, however long the list is.
// The kernels are the grouped twins of unq2_insert_kernel, unq2_scatter_kernel and unq_idx_kernel and share their helpers
// (tfra_unique_device.h).  They have the launch shape of the grouped calls (tfra_many.h): many_desc_of takes the block to its
// descriptor, the record is read with wave-uniform loads, and the body runs on a block index local to the list.
// State: two persistent, self-emptying sets of the call's own in the workspace (tfra_host.h: unqm_*), apart from tfra_unique's.
// A set is one range of slots; every list of a call takes a SUB-SET of it: a power of two of at least 2 n slots and one side slot
// behind them for EMPTY_KEY as an id, so lists never meet in a slot.  The used list records ABSOLUTE slots of the set: the next
// call, whose lists and sub-sets differ, empties the other set without knowing the layout that filled it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_frontend.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_unique_device.h"

using namespace tfra;

namespace {

constexpr size_t UNQM_MAX_LIST = (size_t)1 << 20;    // tfra_unique's three-launch bound
constexpr size_t UNQM_MAX_TOTAL = (size_t)1 << 22;

// One list with n > 0.  A position i of the list is i everywhere (hfirst, hrank, idx_out) but in slot_of, where the call's lists
// stand one behind the other: base + i.
struct UnqManyRec {
  const i64* ids;
  i64* unique_out;
  int* idx_out;       // may be null
  i64* total_out;
  unsigned n;
  unsigned base;      // the list's first position in slot_of
  unsigned set_off;   // the sub-set's first slot
  unsigned cap;       // its slots, a power of two >= 2 n; its side slot is set_off + cap
};

__global__ void unqm_fill_kernel(i64* hkeys0, int* hfirst0, i64* hkeys1, int* hfirst1, size_t slots) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (size_t)gridDim.x * blockDim.x) {
    hkeys0[i] = EMPTY_KEY; hfirst0[i] = 0x7fffffff;
    hkeys1[i] = EMPTY_KEY; hfirst1[i] = 0x7fffffff;
  }
}

// unq2_insert_kernel per list: a list owns ceil(n / UNQ_INS) blocks.  The emptying of the other set runs over the whole grid.
__global__ __launch_bounds__(UNQ_INS) void unqm_insert_kernel(const UnqManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                              unsigned n_lists, UnqSet cur, UnqSet old, int* slot_of) {
  __shared__ i64 l_id[UNQ_INS];
  __shared__ unsigned l_own[UNQ_LCAP];
  __shared__ int l_first[UNQ_LCAP];
  __shared__ int l_slot[UNQ_LCAP];
  __shared__ unsigned s_n, s_base;
  const int t = threadIdx.x;
  const unsigned d = many_desc_of(prefix, n_lists, blockIdx.x);
  const UnqManyRec r = recs[d];
  const size_t i = (size_t)(blockIdx.x - prefix[d]) * UNQ_INS + t;
  const unsigned n_old = *old.nused;
  const bool ok = i < r.n;
  const i64 id = ok ? r.ids[i] : 0;
  const unsigned h = unq_group_in_block(t, ok, id, l_id, l_own, l_first, &s_n);
  bool mine = false;
  unsigned myslot = 0, myidx = 0;
  if (ok && l_first[h] == t) {  // first position of its id in this block
    size_t sl;
    if (id == EMPTY_KEY) {
      sl = (size_t)r.set_off + r.cap;  // the list's side slot for the sentinel value itself
      mine = atomicMin(&cur.hfirst[sl], (int)i) == 0x7fffffff;
    } else {
      unsigned p = (unsigned)fmix64((u64)id) & (r.cap - 1);
      for (;;) {
        const i64 was = (i64)atomicCAS((u64*)&cur.hkeys[(size_t)r.set_off + p], (u64)EMPTY_KEY, (u64)id);
        if (was == EMPTY_KEY) { mine = true; break; }
        if (was == id) break;
        p = (p + 1) & (r.cap - 1);
      }
      sl = (size_t)r.set_off + p;
      atomicMin(&cur.hfirst[sl], (int)i);
    }
    l_slot[h] = (int)sl;
    myslot = (unsigned)sl;
    if (mine) myidx = atomicAdd(&s_n, 1u);
  }
  __syncthreads();
  if (ok) slot_of[(size_t)r.base + i] = l_slot[h];
  if (t == 0) s_base = s_n ? atomicAdd(cur.nused, s_n) : 0u;
  __syncthreads();
  if (mine) cur.used[s_base + myidx] = myslot;
  // the other set: empty the slots its last call used, whichever lists they belonged to
  for (size_t k = (size_t)blockIdx.x * UNQ_INS + t; k < n_old; k += (size_t)gridDim.x * UNQ_INS) {
    const unsigned sl = old.used[k];
    old.hkeys[sl] = EMPTY_KEY;
    old.hfirst[sl] = 0x7fffffff;
  }
}

// unq2_scatter_kernel per list: a list owns ceil(n / UNQ_TILE) tiles.  agg has a word per tile of the GRID; the look-back of a
// list's tile j reads the list's tiles [0, j) only, which have lower block indices in the grid — unq2_scatter_kernel's argument
// (blocks are dispatched in index order: what a waiting tile needs is resident or finished) holds unchanged.  The list's last
// tile writes its count; the counts of the call's lists with n == 0 (zero[0 .. n_zero)) are written here too.
__global__ __launch_bounds__(256) void unqm_scatter_kernel(const UnqManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                           unsigned n_lists, UnqSet cur, UnqSet old, const int* __restrict__ slot_of,
                                                           unsigned long long* agg, unsigned gen, i64* const* __restrict__ zero,
                                                           unsigned n_zero) {
  __shared__ int wsum[4];
  __shared__ int s_off;
  const unsigned d = many_desc_of(prefix, n_lists, blockIdx.x);
  const UnqManyRec r = recs[d];
  const unsigned first = prefix[d], j = blockIdx.x - first;   // the list's first tile, this tile's index in the list
  const int* __restrict__ slot_l = slot_of + r.base;
  const size_t base = (size_t)j * UNQ_TILE + threadIdx.x * UNQ_ITEMS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int flag[UNQ_ITEMS];
  const int excl = unq_flags_scan(r.n, base, cur.hfirst, slot_l, flag, wsum);
  const int tile_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (threadIdx.x == 0)   // publish this tile's count under the call's generation
    __hip_atomic_store(agg + blockIdx.x, ((unsigned long long)gen << 32) | (unsigned)tile_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // offset = counts of the list's earlier tiles, read as they appear (wave 0: 64 tiles per sweep)
  if (w == 0) {
    int sum = 0;
    for (unsigned j0 = 0; j0 < j; j0 += 64) {
      const unsigned jj = j0 + (unsigned)lane;
      if (jj < j) {
        unsigned long long v;
        do { v = __hip_atomic_load(agg + first + jj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((unsigned)(v >> 32) != gen);
        sum += (int)(unsigned)v;
      }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) s_off = sum;
  }
  __syncthreads();
  int pos = s_off + excl;
#pragma unroll
  for (int k = 0; k < UNQ_ITEMS; ++k) {
    if (flag[k]) {
      const size_t i = base + k;
      r.unique_out[pos] = r.ids[i];
      cur.hrank[slot_l[i]] = pos;
      ++pos;
    }
  }
  if (threadIdx.x == 0) {
    if (blockIdx.x + 1 == prefix[d + 1]) *r.total_out = (i64)(s_off + tile_total);
    if (blockIdx.x == gridDim.x - 1) *old.nused = 0;   // the other set is empty again (unqm_insert_kernel of this call emptied it)
  }
  for (unsigned k = blockIdx.x * 256 + threadIdx.x; k < n_zero; k += gridDim.x * 256) *zero[k] = 0;
}

// unq_idx_kernel per list that wants its inverse index: ceil(n / 256) blocks each
__global__ __launch_bounds__(256) void unqm_idx_kernel(const UnqManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                       const unsigned* __restrict__ idx, unsigned n_lists, const int* __restrict__ slot_of,
                                                       const int* __restrict__ hrank) {
  const unsigned d = many_desc_of(prefix, n_lists, blockIdx.x);
  const UnqManyRec& r = recs[idx[d]];
  const size_t i = (size_t)(blockIdx.x - prefix[d]) * 256 + threadIdx.x;
  if (i < r.n) r.idx_out[i] = hrank[slot_of[(size_t)r.base + i]];
}

// a call whose lists are all empty: their counts
__global__ void unqm_zero_kernel(i64* const* __restrict__ zero, unsigned n_zero) {
  for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < n_zero; k += gridDim.x * blockDim.x) *zero[k] = 0;
}

// the persistent buffer: [256 B: the two sets' nused] [set 0] [set 1] [slot_of: nmax ints] [agg: a word per tile];
// a set: hkeys | hfirst | hrank (slots each) | used (nmax)
struct UnqManyLayout {
  size_t hfirst, hrank, used, per, slot_of, agg, bytes;
  UnqManyLayout(size_t slots, size_t nmax, size_t tiles) {
    hfirst = align_up(slots * 8);
    hrank = hfirst + align_up(slots * 4);
    used = hrank + align_up(slots * 4);
    per = used + align_up(nmax * 4);
    slot_of = 256 + 2 * per;
    agg = slot_of + align_up(nmax * 4);
    bytes = agg + align_up(tiles * 8);
  }
  UnqSet set_of(void* buf, unsigned p) const {
    unsigned char* w = (unsigned char*)buf + 256 + (size_t)p * per;
    return UnqSet{(i64*)w, (int*)(w + hfirst), (int*)(w + hrank), (unsigned*)(w + used), (unsigned*)buf + p};
  }
};

// Room for `total` ids in `slots` slots per set and `tiles` scatter tiles; a buffer that is too small in any of the three is
// replaced (behind the stream, as unique_fast's) by one that is at least as large in all of them.
int ensure_sets(tfra_workspace* ws, size_t total, size_t slots, size_t tiles, hipStream_t s) {
  if (ws->unqm_buf && total <= ws->unqm_nmax && slots <= ws->unqm_slots && tiles <= ws->unqm_tiles) return TFRA_OK;
  if (ws->unqm_buf) {
    // (the last call may have run on another stream: it still uses the buffer)
    if (ws->unqm_stream_set && ws->unqm_stream != s && hipStreamSynchronize(ws->unqm_stream) != hipSuccess)
      return set_error(TFRA_ERR_HIP, "multi_unique: free failed");
    if (hipStreamSynchronize(s) != hipSuccess || hipFree(ws->unqm_buf) != hipSuccess) return set_error(TFRA_ERR_HIP, "multi_unique: free failed");
    ws->unqm_buf = nullptr;
  }
  const size_t nmax = std::max<size_t>({total, ws->unqm_nmax, 4096});
  slots = std::max<size_t>({slots, ws->unqm_slots, 2 * 4096 + 1});
  tiles = std::max<size_t>({tiles, ws->unqm_tiles, 64});
  ws->unqm_nmax = ws->unqm_slots = ws->unqm_tiles = 0;
  const UnqManyLayout L(slots, nmax, tiles);
  hipError_t e = hipMalloc(&ws->unqm_buf, L.bytes);
  if (e != hipSuccess) { ws->unqm_buf = nullptr; return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, "multi_unique: hipMalloc failed"); }
  HIP_TRY(hipMemsetAsync(ws->unqm_buf, 0, L.bytes, s));
  ws->unqm_nmax = nmax; ws->unqm_slots = slots; ws->unqm_tiles = tiles; ws->unqm_parity = 1; ws->unqm_gen = 0;
  const UnqSet a = L.set_of(ws->unqm_buf, 0), b = L.set_of(ws->unqm_buf, 1);   // both sets start empty
  unqm_fill_kernel<<<(unsigned)std::min<size_t>(2048, (slots + 255) / 256), 256, 0, s>>>(a.hkeys, a.hfirst, b.hkeys, b.hfirst, slots);
  HIP_TRY(hipGetLastError());
  return TFRA_OK;
}

struct OutRange {
  uintptr_t lo, hi;
  size_t desc;
};

}  // namespace

extern "C" int tfra_multi_unique(tfra_workspace_t* ws, size_t n_lists, const tfra_unique_desc* descs, uint32_t* launches_out,
                                 tfra_stream_t stream) {
  const std::string who = "multi_unique";
  if (launches_out) *launches_out = 0;
  if (n_lists == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, who + ": null argument");
  hipStream_t s = (hipStream_t)stream;
  // every descriptor is checked before anything is enqueued: one bad descriptor and no output and no set changes
  std::vector<const tfra_unique_desc*> act;   // n > 0
  std::vector<i64*> zero;                     // the counts of the lists with n == 0
  std::vector<OutRange> ranges;
  size_t total = 0;
  for (size_t i = 0; i < n_lists; ++i) {
    const tfra_unique_desc& d = descs[i];
    const std::string at_i = who + ": descriptor " + std::to_string(i) + ": ";
    if (d.struct_size != sizeof(tfra_unique_desc)) return set_error(TFRA_ERR_INVALID, at_i + "descriptor size mismatch");
    if (d.flags) return set_error(TFRA_ERR_INVALID, at_i + "unknown flag bits");
    if (!d.d_num_unique) return set_error(TFRA_ERR_INVALID, at_i + "null d_num_unique");
    ranges.push_back({(uintptr_t)d.d_num_unique, (uintptr_t)d.d_num_unique + sizeof(int64_t), i});
    if (d.n == 0) { zero.push_back((i64*)d.d_num_unique); continue; }
    if (!d.ids || !d.unique_out) return set_error(TFRA_ERR_INVALID, at_i + "null buffer");
    if (d.n > UNQM_MAX_LIST) return set_error(TFRA_ERR_INVALID, at_i + "more than 2^20 ids in one list");
    total += d.n;
    if (total > UNQM_MAX_TOTAL) return set_error(TFRA_ERR_INVALID, at_i + "the lists total more than 2^22 ids");
    ranges.push_back({(uintptr_t)d.unique_out, (uintptr_t)d.unique_out + d.n * sizeof(int64_t), i});
    if (d.idx_out) ranges.push_back({(uintptr_t)d.idx_out, (uintptr_t)d.idx_out + d.n * sizeof(int32_t), i});
    act.push_back(&d);
  }
  // every list's outputs are written by blocks of their own with nothing ordered between them: no two output ranges may meet
  std::sort(ranges.begin(), ranges.end(), [](const OutRange& a, const OutRange& b) { return a.lo < b.lo; });
  for (size_t k = 1, top = 0; k < ranges.size(); ++k) {   // top: the range that reaches furthest so far
    if (ranges[k].lo < ranges[top].hi)
      return set_error(TFRA_ERR_INVALID, who + ": descriptor " + std::to_string(std::max(ranges[k].desc, ranges[top].desc)) +
                                             ": an output range overlaps one of descriptor " +
                                             std::to_string(std::min(ranges[k].desc, ranges[top].desc)));
    if (ranges[k].hi > ranges[top].hi) top = k;
  }
  HIP_TRY_AS("hipSetDevice(ws->device)", on_device(ws->device));

  const size_t n_act = act.size(), n_zero = zero.size();
  Blob blob;
  const size_t rec_off = blob.add<UnqManyRec>(n_act);
  const size_t pre_off = blob.add<unsigned>(2 * (n_act + 1) + ClassPool::words(n_act, 1, true));
  const size_t zero_off = blob.add<i64*>(n_zero);
  if (n_act == 0) {   // nothing to de-duplicate: the counts alone, and the sets stay as they are
    ManyUpload up;
    if (int rc = many_begin(ws, 0, blob.bytes(), s, &up)) return rc;
    std::copy(zero.begin(), zero.end(), section<i64*>(up.host, zero_off));
    if (int rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true)) return rc;
    unqm_zero_kernel<<<(unsigned)std::min<size_t>(64, (n_zero + 255) / 256), 256, 0, s>>>(section<i64* const>(up.dev, zero_off), (unsigned)n_zero);
    HIP_TRY(hipGetLastError());
    if (launches_out) *launches_out = 1;
    return TFRA_OK;
  }

  // the sub-sets, one behind the other
  std::vector<unsigned> set_off(n_act), cap(n_act);
  size_t slots = 0, tiles = 0;
  for (size_t k = 0; k < n_act; ++k) {
    unsigned c = 2;
    while (c < 2 * act[k]->n) c <<= 1;
    set_off[k] = (unsigned)slots; cap[k] = c;
    slots += (size_t)c + 1;
    tiles += (act[k]->n + UNQ_TILE - 1) / UNQ_TILE;
  }
  if (int rc = ensure_sets(ws, total, slots, tiles, s)) return rc;
  // The two sets, their parity and generation are STATE of the workspace: calls must reach them in one order (as unique_fast)
  if (ws->unqm_stream_set && ws->unqm_stream != s) {
    if (!ws->unqm_ev) HIP_TRY(hipEventCreateWithFlags(&ws->unqm_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ws->unqm_ev, ws->unqm_stream));
    HIP_TRY(hipStreamWaitEvent(s, ws->unqm_ev, 0));
  }
  ws->unqm_stream = s; ws->unqm_stream_set = true;

  ManyUpload up;
  if (int rc = many_begin(ws, 0, blob.bytes(), s, &up)) return rc;
  UnqManyRec* recs = section<UnqManyRec>(up.host, rec_off);
  unsigned* ins_pre = section<unsigned>(up.host, pre_off);
  unsigned* tile_pre = ins_pre + n_act + 1;
  unsigned base = 0, ins_grid = 0, tile_grid = 0;
  for (size_t k = 0; k < n_act; ++k) {
    const tfra_unique_desc& d = *act[k];
    recs[k] = UnqManyRec{(const i64*)d.ids, (i64*)d.unique_out, d.idx_out, (i64*)d.d_num_unique, (unsigned)d.n, base, set_off[k], cap[k]};
    ins_pre[k] = ins_grid; tile_pre[k] = tile_grid;
    base += (unsigned)d.n;
    ins_grid += (unsigned)((d.n + UNQ_INS - 1) / UNQ_INS);
    tile_grid += (unsigned)((d.n + UNQ_TILE - 1) / UNQ_TILE);
  }
  ins_pre[n_act] = ins_grid; tile_pre[n_act] = tile_grid;
  ClassPool pool{tile_pre + n_act + 1};
  const ManyClass c_idx = pool.put(n_act, true, [&](size_t k) { return act[k]->idx_out != nullptr; },
                                   [&](size_t k) { return (unsigned)((act[k]->n + 255) / 256); });
  std::copy(zero.begin(), zero.end(), section<i64*>(up.host, zero_off));
  if (int rc = many_send(up, s, "hipMemcpyAsync(d_blob, h, blob_bytes, hipMemcpyHostToDevice, s)", true)) return rc;

  const UnqManyLayout L(ws->unqm_slots, ws->unqm_nmax, ws->unqm_tiles);
  const unsigned p = ws->unqm_parity ^ 1u;
  const UnqSet cur = L.set_of(ws->unqm_buf, p), old = L.set_of(ws->unqm_buf, p ^ 1u);
  int* slot_of = (int*)((unsigned char*)ws->unqm_buf + L.slot_of);
  unsigned long long* agg = (unsigned long long*)((unsigned char*)ws->unqm_buf + L.agg);
  if (++ws->unqm_gen == 0) ws->unqm_gen = 1;   // (tile counts of an earlier call carry another generation)
  const UnqManyRec* drecs = section<const UnqManyRec>(up.dev, rec_off);
  const unsigned* dpre = section<const unsigned>(up.dev, pre_off);
  const unsigned* dcls = dpre + 2 * (n_act + 1);
  uint32_t launches = 2;
  unqm_insert_kernel<<<ins_grid, UNQ_INS, 0, s>>>(drecs, dpre, (unsigned)n_act, cur, old, slot_of);
  unqm_scatter_kernel<<<tile_grid, 256, 0, s>>>(drecs, dpre + n_act + 1, (unsigned)n_act, cur, old, slot_of, agg, ws->unqm_gen,
                                                section<i64* const>(up.dev, zero_off), (unsigned)n_zero);
  if (c_idx.n) {
    unqm_idx_kernel<<<c_idx.grid, 256, 0, s>>>(drecs, dcls + c_idx.at, dcls + c_idx.at + c_idx.n + 1, c_idx.n, slot_of, cur.hrank);
    ++launches;
  }
  HIP_TRY(hipGetLastError());
  ws->unqm_parity = p;
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}
