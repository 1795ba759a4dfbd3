// What the grouped calls share (tfra_multi_find_combine: tfra_pool.hip; tfra_multi_apply_planned_combined: tfra_apply_many.hip, with
// its entry-record kernels in tfra_combine.hip; tfra_multi_sparse_plan_build: tfra_csr.hip).
// Device side: the search that takes a block to its descriptor and the records of the launches that run in more than one unit.
// Host side, the frame of a grouped call: the outcome of an operation's argument checks (Check: each operation's checks are ONE
// function, which its single-table call and its grouped call both run), the tables' locks (lock_and_enter), the layout of the
// record blob (Blob), its way to the device through a pinned staging ring (ManyStage, many_begin / many_send) and the block
// prefixes of a launch class (ClassPool).  A grouped call is: check every descriptor, classify, lock, lay out, fill, send, launch.
// The types live in namespace tfra (not in an anonymous one): their launchers cross translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"

namespace tfra {

// The descriptor of block `blk`: the d with prefix[d] <= blk < prefix[d + 1] (prefix[0] = 0, prefix[n] = the grid; strictly
// ascending: no descriptor has zero blocks).  blk is blockIdx.x, so the search, the record's address and the record are
// wave-uniform: scalar loads into scalar registers, as kernel arguments are.
__device__ __forceinline__ unsigned many_desc_of(const unsigned* __restrict__ prefix, unsigned n, unsigned blk) {
  unsigned lo = 0, hi = n;
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (prefix[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// seg64_bounds_many_kernel (tfra_pool.hip): one descriptor's rows' bounds; it owns ceil(nnz / 256) blocks
struct BoundsRec {
  const i64* seg;
  int* se;
  size_t nnz;
  size_t n_rows;
};
// grid = prefix[n]; recs / prefix in device memory
int comb_bounds_many(hipStream_t s, unsigned grid, const BoundsRec* recs, const unsigned* prefix, unsigned n);

// comb_den_many_kernel / comb_ent_many_kernel (tfra_combine.hip): one descriptor's denominators (ceil(n_rows / 256) blocks) and
// per-entry records (ceil(nnz / 256) blocks), what comb_entries makes for one table
struct CombManyRec {
  const i64* seg;
  const float* w;
  const int* se;
  float* den;
  CombEnt* ent;
  size_t nnz;
  size_t n_rows;
  int combiner;
};
// two launches: the denominators of all descriptors' rows, then all descriptors' entry records
int comb_den_ent_many(hipStream_t s, unsigned den_grid, unsigned ent_grid, const CombManyRec* recs, const unsigned* den_prefix,
                      const unsigned* ent_prefix, unsigned n);

// The records reach the device by ONE asynchronous copy per call from a pinned staging slot.  Two calls may be enqueued back to
// back with nothing waited for in between, so a slot must not be rewritten while its copy has not run: the slots form a ring,
// each guarded by an event recorded behind its copy.  Taking a slot waits for ITS event only — in the steady state the copy of
// RING calls ago, long done — never for the stream.  A list that outgrows the slots waits for the pending copies and reallocates.
// One ring per workspace (tfra_workspace::many), whichever grouped call uses it.
struct ManyStage {
  static constexpr int RING = 8;
  unsigned char* host = nullptr;
  size_t slot_bytes = 0;
  hipEvent_t ev[RING] = {};
  bool pending[RING] = {};
  unsigned next = 0;

  static int hip_rc(hipError_t e, const char* what) {
    if (e == hipSuccess) return TFRA_OK;
    return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  int drain() {
    for (int i = 0; i < RING; ++i)
      if (pending[i]) {
        if (int rc = hip_rc(hipEventSynchronize(ev[i]), "staging ring: hipEventSynchronize")) return rc;
        pending[i] = false;
      }
    return TFRA_OK;
  }
  int take(size_t need, unsigned char** out, int* slot) {
    if (!ev[0])
      for (int i = 0; i < RING; ++i)
        if (int rc = hip_rc(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), "staging ring: hipEventCreateWithFlags")) return rc;
    if (need > slot_bytes) {
      int rc = drain();
      if (rc) return rc;
      if (host) {
        if ((rc = hip_rc(hipHostFree(host), "staging ring: hipHostFree"))) return rc;
        host = nullptr; slot_bytes = 0;
      }
      const size_t want = (std::max<size_t>(need, 8192) + 4095) / 4096 * 4096;
      if ((rc = hip_rc(hipHostMalloc((void**)&host, want * RING, hipHostMallocDefault), "staging ring: hipHostMalloc"))) { host = nullptr; return rc; }
      slot_bytes = want;
    }
    const int i = (int)(next++ % RING);
    if (pending[i]) {
      if (int rc = hip_rc(hipEventSynchronize(ev[i]), "staging ring: hipEventSynchronize")) return rc;
      pending[i] = false;
    }
    *out = host + (size_t)i * slot_bytes;
    *slot = i;
    return TFRA_OK;
  }
  // behind the copy out of slot `slot` on stream s
  int sent(int slot, hipStream_t s) {
    if (int rc = hip_rc(hipEventRecord(ev[slot], s), "staging ring: hipEventRecord")) return rc;
    pending[slot] = true;
    return TFRA_OK;
  }
};

// The blob of one call: the workspace holds [front_bytes of the call's own scratch | blob]; `host` is the staging slot to fill,
// `dev` where it lands.  A section sits at the same offset in both (Blob).
struct ManyUpload {
  unsigned char *host = nullptr, *dev = nullptr;
  size_t bytes = 0;
  ManyStage* stage = nullptr;
  int slot = 0;
};
inline int many_begin(tfra_workspace* ws, size_t front_bytes, size_t blob_bytes, hipStream_t s, ManyUpload* u) {
  if (int rc = ws->ensure(front_bytes + blob_bytes, s)) return rc;
  if (!ws->many) ws->many = new ManyStage();   // the workspace's ring, made on first use
  u->stage = reinterpret_cast<ManyStage*>(ws->many);
  u->dev = (unsigned char*)ws->buf + front_bytes;
  u->bytes = blob_bytes;
  return u->stage->take(blob_bytes, &u->host, &u->slot);
}
// the filled slot's copy and the event behind it; a copy that fails: `what` with TFRA_ERR_HIP, or (hip_detail) as ManyStage::hip_rc
inline int many_send(const ManyUpload& u, hipStream_t s, const char* what, bool hip_detail) {
  const hipError_t e = hipMemcpyAsync(u.dev, u.host, u.bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_detail ? ManyStage::hip_rc(e, what) : set_error(TFRA_ERR_HIP, what);
  return u.stage->sent(u.slot, s);
}

// Offsets of the blob's sections: each (element type, count) starts 16-byte aligned, the total is rounded to 256.
struct Blob {
  size_t end = 0;
  template <class T>
  size_t add(size_t count) {
    const size_t at = (end + 15) / 16 * 16;
    end = at + count * sizeof(T);
    return at;
  }
  size_t bytes() const { return (end + 255) / 256 * 256; }
};
template <class T>
inline T* section(unsigned char* base, size_t off) { return reinterpret_cast<T*>(base + off); }

// The launch classes of a call, one after the other in a section of unsigned words: a class is [prefix (n + 1)], then [idx (n)]
// where its kernel reads the records through an index.  put() appends the class of the k in [0, n_all) with member(k), blocks(k)
// blocks each; a class without members takes no words.  words(): what n_all members in at most n_classes classes can take.
struct ManyClass { size_t at = 0; unsigned n = 0, grid = 0; };
struct ClassPool {
  unsigned* host;
  size_t at = 0;
  static size_t words(size_t n_all, size_t n_classes, bool with_idx) { return (with_idx ? 2 : 1) * n_all + n_classes; }
  template <class Member, class Blocks>
  ManyClass put(size_t n_all, bool with_idx, Member&& member, Blocks&& blocks) {
    ManyClass c{at, 0, 0};
    for (size_t k = 0; k < n_all; ++k) c.n += member(k) ? 1 : 0;
    if (!c.n) return c;
    unsigned* pre = host + at;
    unsigned* idx = pre + c.n + 1;
    unsigned j = 0;
    for (size_t k = 0; k < n_all; ++k) {
      if (!member(k)) continue;
      pre[j] = c.grid;
      if (with_idx) idx[j] = (unsigned)k;
      ++j;
      c.grid += blocks(k);
    }
    pre[j] = c.grid;
    at += c.n + 1 + (with_idx ? c.n : 0);
    return c;
  }
};

// Each distinct table of `tabs` locked once, in one global order (by address: two threads with overlapping lists cannot
// deadlock), then entered on s (also: the calling thread is on the tables' device from here on).
inline int lock_and_enter(std::vector<Table*> tabs, hipStream_t s, std::vector<std::unique_lock<std::mutex>>* locks) {
  std::sort(tabs.begin(), tabs.end(), std::less<Table*>());
  tabs.erase(std::unique(tabs.begin(), tabs.end()), tabs.end());
  locks->reserve(tabs.size());
  for (Table* t : tabs) locks->emplace_back(t->mu);
  for (Table* t : tabs)
    if (int rc = t->enter(s)) return rc;
  return TFRA_OK;
}

// The outcome of an operation's argument checks: a code and the message WITHOUT the entry point's prefix (no message: the callee
// that failed has recorded its own), or TFRA_OK and whether there is anything to do.  An operation's checks are one function in
// the single call's order; where that call locks and enters its table the function calls `at_entry`, which the grouped call uses
// for what only a descriptor can get wrong.
struct Check {
  int code = TFRA_OK;
  std::string msg;
  bool active = true;
  bool done() const { return code != TFRA_OK || !active; }
};
inline Check refuse(int code, const char* msg) { return Check{code, msg, false}; }
inline Check nothing_to_do() { return Check{TFRA_OK, "", false}; }
inline int report(const std::string& who, const Check& c) { return c.msg.empty() ? c.code : set_error(c.code, who + c.msg); }

// What a tfra_grads itself must satisfy, before anything is enqueued: ONE copy for the typed write-backs (tfra_apply.hip,
// tfra_apply_many.hip), tfra_table_fetch_planned (tfra_rows.hip) and the typed weight gradients (tfra_wgrad*.hip, tfra_tierwgrad.hip,
// tfra_combine.hip).  forward: float32 without a scale — the untyped call, as it is.
inline Check check_typed(const tfra_grads* g, bool* forward) {
  *forward = false;
  if (!g || !g->grads) return refuse(TFRA_ERR_INVALID, "null gradients");
  if (g->reserved != 0) return refuse(TFRA_ERR_INVALID, "tfra_grads.reserved must be 0");
  if (g->dtype != TFRA_F32 && g->dtype != TFRA_F16 && g->dtype != TFRA_BF16)
    return refuse(TFRA_ERR_INVALID, "tfra_grads.dtype must be float32, float16 or bfloat16");
  if (g->dtype == TFRA_F32) {
    if (g->d_scale) return refuse(TFRA_ERR_UNSUPPORTED, "float32 gradients take no scale (loss scaling belongs to float16)");
    *forward = true;
  } else if ((uintptr_t)g->grads & 7) {
    return refuse(TFRA_ERR_UNSUPPORTED, "half gradients must be 8-B aligned");
  }
  return Check{};
}

}  // namespace tfra
