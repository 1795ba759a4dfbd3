// The overlapped step's driver (tfra_step_driver_t, tfra_table_step[s]_overlap): one launch per step of the kernel in
// tfra_step_impl.h, fed from the plan objects of tfra_csr.hip / tfra_setplan.hip and the ownership pass's host half (tfra_own.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_combine_device.h"
#include "tfra_device.h"
#include "tfra_host.h"
#include "tfra_optim_device.h"
#include "tfra_plan.h"
#include "tfra_reduce_device.h"
#include "tfra_step_impl.h"

using namespace tfra;
using namespace tfra::red;

struct tfra_step_driver {
  Table* t = nullptr;
  tfra_table_t* tp = nullptr;
  static constexpr unsigned NPL = 4;      // plans in rotation: batch b uses plans[b % NPL] (previous, this, next, the one being scattered)
  tfra_sparse_plan* plans[NPL] = {};
  unsigned seq = 0;                        // batches looked up so far
  bool pending = false;                    // the batch of the previous call still has to be written back
  unsigned pend_slot = 0;
  const int64_t* pend_ids = nullptr;       // its ids (the caller keeps them until the batch has been written back)
  size_t pend_n = 0;
  bool ahead = false;                      // plans[seq % NPL] already holds the plan of (ahead_ids, ahead_n): built by the last call
  const int64_t* ahead_ids = nullptr;
  size_t ahead_n = 0;
  unsigned scat_uses = 0;                  // scatters so far (the overflow counter of a plan's segments alternates)
  SetEnt* dummy = nullptr;                 // an empty table (4 entries + the sentinel slots + padding): "no previous batch"
  unsigned* progress = nullptr;            // pinned: [0] step
  unsigned* stat = nullptr;                // device: StepArgs::stat
  u64* tbuf = nullptr;                     // device: StepArgs::tbuf (TFRA_STEP_VARIANT & 16)
  unsigned tinfo[64][7] = {};              // per launch slot: build, scatter, own, lookup blocks, grid (the rest: tail), map blocks, lookup blocks in front of the write-back
  int find_first = 0;                      // TFRA_STEP_FIND_FIRST (tuning): lookup blocks in front of the write-back's
  unsigned own_slice = OWN_SLICE_DEFAULT;  // TFRA_STEP_OWN_SLICE (tuning): plan slots per write-back block (<= 768)
  bool own_slice_fixed = false;            // ... given: no adaptation to the batch's distinct-key count
  // MAP lists (round 5): two buffers of up to MAX_IDS 16-byte entries alternate — one is read by this launch's lookup, the other filled for the next
  unsigned char* mapbuf = nullptr;         // device: 2 x cap entries
  size_t map_cap = 0;
  unsigned map_slot = 0;                   // the list filled last
  bool map_valid = false;                  // ... and what it holds: the positions of (map_ids, map_n) probed in map_plan's current table
  const int64_t* map_ids = nullptr;
  size_t map_n = 0;
  const tfra_sparse_plan* map_plan = nullptr;
  unsigned map_gen = 0;                    // (the plan's build generation at that time)
  unsigned long long n_find_listed = 0;    // lookups served from a MAP list
  unsigned last_tail_step = ~0u;           // step number of the last launch that had a tail (it zeroes the next launch's counters)
  unsigned char* patch = nullptr;          // device: two victim counters (one 128-B line each) + two lists of PATCH_GCAP keys + two sets of 10 sync counters (tail_role)
  unsigned step_no = 0;
  int ablate = 0; unsigned ablate_after = 40;   // TFRA_STEP_ABLATE / TFRA_STEP_ABLATE_AFTER (tuning: timing of the roles alone; results are wrong)
  int variant = 0;                         // TFRA_STEP_VARIANT (tuning): kernel instantiation
  unsigned long long n_overlapped = 0, n_sequential = 0;   // steps taken each way (tfra_step_driver_stats)
  unsigned long long n_built_in_launch = 0, n_built_in_front = 0;   // plans of the next batch built by the step launch / by a launch of their own
  unsigned why_sequential = 0;             // why the last step that was not overlapped was not (bit mask, see step_overlap_one)
  std::vector<hipEvent_t> kev;             // tfra_step_driver_time_kernels: 3 events per timed step (before / behind its launch; the third marks the end of the step)
  size_t kev_left = 0, kev_used = 0;
};

extern "C" int tfra_step_driver_create(tfra_table_t* tp, tfra_step_driver_t** out) {
  Table* t = reinterpret_cast<Table*>(tp);
  if (!t || !out) return set_error(TFRA_ERR_INVALID, "step_driver_create: null argument");
  if (on_device(t->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_driver_create: hipSetDevice");
  tfra_step_driver* d = new tfra_step_driver();
  d->t = t; d->tp = tp;
  for (unsigned i = 0; i < tfra_step_driver::NPL; ++i) {
    int rc = tfra_sparse_plan_create(t->device, &d->plans[i]);
    if (rc) { tfra_step_driver_destroy(d); return rc; }
  }
  const size_t dn = 4 + 2 + SET_PAD;
  if (hipMalloc((void**)&d->dummy, dn * sizeof(SetEnt)) != hipSuccess) { d->dummy = nullptr; tfra_step_driver_destroy(d); return set_error(TFRA_ERR_OOM, "step_driver_create: hipMalloc"); }
  setplan_fill_empty(d->dummy, dn, nullptr);
  constexpr size_t PATCH_BYTES = 256 + 2 * PATCH_GCAP * 8 + 2 * 10 * 128;
  if (hipMalloc((void**)&d->patch, PATCH_BYTES) != hipSuccess || hipMemset(d->patch, 0, PATCH_BYTES) != hipSuccess) { d->patch = nullptr; tfra_step_driver_destroy(d); return set_error(TFRA_ERR_OOM, "step_driver_create: hipMalloc"); }
  if (hipMalloc((void**)&d->stat, 64) != hipSuccess || hipMemset(d->stat, 0, 64) != hipSuccess) { tfra_step_driver_destroy(d); return set_error(TFRA_ERR_OOM, "step_driver_create: hipMalloc"); }
  if (hipHostMalloc((void**)&d->progress, 64, hipHostMallocDefault) != hipSuccess) { d->progress = nullptr; tfra_step_driver_destroy(d); return set_error(TFRA_ERR_OOM, "step_driver_create: hipHostMalloc"); }
  d->progress[0] = d->progress[1] = 0;
  if (hipDeviceSynchronize() != hipSuccess) { tfra_step_driver_destroy(d); return set_error(TFRA_ERR_HIP, "step_driver_create: sync"); }
  const char* ev = std::getenv("TFRA_STEP_VARIANT");
  d->variant = ev ? std::atoi(ev) : 0;
  if (const char* ab = std::getenv("TFRA_STEP_ABLATE")) d->ablate = std::atoi(ab);
  if (const char* ab = std::getenv("TFRA_STEP_ABLATE_AFTER")) d->ablate_after = (unsigned)std::atoi(ab);
  if (const char* os_ = std::getenv("TFRA_STEP_OWN_SLICE")) { d->own_slice = std::min(768u, std::max(64u, (unsigned)std::atoi(os_))); d->own_slice_fixed = true; }
  if (const char* ff = std::getenv("TFRA_STEP_FIND_FIRST")) d->find_first = std::atoi(ff);
  if (d->variant & 16) {
    const size_t bytes = (size_t)TIMING_SLOTS * TIMING_BLOCKS * 16;
    if (hipMalloc((void**)&d->tbuf, bytes) != hipSuccess || hipMemset(d->tbuf, 0, bytes) != hipSuccess) { d->tbuf = nullptr; tfra_step_driver_destroy(d); return set_error(TFRA_ERR_OOM, "step_driver_create: hipMalloc"); }
  }
  *out = d;
  return TFRA_OK;
}

extern "C" int tfra_step_driver_destroy(tfra_step_driver_t* d) {
  if (!d) return TFRA_OK;
  (void)hipSetDevice(d->t->device);
  (void)hipDeviceSynchronize();
  for (unsigned i = 0; i < tfra_step_driver::NPL; ++i) if (d->plans[i]) tfra_sparse_plan_destroy(d->plans[i]);
  if (d->dummy) (void)hipFree(d->dummy);
  if (d->stat) (void)hipFree(d->stat);
  if (d->tbuf) (void)hipFree(d->tbuf);
  if (d->patch) (void)hipFree(d->patch);
  if (d->mapbuf) (void)hipFree(d->mapbuf);
  for (hipEvent_t e : d->kev) (void)hipEventDestroy(e);
  if (d->progress) (void)hipHostFree(d->progress);
  delete d;
  return TFRA_OK;
}

extern "C" int tfra_step_driver_stats(const tfra_step_driver_t* d, uint64_t* overlapped, uint64_t* sequential, int* pending, uint32_t* device_counts,
                                      uint32_t* why_sequential, uint64_t* plans_built) {
  if (!d) return set_error(TFRA_ERR_INVALID, "step_driver_stats: null driver");
  if (why_sequential) *why_sequential = d->why_sequential;
  if (overlapped) *overlapped = d->n_overlapped;
  if (sequential) *sequential = d->n_sequential;
  if (pending) *pending = d->pending ? 1 : 0;
  if (plans_built) { plans_built[0] = d->n_built_in_launch; plans_built[1] = d->n_built_in_front; }
  if (device_counts) {   // synchronises the device
    (void)hipSetDevice(d->t->device);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(device_counts, d->stat, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
      return set_error(TFRA_ERR_HIP, "step_driver_stats: copy");
  }
  return TFRA_OK;
}

extern "C" int tfra_step_driver_lookups_listed(const tfra_step_driver_t* d, uint64_t* out) {
  if (!d || !out) return set_error(TFRA_ERR_INVALID, "step_driver_lookups_listed: null argument");
  *out = d->n_find_listed;
  return TFRA_OK;
}

// tuning: the block time stamps of the last <= 64 launches made with TFRA_STEP_VARIANT & 16, reduced per role —
// out[64][6][4] = {earliest block start, latest block end, median block duration, 95th percentile of the block durations} on the
// device clock (100 MHz) per launch slot (step % 64) and role (build, scatter, write-back, lookup, tail, map), ~0 / 0 where nothing ran;
// synchronises the device and re-arms the stamps.
extern "C" int tfra_step_driver_timing(tfra_step_driver_t* d, uint64_t* out) {
  if (!d) return set_error(TFRA_ERR_INVALID, "step_driver_timing: null driver");
  if (!d->tbuf) return set_error(TFRA_ERR_INVALID, "step_driver_timing: the driver was not created with TFRA_STEP_VARIANT & 16");
  (void)hipSetDevice(d->t->device);
  const size_t words = (size_t)TIMING_SLOTS * TIMING_BLOCKS * 2;
  std::vector<uint64_t> h(words);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), d->tbuf, words * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemset(d->tbuf, 0, words * 8) != hipSuccess)
    return set_error(TFRA_ERR_HIP, "step_driver_timing: copy");
  if (!out) return TFRA_OK;
  for (unsigned sl = 0; sl < TIMING_SLOTS; ++sl) {
    const unsigned* ti = d->tinfo[sl];
    const unsigned grid = std::min(ti[4], TIMING_BLOCKS);
    constexpr int NR = 6;
    auto role_of = [&](unsigned b) { unsigned idx; return step_role(b, ti[0], ti[1], ti[5], ti[6], ti[2], ti[3], ti[4] - ti[0] - ti[1] - ti[5] - ti[2] - ti[3], &idx); };
    std::vector<uint64_t> dur[NR];
    for (int r = 0; r < NR; ++r) { out[(sl * NR + r) * 4] = ~0ULL; out[(sl * NR + r) * 4 + 1] = 0; out[(sl * NR + r) * 4 + 2] = 0; out[(sl * NR + r) * 4 + 3] = 0; }
    for (unsigned b = 0; b < grid; ++b) {
      const uint64_t t0 = h[((size_t)sl * TIMING_BLOCKS + b) * 2], t1 = h[((size_t)sl * TIMING_BLOCKS + b) * 2 + 1];
      if (!t1) continue;
      const int r = role_of(b);
      out[(sl * NR + r) * 4] = std::min(out[(sl * NR + r) * 4], t0);
      out[(sl * NR + r) * 4 + 1] = std::max(out[(sl * NR + r) * 4 + 1], t1);
      dur[r].push_back(t1 - t0);
    }
    if (std::getenv("TFRA_STEP_OCCUPANCY") && sl == 5 && grid) {   // (tuning) resident blocks per role, every microsecond of one launch
      uint64_t tmin = ~0ULL, tmax = 0;
      for (unsigned b = 0; b < grid; ++b) {
        const uint64_t t0 = h[((size_t)sl * TIMING_BLOCKS + b) * 2], t1 = h[((size_t)sl * TIMING_BLOCKS + b) * 2 + 1];
        if (t1) { tmin = std::min(tmin, t0); tmax = std::max(tmax, t1); }
      }
      for (uint64_t t = tmin; t < tmax; t += 100) {   // (the clock ticks at 100 MHz)
        unsigned n[NR] = {0, 0, 0, 0, 0, 0};
        for (unsigned b = 0; b < grid; ++b) {
          const uint64_t t0 = h[((size_t)sl * TIMING_BLOCKS + b) * 2], t1 = h[((size_t)sl * TIMING_BLOCKS + b) * 2 + 1];
          if (t1 && t0 <= t && t < t1) n[role_of(b)] += 1;
        }
        std::fprintf(stderr, "t %2llu us: build %4u scatter %4u map %4u write-back %4u lookup %4u tail %3u  = %4u blocks\n", (unsigned long long)((t - tmin) / 100), n[0], n[1],
                     n[5], n[2], n[3], n[4], n[0] + n[1] + n[2] + n[3] + n[4] + n[5]);
      }
    }
    for (int r = 0; r < NR; ++r) {
      if (dur[r].empty()) continue;
      std::sort(dur[r].begin(), dur[r].end());
      out[(sl * NR + r) * 4 + 2] = dur[r][dur[r].size() / 2];
      out[(sl * NR + r) * 4 + 3] = dur[r][dur[r].size() * 95 / 100];
    }
    d->tinfo[sl][4] = 0;
  }
  return TFRA_OK;
}

// Measurement: HIP events around the launch of each of the next `steps` overlapped steps (on the stream they are launched on);
// tfra_step_driver_kernel_times then waits for them and returns the average duration of each launch in microseconds.
extern "C" int tfra_step_driver_time_kernels(tfra_step_driver_t* d, size_t steps) {
  if (!d) return set_error(TFRA_ERR_INVALID, "step_driver_time_kernels: null driver");
  (void)hipSetDevice(d->t->device);
  while (d->kev.size() < steps * 3) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_driver_time_kernels: event");
    d->kev.push_back(e);
  }
  d->kev_left = steps; d->kev_used = 0;
  return TFRA_OK;
}
extern "C" int tfra_step_driver_kernel_times(tfra_step_driver_t* d, double* step_kernel_us, double* rest_kernel_us, size_t* steps) {
  if (!d) return set_error(TFRA_ERR_INVALID, "step_driver_kernel_times: null driver");
  double a = 0, b = 0;
  for (size_t i = 0; i < d->kev_used; ++i) {
    float x = 0, y = 0;
    if (hipEventSynchronize(d->kev[i * 3 + 2]) != hipSuccess || hipEventElapsedTime(&x, d->kev[i * 3], d->kev[i * 3 + 1]) != hipSuccess ||
        hipEventElapsedTime(&y, d->kev[i * 3 + 1], d->kev[i * 3 + 2]) != hipSuccess)
      return set_error(TFRA_ERR_HIP, "step_driver_kernel_times: event");
    a += x; b += y;
  }
  const double nn = d->kev_used ? (double)d->kev_used : 1.0;
  if (step_kernel_us) *step_kernel_us = a / nn * 1e3;
  if (rest_kernel_us) *rest_kernel_us = b / nn * 1e3;
  if (steps) *steps = d->kev_used;
  d->kev_left = 0; d->kev_used = 0;
  return TFRA_OK;
}

static SetProbe probe_of(const tfra_sparse_plan* pl) { return SetProbe{pl->set_tab[pl->set_parity].ent, pl->set_m2}; }
static bool plan_is_listless(const tfra_sparse_plan* pl) { return pl->kind == 1 && pl->tab_state[pl->set_parity] == 2; }

// variant (TFRA_STEP_VARIANT, tuning): bits 0-2 kernel (0: 8 keys per wave in the write-back, 5 blocks per CU | 1: 4 keys | 2: 4 blocks per CU | 3: 6), 8 every plan as a launch of
// its own, 16 time stamps, 32 no MAP role (round 4's lookup), 64 the lookup reads the table's lines for every id.  TFRA_STEP_OWN_SLICE: a fixed
// write-back slice (else sized from the batch's distinct-key count), TFRA_STEP_FIND_FIRST: lookup blocks in front of the write-back's
static void launch_step(int variant, unsigned grid, hipStream_t s, const StepArgs& a, bool lru) {   // the overlapped step: one launch
  const int k = variant & 7;
  if (!lru) step_k_gen<<<grid, 256, 0, s>>>(a);
  else if (variant & 16) step_k_u2_t<<<grid, 256, 0, s>>>(a);
  else if (k == 1) step_k_u1<<<grid, 256, 0, s>>>(a);
  else if (k == 2) step_k_u2_w4<<<grid, 256, 0, s>>>(a);
  else if (k == 3) step_k_u2_w6<<<grid, 256, 0, s>>>(a);
  else step_k_u2<<<grid, 256, 0, s>>>(a);
}

// One step (n == 0 and no look-ahead: just the pending write-back, the flush).  Caller holds d->t->step_mu.
static int step_overlap_one(tfra_step_driver* d, size_t n, const int64_t* ids, void* rows_out, uint8_t* exists_out, const void* defaults,
                            int default_is_full, const void* values_prev, const uint64_t* scores_prev, size_t n_next,
                            const int64_t* ids_next, size_t n_next2, const int64_t* ids_next2, hipStream_t s) {
  Table* t = d->t;
  if (n && (!ids || !rows_out || !defaults)) return set_error(TFRA_ERR_INVALID, "step_overlap: null buffer");
  if (n > MAX_IDS || n_next > MAX_IDS || n_next2 > MAX_IDS) return set_error(TFRA_ERR_UNSUPPORTED, "step_overlap: at most 2^18 ids per step");
  if (d->pending && !values_prev) return set_error(TFRA_ERR_INVALID, "step_overlap: the previous step's batch has not been written back: values_prev is null");
  if ((n_next && !ids_next) || (n_next2 && !ids_next2)) return set_error(TFRA_ERR_INVALID, "step_overlap: null look-ahead ids");
  constexpr unsigned NPL = tfra_step_driver::NPL;
  const unsigned slot = d->seq % NPL;
  tfra_sparse_plan* plan_cur = d->plans[slot];
  tfra_sparse_plan* plan_prev = d->pending ? d->plans[d->pend_slot] : nullptr;
  tfra_sparse_plan* plan_next = d->plans[(d->seq + 1) % NPL];
  tfra_sparse_plan* plan_next2 = d->plans[(d->seq + 2) % NPL];
  std::unique_lock<std::mutex> lock(t->mu);
  int rc = t->enter(s);
  if (rc) return rc;
  const bool lfu = t->opts.strategy == TFRA_EVICT_LFU;
  // this batch's plan: built by the previous call (look-ahead), else here, in front of the step (one more launch)
  if (n && !(d->ahead && d->ahead_ids == ids && d->ahead_n == n)) {
    rc = setplan_build(plan_cur, n, ids, s, lfu);
    if (rc) return rc;
    d->n_built_in_front += 1;
  }
  if (!n) plan_cur->n = 0;
  d->ahead = false;
  // a MAP list is good for exactly one lookup: these ids, forwarded from that plan as it was built then
  const bool list_ok = d->map_valid && n && d->map_ids == ids && d->map_n == n && plan_prev && d->map_plan == plan_prev && d->map_gen == plan_prev->gen;
  d->map_valid = false;
  // Announced batches are recognised by (address, length).  Whatever this call does not consume is disarmed HERE, on every path: pairs
  // scattered for a batch that is not announced again (no ids_next, the sequential path, a plan launch in front) must not meet a
  // later batch that happens to live at the same address.
  if (!(n_next && plan_next->scat_ids == ids_next && plan_next->scat_n == n_next)) { plan_next->scat_ids = nullptr; plan_next->scat_n = 0; }
  plan_cur->scat_ids = nullptr; plan_cur->scat_n = 0;
  if (plan_prev) { plan_prev->scat_ids = nullptr; plan_prev->scat_n = 0; }
  // (plan_next2's segments are filled by this call or not at all)
  plan_next2->scat_ids = nullptr; plan_next2->scat_n = 0;
  unsigned* tags = t->ensure_own_tags(s);
  // what the TABLE must be for the overlap (constant over its life, but for `dense`) and what this CALL must be
  const bool lru_like = t->opts.strategy == TFRA_EVICT_LRU || t->opts.strategy == TFRA_EVICT_EPOCHLRU;   // a new key is always admitted
  // Round 6: a GROWING table (the cuckoo flavour: no eviction strategy, no max_capacity — what TFRA's default creator instantiates) qualifies
  // too: every key of a batch ends up in it (it grows — own_prepare's prepare_insert, in stream order in front of the launch — instead of
  // refusing or evicting), a new key that finds no free slot in its two home buckets goes to the tail's general (walking) path like any
  // left-over key, and nothing is ever evicted under the lookup.  TFRA_STEP_GROWING=0 keeps such tables on the sequential path.
  static const bool growing_ok = [] { const char* e = std::getenv("TFRA_STEP_GROWING"); return !e || std::atoi(e) != 0; }();
  const bool growing = growing_ok && t->opts.strategy == TFRA_EVICT_NONE && t->opts.max_capacity == 0;
  // ... and so does a BOUNDED LRU / EPOCHLRU table that is not (yet) at its max_capacity or not yet dense: below max_capacity it grows like
  // the cuckoo flavour; at max_capacity but sparse a new key walks four buckets and an eviction — if it comes to one — is the tail's (after
  // every write-back block, victims the lookup asked for corrected as always).  An Hkv table whose max_capacity is never reached — a common
  // deployment — used to stay on the sequential path for ever (reasons 16 / 32).
  const bool any_fill = growing_ok && lru_like;
  const unsigned why_table = (tags ? 0u : 4u) | ((t->opts.aux_fields == 0 && (lru_like || growing)) ? 0u : 8u) |
                             ((growing || any_fill || t->at_max_capacity()) ? 0u : 16u) | ((growing || any_fill || t->dense) ? 0u : 32u) |
                             (t->capture_safe ? 128u : 0u) | ((t->field_bytes & 15u) ? 2u : 0u);
  const bool aligned = (((uintptr_t)rows_out | (uintptr_t)defaults | (uintptr_t)values_prev) & 15) == 0;
  const unsigned why = why_table | (aligned ? 0u : 2u) | (scores_prev ? 8u : 0u) | ((!plan_prev || plan_prev->n > 0) ? 0u : 64u);
  const bool eligible = why == 0 && (n > 0 || plan_prev);
  const unsigned step = ++d->step_no;
  if (!eligible) {
    if (n || plan_prev) d->why_sequential = why ? why : 1u;
    // the same results one after the other: write-back of the previous batch, this lookup, the next batch's plan
    if (plan_prev && plan_prev->n) {
      if (plan_is_listless(plan_prev)) {   // its plan has no key list (built by a step launch): build it again, with one
        rc = setplan_build(plan_prev, d->pend_n, d->pend_ids, s, lfu);
        if (rc) return rc;
      }
      rc = upsert_planned_impl(d->tp, plan_prev, values_prev, scores_prev, s, nullptr, 0);
      if (rc) return rc;
    }
    lock.unlock();
    if (n) { rc = tfra_table_find(d->tp, n, ids, rows_out, exists_out, defaults, default_is_full, s); if (rc) return rc; }
    plan_next->scat_ids = nullptr; plan_next->scat_n = 0;
    if (n_next) {
      rc = setplan_build(plan_next, n_next, ids_next, s, lfu);
      if (rc) return rc;
      d->n_built_in_front += 1;
    }
    if (n || plan_prev) d->n_sequential += 1;
  } else {
    StepArgs a{};
    OwnLaunch L{};
    if (plan_prev) {
      rc = own_prepare(t, plan_prev, values_prev, nullptr, s, nullptr, &L);
      if (rc) return rc;
      a.own = L.a;
      a.ctr = L.ctr; a.own_gen = L.og;
      a.fwd = probe_of(plan_prev);
      if (plan_is_listless(plan_prev) && plan_prev->ucnt) { a.own_ucnt = plan_prev->ucnt; a.own_ucnt_n = plan_prev->set_m2 / SET_WIN; }
      // ~40 keys per write-back block (two rounds of its four waves): the slice follows the density of the plan's table, known from
      // the distinct-key count an earlier launch's tail left in pinned memory (0: none yet)
      a.own_slice = d->own_slice;
      if (!d->own_slice_fixed) {
        const unsigned u_est = __atomic_load_n(d->progress + 1, __ATOMIC_RELAXED);
        // (a launch whose lookup is SMALL — the distinct ids one rank of a sharded table serves: 22 K lookups beside 22 K writes, the whole
        // grid resident at once — runs faster with ~64 keys per write-back block: slices of 640-768 slots 26 us, 448 slots 29 us;
        // the metric's full batches keep ~40: scripts/sweep_owner.sh)
        const bool small_lookup = n < 65536;
        if (u_est) a.own_slice = std::min(small_lookup ? 768u : 512u, std::max(96u, (unsigned)((small_lookup ? 64ull : 40ull) * (a.fwd.m2 + 2) / u_est) & ~31u));
      }
      a.own_blocks = (a.fwd.m2 + 2 + a.own_slice - 1) / a.own_slice;
    } else {
      a.own.v = t->view_of(t->cur);
      a.own_blocks = 0;
      a.fwd = SetProbe{d->dummy, 4};
    }
    a.progress = d->progress; a.progress_val = step; a.stat = d->stat; a.tbuf = d->tbuf;
    a.patch_keys = reinterpret_cast<i64*>(d->patch + 256) + (size_t)PATCH_GCAP * (step & 1u);
    a.nxt = n ? probe_of(plan_cur) : SetProbe{d->dummy, 4};
    a.n = (unsigned)n; a.ids = (const i64*)ids; a.out = (unsigned char*)rows_out; a.exists = exists_out;
    a.defaults = (const unsigned char*)defaults; a.full = default_is_full;
    a.find_blocks = (unsigned)((n + 63) / 64);
    a.tail_blocks = plan_prev ? TAIL_BLOCKS : 0u;
    a.sync = reinterpret_cast<unsigned*>(d->patch + 256 + 2 * PATCH_GCAP * 8 + 1280 * (step & 1u));
    a.sync_next = reinterpret_cast<unsigned*>(d->patch + 256 + 2 * PATCH_GCAP * 8 + 1280 * ((step & 1u) ^ 1u));
    a.patch_count = a.sync + 32 * 9 + 1; a.patch_count_next = a.sync_next + 32 * 9 + 1;   // (read with the tail's arrivals as one 8-byte word)
    a.zero4 = plan_prev ? reinterpret_cast<unsigned*>(L.next_ctr) : nullptr;
    a.serial_probe = (d->variant & 64) ? 0 : 1;
    a.ablate = (d->ablate && d->step_no >= d->ablate_after) ? d->ablate : 0;   // (tuning: TFRA_STEP_ABLATE / _AFTER; results are wrong)
    int map_slot_new = -1;
    if (list_ok) {
      a.find_list = reinterpret_cast<const uint4*>(d->mapbuf + (size_t)d->map_slot * d->map_cap * 16);
      d->n_find_listed += 1;
      a.find_blocks = (unsigned)((n + MAP_SEG - 1) / MAP_SEG) * (MAP_SEG / 64u);   // chunk-major over whole segments
      a.find_first = d->find_first > 0 ? std::min((unsigned)d->find_first, a.find_blocks) : 0u;
    }
    // the NEXT lookup's positions, probed in this batch's plan (complete before this launch): the MAP role
    if (n && n_next && !(d->variant & 32)) {
      if (d->map_cap < std::max(n_next, (size_t)4096)) {
        if (d->mapbuf) { if (hipDeviceSynchronize() != hipSuccess || hipFree(d->mapbuf) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_overlap: free"); d->mapbuf = nullptr; }
        if (a.find_list) { a.find_list = nullptr; a.find_blocks = (unsigned)((n + 63) / 64); a.find_first = 0; }   // (it lived in the buffer just freed; n <= the old capacity < n_next)
        size_t cap = 4096;
        while (cap < n_next) cap <<= 1;
        if (hipMalloc((void**)&d->mapbuf, 2 * cap * 16) != hipSuccess) { d->mapbuf = nullptr; d->map_cap = 0; return set_error(TFRA_ERR_OOM, "step_overlap: hipMalloc"); }
        d->map_cap = cap;
      }
      const unsigned ms = a.find_list ? (d->map_slot ^ 1u) : 0u;
      a.map_n = (unsigned)n_next; a.map_ids = (const i64*)ids_next; a.map_blocks = (unsigned)((n_next + MAP_SEG - 1) / MAP_SEG);
      a.map_out = reinterpret_cast<uint4*>(d->mapbuf + (size_t)ms * d->map_cap * 16);
      map_slot_new = (int)ms;   // (the driver's record of the list is made behind the launch: an error return in between must not arm it)
    }
    // the next batch's plan: its pairs were scattered by the previous call's launch -> this launch builds the table; else a launch of its own, in front
    if (n_next) {
      if (plan_next->scat_ids == ids_next && plan_next->scat_n == n_next && !(d->variant & 8)) {
        setplan_take_listless(plan_next, n_next);
        a.build_ent = plan_next->set_tab[plan_next->set_parity].ent; a.build_m2 = plan_next->set_m2; a.build_tiles = plan_next->seg_tiles; a.build_blocks = plan_next->set_m2 / SET_WIN;
        a.build_pairs = plan_next->seg_pairs; a.build_cnt = plan_next->seg_cnt; a.build_ovf = plan_next->ovf_pairs;
        a.build_ovf_cnt = plan_next->ovf_cnt + 32 * (plan_next->scat_use & 1u);
        a.build_ucnt = plan_next->ucnt;
        d->n_built_in_launch += 1;
      } else {
        rc = setplan_build(plan_next, n_next, ids_next, s, false);
        if (rc) return rc;
        d->n_built_in_front += 1;
      }
      plan_next->scat_ids = nullptr; plan_next->scat_n = 0;
    }
    // the batch after next: its distinct (id, last position) pairs go into plan_next2's segments
    if (n_next2 && !(d->variant & 8)) {
      rc = setplan_prepare_listless(plan_next2, n_next2, s);
      if (rc) return rc;
      plan_next2->scat_use += 1;
      a.scat_n = (unsigned)n_next2; a.scat_ids = (const i64*)ids_next2; a.scat_m2 = plan_next2->set_m2;
      a.scat_tiles = (unsigned)((n_next2 + 1023) / 1024); a.scat_blocks = a.scat_tiles;
      a.scat_pairs = plan_next2->seg_pairs; a.scat_cnt = plan_next2->seg_cnt; a.scat_ovf = plan_next2->ovf_pairs;
      a.scat_ovf_cnt = plan_next2->ovf_cnt + 32 * (plan_next2->scat_use & 1u);
      a.scat_ovf_cnt_next = plan_next2->ovf_cnt + 32 * ((plan_next2->scat_use & 1u) ^ 1u);
      plan_next2->seg_tiles = a.scat_tiles; plan_next2->scat_ids = ids_next2; plan_next2->scat_n = n_next2;
    }
    if (plan_prev && d->last_tail_step + 1 != step) {   // the launch before had no tail: nobody has zeroed this launch's counters
      if (hipMemsetAsync(a.patch_count, 0, 4, s) != hipSuccess || hipMemsetAsync(a.sync, 0, 1280, s) != hipSuccess) return set_error(TFRA_ERR_HIP, "step_overlap: memset");
    }
    if (plan_prev) d->last_tail_step = step;
    const bool timed = d->kev_left > 0 && plan_prev;
    if (timed) (void)hipEventRecord(d->kev[d->kev_used * 3], s);
    {
      // ONE launch: the lookup runs beside the write-back (forwarding, deferred evictions, corrections).  (Measured against it, on
      // the metric's configuration: the same roles as TWO launches one after the other — write-back + tail, then lookup + plan
      // builders, no forwarding — 52 us per step against 33: the write-back alone in its launch still takes 25 us.)
      const unsigned grid = a.build_blocks + a.scat_blocks + a.map_blocks + a.own_blocks + a.find_blocks + a.tail_blocks;
      if (d->tbuf) { unsigned* ti = d->tinfo[step % TIMING_SLOTS]; ti[0] = a.build_blocks; ti[1] = a.scat_blocks; ti[2] = a.own_blocks; ti[3] = a.find_blocks; ti[4] = grid; ti[5] = a.map_blocks; ti[6] = a.find_first; }
      launch_step(d->variant, grid, s, a, t->opts.strategy == TFRA_EVICT_LRU);
      if (timed) (void)hipEventRecord(d->kev[d->kev_used * 3 + 1], s);
    }
    if (timed) { (void)hipEventRecord(d->kev[d->kev_used * 3 + 2], s); d->kev_used += 1; d->kev_left -= 1; }
    if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "step_overlap: launch failed");
    if (map_slot_new >= 0) {
      d->map_slot = (unsigned)map_slot_new; d->map_valid = true; d->map_ids = ids_next; d->map_n = n_next; d->map_plan = plan_cur; d->map_gen = plan_cur->gen;
    }
    if (plan_prev) t->step_epoch();
    d->n_overlapped += 1;
  }
  d->pending = n > 0;
  d->pend_slot = slot; d->pend_ids = ids; d->pend_n = n;
  if (n_next) { d->ahead = true; d->ahead_ids = ids_next; d->ahead_n = n_next; }
  if (n) d->seq += 1;
  return TFRA_OK;
}

extern "C" int tfra_table_step_overlap(tfra_step_driver_t* d, size_t n, const int64_t* ids, void* rows_out, uint8_t* exists_out,
                                       const void* defaults, int default_is_full, const void* values_prev, const uint64_t* scores_prev,
                                       size_t n_next, const int64_t* ids_next, size_t n_next2, const int64_t* ids_next2, tfra_stream_t stream) {
  if (!d) return set_error(TFRA_ERR_INVALID, "step_overlap: null driver");
  if (!n) return set_error(TFRA_ERR_INVALID, "step_overlap: empty batch (tfra_table_step_overlap_flush writes a pending batch back)");
  std::lock_guard<std::mutex> step_lock(d->t->step_mu);
  return step_overlap_one(d, n, ids, rows_out, exists_out, defaults, default_is_full, values_prev, scores_prev, n_next, ids_next, n_next2, ids_next2,
                          (hipStream_t)stream);
}

extern "C" int tfra_table_steps_overlap(tfra_step_driver_t* d, size_t count, const tfra_overlap_step* steps, tfra_stream_t stream) {
  if (!d || (count && !steps)) return set_error(TFRA_ERR_INVALID, "steps_overlap: null argument");
  std::lock_guard<std::mutex> step_lock(d->t->step_mu);
  for (size_t i = 0; i < count; ++i) {
    const tfra_overlap_step& q = steps[i];
    if (q.struct_size != sizeof(tfra_overlap_step)) return set_error(TFRA_ERR_INVALID, "steps_overlap: struct_size mismatch");
    if (!q.n) return set_error(TFRA_ERR_INVALID, "steps_overlap: empty batch");
    int rc = step_overlap_one(d, q.n, q.ids, q.rows_out, q.exists_out, q.defaults, q.default_is_full, q.values_prev, q.scores_prev, q.n_next,
                              q.ids_next, q.n_next2, q.ids_next2, (hipStream_t)stream);
    if (rc) return rc;
  }
  return TFRA_OK;
}

extern "C" int tfra_table_step_overlap_flush(tfra_step_driver_t* d, const void* values_prev, const uint64_t* scores_prev, tfra_stream_t stream) {
  if (!d) return set_error(TFRA_ERR_INVALID, "step_overlap_flush: null driver");
  std::lock_guard<std::mutex> step_lock(d->t->step_mu);
  if (!d->pending) return TFRA_OK;
  if (!values_prev) return set_error(TFRA_ERR_INVALID, "step_overlap_flush: null values_prev");
  // the pending write-back alone: a step without a lookup (its launch holds the ownership pass only), or the planned upsert
  return step_overlap_one(d, 0, nullptr, nullptr, nullptr, nullptr, 0, values_prev, scores_prev, 0, nullptr, 0, nullptr, (hipStream_t)stream);
}

