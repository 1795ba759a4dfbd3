// Write-back of a batch whose ids MAY repeat, organised as CSR-by-key.
//
// Reference: the gradients of duplicate ids are summed, then ONE update per key
// (`_resource_apply_sparse_duplicate_indices` = unique + unsorted_segment_sum,
// PY/dynamic_embedding_optimizer.py:177-190) followed by (1+S) finds + dense apply + (1+S) upserts
// (:165-204); a plain upsert of a batch with repeats keeps the LAST occurrence
// (LaunchTensorsInsert on one thread, K/cuckoo_hashtable_op.cc:104-140).
//
// A Zipf-1.2 batch of 131 072 ids is extremely bimodal: ~790 keys occur more than 8 times and hold
// ~100 000 of the positions (the hottest ~24 000), the other ~21 000 keys share the remaining ~30 000.
//
//   PLAN (id-only, tfra_sparse_plan_build; any stream, typically one batch ahead on a second stream)
//     csr_tile_kernel    one block per 512 ids: equal ids grouped with an LDS hash; one descriptor
//                        (key, tile, count, where the tile keeps the positions) per distinct key of the tile,
//                        appended to the key's merge bucket (hash of the key).
//     csr_bucket_kernel  one block per bucket: groups its descriptors by key, orders a key's descriptors by tile
//                        (per-key tile table + wave scans), and emits
//                          cold keys (<= 8 occurrences): (key, first, count) + their batch positions, ascending;
//                          hot keys: their positions laid out in BINS of 512 entries — every 512 consecutive
//                            occurrences of a key fill one bin, the remainder (< 512, padded to 16) shares a bin
//                            with other remainders, never straddling — and (key, first partial, #partials).
//     csr_finish_kernel  publishes the counts, re-arms the cursors for the next build.
//   GRADIENT HALF (tfra_table_apply_planned; tfra_apply.hip, the bodies in tfra_apply_device.h)
//     hot_sums_kernel    one block per bin: 32 groups x 16 rows in flight, ordered add -> one partial row per run
//     apply_csr_kernel   one 16-lane group per unique key (hot keys first): gathers its <= 8 gradient rows or
//                        its partial rows IN ORDER, sums, locates/claims the table row, applies the optimizer.
//   ASSIGN (tfra_table_upsert_planned; tfra_own.hip): upsert_own_kernel (one pass with bucket ownership) + upsert_rest_kernel (the few
//     keys that pass leaves over) copy the row of every key's LAST occurrence (no sums, any value dtype); the assign-only
//     plan (dim 0: the SET plan, setplan_kernel) is one kernel — distinct ids with their last position — and lives in
//     tfra_setplan.hip with the unique ops built on it.  This unit keeps the plan object's life and tfra_sparse_plan_read.
//
// Round 3, tried and dropped (measured on the 10^9-slot table, B = 131 072 Zipf-1.2; each is in the git history as one
// experiment, none in the code):
//   * the remainder pass deferred to the table's next call and taken into the lookup's kernel (its first 32 blocks run the
//     list, every block waits for them when the list is not empty): a lookup kernel that holds the remainder's code needs
//     81 registers instead of 57 (6 instead of 8 waves per SIMD, or spills on the remainder's path), an agent-scope acquire
//     per waiting block is an L2 invalidate each (60 us per launch), 2000 blocks polling one word take 300 us, and while the
//     blocks wait they hold every wave slot, so the plan kernel of the second stream cannot run beside them: 48-51 us per
//     step against 47; only a sequence whose lists are always empty gained (34 -> 28 us);
//   * keys that lost a claim handled inside the pass (found keys lock their own slot, evictions take their victim by
//     compare-and-swap): correct, 45 % of the lists become empty, but the remainder kernel costs the same 8 us with one item
//     as with sixteen, and the swaps cost the pass 1.5-3 us on batches that evict;
//   * the assign-only plan partitioned by KEY (every block reads all ids and keeps its hash range: no global hash table, no
//     device-scope atomics): one CU streams 1 MB of ids in >= 7 us — 73 us as written, ~13 us at best, against 16 us;
//   * the hot sums as the leading blocks of their consumer kernel (keys with partial rows wait for them): the bin part has
//     to acknowledge its write-through rows before it may count itself done and shares the consumer's registers — 22 us
//     instead of 12 inside a step, and the keys that need it cannot start before it ends: 37-45 us against 38.
//
// Summation tree of a key = f(its occurrence count) only: [16 consecutive occurrences, ascending batch position,
// sequential] -> [the 32 groups of a bin, sequential] -> [the key's partials, sequential]; keys with <= 8
// occurrences are summed strictly in batch order (bit-identical to the reference's sequential sum).  WHERE a
// key's records land (atomic cursors) differs from run to run, the values do not: results are bit-reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tfra_mi355x.h"
#include "tfra_device.h"
#include "tfra_frontend.h"
#include "tfra_host.h"
#include "tfra_many.h"
#include "tfra_plan.h"
#include "tfra_reduce_device.h"

using namespace tfra;
using namespace tfra::red;

namespace {

// ---------------------------------------------------------------------------------------------
// The three plan kernels' bodies take `blk`, the block's index among the blocks of THIS plan: blockIdx.x in the single build's
// kernels, blockIdx.x minus the plan's first block in the grouped build's (csr_*_many_kernel), where the duties of "block 0" fall
// to the first block of each plan.
// plan kernel 1: per tile of 512 ids.
__device__ __forceinline__ void csr_tile_body(const unsigned blk, size_t n, const i64* __restrict__ ids, unsigned P, unsigned cm,
                                              const CsrDesc ds, unsigned* err, unsigned* __restrict__ tile_entries,
                                              unsigned short* __restrict__ run_start, unsigned* __restrict__ tile_len,
                                              u64* counters) {
  // the allocation counters of this build start at zero (the bucket kernel, next on the stream, uses them)
  if (blk == 0 && threadIdx.x <= NSH) counters[(size_t)threadIdx.x * CTR_STRIDE] = 0;
  constexpr unsigned GCAP = 2048;            // group table: 4x the tile => short probe chains
  constexpr int W = TILE / 32;               // words of a position bitmask
  constexpr int GM = GCAP / W;               // multi-member groups ranked per round (mask area = s_owner)
  __shared__ i64 s_key[TILE];
  __shared__ unsigned s_owner[GCAP];         // group table; afterwards the position masks
  __shared__ unsigned s_rep[GCAP];           // smallest input position of the group; later (m << 16 | base)
  __shared__ unsigned s_cnt[GCAP];
  __shared__ unsigned short s_list[TILE];    // positions of the multi-member groups, run after run, ascending
  __shared__ unsigned short s_run[TILE];     // ... and the run (multi-member group) each list entry belongs to
  __shared__ int s_scan[NTA / 64];
  unsigned* const s_mask = s_owner;
  const size_t tile = blk, base = tile * TILE;
  const int nvalid = (int)min((size_t)TILE, n - base);
  const int p = threadIdx.x;
  const bool ok = p < nvalid;
  const i64 key = ok ? ids[base + p] : 0;
  s_key[p] = key;
  for (unsigned b = threadIdx.x; b < GCAP; b += NTA) { s_owner[b] = 0; s_rep[b] = 0xffffffffu; s_cnt[b] = 0; }
  __syncthreads();
  unsigned slot = 0;
  if (ok) {
    slot = lds_group_slot(s_key, s_owner, GCAP, p, fmix64((u64)key));
    atomicMin(&s_rep[slot], (unsigned)p);
    atomicAdd(&s_cnt[slot], 1u);
  }
  __syncthreads();
  const bool head = ok && s_rep[slot] == (unsigned)p;
  const unsigned cnt = ok ? s_cnt[slot] : 0;
  const bool mhead = head && cnt > 1;
  int n_multi, L;
  const int m = block_excl_scan<NTA>(mhead ? 1 : 0, s_scan, &n_multi);
  const int lbase = block_excl_scan<NTA>(mhead ? (int)cnt : 0, s_scan, &L);
  // descriptor append: the returning atomic is issued now and consumed after the ranking rounds
  unsigned desc_pos = 0, desc_bucket = 0;
  if (head) {
    desc_bucket = (unsigned)__umul64hi(fmix64((u64)key), (u64)P);
    desc_pos = atomicAdd(&ds.cursor[(size_t)desc_bucket * CSTRIDE], 1u);
  }
  if (mhead) s_rep[slot] = ((unsigned)m << 16) | (unsigned)lbase;
  __syncthreads();  // s_rep maps slot -> (m, base) for multi groups; s_owner is free
  for (int c0 = 0; c0 < n_multi; c0 += GM) {
    for (unsigned q = threadIdx.x; q < GCAP; q += NTA) s_mask[q] = 0;
    __syncthreads();
    const int mm = (ok && cnt > 1) ? (int)(s_rep[slot] >> 16) - c0 : -1;
    if (mm >= 0 && mm < GM) atomicOr(&s_mask[mm * W + (p >> 5)], 1u << (p & 31));
    __syncthreads();
    if (mm >= 0 && mm < GM) {
      int rank = __popc(s_mask[mm * W + (p >> 5)] & ((1u << (p & 31)) - 1u));
      for (int wds = 0; wds < (p >> 5); ++wds) rank += __popc(s_mask[mm * W + wds]);
      s_list[(int)(s_rep[slot] & 0xffffu) + rank] = (unsigned short)p;  // ascending input position inside the run
      s_run[(int)(s_rep[slot] & 0xffffu) + rank] = (unsigned short)(s_rep[slot] >> 16);
    }
    __syncthreads();
  }
  if (head) {
    const unsigned where = cnt == 1 ? (unsigned)p : (unsigned)m;
    if (cnt > 1) run_start[base + m] = (unsigned short)lbase;
    const unsigned ordv = ((unsigned)tile << 18) | (where << 9) | (cnt - 1);
    if (desc_pos < cm) {
      size_t d = (size_t)desc_bucket * CMAX + desc_pos;
      ds.key[d] = key; ds.ord[d] = ordv;
    } else {
      unsigned o = atomicAdd(ds.ovf_count, 1u);
      if (o < ds.ovf_cap) { ds.ovf_key[o] = key; ds.ovf_ord[o] = ordv; ds.ovf_bucket[o] = desc_bucket; }
      else atomicAdd(err, 1u);
    }
  }
  // the tile keeps its own member lists: csr_scatter_kernel moves them once the bucket kernel has said where to
  for (int q = threadIdx.x; q < L; q += NTA) tile_entries[base + q] = (unsigned)s_list[q] | ((unsigned)s_run[q] << 9);
  if (threadIdx.x == 0) tile_len[tile] = (unsigned)L;
}

__global__ __launch_bounds__(NTA) void csr_tile_kernel(size_t n, const i64* __restrict__ ids, unsigned P, unsigned cm,
                                                       CsrDesc ds, unsigned* err,
                                                       unsigned* __restrict__ tile_entries,
                                                       unsigned short* __restrict__ run_start,
                                                       unsigned* __restrict__ tile_len, u64* counters) {
  csr_tile_body(blockIdx.x, n, ids, P, cm, ds, err, tile_entries, run_start, tile_len, counters);
}

// ---------------------------------------------------------------------------------------------
// plan kernel 2: per merge bucket.  Dynamic LDS: cm*36 + TABW*4 bytes.
__device__ __forceinline__ void csr_bucket_body(const unsigned blk, unsigned P, unsigned ntiles, unsigned cm, const CsrDesc ds,
                                                uint4* __restrict__ drec, const CsrOut out, unsigned* err) {
  extern __shared__ unsigned char smem[];
  i64* const e_key = reinterpret_cast<i64*>(smem);            // [cm] descriptors of the pass
  unsigned* const e_ord = reinterpret_cast<unsigned*>(e_key + cm);
  unsigned* const s_owner = e_ord + cm;                         // [cm] group table (1 + claiming descriptor)
  unsigned* const s_ct = s_owner + cm;                          // [cm] per group: #descriptors | entries << 11
  unsigned* const s_pref = s_ct + cm;                           // [cm] per descriptor: entries of its key in earlier tiles
  unsigned* const s_a = s_pref + cm;                            // [cm] per group: allocation, see below
  unsigned* const s_b = s_a + cm;
  unsigned* const s_tab = s_b + cm;                             // [TABW] tile table of the multi-descriptor keys
  unsigned short* const s_slot = reinterpret_cast<unsigned short*>(s_tab + TABW);  // [cm] group of each descriptor
  unsigned short* const s_hot = s_slot + cm;                    // [cm] head descriptors of the hot keys
  __shared__ int s_scan[NT / 64];
  __shared__ unsigned s_nhot, s_nshared, s_hot_ok;
  __shared__ unsigned s_cold_ok;
  __shared__ unsigned sh_ckbase, sh_hkbase, sh_pbase, sh_bbase;
  const unsigned b = blk;
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = threadIdx.x >> 4, wv = threadIdx.x >> 6;
  const int n_b = (int)ds.cursor[(size_t)b * CSTRIDE];
  if (n_b == 0) return;
  const unsigned n_ovf = n_b > (int)cm ? min(*ds.ovf_count, ds.ovf_cap) : 0u;
  const int n_reg = min(n_b, (int)cm);
  // A bucket with more descriptors than one pass holds (several very hot keys hashing together) is processed in
  // npass = 2^k passes, pass q taking the keys with (hash >> 40) & (npass-1) == q.  Emission goes through atomic
  // cursors and cannot be redone, so npass is fixed up front from a histogram of the 64 finest classes.
  unsigned npass = 1;
  if (n_b > (int)cm) {
    __shared__ unsigned s_hist[MAXPASS_SPLIT];
    __shared__ unsigned s_np;
    if (threadIdx.x < MAXPASS_SPLIT) s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < n_reg + (int)n_ovf; q += NT) {
      i64 k = 0; bool take = false;
      if (q < n_reg) { k = ds.key[(size_t)b * CMAX + q]; take = true; }
      else if (ds.ovf_bucket[q - n_reg] == b) { k = ds.ovf_key[q - n_reg]; take = true; }
      if (take) atomicAdd(&s_hist[(unsigned)(fmix64((u64)k) >> 40) & (MAXPASS_SPLIT - 1)], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned np = 2;
      for (; np < MAXPASS_SPLIT; np <<= 1) {
        unsigned worst = 0;
        for (unsigned c = 0; c < np; ++c) {
          unsigned sum = 0;
          for (unsigned j = c; j < MAXPASS_SPLIT; j += np) sum += s_hist[j];
          worst = max(worst, sum);
        }
        if (worst <= cm) break;
      }
      s_np = np;
    }
    __syncthreads();
    npass = s_np;
  }
  const unsigned ntile_pad = (ntiles + 63) & ~63u;         // table row length (<= 512)
  const int rows_per_round = (int)(TABW / ntile_pad);
  for (unsigned pass = 0; pass < npass; ++pass) {
    int n = 0;
    if (npass == 1) {
      for (int q = threadIdx.x; q < n_reg; q += NT) {
        size_t d = (size_t)b * CMAX + q;
        e_key[q] = ds.key[d]; e_ord[q] = ds.ord[d];
      }
      n = n_reg;
      __syncthreads();
    } else {  // filtered gather from the region and from the overflow list
      int carry = 0;
      bool too_many = false;
      for (int q0 = 0; q0 < n_reg + (int)n_ovf; q0 += NT) {
        int q = q0 + threadIdx.x;
        i64 k = 0; unsigned od = 0; bool take = false;
        if (q < n_reg) {
          size_t d = (size_t)b * CMAX + q;
          k = ds.key[d]; od = ds.ord[d]; take = true;
        } else if (q < n_reg + (int)n_ovf) {
          unsigned o = q - n_reg;
          if (ds.ovf_bucket[o] == b) { k = ds.ovf_key[o]; od = ds.ovf_ord[o]; take = true; }
        }
        take = take && (((unsigned)(fmix64((u64)k) >> 40) & (npass - 1)) == pass);
        int tot;
        int ex = block_excl_scan<NT>(take ? 1 : 0, s_scan, &tot);
        if (carry + tot > (int)cm) too_many = true;
        if (take && !too_many) { e_key[carry + ex] = k; e_ord[carry + ex] = od; }
        carry += tot;
      }
      __syncthreads();
      if (too_many) {  // even 64 classes are not enough (one key with > cm parts cannot happen: cm >= #tiles)
        if (threadIdx.x == 0) atomicAdd(err, 1u);
        continue;
      }
      n = carry;
    }
    if (n == 0) continue;
    // ---- group by key --------------------------------------------------------------------------
    for (unsigned q = threadIdx.x; q < cm; q += NT) { s_owner[q] = 0; s_ct[q] = 0; }
    if (threadIdx.x == 0) { s_nhot = 0; s_nshared = 0; s_hot_ok = 1; }
    __syncthreads();
    for (int q = threadIdx.x; q < n; q += NT) {
      unsigned slot = lds_group_slot(e_key, s_owner, cm, q, fmix64((u64)e_key[q]));
      atomicAdd(&s_ct[slot], 1u | (((e_ord[q] & 511u) + 1u) << 11));
      s_slot[q] = (unsigned short)slot;
      s_pref[q] = 0;
    }
    __syncthreads();
    // ---- entries of the same key in EARLIER tiles, for the keys with more than one descriptor: a row of
    //      per-tile counts per key, exclusive wave scan along the row -------------------------------
    int n_multi = 0;
    for (int pb = 0; pb < n; pb += NT) {
      int q = pb + threadIdx.x;
      unsigned slot = q < n ? s_slot[q] : 0;
      bool mh = q < n && s_owner[slot] - 1 == (unsigned)q && (s_ct[slot] & 2047u) > 1;
      int tm;
      int em = block_excl_scan<NT>(mh ? 1 : 0, s_scan, &tm);
      if (mh) s_a[slot] = (unsigned)(n_multi + em);
      n_multi += tm;
    }
    __syncthreads();
    for (int c0 = 0; c0 < n_multi; c0 += rows_per_round) {
      const int nrows = min(rows_per_round, n_multi - c0);
      for (unsigned q = threadIdx.x; q < (unsigned)nrows * ntile_pad; q += NT) s_tab[q] = 0;
      __syncthreads();
      for (int q = threadIdx.x; q < n; q += NT) {
        unsigned slot = s_slot[q];
        if ((s_ct[slot] & 2047u) > 1) {
          int mrow = (int)s_a[slot] - c0;
          if (mrow >= 0 && mrow < nrows) s_tab[mrow * ntile_pad + (e_ord[q] >> 18)] = (e_ord[q] & 511u) + 1u;
        }
      }
      __syncthreads();
      const unsigned epl = ntile_pad / 64;   // elements per lane (<= 8)
      for (int mrow = wv; mrow < nrows; mrow += NT / 64) {
        unsigned* row = s_tab + mrow * ntile_pad + lane * epl;
        unsigned loc = 0;
        for (unsigned e = 0; e < epl; ++e) loc += row[e];
        unsigned incl = loc;
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
          unsigned t2 = (unsigned)__shfl_up((int)incl, o2);
          if (lane >= o2) incl += t2;
        }
        unsigned run = incl - loc;
        for (unsigned e = 0; e < epl; ++e) { unsigned c = row[e]; row[e] = run; run += c; }
      }
      __syncthreads();
      for (int q = threadIdx.x; q < n; q += NT) {
        unsigned slot = s_slot[q];
        if ((s_ct[slot] & 2047u) > 1) {
          int mrow = (int)s_a[slot] - c0;
          if (mrow >= 0 && mrow < nrows) s_pref[q] = s_tab[mrow * ntile_pad + (e_ord[q] >> 18)];
        }
      }
      __syncthreads();
    }
    // ---- allocation.  keys with few occurrences: a block scan; the others (few keys): thread 0 ------------
    //   few : s_a = rank among the pass's such keys
    //   many: s_a = first partial (relative) | first full bin (relative) << 16, s_b = first 16-entry item of the remainder
    int nck = 0;
    for (int pb = 0; pb < n; pb += NT) {
      int q = pb + threadIdx.x;
      unsigned slot = q < n ? s_slot[q] : 0;
      bool hd = q < n && s_owner[slot] - 1 == (unsigned)q;
      unsigned tot = hd ? (s_ct[slot] >> 11) : 0;
      bool cold = hd && tot <= (unsigned)DIRECT;
      int tt;
      int ex = block_excl_scan<NT>(cold ? 1 : 0, s_scan, &tt);
      if (cold) s_a[slot] = (unsigned)(nck + ex);
      if (hd && !cold) { unsigned i = atomicAdd(&s_nhot, 1u); s_hot[i] = (unsigned short)q; }
      nck += tt;
    }
    __syncthreads();
    const unsigned shard = b & (NSH - 1);
    if (threadIdx.x == 0) {
      const unsigned nh = s_nhot;
      unsigned nshared = 0, used = 32, nfulltot = 0, npart = 0;
      for (unsigned i = 0; i < nh; ++i) {
        const unsigned slot = s_slot[s_hot[i]];
        const unsigned tot = s_ct[slot] >> 11, nfull = tot >> 9, rem = tot & 511u, it = (rem + 15) >> 4;
        unsigned remitem = 0;
        if (rem) {
          if (used + it > 32) { nshared++; used = 0; }
          remitem = (nshared - 1) * 32 + used;
          used += it;
        }
        s_a[slot] = npart | (nfulltot << 16);
        s_b[slot] = remitem;
        nfulltot += nfull;
        npart += nfull + (rem ? 1 : 0);
      }
      const unsigned nbins = nshared + nfulltot;
      const u64 c = atomicAdd(&out.counters[(size_t)shard * CTR_STRIDE],
                              (u64)nck | ((u64)nh << 16) | ((u64)npart << 32) | ((u64)nbins << 48));
      sh_ckbase = (unsigned)(c & 0xffffu); sh_hkbase = (unsigned)((c >> 16) & 0xffffu);
      sh_pbase = (unsigned)((c >> 32) & 0xffffu); sh_bbase = (unsigned)(c >> 48);
      s_nshared = nshared;
      // a shard's range is sized for twice its fair share (+ the single-key worst case for bins / partials): only a
      // pathological hash skew gets here; the keys are skipped and the build reports the error
      s_cold_ok = sh_ckbase + nck <= out.cr;
      s_hot_ok = sh_hkbase + nh <= out.hr && sh_pbase + npart <= out.pr && sh_bbase + nbins <= out.br;
      if (!s_cold_ok || (nh && !s_hot_ok)) atomicAdd(err, 1u);
    }
    __syncthreads();
    const unsigned nh = s_nhot, nshared = s_nshared;
    const bool hot_ok = s_hot_ok != 0, cold_ok = s_cold_ok != 0;
    const unsigned ckbase = shard * out.cr + sh_ckbase, hkbase = shard * out.hr + sh_hkbase,
                   pbase = shard * out.pr + sh_pbase, bbase = shard * out.br + sh_bbase;
    // shared bins start as "nothing here": every 16-entry item is its own empty run
    if (hot_ok)
      for (unsigned q = threadIdx.x; q < nshared * SEG; q += NT)
        out.hent[(size_t)bbase * SEG + q] = E_SKIP | ((q & 15u) == 0 ? E_HEAD : 0u);
    // key records
    if (cold_ok) {
      for (int q = threadIdx.x; q < n; q += NT) {
        unsigned slot = s_slot[q];
        if (s_owner[slot] - 1 != (unsigned)q) continue;
        unsigned tot = s_ct[slot] >> 11;
        if (tot <= (unsigned)DIRECT) {
          unsigned* rec = out.crec + (size_t)(ckbase + s_a[slot]) * REC_WORDS;
          rec[0] = (unsigned)(u64)e_key[q]; rec[1] = (unsigned)((u64)e_key[q] >> 32); rec[2] = tot;
        }
      }
    }
    if (hot_ok) {
      for (unsigned i = threadIdx.x; i < nh; i += NT) {
        const int q = s_hot[i];
        const unsigned slot = s_slot[q];
        const unsigned tot = s_ct[slot] >> 11, nfull = tot >> 9, rem = tot & 511u;
        const unsigned partrel = s_a[slot] & 0xffffu, fullrel = s_a[slot] >> 16, remitem = s_b[slot];
        const unsigned fullbin0 = bbase + nshared + fullrel;
        const unsigned last_addr = rem ? (bbase * SEG + remitem * 16 + rem - 1) : ((fullbin0 + nfull - 1) * SEG + SEG - 1);
        unsigned* rec = out.hrec + (size_t)(hkbase + i) * REC_WORDS;
        rec[0] = (unsigned)(u64)e_key[q]; rec[1] = (unsigned)((u64)e_key[q] >> 32); rec[2] = tot;
        rec[3] = pbase + partrel; rec[4] = nfull + (rem ? 1 : 0); rec[5] = last_addr;
        for (unsigned j = 0; j < nfull; ++j) out.hout[(size_t)(fullbin0 + j) * 32] = pbase + partrel + j;
        if (rem) out.hout[(size_t)bbase * 32 + remitem] = pbase + partrel + nfull;
      }
    }
    __syncthreads();   // the SKIP fill above is ordered before the entries below
    // ---- entries: descriptor (tile, where, c) owns entries [pref, pref + c) of its key ----------------
    auto write_entry = [&](unsigned slot, unsigned e, unsigned position) {
      const unsigned tot = s_ct[slot] >> 11;
      if (tot <= (unsigned)DIRECT) {
        if (cold_ok) {
          unsigned* rec = out.crec + (size_t)(ckbase + s_a[slot]) * REC_WORDS;
          rec[4 + e] = position;
          if (e + 1 == tot) rec[3] = position;   // the key's last occurrence (positions ascend with e)
        }
      } else if (hot_ok) {
        const unsigned nfull = tot >> 9, fullrel = s_a[slot] >> 16;
        size_t addr;
        bool hd;
        if (e < nfull * SEG) { addr = (size_t)(bbase + nshared + fullrel) * SEG + e; hd = (e & (SEG - 1)) == 0; }
        else { addr = (size_t)bbase * SEG + s_b[slot] * 16 + (e - nfull * SEG); hd = e == nfull * SEG; }
        out.hent[addr] = position | (hd ? E_HEAD : 0u);
      }
    };
    for (int q = threadIdx.x; q < n; q += NT) {
      const unsigned od = e_ord[q];
      if ((od & 511u) == 0) write_entry(s_slot[q], s_pref[q], ((od >> 18) << 9) | ((od >> 9) & 511u));
    }
    // descriptors with count >= 2: where their member list goes (csr_scatter_kernel does the moving, one thread per
    // member, all tiles at once — the block of the hottest bucket alone would take ~100 dependent round trips)
    for (int q = threadIdx.x; q < n; q += NT) {
      const unsigned od = e_ord[q];
      if ((od & 511u) == 0) continue;
      const unsigned slot = s_slot[q], tot = s_ct[slot] >> 11, e0 = s_pref[q];
      uint4 r;
      if (tot <= (unsigned)DIRECT) r = cold_ok ? make_uint4((ckbase + s_a[slot]) * REC_WORDS + 4 + e0, 0u, 0u, 0xffffffffu)
                                               : make_uint4(0u, 0u, 0u, 0xfffffffeu);
      else if (hot_ok) r = make_uint4(e0, (bbase + nshared + (s_a[slot] >> 16)) * SEG, bbase * SEG + s_b[slot] * 16, tot >> 9);
      else r = make_uint4(0u, 0u, 0u, 0xfffffffeu);   // dropped (capacity error reported)
      drec[(size_t)(od >> 18) * TILE + ((od >> 9) & 511u)] = r;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NT) void csr_bucket_kernel(unsigned P, unsigned ntiles, unsigned cm, CsrDesc ds,
                                                        uint4* __restrict__ drec, CsrOut out, unsigned* err) {
  csr_bucket_body(blockIdx.x, P, ntiles, cm, ds, drec, out, err);
}

// plan kernel 3 (the last one): per tile again.
//  (a) every member of a multi-member run goes to the place csr_bucket_kernel chose for its descriptor:
//      entry e = e0 + (rank inside the run) of its key;
//  (b) dense maps over the allocation shards: keymap[g] = record of the g-th unique key (keys with many occurrences
//      first), binmap[i] = i-th bin;
//  (c) block 0: publishes the counts (device copy for the kernels of the other half, pinned host copy for the
//      driver), re-arms the bucket cursors for the next build, latches the errors.
//      The published words: PC_* of tfra_plan_device.h.
__device__ __forceinline__ void csr_scatter_body(const unsigned blk, const unsigned* __restrict__ tile_entries,
                                                 const unsigned short* __restrict__ run_start,
                                                 const unsigned* __restrict__ tile_len, const uint4* __restrict__ drec,
                                                 const CsrOut out, unsigned* __restrict__ keymap, i64* __restrict__ dkeys,
                                                 unsigned* __restrict__ binmap, unsigned* cursors, unsigned P,
                                                 unsigned* d_counts, unsigned* host_counts, unsigned gen) {
  __shared__ unsigned s_hpre[NSH + 1], s_cpre[NSH + 1], s_bpre[NSH + 1];
  if (threadIdx.x < 64) {   // wave 0: prefix sums of the shards' counts (clamped to the shard capacities)
    const unsigned sh = threadIdx.x;
    const u64 c = out.counters[(size_t)sh * CTR_STRIDE];
    const unsigned nc = min((unsigned)(c & 0xffffu), out.cr), nh = min((unsigned)((c >> 16) & 0xffffu), out.hr),
                   nb = min((unsigned)(c >> 48), out.br);
    unsigned ic = nc, ih = nh, ib = nb;
    for (int o2 = 1; o2 < 64; o2 <<= 1) {
      unsigned tc = (unsigned)__shfl_up((int)ic, o2), th = (unsigned)__shfl_up((int)ih, o2), tb = (unsigned)__shfl_up((int)ib, o2);
      if ((int)sh >= o2) { ic += tc; ih += th; ib += tb; }
    }
    s_cpre[sh + 1] = ic; s_hpre[sh + 1] = ih; s_bpre[sh + 1] = ib;
    if (sh == 0) { s_cpre[0] = 0; s_hpre[0] = 0; s_bpre[0] = 0; }
  }
  __syncthreads();
  const unsigned nhot = s_hpre[NSH], ncold = s_cpre[NSH], nbins = s_bpre[NSH];
  auto shard_of = [](const unsigned* pre, unsigned x) {   // largest s with pre[s] <= x
    unsigned lo = 0;
    for (unsigned step = NSH / 2; step > 0; step >>= 1) if (pre[lo + step] <= x) lo += step;
    return lo;
  };
  const unsigned gid = blk * NTA + threadIdx.x;
  // dkeys[g] = the key itself: the write-back kernels start the table probe from it while keymap -> record resolves
  if (gid < nhot) {
    const unsigned sh = shard_of(s_hpre, gid), r = sh * out.hr + (gid - s_hpre[sh]);
    keymap[gid] = KM_MANY | r;
    dkeys[gid] = *reinterpret_cast<const i64*>(out.hrec + (size_t)r * REC_WORDS);
  } else if (gid < nhot + ncold) {
    const unsigned x = gid - nhot, sh = shard_of(s_cpre, x), r = sh * out.cr + (x - s_cpre[sh]);
    keymap[gid] = r;
    dkeys[gid] = *reinterpret_cast<const i64*>(out.crec + (size_t)r * REC_WORDS);
  }
  if (gid < nbins) {
    const unsigned sh = shard_of(s_bpre, gid);
    binmap[gid] = sh * out.br + (gid - s_bpre[sh]);
  }
  // (a)
  const size_t base = (size_t)blk * TILE;
  const int L = (int)tile_len[blk];
  const int q = threadIdx.x;
  if (q < L) {
    const unsigned te = tile_entries[base + q];
    const unsigned m = te >> 9, position = (unsigned)base + (te & 511u);
    const unsigned rank = (unsigned)q - run_start[base + m];
    const uint4 r = drec[base + m];
    if (r.w == 0xffffffffu) {
      const unsigned idx = r.x + rank, rb = idx & ~(REC_WORDS - 1);   // a record is 16 words, positions in words 4..11
      out.crec[idx] = position;
      if ((idx & (REC_WORDS - 1)) - 3 == out.crec[rb + 2]) out.crec[rb + 3] = position;   // the key's last occurrence
    } else if (r.w != 0xfffffffeu) {
      const unsigned e = r.x + rank, nfull = r.w;
      if (e < nfull * SEG) out.hent[(size_t)r.y + e] = position | ((e & (SEG - 1)) == 0 ? E_HEAD : 0u);
      else out.hent[(size_t)r.z + (e - nfull * SEG)] = position | (e == nfull * SEG ? E_HEAD : 0u);
    }
  }
  // (c) block 0: counts for the kernels of the other half (device copy) and for the host's grid sizes (pinned copy), cursors
  // re-armed for the next build, errors latched.  NOT a completion signal: other blocks are still scattering — whoever needs
  // the finished plan on another stream waits for the build's event (tfra_table_step_prefetch: hipEventQuery on the host), or
  // is ordered behind it by the stream.  (Round 2 treated the pinned generation as "plan complete" — ADVICE r2; a per-block
  // release + ticket here cost the kernel 8 us, the event costs nothing on the critical path.)
  if (blk == 0) {
    __syncthreads();
    for (unsigned i = threadIdx.x; i <= P; i += NTA) cursors[(size_t)i * CSTRIDE] = 0;   // bucket cursors + overflow count
    if (threadIdx.x == 0) {
      const unsigned e = cursors[(size_t)(P + 1) * CSTRIDE];
      cursors[(size_t)(P + 1) * CSTRIDE] = 0;
      unsigned v[PC_PUBLISHED] = {};
      v[PC_HOT] = nhot; v[PC_COLD] = ncold; v[PC_BINS] = nbins; v[PC_OVERFLOW] = e;
      for (unsigned k = 0; k < PC_PUBLISHED; ++k) d_counts[k] = v[k];
      *reinterpret_cast<i64*>(d_counts + PC_PART_COUNT) = (i64)nhot + (i64)ncold;   // tfra_plan_partition: the count as tfra_partition reads it
      if (host_counts) {
        for (unsigned k = 0; k < PC_PUBLISHED; ++k) __hip_atomic_store(host_counts + HC_SHIFT + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_counts + HC_GEN, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

__global__ __launch_bounds__(NTA) void csr_scatter_kernel(const unsigned* __restrict__ tile_entries,
                                                          const unsigned short* __restrict__ run_start,
                                                          const unsigned* __restrict__ tile_len,
                                                          const uint4* __restrict__ drec, CsrOut out,
                                                          unsigned* __restrict__ keymap, i64* __restrict__ dkeys,
                                                          unsigned* __restrict__ binmap, unsigned* cursors, unsigned P,
                                                          unsigned* d_counts, unsigned* host_counts, unsigned gen) {
  csr_scatter_body(blockIdx.x, tile_entries, run_start, tile_len, drec, out, keymap, dkeys, binmap, cursors, P, d_counts, host_counts,
                   gen);
}

// ---- the grouped build (tfra_multi_sparse_plan_build): the three kernels over a LIST of plans.  What a single build's kernels take
// as arguments is a record in device memory; a block finds its plan by many_desc_of (tfra_many.h) — blockIdx.x is wave-uniform, so
// the search and the record are scalar loads, as kernel arguments are — and runs the single build's body with its index inside the
// plan.  The kernels are block-per-work-item (a tile, a merge bucket, a tile) and no block waits for another, so plan d's blocks
// are exactly the single build's blocks: ntiles, P, ntiles.  The bucket launch is one class per cm (its dynamic LDS), reading the
// records through the class's index.
struct PlanManyRec {
  size_t n;
  const i64* ids;
  unsigned P, cm, ntiles, gen;
  CsrDesc ds;
  CsrOut out;
  unsigned* err;
  unsigned* tile_entries;
  unsigned short* run_start;
  unsigned* tile_len;
  uint4* drec;
  unsigned* keymap;
  i64* dkeys;
  unsigned* binmap;
  unsigned* cursors;
  unsigned* d_counts;
  unsigned* host_counts;
};

__global__ __launch_bounds__(NTA) void csr_tile_many_kernel(const PlanManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                            unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const PlanManyRec r = recs[d];
  csr_tile_body(blockIdx.x - prefix[d], r.n, r.ids, r.P, r.cm, r.ds, r.err, r.tile_entries, r.run_start, r.tile_len, r.out.counters);
}

__global__ __launch_bounds__(NT) void csr_bucket_many_kernel(const PlanManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                             const unsigned* __restrict__ idx, unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const PlanManyRec r = recs[idx[d]];
  csr_bucket_body(blockIdx.x - prefix[d], r.P, r.ntiles, r.cm, r.ds, r.drec, r.out, r.err);
}

__global__ __launch_bounds__(NTA) void csr_scatter_many_kernel(const PlanManyRec* __restrict__ recs, const unsigned* __restrict__ prefix,
                                                               unsigned n) {
  const unsigned d = many_desc_of(prefix, n, blockIdx.x);
  const PlanManyRec r = recs[d];
  csr_scatter_body(blockIdx.x - prefix[d], r.tile_entries, r.run_start, r.tile_len, r.drec, r.out, r.keymap, r.dkeys, r.binmap, r.cursors,
                   r.P, r.d_counts, r.host_counts, r.gen);
}

}  // namespace

extern "C" int tfra_sparse_plan_create(int device, tfra_sparse_plan_t** out) {
  if (!out) return set_error(TFRA_ERR_INVALID, "sparse_plan_create: null out");
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_create: no device");
  tfra_sparse_plan* pl = new tfra_sparse_plan();
  pl->device = device;
  *out = pl;
  return TFRA_OK;
}

extern "C" int tfra_sparse_plan_destroy(tfra_sparse_plan_t* pl) {
  if (!pl) return TFRA_OK;
  if (pl->buf || pl->setbuf || pl->segbuf) {
    (void)hipSetDevice(pl->device); (void)hipDeviceSynchronize();
    (void)hipFree(pl->buf); (void)hipFree(pl->setbuf); (void)hipFree(pl->segbuf);   // (a null pointer: nothing to free)
  }
  if (pl->host_counts) (void)hipHostFree(pl->host_counts);
  if (pl->built_ev) (void)hipEventDestroy(pl->built_ev);
  delete pl;
  return TFRA_OK;
}

static size_t plan_smem_bytes(unsigned cm) { return (size_t)cm * 36 + (size_t)TABW * 4; }


// The argument checks of a plan build, for the single call and for a descriptor of the grouped one (tfra_multi_sparse_plan_build).
// active: there are ids.  dim 0 (the SET plan) passes: the single call builds it, the grouped call refuses it at its entry.
template <class AtEntry>
static Check check_plan_build(const tfra_sparse_plan* pl, size_t n, const int64_t* ids, int dim, AtEntry&& at_entry) {
  if (!pl) return refuse(TFRA_ERR_INVALID, "null plan");
  if (Check e = at_entry(); e.done()) return e;
  if (n == 0) return nothing_to_do();
  if (!ids) return refuse(TFRA_ERR_INVALID, "null ids");
  if (dim != 0 && (dim < 0 || dim % 4 != 0 || dim > 64 * MAXCH))
    return refuse(TFRA_ERR_UNSUPPORTED, "needs dim % 4 == 0 and dim <= 256 (dim 0: assign-only plan)");
  if (n > MAX_IDS) return refuse(TFRA_ERR_UNSUPPORTED, "at most 2^18 ids per plan");
  return Check{};
}

// The host part of a CSR build, shared by the single and the grouped call, in three steps:
//   plan_layout   sizes only: tiles, merge buckets, the pass size, the shards' capacities, the buffer's sections;
//   plan_grow     the buffer, when the layout outgrew it — the ONLY step that can fail for lack of memory or synchronise (a
//                 replaced buffer is freed behind hipDeviceSynchronize); it enqueues nothing, and a plan whose buffer was
//                 replaced holds no build;
//   plan_lay_out  the plan's pointers into its buffer, gen += 1, and the memsets a build needs when the plan is not armed or
//                 its number of merge buckets changed (cursors, counters, counts) or the left-over flags moved.  In the
//                 steady state — armed, same layout — it enqueues nothing.
struct PlanLayout {
  size_t n, ntiles, npad;
  unsigned P, cm;
  int dim;
  unsigned cr, hr, pr, br;
  size_t reg, head, ctr, nrec_c, nrec_h, nbin, npart, bytes;
};

static PlanLayout plan_layout(size_t n, int dim) {
  PlanLayout L{};
  L.n = n; L.dim = dim;
  L.ntiles = (n + TILE - 1) / TILE; L.npad = L.ntiles * TILE;
  const size_t ntiles = L.ntiles, npad = L.npad;
  unsigned P = 64;
  while (P < 2048 && (size_t)P * 128 < n) P <<= 1;
  L.P = P;
  L.cm = ntiles <= 256 ? 512u : 1024u;   // a key present in every tile must fit one pass with room to spare
  L.reg = (size_t)P * CMAX;
  L.head = align_up((size_t)(P + 2) * CSTRIDE * 4);
  L.ctr = align_up((size_t)(NSH + 1) * CTR_STRIDE * 8);
  // per-shard capacities: twice the fair share + slack; bins / partial rows also cover ONE key holding every id
  L.cr = (unsigned)(2 * npad / NSH + 64);
  L.hr = (unsigned)(2 * (npad / 9) / NSH + 64);
  L.pr = (unsigned)(npad / SEG + 2 * (npad / 9) / NSH + 64);
  L.br = (unsigned)(npad / SEG + (npad / 16 + npad / 9) / NSH / 16 + 2 * (P / NSH + 1) + 32);
  L.nrec_c = (size_t)NSH * L.cr; L.nrec_h = (size_t)NSH * L.hr; L.nbin = (size_t)NSH * L.br; L.npart = (size_t)NSH * L.pr;
  const auto al = [](size_t x) { return align_up(x); };
  L.bytes = L.head + L.ctr + PC_WORDS * 4                                              // cursors, counters, d_counts
            + al(L.reg * 8) + al(L.reg * 4) + al(npad * 8) + 2 * al(npad * 4)          // descriptors + overflow list
            + al(npad * 4) + al(npad * 2) + al(ntiles * 4) + al(npad * 16)             // tile lists, run starts, lengths, destinations
            + al(L.nrec_c * REC_WORDS * 4) + al(L.nrec_h * REC_WORDS * 4)              // key records
            + al(L.nbin * SEG * 4) + al(L.nbin * 32 * 4)                               // bins + run outputs
            + al(npad * 4) + al(npad * 8) + al(L.nbin * 4)                             // keymap, dense keys, binmap
            + al(npad) + al((size_t)SLOW_CAP * sizeof(OwnItem))                        // deferred flags, left-over item list
            + al(L.npart * 4)                                                          // partial row -> destination (route helpers)
            + al(L.npart * (size_t)dim * 4);                                           // partial rows
  return L;
}

static int plan_grow(tfra_sparse_plan* pl, const PlanLayout& L) {
  if (pl->bytes >= L.bytes) return TFRA_OK;
  if (pl->buf) {
    if (hipDeviceSynchronize() != hipSuccess || hipFree(pl->buf) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: free");
    pl->buf = nullptr; pl->bytes = 0;
    if (pl->kind == 0) pl->n = 0;
  }
  hipError_t e = hipMalloc(&pl->buf, L.bytes);
  if (e != hipSuccess) { pl->buf = nullptr; return set_error(e == hipErrorOutOfMemory ? TFRA_ERR_OOM : TFRA_ERR_HIP, "sparse_plan_build: hipMalloc"); }
  pl->bytes = L.bytes;
  pl->armed = false;
  pl->dflag = nullptr;
  return TFRA_OK;
}

static int plan_lay_out(tfra_sparse_plan* pl, const PlanLayout& L, hipStream_t s) {
  const auto al = [](size_t x) { return align_up(x); };
  const size_t npad = L.npad;
  CsrOut& o = pl->out;
  o.cr = L.cr; o.hr = L.hr; o.pr = L.pr; o.br = L.br;
  unsigned char* w = (unsigned char*)pl->buf;
  pl->cursors = (unsigned*)w; w += L.head;
  o.counters = (u64*)w; w += L.ctr;
  pl->d_counts = (unsigned*)w; w += PC_WORDS * 4;
  const bool same_layout = pl->armed && pl->P == L.P;
  if (!same_layout && hipMemsetAsync(pl->buf, 0, L.head + L.ctr + PC_WORDS * 4, s) != hipSuccess)
    return set_error(TFRA_ERR_HIP, "sparse_plan_build: memset");
  CsrDesc& ds = pl->ds;
  ds.key = (i64*)w; w += al(L.reg * 8);
  ds.ord = (unsigned*)w; w += al(L.reg * 4);
  ds.ovf_key = (i64*)w; w += al(npad * 8);
  ds.ovf_ord = (unsigned*)w; w += al(npad * 4);
  ds.ovf_bucket = (unsigned*)w; w += al(npad * 4);
  pl->tile_entries = (unsigned*)w; w += al(npad * 4);
  pl->run_start = (unsigned short*)w; w += al(npad * 2);
  pl->tile_len = (unsigned*)w; w += al(L.ntiles * 4);
  pl->drec = (uint4*)w; w += al(npad * 16);
  o.crec = (unsigned*)w; w += al(L.nrec_c * REC_WORDS * 4);
  o.hrec = (unsigned*)w; w += al(L.nrec_h * REC_WORDS * 4);
  o.hent = (unsigned*)w; w += al(L.nbin * SEG * 4);
  o.hout = (unsigned*)w; w += al(L.nbin * 32 * 4);
  pl->keymap = (unsigned*)w; w += al(npad * 4);
  pl->dkeys = (i64*)w; w += al(npad * 8);
  pl->binmap = (unsigned*)w; w += al(L.nbin * 4);
  if (pl->dflag != (uint8_t*)w || pl->dflag_len != npad) {   // the left-over flags are all zero between launches (upsert_own_kernel)
    if (hipMemsetAsync(w, 0, al(npad), s) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: memset");
    pl->dflag_len = npad;
  }
  pl->dflag = (uint8_t*)w; w += al(npad);
  pl->slow_items = (OwnItem*)w; w += al((size_t)SLOW_CAP * sizeof(OwnItem));
  pl->any_deferred = pl->d_counts + PC_ANY_DEFERRED;
  pl->prow_dest = (int*)w; w += al(L.npart * 4);
  pl->partial = (float*)w;
  pl->gen += 1;
  ds.cursor = pl->cursors;
  ds.ovf_count = pl->cursors + (size_t)L.P * CSTRIDE;
  ds.ovf_cap = (unsigned)npad;
  return TFRA_OK;
}
// the error counter of a plan laid out for L.P merge buckets
static unsigned* plan_err_word(const tfra_sparse_plan* pl, unsigned P) { return pl->cursors + (size_t)(P + 1) * CSTRIDE; }
// ... and what the object remembers of a build whose launches were enqueued
static void plan_built(tfra_sparse_plan* pl, const PlanLayout& L) {
  pl->n = L.n; pl->npad = L.npad; pl->ntiles = L.ntiles; pl->P = L.P; pl->cm = L.cm; pl->dim = L.dim; pl->kind = 0;
}

extern "C" int tfra_sparse_plan_build(tfra_sparse_plan_t* pl, size_t n, const int64_t* ids, int dim, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  bool skip_counts = false;
  const Check c = check_plan_build(pl, n, ids, dim, [&] {
    skip_counts = pl->skip_counts_once;   // consumed here on EVERY path (an empty batch or an error must not leak it into the next build)
    pl->skip_counts_once = false;
    if (on_device(pl->device) != hipSuccess) return refuse(TFRA_ERR_HIP, "hipSetDevice");
    pl->n = 0;
    pl->ever_built = true;
    return Check{};
  });
  if (c.code) return report("sparse_plan_build: ", c);
  if (!c.active) return TFRA_OK;
  if (dim == 0) return setplan_build(pl, n, ids, s, !skip_counts);   // assign-only: the last position and the count of every distinct id
  const PlanLayout L = plan_layout(n, dim);
  int rc = plan_grow(pl, L);
  if (rc) return rc;
  if ((rc = plan_lay_out(pl, L, s))) return rc;
  const CsrDesc& ds = pl->ds;
  const CsrOut& o = pl->out;
  unsigned* err = plan_err_word(pl, L.P);
  csr_tile_kernel<<<dim3((unsigned)L.ntiles), NTA, 0, s>>>(n, (const i64*)ids, L.P, L.cm, ds, err, pl->tile_entries, pl->run_start, pl->tile_len, o.counters);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(csr_bucket_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)plan_smem_bytes(1024));
    attr_set = true;
  }
  csr_bucket_kernel<<<dim3(L.P), NT, plan_smem_bytes(L.cm), s>>>(L.P, (unsigned)L.ntiles, L.cm, ds, pl->drec, o, err);
  csr_scatter_kernel<<<dim3((unsigned)L.ntiles), NTA, 0, s>>>(pl->tile_entries, pl->run_start, pl->tile_len, pl->drec, o, pl->keymap,
                                                             pl->dkeys, pl->binmap, pl->cursors, L.P, pl->d_counts, pl->host_counts, pl->gen);
  pl->armed = true;
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_build: launch failed");
  plan_built(pl, L);
  return TFRA_OK;
}

// tfra_multi_sparse_plan_build: the CSR builds of a LIST of plans with launches that do not grow with the list (the frame of
// tfra_many.h: check every descriptor, classify, lay out, fill one blob, send it, launch).  Everything that can fail for an
// argument or for memory, or that synchronises — the checks of ALL descriptors, every plan's buffer (plan_grow), the workspace and
// its staging slot (many_begin) — comes before the first enqueue.
namespace {
Check check_plan_desc(const tfra_plan_build_desc& d, const tfra_workspace* ws) {
  if (d.struct_size != sizeof(tfra_plan_build_desc)) return refuse(TFRA_ERR_INVALID, "descriptor size mismatch");
  return check_plan_build(d.plan, d.n, d.ids, d.dim, [&] {
    if (d.plan->device != ws->device) return refuse(TFRA_ERR_INVALID, "workspace and plan live on different devices");
    if (d.dim == 0) return refuse(TFRA_ERR_UNSUPPORTED, "the assign-only plan (dim 0) is one kernel already and is not grouped");
    return Check{};
  });
}
}  // namespace

extern "C" int tfra_multi_sparse_plan_build(tfra_workspace_t* ws, size_t n_plans, const tfra_plan_build_desc* descs,
                                            uint32_t* launches_out, tfra_stream_t stream) {
  if (launches_out) *launches_out = 0;
  if (n_plans == 0) return TFRA_OK;
  if (!ws || !descs) return set_error(TFRA_ERR_INVALID, "multi_sparse_plan_build: null argument");
  hipStream_t s = (hipStream_t)stream;
  const std::string who = "multi_sparse_plan_build: descriptor ";
  // every descriptor is checked before any plan is touched
  std::vector<size_t> act;   // the descriptors with ids, in input order: record k belongs to descs[act[k]]
  for (size_t i = 0; i < n_plans; ++i) {
    const Check c = check_plan_desc(descs[i], ws);
    if (c.code) return report(who + std::to_string(i) + ": ", c);
    if (c.active) act.push_back(i);
  }
  for (size_t i = 0; i < n_plans; ++i)   // a plan object holds ONE build
    for (size_t j = i + 1; j < n_plans; ++j)
      if (descs[i].plan == descs[j].plan)
        return set_error(TFRA_ERR_INVALID, who + std::to_string(i) + " and descriptor " + std::to_string(j) + " name the same plan");
  if (on_device(ws->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "multi_sparse_plan_build: hipSetDevice");
  const size_t n_act = act.size();
  std::vector<PlanLayout> lay(n_act);
  u64 tile_blocks = 0, bucket_blocks = 0;
  for (size_t k = 0; k < n_act; ++k) {
    lay[k] = plan_layout(descs[act[k]].n, descs[act[k]].dim);
    tile_blocks += lay[k].ntiles;
    bucket_blocks += lay[k].P;
  }
  if (tile_blocks >= (1ULL << 31) || bucket_blocks >= (1ULL << 31))
    return set_error(TFRA_ERR_UNSUPPORTED, "multi_sparse_plan_build: too many ids in one call");
  int rc;
  for (size_t k = 0; k < n_act; ++k)
    if ((rc = plan_grow(descs[act[k]].plan, lay[k]))) return rc;
  // the blob: [records | unsigned pool: the tiles' prefix (the tile and the scatter launch), then per cm class its prefix and its
  // record indices]
  Blob blob;
  const size_t rec_off = blob.add<PlanManyRec>(n_act);
  const size_t pool_off = blob.add<unsigned>(ClassPool::words(n_act, 1, false) + ClassPool::words(n_act, 2, true));
  ManyUpload up;
  if (n_act && (rc = many_begin(ws, 0, blob.bytes(), s, &up))) return rc;
  // from here on the call enqueues.  As in the single call, a plan holds no build until its launches are enqueued, and a public
  // build always counts
  for (size_t i = 0; i < n_plans; ++i) { descs[i].plan->skip_counts_once = false; descs[i].plan->n = 0; descs[i].plan->ever_built = true; }
  if (n_act == 0) return TFRA_OK;
  PlanManyRec* recs = section<PlanManyRec>(up.host, rec_off);
  for (size_t k = 0; k < n_act; ++k) {
    const tfra_plan_build_desc& d = descs[act[k]];
    tfra_sparse_plan* pl = d.plan;
    const PlanLayout& L = lay[k];
    if ((rc = plan_lay_out(pl, L, s))) return rc;
    recs[k] = PlanManyRec{L.n, (const i64*)d.ids, L.P, L.cm, (unsigned)L.ntiles, pl->gen, pl->ds, pl->out, plan_err_word(pl, L.P),
                          pl->tile_entries, pl->run_start, pl->tile_len, pl->drec, pl->keymap, pl->dkeys, pl->binmap, pl->cursors,
                          pl->d_counts, pl->host_counts};
  }
  ClassPool pool{section<unsigned>(up.host, pool_off)};
  const ManyClass tile_cls = pool.put(n_act, false, [](size_t) { return true; }, [&](size_t k) { return (unsigned)lay[k].ntiles; });
  ManyClass bucket_cls[2];   // cm 512 | 1024: the bucket kernel's dynamic LDS
  for (int c = 0; c < 2; ++c)
    bucket_cls[c] = pool.put(n_act, true, [&](size_t k) { return lay[k].cm == (c ? 1024u : 512u); }, [&](size_t k) { return lay[k].P; });
  if ((rc = many_send(up, s, "multi_sparse_plan_build: record upload", false))) return rc;
  const PlanManyRec* d_recs = section<const PlanManyRec>(up.dev, rec_off);
  const unsigned* d_pool = section<const unsigned>(up.dev, pool_off);
  uint32_t launches = 0;
  csr_tile_many_kernel<<<tile_cls.grid, NTA, 0, s>>>(d_recs, d_pool + tile_cls.at, (unsigned)n_act);
  ++launches;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(csr_bucket_many_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)plan_smem_bytes(1024));
    attr_set = true;
  }
  for (int c = 0; c < 2; ++c) {
    const ManyClass& k = bucket_cls[c];
    if (!k.n) continue;
    csr_bucket_many_kernel<<<k.grid, NT, plan_smem_bytes(c ? 1024u : 512u), s>>>(d_recs, d_pool + k.at, d_pool + k.at + k.n + 1, k.n);
    ++launches;
  }
  csr_scatter_many_kernel<<<tile_cls.grid, NTA, 0, s>>>(d_recs, d_pool + tile_cls.at, (unsigned)n_act);
  ++launches;
  for (size_t k = 0; k < n_act; ++k) descs[act[k]].plan->armed = true;
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "multi_sparse_plan_build: launch failed");
  for (size_t k = 0; k < n_act; ++k) plan_built(descs[act[k]].plan, lay[k]);
  if (launches_out) *launches_out = launches;
  return TFRA_OK;
}

// the plan's counts as the host knows them: exact when the build has completed and published them
// (step driver), otherwise the worst case (grid-stride kernels read the real counts from device memory)
void tfra::plan_grids(const tfra_sparse_plan* pl, unsigned* key_blocks, unsigned* bin_blocks) {
  size_t keys = pl->n, bins = (size_t)NSH * pl->out.br;
  if (pl->host_counts && (int)(*(volatile unsigned*)(pl->host_counts + HC_GEN) - pl->gen) >= 0) {
    keys = (size_t)pl->host_counts[HC_SHIFT + PC_HOT] + pl->host_counts[HC_SHIFT + PC_COLD];
    bins = pl->host_counts[HC_SHIFT + PC_BINS];
  } else {
    keys = std::min<size_t>(keys, 32768);   // grid-stride beyond 2048 blocks
    bins = std::min<size_t>(bins, 1024);
  }
  *key_blocks = (unsigned)std::max<size_t>(1, (keys * 16 + 255) / 256);
  *bin_blocks = (unsigned)std::max<size_t>(1, bins);
}

// Introspection for tests and tools: the plan's CSR as flat arrays (copies; synchronises the stream).
//   counts[6]; keys[nkeys] (keys with many occurrences first); cnt[nkeys]; positions[n]: key 0's, key 1's, ... each ascending
extern "C" int tfra_sparse_plan_read(const tfra_sparse_plan_t* pl, uint32_t* counts, int64_t* keys, uint32_t* cnt,
                                     uint32_t* positions, size_t cap, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!pl || !counts) return set_error(TFRA_ERR_INVALID, "sparse_plan_read: null argument");
  if (pl->n == 0) { for (int i = 0; i < 6; ++i) counts[i] = 0; return TFRA_OK; }
  if (hipMemcpyAsync(counts, keys_of(pl).d_counts, 6 * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return set_error(TFRA_ERR_HIP, "sparse_plan_read: copy");
  const unsigned nhot = counts[0], ncold = counts[1], nbins = counts[3];
  if (!keys) return TFRA_OK;
  if (pl->kind == 1 && pl->tab_state[pl->set_parity] == TAB_LISTLESS)
    return set_error(TFRA_ERR_UNSUPPORTED, "sparse_plan_read: this plan was built by the overlapped step, without a key list");
  if (pl->kind == 1) {   // SET plan: distinct keys and their occurrence counts; it keeps no positions list
    if (positions) return set_error(TFRA_ERR_UNSUPPORTED, "sparse_plan_read: an assign-only plan keeps the last position of a key, not the list of its positions");
    if ((size_t)ncold > cap) return set_error(TFRA_ERR_INVALID, "sparse_plan_read: buffers too small");
    const SetTab& tb = pl->set_tab[pl->set_parity];
    std::vector<unsigned> sl(ncold);
    std::vector<SetEnt> pc((size_t)pl->set_m2 + 2);
    if ((ncold && hipMemcpyAsync(keys, tb.ukeys, (size_t)ncold * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        (ncold && hipMemcpyAsync(sl.data(), tb.uslot, (size_t)ncold * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipMemcpyAsync(pc.data(), tb.ent, pc.size() * sizeof(SetEnt), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return set_error(TFRA_ERR_HIP, "sparse_plan_read: copy");
    for (unsigned i = 0; i < ncold; ++i) cnt[i] = pc[sl[i]].cnt;
    return TFRA_OK;
  }
  if ((size_t)nhot + ncold > cap) return set_error(TFRA_ERR_INVALID, "sparse_plan_read: buffers too small");
  const CsrOut& o = pl->out;
  const size_t nrec_c = (size_t)NSH * o.cr, nrec_h = (size_t)NSH * o.hr, nbin = (size_t)NSH * o.br;
  std::vector<unsigned> km((size_t)nhot + ncold), bm(nbins), crec(nrec_c * REC_WORDS), hrec(nrec_h * REC_WORDS), hent(nbin * SEG), hout(nbin * 32);
  auto cp = [&](void* d, const void* sdev, size_t b) { return b == 0 || hipMemcpyAsync(d, sdev, b, hipMemcpyDeviceToHost, s) == hipSuccess; };
  bool ok = cp(km.data(), pl->keymap, km.size() * 4) && cp(bm.data(), pl->binmap, bm.size() * 4) && cp(crec.data(), o.crec, crec.size() * 4) &&
            cp(hrec.data(), o.hrec, hrec.size() * 4) && cp(hent.data(), o.hent, hent.size() * 4) && cp(hout.data(), o.hout, hout.size() * 4);
  if (!ok || hipStreamSynchronize(s) != hipSuccess) return set_error(TFRA_ERR_HIP, "sparse_plan_read: copy");
  // partial row -> entry address of the head of its run (only the bins of this build)
  std::vector<std::pair<unsigned, size_t>> heads;
  for (unsigned i = 0; i < nbins; ++i) {
    const size_t bin = bm[i];
    for (unsigned it = 0; it < 32; ++it) {
      const unsigned e = hent[bin * SEG + it * 16];
      if ((e & E_HEAD) && !(e & E_SKIP)) heads.push_back({hout[bin * 32 + it], bin * SEG + it * 16});
    }
  }
  std::sort(heads.begin(), heads.end());
  size_t w = 0;
  for (size_t i = 0; i < km.size(); ++i) {
    const bool many = (km[i] & KM_MANY) != 0;
    const unsigned* rec = (many ? hrec.data() : crec.data()) + (size_t)(km[i] & ~KM_MANY) * REC_WORDS;
    keys[i] = (int64_t)(((uint64_t)rec[1] << 32) | rec[0]);
    cnt[i] = rec[2];
    if (!many) {
      for (unsigned j = 0; j < rec[2]; ++j) { if (w >= pl->n) return set_error(TFRA_ERR_INVALID, "sparse_plan_read: too many entries"); positions[w++] = rec[4 + j]; }
      continue;
    }
    for (unsigned pth = 0; pth < rec[4]; ++pth) {
      auto itp = std::lower_bound(heads.begin(), heads.end(), std::make_pair(rec[3] + pth, (size_t)0));
      if (itp == heads.end() || itp->first != rec[3] + pth) return set_error(TFRA_ERR_INVALID, "sparse_plan_read: a partial has no run");
      size_t a = itp->second;
      bool first = true;
      for (; (a % SEG != 0 || first) && (first || !(hent[a] & E_HEAD)); ++a) {
        first = false;
        if (!(hent[a] & E_SKIP)) { if (w >= pl->n) return set_error(TFRA_ERR_INVALID, "sparse_plan_read: too many entries"); positions[w++] = hent[a] & E_POS; }
      }
    }
  }
  return TFRA_OK;
}

// ---------------------------------------------------------------------------------------------
// One-call forms: the plan is built on the caller's stream into a plan object owned by the table.
int tfra::own_plan(Table* t, tfra_sparse_plan** out) {
  if (!t->own_plan) {
    tfra_sparse_plan* pl = nullptr;
    int rc = tfra_sparse_plan_create(t->device, &pl);
    if (rc) return rc;
    t->own_plan = pl;
  }
  *out = reinterpret_cast<tfra_sparse_plan*>(t->own_plan);
  return TFRA_OK;
}

namespace tfra {
void destroy_own_plan(Table* t) {
  if (t->big_ws) { tfra_workspace_destroy(reinterpret_cast<tfra_workspace_t*>(t->big_ws)); t->big_ws = nullptr; }
  if (t->comb_ws) { tfra_workspace_destroy(reinterpret_cast<tfra_workspace_t*>(t->comb_ws)); t->comb_ws = nullptr; }
  if (t->own_plan) { tfra_sparse_plan_destroy(reinterpret_cast<tfra_sparse_plan*>(t->own_plan)); t->own_plan = nullptr; }
}
}  // namespace tfra

// ---------------------------------------------------------------------------------------------
// Route helpers: the distinct keys of a built plan stand in for tf.unique (PY/shadow_embedding_ops.py:316 does unique,
// then partitions the distinct ids by owner).  tfra_plan_partition = tfra_partition over the plan's keys;
// tfra_plan_positions_to expands its perm to every batch position: dest[p] = j for the positions p of key perm[j].
__global__ __launch_bounds__(256) void plan_dest_keys_kernel(CsrKeys ks, const int* __restrict__ perm, int* __restrict__ dest,
                                                             int* __restrict__ prow_dest) {
  const unsigned total = ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD];
  for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x) {
    const unsigned km = ks.keymap[perm[j]];
    if (km & KM_MANY) {   // its positions sit in the bins: tag the key's partial rows, plan_dest_bins_kernel does the rest
      const unsigned* rec = ks.hrec + (size_t)(km & ~KM_MANY) * REC_WORDS;
      const unsigned first = rec[3], nsrc = rec[4];
      for (unsigned t = 0; t < nsrc; ++t) prow_dest[first + t] = (int)j;
    } else {
      const unsigned* rec = ks.crec + (size_t)km * REC_WORDS;
      const unsigned cnt = rec[2];
      for (unsigned e = 0; e < cnt; ++e) dest[rec[4 + e]] = (int)j;
    }
  }
}

// one block per bin of 512 entries, a 16-lane group per item (the layout hot_sums_kernel reduces)
__global__ __launch_bounds__(NTA) void plan_dest_bins_kernel(const unsigned* __restrict__ hent, const unsigned* __restrict__ hout,
                                                             const unsigned* __restrict__ binmap, const unsigned* __restrict__ d_counts,
                                                             const int* __restrict__ prow_dest, int* __restrict__ dest) {
  constexpr int NG = NTA / 16;
  __shared__ unsigned char s_kind[NG];   // 0 = continues the run of the item before, 1 = first item of a run, 2 = empty item
  __shared__ unsigned s_row[NG];
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, g = threadIdx.x >> 4;
  const unsigned nbins = d_counts[PC_BINS];
  for (unsigned ib = blockIdx.x; ib < nbins; ib += gridDim.x) {
    const unsigned bin = binmap[ib];
    const unsigned e = hent[(size_t)bin * SEG + threadIdx.x];
    const unsigned e0 = (unsigned)__shfl((int)e, gshift);
    const bool empty = (e0 & E_SKIP) != 0, first = (e0 & E_HEAD) != 0;
    if (sub == 0) {
      s_kind[g] = empty ? 2 : (first ? 1 : 0);
      s_row[g] = (first && !empty) ? hout[(size_t)bin * 32 + g] : 0u;
    }
    __syncthreads();
    if (!empty && !(e & E_SKIP)) {
      int g2 = g;
      while (g2 > 0 && s_kind[g2] == 0) --g2;
      dest[e & E_POS] = prow_dest[s_row[g2]];
    }
    __syncthreads();
  }
}

extern "C" int tfra_plan_partition(const tfra_sparse_plan_t* pl, tfra_workspace_t* ws, int num_shards, int mode,
                                   int64_t* keys_out, int32_t* perm_out, int64_t* d_counts, tfra_stream_t stream) {
  if (!pl || pl->n == 0) return set_error(TFRA_ERR_INVALID, "plan_partition: no built plan");
  if (pl->kind == 1) return set_error(TFRA_ERR_UNSUPPORTED, "plan_partition: needs a plan built with the table's dim (an assign-only plan keeps no positions)");
  return tfra_partition(ws, pl->n, reinterpret_cast<const int64_t*>(pl->d_counts + PC_PART_COUNT), (const int64_t*)pl->dkeys, num_shards, mode,
                        keys_out, perm_out, d_counts, stream);
}

extern "C" int tfra_plan_positions_to(const tfra_sparse_plan_t* pl, const int32_t* perm, int32_t* dest_out, tfra_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!pl || pl->n == 0) return set_error(TFRA_ERR_INVALID, "plan_positions_to: no built plan");
  if (pl->kind == 1) return set_error(TFRA_ERR_UNSUPPORTED, "plan_positions_to: needs a plan built with the table's dim (an assign-only plan keeps no positions)");
  if (!perm || !dest_out) return set_error(TFRA_ERR_INVALID, "plan_positions_to: null buffer");
  if (on_device(pl->device) != hipSuccess) return set_error(TFRA_ERR_HIP, "plan_positions_to: hipSetDevice");
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  plan_dest_keys_kernel<<<(unsigned)std::min<size_t>(2048, (pl->n + 255) / 256), 256, 0, s>>>(keys_of(pl), perm, dest_out, pl->prow_dest);
  plan_dest_bins_kernel<<<bin_blocks, NTA, 0, s>>>(pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->prow_dest, dest_out);
  if (hipGetLastError() != hipSuccess) return set_error(TFRA_ERR_HIP, "plan_positions_to: launch failed");
  return TFRA_OK;
}

namespace tfra {
void destroy_workspace_plan(void* plan) { if (plan) tfra_sparse_plan_destroy(reinterpret_cast<tfra_sparse_plan*>(plan)); }
}  // namespace tfra
