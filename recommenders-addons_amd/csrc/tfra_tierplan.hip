// The tier's admitting lookup over a write-back plan: tfra_tier_find_or_insert_planned — tfra_tier_find_or_insert
// (tfra_tierstep.hip) over the DISTINCT keys of a built CSR plan, every batch position of a key getting its row and
// its `where` byte, as tfra_table_find_or_insert_planned (tfra_find_insert.hip) relates to tfra_table_find_or_insert.
// The launches: tier_begin_kernel; tier_plan_keys_kernel on the upper table (here: probe, touch, the hits' rows to their
// positions, the misses to the tier's miss list); tier_fetch_kernel on the lower table; the two whole-row upserts of tier_put;
// tier_plan_spread_kernel (here: a missed key's row from L(k) to its other positions); find_plan_bins_kernel (the positions that
// sit in the plan's bins); with TFRA_TIER_VERIFY a count-only find_missed_kernel over the plan's dense keys.
// (GroupRow and find_plan_bins_kernel: tfra_find_insert_device.h.)
#include <hip/hip_runtime.h>

#include "tfra_find_insert_device.h"
#include "tfra_host.h"
#include "tfra_plan.h"
#include "tfra_tier.h"

using namespace tfra;

// A block of the key launch is PLAN_GROUPS 16-lane groups, and a TILE of PLAN_GROUPS * PLAN_ROUNDS plan keys stands behind each of
// its adds on the miss counter: adds to one address serialise (tfra_tier.h: TIER_TILES).
constexpr int PLAN_GROUPS = 64, PLAN_ROUNDS = 2, PLAN_TILE = PLAN_GROUPS * PLAN_ROUNDS;
constexpr unsigned NO_MISS = 0xffffffffu;
static_assert(PLAN_TILE % 64 == 0 && PLAN_TILE <= 16 * PLAN_GROUPS, "the tile's misses are compacted by its first PLAN_TILE threads, whole waves");

// What the key launch and the spread launch read and write beside the upper table and the plan.
struct TierPlanIO {
  unsigned char* rows;   // [n, field_bytes] by batch position; may be null
  uint8_t* where;        // [n] by batch position; may be null
  unsigned n;            // the plan's id count: rows of `rows`, upper bound of its keys
  u64* counter;          // the tier's TC_MISSED
  u64 cap;               // entries of the three lists
  i64* miss_keys;        // the miss list: key,
  int* miss_idx;         // its last batch position L(k),
  int* miss_rec;         // and its index among the plan's keys
};

// Key launch: one 16-lane group per plan key, a tile of PLAN_TILE keys per block and pass (grid-stride over tiles, bounded by the
// count on the device).  The probe is find_wave's (read-only: nothing is claimed here).  A hit is touched as
// find_missed_touch_kernel touches it; its row and where = 1 go to every position of a key with at most DIRECT occurrences, and to
// position L(k) of a key whose positions sit in the bins (find_plan_bins_kernel copies them on from there).  A miss goes to the
// tier's miss list as (key, L(k), index of its record): the tile's misses are compacted in LDS and take their range with ONE add.
// A key in the bins gets prow_dest set whether it hit or missed: after the fetch its row stands at L(k) either way.
template <int G, bool PF1>
__global__ __launch_bounds__(16 * PLAN_GROUPS) void tier_plan_keys_kernel(TableView v, CsrKeys ks, TierPlanIO io, int strategy, u64 epoch,
                                                                         int* __restrict__ prow_dest) {
  constexpr int NW = PLAN_TILE / 64;
  __shared__ i64 s_key[PLAN_TILE];
  __shared__ unsigned s_pos[PLAN_TILE];   // L(k) of a miss, NO_MISS otherwise
  __shared__ unsigned s_cnt[NW];
  __shared__ u64 s_base;
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48, grp = threadIdx.x >> 4, wv = threadIdx.x >> 6;
  const unsigned total = min(ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD], io.n);
  if (blockIdx.x == 0 && threadIdx.x == 0 && ks.d_counts[PC_OVERFLOW]) atomicAdd(v.err_count, ks.d_counts[PC_OVERFLOW]);  // plan overflow
  const unsigned fb = v.field_bytes;
  for (unsigned tile = blockIdx.x * PLAN_TILE; tile < total; tile += gridDim.x * PLAN_TILE) {   // (uniform in the block)
    for (int r = 0; r < PLAN_ROUNDS; ++r) {
      const unsigned t = (unsigned)(r * PLAN_GROUPS + grp), g = tile + t;
      i64 key = 0;
      unsigned misspos = NO_MISS;
      if (g < total) {   // (uniform in the group)
        key = ks.dkeys[g];   // the key itself: the probe starts from it while keymap -> record resolves
        bool many;
        const unsigned w = load_record(ks, g, sub, many);
        u64 h;
        const u64 b0 = bucket0(key, v.nb, h), b1 = bucket1(h, b0, v.nb);
        const i64 k0 = key_line(v, b0)[sub];
        const i64 k1 = PF1 ? key_line(v, b1)[sub] : 0;   // a dense table: both home-bucket lines in flight together
        const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
        unsigned lastp = (unsigned)__shfl((int)w, gshift + (many ? 5 : 3));   // few: the last position itself; many: where it is stored
        if (many) lastp = ks.hent[lastp];
        lastp &= E_POS;
        if (lastp < io.n) {   // (no record of a completed build says otherwise)
          const i64 word = probe_find_word(v, key, b0, b1, k0, sub, gshift, PF1 ? &k1 : nullptr);
          const bool hit = word >= 0;
          GroupRow<G> row{};
          if (hit) {
            update_score(v, (i64)(((u64)word >> 4) * SLOTS + ((u64)word & 15)), false, strategy, 1, epoch, sub);
            if (io.rows) row.load(word_row_ptr(v, (u64)word), fb, sub);
          } else {
            misspos = lastp;
          }
          if (many) {
            if (hit) {
              if (io.rows) row.store(io.rows + (size_t)lastp * fb, fb, sub);
              if (io.where && sub == 0) io.where[lastp] = 1;
            }
            if (prow_dest) {
              const unsigned first = (unsigned)__shfl((int)w, gshift + 3), nsrc = (unsigned)__shfl((int)w, gshift + 4);
              for (unsigned i = sub; i < nsrc; i += 16) prow_dest[first + i] = (int)lastp;
            }
          } else if (hit) {
            for (unsigned e = 0; e < min(cnt, (unsigned)DIRECT); ++e) {
              const unsigned p = (unsigned)__shfl((int)w, gshift + 4 + (int)e);
              if (p >= io.n) continue;
              if (io.rows) row.store(io.rows + (size_t)p * fb, fb, sub);
              if (io.where && sub == 0) io.where[p] = 1;
            }
          }
        }
      }
      if (sub == 0) {
        s_key[t] = key;
        s_pos[t] = misspos;
      }
    }
    __syncthreads();
    // the tile's misses, compacted: thread t < PLAN_TILE stands for key tile + t
    const unsigned pos = threadIdx.x < PLAN_TILE ? s_pos[threadIdx.x] : NO_MISS;
    const u64 m = __ballot(pos != NO_MISS);
    if (wv < NW && lane == 0) s_cnt[wv] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned sum = 0;
#pragma unroll
      for (int i = 0; i < NW; ++i) sum += s_cnt[i];
      s_base = sum ? atomicAdd(io.counter, (u64)sum) : 0;
    }
    __syncthreads();
    if (pos != NO_MISS) {
      unsigned before = 0;
      for (int i = 0; i < wv; ++i) before += s_cnt[i];
      const u64 p = s_base + before + (unsigned)__popcll(m & ((1ULL << lane) - 1ULL));
      if (p < io.cap) {
        io.miss_keys[p] = s_key[threadIdx.x];
        io.miss_idx[p] = (int)pos;
        io.miss_rec[p] = (int)(tile + threadIdx.x);
      }
    }
    __syncthreads();   // (the next tile writes s_key / s_pos / s_cnt again)
  }
}

// Spread launch, behind the promotion: one 16-lane group per entry of the miss list (grid-stride, bounded by the count on the
// device).  The fetch left the key's row and its byte (2 / 0) at L(k); a key with 2 .. DIRECT occurrences gets them copied to its
// other recorded positions.  (A key with more sits in the bins: find_plan_bins_kernel; a key with one is done.)
template <int G>
__global__ __launch_bounds__(256) void tier_plan_spread_kernel(CsrKeys ks, TierPlanIO io, unsigned fb) {
  const int lane = threadIdx.x & 63, sub = lane & 15, gshift = lane & 48;
  const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, ngroups = (gridDim.x * blockDim.x) >> 4;
  const unsigned nkeys = min(ks.d_counts[PC_HOT] + ks.d_counts[PC_COLD], io.n);
  const unsigned total = (unsigned)min(*io.counter, io.cap);
  for (unsigned j = tid >> 4; j < total; j += ngroups) {
    const unsigned g = (unsigned)io.miss_rec[j];
    if (g >= nkeys) continue;   // (no entry of this call's list says so)
    bool many;
    const unsigned w = load_record(ks, g, sub, many);
    const unsigned cnt = (unsigned)__shfl((int)w, gshift + 2);
    if (many || cnt < 2) continue;
    const unsigned lastp = (unsigned)__shfl((int)w, gshift + 3) & E_POS;
    if (lastp >= io.n) continue;
    GroupRow<G> row{};
    if (io.rows) row.load(io.rows + (size_t)lastp * fb, fb, sub);
    const uint8_t f = io.where ? io.where[lastp] : 0;
    for (unsigned e = 0; e < min(cnt, (unsigned)DIRECT); ++e) {
      const unsigned p = (unsigned)__shfl((int)w, gshift + 4 + (int)e);
      if (p >= io.n || p == lastp) continue;
      if (io.rows) row.store(io.rows + (size_t)p * fb, fb, sub);
      if (io.where && sub == 0) io.where[p] = f;
    }
  }
}

extern "C" int tfra_tier_find_or_insert_planned(tfra_tier_t* tier, const tfra_sparse_plan_t* pl, const void* init_values,
                                                int init_is_full, void* rows_out, uint8_t* where, uint32_t flags,
                                                tfra_stream_t stream) {
  const std::string who = "tfra_tier_find_or_insert_planned: ";
  if (!tier) return set_error(TFRA_ERR_INVALID, who + "null tier");
  if (!pl) return set_error(TFRA_ERR_INVALID, who + "null plan");
  if (!init_values) return set_error(TFRA_ERR_INVALID, who + "null buffer");
  if (flags & ~TFRA_TIER_VERIFY) return set_error(TFRA_ERR_INVALID, who + "unknown flag bits");
  if (pl->n == 0) return set_error(TFRA_ERR_INVALID, who + "no built plan");
  if (pl->kind == 1)
    return set_error(TFRA_ERR_UNSUPPORTED, who + "needs a plan built with the table's dim (an assign-only plan keeps no positions)");
  Table* upper = tier->upper;
  {
    const int dt = upper->opts.value_dtype, dim = upper->opts.dim;
    if (pl->dim != dim) return set_error(TFRA_ERR_INVALID, who + "the plan was built for another dim");
    if (upper->opts.device != pl->device && upper->opts.device >= 0)
      return set_error(TFRA_ERR_INVALID, who + "plan and tier live on different devices");
    if (dt != TFRA_F32 && dt != TFRA_F16 && dt != TFRA_BF16)
      return set_error(TFRA_ERR_UNSUPPORTED, who + "value_dtype must be float32, float16 or bfloat16");
    if (dim % 4 != 0 || dim > 256 || (((uintptr_t)init_values | (uintptr_t)rows_out) & 15))
      return set_error(TFRA_ERR_UNSUPPORTED, who + "needs dim % 4 == 0, dim <= 256 and 16-B aligned buffers");
  }
  // (the plan's id count is the host's upper bound of its keys, and the staging holds max_batch)
  if (pl->n > tier->max_batch) return set_error(TFRA_ERR_INVALID, who + "more ids in the plan than the tier's max_batch");
  hipStream_t s = (hipStream_t)stream;
  TierEntry entry;
  if (int rc = tier_enter(tier, s, &entry)) return rc;
  const size_t n = pl->n;
  const unsigned fb = upper->field_bytes;
  const unsigned char* init = (const unsigned char*)init_values;
  const bool hand_back = rows_out || where;
  const int g = granule_of(fb, init_values, rows_out) >= 16 ? 16 : 8;   // (dim % 4 == 0: rows of at least 8 bytes, at most 1024)
  const TierPlanIO io{(unsigned char*)rows_out, where, (unsigned)n, tier->words + TC_MISSED, (u64)tier->max_batch,
                      tier->miss_keys, tier->miss_idx, tier->miss_rec};
  const TableView v = upper->view_of(upper->cur);
  const int strat = upper->opts.strategy;
  const u64 epoch = upper->global_epoch;
  unsigned key_blocks, bin_blocks;
  plan_grids(pl, &key_blocks, &bin_blocks);
  const unsigned tile_blocks = std::max(1u, (unsigned)(((size_t)key_blocks * 16 + PLAN_TILE - 1) / PLAN_TILE));
  const CsrKeys ks = keys_of(pl);
  int* prow_dest = hand_back ? pl->prow_dest : nullptr;
  tier_begin(tier, s);
  // 1. the upper table: rows and `where` of the hits at their positions, their scores touched; the misses to the list
  auto keys_launch = [&](auto G) {
    if (upper->dense) tier_plan_keys_kernel<G, true><<<tile_blocks, 16 * PLAN_GROUPS, 0, s>>>(v, ks, io, strat, epoch, prow_dest);
    else tier_plan_keys_kernel<G, false><<<tile_blocks, 16 * PLAN_GROUPS, 0, s>>>(v, ks, io, strat, epoch, prow_dest);
  };
  if (g == 16) keys_launch(std::integral_constant<int, 16>{});
  else keys_launch(std::integral_constant<int, 8>{});
  // 2. the lower table: the whole row of every listed key, or the row a never-seen key starts with; row and byte to L(k)
  const FetchIO fio{tier->miss_keys, tier->miss_idx, tier->words + TC_MISSED, n, (unsigned char*)rows_out, where,
                    init, init_is_full, tier->up_rows, tier->words + TS_LOWER_HITS};
  launch_fetch(tier->lower, s, n, fio, upper->aux);
  HIP_TRY(hipGetLastError());
  // 3. + 4. up they go; what they displace goes down
  if (int rc = tier_put(tier, s, n, (const long long*)(tier->words + TC_MISSED), tier->miss_keys, tier->up_rows, true)) return rc;
  // 5. + 6. from L(k) to every other position: the missed keys with few occurrences, then the bins (hits and misses; always
  // launched: the host does not know the bin count; without bins it does nothing)
  if (hand_back) {
    const unsigned row_bytes = rows_out ? fb : 0u;
    auto spread_launch = [&](auto G) {
      tier_plan_spread_kernel<G><<<key_blocks, 256, 0, s>>>(ks, io, fb);
      // (rows_out == NULL: rows of 0 bytes — the kernel then moves the bytes of `where` alone)
      find_plan_bins_kernel<G><<<bin_blocks, NTA, 0, s>>>(pl->out.hent, pl->out.hout, pl->binmap, pl->d_counts, pl->prow_dest,
                                                          (unsigned char*)rows_out, where, row_bytes, (unsigned)n);
    };
    if (g == 16) spread_launch(std::integral_constant<int, 16>{});
    else spread_launch(std::integral_constant<int, 8>{});
    HIP_TRY(hipGetLastError());
  }
  // 7. how many distinct keys of the plan are NOT resident now (a batch that saturates its own home buckets)
  if (flags & TFRA_TIER_VERIFY) {
    const MissOut count{tier->words + TS_NOT_RESIDENT, 0, nullptr, nullptr, nullptr};
    launch_find_missed(upper, s, n, (const long long*)(pl->d_counts + PC_PART_COUNT), pl->dkeys, nullptr, nullptr, nullptr, 0, count, false);
    HIP_TRY(hipGetLastError());
  }
  return TFRA_OK;
}
