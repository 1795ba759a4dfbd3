"""What the gradient of the pooled lookup's weights costs over a tier: tfra_tier_find_combine_backprop_weights against the op chain
that was the only route for a tiered variable before it, against the one-table call on the cache alone, and beside the forward, in
ONE process on one MI355X.

float32 dim 64; an upper LRU table of --slots slots at max_capacity, filled past its capacity; a lower table holding --lower keys
(every key of the upper table among them); batches of nnz = 131 072 Zipf-1.2 ids, 16 per row (8192 rows), combiner mean, random
weights in [0.1, 2), a random float32 grad_out.  Of the entries of a batch 0 %, 10 % or 50 % are drawn from keys the upper table was
never given; the share of ENTRIES that is really only below is taken from tfra_tier_find's `where` and recorded (`below_pct`), not
assumed.  One more shape, `distinct`: 131 072 DISTINCT keys, one entry per row (131 072 rows), half of them cold.  Per mix:
  (a) device_ops.unique (one host read of the count) + tier.find of the unique ids + device_ops.sparse_segment_combine_weight_grad;
  (b) tier.find_combine_weight_grad: tfra_tier_find_combine_backprop_weights, no unique pass, no [U, dim] rows, no host read;
  (c) at the 0 % mix only: find_combine_weight_grad on the upper table alone — the floor: what carrying the second view costs a hit;
  (d) tier.find_combine, the forward over the same batch, for scale.
All forms are reads, so one table pair serves every mix; their windows ALTERNATE: a, b, (c,) d, a, b, ...

HIP events around windows of --steps calls, --windows windows per form (alternating) after --warmup calls; one JSON line per mix:
median, min and max of the windows in us per call, the spreads, (a) - (b) against the sum of both spreads, and (b) - (c).
   python scripts/mb_tier_weight_grad.py [--slots 2097150] [--lower 8388608] [--steps 20] [--windows 5] [--warmup 5]
                                         [--out profiles/tier_weight_grad_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, NNZ, PER_ROW = 64, 131072, 16
MIXES = (0, 10, 50, "distinct")
CHUNK = 1 << 20


def window(f, n):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  for _ in range(n):
    f()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) * 1000.0 / n


def stats(us):
  return {"median": round(float(np.median(us)), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}


def key_of(i):
  return i * 2654435761 + 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--slots", type=int, default=2097150)
  ap.add_argument("--lower", type=int, default=8388608)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tier_weight_grad_mb.jsonl"))
  a = ap.parse_args()
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier

  up = _DeviceTable(torch.int64, torch.float32, torch.zeros(DIM), "mb_twg_up", "cuda:0", dim=DIM, init_capacity=a.slots, max_capacity=a.slots,
                    strategy=0)
  lo = _DeviceTable(torch.int64, torch.float32, torch.zeros(DIM), "mb_twg_lo", "cuda:0", dim=DIM, init_capacity=2 * a.lower)
  n_up = a.slots + a.slots // 4                      # the upper table is given the indices [0, n_up), the highest first:
  for t, n in ((lo, a.lower), (up, n_up)):           # it forgets some of the high ones, the low ones are its newest
    for s in range(0, n, CHUNK):
      i = torch.arange(s, min(s + CHUNK, n), dtype=torch.int64, device="cuda")
      k = key_of(i if t is lo else n_up - 1 - i)
      t.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous(), unique_keys=True)
    t.check_errors()
  tier = _DeviceTier(up, lo, NNZ)
  default_row = torch.zeros(DIM, device="cuda")
  rng = np.random.default_rng(7)
  gen = torch.Generator(device="cuda").manual_seed(7)
  lines = []
  for mix in MIXES:
    if mix == "distinct":                            # distinct keys, one per row, every second one cold
      half = NNZ // 2
      index = np.concatenate([rng.choice(a.slots // 2, half, replace=False), n_up + rng.choice(a.lower - n_up, half, replace=False)])
      rng.shuffle(index)
      per_row = 1
    else:
      rank = rng.zipf(1.2, size=NNZ).astype(np.int64) - 1
      cold = rng.random(NNZ) < mix / 100.0
      index = np.where(cold, n_up + rank % (a.lower - n_up), rank % (a.slots // 2))
      per_row = PER_ROW
    n_rows = NNZ // per_row
    seg = torch.arange(NNZ, dtype=torch.int64, device="cuda") // per_row
    ids = key_of(torch.from_numpy(index).cuda())
    w = torch.rand(NNZ, generator=gen, device="cuda") * 1.9 + 0.1
    G = torch.randn((n_rows, DIM), generator=gen, device="cuda")
    where = tier.find(ids, default_row, return_where=True)[1]
    below_pct = 100.0 * float((where == 2).sum()) / NNZ
    assert int((where == 0).sum()) == 0

    def chain():
      uniq, idx, _ = de.device_ops.unique(ids)
      return de.device_ops.sparse_segment_combine_weight_grad(tier.find(uniq, default_row), idx, G, seg, w, "mean")

    def table_route():
      return tier.find_combine_weight_grad(ids, seg, w, 1, G, default_row)

    def cache_only():
      return up.find_combine_weight_grad(ids, seg, w, 1, G, default_row)

    def forward():
      return tier.find_combine(ids, seg, w, 1, n_rows, default_row)

    run = {"a": chain, "b": table_route}
    if mix == 0:
      run["c"] = cache_only
    run["d"] = forward
    assert torch.equal(chain(), table_route())
    us = {n: [] for n in run}
    for f in run.values():
      for _ in range(a.warmup):
        f()
    for _ in range(a.windows):
      for n, f in run.items():
        us[n].append(window(f, a.steps))
    up.check_errors()
    lo.check_errors()
    out = {"what": "tier_weight_grad", "dim": DIM, "nnz": NNZ, "per_row": per_row, "combiner": "mean", "weights": "random",
           "ids": "distinct" if mix == "distinct" else "zipf 1.2", "cold_pct": 50 if mix == "distinct" else mix,
           "below_pct": round(below_pct, 2), "unique_ids": int(torch.unique(ids).numel()), "upper_slots": a.slots, "lower_keys": a.lower,
           "steps": a.steps, "windows": a.windows, "warmup": a.warmup, "order": "windows alternate " + ", ".join(run)}
    for n in run:
      out[n + "_us"] = stats(us[n])
      out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
    out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
    out["sum_of_spreads_us"] = round(out["a_spread_us"] + out["b_spread_us"], 1)
    out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["sum_of_spreads_us"]
    if "c" in run:
      out["b_minus_c_us"] = round(out["b_us"]["median"] - out["c_us"]["median"], 1)
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
  with open(a.out, "a") as fh:
    fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
