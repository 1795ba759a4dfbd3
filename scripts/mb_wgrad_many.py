"""The gradient of sp_weights of a many-table model, two ways, in ONE process on one MI355X:
  (a) the loop of find_combine_weight_grad / find_combine_ragged_weight_grad (tfra_table_find_combine[_ragged]_backprop_weights, or
      tfra_tier_find_combine[_ragged]_backprop_weights over a tier), one call per owner — the route before the grouped call;
  (b) ONE table_ops.find_combine_weight_grad_many / find_combine_ragged_weight_grad_many over the same requests
      (tfra_multi_find_combine[_ragged]_backprop_weights).
--owners (26) float32 owners, dims cycling 16 / 32 / 64 / 128, once as PLAIN tables of --lower keys and once as TIERS: an upper
LRU table of --slots slots at max_capacity, given --slots * 5 / 4 keys (the highest indices first, so it keeps the low ones), over
a lower table of --lower keys that holds every key.  Per owner a batch of 8 192 rows x 4 Zipf-1.2 ids, combiner mean, weights
uniform in [0.1, 2); over tiers 10 % of the entries are drawn from keys the upper table was never given, the others from the low
indices it kept, and the share of ENTRIES that is really only below is taken from tfra_tier_find's `where` and recorded
(`below_pct`), not assumed.  Each form runs on owners of its OWN (two sets, filled alike); the forms' windows ALTERNATE: a, b, a,
b, ...  Points, for each kind of owner:
  tuple     26 owners, the tuple form
  ragged    26 owners, the ragged form
  one       one owner (dim 64) alone in the list: what the grouping costs where it cannot help
HIP events around windows of --steps calls, --windows windows per form after --warmup calls; one JSON line per point (median, min
and max of the windows in us per call, host calls included; (a) - (b) against the sum of both spreads), written to --out, and the
table of DESIGN §4.24 on stdout.
   python scripts/mb_wgrad_many.py [--owners 26] [--kinds plain,tiers] [--slots 65534] [--lower 262144] [--steps 20] [--windows 5]
                                   [--warmup 5] [--out profiles/wgrad_many_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

N_ROWS, PER_ROW = 8192, 4
NNZ = N_ROWS * PER_ROW
DIMS = (16, 32, 64, 128)
COLD_PCT = 10
CHUNK = 1 << 18


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
  ap.add_argument("--owners", type=int, default=26)
  ap.add_argument("--kinds", default="plain,tiers")
  ap.add_argument("--slots", type=int, default=65534)
  ap.add_argument("--lower", type=int, default=262144)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgrad_many_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_wgrad_many: no GPU visible; this is a measurement, it has no CPU form")
  from tfra_amd.dynamic_embedding import table_ops
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier

  n_up = a.slots + a.slots // 4
  seg = torch.arange(NNZ, dtype=torch.int64, device="cuda") // PER_ROW
  splits = torch.arange(0, NNZ + 1, PER_ROW, dtype=torch.int64, device="cuda")
  rng = np.random.default_rng(11)
  one = 2 % a.owners                                  # a dim-64 owner
  lines, table = [], []

  def fill(t, n, reverse):
    for s in range(0, n, CHUNK):
      i = torch.arange(s, min(s + CHUNK, n), dtype=torch.int64, device="cuda")
      k = key_of(n - 1 - i if reverse else i)
      t.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, t._dim).contiguous(), unique_keys=True)
    t.check_errors()

  for kind in a.kinds.split(","):
    tiered = kind == "tiers"
    sets = {}
    for form in "ab":                                 # each form reads owners of its own, filled alike
      owners = []
      for j in range(a.owners):
        dim = DIMS[j % 4]
        lo = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_wgm_%s_%s_lo%d" % (kind, form, j), "cuda:0", dim=dim,
                          init_capacity=2 * a.lower)
        fill(lo, a.lower, False)
        if not tiered:
          owners.append(lo)
          continue
        up = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_wgm_%s_up%d" % (form, j), "cuda:0", dim=dim,
                          init_capacity=a.slots, max_capacity=a.slots, strategy=0)
        fill(up, n_up, True)                          # the upper table forgets some of the high indices, the low ones are its newest
        owners.append(_DeviceTier(up, lo, NNZ))
      sets[form] = owners
    ids, ws, gs, below = [], [], [], []
    for j in range(a.owners):
      dim = DIMS[j % 4]
      rank = rng.zipf(1.2, size=NNZ).astype(np.int64) - 1
      if tiered:
        cold = rng.random(NNZ) < COLD_PCT / 100.0
        # the hot keys: the low indices BOTH sets' upper tables really kept (a full bucket drops a key or two even of its newest)
        low = key_of(torch.arange(a.slots // 2, dtype=torch.int64, device="cuda"))
        kept = torch.nonzero(sets["a"][j]._upper.contains(low) & sets["b"][j]._upper.contains(low)).reshape(-1).cpu().numpy()
        index = np.where(cold, n_up + rank % (a.lower - n_up), kept[rank % kept.size])
      else:
        index = rank % a.lower
      ids.append(key_of(torch.from_numpy(index).cuda()))
      ws.append(torch.from_numpy(rng.uniform(0.1, 2.0, size=NNZ).astype(np.float32)).cuda())
      gs.append(torch.from_numpy(rng.standard_normal((N_ROWS, dim)).astype(np.float32)).cuda())
      if tiered:
        default_row = torch.zeros(dim, device="cuda")
        for form in "ab":
          where = sets[form][j].find(ids[j], default_row, return_where=True)[1]
          assert int((where == 0).sum()) == 0
          below.append(100.0 * float((where == 2).sum()) / NNZ)
    below_pct = [round(min(below), 2), round(float(np.mean(below)), 2), round(max(below), 2)] if tiered else [0.0, 0.0, 0.0]

    def tup(owner, j):
      return (owner, ids[j], seg, ws[j], 1, gs[j])

    def rag(owner, j):
      return (owner, splits, ids[j], ws[j], 1, gs[j])

    A, B = sets["a"], sets["b"]
    every = range(a.owners)
    points = {
        "tuple": (lambda: [A[j].find_combine_weight_grad(ids[j], seg, ws[j], 1, gs[j]) for j in every],
                  lambda: table_ops.find_combine_weight_grad_many([tup(B[j], j) for j in every]), a.owners),
        "ragged": (lambda: [A[j].find_combine_ragged_weight_grad(splits, ids[j], ws[j], 1, gs[j]) for j in every],
                   lambda: table_ops.find_combine_ragged_weight_grad_many([rag(B[j], j) for j in every]), a.owners),
        "one": (lambda: [A[one].find_combine_weight_grad(ids[one], seg, ws[one], 1, gs[one])],
                lambda: table_ops.find_combine_weight_grad_many([tup(B[one], one)]), 1),
    }
    for name, (fa, fb, n_owners) in points.items():
      run = {"a": fa, "b": fb}
      for x, y in zip(fa(), fb()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "(a) and (b) differ at " + name
      us = {n: [] for n in run}
      for f in run.values():
        for _ in range(a.warmup):
          f()
      for _ in range(a.windows):
        for n, f in run.items():
          us[n].append(window(f, a.steps))
      for t in A + B:
        for x in ((t._upper, t._lower) if tiered else (t,)):
          x.check_errors()
      out = {"what": "wgrad_many", "owners_are": kind, "point": name, "owners": n_owners, "dims": list(DIMS), "dtype": "float32",
             "n_rows": N_ROWS, "per_row": PER_ROW, "nnz_per_table": NNZ, "combiner": "mean", "weights": "uniform [0.1, 2)", "zipf": 1.2,
             "cold_pct": COLD_PCT if tiered else 0, "below_pct_min_mean_max": below_pct, "upper_slots": a.slots if tiered else None,
             "upper_given_keys": n_up if tiered else None, "lower_keys": a.lower, "steps": a.steps, "windows": a.windows,
             "warmup": a.warmup, "order": "windows alternate a, b; each form on owners of its own"}
      for n in run:
        out[n + "_us"] = stats(us[n])
        out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
      out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
      out["sum_of_spreads_us"] = round(out["a_spread_us"] + out["b_spread_us"], 1)
      out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["sum_of_spreads_us"]
      print(json.dumps(out), flush=True)
      lines.append(json.dumps(out))
      fmt = lambda s: "%.1f [%.1f - %.1f]" % (s["median"], s["min"], s["max"])
      table.append("| %s | %d %s | %.2f %% | %s | %s | %.1f | %.1f | %s |" % (
          name, n_owners, kind, below_pct[1], fmt(out["a_us"]), fmt(out["b_us"]), out["a_minus_b_us"], out["sum_of_spreads_us"],
          "yes" if out["b_below_a_by_more_than_both_spreads"] else "no"))
    del sets, A, B, points                            # the next kind's owners take the memory
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
  print("| point | owners | entries only below | (a) loop of single calls, us | (b) one grouped call, us | (a) - (b) | sum of spreads | beyond it |")
  print("|---|---|---|---|---|---|---|---|")
  print("\n".join(table))


if __name__ == "__main__":
  main()
