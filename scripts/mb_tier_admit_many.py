"""The admission of a many-table model whose tables are TIERED, two ways, in ONE process on one MI355X:
  (a) the loop of tier.admit (tfra_tier_find_or_insert with no outputs), one chain of 6 launches per tier — what
      variable._admit_entries_many did before the grouped call;
  (b) ONE table_ops.admit_many over the same requests (tfra_multi_tier_find_or_insert): one chain for the whole list.
--tiers (26) float32 tiers with two slot vectors, dims cycling 16 / 32 / 64 / 128: an upper LRU table of --slots slots at
max_capacity, given --slots * 5 / 4 keys (the highest indices first, so it keeps the low ones), over a lower table of --lower keys
that holds every key.  Per tier a batch: the UNIQUE ids of 8 192 x 4 Zipf-1.2 entries over the low indices the upper table kept;
at the 10 % mix the first tenth of them is replaced, call by call, by keys from a range the upper table was never given — the
range is walked round, and a key that comes round again has long been evicted.  The share of a batch that really missed the
upper table is taken from the drivers' statistics and recorded (`missed_pct`), not assumed.  Each form runs on tiers of its OWN
(two sets, filled alike); the forms' windows ALTERNATE: a, b, a, b, ...; before every window, outside the timed region, the form
writes its hot keys once more, so their clocks are the newest and the window's promotions displace older keys first.
Points, each at both mixes:
  admit     --tiers tiers: the loop against the grouped call (the bar of DESIGN §4.25)
  two       two tiers (the variable layer groups from three on: what a list of two would gain)
  one       one tier (dim 64) alone in the list: what the grouping costs where it cannot help
  step      the whole grouped training lookup of --tiers tiers: admission, then ONE find_combine_many over the entries — (a) with
            the loop in front of it (before), (b) with admit_many (after)
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per point and mix
(median, min and max of the windows in us per step, host calls included; (a) - (b) against the sum of both spreads), written to
--out, and the table of DESIGN §4.25 on stdout.
   python scripts/mb_tier_admit_many.py [--tiers 26] [--slots 65534] [--lower 262144] [--steps 20] [--windows 5] [--warmup 5]
                                        [--out profiles/tier_admit_many_mb.jsonl]"""
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
AUX = 2
MIXES = (0, 10)
CHUNK = 1 << 18


def window(f, items):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  for x in items:
    f(x)
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) * 1000.0 / len(items)


def stats(us):
  return {"median": round(float(np.median(us)), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}


def key_of(i):
  return i * 2654435761 + 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--tiers", type=int, default=26)
  ap.add_argument("--slots", type=int, default=65534)
  ap.add_argument("--lower", type=int, default=262144)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tier_admit_many_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_tier_admit_many: no GPU visible; this is a measurement, it has no CPU form")
  from tfra_amd.dynamic_embedding import table_ops
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier

  n_up = a.slots + a.slots // 4
  n_cold = a.lower - n_up
  sets = {}
  for form in "ab":                                   # each form admits into tiers of its own, filled alike
    tiers = []
    for j in range(a.tiers):
      dim = DIMS[j % 4]
      up = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_tam_%s_up%d" % (form, j), "cuda:0", dim=dim, aux_fields=AUX,
                        init_capacity=a.slots, max_capacity=a.slots, strategy=0)
      lo = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_tam_%s_lo%d" % (form, j), "cuda:0", dim=dim, aux_fields=AUX,
                        init_capacity=2 * a.lower)
      for t, n in ((lo, a.lower), (up, n_up)):        # the upper table forgets some of the high indices, the low ones are its newest
        for s in range(0, n, CHUNK):
          i = torch.arange(s, min(s + CHUNK, n), dtype=torch.int64, device="cuda")
          k = key_of(i if t is lo else n_up - 1 - i)
          t.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, dim).contiguous(), unique_keys=True)
        t.check_errors()
      tiers.append(_DeviceTier(up, lo, NNZ))
    sets[form] = tiers
  seg = torch.arange(NNZ, dtype=torch.int64, device="cuda") // PER_ROW
  rng = np.random.default_rng(7)
  one = 2 % a.tiers                                   # a dim-64 tier
  # per tier: the entries of a batch (hot keys, repeating) and their unique ids
  entries, hot, hot_rows = [], [], []
  for j in range(a.tiers):
    rank = rng.zipf(1.2, size=NNZ).astype(np.int64) - 1
    low = key_of(torch.arange(a.slots // 2, dtype=torch.int64, device="cuda"))
    kept = torch.nonzero(sets["a"][j]._upper.contains(low) & sets["b"][j]._upper.contains(low)).reshape(-1).cpu().numpy()
    index = kept[rank % kept.size]
    entries.append(key_of(torch.from_numpy(index).cuda()))
    hot.append(key_of(torch.from_numpy(np.unique(index)).cuda()))
    hot_rows.append(torch.zeros((hot[j].numel(), DIMS[j % 4]), device="cuda"))
  uniq = [int(h.numel()) for h in hot]
  lines, table = [], []
  for mix in MIXES:
    cursor = {(form, j): 0 for form in "ab" for j in range(a.tiers)}   # where each tier's walk of its cold range stands

    def batch(form, members):
      """the members' unique ids of one step: the hot ones, the first mix % of them replaced by keys that are only below"""
      out = []
      for j in members:
        k = hot[j].clone()
        n_miss = uniq[j] * mix // 100
        if n_miss:
          k[:n_miss] = key_of(n_up + (cursor[form, j] + torch.arange(n_miss, dtype=torch.int64, device="cuda")) % n_cold)
          cursor[form, j] += n_miss
        out.append(k)
      return out

    A, B = sets["a"], sets["b"]
    everyone = list(range(a.tiers))

    def loop(tiers, members):
      def f(keys):
        for j, k in zip(members, keys):
          tiers[j].admit(k)
      return f

    def grouped(tiers, members):
      def f(keys):
        table_ops.admit_many([(tiers[j], k) for j, k in zip(members, keys)])
      return f

    def read(tiers):
      return table_ops.find_combine_many([(tiers[j], entries[j], seg, None, 1, N_ROWS) for j in everyone])

    def step(admit, tiers):
      def f(keys):
        admit(keys)
        read(tiers)
      return f

    points = {
        "admit": (everyone, loop(A, everyone), grouped(B, everyone)),
        "two": (everyone[:2], loop(A, everyone[:2]), grouped(B, everyone[:2])),
        "one": ([one], loop(A, [one]), grouped(B, [one])),
        "step": (everyone, step(loop(A, everyone), A), step(grouped(B, everyone), B)),
    }
    for name, (members, fa, fb) in points.items():
      run = {"a": fa, "b": fb}
      own = {"a": A, "b": B}
      us = {n: [] for n in run}
      for n, f in run.items():
        for _ in range(a.warmup):
          f(batch(n, members))
      before = {n: [own[n][j].stats() for j in members] for n in run}
      for _ in range(a.windows):
        for n, f in run.items():
          for j in members:      # outside the timed region: the hot keys' clocks are the newest
            own[n][j]._upper.upsert(hot[j], hot_rows[j], unique_keys=True)
          items = [batch(n, members) for _ in range(a.steps)]
          us[n].append(window(f, items))
      missed = {}
      for n in run:
        after = [own[n][j].stats() for j in members]
        calls = sum(y["calls"] - x["calls"] for x, y in zip(before[n], after))
        assert calls == a.windows * a.steps * len(members), (name, n, calls)
        assert all(y["not_resident"] == 0 for y in after)
        missed[n] = 100.0 * sum(y["missed"] - x["missed"] for x, y in zip(before[n], after)) / (a.windows * a.steps * sum(uniq[j] for j in members))
      for t in A + B:
        t._upper.check_errors()
        t._lower.check_errors()
      out = {"what": "tier_admit_many", "point": name, "tiers": len(members), "dims": list(DIMS), "dtype": "float32", "aux_fields": AUX,
             "n_rows": N_ROWS, "per_row": PER_ROW, "unique_ids_per_tier_min_mean_max": [min(uniq), round(float(np.mean(uniq)), 1), max(uniq)],
             "zipf": 1.2, "cold_pct": mix, "a_missed_pct": round(missed["a"], 2), "b_missed_pct": round(missed["b"], 2),
             "upper_slots": a.slots, "upper_given_keys": n_up, "lower_keys": a.lower, "steps": a.steps, "windows": a.windows,
             "warmup": a.warmup, "order": "windows alternate a, b; each form on tiers of its own; hot keys re-touched before every window"}
      for n in run:
        out[n + "_us"] = stats(us[n])
        out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
      out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
      out["sum_of_spreads_us"] = round(out["a_spread_us"] + out["b_spread_us"], 1)
      out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["sum_of_spreads_us"]
      print(json.dumps(out), flush=True)
      lines.append(json.dumps(out))
      fmt = lambda s: "%.1f [%.1f - %.1f]" % (s["median"], s["min"], s["max"])
      table.append("| %s | %d | %d %% (%.1f %% / %.1f %%) | %s | %s | %.1f | %.1f | %s |" % (
          name, len(members), mix, missed["a"], missed["b"], fmt(out["a_us"]), fmt(out["b_us"]), out["a_minus_b_us"],
          out["sum_of_spreads_us"], "yes" if out["b_below_a_by_more_than_both_spreads"] else "no"))
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
  print("| point | tiers | cold (missed, a / b) | (a) loop, us | (b) grouped, us | (a) - (b) | sum of spreads | beyond it |")
  print("|---|---|---|---|---|---|---|---|")
  print("\n".join(table))


if __name__ == "__main__":
  main()
