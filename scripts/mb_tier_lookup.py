"""What the tier driver's lookup costs: tfra_tier_find_or_insert against the composed route that existed before it, in ONE
process on one MI355X.

float32 dim 64 with 2 slot vectors; an upper LRU table of --slots slots at max_capacity, filled past its capacity; a lower table
holding --lower keys; batches of B = 131 072 unique keys of which 0 %, 10 % or 50 % miss the upper table (all of them are below).
Per mix:
  (a) the composed route: find_missed(sync=True) on the upper table + find on the lower one + an index copy into the rows +
      upsert_and_evict(sync=True) + upsert of what came back into the lower table.  The EMBEDDING field only; two host reads.
  (b) tfra_tier_find_or_insert: whole rows (three times the bytes per moved key), no host read, no index copy.
Both forms keep a table pair of their own alive for the whole mix (about 15 GB each) and their windows ALTERNATE: a, b, a, b, ...
The missing keys of a call come from a range of the lower table that the upper one does not hold; the range is walked round, and
a key that comes round again has long been evicted.  (b) touches its hits, (a) does not (the composed loop touches them in its
write-back, which neither form runs), so before every window, outside the timed region, BOTH forms write their hot keys once
more: their clocks are the newest at the window's start and the window's promotions displace older keys first.  Each line also
records the share of a batch that really missed the upper table, per form (`a_missed_pct`, `b_missed_pct`).

HIP events around windows of --steps calls, --windows windows per form (alternating) after --warmup calls; one JSON line per mix:
median, min and max of the windows in us per call for both forms, their spreads, and whether (b) is below (a) by more than the sum
of both spreads.
   python scripts/mb_tier_lookup.py [--slots 2097150] [--lower 8388608] [--steps 20] [--windows 5] [--warmup 5]
                                    [--out profiles/tier_lookup_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, AUX, B = 64, 2, 131072
MIXES = (0, 10, 50)
CHUNK = 1 << 20


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
  ap.add_argument("--slots", type=int, default=2097150)
  ap.add_argument("--lower", type=int, default=8388608)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tier_lookup_mb.jsonl"))
  a = ap.parse_args()
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier

  def tables(tag):
    up = _DeviceTable(torch.int64, torch.float32, torch.zeros(DIM), "mb_tier_up_" + tag, "cuda:0", dim=DIM, aux_fields=AUX,
                      init_capacity=a.slots, max_capacity=a.slots, strategy=0)
    lo = _DeviceTable(torch.int64, torch.float32, torch.zeros(DIM), "mb_tier_lo_" + tag, "cuda:0", dim=DIM, aux_fields=AUX,
                      init_capacity=2 * a.lower)
    for t, n in ((lo, a.lower), (up, a.slots + a.slots // 4)):     # the upper table: the tail of the lower table's keys, past capacity
      for s in range(0, n, CHUNK):
        i = torch.arange(s, min(s + CHUNK, n), dtype=torch.int64, device="cuda")
        k = key_of(i if t is lo else a.lower - 1 - i)
        t.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous(), unique_keys=True)
      t.check_errors()
    return up, lo

  lines = []
  init = torch.zeros(DIM, device="cuda")
  hot_rows = torch.zeros((B, DIM), device="cuda")
  for mix in MIXES:
    n_miss = B * mix // 100
    n_cold = a.lower - a.slots - a.slots // 4 - B
    assert n_cold >= 2 * a.slots, "the cold range must be longer than the upper table remembers"
    hot = key_of(a.lower - 1 - torch.arange(B, dtype=torch.int64, device="cuda"))
    forms = {}
    for form in ("a", "b"):     # both table pairs stay alive: the windows alternate
      up, lo = tables("%s%d" % (form, mix))
      forms[form] = {"up": up, "lo": lo, "tier": _DeviceTier(up, lo, B) if form == "b" else None, "cold": 0, "missed": 0, "calls": 0}

    def batch(st):
      k = hot.clone()
      if n_miss:
        k[:n_miss] = key_of((st["cold"] + torch.arange(n_miss, dtype=torch.int64, device="cuda")) % n_cold)
        st["cold"] += n_miss
      return k

    def composed(k, st=forms["a"]):
      up, lo = st["up"], st["lo"]
      rows, mk, mi = up.find_missed(k, init)
      st["missed"] += mk.numel()
      st["calls"] += 1
      if mk.numel():
        fetched = lo.find(mk)
        rows[mi.long()] = fetched
        ek, ev, _ = up.upsert_and_evict(mk, fetched)
        if ek.numel():
          lo.upsert(ek, ev, unique_keys=True)
      return rows

    def driven(k, st=forms["b"]):
      return st["tier"].find_or_insert(k, init)

    run = {"a": composed, "b": driven}
    us = {"a": [], "b": []}
    for form in ("a", "b"):
      forms[form]["up"].upsert(hot, hot_rows, unique_keys=True)     # written last: resident
      for _ in range(a.warmup):
        run[form](batch(forms[form]))
    forms["a"]["missed"] = forms["a"]["calls"] = 0
    b_before = forms["b"]["tier"].stats()
    for _ in range(a.windows):
      for form in ("a", "b"):
        st = forms[form]
        st["up"].upsert(hot, hot_rows, unique_keys=True)            # outside the timed region: the hot keys' clocks are the newest
        items = [batch(st) for _ in range(a.steps)]
        us[form].append(window(run[form], items))
    b_after = forms["b"]["tier"].stats()
    for st in forms.values():
      st["up"].check_errors()
      st["lo"].check_errors()
    a_missed = 100.0 * forms["a"]["missed"] / (max(forms["a"]["calls"], 1) * B)
    b_missed = 100.0 * (b_after["missed"] - b_before["missed"]) / (max(b_after["calls"] - b_before["calls"], 1) * B)
    forms.clear()
    del composed, driven, run
    torch.cuda.empty_cache()
    out = {"what": "tier_lookup", "dim": DIM, "aux_fields": AUX, "B": B, "miss_pct": mix, "upper_slots": a.slots, "lower_keys": a.lower,
           "steps": a.steps, "windows": a.windows, "warmup": a.warmup, "order": "windows alternate a, b",
           "a_missed_pct": round(a_missed, 2), "b_missed_pct": round(b_missed, 2)}
    for n in ("a", "b"):
      out[n + "_us"] = stats(us[n])
      out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
    out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
    out["sum_of_spreads_us"] = round(out["a_spread_us"] + out["b_spread_us"], 1)
    out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["sum_of_spreads_us"]
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
  with open(a.out, "a") as fh:
    fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
