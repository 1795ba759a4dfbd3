"""What one de-duplication per step would buy a TIERED variable: a training step whose ids are looked up through their write-back
plan (tfra_sparse_plan_build + tfra_tier_find_or_insert_planned) and written back with that same plan (apply_planned) — the step
init_on_lookup="plan" makes on a plain table — against init_on_lookup=True on the same kind of tier in the same run — tfra_unique +
tfra_tier_find_or_insert + tfra_gather_rows, then a write-back that de-duplicates the batch a second time.  True is the yardstick:
it is the route a tiered variable takes for "plan" too.  The variable layer routes tiered shards to the planned call only if this
measurement says so, so the "plan" step is composed here from the layers below it: the variable's one initializer
draw, `TieredHashTable.find_or_insert_planned` and `DynamicEmbeddingOptimizer.apply_sparse(plan=...)`, which is what
`TrainableWrapper._lookup_admitting` and `apply_gradients` do for a plain table.

The table pair of DESIGN 4.20: float32 dim 64 with two slot vectors (Adam), a cache of --slots slots at max_capacity filled past its
capacity, a lower table holding --lower keys.  A step is the lookup and the write-back of B = 131 072 Zipf-1.2 ids of a hot set
that is resident in the cache; of the DISTINCT ids of a batch 0 % or 10 % are replaced by keys that are
only below (a cold range of the lower table that is walked round: a key that comes round again has long been evicted).  One
variable per setting, both alive for the whole run; before every window, outside the timed region, the hot keys are written once
more, so their clocks are the newest at the window's start.

HIP events around windows of --steps steps, --windows windows per setting after --warmup steps, the settings ALTERNATING window by
window; one JSON line per mix: median, min and max of the windows in us per step for both settings, their spreads, the distinct keys
that missed the cache per step, and the decision — "plan" is below True by more than the sum of both spreads, or not.
   python scripts/mb_tier_planned.py [--slots 2097150] [--lower 8388608] [--steps 20] [--windows 5] [--warmup 5] [--mixes 0,10]
                                     [--out profiles/tier_planned_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, B = 64, 131072
MIXES = (0, 10)
CHUNK = 1 << 20
SETTINGS = (("true", True), ("plan", "plan"))


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
  ap.add_argument("--mixes", default=",".join(str(m) for m in MIXES), help="per cent of a batch's distinct ids that are only below")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tier_planned_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_tier_planned: no GPU visible; this is a measurement, it has no CPU form")
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan

  n_cold = a.lower - a.slots - a.slots // 4 - B
  assert n_cold >= 2 * a.slots, "the cold range must be longer than the cache remembers"
  hot = key_of(a.lower - 1 - torch.arange(B, dtype=torch.int64, device="cuda"))
  hot_rows = torch.zeros((B, DIM), device="cuda")
  grads = torch.randn(B, DIM, device="cuda") * 0.01
  rng = np.random.default_rng(7)

  def make(name, on):
    opt = de.optimizers.Adam(0.001)
    cfg = de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=a.slots, max_capacity=a.slots, evict_strategy=de.HkvEvictStrategy.LRU),
                                   max_batch=B)
    var = de.get_variable("mb_tier_planned_" + name, key_dtype=torch.int64, value_dtype=torch.float32, dim=DIM, devices=["cuda:0"],
                          initializer=lambda shape: torch.randn(tuple(shape), device="cuda") * 0.05, init_on_lookup=on,
                          kv_creator=de.TieredHashTableCreator(cfg), init_size=2 * a.lower, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    t = var.tables[0]
    for tbl, n in ((t._lower, a.lower), (t._table, a.slots + a.slots // 4)):     # the cache: the tail of the lower table's keys, past capacity
      for s in range(0, n, CHUNK):
        i = torch.arange(s, min(s + CHUNK, n), dtype=torch.int64, device="cuda")
        k = key_of(i if tbl is t._lower else a.lower - 1 - i)
        tbl.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous() * 0.001, unique_keys=True)
      tbl.check_errors()
    return {"var": var, "deo": de.DynamicEmbeddingOptimizer(opt), "t": t, "cold": 0, "plan": SparsePlan(t._device, DIM) if on == "plan" else None}

  forms = {n: make(n, on) for n, on in SETTINGS}

  def batch(st, pct):
    idx = torch.from_numpy(((rng.zipf(1.2, size=B) - 1) % B).astype(np.int64)).cuda()
    keys = hot.clone()
    if pct:      # pct % of the batch's DISTINCT ids become keys that are only below
      distinct = torch.unique(idx)
      n_cold_ids = distinct.numel() * pct // 100
      pick = distinct[torch.randperm(distinct.numel(), device="cuda")[:n_cold_ids]]
      keys[pick] = key_of((st["cold"] + torch.arange(n_cold_ids, dtype=torch.int64, device="cuda")) % n_cold)
      st["cold"] += n_cold_ids
    return keys[idx].contiguous()

  def step_of(st):
    var, deo, t = st["var"], st["deo"], st["t"]
    if st["plan"] is None:
      def step(ids):
        _, tw = de.embedding_lookup(var, ids, return_trainable=True)
        deo.apply_gradients([(grads, tw)])
    else:
      def step(ids, plan=st["plan"]):
        plan.build(ids)
        t.find_or_insert_planned(plan, dynamic_default_values=var._create_default_values_by_initializer(ids.numel(), t._device))
        deo.apply_sparse(var, ids, grads, plan=plan)
    return step

  lines = []
  for pct in (int(m) for m in a.mixes.split(",")):
    us = {n: [] for n in forms}
    for n, st in forms.items():
      st["t"]._table.upsert(hot, hot_rows, unique_keys=True)          # written last: resident
      window(step_of(st), [batch(st, pct) for _ in range(a.warmup)])
    before = {n: st["t"]._tier.stats() for n, st in forms.items()}
    for _ in range(a.windows):
      for n, st in forms.items():
        st["t"]._table.upsert(hot, hot_rows, unique_keys=True)        # outside the timed region: the hot keys' clocks are the newest
        items = [batch(st, pct) for _ in range(a.steps)]
        us[n].append(window(step_of(st), items))
    out = {"what": "tier_planned", "level": "train", "dim": DIM, "aux_fields": 2, "optimizer": "Adam", "B": B, "ids": "Zipf 1.2 over a resident hot set",
           "distinct_only_below_pct": pct, "upper_slots": a.slots, "lower_keys": a.lower, "steps": a.steps, "windows": a.windows,
           "warmup": a.warmup, "order": "windows alternate true, plan", "true": "init_on_lookup=True: unique + tier find_or_insert + gather_rows, apply_sparse",
           "plan": "sparse_plan_build + tier find_or_insert_planned, apply_planned on that plan"}
    for n, st in forms.items():
      st["t"]._table.check_errors()
      st["t"]._lower.check_errors()
      s = st["t"]._tier.stats()
      calls = max(s["calls"] - before[n]["calls"], 1)
      out[n + "_distinct_missed_per_step"] = round((s["missed"] - before[n]["missed"]) / calls, 1)
      out[n + "_us"] = stats(us[n])
      out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
    out["true_minus_plan_us"] = round(out["true_us"]["median"] - out["plan_us"]["median"], 1)
    out["sum_of_spreads_us"] = round(out["true_spread_us"] + out["plan_spread_us"], 1)
    out["plan_below_true_by_more_than_both_spreads"] = out["true_minus_plan_us"] > out["sum_of_spreads_us"]
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "a") as fh:
    fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
