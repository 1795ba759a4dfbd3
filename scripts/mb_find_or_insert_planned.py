"""What one de-duplication per step buys: tfra_table_find_or_insert_planned against the unique + find_or_insert + gather it replaces,
and a training step of a variable with a callable initializer under the four lookup settings, in ONE process on one MI355X.

Table level (float32 dim 64, batches of B = 131 072 Zipf-1.2 ids over a resident hot set, of which 0 %, 10 % or 50 % of the POSITIONS
carry ids never seen before — every step has never-seen ids of its own), on
  growing   a growing table of --grow-slots slots holding half as many keys (load 0.5); the keys a window admitted are erased behind
            it, so every window starts from the same table
  bounded   an LRU table of --slots slots at max_capacity, filled past its capacity so that every bucket is full
Per table and mix:
  (a) tfra_unique + tfra_table_find_or_insert (count on the device) + tfra_gather_rows: the init_on_lookup=True lookup
  (b) tfra_sparse_plan_build + tfra_table_find_or_insert_planned: the init_on_lookup="plan" lookup
  (c) tfra_table_find_or_insert_planned alone, over plans built outside the timed window ((b) without the build)

Training level: one single-shard variable per setting, dim 64, random-normal initializer, Adam, B = 131 072 Zipf-1.2 ids per step of
which 10 % of the positions are never-seen ids; a step is embedding_lookup(return_trainable=True) + apply_gradients, with
  init_on_lookup=False | True | True and plan_writeback=True | "plan"
The yardstick of "plan" is True, measured in the same run.

HIP events around windows of --steps calls, --windows windows per form (alternating) after --warmup calls; one JSON line per shape:
median, min and max of the windows in us per call for every form and their spreads.
   python scripts/mb_find_or_insert_planned.py [--slots 8388600] [--grow-slots 16777216] [--steps 20] [--windows 5] [--warmup 5]
                                               [--what table,train] [--lib PATH] [--tag this-tree]
                                               [--out profiles/find_or_insert_planned_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, B = 64, 131072
MIXES = (0, 10, 50)
CHUNK = 1 << 21


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


def summarize(out, us, yardstick, candidate):
  for n in us:
    out[n + "_us"] = stats(us[n])
    out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
  y, c = out[yardstick + "_us"], out[candidate + "_us"]
  out["%s_minus_%s_us" % (candidate, yardstick)] = round(c["median"] - y["median"], 1)
  out["larger_spread_us"] = max(out[yardstick + "_spread_us"], out[candidate + "_spread_us"])
  out["%s_beats_%s_by_more_than_the_spread" % (candidate, yardstick)] = y["median"] - c["median"] > out["larger_spread_us"]
  return out


def fill(tbl, n):
  for lo in range(0, n, CHUNK):
    k = torch.arange(lo, min(lo + CHUNK, n), dtype=torch.int64, device="cuda") * 2654435761 + 1
    tbl.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous(), unique_keys=True)
  tbl.check_errors()


def table_level(a, kind):
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  if kind == "growing":
    tbl = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(DIM), device="cuda:0", dim=DIM, init_size=8192, name="mb_foip_g")._table
    tbl.reserve(a.grow_slots)
    slots = tbl.capacity() - 2
    fill(tbl, slots // 2 - B)
  else:
    tbl = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(DIM), init_capacity=a.slots, max_capacity=a.slots, device="cuda:0",
                          dim=DIM, evict_strategy=de.HkvEvictStrategy.LRU, name="mb_foip_b")._table
    slots = tbl.capacity() - 2
    fill(tbl, int(slots * 1.3))
  dev = tbl.device
  init = torch.randn(B, DIM, device="cuda")
  rows = torch.empty(B, DIM, device="cuda")
  urows = torch.empty(B, DIM, device="cuda")
  hot = torch.arange(B, dtype=torch.int64, device="cuda") * 40503 + (1 << 50)
  rng = np.random.default_rng(5)
  serial = [0]
  plan = SparsePlan(dev, DIM)
  pool = [SparsePlan(dev, DIM) for _ in range(max(a.steps, a.warmup))]

  def batches(pct, steps):
    out, new_keys, n_new = [], [], B * pct // 100
    for _ in range(steps):
      ids = hot[torch.from_numpy(((rng.zipf(1.2, size=B) - 1) % B).astype(np.int64)).cuda()]
      if n_new:
        # the never-seen positions carry Zipf ids of a never-seen universe of their own: they repeat too
        new = (torch.from_numpy(((rng.zipf(1.2, size=n_new) - 1) % n_new).astype(np.int64)).cuda() + serial[0]) * 6700417 + (1 << 40)
        serial[0] += n_new
        ids[torch.from_numpy(rng.choice(B, size=n_new, replace=False)).cuda()] = new
        new_keys.append(new)
      out.append(ids.contiguous())
    return out, new_keys

  def form_a(k):
    uniq, idx, cnt = device_ops.unique_no_sync(k)
    tbl.find_or_insert(uniq, init, count=cnt, out=urows)
    device_ops.gather_rows(urows, idx)

  def form_b(k):
    plan.build(k)
    tbl.find_or_insert_planned(plan, init, out=rows)

  def form_c(item):
    tbl.find_or_insert_planned(item, init, out=rows)

  def run(n, pct, steps):
    ks, new = batches(pct, steps)
    if n == "c":
      us = window(form_c, [pool[i].build(k) for i, k in enumerate(ks)])
    else:
      us = window(form_a if n == "a" else form_b, ks)
    if kind == "growing" and pct:      # the same table for the next window
      tbl.erase(torch.unique(torch.cat(new)))
      tbl.size_host()
    return us

  lines = []
  for pct in MIXES:
    tbl.find_or_insert(hot, init)       # the hot set is resident (and young)
    resident = tbl.size_host()
    for n in "abc":
      run(n, pct, a.warmup)
    us = {"a": [], "b": [], "c": []}
    for _ in range(a.windows):
      for n in "abc":
        us[n].append(run(n, pct, a.steps))
    tbl.check_errors()
    out = {"level": "table", "table": kind, "never_seen_pct": pct, "slots": slots, "resident": resident, "batch": B, "dim": DIM,
           "steps_per_window": a.steps, "a": "unique + find_or_insert(device count) + gather_rows",
           "b": "sparse_plan_build + find_or_insert_planned", "c": "find_or_insert_planned alone (plan built outside the window)"}
    line = json.dumps(summarize(out, us, "a", "b"))
    print(line, flush=True)
    lines.append(line)
  return lines


SETTINGS = (("false", False, False), ("true", True, False), ("true_plan_writeback", True, True), ("plan", "plan", False))


def train_level(a):
  import tfra_amd.dynamic_embedding as de
  universe = 1 << 20
  rng = np.random.default_rng(3)
  n_new = B // 10
  serial = [0]

  def make(name, on):
    opt = de.optimizers.Adam(0.001)
    var = de.get_variable(name, key_dtype=torch.int64, value_dtype=torch.float32, dim=DIM, devices=["cuda:0"],
                          initializer=lambda shape: torch.randn(tuple(shape), device="cuda") * 0.05, init_on_lookup=on,
                          **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    tbl = var.tables[0]._table
    tbl.reserve(1 << 23)
    for lo in range(0, universe, CHUNK):
      k = torch.arange(lo, min(lo + CHUNK, universe), dtype=torch.int64, device="cuda")
      tbl.upsert(k, torch.randn(k.numel(), DIM, device="cuda") * 0.05, unique_keys=True)
    return var, de.DynamicEmbeddingOptimizer(opt)

  def batches(steps):
    out = []
    for _ in range(steps):
      ids = (rng.zipf(1.2, size=B) - 1) % universe
      pos = rng.choice(B, size=n_new, replace=False)
      ids[pos] = universe + serial[0] + np.arange(n_new)
      serial[0] += n_new
      out.append(torch.from_numpy(ids.astype(np.int64)).cuda())
    return out

  grads = torch.randn(B, DIM, device="cuda") * 0.01
  forms = {}
  for n, on, pw in SETTINGS:
    var, deo = make("mb_foip_train_" + n, on)

    def step(ids, var=var, deo=deo, pw=pw):
      _, tw = de.embedding_lookup(var, ids, return_trainable=True, plan_writeback=pw)
      deo.apply_gradients([(grads, tw)])

    forms[n] = (step, var)
  for n in forms:
    window(forms[n][0], batches(a.warmup))
  us = {n: [] for n in forms}
  for _ in range(a.windows):
    for n in forms:
      us[n].append(window(forms[n][0], batches(a.steps)))
  for n in forms:
    forms[n][1].tables[0]._table.check_errors()
  out = {"level": "train", "batch": B, "dim": DIM, "optimizer": "Adam", "ids": "Zipf 1.2, 10 % of the positions never seen",
         "steps_per_window": a.steps, "false": "init_on_lookup=False", "true": "init_on_lookup=True",
         "true_plan_writeback": "init_on_lookup=True, plan_writeback=True", "plan": "init_on_lookup=\"plan\""}
  line = json.dumps(summarize(out, us, "true", "plan"))
  print(line, flush=True)
  return [line]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--slots", type=int, default=8388600)
  ap.add_argument("--grow-slots", type=int, default=1 << 24)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--what", default="table,train")
  ap.add_argument("--lib", default=None)
  ap.add_argument("--tag", default="this tree")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_find_or_insert_planned: no GPU visible; this is a measurement, it has no CPU form")
  if a.lib:   # another build of the library (the parent commit's), as mb_insert_and_evict.py takes one
    from tfra_amd import _capi
    _capi.LIB_PATH = os.path.abspath(a.lib)
  lines = []
  if "table" in a.what:
    for kind in ("growing", "bounded"):
      lines += table_level(a, kind)
      torch.cuda.empty_cache()
  if "train" in a.what:
    lines += train_level(a)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
      f.write("\n".join(json.dumps({"tag": a.tag, **json.loads(l)}) for l in lines) + "\n")


if __name__ == "__main__":
  main()
