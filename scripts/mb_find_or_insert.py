"""What the admitting lookup costs: tfra_table_find_or_insert against the two calls it replaces, and a training step of a variable
with a callable initializer with and without init_on_lookup, in ONE process on one MI355X.

Table level (float32 dim 64, batches of B = 131 072 unique keys of which 0 %, 10 % or 50 % have never been seen — every step has
never-seen keys of its own, the rest are the head of a hot set that is resident), on
  growing   a growing table of --grow-slots slots holding half as many keys (load 0.5); the keys a window admitted are erased behind
            it, so every window starts from the same table
  bounded   an LRU table of --slots slots at max_capacity, filled past its capacity so that every bucket is full
Per table and mix:
  (a) the parent's route: tfra_table_find with the init rows as full defaults (values = hit ? row : init, found) followed by
      tfra_table_insert_or_assign of ALL keys with those values, TFRA_FLAG_UNIQUE_KEYS, on the route that call chooses by itself
  (b) tfra_table_find_or_insert: one probe, only the never-seen rows written
Algorithmic bytes per call (key 8 B, bucket line 128 B, row 256 B): (a) two probes, B rows read, B rows out, B rows read again, B rows
written; (b) one probe, B rows read (table or init), B rows out, the never-seen rows written.

Training level: one single-shard variable, dim 64, random-normal initializer, Adam, B = 131 072 Zipf-1.2 ids per step of which 10 % of the
positions are never-seen ids; a step is embedding_lookup(return_trainable=True) + apply_gradients.  init_on_lookup=False (reduce_by_key,
a host read of the unique count, apply_optimizer with a second draw) against True (unique, one draw, find_or_insert, gather, the one-call
fused write-back).

HIP events around windows of --steps calls, --windows windows per form (alternating) after --warmup calls; one JSON line per shape:
median, min and max of the windows in us per call for both forms and their spreads.
   python scripts/mb_find_or_insert.py [--slots 8388600] [--grow-slots 16777216] [--steps 20] [--windows 5] [--warmup 5]
                                       [--what table,train] [--lib PATH] [--tag this-tree]
                                       [--out profiles/find_or_insert_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, ROW, LINE, B = 64, 256, 128, 131072
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


def compare(out, us):
  """both forms' statistics, their spreads, b - a and whether b is within the larger spread of a"""
  for n in ("a", "b"):
    out[n + "_us"] = stats(us[n])
    out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
  out["b_minus_a_us"] = round(out["b_us"]["median"] - out["a_us"]["median"], 1)
  out["larger_spread_us"] = max(out["a_spread_us"], out["b_spread_us"])
  out["b_not_slower_than_a_by_more_than_the_spread"] = out["b_minus_a_us"] <= out["larger_spread_us"]
  return out


def fill(tbl, n):
  for lo in range(0, n, CHUNK):
    k = torch.arange(lo, min(lo + CHUNK, n), dtype=torch.int64, device="cuda") * 2654435761 + 1
    tbl.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous(), unique_keys=True)
  tbl.check_errors()


def table_level(a, kind):
  from tfra_amd import _capi
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  if kind == "growing":
    tbl = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(DIM), device="cuda:0", dim=DIM, init_size=8192, name="mb_foi_g")._table
    tbl.reserve(a.grow_slots)
    slots = tbl.capacity() - 2
    fill(tbl, slots // 2 - B)
  else:
    tbl = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(DIM), init_capacity=a.slots, max_capacity=a.slots, device="cuda:0",
                          dim=DIM, evict_strategy=de.HkvEvictStrategy.LRU, name="mb_foi_b")._table
    slots = tbl.capacity() - 2
    fill(tbl, int(slots * 1.3))
  dev = tbl.device
  init = torch.randn(B, DIM, device="cuda")
  rows = torch.empty(B, DIM, device="cuda")
  found = torch.empty(B, dtype=torch.bool, device="cuda")
  hot = torch.arange(B, dtype=torch.int64, device="cuda") * 40503 + (1 << 50)
  serial = [0]

  def batches(pct, steps):
    out, new_keys, n_new = [], [], B * pct // 100
    for _ in range(steps):
      new = (torch.arange(n_new, dtype=torch.int64, device="cuda") + serial[0]) * 6700417 + (1 << 40)
      serial[0] += n_new
      k = torch.cat([new, hot[:B - n_new]])
      out.append(k[torch.randperm(B, device="cuda")].contiguous())
      new_keys.append(new)
    return out, new_keys

  def form_a(k):
    _capi.call("tfra_table_find", tbl._h, B, _ptr(k), _ptr(rows), _ptr(found), _ptr(init), 1, _stream(dev))
    _capi.call("tfra_table_insert_or_assign", tbl._h, B, _ptr(k), _ptr(rows), None, _capi.FLAG_UNIQUE_KEYS, _stream(dev))

  def form_b(k):
    _capi.call("tfra_table_find_or_insert", tbl._h, B, None, _ptr(k), _ptr(init), 1, None, _ptr(rows), _ptr(found), _stream(dev))

  def run(f, pct, steps):
    ks, new = batches(pct, steps)
    us = window(f, ks)
    if kind == "growing" and pct:      # the same table for the next window
      tbl.erase(torch.cat(new))
      tbl.size_host()
    return us

  lines = []
  for pct in MIXES:
    form_b(hot)       # the hot set is resident (and young)
    resident = tbl.size_host()
    for f in (form_a, form_b):
      run(f, pct, a.warmup)
    us = {"a": [], "b": []}
    for _ in range(a.windows):
      for n, f in (("a", form_a), ("b", form_b)):
        us[n].append(run(f, pct, a.steps))
    tbl.check_errors()
    n_new = B * pct // 100
    out = {"level": "table", "table": kind, "never_seen_pct": pct, "slots": slots, "resident": resident, "batch": B, "dim": DIM,
           "steps_per_window": a.steps, "a": "find + insert_or_assign(all keys)", "b": "find_or_insert",
           "a_algorithmic_bytes": 2 * B * (8 + LINE) + 4 * B * ROW, "b_algorithmic_bytes": B * (8 + LINE) + 2 * B * ROW + n_new * ROW}
    line = json.dumps(compare(out, us))
    print(line, flush=True)
    lines.append(line)
  return lines


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
  for n, on in (("a", False), ("b", True)):
    var, deo = make("mb_foi_train_" + n, on)

    def step(ids, var=var, deo=deo):
      _, tw = de.embedding_lookup(var, ids, return_trainable=True)
      deo.apply_gradients([(grads, tw)])

    forms[n] = (step, var)
  for n in ("a", "b"):
    window(forms[n][0], batches(a.warmup))
  us = {"a": [], "b": []}
  for _ in range(a.windows):
    for n in ("a", "b"):
      us[n].append(window(forms[n][0], batches(a.steps)))
  for n in ("a", "b"):
    forms[n][1].tables[0]._table.check_errors()
  out = {"level": "train", "batch": B, "dim": DIM, "optimizer": "Adam", "ids": "Zipf 1.2, 10 % of the positions never seen",
         "steps_per_window": a.steps, "a": "init_on_lookup=False", "b": "init_on_lookup=True"}
  line = json.dumps(compare(out, us))
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
    raise SystemExit("mb_find_or_insert: no GPU visible; this is a measurement, it has no CPU form")
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
