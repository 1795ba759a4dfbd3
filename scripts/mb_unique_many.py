"""The grouped de-duplication against the loop of single calls, in ONE process on one MI355X (the protocol of §4.17:
HIP events around windows of --steps calls after --warmup calls, the forms' windows alternating, the median of --windows windows
and [min - max]):
  unique  lists of 8 192 x 4 Zipf-1.2 ids (32 768 each), 1, 2, 3, 4, 8 and 26 of them, and ONE list of 131 072 ids:
          (a) a loop of device_ops.unique_no_sync — tfra_unique, three launches per list: the parent commit's code, unchanged;
          (b) ONE device_ops.unique_many (tfra_multi_unique, three launches);
          (c) the same with want_idx=False (two launches: what admission asks for).
  step    the whole grouped training lookup (embedding_lookup_sparse_many, return_trainable=True) of --tables
          init_on_lookup="pooled" variables ("pooled") and of as many tiered variables ("tiers"):
          (a) with device_ops.unique_many replaced by the loop of unique_no_sync — before; (b) as it is — after.  Each form on
          variables of its own, filled alike.
One JSON line per point to --out, and the table of DESIGN §4.28 on stdout.
   python scripts/mb_unique_many.py [--tables 26] [--universe 65536] [--steps 20] [--windows 5] [--warmup 5]
                                    [--out profiles/unique_many_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIMS = (16, 32, 64, 128)
LISTS = (1, 2, 3, 4, 8, 26)


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
  ap.add_argument("--tables", type=int, default=26)
  ap.add_argument("--universe", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unique_many_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_unique_many: no GPU visible; this is a measurement, it has no CPU form")
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops

  rng = np.random.default_rng(7)
  grouped_unique = device_ops.unique_many

  def loop_unique(ids_list, want_idx=True, return_launches=False):
    return [device_ops.unique_no_sync(ids) for ids in ids_list]

  def zipf_ids(nnz):
    return key_of(torch.from_numpy((rng.zipf(1.2, size=nnz).astype(np.int64) - 1) % a.universe).cuda())

  table = []
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  fh = open(a.out, "w")

  def report(point, n_lists, us, extra):
    out = {"what": "unique_many", "point": point, "lists": n_lists, "zipf": 1.2, "steps": a.steps, "windows": a.windows,
           "warmup": a.warmup, "order": "the forms' windows alternate"}
    out.update(extra)
    for n in us:
      out[n + "_us"] = stats(us[n])
      out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
    for n in us:
      if n == "a":
        continue
      out["a_minus_%s_us" % n] = round(out["a_us"]["median"] - out[n + "_us"]["median"], 1)
      out["sum_of_spreads_a_%s_us" % n] = round(out["a_spread_us"] + out[n + "_spread_us"], 1)
      out["%s_below_a_by_more_than_both_spreads" % n] = out["a_minus_%s_us" % n] > out["sum_of_spreads_a_%s_us" % n]
    print(json.dumps(out), flush=True)
    fh.write(json.dumps(out) + "\n")
    fh.flush()
    fmt = lambda s: "%.1f [%.1f - %.1f]" % (s["median"], s["min"], s["max"])
    cells = [fmt(out[n + "_us"]) for n in us]
    verdict = ["%.1f / %.1f: %s" % (out["a_minus_%s_us" % n], out["sum_of_spreads_a_%s_us" % n],
                                    "yes" if out["%s_below_a_by_more_than_both_spreads" % n] else "no") for n in us if n != "a"]
    table.append("| %s | %d | %s | %s |" % (point, n_lists, " | ".join(cells + [""] * (3 - len(cells))), " ; ".join(verdict)))

  def measure(run):
    us = {n: [] for n in run}
    for f in run.values():
      for _ in range(a.warmup):
        f()
    for _ in range(a.windows):
      for n, f in run.items():
        us[n].append(window(f, a.steps))
    return us

  # ---- unique: the loop against the grouped call ------------------------------------------------------------------------------------
  n_rows, per_row = 8192, 4
  nnz = n_rows * per_row
  entries = [zipf_ids(nnz) for _ in range(max(LISTS))]
  for n_list in LISTS:
    lists = entries[:n_list]
    us = measure({"a": lambda: loop_unique(lists), "b": lambda: grouped_unique(lists), "c": lambda: grouped_unique(lists, want_idx=False)})
    report("unique", n_list, us, {"ids_per_list": nnz, "a": "loop of unique_no_sync", "b": "unique_many", "c": "unique_many(want_idx=False)"})
  big = [zipf_ids(131072)]
  us = measure({"a": lambda: loop_unique(big), "b": lambda: grouped_unique(big), "c": lambda: grouped_unique(big, want_idx=False)})
  report("unique_131072", 1, us, {"ids_per_list": 131072, "a": "loop of unique_no_sync", "b": "unique_many", "c": "unique_many(want_idx=False)"})

  # ---- step: the whole grouped training lookup, before and after ----------------------------------------------------------------------
  draw = lambda shape: torch.randn(tuple(int(x) for x in shape), device="cuda") * 0.01
  seg = torch.arange(nnz, dtype=torch.int64, device="cuda") // per_row

  def variable(name, dim, tiered):
    creator = None
    if tiered:
      creator = de.TieredHashTableCreator(de.TieredHashTableConfig(
          upper=de.HkvHashTableConfig(init_capacity=2 * a.universe, max_capacity=2 * a.universe, evict_strategy=de.HkvEvictStrategy.LRU),
          max_batch=nnz))
    v = de.Variable(dim=dim, name=name, initializer=draw, init_on_lookup="pooled", init_size=4 * a.universe, devices=["cuda:0"],
                    kv_creator=creator)
    k = key_of(torch.arange(a.universe, dtype=torch.int64, device="cuda"))
    v.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, dim).contiguous())
    return v

  sp = [(seg, e) for e in entries[:a.tables]]
  for point, tiered in (("step_pooled", False), ("step_tiers", True)):
    sets = {f: [variable("mb_um_%s_%s_%d" % (point, f, j), DIMS[j % 4], tiered) for j in range(a.tables)] for f in "ab"}

    def step(vs, unique):
      device_ops.unique_many = unique
      try:
        de.embedding_lookup_sparse_many(vs, sp, None, combiner="sum", return_trainable=True, num_rows=[n_rows] * a.tables)
      finally:
        device_ops.unique_many = grouped_unique

    us = measure({"a": lambda: step(sets["a"], loop_unique), "b": lambda: step(sets["b"], grouped_unique)})
    report(point, a.tables, us, {"dims": list(DIMS), "dtype": "float32", "n_rows": n_rows, "per_row": per_row,
                                 "a": "unique_many = loop of unique_no_sync (before)", "b": "unique_many (after)"})
    del sets
  fh.close()
  print("| point | lists | (a), us | (b), us | (c), us | (a) - form / sum of spreads: beyond it |")
  print("|---|---|---|---|---|---|")
  print("\n".join(table))


if __name__ == "__main__":
  main()
