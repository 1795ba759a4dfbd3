"""The training lookup of variables with a RANDOM initializer, the chain against the pooled route, in ONE process on one MI355X
(the protocol of §4.17: HIP events around windows of --steps calls after --warmup calls, the forms' windows
alternating a, b, a, b, ..., the median of --windows windows and [min - max], each form on tables of its own, filled alike):
  one     one variable, dim 64 float32, 8 192 rows x 16 Zipf-1.2 entries (nnz 131 072):
          (a) embedding_lookup_sparse(..., return_trainable=True) under init_on_lookup=True — the chain: unique with a host read of
              the count, one draw of [U, dim], find_or_insert returning [U, dim], sparse_segment_combine;
          (b) the same call under init_on_lookup="pooled": unique with the count left on the device, one draw of
              [n_entry_ids, dim] (131 072 rows where the chain draws U: part of what is measured), admit, ONE pooled read.
  admit   26 float32 tables (dims 16 / 32 / 64 / 128) x the unique ids of 8 192 x 4 Zipf-1.2 entries, lists of 1, 2, 3, 4, 5, 6, 8 and 26:
          (a) a loop of _DeviceTable.admit, (b) ONE table_ops.table_admit_many (tfra_multi_find_or_insert).  The init rows are
          buffers made beforehand: no draw is in this point.  ADMIT_MANY_MIN_TABLES is the shortest list where (b) is below (a) by
          more than the sum of both spreads.
  step    the whole grouped training lookup of the 26 variables (embedding_lookup_sparse_many, return_trainable=True):
          (a) init_on_lookup=True — 26 chains; (b) "pooled" — 26 uniques and draws, ONE grouped admission, ONE grouped read.
Every point at 0 % and 10 % never-seen ids: at 10 % the first tenth of a batch's positions (one / step) or unique ids (admit) is
replaced, call by call, by ids no table has seen; the tables grow under them (a growth that falls into a window is in its time, for both forms alike).
One JSON line per point and mix to --out, and the table of DESIGN §4.27 on stdout.
   python scripts/mb_admit_pooled.py [--tables 26] [--universe 65536] [--steps 20] [--windows 5] [--warmup 5]
                                     [--out profiles/admit_pooled_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIMS = (16, 32, 64, 128)
MIXES = (0, 10)
LISTS = (1, 2, 3, 4, 5, 6, 8, 26)


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
  ap.add_argument("--tables", type=int, default=26)
  ap.add_argument("--universe", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit_pooled_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_admit_pooled: no GPU visible; this is a measurement, it has no CPU form")
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops

  rng = np.random.default_rng(7)
  draw = lambda shape: torch.randn(tuple(int(x) for x in shape), device="cuda") * 0.01
  fresh = [a.universe]                                  # the next index no table has seen

  def never_seen(n):
    k = key_of(torch.arange(fresh[0], fresh[0] + n, dtype=torch.int64, device="cuda"))
    fresh[0] += n
    return k

  def variable(name, dim, mode):
    v = de.Variable(dim=dim, name=name, initializer=draw, init_on_lookup=mode, init_size=4 * a.universe, devices=["cuda:0"])
    k = key_of(torch.arange(a.universe, dtype=torch.int64, device="cuda"))
    v.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, dim).contiguous())
    return v

  def zipf_ids(nnz):
    return key_of(torch.from_numpy((rng.zipf(1.2, size=nnz).astype(np.int64) - 1) % a.universe).cuda())

  lines, table = [], []

  def report(point, n_tables, mix, us, extra):
    out = {"what": "admit_pooled", "point": point, "tables": n_tables, "never_seen_pct": mix, "zipf": 1.2, "steps": a.steps,
           "windows": a.windows, "warmup": a.warmup, "order": "windows alternate a, b; each form on tables of its own"}
    out.update(extra)
    for n in "ab":
      out[n + "_us"] = stats(us[n])
      out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
    out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
    out["sum_of_spreads_us"] = round(out["a_spread_us"] + out["b_spread_us"], 1)
    out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["sum_of_spreads_us"]
    print(json.dumps(out), flush=True)
    lines.append(json.dumps(out))
    fmt = lambda s: "%.1f [%.1f - %.1f]" % (s["median"], s["min"], s["max"])
    table.append("| %s | %d | %d %% | %s | %s | %.1f | %.1f | %s |" % (
        point, n_tables, mix, fmt(out["a_us"]), fmt(out["b_us"]), out["a_minus_b_us"], out["sum_of_spreads_us"],
        "yes" if out["b_below_a_by_more_than_both_spreads"] else "no"))

  def measure(run, make_item):
    us = {n: [] for n in run}
    for n, f in run.items():
      for _ in range(a.warmup):
        f(make_item())
    for _ in range(a.windows):
      for n, f in run.items():
        items = [make_item() for _ in range(a.steps)]
        us[n].append(window(f, items))
    return us

  # ---- one: one variable, the chain against the pooled route ---------------------------------------------------------------------
  n_rows, per_row = 8192, 16
  nnz = n_rows * per_row
  seg = torch.arange(nnz, dtype=torch.int64, device="cuda") // per_row
  ids0 = zipf_ids(nnz)
  vs = {"a": variable("mb_ap_one_true", 64, True), "b": variable("mb_ap_one_pooled", 64, "pooled")}
  for mix in MIXES:
    def item():
      ids = ids0.clone()
      if mix:
        ids[:nnz * mix // 100] = never_seen(nnz * mix // 100)
      return ids
    run = {n: (lambda ids, v=v: de.embedding_lookup_sparse(v, (seg, ids), None, combiner="sum", return_trainable=True, num_rows=n_rows))
           for n, v in vs.items()}
    us = measure(run, item)
    report("one", 1, mix, us, {"dim": 64, "dtype": "float32", "nnz": nnz, "per_row": per_row,
                               "unique_ids": int(torch.unique(ids0).numel()), "a": "init_on_lookup=True (chain)", "b": "init_on_lookup=\"pooled\""})
  for v in vs.values():
    v._tables[0]._table.check_errors()
  del vs

  # ---- admit: the loop of admit against table_admit_many ---------------------------------------------------------------------------
  n_rows, per_row = 8192, 4
  nnz = n_rows * per_row
  seg = torch.arange(nnz, dtype=torch.int64, device="cuda") // per_row
  entries = [zipf_ids(nnz) for _ in range(a.tables)]
  hot = [torch.unique(e) for e in entries]
  uniq = [int(h.numel()) for h in hot]
  sets = {}
  for form, mode in (("a", True), ("b", "pooled")):
    sets[form] = [variable("mb_ap_%s_%d" % (form, j), DIMS[j % 4], mode) for j in range(a.tables)]
  init = [draw((uniq[j], DIMS[j % 4])) for j in range(a.tables)]
  for mix in MIXES:
    def keys_of(members):
      out = []
      for j in members:
        k = hot[j].clone()
        if mix:
          k[:uniq[j] * mix // 100] = never_seen(uniq[j] * mix // 100)
        out.append(k)
      return out
    for n_list in LISTS:
      if n_list > a.tables:
        continue
      members = list(range(n_list)) if n_list > 1 else [2 % a.tables]      # (alone: a dim-64 table)
      tabs = {form: [v._tables[0]._table for v in sets[form]] for form in "ab"}

      def loop(keys, t=tabs["a"]):
        for j, k in zip(members, keys):
          t[j].admit(k, init[j])

      def grouped(keys, t=tabs["b"]):
        table_ops.table_admit_many([(t[j], k, init[j]) for j, k in zip(members, keys)])

      us = measure({"a": loop, "b": grouped}, lambda: keys_of(members))
      report("admit", n_list, mix, us, {"dims": [DIMS[j % 4] for j in members], "dtype": "float32", "n_rows": n_rows, "per_row": per_row,
                                        "unique_ids_min_mean_max": [min(uniq), round(float(np.mean(uniq)), 1), max(uniq)],
                                        "a": "loop of _DeviceTable.admit", "b": "table_admit_many"})
    # ---- step: the whole grouped training lookup ----------------------------------------------------------------------------------
    def items():
      out = []
      for j in range(a.tables):
        ids = entries[j].clone()
        if mix:
          ids[:nnz * mix // 100] = never_seen(nnz * mix // 100)
        out.append((seg, ids))
      return out
    run = {n: (lambda sp, vs=sets[n]: de.embedding_lookup_sparse_many(vs, sp, None, combiner="sum", return_trainable=True,
                                                                       num_rows=[n_rows] * a.tables)) for n in "ab"}
    us = measure(run, items)
    report("step", a.tables, mix, us, {"dims": list(DIMS), "dtype": "float32", "n_rows": n_rows, "per_row": per_row,
                                       "a": "init_on_lookup=True (26 chains)", "b": "init_on_lookup=\"pooled\""})
  for form in "ab":
    for v in sets[form]:
      v._tables[0]._table.check_errors()
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
  print("| point | tables | never seen | (a), us | (b), us | (a) - (b) | sum of spreads | beyond it |")
  print("|---|---|---|---|---|---|---|---|")
  print("\n".join(table))


if __name__ == "__main__":
  main()
