"""The write-back of a many-table model's embedding_lookup_sparse two ways, in ONE process, alternating over the same pre-built
plans and the same grad_out: --tables (26) growing float32 tables, dims cycling 16 / 32 / 64 / 128, each pre-filled with --keys
rows; per table one batch of 8 192 rows x 4 Zipf-1.2 ids, combiner mean, no weights; Adam, then SGD (on the same tables: a table
may carry more slot fields than the rule uses):
  A  the loop of single-table combined write-backs: one _DeviceTable.apply_planned_combined (tfra_table_apply_planned_combined)
     per table — the code of the parent commit
  B  the grouped combined write-back: ONE table_ops.apply_planned_combined_many (tfra_multi_apply_planned_combined)
and the same pair with ONE table in the list (dim 64): what the grouping costs where it cannot help.
A and B write TWIN table sets (same rows, same plans' ids, same gradients); the rows of the batch's ids are compared bit for bit
after every warm-up step.  A plan is applied many times (it is read-only but for its partial sums, rewritten by every use); each
form has its own plan objects.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per point (median, min
and max of the windows, us per step, host calls included; whether the gap between the medians exceeds the spread of A's own
windows), written to --out.
   python scripts/mb_combined_many.py [--tables 26] [--keys 200000] [--steps 20] [--windows 5] [--warmup 5] [--out profiles/combined_many_mb.jsonl]
   --only A|B: that form alone, no comparison (for a kernel trace of one form in a run of its own)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402
from tfra_amd.dynamic_embedding import device_ops, table_ops  # noqa: E402

N_ROWS, PER_ROW = 8192, 4
DIMS = (16, 32, 64, 128)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--tables", type=int, default=26)
  ap.add_argument("--keys", type=int, default=200_000)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--only", choices=["A", "B"], default=None)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_combined_many: no GPU visible; this is a measurement, it has no CPU form")
  forms = a.only or "AB"
  nnz = N_ROWS * PER_ROW
  rng = np.random.default_rng(0)
  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  rkeys = torch.from_numpy(resident).cuda()
  seg = (torch.arange(nnz, device="cuda") // PER_ROW).to(torch.int64)
  adam = de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)
  rules = [("adam", adam), ("sgd", de.optimizers.SGD(0.1))]
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(adam)
  tabs = {f: [] for f in forms}
  plans = {f: [] for f in forms}
  ids, grads = [], []
  for j in range(a.tables):
    dim = DIMS[j % 4]
    ids.append(torch.from_numpy(resident[(rng.zipf(1.2, size=nnz) - 1) % a.keys]).cuda())
    g = torch.Generator(device="cuda").manual_seed(j)
    grads.append(torch.randn((N_ROWS, dim), generator=g, device="cuda") * 0.01)
    for f in forms:
      var = de.Variable(dim=dim, name="mb_cm_%s_%d" % (f, j), initializer=0.0, init_size=2 * a.keys, **kw)
      for off in range(0, a.keys, 1 << 18):
        k = rkeys[off:off + (1 << 18)]
        var.upsert(k, torch.full((k.numel(), dim), 0.01 * (j + 1), device="cuda"))
      tabs[f].append(var)
      plans[f].append(table_ops.SparsePlan(var._primary, dim).build(ids[j]))
  comb = device_ops.COMBINERS["mean"]

  def step(f, idx, p):
    ts = [tabs[f][j]._tables[0] for j in idx]
    if f == "A":
      for j, t in zip(idx, ts):
        t._table.apply_planned_combined(p, plans[f][j], grads[j], seg, None, comb, t._default_value)
      return 0
    return table_ops.apply_planned_combined_many(
        [(t._table, plans[f][j], grads[j], seg, None, comb, t._default_value) for j, t in zip(idx, ts)], p)

  lines = []
  n_step = 0
  for rule, opt in rules:
    for label, idx in (("%d tables" % a.tables, list(range(a.tables))), ("1 table", [2 % a.tables])):
      launches = 0
      for s in range(a.warmup):
        n_step += 1
        p = opt.params(n_step)
        for f in forms:
          launches = step(f, idx, p) or launches
        if len(forms) == 2:
          for j in idx:
            x, y = tabs["A"][j].lookup(ids[j]), tabs["B"][j].lookup(ids[j])
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "A and B differ (table %d)" % j
      torch.cuda.synchronize()
      us = {f: [] for f in forms}
      for wi in range(a.windows):
        for f in forms:   # alternating: both forms run window wi's steps
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for s in range(a.steps):
            step(f, idx, opt.params(n_step + wi * a.steps + s + 1))
          e1.record()
          e1.synchronize()
          us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
      n_step += a.windows * a.steps
      for f in forms:
        for j in idx:
          tabs[f][j]._tables[0]._table.check_errors()
      out = {"point": label, "rule": rule, "tables": len(idx), "dims": [DIMS[j % 4] for j in idx][:4], "dtype": "float32",
             "n_rows": N_ROWS, "per_row": PER_ROW, "nnz_per_table": nnz, "resident_keys_per_table": a.keys,
             "steps_per_window": a.steps, "A_enqueues_per_step": 6 * len(idx), "B_kernel_launches_per_step": launches,
             "B_enqueues_per_step": launches + 2}
      for f, name in (("A", "A_loop_of_apply_planned_combined_us"), ("B", "B_apply_planned_combined_many_us")):
        if f in forms:
          out[name] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                       "windows": [round(x, 2) for x in us[f]]}
      if len(forms) == 2:
        A, B = out["A_loop_of_apply_planned_combined_us"], out["B_apply_planned_combined_many_us"]
        out["A_spread_us"] = round(A["max"] - A["min"], 2)
        out["B_below_A_by_more_than_A_spread"] = bool(A["median"] - B["median"] > A["max"] - A["min"])
        out["B_above_A_by_more_than_A_spread"] = bool(B["median"] - A["median"] > A["max"] - A["min"])
      line = json.dumps(out)
      print(line, flush=True)
      lines.append(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
