"""The forward of a many-table model two ways, in ONE process, alternating on the same batches: --tables (26) growing float32
tables, dims cycling 16 / 32 / 64 / 128, each pre-filled with --keys rows; per table a batch of 8 192 rows x 4 Zipf-1.2 ids,
combiner mean, no weights (--batches distinct batches per table, taken in turn):
  A  the loop of single-table pooled lookups: one Variable.lookup_combined (tfra_table_find_combine) per table
  B  the grouped pooled lookup: ONE table_ops.find_combine_many (tfra_multi_find_combine) over the same requests
and the same pair with ONE table in the list (dim 64): what the grouping costs where it cannot help.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per point (median, min
and max of the windows, us per step, host calls included; whether the gap between the medians exceeds the spread of A's own
windows), written to --out.
   python scripts/mb_pooled_many.py [--tables 26] [--keys 200000] [--steps 20] [--windows 5] [--warmup 5] [--out profiles/pooled_many_mb.jsonl]"""
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
  ap.add_argument("--batches", type=int, default=8)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_pooled_many: no GPU visible; this is a measurement, it has no CPU form")
  nnz = N_ROWS * PER_ROW
  rng = np.random.default_rng(0)
  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  rkeys = torch.from_numpy(resident).cuda()
  seg = (torch.arange(nnz, device="cuda") // PER_ROW).to(torch.int64)
  variables, batches = [], []
  for j in range(a.tables):
    dim = DIMS[j % 4]
    var = de.Variable(dim=dim, name="mb_many_%d" % j, initializer=0.0, init_size=2 * a.keys)
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, torch.full((k.numel(), dim), 0.01 * (j + 1), device="cuda"))
    variables.append(var)
    batches.append([torch.from_numpy(resident[(rng.zipf(1.2, size=nnz) - 1) % a.keys]).cuda() for _ in range(a.batches)])

  def requests(vs, idx, s):
    return [(v._tables[0]._table, batches[j][s % a.batches], seg, None, device_ops.COMBINERS["mean"], N_ROWS,
             v._tables[0]._default_value) for v, j in zip(vs, idx)]

  def step(f, vs, idx, s):
    if f == "A":
      return [v.lookup_combined(batches[j][s % a.batches], seg, None, "mean", N_ROWS) for v, j in zip(vs, idx)]
    return table_ops.find_combine_many(requests(vs, idx, s))

  lines = []
  for label, idx in (("%d tables" % a.tables, list(range(a.tables))), ("1 table", [2 % a.tables])):
    vs = [variables[j] for j in idx]
    for s in range(a.warmup):
      for x, y in zip(step("A", vs, idx, s), step("B", vs, idx, s)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "A and B differ"
    _, launches = table_ops.find_combine_many(requests(vs, idx, 0), return_launches=True)
    torch.cuda.synchronize()
    us = {f: [] for f in "AB"}
    for wi in range(a.windows):
      for f in "AB":   # alternating: both forms see window wi's batches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(a.steps):
          step(f, vs, idx, a.warmup + wi * a.steps + s)
        e1.record()
        e1.synchronize()
        us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    for v in vs:
      v._tables[0]._table.check_errors()
    out = {"point": label, "tables": len(idx), "dims": [DIMS[j % 4] for j in idx][:4], "dtype": "float32", "n_rows": N_ROWS,
           "per_row": PER_ROW, "nnz_per_table": nnz, "resident_keys_per_table": a.keys, "steps_per_window": a.steps,
           "A_enqueues_per_step": 3 * len(idx), "B_kernel_launches_per_step": launches, "B_enqueues_per_step": launches + 2}
    for f, name in (("A", "A_loop_of_find_combine_us"), ("B", "B_find_combine_many_us")):
      out[name] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                   "windows": [round(x, 2) for x in us[f]]}
    A, B = out["A_loop_of_find_combine_us"], out["B_find_combine_many_us"]
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
