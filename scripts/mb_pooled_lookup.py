"""The forward of embedding_lookup_sparse three ways, in ONE process, alternating on the same batches (growing table pre-filled with
--keys rows, nnz = 131 072 Zipf-1.2 ids per batch, seg = nnz / n_rows entries per row, random weights, combiner mean):
  A  the op chain: device_ops.unique (tfra_unique + its host read of the count) -> Variable.lookup -> sparse_segment_combine
  B  the pooled lookup: Variable.lookup_combined (tfra_table_find_combine)
  C  tfra_table_find alone on the same ids, for scale
Shapes: n_rows 131 072 / 8 192 / 512 (1 / 16 / 256 entries per row) at dim 64 float32, and dim 128 float16 at n_rows 8 192.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per shape (median,
min and max of the windows, us per step; B's algorithmic bytes and their share of the 8 TB/s HBM roofline), appended to --out.
   python scripts/mb_pooled_lookup.py [--keys 2000000] [--steps 20] [--windows 5] [--warmup 5] [--out profiles/pooled_lookup_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  B = 131072
  n_steps = a.warmup + a.steps * a.windows
  rng = np.random.default_rng(0)
  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  batches = [torch.from_numpy(resident[(rng.zipf(1.2, size=B) - 1) % a.keys]).cuda() for _ in range(n_steps)]
  w = torch.from_numpy(rng.uniform(0.1, 2.0, size=B).astype(np.float32)).cuda()
  rkeys = torch.from_numpy(resident).cuda()
  lines = []
  for dim, vd, n_rows in ((64, "float32", 131072), (64, "float32", 8192), (64, "float32", 512), (128, "float16", 8192)):
    dt = getattr(torch, vd)
    var = de.Variable(dim=dim, name="mb_pool_%d_%s_%d" % (dim, vd, n_rows), value_dtype=dt, initializer=0.0, init_size=2 * a.keys)
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
    table = var._tables[0]._table
    seg = (torch.arange(B, device="cuda") // (B // n_rows)).to(torch.int64)

    def step(f, ids):
      if f == "A":
        uniq, idx, _ = de.device_ops.unique(ids)
        return de.device_ops.sparse_segment_combine(var.lookup(uniq), idx, seg, w, "mean", n_rows)
      if f == "B":
        return var.lookup_combined(ids, seg, w, "mean", n_rows)
      return table.find(ids)

    for s in range(a.warmup):
      ra, rb = step("A", batches[s]), step("B", batches[s])
      step("C", batches[s])
      assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), "A and B differ"
    torch.cuda.synchronize()
    us = {f: [] for f in "ABC"}
    for wi in range(a.windows):
      for f in "ABC":   # alternating: every form sees window wi's batches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(a.steps):
          step(f, batches[a.warmup + wi * a.steps + s])
        e1.record()
        e1.synchronize()
        us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
    table.check_errors()
    row_bytes = dim * (4 if vd == "float32" else 2)
    alg = B * (128 + row_bytes) + n_rows * dim * 4 + B * 20   # key line + row per entry, the result, id + seg + weight per entry
    out = {"dim": dim, "dtype": vd, "nnz": B, "n_rows": n_rows, "per_row": B // n_rows, "resident_keys": a.keys,
           "steps_per_window": a.steps, "unique_per_batch": int(torch.unique(batches[a.warmup]).numel()), "B_algorithmic_bytes": alg}
    for f, label in (("A", "A_unique_lookup_combine_us"), ("B", "B_find_combine_us"), ("C", "C_find_only_us")):
      out[label] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                    "windows": [round(x, 2) for x in us[f]]}
    out["B_roofline_fraction_8TBps"] = round(alg / HBM_BYTES_PER_S / (out["B_find_combine_us"]["median"] * 1e-6), 3)
    out["B_below_A_by_more_than_A_spread"] = bool(
        out["A_unique_lookup_combine_us"]["median"] - out["B_find_combine_us"]["median"] >
        out["A_unique_lookup_combine_us"]["max"] - out["A_unique_lookup_combine_us"]["min"])
    line = json.dumps(out)
    print(line, flush=True)
    lines.append(line)
    del var, table
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
