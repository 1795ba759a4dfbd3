"""The block-per-row wide pooled lookup and weight gradient (256 < dim <= 1024, wide_rows="block") against the wave-per-row forms
(wide_rows=True), in ONE process, alternating on the same batches (growing table pre-filled with --keys rows, nnz = 131 072
Zipf-1.2 ids per batch, seg = nnz / n_rows entries per row, random weights and grad_out, combiner mean):
  FW the wave forward, de.embedding_lookup_sparse(wide_rows=True) (tfra_table_find_combine_wide: one wave per output row)
  FB the block forward, de.embedding_lookup_sparse(wide_rows="block") (tfra_table_find_combine_wide_long: one block per output row)
  GW the wave gradient, Variable.lookup_combined_weight_grad_wide (tfra_table_find_combine_backprop_weights_wide)
  GB the block gradient, Variable.lookup_combined_weight_grad_wide_long (tfra_table_find_combine_backprop_weights_wide_long)
Shapes: dim 512 float32 and dim 1024 bfloat16, each at 1 / 16 / 64 / 256 / 1024 entries per row.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per shape (median,
min and max of the windows, us per step), written to --out.  A form "wins" only beyond the sum of both spreads (max - min).
   python scripts/mb_wide_long.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--out profiles/wide_long_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

FORMS = (("FW", "FW_find_combine_wide_us"), ("FB", "FB_find_combine_wide_long_us"), ("GW", "GW_weight_grad_wide_us"),
         ("GB", "GB_weight_grad_wide_long_us"))


def beyond_spreads(a, b):
  """a's median below b's by more than the sum of both spreads"""
  return bool(b["median"] - a["median"] > (a["max"] - a["min"]) + (b["max"] - b["min"]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
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
  for dim, vd in ((512, "float32"), (1024, "bfloat16")):
    dt = getattr(torch, vd)
    var = de.Variable(dim=dim, name="mb_wl_%d_%s" % (dim, vd), value_dtype=dt, initializer=0.0, init_size=2 * a.keys)
    gen = torch.Generator(device="cuda").manual_seed(dim)
    for off in range(0, a.keys, 1 << 17):
      k = rkeys[off:off + (1 << 17)]
      var.upsert(k, (torch.randn((k.numel(), dim), generator=gen, device="cuda") * 0.1).to(dt))
    for per_row in (1, 16, 64, 256, 1024):
      n_rows = B // per_row
      seg = (torch.arange(B, device="cuda") // per_row).to(torch.int64)
      G = torch.randn((n_rows, dim), generator=gen, device="cuda")

      def step(f, s):
        ids = batches[s]
        if f == "FW":
          return de.embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", num_rows=n_rows, wide_rows=True)
        if f == "FB":
          return de.embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", num_rows=n_rows, wide_rows="block")
        if f == "GW":
          return var.lookup_combined_weight_grad_wide(ids, seg, w, "mean", G)
        return var.lookup_combined_weight_grad_wide_long(ids, seg, w, "mean", G)

      for s in range(a.warmup):
        r = {f: step(f, s) for f, _ in FORMS}
        assert torch.equal(r["FW"].view(torch.int32), r["FB"].view(torch.int32)), "FW and FB differ"
        assert torch.equal(r["GW"].view(torch.int32), r["GB"].view(torch.int32)), "GW and GB differ"
      torch.cuda.synchronize()
      us = {f: [] for f, _ in FORMS}
      for wi in range(a.windows):
        for f, _ in FORMS:   # alternating: every form sees window wi's batches
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for s in range(a.steps):
            step(f, a.warmup + wi * a.steps + s)
          e1.record()
          e1.synchronize()
          us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
      var._tables[0]._table.check_errors()
      out = {"dim": dim, "dtype": vd, "nnz": B, "n_rows": n_rows, "per_row": per_row, "resident_keys": a.keys, "combiner": "mean",
             "steps_per_window": a.steps}
      for f, label in FORMS:
        out[label] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                      "windows": [round(x, 2) for x in us[f]]}
      for name, (block, wave) in {"forward": ("FB_find_combine_wide_long_us", "FW_find_combine_wide_us"),
                                  "weight_grad": ("GB_weight_grad_wide_long_us", "GW_weight_grad_wide_us")}.items():
        out[name + "_block_wins"] = beyond_spreads(out[block], out[wave])
        out[name + "_block_loses"] = beyond_spreads(out[wave], out[block])
      line = json.dumps(out)
      print(line, flush=True)
      lines.append(line)
    del var
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
