"""The long-row pooled lookup and weight gradient against their twins, in ONE process, alternating on the same batches (growing
table pre-filled with --keys rows, nnz = 131 072 Zipf-1.2 ids per batch, seg = nnz / n_rows entries per row, random weights and
grad_out, combiner mean):
  F  the forward's twin, Variable.lookup_combined (tfra_table_find_combine: one 16-lane group per row)
  FL the long form, Variable.lookup_combined(long_rows=True) (tfra_table_find_combine_long: one 256-thread block per row)
  G  the weight gradient's twin, Variable.lookup_combined_weight_grad (tfra_table_find_combine_backprop_weights)
  GL its long form, Variable.lookup_combined_weight_grad_long (tfra_table_find_combine_backprop_weights_long)
  A  the gradient without either call: Variable.lookup of the entry ids ([nnz, dim] rows), then torch ops
Shapes: dim 64 float32 and dim 128 float16, each at 1 / 16 / 64 / 256 / 1024 entries per row.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per shape (median,
min and max of the windows, us per step), written to --out.  A form "wins" only beyond the sum of both spreads (max - min).
   python scripts/mb_long_rows.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--out profiles/long_rows_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

FORMS = (("F", "F_find_combine_us"), ("FL", "FL_find_combine_long_us"), ("G", "G_weight_grad_us"), ("GL", "GL_weight_grad_long_us"),
         ("A", "A_lookup_then_torch_us"))


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
  for dim, vd in ((64, "float32"), (128, "float16")):
    dt = getattr(torch, vd)
    var = de.Variable(dim=dim, name="mb_lr_%d_%s" % (dim, vd), value_dtype=dt, initializer=0.0, init_size=2 * a.keys)
    gen = torch.Generator(device="cuda").manual_seed(dim)
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, (torch.randn((k.numel(), dim), generator=gen, device="cuda") * 0.1).to(dt))
    for per_row in (1, 16, 64, 256, 1024):
      n_rows = B // per_row
      seg = (torch.arange(B, device="cuda") // per_row).to(torch.int64)
      G = torch.randn((n_rows, dim), generator=gen, device="cuda")

      def step(f, ids):
        if f == "F":
          return var.lookup_combined(ids, seg, w, "mean", n_rows)
        if f == "FL":
          return var.lookup_combined(ids, seg, w, "mean", n_rows, long_rows=True)
        if f == "G":
          return var.lookup_combined_weight_grad(ids, seg, w, "mean", G)
        if f == "GL":
          return var.lookup_combined_weight_grad_long(ids, seg, w, "mean", G)
        x = var.lookup(ids).to(torch.float32)
        d = (x * G[seg]).sum(-1)
        W = torch.zeros(n_rows, device="cuda").index_add_(0, seg, w)
        s = torch.zeros(n_rows, device="cuda").index_add_(0, seg, w * d)
        return (d - (s / W)[seg]) / W[seg]

      for s in range(a.warmup):
        r = {f: step(f, batches[s]) for f, _ in FORMS}
        assert torch.equal(r["F"].view(torch.int32), r["FL"].view(torch.int32)), "F and FL differ"
        assert torch.equal(r["G"].view(torch.int32), r["GL"].view(torch.int32)), "G and GL differ"
        assert torch.allclose(r["A"], r["GL"], rtol=1e-3, atol=1e-4), "A and GL differ"
      torch.cuda.synchronize()
      us = {f: [] for f, _ in FORMS}
      for wi in range(a.windows):
        for f, _ in FORMS:   # alternating: every form sees window wi's batches
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for s in range(a.steps):
            step(f, batches[a.warmup + wi * a.steps + s])
          e1.record()
          e1.synchronize()
          us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
      var._tables[0]._table.check_errors()
      out = {"dim": dim, "dtype": vd, "nnz": B, "n_rows": n_rows, "per_row": per_row, "resident_keys": a.keys, "combiner": "mean",
             "steps_per_window": a.steps}
      for f, label in FORMS:
        out[label] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                      "windows": [round(x, 2) for x in us[f]]}
      pairs = {"forward": ("FL_find_combine_long_us", "F_find_combine_us"), "weight_grad": ("GL_weight_grad_long_us", "G_weight_grad_us"),
               "weight_grad_vs_torch": ("GL_weight_grad_long_us", "A_lookup_then_torch_us")}
      for name, (long, other) in pairs.items():
        out[name + "_long_wins"] = beyond_spreads(out[long], out[other])
        out[name + "_long_loses"] = beyond_spreads(out[other], out[long])
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
