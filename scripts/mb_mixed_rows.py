"""The mixed-row pooled lookup and weight gradient against both their parents, in ONE process, alternating on the same batches
(growing table pre-filled with --keys rows, nnz = 131 072 Zipf-1.2 ids per batch, random weights and grad_out, combiner mean):
  F  the forward's twin, Variable.lookup_combined (tfra_table_find_combine: one 16-lane group per row)
  FL the long form, Variable.lookup_combined(long_rows=True) (tfra_table_find_combine_long: one 256-thread block per row)
  FM the mixed form at long_from = 32 / 64 / 128 (tfra_table_find_combine_mixed: 16 rows per block, long rows by the block);
     64 is the library's default, what Variable.lookup_combined(mixed_rows=True) runs
  G / GL / GM  the same three for the weight gradient (tfra_table_find_combine_backprop_weights[_long | _mixed])
Shapes: dim 64 float32 and dim 128 float16, each on
  tail  a heavy-tailed batch: row lengths log-uniform on 1 .. 1024 (seed 0), the batch this form exists for
  16 / 1 / 256  entries per row, uniform: what the form costs on either parent's ground.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per shape (median,
min and max of the windows, us per step), written to --out.  A form "wins" only beyond the sum of both spreads (max - min).
   python scripts/mb_mixed_rows.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--out profiles/mixed_rows_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

THRESHOLDS = (32, 64, 128)
FORMS = (["F", "FL"] + ["FM%d" % t for t in THRESHOLDS] + ["G", "GL"] + ["GM%d" % t for t in THRESHOLDS])


def beyond_spreads(a, b):
  """a's median below b's by more than the sum of both spreads"""
  return bool(b["median"] - a["median"] > (a["max"] - a["min"]) + (b["max"] - b["min"]))


def tail_lengths(nnz):
  """row lengths log-uniform on 1 .. 1024 until they cover nnz entries (the last row shortened)"""
  rng = np.random.default_rng(0)
  lens = np.floor(np.exp(rng.uniform(0.0, np.log(1025.0), size=nnz))).astype(np.int64).clip(1, 1024)
  n = int(np.searchsorted(np.cumsum(lens), nnz)) + 1
  lens = lens[:n]
  lens[-1] -= lens.sum() - nnz
  return lens


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
    var = de.Variable(dim=dim, name="mb_mx_%d_%s" % (dim, vd), value_dtype=dt, initializer=0.0, init_size=2 * a.keys)
    gen = torch.Generator(device="cuda").manual_seed(dim)
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, (torch.randn((k.numel(), dim), generator=gen, device="cuda") * 0.1).to(dt))
    shard = var._tables[0]
    tab, default = shard._table, shard._default_value
    for shape in ("tail", 16, 1, 256):
      lens = tail_lengths(B) if shape == "tail" else np.full(B // shape, shape, dtype=np.int64)
      n_rows = int(lens.size)
      seg = torch.from_numpy(np.repeat(np.arange(n_rows, dtype=np.int64), lens)).cuda()
      G = torch.randn((n_rows, dim), generator=gen, device="cuda")

      def step(f, ids):
        if f == "F":
          return var.lookup_combined(ids, seg, w, "mean", n_rows)
        if f == "FL":
          return var.lookup_combined(ids, seg, w, "mean", n_rows, long_rows=True)
        if f.startswith("FM"):
          return tab.find_combine_mixed(ids, seg, w, 1, n_rows, default, long_from=int(f[2:]))
        if f == "G":
          return var.lookup_combined_weight_grad(ids, seg, w, "mean", G)
        if f == "GL":
          return var.lookup_combined_weight_grad_long(ids, seg, w, "mean", G)
        return tab.find_combine_weight_grad_mixed(ids, seg, w, 1, G, default, long_from=int(f[2:]))

      for s in range(a.warmup):
        r = {f: step(f, batches[s]) for f in FORMS}
        for f in FORMS:
          assert torch.equal(r[f].view(torch.int32), r[f[0]].view(torch.int32)), "%s and %s differ" % (f, f[0])
      torch.cuda.synchronize()
      us = {f: [] for f in FORMS}
      for wi in range(a.windows):
        for f in FORMS:   # alternating: every form sees window wi's batches
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for s in range(a.steps):
            step(f, batches[a.warmup + wi * a.steps + s])
          e1.record()
          e1.synchronize()
          us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
      tab.check_errors()
      out = {"dim": dim, "dtype": vd, "nnz": B, "n_rows": n_rows, "shape": shape, "longest_row": int(lens.max()),
             "rows_of_64_or_more": int((lens >= 64).sum()), "resident_keys": a.keys, "combiner": "mean", "steps_per_window": a.steps}
      for f in FORMS:
        out[f + "_us"] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                          "windows": [round(x, 2) for x in us[f]]}
      for kind in "FG":
        for t in THRESHOLDS:
          m = out["%sM%d_us" % (kind, t)]
          for other in (kind, kind + "L"):
            out["%sM%d_vs_%s" % (kind, t, other)] = ("wins" if beyond_spreads(m, out[other + "_us"]) else
                                                     "loses" if beyond_spreads(out[other + "_us"], m) else "within spreads")
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
