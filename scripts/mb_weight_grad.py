"""The gradient of embedding_lookup_sparse's weights four ways, in ONE process, alternating on the same batches (growing table
pre-filled with --keys rows, nnz = 131 072 Zipf-1.2 ids per batch, seg = nnz / n_rows entries per row, random weights and
grad_out, combiner mean):
  A  what a user had to do without the call: Variable.lookup of the entry ids ([nnz, dim] rows), then torch ops
     (gather grad_out by seg, multiply, sum over dim, two index_add per row sum, the mean formula)
  B  the chain twin: Variable.lookup of the entry ids, then device_ops.sparse_segment_combine_weight_grad
  C  the table call: Variable.lookup_combined_weight_grad (tfra_table_find_combine_backprop_weights)
  D  the forward, Variable.lookup_combined (tfra_table_find_combine), for scale
Shapes: n_rows 131 072 / 8 192 / 512 (1 / 16 / 256 entries per row) at dim 64 float32, and dim 128 float16 at n_rows 8 192.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per shape (median,
min and max of the windows, us per step; C's algorithmic bytes and their share of the 8 TB/s HBM roofline), written to --out.
   python scripts/mb_weight_grad.py [--keys 2000000] [--steps 20] [--windows 5] [--warmup 5] [--out profiles/weight_grad_mb.jsonl]"""
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
FORMS = (("A", "A_lookup_then_torch_us"), ("B", "B_lookup_then_chain_twin_us"), ("C", "C_table_call_us"), ("D", "D_forward_find_combine_us"))


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
  arange = torch.arange(B, dtype=torch.int32, device="cuda")
  lines = []
  for dim, vd, n_rows in ((64, "float32", 131072), (64, "float32", 8192), (64, "float32", 512), (128, "float16", 8192)):
    dt = getattr(torch, vd)
    var = de.Variable(dim=dim, name="mb_wg_%d_%s_%d" % (dim, vd, n_rows), value_dtype=dt, initializer=0.0, init_size=2 * a.keys)
    gen = torch.Generator(device="cuda").manual_seed(dim + n_rows)
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, (torch.randn((k.numel(), dim), generator=gen, device="cuda") * 0.1).to(dt))
    table = var._tables[0]._table
    seg = (torch.arange(B, device="cuda") // (B // n_rows)).to(torch.int64)
    G = torch.randn((n_rows, dim), generator=gen, device="cuda")

    def step(f, ids):
      if f == "A":
        x = var.lookup(ids).to(torch.float32)
        d = (x * G[seg]).sum(-1)
        W = torch.zeros(n_rows, device="cuda").index_add_(0, seg, w)
        s = torch.zeros(n_rows, device="cuda").index_add_(0, seg, w * d)
        return (d - (s / W)[seg]) / W[seg]
      if f == "B":
        return de.device_ops.sparse_segment_combine_weight_grad(var.lookup(ids).to(torch.float32), arange, G, seg, w, "mean")
      if f == "C":
        return var.lookup_combined_weight_grad(ids, seg, w, "mean", G)
      return var.lookup_combined(ids, seg, w, "mean", n_rows)

    for s in range(a.warmup):
      ra, rb, rc = step("A", batches[s]), step("B", batches[s]), step("C", batches[s])
      step("D", batches[s])
      assert torch.equal(rb.view(torch.int32), rc.view(torch.int32)), "B and C differ"
      assert torch.allclose(ra, rc, rtol=1e-3, atol=1e-4), "A and C differ"
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
    table.check_errors()
    row_bytes = dim * (4 if vd == "float32" else 2)
    # key line + row per entry, grad_out once per row, id + seg + weight per entry, dw written (and, for mean, read and written again)
    alg = B * (128 + row_bytes) + n_rows * dim * 4 + B * 20 + B * 12
    out = {"dim": dim, "dtype": vd, "nnz": B, "n_rows": n_rows, "per_row": B // n_rows, "resident_keys": a.keys, "combiner": "mean",
           "steps_per_window": a.steps, "C_algorithmic_bytes": alg}
    for f, label in FORMS:
      out[label] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                    "windows": [round(x, 2) for x in us[f]]}
    out["C_roofline_fraction_8TBps"] = round(alg / HBM_BYTES_PER_S / (out["C_table_call_us"]["median"] * 1e-6), 3)
    out["C_over_D"] = round(out["C_table_call_us"]["median"] / out["D_forward_find_combine_us"]["median"], 2)
    out["C_below_A_by_more_than_A_spread"] = bool(
        out["A_lookup_then_torch_us"]["median"] - out["C_table_call_us"]["median"] >
        out["A_lookup_then_torch_us"]["max"] - out["A_lookup_then_torch_us"]["min"])
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
