"""Sparse write-back of a half-precision table, three ways, in ONE process, alternating (dim 128, B = 131 072 Zipf-1.2 ids, about
10 % of every batch never seen before, growing table pre-filled with --keys rows; float16 and bfloat16, Adam and SGD):
  A  tfra_reduce_by_key + tfra_table_apply_optimizer   (the route half tables took before the planned kernels served them)
  B  tfra_table_apply_sparse on the half table         (plan + hot sums + apply_csr_kernel<.., TFRA_F16 / TFRA_BF16>)
  C  tfra_table_apply_sparse on a float32 table of the same dim, for scale
Each form has a table of its own and sees the same batches.  HIP events around windows of --steps steps, --windows windows per
form after --warmup steps; prints one JSON line per (dtype, optimizer): median, min and max of the windows, us per step.
   python scripts/mb_half_apply.py [--keys 2000000] [--steps 20] [--windows 5] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  a = ap.parse_args()
  dim, B = 128, 131072
  n_steps = a.warmup + a.steps * a.windows
  rng = np.random.default_rng(0)
  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  fresh_base = int(resident[-1]) + 1
  batches = []
  for s in range(n_steps):
    ids = resident[(rng.zipf(1.2, size=B) - 1) % a.keys]
    new = rng.random(B) < 0.10
    ids[new] = fresh_base + s * B + np.arange(int(new.sum()), dtype=np.int64)   # never-seen, distinct
    batches.append(torch.from_numpy(ids).cuda())
  g = torch.from_numpy((rng.standard_normal((B, dim)) * 0.01).astype(np.float32)).cuda()
  rkeys = torch.from_numpy(resident).cuda()

  def table(name, opt, dt):
    var = de.Variable(dim=dim, name=name, value_dtype=dt, initializer=0.0, init_size=2 * a.keys + 2 * n_steps * B // 10,
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
    return var

  for vd in ("float16", "bfloat16"):
    for oname, opt in (("adam", de.optimizers.Adam(1e-3)), ("sgd", de.optimizers.SGD(0.01))):
      dt = getattr(torch, vd)
      p = opt.params(1)
      vs = {f: table("mb_half_%s_%s_%s" % (vd, oname, f), opt, torch.float32 if f == "C" else dt) for f in "ABC"}
      ts = {f: v._tables[0] for f, v in vs.items()}
      ds = {f: t._default_value.to(torch.float32) for f, t in ts.items()}

      def step(f, ids):
        t = ts[f]._table
        if f == "A":
          uniq, gsum, cnt = de.device_ops.reduce_by_key(ids, g)
          t.apply_optimizer(p, uniq, gsum, ds[f], n_dev=cnt)
        else:
          t.apply_sparse(p, ids, g, ds[f])

      for f in "ABC":
        for s in range(a.warmup):
          step(f, batches[s])
      torch.cuda.synchronize()
      us = {f: [] for f in "ABC"}
      for w in range(a.windows):
        for f in "ABC":   # alternating: every form sees window w's batches on its own table
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for s in range(a.steps):
            step(f, batches[a.warmup + w * a.steps + s])
          e1.record()
          e1.synchronize()
          us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
      for f in "ABC":
        ts[f]._table.check_errors()
      sizes = {f: int(vs[f].size()) for f in "ABC"}
      assert sizes["A"] == sizes["B"] == sizes["C"], sizes
      out = {"dtype": vd, "opt": oname, "dim": dim, "batch": B, "resident_keys": a.keys, "steps_per_window": a.steps,
             "unique_per_batch": int(torch.unique(batches[a.warmup]).numel()), "table_size_after": sizes["B"]}
      for f, label in (("A", "A_reduce_by_key_plus_apply_optimizer_us"), ("B", "B_apply_sparse_half_us"), ("C", "C_apply_sparse_f32_us")):
        out[label] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                      "windows": [round(x, 2) for x in us[f]]}
      print(json.dumps(out), flush=True)
      del vs, ts


if __name__ == "__main__":
  main()
