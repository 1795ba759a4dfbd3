"""Write-back of an embedding_lookup_sparse gradient, three ways, on one shard (growing table sized for 10^8 keys, dim 64
fp32), 16 384 rows x 8 entries (nnz 131 072) of Zipf-1.2 ids, weighted mean; SGD and Adam:
  (a) tfra_sparse_segment_combine_backprop + tfra_table_apply_sparse    (the [nnz, dim] gradient written and read back)
  (b) tfra_table_apply_planned_combined, plan built beforehand (as at lookup time)
  (c) for reference, tfra_table_apply_planned on a pre-expanded [nnz, dim] gradient, same plan
Prints one JSON line per optimizer (us per call, HIP events around `--iters` calls, median of `--reps`).
   python scripts/mb_sparse_combined.py [--keys 100000000] [--iters 50] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402


def timed(fn, iters, reps):
  fn()
  torch.cuda.synchronize()
  out = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
      fn()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b) * 1000.0 / iters)
  return float(np.median(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=10**8)
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--reps", type=int, default=5)
  a = ap.parse_args()
  dim, n_rows, per = 64, 16384, 8
  rng = np.random.default_rng(0)
  ids = (rng.zipf(1.2, size=n_rows * per) % a.keys).astype(np.int64)
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), per)
  w = rng.uniform(0.1, 2.0, size=ids.size).astype(np.float32)
  it, st, wt = (torch.from_numpy(x).cuda() for x in (ids, seg, w))
  G = torch.from_numpy((rng.standard_normal((n_rows, dim)) * 0.01).astype(np.float32)).cuda()
  for name, opt in (("sgd", de.optimizers.SGD(0.01)), ("adam", de.optimizers.Adam(1e-3))):
    var = de.Variable(dim=dim, name="mb_sc_" + name, initializer=0.0, init_size=a.keys,
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    deo = de.DynamicEmbeddingOptimizer(opt)
    t = var._tables[0]
    d = t._default_value.to(torch.float32)
    p = deo.begin_step()
    plan = de.SparsePlan(var._primary, dim).build(it)
    eg = de.device_ops.sparse_segment_combine_backprop(G, st, wt, "mean")
    ua = timed(lambda: t._table.apply_sparse(p, it, de.device_ops.sparse_segment_combine_backprop(G, st, wt, "mean"), d),
               a.iters, a.reps)
    ub = timed(lambda: t._table.apply_planned_combined(p, plan, G, st, wt, 1, d), a.iters, a.reps)
    uc = timed(lambda: t._table.apply_planned(p, plan, eg, d), a.iters, a.reps)
    ubp = timed(lambda: de.device_ops.sparse_segment_combine_backprop(G, st, wt, "mean"), a.iters, a.reps)
    print(json.dumps({"opt": name, "nnz": int(ids.size), "unique": int(np.unique(ids).size), "dim": dim, "table_keys": a.keys,
                      "a_backprop_plus_apply_sparse_us": round(ua, 2), "b_apply_planned_combined_us": round(ub, 2),
                      "c_apply_planned_expanded_us": round(uc, 2), "backprop_alone_us": round(ubp, 2),
                      "table_size": int(var.size())}), flush=True)
    del var, plan


if __name__ == "__main__":
  main()
