"""Momentum, Nesterov and RMSProp through the Generic route and through the fused write-backs, in ONE process and one build,
alternating:
  generic  optimizers.Momentum / RMSProp(...)              reduce by key + a host read of the unique count, (1+S) finds, the rule as
                                                           torch ops on [U, dim], (1+S) upserts — DynamicEmbeddingOptimizer._apply_generic
  fused    optimizers.Momentum / RMSProp(..., fused=True)  tfra_table_apply_sparse: apply_csr_kernel<TFRA_OPT_MOMENTUM / _NESTEROV / _RMSPROP>
Sparse cases (float32 dim 64, float16 dim 128): B = 131 072 Zipf-1.2 ids, about 10 % of every batch never seen before, growing
table pre-filled with --keys rows, through DynamicEmbeddingOptimizer.apply_sparse.  Combined case: a 26-variable step —
embedding_lookup_sparse_many(..., return_trainable=True) + apply_combined_gradients_many, 8 192 rows x 4 ids per table, float32
dim 64, RMSProp.  Each form has tables of its own and sees the same batches.  HIP events around windows of --steps steps, --windows
windows per form after --warmup steps; prints one JSON line per case: median, min and max of the windows in us per step, the
difference of the medians and the two spreads (max - min) it has to be read against.
   python scripts/mb_fused_rules.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--tables 26]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

FORMS = ("generic", "fused")
RULES = {
    "momentum": lambda fused: de.optimizers.Momentum(0.05, 0.9, fused=fused),
    "nesterov": lambda fused: de.optimizers.Momentum(0.05, 0.9, use_nesterov=True, fused=fused),
    "rmsprop": lambda fused: de.optimizers.RMSProp(0.01, 0.9, 0.5, 1e-10, fused=fused),
}


def windows(a, step_of):
  """us per step of every window and form: alternating, and alternating which form goes first."""
  us = {f: [] for f in FORMS}
  for w in range(a.windows):
    for f in (FORMS if w % 2 == 0 else FORMS[::-1]):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for s in range(a.steps):
        step_of(f, a.warmup + w * a.steps + s)
      e1.record()
      e1.synchronize()
      us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
  return us


def report(out, us):
  for f in FORMS:
    out[f + "_us"] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                      "windows": [round(x, 2) for x in us[f]]}
  out["generic_minus_fused_us"] = round(out["generic_us"]["median"] - out["fused_us"]["median"], 2)
  out["sum_of_spreads_us"] = round(sum(out[f + "_us"]["max"] - out[f + "_us"]["min"] for f in FORMS), 2)
  out["fused_faster_by_more_than_the_spreads"] = bool(out["generic_minus_fused_us"] > out["sum_of_spreads_us"])
  print(json.dumps(out), flush=True)


def sparse_cases(a):
  B = 131072
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
  rkeys = torch.from_numpy(resident).cuda()
  for vd, dim in (("float32", 64), ("float16", 128)):
    dt = getattr(torch, vd)
    g = torch.from_numpy((rng.standard_normal((B, dim)) * 0.01).astype(np.float32)).cuda()
    for rule, make in RULES.items():
      vs, deos = {}, {}
      for f in FORMS:
        opt = make(f == "fused")
        var = de.Variable(dim=dim, name="mb_fr_%s_%d_%s_%s" % (vd, dim, rule, f), value_dtype=dt, initializer=0.0,
                          init_size=2 * a.keys + 2 * n_steps * B // 10, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
        for off in range(0, a.keys, 1 << 18):
          k = rkeys[off:off + (1 << 18)]
          var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
        vs[f], deos[f] = var, de.DynamicEmbeddingOptimizer(opt)
      step_of = lambda f, s: deos[f].apply_sparse(vs[f], batches[s], g)
      for f in FORMS:
        for s in range(a.warmup):
          step_of(f, s)
      torch.cuda.synchronize()
      us = windows(a, step_of)
      for f in FORMS:
        vs[f]._tables[0]._table.check_errors()
      sizes = {f: int(vs[f].size()) for f in FORMS}
      assert sizes["generic"] == sizes["fused"], sizes
      # the two forms compute one rule: the rows agree up to the association of the duplicate sums
      probe = batches[a.warmup][:4096]
      diff = float((vs["generic"].lookup(probe).float() - vs["fused"].lookup(probe).float()).abs().max())
      report({"case": "apply_sparse", "dtype": vd, "dim": dim, "rule": rule, "batch": B, "resident_keys": a.keys,
              "steps_per_window": a.steps, "unique_per_batch": int(torch.unique(batches[a.warmup]).numel()),
              "table_size_after": sizes["fused"], "max_abs_row_difference": diff}, us)
      del vs, deos


def combined_case(a):
  nt, rows, per_row, dim, keys = a.tables, 8192, 4, 64, 200_000
  rng = np.random.default_rng(1)
  n_batches = 8   # the steps cycle over these
  seg = torch.from_numpy(np.repeat(np.arange(rows, dtype=np.int64), per_row)).cuda()
  ids = [[torch.from_numpy(((rng.zipf(1.2, size=rows * per_row) - 1) % keys).astype(np.int64) * 7919 + 1).cuda() for _ in range(nt)]
         for _ in range(n_batches)]
  g = [torch.from_numpy((rng.standard_normal((rows, dim)) * 0.01).astype(np.float32)).cuda() for _ in range(nt)]
  rkeys = torch.arange(keys, dtype=torch.int64, device="cuda") * 7919 + 1
  vs, deos = {}, {}
  for f in FORMS:
    opt = RULES["rmsprop"](f == "fused")
    vs[f] = []
    for i in range(nt):
      var = de.Variable(dim=dim, name="mb_fr_comb_%s_%d" % (f, i), initializer=0.0, init_size=2 * keys,
                        **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
      var.upsert(rkeys, torch.full((keys, dim), 0.01, device="cuda"))
      vs[f].append(var)
    deos[f] = de.DynamicEmbeddingOptimizer(opt)

  def step_of(f, s):
    b = ids[s % n_batches]
    res = de.embedding_lookup_sparse_many(vs[f], [(seg, b[i]) for i in range(nt)], None, combiner="mean", return_trainable=True,
                                          num_rows=rows)
    deos[f].apply_combined_gradients_many([(g[i], res[i][1]) for i in range(nt)])

  for f in FORMS:
    for s in range(a.warmup):
      step_of(f, s)
  torch.cuda.synchronize()
  us = windows(a, step_of)
  for f in FORMS:
    for v in vs[f]:
      v._tables[0]._table.check_errors()
  diff = max(float((x.lookup(rkeys[:4096]) - y.lookup(rkeys[:4096])).abs().max()) for x, y in zip(vs["generic"], vs["fused"]))
  report({"case": "combined_many", "dtype": "float32", "dim": dim, "rule": "rmsprop", "tables": nt, "rows": rows, "ids_per_row": per_row,
          "resident_keys_per_table": keys, "steps_per_window": a.steps, "max_abs_row_difference": diff}, us)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--tables", type=int, default=26)
  ap.add_argument("--only", choices=("sparse", "combined"), default=None)
  a = ap.parse_args()
  if a.only != "combined":
    sparse_cases(a)
  if a.only != "sparse":
    combined_case(a)


if __name__ == "__main__":
  main()
