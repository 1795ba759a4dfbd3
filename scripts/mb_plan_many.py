"""The write-back plans of a many-table model built two ways, in ONE process, alternating over the same ids: --plans (26) plans,
dims cycling 16 / 32 / 64 / 128, per plan one batch of 8 192 x 4 Zipf-1.2 ids, fresh ids every step from a pre-generated pool:
  A  the loop of single builds on one stream: one SparsePlan.build (tfra_sparse_plan_build, 3 launches) per plan — the code of the
     parent commit
  B  the grouped build: ONE table_ops.build_plans_many (tfra_multi_sparse_plan_build, 3 launches)
and the same pair with ONE plan in the list (what the grouping costs where it cannot help), with 26 plans of 131 072 ids (where the
kernels rather than the launches should dominate), and the whole sparse step of --plans tables — embedding_lookup_sparse_many(
plan_writeback=True) -> apply_combined_gradients_many — with the plans started per variable on the variables' own side streams (A,
the parent commit's path: `_plans_at_lookup_many` switched off) and by one grouped build on one side stream (B).
Each form has its own plan objects (and, for the step, its own twin tables).  After the warm-up the two forms' plans are compared
key by key (tfra_sparse_plan_read), the step's tables bit for bit.
HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one JSON line per point (median, min
and max of the windows, us per step, host calls included; whether the gap between the medians exceeds the spread of A's own
windows), written to --out.
   python scripts/mb_plan_many.py [--plans 26] [--steps 20] [--windows 5] [--warmup 5] [--out profiles/plan_many_mb.jsonl]
   --only A|B: that form alone, first point only, no comparison (for a kernel trace of one form in a run of its own)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402
from tfra_amd.dynamic_embedding import table_ops, variable  # noqa: E402

N_ROWS, PER_ROW = 8192, 4
DIMS = (16, 32, 64, 128)
POOL = 8
KEYS = 200_000


def read_sorted(plan):
  counts, keys, cnt, pos = plan.read()
  o = np.argsort(keys, kind="stable")
  return keys[o], cnt[o], counts["many"], counts["errors"]


def timed(fn, steps, windows, forms):
  us = {f: [] for f in forms}
  for wi in range(windows):
    for f in forms:   # alternating: both forms run window wi's steps
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for s in range(steps):
        fn(f, wi * steps + s)
      e1.record()
      e1.synchronize()
      torch.cuda.synchronize()
      us[f].append(e0.elapsed_time(e1) * 1000.0 / steps)
  return us


def summary(out, us, forms, names):
  for f in forms:
    out[names[f]] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                     "windows": [round(x, 2) for x in us[f]]}
  if len(forms) == 2:
    A, B = out[names["A"]], out[names["B"]]
    out["A_spread_us"] = round(A["max"] - A["min"], 2)
    out["B_below_A_by_more_than_A_spread"] = bool(A["median"] - B["median"] > A["max"] - A["min"])
    out["B_above_A_by_more_than_A_spread"] = bool(B["median"] - A["median"] > A["max"] - A["min"])
  return out


def build_point(a, forms, label, n_plans, n_ids, rng):
  dims = [DIMS[j % 4] for j in range(n_plans)] if n_plans > 1 else [64]
  ids = [[torch.from_numpy(((rng.zipf(1.2, size=n_ids) - 1) % KEYS).astype(np.int64) * 7919 + 1).cuda() for _ in range(n_plans)]
         for _ in range(POOL)]
  plans = {f: [table_ops.SparsePlan("cuda:%d" % torch.cuda.current_device(), d) for d in dims] for f in forms}
  launches = [0]

  def step(f, s):
    batch = ids[s % POOL]
    if f == "A":
      for pl, t in zip(plans[f], batch):
        pl.build(t)
    else:
      launches[0] = table_ops.build_plans_many(plans[f], batch, return_launches=True)[1]

  for s in range(a.warmup):
    for f in forms:
      step(f, s)
  if len(forms) == 2:
    for pa, pb in zip(plans["A"], plans["B"]):
      x, y = read_sorted(pa), read_sorted(pb)
      assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:] and x[3] == 0, "A and B differ"
  torch.cuda.synchronize()
  us = timed(step, a.steps, a.windows, forms)
  out = {"point": label, "plans": n_plans, "dims": dims[:4], "ids_per_plan": n_ids, "steps_per_window": a.steps,
         "A_kernel_launches_per_step": 3 * n_plans, "B_kernel_launches_per_step": launches[0]}
  return summary(out, us, forms, {"A": "A_loop_of_plan_build_us", "B": "B_build_plans_many_us"})


def step_point(a, n_tables, rng):
  """lookup (plans started at lookup time) -> gradient -> write-back, per-variable side streams (A) against one grouped build (B)"""
  nnz = N_ROWS * PER_ROW
  adam = de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(adam)
  resident = torch.arange(KEYS, dtype=torch.int64, device="cuda") * 7919 + 1
  seg = (torch.arange(nnz, device="cuda") // PER_ROW).to(torch.int64)
  tabs = {f: [] for f in "AB"}
  for j in range(n_tables):
    for f in "AB":
      var = de.Variable(dim=DIMS[j % 4], name="mb_pm_%s_%d" % (f, j), initializer=0.0, init_size=2 * KEYS, **kw)
      var.upsert(resident, torch.full((KEYS, DIMS[j % 4]), 0.01 * (j + 1), device="cuda"))
      tabs[f].append(var)
  ids = [[torch.from_numpy(((rng.zipf(1.2, size=nnz) - 1) % KEYS).astype(np.int64) * 7919 + 1).cuda() for _ in range(n_tables)]
         for _ in range(POOL)]
  grads = [torch.randn((N_ROWS, DIMS[j % 4]), generator=torch.Generator(device="cuda").manual_seed(j), device="cuda") * 0.01
           for j in range(n_tables)]
  deo = {f: de.DynamicEmbeddingOptimizer(adam) for f in "AB"}
  grouped = variable._plans_at_lookup_many

  def step(f, s):
    variable._plans_at_lookup_many = grouped if f == "B" else (lambda device, members: None)
    try:
      res = de.embedding_lookup_sparse_many(tabs[f], [(seg, t) for t in ids[s % POOL]], None, combiner="mean", return_trainable=True,
                                            num_rows=N_ROWS, plan_writeback=True)
    finally:
      variable._plans_at_lookup_many = grouped
    deo[f].apply_combined_gradients_many([(g, tw) for g, (_, tw) in zip(grads, res)])

  for s in range(a.warmup):
    for f in "AB":
      step(f, s)
  for va, vb in zip(tabs["A"], tabs["B"]):
    x, y = va.lookup(resident[:4096]), vb.lookup(resident[:4096])
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "A and B differ"
  torch.cuda.synchronize()
  us = timed(step, a.steps, a.windows, "AB")
  out = {"point": "whole sparse step, %d tables" % n_tables, "tables": n_tables, "ids_per_table": nnz, "steps_per_window": a.steps,
         "resident_keys_per_table": KEYS}
  return summary(out, us, "AB", {"A": "A_plans_per_variable_side_streams_us", "B": "B_one_grouped_build_one_side_stream_us"})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--plans", type=int, default=26)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--only", choices=["A", "B"], default=None)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_plan_many: no GPU visible; this is a measurement, it has no CPU form")
  forms = a.only or "AB"
  rng = np.random.default_rng(0)
  lines = []

  def emit(out):
    line = json.dumps(out)
    print(line, flush=True)
    lines.append(line)

  emit(build_point(a, forms, "%d plans" % a.plans, a.plans, N_ROWS * PER_ROW, rng))
  if not a.only:
    emit(build_point(a, forms, "1 plan", 1, N_ROWS * PER_ROW, rng))
    emit(build_point(a, forms, "%d plans of 131072 ids" % a.plans, a.plans, 131072, rng))
    emit(step_point(a, a.plans, rng))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
