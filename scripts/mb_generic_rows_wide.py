"""The Generic route of a dense update rule on a WIDE variable (256 < dim <= 1024) with and without whole_rows, both under
DynamicEmbeddingOptimizer(opt, wide_rows=True), in ONE process and one build, alternating (the protocol of scripts/mb_generic_rows.py):
  generic      whole_rows=False  unique + segment_sum + a host read of the unique count, (1+S) finds, the rule as torch ops on
                                 [U, dim], (1+S) upserts — _apply_generic, what such a variable does without the keyword
  whole_rows   whole_rows=True   a wide plan build, tfra_table_fetch_planned_wide, the same host read, the same torch ops,
                                 tfra_table_store_rows_wide — _apply_generic_rows
  table_calls  for scale: the plan build and the two table calls of whole_rows alone, the count staying on the device (no host
               read, no rule) on a table of its own; whole_rows minus table_calls is the rule's torch kernels plus the host read
Shapes: float32 dim 512 and bfloat16 dim 1024, each with Momentum (one slot) and an AdamW-shaped two-slot Generic rule.
B = 131 072 Zipf-1.2 ids, about 10 % of every batch never seen before, growing table pre-filled with --keys rows.  Each route has a
table of its own and sees the same batches.  HIP events around windows of --steps steps, --windows windows per route after --warmup
steps; prints one JSON line per shape: median, min and max of the windows in us per step, generic minus whole_rows and the two
spreads (max - min) it has to be read against.  The two routes sum duplicate gradients in different orders (sequential | the plan's
tree), so their tables are compared within a tolerance, not bit for bit: the largest difference is printed.
   python scripts/mb_generic_rows_wide.py [--keys 2000000] [--steps 10] [--windows 7] [--warmup 3] [--out profiles/generic_rows_wide_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402
from tfra_amd.dynamic_embedding.table_ops import SparsePlan  # noqa: E402

ROUTES = ("generic", "whole_rows", "table_calls")


def adamw(step, p, g, m, v):
  m = m * 0.9 + g * 0.1
  v = v * 0.999 + g * g * 0.001
  return p - 0.01 * (m / (v.sqrt() + 1e-8) + 0.01 * p), m, v


RULES = {
    "momentum": lambda whole: de.optimizers.Momentum(0.05, 0.9, whole_rows=whole),
    "adamw_two_slots": lambda whole: de.optimizers.Generic(slots=("m", "v"), slot_init=(0.0, 0.0), update=adamw, whole_rows=whole),
}
SHAPES = (("float32", 512, "momentum"), ("float32", 512, "adamw_two_slots"), ("bfloat16", 1024, "momentum"),
          ("bfloat16", 1024, "adamw_two_slots"))


def windows(a, step_of):
  """us per step of every window and route: alternating, and rotating which route goes first."""
  us = {r: [] for r in ROUTES}
  for w in range(a.windows):
    k = w % len(ROUTES)
    for r in ROUTES[k:] + ROUTES[:k]:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for s in range(a.steps):
        step_of(r, a.warmup + w * a.steps + s)
      e1.record()
      e1.synchronize()
      us[r].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
  return us


def state(var, deo):
  """The keys in ascending order, and behind them the embedding and every slot as float32."""
  k, v = var.export()
  o = torch.argsort(k)
  k = k[o]
  return [k, v[o].float()] + [deo.get_slot(var, s).lookup(k).float() for s in deo.opt.slots]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
  a = ap.parse_args()
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
  for vd, dim, rule in SHAPES:
    dt = getattr(torch, vd)
    g = torch.from_numpy((rng.standard_normal((B, dim)) * 0.01).astype(np.float32)).cuda()
    vs, deos = {}, {}
    for r in ROUTES:
      opt = RULES[rule](r != "generic")
      var = de.Variable(dim=dim, name="mb_grw_%s_%d_%s_%s" % (vd, dim, rule, r), value_dtype=dt, initializer=0.0,
                        init_size=2 * a.keys + 2 * n_steps * B // 10, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
      for off in range(0, a.keys, 1 << 18):
        k = rkeys[off:off + (1 << 18)]
        var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
      vs[r], deos[r] = var, de.DynamicEmbeddingOptimizer(opt, wide_rows=True)
    plan = SparsePlan(vs["table_calls"]._primary, dim)

    def step_of(r, s):
      if r != "table_calls":
        return deos[r].apply_sparse(vs[r], batches[s], g)
      t = vs[r]._tables[0]._table
      keys, fields, gsum, cnt = t.fetch_planned_wide(plan.build(batches[s]), grads=g)
      t.store_rows_wide(keys, fields, count=cnt)

    for r in ROUTES:
      for s in range(a.warmup):
        step_of(r, s)
    torch.cuda.synchronize()
    us = windows(a, step_of)
    for r in ROUTES:
      vs[r]._tables[0]._table.check_errors()
    out = {"case": "apply_sparse", "dtype": vd, "dim": dim, "rule": rule, "batch": B, "resident_keys": a.keys,
           "steps_per_window": a.steps, "unique_per_batch": int(torch.unique(batches[a.warmup]).numel())}
    for r in ROUTES:
      out[r + "_us"] = {"median": round(float(np.median(us[r])), 2), "min": round(min(us[r]), 2), "max": round(max(us[r]), 2),
                        "windows": [round(x, 2) for x in us[r]]}
    out["generic_minus_whole_rows_us"] = round(out["generic_us"]["median"] - out["whole_rows_us"]["median"], 2)
    out["sum_of_spreads_us"] = round(sum(out[r + "_us"]["max"] - out[r + "_us"]["min"] for r in ("generic", "whole_rows")), 2)
    out["whole_rows_faster_by_more_than_the_spreads"] = bool(out["generic_minus_whole_rows_us"] > out["sum_of_spreads_us"])
    out["rule_and_host_read_us"] = round(out["whole_rows_us"]["median"] - out["table_calls_us"]["median"], 2)
    ref, got = state(vs["generic"], deos["generic"]), state(vs["whole_rows"], deos["whole_rows"])
    out["table_size_after"] = int(ref[0].numel())
    out["same_keys_as_generic"] = bool(torch.equal(ref[0], got[0]))
    out["max_abs_difference_to_generic"] = max(float((x - y).abs().max()) for x, y in zip(ref[1:], got[1:])) if out["same_keys_as_generic"] else None
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
      with open(a.out, "a") as f:
        f.write(line + "\n")
    del vs, deos, ref, got, plan
    torch.cuda.empty_cache()
    assert out["same_keys_as_generic"], "the whole_rows table does not hold the generic table's keys"


if __name__ == "__main__":
  main()
