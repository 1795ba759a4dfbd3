"""The Generic route of a dense update rule with and without whole_rows, and the fused write-back for scale, in ONE process and one
build, alternating (the protocol of scripts/mb_fused_rules.py):
  generic     optimizers.Momentum / RMSProp(...)                   reduce by key + a host read of the unique count, (1+S) finds, the rule
                                                                   as torch ops on [U, dim], (1+S) upserts — _apply_generic
  whole_rows  optimizers.Momentum / RMSProp(..., whole_rows=True)  a plan build, tfra_table_fetch_planned, the same host read, the same
                                                                   torch ops, tfra_table_store_rows — _apply_generic_rows
  fused       optimizers.Momentum / RMSProp(..., fused=True)       tfra_table_apply_sparse
Shapes: float32 dim 64 with Momentum and RMSProp, float16 dim 128 with RMSProp.  B = 131 072 Zipf-1.2 ids, about 10 % of every
batch never seen before, growing table pre-filled with --keys rows, through DynamicEmbeddingOptimizer.apply_sparse.  Each route has
tables of its own and sees the same batches.  HIP events around windows of --steps steps, --windows windows per route after
--warmup steps; prints one JSON line per shape: median, min and max of the windows in us per step, generic minus whole_rows and the
two spreads (max - min) it has to be read against.  Every route's table must end with the same keys and the same bits in the
embedding and in every slot: asserted behind the shape's line.
   python scripts/mb_generic_rows.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--out profiles/generic_rows_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

ROUTES = ("generic", "whole_rows", "fused")
RULES = {
    "momentum": lambda r: de.optimizers.Momentum(0.05, 0.9, fused=r == "fused", whole_rows=r == "whole_rows"),
    "rmsprop": lambda r: de.optimizers.RMSProp(0.01, 0.9, 0.5, 1e-10, fused=r == "fused", whole_rows=r == "whole_rows"),
}
SHAPES = (("float32", 64, "momentum"), ("float32", 64, "rmsprop"), ("float16", 128, "rmsprop"))


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


def bits(t):
  return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def state(var, deo):
  """The keys in ascending order, and behind them the bits of the embedding and of every slot."""
  k, v = var.export()
  o = torch.argsort(k)
  k = k[o]
  return [k, bits(v[o])] + [bits(deo.get_slot(var, s).lookup(k)) for s in deo.opt.slots]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
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
  mismatches = []
  for vd, dim, rule in SHAPES:
    dt = getattr(torch, vd)
    g = torch.from_numpy((rng.standard_normal((B, dim)) * 0.01).astype(np.float32)).cuda()
    vs, deos = {}, {}
    for r in ROUTES:
      opt = RULES[rule](r)
      var = de.Variable(dim=dim, name="mb_gr_%s_%d_%s_%s" % (vd, dim, rule, r), value_dtype=dt, initializer=0.0,
                        init_size=2 * a.keys + 2 * n_steps * B // 10, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
      for off in range(0, a.keys, 1 << 18):
        k = rkeys[off:off + (1 << 18)]
        var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
      vs[r], deos[r] = var, de.DynamicEmbeddingOptimizer(opt)
    step_of = lambda r, s: deos[r].apply_sparse(vs[r], batches[s], g)
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
    ref = state(vs["generic"], deos["generic"])
    out["table_size_after"] = int(ref[0].numel())
    for r in ROUTES[1:]:
      got = state(vs[r], deos[r])
      same = len(got) == len(ref) and all(x.shape == y.shape and bool(torch.equal(x, y)) for x, y in zip(got, ref))
      out[r + "_bit_identical_to_generic"] = same
      if not same:
        mismatches.append((vd, dim, rule, r))
      del got
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
      with open(a.out, "a") as f:
        f.write(line + "\n")
    del vs, deos, ref
    torch.cuda.empty_cache()
  assert not mismatches, "routes whose tables do not end bit-identical to the generic route's: %r" % (mismatches,)


if __name__ == "__main__":
  main()
