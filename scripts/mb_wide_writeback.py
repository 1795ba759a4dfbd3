"""The wide sparse write-back (256 < dim <= 1024, DynamicEmbeddingOptimizer(wide_rows=True)) against the route such a variable has
without it (wide_rows=False), in ONE process, alternating on the same batches.  Two growing tables per case, pre-filled with
--keys rows each, one per route (a write-back changes its table); nnz = B = 131 072 Zipf-1.2 ids per batch:
  S   apply_sparse today: unique_no_sync + segment_sum + apply_optimizer
  SW  apply_sparse, wide_rows=True: tfra_table_apply_sparse_wide (plan build, sums, one wave per key)
  C   apply_combined_gradients today: the expanded [nnz, dim] entry gradient, then route S
  CW  apply_combined_gradients, wide_rows=True: plan build + tfra_table_apply_planned_combined_wide
Shapes: dim 512 float32 and dim 1024 bfloat16, SGD and Adam, apply_sparse and the combined write-back at 16 entries per row; dim 512
also at 1 and 256 entries per row.  HIP events around windows of --steps steps, --windows windows per form after --warmup steps; one
JSON line per case (median, min and max of the windows, us per step), written to --out.  A route "wins" only beyond the sum of both
spreads (max - min).
   python scripts/mb_wide_writeback.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 3] [--out profiles/wide_writeback_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402


def beyond_spreads(a, b):
  """a's median below b's by more than the sum of both spreads"""
  return bool(b["median"] - a["median"] > (a["max"] - a["min"]) + (b["max"] - b["min"]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=3)
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
    for rule in ("sgd", "adam"):
      opt = de.optimizers.SGD(0.01) if rule == "sgd" else de.optimizers.Adam(1e-3)
      deos = {False: de.DynamicEmbeddingOptimizer(opt), True: de.DynamicEmbeddingOptimizer(opt, wide_rows=True)}
      tabs = {}
      gen = torch.Generator(device="cuda").manual_seed(dim)
      for wide in (False, True):
        tabs[wide] = de.Variable(dim=dim, name="mb_ww_%d_%s_%s_%d" % (dim, vd, rule, wide), value_dtype=dt, initializer=0.0,
                                 init_size=2 * a.keys, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
        for off in range(0, a.keys, 1 << 17):
          k = rkeys[off:off + (1 << 17)]
          tabs[wide].upsert(k, (torch.randn((k.numel(), dim), generator=gen, device="cuda") * 0.1).to(dt))
      G = torch.randn((B, dim), generator=gen, device="cuda") * 0.01
      for form, per_row in (("sparse", 0), ("combined", 16)) + ((("combined", 1), ("combined", 256)) if dim == 512 else ()):
        n_rows = B // max(per_row, 1)
        seg = (torch.arange(B, device="cuda") // max(per_row, 1)).to(torch.int64)

        def step(wide, s):
          var, deo, ids = tabs[wide], deos[wide], batches[s]
          if form == "sparse":
            return deo.apply_sparse(var, ids, G)
          _, tw = de.embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", num_rows=n_rows, return_trainable=True)
          torch.cuda.synchronize()   # (the lookup is not what is timed: see the events below)
          return tw

        def timed(wide, lo, n):
          """us per step of n steps; the combined form's lookups run ahead, only the write-backs stand between the events"""
          tws = [step(wide, lo + i) for i in range(n)] if form == "combined" else None
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for i in range(n):
            if form == "combined":
              deos[wide].apply_combined_gradients([(G[:n_rows], tws[i])])
            else:
              step(wide, lo + i)
          e1.record()
          e1.synchronize()
          return e0.elapsed_time(e1) * 1000.0 / n

        for wide in (False, True):
          timed(wide, 0, a.warmup)
        us = {False: [], True: []}
        for wi in range(a.windows):
          for wide in (False, True):   # alternating: both routes see window wi's batches
            us[wide].append(timed(wide, a.warmup + wi * a.steps, a.steps))
        out = {"dim": dim, "dtype": vd, "rule": rule, "form": form, "per_row": per_row, "nnz": B, "resident_keys": a.keys,
               "steps_per_window": a.steps}
        for wide, label in ((False, "today_us"), (True, "wide_us")):
          tabs[wide]._tables[0]._table.check_errors()
          out[label] = {"median": round(float(np.median(us[wide])), 2), "min": round(min(us[wide]), 2), "max": round(max(us[wide]), 2),
                        "windows": [round(x, 2) for x in us[wide]]}
        out["wide_wins"] = beyond_spreads(out["wide_us"], out["today_us"])
        out["wide_loses"] = beyond_spreads(out["today_us"], out["wide_us"])
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        if a.out:   # (kept up to date case by case)
          os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
          with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
      del tabs


if __name__ == "__main__":
  main()
