"""Sparse write-back of a batch whose gradients are held in float16 / bfloat16, three ways, in ONE process, alternating
(B = 131 072 Zipf-1.2 ids, about 10 % of every batch never seen before, growing table pre-filled with --keys rows; tables float32
dim 64 and bfloat16 dim 128, SGD and Adam; gradients float16 with a loss scale to undo, bfloat16 without one):
  i    grad.to(float32) (float16: * scale) + tfra_table_apply_sparse     (what such a caller did before the typed calls)
  ii   tfra_table_apply_sparse_typed on the half matrix, the scale read by the kernels
  iii  tfra_table_apply_sparse on gradients that are float32 already, for scale
Each route has a table of its own and sees the same batches.  HIP events around windows of --steps steps, --windows windows per
route after --warmup steps; prints one JSON line per (table, rule, gradient format): median, min and max of the windows, us per
step, and whether ii is below i by more than the sum of both spreads (max - min).
   python scripts/mb_half_grads.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

ROUTES = ("i", "ii", "iii")
LABELS = {"i": "i_upcast_plus_apply_sparse_us", "ii": "ii_apply_sparse_typed_us", "iii": "iii_apply_sparse_f32_grads_us"}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--batch", type=int, default=131072)
  a = ap.parse_args()
  B = a.batch
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
  inv_scale = torch.full((1,), 1.0 / 1024, dtype=torch.float32, device="cuda")

  def table(name, opt, dt, dim):
    var = de.Variable(dim=dim, name=name, value_dtype=dt, initializer=0.0, init_size=2 * a.keys + 2 * n_steps * B // 10,
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    for off in range(0, a.keys, 1 << 18):
      k = rkeys[off:off + (1 << 18)]
      var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
    return var

  for vd, dim in (("float32", 64), ("bfloat16", 128)):
    g32_base = torch.from_numpy((rng.standard_normal((B, dim)) * 0.01).astype(np.float32)).cuda()
    for oname, opt in (("sgd", de.optimizers.SGD(0.01)), ("adam", de.optimizers.Adam(1e-3))):
      for gd in ("float16", "bfloat16"):
        scale = inv_scale if gd == "float16" else None   # loss scaling belongs to float16
        gh = (g32_base * 1024 if scale is not None else g32_base).to(getattr(torch, gd)).contiguous()
        g32 = gh.to(torch.float32) * scale if scale is not None else gh.to(torch.float32)   # route iii reads what i and ii form
        p = opt.params(1)
        vs = {r: table("mb_hg_%s_%s_%s_%s" % (vd, oname, gd, r), opt, getattr(torch, vd), dim) for r in ROUTES}
        ts = {r: v._tables[0] for r, v in vs.items()}
        ds = {r: t._default_value.to(torch.float32) for r, t in ts.items()}

        def step(r, ids):
          t = ts[r]._table
          if r == "i":
            g = gh.to(torch.float32)
            if scale is not None:
              g = g * scale
            t.apply_sparse(p, ids, g, ds[r])
          elif r == "ii":
            t.apply_sparse(p, ids, gh, ds[r], grad_scale=scale)
          else:
            t.apply_sparse(p, ids, g32, ds[r])

        for r in ROUTES:
          for s in range(a.warmup):
            step(r, batches[s])
        torch.cuda.synchronize()
        us = {r: [] for r in ROUTES}
        for w in range(a.windows):
          for r in ROUTES:   # alternating: every route sees window w's batches on its own table
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(a.steps):
              step(r, batches[a.warmup + w * a.steps + s])
            e1.record()
            e1.synchronize()
            us[r].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
        for r in ROUTES:
          ts[r]._table.check_errors()
        sizes = {r: int(vs[r].size()) for r in ROUTES}
        assert sizes["i"] == sizes["ii"] == sizes["iii"], sizes
        keys = batches[a.warmup][:4096]
        same = all(torch.equal(vs["i"].lookup(keys).view(torch.int16 if vd == "bfloat16" else torch.int32),
                               vs[r].lookup(keys).view(torch.int16 if vd == "bfloat16" else torch.int32)) for r in ("ii", "iii"))
        out = {"table": vd, "dim": dim, "opt": oname, "grads": gd, "scale": scale is not None, "batch": B, "resident_keys": a.keys,
               "steps_per_window": a.steps, "windows_n": a.windows, "unique_per_batch": int(torch.unique(batches[a.warmup]).numel()),
               "table_size_after": sizes["ii"], "rows_bit_identical": bool(same)}
        for r in ROUTES:
          out[LABELS[r]] = {"median": round(float(np.median(us[r])), 2), "min": round(min(us[r]), 2), "max": round(max(us[r]), 2),
                            "windows": [round(x, 2) for x in us[r]]}
        spread = lambda r: max(us[r]) - min(us[r])
        gain = float(np.median(us["i"]) - np.median(us["ii"]))
        out["ii_below_i_us"] = round(gain, 2)
        out["sum_of_spreads_us"] = round(spread("i") + spread("ii"), 2)
        out["ii_clears_the_bar"] = bool(gain > spread("i") + spread("ii"))
        print(json.dumps(out), flush=True)
        del vs, ts


if __name__ == "__main__":
  main()
