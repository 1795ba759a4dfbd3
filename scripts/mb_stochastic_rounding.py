"""Sparse write-back of a half-precision table with TFRA_OPTION_STOCHASTIC_ROUNDING off and on, in ONE process and one build,
alternating (B = 131 072 Zipf-1.2 ids, about 10 % of every batch never seen before, growing table pre-filled with --keys rows;
float16 and bfloat16, dim 128 and 64, SGD and Adam):
  off  tfra_table_apply_sparse on a table that never had the option: apply_csr_kernel<KIND, .., ST>, the parent's code
  on   the same call on a table with a seed: apply_csr_kernel<KIND, .., ST, StochP> (three 64-bit hashes per lane, field and granule)
Each form has a table of its own and sees the same batches.  HIP events around windows of --steps steps, --windows windows per
form after --warmup steps; prints one JSON line per (dtype, dim, optimizer): median, min and max of the windows in us per step,
the difference of the medians and the two spreads (max - min) it has to be read against.
   python scripts/mb_stochastic_rounding.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

FORMS = ("off", "on")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
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

  for vd in ("float16", "bfloat16"):
    for dim in (128, 64):
      g = torch.from_numpy((rng.standard_normal((B, dim)) * 0.01).astype(np.float32)).cuda()
      for oname, opt in (("sgd", de.optimizers.SGD(0.01)), ("adam", de.optimizers.Adam(1e-3))):
        dt = getattr(torch, vd)
        p = opt.params(1)
        vs = {}
        for f in FORMS:
          var = de.Variable(dim=dim, name="mb_sr_%s_%d_%s_%s" % (vd, dim, oname, f), value_dtype=dt, initializer=0.0,
                            init_size=2 * a.keys + 2 * n_steps * B // 10, stochastic_rounding=0x5EED if f == "on" else None,
                            **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
          for off in range(0, a.keys, 1 << 18):
            k = rkeys[off:off + (1 << 18)]
            var.upsert(k, torch.full((k.numel(), dim), 0.01, dtype=dt, device="cuda"))
          vs[f] = var
        ts = {f: v._tables[0]._table for f, v in vs.items()}
        ds = {f: v._tables[0]._default_value.to(torch.float32) for f, v in vs.items()}
        for f in FORMS:
          for s in range(a.warmup):
            ts[f].apply_sparse(p, batches[s], g, ds[f])
        torch.cuda.synchronize()
        us = {f: [] for f in FORMS}
        for w in range(a.windows):
          for f in (FORMS if w % 2 == 0 else FORMS[::-1]):   # alternating, and alternating which form goes first
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(a.steps):
              ts[f].apply_sparse(p, batches[a.warmup + w * a.steps + s], g, ds[f])
            e1.record()
            e1.synchronize()
            us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
        for f in FORMS:
          ts[f].check_errors()
        sizes = {f: int(vs[f].size()) for f in FORMS}
        assert sizes["off"] == sizes["on"], sizes
        # the two tables hold different bits: the option is on where it should be
        probe = batches[a.warmup][:4096]
        assert not torch.equal(vs["off"].lookup(probe).view(torch.int16), vs["on"].lookup(probe).view(torch.int16))
        out = {"dtype": vd, "dim": dim, "opt": oname, "batch": B, "resident_keys": a.keys, "steps_per_window": a.steps,
               "unique_per_batch": int(torch.unique(batches[a.warmup]).numel()), "table_size_after": sizes["on"]}
        for f in FORMS:
          out[f + "_us"] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                            "windows": [round(x, 2) for x in us[f]]}
        out["on_minus_off_us"] = round(out["on_us"]["median"] - out["off_us"]["median"], 2)
        out["sum_of_spreads_us"] = round(sum(out[f + "_us"]["max"] - out[f + "_us"]["min"] for f in FORMS), 2)
        print(json.dumps(out), flush=True)
        del vs, ts


if __name__ == "__main__":
  main()
