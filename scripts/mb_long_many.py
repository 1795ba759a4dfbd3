"""The grouped pooled calls with long members against the two routes a many-table model with sequence features has without
them, in ONE process, alternating on the same batches.  26 float32 tables of dims 16 / 32 / 64 / 128 over --keys resident keys in
all, Zipf-1.2 ids, random weights and grad_out, combiner mean: 22 categorical features (8 192 rows x 4 ids) and 4 histories
(512 rows x 256 ids).  For the forward and the weight gradient, tuple and ragged form:
  a  today's grouped call with the histories in it (one 16-lane group per row for every member)
  b  today's grouped call for the 22, plus a loop of four single *_long calls
  c  the grouped call with long_rows flagged for the histories (tfra_multi_find_combine*_long)
  s  one history alone: the single *_long call          g  the same member as a list of one, flagged
HIP events around windows of --steps calls, --windows windows per route after --warmup calls; one JSON line per (operation,
form) with median, min and max of the windows in us per call, written to --out.  A route "wins" only beyond the sum of both
spreads (max - min).
   python scripts/mb_long_many.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--out profiles/long_many_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402
from tfra_amd.dynamic_embedding import table_ops  # noqa: E402

N_CAT, N_HIST, DIMS = 22, 4, (16, 32, 64, 128)
ROUTES = ("a", "b", "c", "s", "g")


def beyond_spreads(a, b):
  """a's median below b's by more than the sum of both spreads"""
  return bool(b["median"] - a["median"] > (a["max"] - a["min"]) + (b["max"] - b["min"]))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  rng = np.random.default_rng(0)
  n_t = N_CAT + N_HIST
  per_table = a.keys // n_t
  resident = np.arange(per_table, dtype=np.int64) * 7919 + 1
  rkeys = torch.from_numpy(resident).cuda()
  members = []   # (table, ids, seg, row_splits, w, n_rows, grad_out)
  for k in range(n_t):
    dim = DIMS[k % len(DIMS)]
    t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(dim), name="mb_lm_%d" % k, dim=dim, init_size=2 * per_table)
    gen = torch.Generator(device="cuda").manual_seed(k)
    for off in range(0, per_table, 1 << 18):
      kk = rkeys[off:off + (1 << 18)]
      t.insert(kk, torch.randn((kk.numel(), dim), generator=gen, device="cuda") * 0.1)
    n_rows, per_row = (8192, 4) if k < N_CAT else (512, 256)
    nnz = n_rows * per_row
    ids = torch.from_numpy(resident[(rng.zipf(1.2, size=nnz) - 1) % per_table]).cuda()
    seg = (torch.arange(nnz, device="cuda") // per_row).to(torch.int64)
    rs = (torch.arange(n_rows + 1, device="cuda") * per_row).to(torch.int64)
    w = torch.from_numpy(rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)).cuda()
    members.append((t, ids, seg, rs, w, n_rows, torch.randn((n_rows, dim), generator=gen, device="cuda")))
  flags = [k >= N_CAT for k in range(n_t)]
  lines = []
  for op in ("forward", "weight_grad"):
    for form in ("tuple", "ragged"):
      if op == "forward":
        req = (lambda m: (m[0], m[1], m[2], m[4], 1, m[5])) if form == "tuple" else (lambda m: (m[0], m[3], m[1], m[4], 1))
        many = many_long = table_ops.find_combine_many if form == "tuple" else table_ops.find_combine_ragged_many
        single = ((lambda m: m[0].find_combine_long(m[1], m[2], m[4], 1, m[5])) if form == "tuple" else
                  (lambda m: m[0].find_combine_ragged_long(m[3], m[1], m[4], 1)))
      else:
        req = (lambda m: (m[0], m[1], m[2], m[4], 1, m[6])) if form == "tuple" else (lambda m: (m[0], m[3], m[1], m[4], 1, m[6]))
        many = table_ops.find_combine_weight_grad_many if form == "tuple" else table_ops.find_combine_ragged_weight_grad_many
        many_long = (table_ops.find_combine_weight_grad_many_long if form == "tuple" else
                     table_ops.find_combine_ragged_weight_grad_many_long)
        single = ((lambda m: m[0].find_combine_weight_grad_long(m[1], m[2], m[4], 1, m[6])) if form == "tuple" else
                  (lambda m: m[0].find_combine_ragged_weight_grad_long(m[3], m[1], m[4], 1, m[6])))
      reqs = [req(m) for m in members]

      def step(route):
        if route == "a":
          return many(reqs)
        if route == "b":
          return many(reqs[:N_CAT]) + [single(m) for m in members[N_CAT:]]
        if route == "c":
          return many_long(reqs, long_rows=flags)
        if route == "s":
          return [single(members[N_CAT])]
        return many_long(reqs[N_CAT:N_CAT + 1], long_rows=True)

      for _ in range(a.warmup):
        r = {f: step(f) for f in ROUTES}
        for x, y, z in zip(r["a"], r["b"], r["c"]):
          assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
        assert torch.equal(r["s"][0].view(torch.int32), r["g"][0].view(torch.int32))
      torch.cuda.synchronize()
      us = {f: [] for f in ROUTES}
      for _ in range(a.windows):
        for f in ROUTES:   # alternating
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          e0.record()
          for _s in range(a.steps):
            step(f)
          e1.record()
          e1.synchronize()
          us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
      out = {"op": op, "form": form, "tables": n_t, "histories": N_HIST, "resident_keys": per_table * n_t, "combiner": "mean",
             "launches": {"a": many(reqs, return_launches=True)[1], "c": many_long(reqs, return_launches=True, long_rows=flags)[1]},
             "steps_per_window": a.steps}
      for f in ROUTES:
        out[f + "_us"] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                          "windows": [round(x, 2) for x in us[f]]}
      for other in ("a", "b"):
        out["c_wins_over_" + other] = beyond_spreads(out["c_us"], out[other + "_us"])
        out["c_loses_to_" + other] = beyond_spreads(out[other + "_us"], out["c_us"])
      out["g_loses_to_s"] = beyond_spreads(out["s_us"], out["g_us"])
      line = json.dumps(out)
      print(line, flush=True)
      lines.append(line)
  for m in members:
    m[0]._table.check_errors()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
