"""A lookup whose reader wants another type than the call writes, three ways, in ONE process, alternating:
  i    the untyped call + .to(dtype)        (the route without the typed lookups: a conversion launch behind every lookup)
  ii   the typed call (out_dtype=)          (the conversion in the lookup's kernel)
  iii  the untyped call alone, for scale
find     _DeviceTable.find, B = 131 072 Zipf-1.2 keys over --keys resident rows: float32 rows dim 64 -> bfloat16, float32 rows dim
         128 -> float16, float16 rows dim 128 -> float32.
pooled   _DeviceTable.find_combine, nnz 131 072, 16 per row, float32 dim 64 -> bfloat16.
grouped  table_ops.find_combine_many / find_combine_ragged_many: 26 float32 tables of dims 16 / 32 / 64 / 128 with --many-keys
         rows, 8 192 rows x 4 ids per table -> bfloat16; route i converts table by table (26 launches behind the call).
The three routes read the same table(s); the results of i and ii are compared bit for bit after the warm-up.  HIP events around
windows of --steps steps, --windows windows per route after --warmup steps; one JSON line per case: median, min and max of the
windows, us per step, host calls included, whether ii is below i by more than the sum of both spreads (max - min), and whether ii
is above iii by more than the sum of theirs.
   python scripts/mb_typed_lookup.py [--keys 2000000] [--many-keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402
from tfra_amd.dynamic_embedding import device_ops, table_ops  # noqa: E402

ROUTES = ("i", "ii", "iii")
LABELS = {"i": "i_untyped_plus_to_us", "ii": "ii_typed_us", "iii": "iii_untyped_alone_us"}


def measure(a, step, check):
  """Warm-up, the check, then the alternating windows -> {route: [us per step, one per window]}."""
  for r in ROUTES:
    for s in range(a.warmup):
      step(r)
  torch.cuda.synchronize()
  check()
  us = {r: [] for r in ROUTES}
  for w in range(a.windows):
    for r in ROUTES:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for s in range(a.steps):
        step(r)
      e1.record()
      e1.synchronize()
      us[r].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
  return us


def report(out, us):
  for r in ROUTES:
    out[LABELS[r]] = {"median": round(float(np.median(us[r])), 2), "min": round(min(us[r]), 2), "max": round(max(us[r]), 2),
                      "windows": [round(x, 2) for x in us[r]]}
  spread = lambda r: max(us[r]) - min(us[r])
  gain = float(np.median(us["i"]) - np.median(us["ii"]))
  over = float(np.median(us["ii"]) - np.median(us["iii"]))
  out["ii_below_i_us"] = round(gain, 2)
  out["sum_of_spreads_i_ii_us"] = round(spread("i") + spread("ii"), 2)
  out["ii_clears_the_bar"] = bool(gain > spread("i") + spread("ii"))
  out["ii_above_iii_us"] = round(over, 2)
  out["ii_slower_than_untyped_alone"] = bool(over > spread("ii") + spread("iii"))
  line = json.dumps(out)
  print(line, flush=True)
  return line


def filled(name, dt, dim, rkeys):
  t = table_ops._DeviceTable(torch.int64, dt, torch.zeros(dim, dtype=dt), name, "cuda", dim=dim, init_capacity=2 * rkeys.numel())
  g = torch.Generator(device="cuda").manual_seed(dim)
  for off in range(0, rkeys.numel(), 1 << 18):
    k = rkeys[off:off + (1 << 18)]
    t.upsert(k, torch.randn((k.numel(), dim), generator=g, device="cuda").to(dt))
  return t


def same_bits(x, y):
  return x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def zipf_ids(rng, n, resident):
  return torch.from_numpy(resident[(rng.zipf(1.2, size=n) - 1) % resident.size]).cuda()


def single(a, lines):
  B = 131072
  rng = np.random.default_rng(0)
  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  rkeys = torch.from_numpy(resident).cuda()
  ids = zipf_ids(rng, B, resident)
  seg = (torch.arange(B, device="cuda") // 16).to(torch.int64)
  tabs = {}
  for case, vd, dim, od in (("find", "float32", 64, "bfloat16"), ("find", "float32", 128, "float16"), ("find", "float16", 128, "float32"),
                            ("pooled", "float32", 64, "bfloat16")):
    if (vd, dim) not in tabs:
      tabs[(vd, dim)] = filled("mb_tl_%s_%d" % (vd, dim), getattr(torch, vd), dim, rkeys)
    t, d = tabs[(vd, dim)], getattr(torch, od)
    if case == "find":
      untyped = lambda: t.find(ids)
      typed = lambda: t.find(ids, out_dtype=d)
    else:
      untyped = lambda: t.find_combine(ids, seg, None, device_ops.COMBINERS["mean"], B // 16)
      typed = lambda: t.find_combine_typed(ids, seg, None, device_ops.COMBINERS["mean"], B // 16, out_dtype=d)
    step = lambda r: untyped().to(d) if r == "i" else typed() if r == "ii" else untyped()

    def check():
      assert same_bits(untyped().to(d), typed()), (case, vd, dim, od)

    out = {"case": case, "value_dtype": vd, "dim": dim, "out_dtype": od, "n": B, "resident_keys": a.keys, "steps": a.steps,
           "windows": a.windows}
    lines.append(report(out, measure(a, step, check)))


def grouped(a, lines):
  dims = [16, 32, 64, 128]
  n_rows, per_row = 8192, 4
  rng = np.random.default_rng(1)
  resident = np.arange(a.many_keys, dtype=np.int64) * 7919 + 1
  rkeys = torch.from_numpy(resident).cuda()
  tabs = [filled("mb_tl_many_%d" % i, torch.float32, dims[i % 4], rkeys) for i in range(26)]
  idl = [zipf_ids(rng, n_rows * per_row, resident) for _ in range(26)]
  seg = (torch.arange(n_rows * per_row, device="cuda") // per_row).to(torch.int64)
  rs = (torch.arange(n_rows + 1, device="cuda") * per_row).to(torch.int64)
  comb = device_ops.COMBINERS["mean"]
  d = torch.bfloat16
  for form in ("tuple", "ragged"):
    if form == "tuple":
      reqs = [(t, ids, seg, None, comb, n_rows) for t, ids in zip(tabs, idl)]
      call = table_ops.find_combine_many
    else:
      reqs = [(t, rs, ids, None, comb) for t, ids in zip(tabs, idl)]
      call = table_ops.find_combine_ragged_many
    step = lambda r: [o.to(d) for o in call(reqs)] if r == "i" else call(reqs, out_dtype=d) if r == "ii" else call(reqs)

    def check():
      for x, y in zip(call(reqs), call(reqs, out_dtype=d)):
        assert same_bits(x.to(d), y), form

    _, launches = call(reqs, return_launches=True, out_dtype=d)
    out = {"case": "grouped_" + form, "tables": 26, "dims": dims, "rows_per_table": n_rows, "ids_per_row": per_row, "out_dtype": "bfloat16",
           "resident_keys_per_table": a.many_keys, "launches_typed": launches, "steps": a.steps, "windows": a.windows}
    lines.append(report(out, measure(a, step, check)))


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--keys", type=int, default=2_000_000)
  p.add_argument("--many-keys", type=int, default=2_000_000)
  p.add_argument("--steps", type=int, default=40)
  p.add_argument("--windows", type=int, default=7)
  p.add_argument("--warmup", type=int, default=5)
  p.add_argument("--only", choices=("single", "grouped"), default=None)
  p.add_argument("--out", default=None)
  a = p.parse_args()
  lines = []
  if a.only in (None, "single"):
    single(a, lines)
  if a.only in (None, "grouped"):
    grouped(a, lines)
  if a.out:
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
