"""The device builder of a field-wise embedding's pooling lists against the torch route it replaces, in ONE process on one MI355X
(the protocol of §4.29: HIP events around windows of --steps calls after --warmup calls, the forms' windows
alternating, the median of --windows windows and [min - max]).  Shapes: batch 4096 x 64 ids and 8192 x 26 ids, nslots 26, slot =
id mod 26, Zipf-1.2 ids over --universe resident keys, dim 64 float32:
  lists    (a) device_ops._field_entries_torch — clamp, bias, a stable device-wide sort, a gather, searchsorted;
           (b) device_ops.field_entries — tfra_field_entries, one launch.
  forward  the whole FieldWiseEmbedding forward (slot_map_fn, the lists, the ragged pooled lookup, the reshape):
           (a) with device_ops.field_entries replaced by _field_entries_torch; (b) as it is.
One JSON line per point to --out, and the table of DESIGN §4.30 on stdout.
   python scripts/mb_field_entries.py [--universe 2000000] [--steps 20] [--windows 5] [--warmup 5]
                                      [--out profiles/field_entries_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

SHAPES = ((4096, 64), (8192, 26))
NSLOTS, DIM = 26, 64


def window(f, n):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  for _ in range(n):
    f()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) * 1000.0 / n


def stats(us):
  return {"median": round(float(np.median(us)), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}


def key_of(i):
  return i * 2654435761 + 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--universe", type=int, default=2000000)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_entries_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_field_entries: no GPU visible; this is a measurement, it has no CPU form")
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops

  rng = np.random.default_rng(7)
  slot_of = lambda ids: ids % NSLOTS
  table = []
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  fh = open(a.out, "w")

  def report(point, shape, us, extra):
    out = {"what": "field_entries", "point": point, "batch": shape[0], "per_sample": shape[1], "nslots": NSLOTS, "zipf": 1.2,
           "universe": a.universe, "steps": a.steps, "windows": a.windows, "warmup": a.warmup, "order": "the forms' windows alternate"}
    out.update(extra)
    for n in us:
      out[n + "_us"] = stats(us[n])
      out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
    out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
    out["sum_of_spreads_us"] = round(out["a_spread_us"] + out["b_spread_us"], 1)
    out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["sum_of_spreads_us"]
    print(json.dumps(out), flush=True)
    fh.write(json.dumps(out) + "\n")
    fh.flush()
    fmt = lambda s: "%.1f [%.1f - %.1f]" % (s["median"], s["min"], s["max"])
    table.append("| %s | %d x %d | %s | %s | %.1f / %.1f: %s |" % (point, shape[0], shape[1], fmt(out["a_us"]), fmt(out["b_us"]),
                                                                  out["a_minus_b_us"], out["sum_of_spreads_us"],
                                                                  "yes" if out["b_below_a_by_more_than_both_spreads"] else "no"))

  def measure(run):
    us = {n: [] for n in run}
    for f in run.values():
      for _ in range(a.warmup):
        f()
    for _ in range(a.windows):
      for n, f in run.items():
        us[n].append(window(f, a.steps))
    return us

  layer = de.layers.FieldWiseEmbedding(DIM, NSLOTS, slot_map_fn=slot_of, initializer=0.0, name="mb_field_entries",
                                       init_capacity=2 * a.universe)
  for lo in range(0, a.universe, 1 << 18):
    k = key_of(torch.arange(lo, min(lo + (1 << 18), a.universe), dtype=torch.int64, device="cuda"))
    layer.params.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous())
  builder = device_ops.field_entries

  def forward(ids, build):
    device_ops.field_entries = build
    try:
      return layer(ids)
    finally:
      device_ops.field_entries = builder

  for shape in SHAPES:
    ids = torch.from_numpy(key_of((rng.zipf(1.2, size=shape).astype(np.int64) - 1) % a.universe)).cuda()
    slots = slot_of(ids)
    got, want = builder(ids, slots, NSLOTS, want_pos=True), device_ops._field_entries_torch(ids, slots, NSLOTS, want_pos=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want)), "the builder's lists differ from the torch route's"
    assert torch.equal(forward(ids, builder), forward(ids, device_ops._field_entries_torch))
    us = measure({"a": lambda: device_ops._field_entries_torch(ids, slots, NSLOTS), "b": lambda: builder(ids, slots, NSLOTS)})
    report("lists", shape, us, {"a": "_field_entries_torch", "b": "field_entries (tfra_field_entries, one launch)"})
    us = measure({"a": lambda: forward(ids, device_ops._field_entries_torch), "b": lambda: forward(ids, builder)})
    report("forward", shape, us, {"dim": DIM, "dtype": "float32", "a": "FieldWiseEmbedding forward over _field_entries_torch",
                                  "b": "FieldWiseEmbedding forward as it is"})
  fh.close()
  print("| point | batch x ids | (a), us | (b), us | (a) - (b) / sum of spreads: beyond it |")
  print("|---|---|---|---|---|")
  print("\n".join(table))


if __name__ == "__main__":
  main()
