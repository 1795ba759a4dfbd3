"""What the read side of a tier costs: tfra_table_find_missed against the route through existing entry points, tfra_table_assign
against insert_or_assign of the same resident keys, tfra_table_contains against find, in ONE process on one MI355X.

Shape: float32 dim 64, a growing table holding 2 M keys (load 0.5), batches of B = 131 072 unique keys of which 0, 10, 50 or 100 % are
not resident.  Per mix:
  (a) today's route: tfra_table_find with exists, torch.nonzero of the misses (the host reads their count), keys[idx]
  (b) tfra_table_find_missed with nothing read on the host (find_missed(sync=False)): the counter zeroed, then rows, exists, the miss
      list and its count on the device
  (c) plain tfra_table_find, for scale
  (d) tfra_table_find_missed next to (c): rows and the count alone, on a counter that is not zeroed — what the kernel adds to find's
then, on a batch of resident keys: tfra_table_assign against tfra_table_insert_or_assign(TFRA_FLAG_UNIQUE_KEYS), and
tfra_table_contains against tfra_table_find with exists.  The C entry points are called on buffers allocated once, as
scripts/mb_find_or_insert.py does; the route (a) allocates what torch.nonzero and the gather return, as it has to.

HIP events around windows of --steps calls, --windows windows per form (alternating) after --warmup calls; one JSON line per
comparison: median, min and max of the windows in us per call and the spreads.  --tiles records which TIER_TILES (csrc/tfra_tier.hip)
the measured library was built with (--lib PATH: another build, e.g. one made with TFRA_EXTRA_FLAGS=-DTFRA_TIER_TILES=8).
   python scripts/mb_find_missed.py [--resident 2097152] [--steps 20] [--windows 5] [--warmup 5] [--lib PATH] [--tiles 4]
                                    [--tag this-tree] [--out profiles/find_missed_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, B = 64, 131072
MIXES = (0, 10, 50, 100)
CHUNK = 1 << 20


def window(f, steps):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  for _ in range(steps):
    f()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) * 1000.0 / steps


def stats(us):
  return {"median": round(float(np.median(us)), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}


def measure(a, forms):
  """{name: stats} of the forms, their windows alternating"""
  for f in forms.values():
    window(f, a.warmup)
  us = {n: [] for n in forms}
  for _ in range(a.windows):
    for n, f in forms.items():
      us[n].append(window(f, a.steps))
  out = {}
  for n in forms:
    out[n + "_us"] = stats(us[n])
    out[n + "_spread_us"] = round(out[n + "_us"]["max"] - out[n + "_us"]["min"], 1)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--resident", type=int, default=1 << 21)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--lib", default=None)
  ap.add_argument("--tiles", type=int, default=4)
  ap.add_argument("--tag", default="this tree")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_find_missed: no GPU visible; this is a measurement, it has no CPU form")
  from tfra_amd import _capi
  if a.lib:
    _capi.LIB_PATH = os.path.abspath(a.lib)
  import tfra_amd.dynamic_embedding as de
  tbl = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(DIM), device="cuda:0", dim=DIM, init_size=8192, name="mb_fm")._table
  tbl.reserve(2 * a.resident)
  for lo in range(0, a.resident, CHUNK):
    k = torch.arange(lo, min(lo + CHUNK, a.resident), dtype=torch.int64, device="cuda") * 2654435761 + 1
    tbl.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous(), unique_keys=True)
  tbl.check_errors()
  g = torch.Generator(device="cuda").manual_seed(1)
  hot = torch.randperm(a.resident, device="cuda", generator=g)[:B].to(torch.int64) * 2654435761 + 1
  absent = torch.arange(B, dtype=torch.int64, device="cuda") * 6700417 + (1 << 50)
  base = {"tag": a.tag, "tiles_per_block": a.tiles, "batch": B, "dim": DIM, "resident": tbl.size_host(), "slots": tbl.capacity() - 2,
          "steps_per_window": a.steps}
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  dev = tbl.device
  dflt = torch.zeros(DIM, device="cuda")
  rows = torch.empty(B, DIM, device="cuda")
  ex = torch.empty(B, dtype=torch.bool, device="cuda")
  counter = torch.zeros(1, dtype=torch.int64, device="cuda")
  running = torch.zeros(1, dtype=torch.int64, device="cuda")
  mk = torch.empty(B, dtype=torch.int64, device="cuda")
  mi = torch.empty(B, dtype=torch.int32, device="cuda")
  lines = []
  for pct in MIXES:
    n_abs = B * pct // 100
    keys = torch.cat([absent[:n_abs], hot[:B - n_abs]])[torch.randperm(B, device="cuda", generator=g)].contiguous()

    def form_a():
      _capi.call("tfra_table_find", tbl._h, B, _ptr(keys), _ptr(rows), _ptr(ex), _ptr(dflt), 0, _stream(dev))
      idx = torch.nonzero(~ex).reshape(-1)
      return keys[idx], idx

    def form_b():
      counter.zero_()
      _capi.call("tfra_table_find_missed", tbl._h, B, None, _ptr(keys), _ptr(rows), _ptr(ex), None, _ptr(dflt), 0, _ptr(counter), B,
                 _ptr(mk), _ptr(mi), _stream(dev))

    def form_c():
      _capi.call("tfra_table_find", tbl._h, B, _ptr(keys), _ptr(rows), None, _ptr(dflt), 0, _stream(dev))

    def form_d():     # (b) without the memset launch: count only on a counter that runs on, the launch next to (c)'s
      _capi.call("tfra_table_find_missed", tbl._h, B, None, _ptr(keys), _ptr(rows), None, None, _ptr(dflt), 0, _ptr(running), 0,
                 None, None, _stream(dev))

    form_b()
    assert int(counter.item()) == n_abs == form_a()[1].numel()
    out = dict(base, what="find_missed", missing_pct=pct, a="find(return_exists) + nonzero + keys[idx]", b="find_missed(sync=False)", c="find")
    out["d"] = "find_missed, count only, no exists, the counter not zeroed"
    out.update(measure(a, {"a": form_a, "b": form_b, "c": form_c, "d": form_d}))
    out["d_minus_c_us"] = round(out["d_us"]["median"] - out["c_us"]["median"], 1)
    out["b_minus_c_us"] = round(out["b_us"]["median"] - out["c_us"]["median"], 1)
    out["b_within_c_spread"] = out["b_minus_c_us"] <= out["c_spread_us"]
    out["a_minus_b_us"] = round(out["a_us"]["median"] - out["b_us"]["median"], 1)
    out["b_below_a_by_more_than_both_spreads"] = out["a_minus_b_us"] > out["a_spread_us"] + out["b_spread_us"]
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
  vals = torch.randn(B, DIM, device="cuda")
  out = dict(base, what="assign", a="upsert(unique_keys=True) of resident keys", b="assign")
  out.update(measure(a, {
      "a": lambda: _capi.call("tfra_table_insert_or_assign", tbl._h, B, _ptr(hot), _ptr(vals), None, _capi.FLAG_UNIQUE_KEYS, _stream(dev)),
      "b": lambda: _capi.call("tfra_table_assign", tbl._h, B, None, _ptr(hot), _ptr(vals), None, None, _stream(dev))}))
  out["b_minus_a_us"] = round(out["b_us"]["median"] - out["a_us"]["median"], 1)
  lines.append(json.dumps(out))
  print(lines[-1], flush=True)
  out = dict(base, what="contains", a="find", b="contains")
  out.update(measure(a, {
      "a": lambda: _capi.call("tfra_table_find", tbl._h, B, _ptr(hot), _ptr(rows), _ptr(ex), _ptr(dflt), 0, _stream(dev)),
      "b": lambda: _capi.call("tfra_table_contains", tbl._h, B, None, _ptr(hot), _ptr(ex), _stream(dev))}))
  out["b_minus_a_us"] = round(out["b_us"]["median"] - out["a_us"]["median"], 1)
  lines.append(json.dumps(out))
  print(lines[-1], flush=True)
  tbl.check_errors()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
