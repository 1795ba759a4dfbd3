"""The weight gradient of the pooled lookups for a grad_out held in float16 / bfloat16, three ways, in ONE process on one MI355X,
alternating (gradients: bfloat16 without a scale, float16 with a loss scale to undo):
  a  grad_out.float() (float16: * scale) + the untyped call             (the route before the typed calls)
  b  the typed call on the half matrix, the scale read by the kernel
  c  the untyped call on a grad_out that is float32 already, for scale
single   tfra_table_find_combine_backprop_weights[_typed]: nnz 131 072 Zipf-1.2 ids, 16 per row (8 192 rows), on --keys resident
         keys, combiner mean, random weights in [0.1, 2); float32 rows at dim 64 and float16 rows at dim 128; and one tier case
         (tfra_tier_find_combine_backprop_weights[_typed], float32 dim 64: an upper LRU table of --slots slots at max_capacity over
         a lower table of --lower keys, 10 % of the entries drawn from keys the upper table was never given).
grouped  tfra_multi_find_combine[_ragged]_backprop_weights[_typed]: 26 float32 owners of dims 16 / 32 / 64 / 128 with --many-keys
         keys, 8 192 rows x 4 ids each, in the tuple and the ragged form; route a up-casts owner by owner.
All routes are reads and share their tables; the results of a and b are compared bit for bit before the windows.  HIP events around
windows of --steps calls, --windows windows per route (alternating a, b, c, a, ...) after --warmup calls; one JSON line per case:
median, min and max of the windows in us per call, host calls included, b against a and b against c, each beside the sum of both
spreads (max - min).
   python scripts/mb_wgrad_half.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--only single|tier|grouped] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

ROUTES = ("a", "b", "c")
LABELS = {"a": "a_upcast_plus_untyped_us", "b": "b_typed_us", "c": "c_untyped_f32_grad_out_us"}
GRADS = (("bfloat16", False), ("float16", True))   # (format, with a scale): loss scaling belongs to float16
LOSS_SCALE = 1024.0
CHUNK = 1 << 18


def key_of(i):
  return i * 2654435761 + 1


def measure(a, run):
  for r in ROUTES:
    for _ in range(a.warmup):
      run[r]()
  torch.cuda.synchronize()
  it = torch.int32
  assert torch.equal(torch.cat([x.reshape(-1) for x in _flat(run["a"]())]).view(it),
                     torch.cat([x.reshape(-1) for x in _flat(run["b"]())]).view(it)), "routes a and b differ"
  us = {r: [] for r in ROUTES}
  for _ in range(a.windows):
    for r in ROUTES:
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize()
      e0.record()
      for _ in range(a.steps):
        run[r]()
      e1.record()
      e1.synchronize()
      us[r].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
  return us


def _flat(x):
  return x if isinstance(x, (list, tuple)) else [x]


def report(out, us):
  for r in ROUTES:
    out[LABELS[r]] = {"median": round(float(np.median(us[r])), 2), "min": round(min(us[r]), 2), "max": round(max(us[r]), 2),
                      "windows": [round(x, 2) for x in us[r]]}
  spread = lambda r: max(us[r]) - min(us[r])
  med = lambda r: float(np.median(us[r]))
  out["b_below_a_us"] = round(med("a") - med("b"), 2)
  out["a_b_sum_of_spreads_us"] = round(spread("a") + spread("b"), 2)
  out["b_below_a_beyond_both_spreads"] = bool(med("a") - med("b") > spread("a") + spread("b"))
  out["b_above_c_us"] = round(med("b") - med("c"), 2)
  out["b_c_sum_of_spreads_us"] = round(spread("b") + spread("c"), 2)
  out["b_above_c_beyond_both_spreads"] = bool(med("b") - med("c") > spread("b") + spread("c"))
  line = json.dumps(out)
  print(line, flush=True)
  return line


def grads_of(base32, fmt, scaled):
  gh = (base32 * LOSS_SCALE if scaled else base32).to(getattr(torch, fmt)).contiguous()
  return gh


def fill(t, n, dim, dt, reverse_from=None):
  for s in range(0, n, CHUNK):
    i = torch.arange(s, min(s + CHUNK, n), dtype=torch.int64, device="cuda")
    k = key_of(i if reverse_from is None else reverse_from - 1 - i)
    t.upsert(k, ((k % 1000).to(torch.float32) * 1e-3)[:, None].expand(-1, dim).to(dt).contiguous(), unique_keys=True)
  t.check_errors()


def routes_single(owner, ids, seg, w, gh, scale, default_row):
  g32 = gh.to(torch.float32) * scale if scale is not None else gh.to(torch.float32)

  def a():
    g = gh.to(torch.float32)
    if scale is not None:
      g = g * scale
    return owner.find_combine_weight_grad(ids, seg, w, 1, g, default_row)

  return {"a": a, "b": lambda: owner.find_combine_weight_grad_typed(ids, seg, w, 1, gh, default_row, grad_scale=scale),
          "c": lambda: owner.find_combine_weight_grad(ids, seg, w, 1, g32, default_row)}


def single(a, lines, tier_case):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
  nnz, per_row = 131072, 16
  n_rows = nnz // per_row
  rng = np.random.default_rng(0)
  gen = torch.Generator(device="cuda").manual_seed(0)
  seg = torch.arange(nnz, dtype=torch.int64, device="cuda") // per_row
  w = torch.rand(nnz, generator=gen, device="cuda") * 1.9 + 0.1
  inv_scale = torch.full((1,), 1.0 / LOSS_SCALE, dtype=torch.float32, device="cuda")
  cases = []
  if not tier_case:
    for vd, dim in (("float32", 64), ("float16", 128)):
      dt = getattr(torch, vd)
      t = _DeviceTable(torch.int64, dt, torch.zeros(dim, dtype=dt), "mb_wgh_%s" % vd, "cuda:0", dim=dim, init_capacity=2 * a.keys)
      fill(t, a.keys, dim, dt)
      ids = key_of(torch.from_numpy((rng.zipf(1.2, size=nnz).astype(np.int64) - 1) % a.keys).cuda())
      cases.append(("table", vd, dim, t, ids, torch.zeros(dim, dtype=dt, device="cuda"), {"resident_keys": a.keys}))
  else:
    dim = 64
    up = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_wgh_up", "cuda:0", dim=dim, init_capacity=a.slots,
                      max_capacity=a.slots, strategy=0)
    lo = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_wgh_lo", "cuda:0", dim=dim, init_capacity=2 * a.lower)
    n_up = a.slots + a.slots // 4
    fill(lo, a.lower, dim, torch.float32)
    fill(up, n_up, dim, torch.float32, reverse_from=n_up)
    tier = _DeviceTier(up, lo, nnz)
    rank = rng.zipf(1.2, size=nnz).astype(np.int64) - 1
    cold = rng.random(nnz) < 0.10
    ids = key_of(torch.from_numpy(np.where(cold, n_up + rank % (a.lower - n_up), rank % (a.slots // 2))).cuda())
    d = torch.zeros(dim, device="cuda")
    where = tier.find(ids, d, return_where=True)[1]
    cases.append(("tier", "float32", dim, tier, ids, d, {"upper_slots": a.slots, "lower_keys": a.lower, "cold_pct": 10,
                                                         "below_pct": round(100.0 * float((where == 2).sum()) / nnz, 2)}))
  for kind, vd, dim, owner, ids, d, extra in cases:
    base = torch.randn((n_rows, dim), generator=gen, device="cuda") * 0.01
    for fmt, scaled in GRADS:
      scale = inv_scale if scaled else None
      us = measure(a, routes_single(owner, ids, seg, w, grads_of(base, fmt, scaled), scale, d))
      out = {"call": "single", "owner": kind, "table": vd, "dim": dim, "grad_out": fmt, "scale": scaled, "nnz": nnz, "n_rows": n_rows,
             "per_row": per_row, "combiner": "mean", "steps_per_window": a.steps, "windows_n": a.windows, "a_equals_b_bitwise": True}
      out.update(extra)
      lines.append(report(out, us))


def grouped(a, lines):
  from tfra_amd.dynamic_embedding import table_ops
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  n_rows, per_row, dims, n_owners = 8192, 4, (16, 32, 64, 128), 26
  nnz = n_rows * per_row
  rng = np.random.default_rng(1)
  gen = torch.Generator(device="cuda").manual_seed(1)
  seg = torch.arange(nnz, dtype=torch.int64, device="cuda") // per_row
  splits = torch.arange(0, nnz + 1, per_row, dtype=torch.int64, device="cuda")
  inv_scale = torch.full((1,), 1.0 / LOSS_SCALE, dtype=torch.float32, device="cuda")
  owners, ids, ws, base = [], [], [], []
  for j in range(n_owners):
    dim = dims[j % 4]
    t = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "mb_wghm_%d" % j, "cuda:0", dim=dim, init_capacity=2 * a.many_keys)
    fill(t, a.many_keys, dim, torch.float32)
    owners.append(t)
    ids.append(key_of(torch.from_numpy((rng.zipf(1.2, size=nnz).astype(np.int64) - 1) % a.many_keys).cuda()))
    ws.append(torch.rand(nnz, generator=gen, device="cuda") * 1.9 + 0.1)
    base.append(torch.randn((n_rows, dim), generator=gen, device="cuda") * 0.01)
  for form in ("tuple", "ragged"):
    many = table_ops.find_combine_weight_grad_many if form == "tuple" else table_ops.find_combine_ragged_weight_grad_many

    def reqs_of(gs):
      if form == "tuple":
        return [(t, ids[j], seg, ws[j], 1, gs[j]) for j, t in enumerate(owners)]
      return [(t, splits, ids[j], ws[j], 1, gs[j]) for j, t in enumerate(owners)]

    for fmt, scaled in GRADS:
      scale = inv_scale if scaled else None
      ghs = [grads_of(b, fmt, scaled) for b in base]
      g32s = [(g.to(torch.float32) * scale if scale is not None else g.to(torch.float32)) for g in ghs]
      launches = {}

      def ra():
        gs = [(g.to(torch.float32) * scale if scale is not None else g.to(torch.float32)) for g in ghs]
        out, launches["a"] = many(reqs_of(gs), return_launches=True)
        return out

      def rb():
        out, launches["b"] = many(reqs_of(ghs), return_launches=True, grad_scale=scale)
        return out

      def rc():
        out, launches["c"] = many(reqs_of(g32s), return_launches=True)
        return out

      us = measure(a, {"a": ra, "b": rb, "c": rc})
      lines.append(report({"call": "grouped", "form": form, "owners": n_owners, "dims": list(dims), "table": "float32", "grad_out": fmt,
                           "scale": scaled, "n_rows": n_rows, "per_row": per_row, "nnz_per_owner": nnz,
                           "resident_keys_per_owner": a.many_keys, "combiner": "mean", "steps_per_window": a.steps,
                           "windows_n": a.windows, "kernel_launches_per_call": launches,
                           "torch_launches_in_front_of_a": n_owners * (2 if scaled else 1), "a_equals_b_bitwise": True}, us))
  for t in owners:
    t.check_errors()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--many-keys", type=int, default=200_000)
  ap.add_argument("--slots", type=int, default=2097150)
  ap.add_argument("--lower", type=int, default=8388608)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--only", choices=["single", "tier", "grouped"], default=None)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_wgrad_half: no GPU visible; this is a measurement, it has no CPU form")
  lines = []
  if a.only in (None, "single"):
    single(a, lines, False)
  if a.only in (None, "tier"):
    single(a, lines, True)
  if a.only in (None, "grouped"):
    grouped(a, lines)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
