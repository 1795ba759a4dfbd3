"""The combined sparse write-back of a batch whose grad_out is held in float16 / bfloat16, three ways, in ONE process, alternating
(gradients: bfloat16 without a scale, float16 with a loss scale to undo):
  i    grad_out.float() (float16: * scale) + the untyped call          (what such a caller does without the typed calls)
  ii   the typed call on the half matrix, the scale read by the kernels
  iii  the untyped call on a grad_out that is float32 already, for scale
single   tfra_table_apply_planned_combined[_typed]: nnz 131 072 Zipf-1.2 entries, 16 per row (8 192 rows), about 10 % of a batch's
         ids never seen when it first comes, a growing table pre-filled with --keys rows; tables float32 dim 64 and bfloat16 dim
         128; SGD and Adam; combiner mean, no weights.  --plans batches, each with a plan built ahead per route, in turn.
grouped  tfra_multi_apply_planned_combined[_typed]: the 26-table case of scripts/mb_combined_many.py (float32 tables of dims 16 /
         32 / 64 / 128 with --many-keys rows, 8 192 rows x 4 ids per table, plans built ahead); route i up-casts table by table.
Each route has tables (and plans) of its own and sees the same batches; the rows of a batch's ids are compared bit for bit across
the routes after the warm-up.  HIP events around windows of --steps steps, --windows windows per route after --warmup steps; one
JSON line per case: median, min and max of the windows, us per step, host calls included, and whether ii is below i by more than
the sum of both spreads (max - min).
   python scripts/mb_combined_half.py [--keys 2000000] [--steps 40] [--windows 7] [--warmup 5] [--only single|grouped] [--out FILE]"""
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
LABELS = {"i": "i_upcast_plus_untyped_us", "ii": "ii_typed_us", "iii": "iii_untyped_f32_grad_out_us"}
GRADS = (("bfloat16", False), ("float16", True))   # (format, with a scale): loss scaling belongs to float16
LOSS_SCALE = 1024.0


def measure(a, step, check):
  """Warm-up, the check, then the alternating windows -> {route: [us per step, one per window]}."""
  for r in ROUTES:
    for s in range(a.warmup):
      step(r, s)
  torch.cuda.synchronize()
  check()
  us = {r: [] for r in ROUTES}
  for w in range(a.windows):
    for r in ROUTES:   # alternating: every route sees window w's batches on its own tables
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for s in range(a.steps):
        step(r, a.warmup + w * a.steps + s)
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
  out["ii_below_i_us"] = round(gain, 2)
  out["sum_of_spreads_us"] = round(spread("i") + spread("ii"), 2)
  out["ii_clears_the_bar"] = bool(gain > spread("i") + spread("ii"))
  line = json.dumps(out)
  print(line, flush=True)
  return line


def filled(name, opt_for_slots, dt, dim, rkeys, init_size, value):
  var = de.Variable(dim=dim, name=name, value_dtype=dt, initializer=0.0, init_size=init_size,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt_for_slots))
  for off in range(0, rkeys.numel(), 1 << 18):
    k = rkeys[off:off + (1 << 18)]
    var.upsert(k, torch.full((k.numel(), dim), value, dtype=dt, device="cuda"))
  return var


def grads_of(g32_base, gd, scaled, inv_scale):
  """(half matrix, the float32 matrix routes i and ii form from it)."""
  gh = (g32_base * LOSS_SCALE if scaled else g32_base).to(getattr(torch, gd)).contiguous()
  return gh, (gh.to(torch.float32) * inv_scale if scaled else gh.to(torch.float32))


def same_rows(vs, keys):
  views = [v.lookup(keys) for v in vs]
  it = torch.int16 if views[0].element_size() == 2 else torch.int32
  return all(torch.equal(views[0].view(it), x.view(it)) for x in views[1:])


def single(a, lines):
  nnz, per_row = 131072, 16
  n_rows = nnz // per_row
  rng = np.random.default_rng(0)
  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  fresh_base = int(resident[-1]) + 1
  batches = []
  for s in range(a.plans):
    ids = resident[(rng.zipf(1.2, size=nnz) - 1) % a.keys]
    new = rng.random(nnz) < 0.10
    ids[new] = fresh_base + s * nnz + np.arange(int(new.sum()), dtype=np.int64)   # never-seen when the batch first comes, distinct
    batches.append(torch.from_numpy(ids).cuda())
  rkeys = torch.from_numpy(resident).cuda()
  seg = (torch.arange(nnz, device="cuda") // per_row).to(torch.int64)
  inv_scale = torch.full((1,), 1.0 / LOSS_SCALE, dtype=torch.float32, device="cuda")
  comb = device_ops.COMBINERS["mean"]
  adam = de.optimizers.Adam(1e-3)
  for vd, dim in (("float32", 64), ("bfloat16", 128)):
    g32_base = torch.from_numpy((rng.standard_normal((n_rows, dim)) * 0.01).astype(np.float32)).cuda()
    for oname, opt in (("sgd", de.optimizers.SGD(0.01)), ("adam", adam)):
      vs = {r: filled("mb_ch_%s_%s_%s" % (vd, oname, r), opt, getattr(torch, vd), dim, rkeys, 2 * a.keys + a.plans * nnz // 5, 0.01)
            for r in ROUTES}
      ts = {r: v._tables[0] for r, v in vs.items()}
      ds = {r: t._default_value.to(torch.float32) for r, t in ts.items()}
      plans = {r: [table_ops.SparsePlan(vs[r]._primary, dim).build(b) for b in batches] for r in ROUTES}
      p = opt.params(1)
      for gd, scaled in GRADS:
        scale = inv_scale if scaled else None
        gh, g32 = grads_of(g32_base, gd, scaled, inv_scale)

        def step(r, s):
          t, plan = ts[r]._table, plans[r][s % a.plans]
          if r == "i":
            g = gh.to(torch.float32)
            if scale is not None:
              g = g * scale
            t.apply_planned_combined(p, plan, g, seg, None, comb, ds[r])
          elif r == "ii":
            t.apply_planned_combined(p, plan, gh, seg, None, comb, ds[r], grad_scale=scale)
          else:
            t.apply_planned_combined(p, plan, g32, seg, None, comb, ds[r])

        def check():
          assert same_rows([vs[r] for r in ROUTES], batches[0][:4096]), "the routes' rows differ"

        us = measure(a, step, check)
        for r in ROUTES:
          ts[r]._table.check_errors()
        sizes = {r: int(vs[r].size()) for r in ROUTES}
        assert sizes["i"] == sizes["ii"] == sizes["iii"], sizes
        check()
        lines.append(report({"call": "single", "table": vd, "dim": dim, "opt": oname, "grad_out": gd, "scale": scaled, "nnz": nnz,
                             "n_rows": n_rows, "per_row": per_row, "resident_keys": a.keys, "steps_per_window": a.steps,
                             "windows_n": a.windows, "plans_in_turn": a.plans, "table_size_after": sizes["ii"],
                             "rows_bit_identical": True}, us))
      del vs, ts, plans


def grouped(a, lines):
  n_rows, per_row, dims, n_tables = 8192, 4, (16, 32, 64, 128), 26
  nnz = n_rows * per_row
  rng = np.random.default_rng(0)
  resident = np.arange(a.many_keys, dtype=np.int64) * 7919 + 1
  rkeys = torch.from_numpy(resident).cuda()
  seg = (torch.arange(nnz, device="cuda") // per_row).to(torch.int64)
  inv_scale = torch.full((1,), 1.0 / LOSS_SCALE, dtype=torch.float32, device="cuda")
  comb = device_ops.COMBINERS["mean"]
  adam = de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)
  ids, base = [], []
  tabs, plans = {r: [] for r in ROUTES}, {r: [] for r in ROUTES}
  for j in range(n_tables):
    dim = dims[j % 4]
    ids.append(torch.from_numpy(resident[(rng.zipf(1.2, size=nnz) - 1) % a.many_keys]).cuda())
    g = torch.Generator(device="cuda").manual_seed(j)
    base.append(torch.randn((n_rows, dim), generator=g, device="cuda") * 0.01)
    for r in ROUTES:
      var = filled("mb_chm_%s_%d" % (r, j), adam, torch.float32, dim, rkeys, 2 * a.many_keys, 0.01 * (j + 1))
      tabs[r].append(var)
      plans[r].append(table_ops.SparsePlan(var._primary, dim).build(ids[j]))
  n_step = [0]
  for oname, opt in (("adam", adam), ("sgd", de.optimizers.SGD(0.1))):
    for gd, scaled in GRADS:
      scale = inv_scale if scaled else None
      pairs = [grads_of(b, gd, scaled, inv_scale) for b in base]
      launches = {}

      def step(r, s):
        p = opt.params(n_step[0] + s + 1)
        ts = [v._tables[0] for v in tabs[r]]
        if r == "i":
          gs = [(gh.to(torch.float32) * scale if scale is not None else gh.to(torch.float32)) for gh, _ in pairs]
        elif r == "ii":
          gs = [gh for gh, _ in pairs]
        else:
          gs = [g32 for _, g32 in pairs]
        reqs = [(t._table, plans[r][j], gs[j], seg, None, comb, t._default_value) for j, t in enumerate(ts)]
        launches[r] = table_ops.apply_planned_combined_many(reqs, p, grad_scale=scale if r == "ii" else None)

      def check():
        for j in range(n_tables):
          assert same_rows([tabs[r][j] for r in ROUTES], ids[j][:4096]), "the routes' rows differ (table %d)" % j

      us = measure(a, step, check)
      n_step[0] += a.warmup + a.windows * a.steps
      for r in ROUTES:
        for v in tabs[r]:
          v._tables[0]._table.check_errors()
      check()
      lines.append(report({"call": "grouped", "tables": n_tables, "dims": list(dims), "table": "float32", "opt": oname, "grad_out": gd,
                           "scale": scaled, "n_rows": n_rows, "per_row": per_row, "nnz_per_table": nnz,
                           "resident_keys_per_table": a.many_keys, "steps_per_window": a.steps, "windows_n": a.windows,
                           "kernel_launches_per_call": launches, "torch_launches_in_front_of_i": n_tables * (2 if scaled else 1),
                           "rows_bit_identical": True}, us))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--many-keys", type=int, default=200_000)
  ap.add_argument("--plans", type=int, default=8)
  ap.add_argument("--steps", type=int, default=40)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--only", choices=["single", "grouped"], default=None)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_combined_half: no GPU visible; this is a measurement, it has no CPU form")
  lines = []
  if a.only != "grouped":
    single(a, lines)
  if a.only != "single":
    grouped(a, lines)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
