"""The device builder of the safe lookups' entry lists against the torch preprocessing it replaces, in ONE process on one MI355X
(the protocol of §4.17: HIP events around windows of --steps calls after --warmup calls, the forms' windows
alternating, the median of --windows windows and [min - max]):
  lists   lists of 8 192 rows x 4 Zipf-1.2 ids, 10 % of the rows without entries, 10 % of the weights <= 0, default_id given;
          1, 3, 8 and 26 of them:
          (a) a loop of variable._safe_sparse_args_torch — boolean masks, nonzero, cat, a stable sort: the parent commit's code;
          (b) ONE device_ops.safe_entries_many (tfra_multi_safe_entries and the one read of all counts).
  step    the whole training step of --tables variables (Adam): safe_embedding_lookup_sparse_many(return_trainable=True) and
          apply_combined_gradients_many: (a) with variable._safe_sparse_args_many replaced by the loop of _safe_sparse_args_torch —
          before; (b) as it is — after.  Each form on variables of its own, filled alike.
One JSON line per point to --out, and the table of DESIGN §4.29 on stdout.
   python scripts/mb_safe_entries.py [--tables 26] [--universe 65536] [--steps 20] [--windows 5] [--warmup 5]
                                     [--out profiles/safe_entries_mb.jsonl]"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIMS = (16, 32, 64, 128)
LISTS = (1, 3, 8, 26)
N_ROWS, PER_ROW, DEFAULT_ID = 8192, 4, 1


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
  ap.add_argument("--tables", type=int, default=26)
  ap.add_argument("--universe", type=int, default=65536)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "safe_entries_mb.jsonl"))
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_safe_entries: no GPU visible; this is a measurement, it has no CPU form")
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops, variable

  rng = np.random.default_rng(7)
  cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

  def one_list():
    per = np.where(rng.random(N_ROWS) < 0.1, 0, PER_ROW)
    rows = np.repeat(np.arange(N_ROWS, dtype=np.int64), per)
    ids = key_of((rng.zipf(1.2, size=rows.size).astype(np.int64) - 1) % a.universe)
    w = rng.uniform(0.1, 2.0, size=rows.size).astype(np.float32)
    w[rng.random(rows.size) < 0.1] = np.float32(-0.5)
    return cuda(rows), cuda(ids), cuda(w)

  batches = [one_list() for _ in range(max(max(LISTS), a.tables))]
  table = []
  os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
  fh = open(a.out, "w")

  def report(point, n_lists, us, extra):
    out = {"what": "safe_entries", "point": point, "lists": n_lists, "zipf": 1.2, "n_rows": N_ROWS, "per_row": PER_ROW, "steps": a.steps,
           "windows": a.windows, "warmup": a.warmup, "order": "the forms' windows alternate"}
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
    table.append("| %s | %d | %s | %s | %.1f / %.1f: %s |" % (point, n_lists, fmt(out["a_us"]), fmt(out["b_us"]), out["a_minus_b_us"],
                                                             out["sum_of_spreads_us"],
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

  # ---- lists: the torch preprocessing against the builder ----------------------------------------------------------------------------
  params = types.SimpleNamespace(_primary=torch.device("cuda", torch.cuda.current_device()), dim=64)

  def torch_loop(bs):
    return [variable._safe_sparse_args_torch(params, (rows, ids), w, "mean", DEFAULT_ID, True, N_ROWS) for rows, ids, w in bs]

  def builder(bs):
    return device_ops.safe_entries_many([(rows, ids, w, N_ROWS, True, DEFAULT_ID, False) for rows, ids, w in bs])

  for n_list in LISTS:
    bs = batches[:n_list]
    _, launches = device_ops.safe_entries_many([(rows, ids, w, N_ROWS, True, DEFAULT_ID, False) for rows, ids, w in bs], return_launches=True)
    us = measure({"a": lambda: torch_loop(bs), "b": lambda: builder(bs)})
    report("lists", n_list, us, {"a": "loop of _safe_sparse_args_torch", "b": "safe_entries_many with its counts read",
                                 "b_launches": launches, "b_host_reads": 1, "a_host_reads": 4 * n_list})

  # ---- step: the whole grouped training step, before and after -----------------------------------------------------------------------
  opt = de.optimizers.Adam(0.01)

  def make(name, dim):
    v = de.Variable(dim=dim, name=name, initializer=0.0, init_size=4 * a.universe, devices=["cuda:0"],
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    k = key_of(torch.arange(a.universe, dtype=torch.int64, device="cuda"))
    v.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, dim).contiguous())
    return v

  def many_torch(params_list, sp_ids_list, weights, combiners, default_ids, return_trainable, num, ragged=False):
    return [variable._safe_sparse_args_torch(p, sp_ids_list[i], weights[i], combiners[i], default_ids[i], return_trainable, num[i])
            for i, p in enumerate(params_list)]

  grouped = variable._safe_sparse_args_many
  bs = batches[:a.tables]
  sp, ws = [(rows, ids) for rows, ids, _ in bs], [w for _, _, w in bs]
  sets = {f: [make("mb_se_%s_%d" % (f, j), DIMS[j % 4]) for j in range(a.tables)] for f in "ab"}
  deos = {f: de.DynamicEmbeddingOptimizer(opt) for f in "ab"}
  grads = [torch.randn((N_ROWS, DIMS[j % 4]), device="cuda") * 0.01 for j in range(a.tables)]

  def step(f, args_many):
    variable._safe_sparse_args_many = args_many
    try:
      res = de.safe_embedding_lookup_sparse_many(sets[f], sp, ws, combiner="mean", default_id=DEFAULT_ID, return_trainable=True,
                                                 num_rows=[N_ROWS] * a.tables)
    finally:
      variable._safe_sparse_args_many = grouped
    deos[f].apply_combined_gradients_many([(g, tw) for g, (_, tw) in zip(grads, res)])

  us = measure({"a": lambda: step("a", many_torch), "b": lambda: step("b", grouped)})
  report("step", a.tables, us, {"dims": list(DIMS), "dtype": "float32", "optimizer": "Adam",
                                "a": "_safe_sparse_args_many = loop of _safe_sparse_args_torch (before)", "b": "as it is (after)"})
  fh.close()
  print("| point | lists | (a), us | (b), us | (a) - (b) / sum of spreads: beyond it |")
  print("|---|---|---|---|---|")
  print("\n".join(table))


if __name__ == "__main__":
  main()
