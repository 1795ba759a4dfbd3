"""The ragged pooled lookup against the tuple form, in ONE process, the two forms alternating on the same batches (--batches
distinct batches per table, taken in turn).  A batch is 8 192 rows x 16 Zipf-1.2 ids with ~2 % of the rows emptied; weights
uniform in (0.1, 2) with ~10 % not > 0.
  1  one growing float32 table, dim 64, --keys (2 M) resident rows; weights, default_id set, combiner mean:
       A  de.safe_embedding_lookup_sparse (tuple form: boolean-mask pruning, pooled lookup, a lookup of default_id, torch.where)
       B  de.ragged_embedding_ops.safe_embedding_lookup_sparse (one launch)
  2  the same batches with no weights and no default_id — what the memset and the bounds launch cost:
       A  Variable.lookup_combined          B  Variable.lookup_combined_ragged
  3  --tables (26) growing float32 tables, dims cycling 16 / 32 / 64 / 128, --many-keys (200 000) rows each, (1)'s weights:
       A  de.safe_embedding_lookup_sparse_many    B  de.ragged_embedding_ops.safe_embedding_lookup_sparse_many
HIP events around windows of --steps steps, --windows windows per form after --warmup steps during which the two results are
compared bit for bit; one JSON line per shape (median, min and max of the windows, us per step, host work included; B counts as
faster only if its median lies below A's by more than A's own min-max spread), written to --out.
   python scripts/mb_ragged_lookup.py [--keys 2000000] [--tables 26] [--steps 20] [--windows 5] [--warmup 5] [--out profiles/ragged_lookup_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

reo = de.ragged_embedding_ops
N_ROWS, PER_ROW = 8192, 16
DIMS = (16, 32, 64, 128)
DEFAULT_ID = 7919 + 1   # resident


def make_batch(rng, resident):
  """(row_splits, row ids, ids, weights) on the device."""
  counts = np.full(N_ROWS, PER_ROW)
  counts[rng.random(N_ROWS) < 0.02] = 0
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  nnz = int(rs[-1])
  seg = np.repeat(np.arange(N_ROWS, dtype=np.int64), counts)
  ids = resident[(rng.zipf(1.2, size=nnz) - 1) % resident.size]
  w = rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)
  w[rng.random(nnz) < 0.10] *= -1.0
  return tuple(torch.from_numpy(x).cuda() for x in (rs, seg, ids, w))


def filled(name, dim, resident):
  var = de.Variable(dim=dim, name=name, initializer=0.0, init_size=2 * resident.size)
  rkeys = torch.from_numpy(resident).cuda()
  g = torch.Generator(device="cuda").manual_seed(dim)
  for off in range(0, resident.size, 1 << 18):
    k = rkeys[off:off + (1 << 18)]
    var.upsert(k, torch.randn((k.numel(), dim), generator=g, device="cuda"))
  return var


def measure(a, label, extra, step):
  """step(form, s) -> list of results.  Warm-up compares A and B bit for bit; then windows, alternating."""
  for s in range(a.warmup):
    for x, y in zip(step("A", s), step("B", s)):
      assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: A and B differ" % label
  torch.cuda.synchronize()
  us = {f: [] for f in "AB"}
  for wi in range(a.windows):
    for f in "AB":   # alternating: both forms see window wi's batches
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for s in range(a.steps):
        step(f, a.warmup + wi * a.steps + s)
      e1.record()
      e1.synchronize()
      us[f].append(e0.elapsed_time(e1) * 1000.0 / a.steps)
  out = dict(point=label, n_rows=N_ROWS, per_row=PER_ROW, dtype="float32", steps_per_window=a.steps, **extra)
  for f, name in (("A", "A_tuple_form_us"), ("B", "B_ragged_us")):
    out[name] = {"median": round(float(np.median(us[f])), 2), "min": round(min(us[f]), 2), "max": round(max(us[f]), 2),
                 "windows": [round(x, 2) for x in us[f]]}
  A, B = out["A_tuple_form_us"], out["B_ragged_us"]
  out["A_spread_us"] = round(A["max"] - A["min"], 2)
  out["B_below_A_by_more_than_A_spread"] = bool(A["median"] - B["median"] > A["max"] - A["min"])
  out["B_above_A_by_more_than_A_spread"] = bool(B["median"] - A["median"] > A["max"] - A["min"])
  line = json.dumps(out)
  print(line, flush=True)
  return line


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--keys", type=int, default=2_000_000)
  ap.add_argument("--tables", type=int, default=26)
  ap.add_argument("--many-keys", type=int, default=200_000)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--batches", type=int, default=8)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_ragged_lookup: no GPU visible; this is a measurement, it has no CPU form")
  rng = np.random.default_rng(0)
  lines = []

  resident = np.arange(a.keys, dtype=np.int64) * 7919 + 1
  var = filled("mb_ragged_one", 64, resident)
  bs = [make_batch(rng, resident) for _ in range(a.batches)]

  def safe_one(f, s):
    rs, seg, ids, w = bs[s % a.batches]
    if f == "A":
      return [de.safe_embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", default_id=DEFAULT_ID, num_rows=N_ROWS)]
    return [reo.safe_embedding_lookup_sparse(var, (rs, ids), w, combiner="mean", default_id=DEFAULT_ID)]

  def plain_one(f, s):
    rs, seg, ids, w = bs[s % a.batches]
    if f == "A":
      return [var.lookup_combined(ids, seg, None, "mean", N_ROWS)]
    return [var.lookup_combined_ragged(rs, ids, None, "mean")]

  one = dict(tables=1, dims=[64], resident_keys_per_table=a.keys)
  lines.append(measure(a, "1 safe: weights, default_id, mean", dict(one, A="de.safe_embedding_lookup_sparse",
                                                                    B="ragged_embedding_ops.safe_embedding_lookup_sparse"), safe_one))
  lines.append(measure(a, "2 plain: no weights, no default_id, mean", dict(one, A="Variable.lookup_combined",
                                                                          B="Variable.lookup_combined_ragged"), plain_one))
  var._tables[0]._table.check_errors()

  resident = np.arange(a.many_keys, dtype=np.int64) * 7919 + 1
  variables = [filled("mb_ragged_many_%d" % j, DIMS[j % 4], resident) for j in range(a.tables)]
  mbs = [[make_batch(rng, resident) for _ in range(a.batches)] for _ in range(a.tables)]

  def safe_many(f, s):
    b = [mbs[j][s % a.batches] for j in range(a.tables)]
    if f == "A":
      return de.safe_embedding_lookup_sparse_many(variables, [(x[1], x[2]) for x in b], [x[3] for x in b], combiner="mean",
                                                  default_id=DEFAULT_ID, num_rows=N_ROWS)
    return reo.safe_embedding_lookup_sparse_many(variables, [(x[0], x[2]) for x in b], [x[3] for x in b], combiner="mean",
                                                 default_id=DEFAULT_ID)

  lines.append(measure(a, "3 safe, %d tables" % a.tables,
                       dict(tables=a.tables, dims=list(DIMS), resident_keys_per_table=a.many_keys,
                            A="de.safe_embedding_lookup_sparse_many", B="ragged_embedding_ops.safe_embedding_lookup_sparse_many"),
                       safe_many))
  for v in variables:
    v._tables[0]._table.check_errors()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
