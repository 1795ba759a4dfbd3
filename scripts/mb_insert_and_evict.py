"""What capture costs: tfra_table_insert_and_evict against tfra_table_insert_or_assign on the same route, in ONE process: one bounded LRU
float32 dim-64 table of --slots slots at max_capacity, filled past its capacity so that every bucket is full; batches of B = 131 072
unique keys of which 0 %, 50 % or 100 % have never been seen (every step has never-seen keys of its own; the rest are a hot set that
every step rewrites).  Per mix:
  (a) tfra_table_insert_or_assign, TFRA_FLAG_UNIQUE_KEYS, owner tags off: insert_unique_kernel + insert_evict_kernel<G, false>
  (b) tfra_table_insert_and_evict into preallocated buffers (cap = B), its counter zeroed in front of every call (timed):
      insert_unique_kernel + insert_evict_kernel<G, true>
HIP events around windows of --steps calls, --windows windows per form (alternating) after --warmup calls; one JSON line per mix: median,
min and max of the windows in us per call for both forms, (b) - (a), the entries (b) reported per call, the bytes they add (one row
read + one row, key and score write = 2 * 256 + 16 B each) and the time those bytes take at the byte rate (a) itself achieves on its
own algorithmic bytes (per key: 8 B key + 256 B caller's row + 256 B table row; per never-seen key also the key and score lines of
both home buckets, 512 B).  --forms a: only (a), for a library that lacks the new call (--lib: the parent commit's build).
   python scripts/mb_insert_and_evict.py [--slots 8388608] [--steps 20] [--windows 5] [--warmup 5] [--forms ab] [--lib PATH]
                                         [--tag this-tree] [--out profiles/insert_and_evict_mb.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))

DIM, ROW, B = 64, 256, 131072
MIXES = (0, 50, 100)
CHUNK = 1 << 21
ENTRY_BYTES = 2 * ROW + 16


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--slots", type=int, default=8 << 20)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--forms", default="ab")
  ap.add_argument("--lib", default=None)
  ap.add_argument("--tag", default="this tree")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_insert_and_evict: no GPU visible; this is a measurement, it has no CPU form")
  from tfra_amd import _capi
  if a.lib:
    _capi.LIB_PATH = os.path.abspath(a.lib)
  if "b" not in a.forms:
    _capi._SIGS.pop("tfra_table_insert_and_evict", None)   # a library from before the call
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream

  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(DIM), init_capacity=a.slots, max_capacity=a.slots, device="cuda:0", dim=DIM,
                      evict_strategy=de.HkvEvictStrategy.LRU, name="mb_ie")
  tbl = t._table
  dev = tbl.device
  slots = tbl.capacity() - 2
  fill = int(slots * 1.3)
  for lo in range(0, fill, CHUNK):
    k = torch.arange(lo, min(lo + CHUNK, fill), dtype=torch.int64, device="cuda") * 2654435761 + 1
    tbl.upsert(k, (k % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous(), unique_keys=True)
  tbl.check_errors()
  resident = tbl.size_host()
  tbl.set_owner_tags(False)
  vals = torch.randn(B, DIM, device="cuda")
  hot = torch.arange(B, dtype=torch.int64, device="cuda") * 40503 + (1 << 50)
  counter = torch.zeros(1, dtype=torch.int64, device="cuda")
  ek = torch.empty(B, dtype=torch.int64, device="cuda")
  ev = torch.empty((B, DIM), dtype=torch.float32, device="cuda")
  es = torch.empty(B, dtype=torch.int64, device="cuda")
  serial = [0]

  def batches(pct, steps):
    """`steps` batches: pct % never-seen keys (their own every time), the rest the head of the hot set; shuffled"""
    out, n_new = [], B * pct // 100
    for _ in range(steps):
      new = (torch.arange(n_new, dtype=torch.int64, device="cuda") + serial[0]) * 6700417 + (1 << 40)
      serial[0] += n_new
      k = torch.cat([new, hot[:B - n_new]])
      out.append(k[torch.randperm(B, device="cuda")].contiguous())
    return out

  def form_a(k):
    _capi.call("tfra_table_insert_or_assign", tbl._h, B, _ptr(k), _ptr(vals), None, _capi.FLAG_UNIQUE_KEYS, _stream(dev))

  def form_b(k):
    counter.zero_()
    _capi.call("tfra_table_insert_and_evict", tbl._h, B, _ptr(k), _ptr(vals), None, 0, _ptr(counter), B, _ptr(ek), _ptr(ev), _ptr(es),
               _stream(dev))

  forms = [(n, f) for n, f in (("a", form_a), ("b", form_b)) if n in a.forms]

  def window(f, ks):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in ks:
      f(k)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / len(ks)

  def stats(us):
    return {"median": round(float(np.median(us)), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}

  lines = []
  for pct in MIXES:
    form_a(hot)       # the hot set is resident and young
    for _, f in forms:
      for k in batches(pct, a.warmup):
        f(k)
    us = {n: [] for n, _ in forms}
    reported = 0
    for _ in range(a.windows):
      for n, f in forms:
        us[n].append(window(f, batches(pct, a.steps)))
        if n == "b":
          reported = int(counter.item())
    tbl.check_errors()
    n_new = B * pct // 100
    out = {"tag": a.tag, "never_seen_pct": pct, "slots": slots, "resident": resident, "batch": B, "steps_per_window": a.steps}
    for n, _ in forms:
      out[n + "_us"] = stats(us[n])
    if "a" in us:
      a_bytes = B * (8 + 2 * ROW) + n_new * 512
      out["a_algorithmic_bytes"] = a_bytes
      out["a_spread_us"] = round(out["a_us"]["max"] - out["a_us"]["min"], 1)
      out["a_bytes_per_us"] = round(a_bytes / out["a_us"]["median"], 0)
    if "a" in us and "b" in us:
      extra = reported * ENTRY_BYTES
      out.update({"reported_per_call": reported, "b_extra_bytes": extra, "b_minus_a_us": round(out["b_us"]["median"] - out["a_us"]["median"], 1),
                  "extra_bytes_at_a_rate_us": round(extra / (a_bytes / out["a_us"]["median"]), 1)})
    line = json.dumps(out)
    print(line, flush=True)
    lines.append(line)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
