"""Score-filtered export / count / erase / save against the code of the parent commit, in ONE process: one bounded CUSTOMIZED float32
dim-64 table of --slots (64 M) slots at 50 % fill; the scores are 0..99 by key, so a threshold picks the match rate (1 %, 10 %, 100 %).
Per match rate the pairs (the second member is the baseline):
  (a) export_if                 | export_all(with_scores=True), then a torch mask of keys, rows and scores on the device
  (b) count_if                  | the same full export, then the mask's sum
  (c) erase_if                  | full export + mask + erase(keys)         (the erased keys are put back, untimed, between calls: this
                                                                            pair is timed call by call and the window is the sum)
  (d) save_if                   | save, on a table of --save-slots (4 M) slots; file I/O dominates, bytes written are recorded
HIP events around windows of --steps calls, --windows windows per form after --warmup calls; one JSON line per (pair, match rate): median,
min and max of the windows in us per call, whether the new form's median lies below the baseline's by more than the baseline's own
min-max spread, and the algorithmic bytes of the new form (256 B per bucket scanned + (8 + 8 + row) B per match) against 8 TB/s.
   python scripts/mb_score_filter.py [--slots 67108864] [--save-slots 4194304] [--steps 20] [--windows 5] [--warmup 5]
                                     [--out profiles/score_filter_mb.jsonl]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "recommenders-addons_amd"))
import tfra_amd.dynamic_embedding as de  # noqa: E402

DIM = 64
ROW = DIM * 4
RATES = ((1, 99), (10, 90), (100, 0))     # (% of the keys that match "ge", threshold): scores are key % 100
CHUNK = 1 << 22


def make_table(slots, name):
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(DIM), init_capacity=slots, max_capacity=slots, device="cuda:0", dim=DIM,
                      evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, name=name)
  tbl = t._table
  n = (tbl.capacity() - 2) // 2
  for a in range(0, n, CHUNK):
    k = torch.arange(a, min(a + CHUNK, n), dtype=torch.int64, device="cuda") * 2654435761 + 1
    put(tbl, k)
  tbl.check_errors()
  assert tbl.size_host() == n, "the fill evicted"
  return tbl, n


def put(tbl, k):
  for a in range(0, k.numel(), CHUNK):
    kk = k[a:a + CHUNK]
    v = (kk % 1000).to(torch.float32)[:, None].expand(-1, DIM).contiguous()
    tbl.upsert(kk, v, scores=kk % 100, unique_keys=True)


def window(fn, steps):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(steps):
    fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) * 1000.0 / steps


def window_with_undo(fn, undo, steps):
  """per-call events, the undo between them untimed"""
  total = 0.0
  for _ in range(steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    got = fn()
    e1.record()
    e1.synchronize()
    total += e0.elapsed_time(e1) * 1000.0
    undo(got)
    torch.cuda.synchronize()
  return total / steps


def stats(us):
  return {"median": round(float(np.median(us)), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}


def pair(a, label, pct, new, base, undo=None, extra=None):
  run = (lambda f: window(f, a.steps)) if undo is None else (lambda f: window_with_undo(f, undo, a.steps))
  for f in (new, base):
    if undo is None:
      for _ in range(a.warmup):
        f()
    else:
      window_with_undo(f, undo, a.warmup)
  torch.cuda.synchronize()
  us = {"new": [], "base": []}
  for _ in range(a.windows):     # alternating
    us["new"].append(run(new))
    us["base"].append(run(base))
  n, b = stats(us["new"]), stats(us["base"])
  out = {"pair": label, "match_pct": pct, "steps_per_window": a.steps, "new_us": n, "baseline_us": b,
         "baseline_spread_us": round(b["max"] - b["min"], 1),
         "new_below_baseline_by_more_than_its_spread": bool(b["median"] - n["median"] > b["max"] - b["min"])}
  out.update(extra or {})
  return out


def roofline(nb, matches, rows):
  byts = 256 * nb + matches * (16 + (ROW if rows else 0))
  return {"algorithmic_bytes": int(byts), "us_at_8TBps": round(byts / 8e12 * 1e6, 1)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--slots", type=int, default=64 << 20)
  ap.add_argument("--save-slots", type=int, default=4 << 20)
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("mb_score_filter: no GPU visible; this is a measurement, it has no CPU form")
  lines = []

  def emit(out):
    line = json.dumps(out)
    print(line, flush=True)
    lines.append(line)

  tbl, n = make_table(a.slots, "mb_sf")
  nb = (tbl.capacity() - 2) // 15

  def full_mask(thr):
    k, v, s = tbl.export_all(with_scores=True)
    m = s >= thr
    return k, v, s, m

  for pct, thr in RATES:
    matches = int(tbl.count_if(thr, "ge").item())
    k, v, s, m = full_mask(thr)
    assert int(m.sum().item()) == matches and torch.equal(torch.sort(tbl.export_if(thr, "ge")[0])[0], torch.sort(k[m])[0])
    del k, v, s, m
    info = {"slots": a.slots, "resident": n, "matches": matches}

    def base_export():
      k, v, s, m = full_mask(thr)
      return k[m], v[m], s[m]

    emit(pair(a, "a export_if | export_all + mask", pct, lambda: tbl.export_if(thr, "ge"), base_export,
              extra=dict(info, **roofline(2 * nb, matches, True))))     # two passes: the count, then the export
    emit(pair(a, "b count_if | export_all + mask.sum", pct, lambda: tbl.count_if(thr, "ge"), lambda: full_mask(thr)[3].sum(),
              extra=dict(info, **roofline(nb, 0, False))))

    gone = tbl.export_if(thr, "ge")[0]

    def base_erase():
      k, v, s, m = full_mask(thr)
      tbl.erase(k[m])

    emit(pair(a, "c erase_if | export_all + mask + erase", pct, lambda: tbl.erase_if(thr, "ge"), base_erase, undo=lambda _: put(tbl, gone),
              extra=dict(info, **roofline(nb, matches, False))))
    assert tbl.size_host() == n
    del gone
  del tbl
  torch.cuda.empty_cache()

  tbl, n = make_table(a.save_slots, "mb_sf_save")
  nb = (tbl.capacity() - 2) // 15
  with tempfile.TemporaryDirectory() as d:
    for pct, thr in RATES:
      matches = int(tbl.count_if(thr, "ge").item())
      pn, pb = os.path.join(d, "new%d" % pct), os.path.join(d, "base%d" % pct)
      out = pair(a, "d save_if | save", pct, lambda: tbl.save_if(pn, thr, "ge"), lambda: tbl.save(pb),
                 extra=dict({"slots": a.save_slots, "resident": n, "matches": matches}, **roofline(nb, matches, True)))
      out["new_bytes_written"] = os.path.getsize(pn + "-keys") + os.path.getsize(pn + "-values")
      out["baseline_bytes_written"] = os.path.getsize(pb + "-keys") + os.path.getsize(pb + "-values")
      emit(out)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
