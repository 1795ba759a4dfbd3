"""GPU: stream ordering on every table and tier entry point — the threading contract of include/tfra_mi355x.h: a call on
stream B sees what the previous call on the same table queued on stream A, with no synchronisation by the caller (each entry
point locks the table and runs Table::enter, which makes the new stream wait for an event on the last one; the grouped calls
through lock_and_enter / lock_tiers_and_tables, the tier calls through tier_enter).

One case = two (or more) calls on one table.  All inputs, and every SparsePlan (caller data, like a tensor), exist before a
device-wide synchronise; then stream A gets `torch.cuda._sleep(SLEEP_CYCLES)` and the first call, stream B the second call.
What is expected comes from the same calls issued one after the other on ONE stream, without the sleep, on a freshly built
identical table (the twin).  Every output of every call and the final table — export sorted by key, every co-located field,
the scores where the test wrote them — are compared bit for bit.

The control (fixture `streams`): the streams of a case are a pair on which a plain torch operation DOES overtake the sleep, so
a missing wait shows every time.  If no such pair exists the machine serialises its streams and the cases skip.

A delayed call that reads on the host — load, export, export_if, size / check_errors / slot_census, save — has finished when it
returns, so its case cannot fail on ordering (with the wait of Table::enter taken out of a scratch build these cases passed,
every other one failed); they are here because their outputs and end states are still pinned to the twin's.

Which residents an LRU table evicts depends on device clocks (tests/test_gpu_tier_driver.py), so the tier cases compare what
does not: the row of every key through `tier.find`, the whole row of every key wherever it lives, and of `stats()` the
counters `calls` and `not_resident`.  EXCLUDED from the comparison: `missed`, `lower_hits` and `demoted` — they count keys by
the tier that held them, which follows the victims — and the `where` bytes beyond "found or not".

Entry points of the header that take a table or tier and a stream and are NOT driven here, on purpose:
  * tfra_table_step_overlap, tfra_table_step_overlap_flush, tfra_table_steps_overlap, tfra_multi_step_prefetch and the route
    calls (tfra_route_*, tfra_assign_route_*): the overlap and route drivers own their streams (a step driver / route object
    holds them), the caller's stream only brackets them; tests/test_gpu_overlap.py and tests/test_gpu_int32_surface.py order
    those.
  * anything under TFRA_OPTION_CAPTURE_SAFE: that mode skips the chaining on purpose (a captured graph orders by its edges).
  * tfra_table_save / tfra_table_load: the Python layer binds the field forms only (field 0 is the same file and frame)."""
import os

import numpy as np
import pytest

from tests.test_gpu_int32_surface import SLEEP_CYCLES

pytestmark = pytest.mark.gpu

N, DIM, SEEN, ROWS = 512, 8, 384, 64        # keys, row width, keys resident at the start, rows of a pooled lookup
CHOSEN = {}                                  # what the control chose (printed once, for the record)


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _overtakes(torch, a, b):
  """A plain torch operation on `b` runs before one queued earlier on `a` behind a sleep."""
  x = torch.zeros(1024, device="cuda")
  torch.cuda.synchronize()
  with torch.cuda.stream(a):
    torch.cuda._sleep(SLEEP_CYCLES)
    x.fill_(1)
  with torch.cuda.stream(b):
    y = x.clone()
  torch.cuda.synchronize()
  return bool((y == 0).all())


@pytest.fixture(scope="module")
def streams(env):
  """(A, B, C): pool streams such that work on B and on C overtakes work on A (up to 8 candidates are tried)."""
  torch, _ = env
  cand = [torch.cuda.Stream() for _ in range(8)]
  for ia, a in enumerate(cand):
    free = [ib for ib, b in enumerate(cand) if ib != ia and b.cuda_stream != a.cuda_stream and _overtakes(torch, a, b)]
    if len(free) >= 2:
      CHOSEN.update(a=ia, b=free[0], c=free[1])
      print("\nstream control: A = candidate %d, B = candidate %d, C = candidate %d of 8 overtake" % (ia, free[0], free[1]))
      return a, cand[free[0]], cand[free[1]]
  pytest.skip("no pair of streams overtakes on this machine: its streams are serialised, an ordering check proves nothing")


# ---- inputs: functions of the key, the same in both runs ---------------------------------------------------------------------
def _keys():
  rng = np.random.default_rng(1105)
  k = np.unique(rng.integers(1, 2**40, size=N + 64, dtype=np.int64))
  rng.shuffle(k)
  return k[:N]


KEYS = _keys()
_RNG = np.random.default_rng(1106)
REP = KEYS[_RNG.integers(0, N, size=N)]                      # a batch whose ids repeat
SEG = np.sort(_RNG.integers(0, ROWS, size=N)).astype(np.int64)
SPLITS = np.searchsorted(SEG, np.arange(ROWS + 1)).astype(np.int64)
WEIGHTS = _RNG.uniform(0.25, 2.0, size=N).astype(np.float32)
GRADS = (_RNG.standard_normal((N, DIM)) * 0.125).astype(np.float32)
GRAD_OUT = (_RNG.standard_normal((ROWS, DIM)) * 0.125).astype(np.float32)


def _rows_np(keys, ver):
  return ((keys[:, None] % 997).astype(np.float32) * np.float32(0.25) + np.float32(ver) + np.arange(DIM, dtype=np.float32)[None, :] * np.float32(0.125))


class Ctx:
  """The tables, tiers and inputs of ONE run of a case; `tag` keeps the two runs' table names apart."""

  def __init__(self, env, tag, tmp):
    self.torch, self.de = env
    self.tag, self.tmp = tag, str(tmp)
    self.tables, self.tiers, self.keep = [], [], []
    self.keys = self.T(KEYS)
    self.rep = self.T(REP)
    self.seg, self.splits, self.w = self.T(SEG), self.T(SPLITS), self.T(WEIGHTS)
    self.grads, self.grad_out = self.T(GRADS), self.T(GRAD_OUT)
    self.default = self.torch.full((DIM,), 0.5, device="cuda")

  def T(self, a):
    return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

  def rows(self, keys, ver, dtype=None):
    r = self.T(_rows_np(np.asarray(keys), ver))
    return r if dtype is None else r.to(dtype)

  def scores(self, base):
    return self.T(np.arange(base, base + N, dtype=np.int64))

  def table(self, name, dtype=None, aux=0, scored=False, prefill=True, track=True):
    """A _DeviceTable of 8192 slots (nothing grows, nothing is evicted) holding KEYS[:SEEN] at version 1; scored: CUSTOMIZED,
    key i with score 1000 + i."""
    from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
    torch = self.torch
    dtype = dtype or torch.float32
    kw = dict(init_capacity=8192, max_capacity=8192, strategy=4) if scored else dict(init_capacity=8192)
    dt = _DeviceTable(torch.int64, dtype, torch.full((DIM,), -1.0, dtype=dtype), "so_%s_%s" % (name, self.tag), "cuda:0", dim=DIM,
                      aux_fields=aux, aux_init=(0.5, 0.25, 0.0, 0.0), **kw)
    if prefill:
      dt.upsert(self.keys[:SEEN], self.rows(KEYS[:SEEN], 1, dtype), scores=self.scores(1000)[:SEEN] if scored else None, unique_keys=True)
    if track:
      self.tables.append((dt, scored))
    return dt

  def tier(self, name):
    """A cache of 360 slots (LRU, at max_capacity) over a growing table, filled through the tier with KEYS[:SEEN] in batches of
    64: more keys than the cache holds, so rows were demoted; KEYS[SEEN:] have never been seen."""
    from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
    torch = self.torch
    up = _DeviceTable(torch.int64, torch.float32, torch.full((DIM,), -1.0), "so_up_%s_%s" % (name, self.tag), "cuda:0", dim=DIM,
                      aux_fields=2, init_capacity=360, max_capacity=360, strategy=0, aux_init=(0.5, 0.25, 0.0, 0.0))
    lo = _DeviceTable(torch.int64, torch.float32, torch.full((DIM,), -1.0), "so_lo_%s_%s" % (name, self.tag), "cuda:0", dim=DIM,
                      aux_fields=2, init_capacity=8192, aux_init=(0.5, 0.25, 0.0, 0.0))
    tier = _DeviceTier(up, lo, N)
    for a in range(0, SEEN, 64):
      tier.insert(self.keys[a:a + 64], self.rows(KEYS[a:a + 64], 1))
    assert up.size_host() + lo.size_host() >= SEEN and lo.size_host() > 0
    self.tiers.append((up, lo, tier))
    return up, lo, tier

  def reads(self, dt):
    """The reader of a read-after-write case: find of every key, and of every co-located field."""
    return lambda: [dt.find(self.keys, return_exists=True)] + [dt.find(self.keys, field=f) for f in range(1, dt._aux_fields + 1)]

  # ---- the end state
  def state(self):
    torch = self.torch
    out = []
    for dt, scored in self.tables:
      dt.check_errors()
      if dt.size_host() == 0:
        out.append("empty")
        continue
      k, v, s = dt.export_all(with_scores=scored)
      o = torch.argsort(k)
      out.append([k[o], v[o]] + ([s[o]] if scored else []) + [dt.find(k[o], field=f) for f in range(1, dt._aux_fields + 1)])
    for up, lo, tier in self.tiers:
      up.check_errors()
      lo.check_errors()
      inup = up.contains(self.keys)
      whole = [torch.where(inup[:, None], up.find(self.keys, field=f), lo.find(self.keys, field=f)) for f in range(3)]
      st = tier.stats()
      out.append([tier.find(self.keys), inup | lo.contains(self.keys), whole, st["calls"], st["not_resident"]])
    return out


# ---- playing a case, and comparing two runs --------------------------------------------------------------------------------------
def _play(env, streams, case, tag, tmp):
  """One run of `case`: a function of a Ctx that builds tables and inputs and returns its steps, (stream index, call[, post]).
  streams None: the twin — one stream, no sleep.  Only the FIRST step is delayed.  `post` canonicalises an output whose order
  is unspecified; it runs after the final synchronise, so that no step reads on the host on its behalf."""
  torch = env[0]
  c = Ctx(env, tag, tmp)
  steps = case(c)
  torch.cuda.synchronize()
  outs = []
  for i, step in enumerate(steps):
    si, fn = step[0], step[1]
    if streams is None:
      outs.append(fn())
    else:
      with torch.cuda.stream(streams[si]):
        if i == 0:
          torch.cuda._sleep(SLEEP_CYCLES)
        outs.append(fn())
  torch.cuda.synchronize()
  outs = [step[2](o) if len(step) > 2 else o for step, o in zip(steps, outs)]
  return [outs, c.state()]


def _canon(torch, x):
  if torch.is_tensor(x):
    a = x.detach().contiguous().reshape(-1)
    return ("tensor", str(x.dtype), tuple(x.shape), a.view(torch.uint8).cpu().numpy().tobytes())
  if isinstance(x, (list, tuple)):
    return [_canon(torch, y) for y in x]
  if isinstance(x, dict):
    return [(k, _canon(torch, x[k])) for k in sorted(x)]
  return x


def _first_difference(a, b, path="run"):
  if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
    for i, (x, y) in enumerate(zip(a, b)):
      d = _first_difference(x, y, "%s[%d]" % (path, i))
      if d:
        return d
    return None
  if a == b:
    return None
  if isinstance(a, tuple) and isinstance(b, tuple) and a[:1] == b[:1] == ("tensor",) and a[1:3] == b[1:3]:
    x, y = np.frombuffer(a[3], np.uint8), np.frombuffer(b[3], np.uint8)
    return "%s: %s %s differs in %d of %d bytes (first at byte %d)" % (path, a[1], a[2], int((x != y).sum()), x.size, int(np.argmax(x != y)))
  return "%s: %r vs %r" % (path, a if not isinstance(a, tuple) else a[:3], b if not isinstance(b, tuple) else b[:3])


def _check(env, streams, case, tmp_path):
  """[outputs of step 0, of step 1, ...] and the end state of the delayed two-stream run against the one-stream twin's.  The twin
  runs FIRST: the first launch of a kernel loads its code object, which can synchronise the device — in the delayed run that
  would hold the host until stream A has finished, and the case would pass whatever the library does."""
  torch = env[0]
  want = _canon(torch, _play(env, None, case, "t", tmp_path / "t"))
  got = _canon(torch, _play(env, streams, case, "d", tmp_path / "d"))
  diff = _first_difference(got, want)
  assert diff is None, "delayed two-stream run vs one-stream twin, [0] = outputs per step, [1] = end state: " + diff


def _params(de, kind):
  return (de.optimizers.SGD(0.5) if kind == "sgd" else de.optimizers.Adam(0.05)).params(1)


def _by(torch, key, *rest):
  o = torch.argsort(key)
  return [key[o]] + [r[o] for r in rest]


def _listed(torch, counter, cap, key, *rest):
  """a counted list whose order is unspecified -> [count, the entries sorted by `key`]"""
  n = min(int(counter.reshape(-1)[0].item()), cap)
  return [n] + _by(torch, key[:n], *[r[:n] for r in rest])


def _plan(c, ids, dim=DIM):
  plan = c.de.SparsePlan("cuda:0", dim).build(ids)
  c.keep.append(plan)
  return plan


def _f16(c):
  return c.torch.float16


# ---- 1. read after write: each writer delayed on A, find of the same keys on B ---------------------------------------------------
def _w_upsert(c, dtype=None, unique=False):
  dt = c.table("t", dtype)
  v = c.rows(KEYS, 2, dtype)
  return dt, lambda: dt.upsert(c.keys, v, unique_keys=unique)


def _w_accum(c):
  dt = c.table("t")
  ex = np.arange(N) < SEEN
  ex[::7] ^= True
  ex, d = c.T(ex), c.rows(KEYS, 3)
  return dt, lambda: dt.accum_or_assign(c.keys, d, ex)


def _w_assign(c):
  dt = c.table("t")
  v = c.rows(KEYS, 2)
  return dt, lambda: dt.assign(c.keys, v, return_found=True)


def _w_insert_field(c):
  dt = c.table("t", aux=2)
  v = c.rows(KEYS, 4)
  return dt, lambda: dt.upsert(c.keys, v, field=1)


def _w_find_or_insert(c, dtype=None):
  dt = c.table("t", dtype)
  v = c.rows(KEYS, 2, dtype)
  return dt, lambda: dt.find_or_insert(c.keys, init_values=v, return_exists=True)


def _w_find_or_insert_planned(c, dtype=None):
  dt = c.table("t", dtype)
  plan, v = _plan(c, c.rep), c.rows(REP, 2, dtype)
  return dt, lambda: dt.find_or_insert_planned(plan, init_values=v, return_exists=True)


def _w_store_rows(c, dtype=None):
  dt = c.table("t", dtype, aux=2)
  f0, f1 = c.rows(KEYS, 2), c.rows(KEYS, 5)
  return dt, lambda: dt.store_rows(c.keys, [f0, f1, None])


def _w_remove(c):
  dt = c.table("t")
  gone = c.keys[::2].contiguous()
  return dt, lambda: dt.erase(gone)


def _w_remove_if(c):
  dt = c.table("t", scored=True)
  return dt, lambda: dt.erase_if(1200, "lt")


def _w_clear(c):
  dt = c.table("t")
  return dt, lambda: dt.clear_all()


def _w_load(c):
  dt = c.table("t", aux=1)
  src = c.table("src", prefill=False, track=False)
  src.upsert(c.keys, c.rows(KEYS, 2), unique_keys=True)
  os.makedirs(c.tmp, exist_ok=True)
  prefix = os.path.join(c.tmp, "ckpt")
  src.save(prefix)
  return dt, lambda: [dt.load(prefix), dt.load(prefix, field=1)]


def _w_apply_optimizer(c, kind):
  dt = c.table("t", aux=2)
  p = _params(c.de, kind)
  return dt, lambda: dt.apply_optimizer(p, c.keys, c.grads, c.default)


def _w_apply_sparse(c, kind, half=False, dtype=None):
  dt = c.table("t", dtype, aux=2)
  p, g = _params(c.de, kind), (c.grads.half() if half else c.grads)
  return dt, lambda: dt.apply_sparse(p, c.rep, g, c.default)


def _w_apply_planned(c, half=False, dtype=None):
  dt = c.table("t", dtype, aux=2)
  p, plan, g = _params(c.de, "adam"), _plan(c, c.rep), (c.grads.half() if half else c.grads)
  return dt, lambda: dt.apply_planned(p, plan, g, c.default)


def _w_apply_planned_combined(c, half=False, dtype=None):
  dt = c.table("t", dtype, aux=2)
  p, plan, g = _params(c.de, "adam"), _plan(c, c.rep), (c.grad_out.half() if half else c.grad_out)
  return dt, lambda: dt.apply_planned_combined(p, plan, g, c.seg, c.w, 1, c.default)


def _w_upsert_n(c):
  dt = c.table("t")
  v, count = c.rows(KEYS, 2), c.T(np.array([300], np.int64))
  return dt, lambda: dt.upsert_n(c.keys, count, v)


def _w_upsert_and_evict_n(c):
  dt = c.table("t")
  v, count = c.rows(KEYS, 2), c.T(np.array([300], np.int64))
  return dt, lambda: dt.upsert_and_evict(c.keys, v, count=count, sync=False)[0]      # (a table with room reports nothing)


def _w_upsert_sparse(c):
  dt = c.table("t")
  v = c.rows(REP, 2) + c.T(np.arange(N, dtype=np.float32))[:, None]      # the LAST occurrence of an id wins
  return dt, lambda: dt.upsert_sparse(c.rep, v)


def _w_upsert_planned(c):
  dt = c.table("t")
  plan, v = _plan(c, c.rep, dim=0), c.rows(REP, 2) + c.T(np.arange(N, dtype=np.float32))[:, None]
  return dt, lambda: dt.upsert_planned(plan, v)


def _w_reserve(c):
  dt = c.table("t")
  return dt, lambda: dt.reserve(40000)      # (the one case that rehashes: the find must see the new storage)


def _w_prefetch_assign(c):
  dt = c.table("t")
  ps = c.de.PrefetchAssignStep(dt).prime(c.rep)
  c.keep.append(ps)
  v, nxt = c.rows(REP, 2) + c.T(np.arange(N, dtype=np.float32))[:, None], c.keys.clone()
  return dt, lambda: ps.step(v, nxt)


RAW = {
    "insert_or_assign": _w_upsert,
    "insert_or_assign-unique_keys": lambda c: _w_upsert(c, unique=True),
    "insert_or_assign-f16": lambda c: _w_upsert(c, _f16(c)),
    "accum": _w_accum,
    "assign": _w_assign,
    "insert_field": _w_insert_field,
    "find_or_insert": _w_find_or_insert,
    "find_or_insert-f16": lambda c: _w_find_or_insert(c, _f16(c)),
    "find_or_insert_planned": _w_find_or_insert_planned,
    "find_or_insert_planned-f16": lambda c: _w_find_or_insert_planned(c, _f16(c)),
    "store_rows": _w_store_rows,
    "store_rows-f16": lambda c: _w_store_rows(c, _f16(c)),
    "remove": _w_remove,
    "remove_if": _w_remove_if,
    "clear": _w_clear,
    "load": _w_load,
    "apply_optimizer-sgd": lambda c: _w_apply_optimizer(c, "sgd"),
    "apply_optimizer-adam": lambda c: _w_apply_optimizer(c, "adam"),
    "apply_sparse-sgd": lambda c: _w_apply_sparse(c, "sgd"),
    "apply_sparse-adam": lambda c: _w_apply_sparse(c, "adam"),
    "apply_sparse-adam-f16": lambda c: _w_apply_sparse(c, "adam", dtype=_f16(c)),
    "apply_sparse_typed-sgd": lambda c: _w_apply_sparse(c, "sgd", half=True),
    "apply_sparse_typed-adam": lambda c: _w_apply_sparse(c, "adam", half=True),
    "apply_planned": _w_apply_planned,
    "apply_planned-f16": lambda c: _w_apply_planned(c, dtype=_f16(c)),
    "apply_planned_typed": lambda c: _w_apply_planned(c, half=True),
    "apply_planned_combined": _w_apply_planned_combined,
    "apply_planned_combined-f16": lambda c: _w_apply_planned_combined(c, dtype=_f16(c)),
    "apply_planned_combined_typed": lambda c: _w_apply_planned_combined(c, half=True),
    "insert_or_assign_n": _w_upsert_n,
    "insert_and_evict_n": _w_upsert_and_evict_n,
    "upsert_sparse": _w_upsert_sparse,
    "upsert_planned": _w_upsert_planned,
    "reserve": _w_reserve,
    "step_prefetch_assign": _w_prefetch_assign,
}


@pytest.mark.parametrize("name", sorted(RAW))
def test_read_after_write(env, streams, tmp_path, name):
  def case(c):
    dt, write = RAW[name](c)
    return [(0, write), (1, c.reads(dt))]
  _check(env, streams, case, tmp_path)


def test_read_after_upsert_and_evict_on_a_full_table(env, streams, tmp_path):
  """tfra_table_insert_and_evict on the full bounded table of tests/test_gpu_eviction.py (CUSTOMIZED, distinct scores: the
  victims are determined); the find on B reads the fresh keys and the residents, so it sees who came and who left."""
  from tests.test_gpu_eviction import F_CALL1, Scene, _distinct_scores
  torch = env[0]

  def case(c):
    scn = Scene(env, "so_evict_%s" % c.tag, "CUSTOMIZED", score=_distinct_scores(1))
    c.keep.append(scn)
    c.tables.append((scn.tbl, True))
    fresh = np.concatenate([scn.fresh[i][:f] for i, f in enumerate(F_CALL1)])
    probe = c.T(np.concatenate([fresh] + list(scn.res)))
    k, v, s = c.T(fresh), c.T(scn.rows(fresh, 2)), c.T(np.arange(5000, 5000 + fresh.size, dtype=np.int64))
    return [(0, lambda: scn.tbl.upsert_and_evict(k, v, scores=s, sync=False), lambda o: _listed(torch, o[0], k.numel(), *o[1:])),
            (1, lambda: scn.tbl.find(probe, return_exists=True))]
  _check(env, streams, case, tmp_path)


def test_read_after_grouped_combined_write_back(env, streams, tmp_path):
  """apply_planned_combined_many over three tables (the untyped call, then — one member with a float16 grad_out — the typed one)
  on A; on B every table is read."""
  from tfra_amd.dynamic_embedding.table_ops import apply_planned_combined_many
  for half in (False, True):
    def case(c, half=half):
      tabs = [c.table("m%d" % i, aux=2) for i in range(3)]
      plans = [_plan(c, c.rep) for _ in tabs]
      p = _params(c.de, "adam")
      reqs = [(t, pl, (c.grad_out.half() if half and i == 1 else c.grad_out * (i + 1)), c.seg, c.w, i % 3, c.default)
              for i, (t, pl) in enumerate(zip(tabs, plans))]
      return [(0, lambda: apply_planned_combined_many(reqs, p)), (1, lambda: [c.reads(t)() for t in tabs])]
    _check(env, streams, case, tmp_path / ("typed" if half else "f32"))


def test_read_after_grouped_admission(env, streams, tmp_path):
  """find_or_insert_many, then table_admit_many (the same C call without outputs), over four tables on A; every table read on B."""
  from tfra_amd.dynamic_embedding.table_ops import find_or_insert_many, table_admit_many
  for admit in (False, True):
    def case(c, admit=admit):
      tabs = [c.table("m%d" % i, c.torch.float16 if i == 3 else None) for i in range(4)]
      reqs = [(t, c.keys, c.rows(KEYS, 2 + i, t.value_dtype)) for i, t in enumerate(tabs)]
      call = (lambda: table_admit_many(reqs)) if admit else (lambda: find_or_insert_many(reqs))
      return [(0, call), (1, lambda: [c.reads(t)() for t in tabs])]
    _check(env, streams, case, tmp_path / ("admit" if admit else "rows"))


def test_read_after_a_prefetch_step(env, streams, tmp_path):
  """One PrefetchStep step (tfra_table_step_prefetch: lookup, Adam write-back, the next batch's plan on the driver's side stream)
  with A as its main stream; the table's rows and both slots read on B."""
  torch, de = env

  def case(c):
    opt = de.optimizers.Adam(0.05)
    var = de.Variable(dim=DIM, name="so_prefetch_%s" % c.tag, initializer=0.5, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    var.upsert(c.keys[:SEEN], c.rows(KEYS[:SEEN], 1))
    dt = var.tables[0]._table
    c.tables.append((dt, False))
    ps = de.PrefetchStep(var, de.DynamicEmbeddingOptimizer(opt)).prime(c.rep)
    c.keep += [var, ps]
    nxt = c.keys.clone()
    return [(0, lambda: ps.step(c.grads, nxt)), (1, c.reads(dt))]
  _check(env, streams, case, tmp_path)


# ---- 2. write after read: each reader delayed on A, insert_or_assign of new rows for the same keys on B ----------------------------
def _r_find(c, dt):
  return lambda: dt.find(c.keys, return_exists=True)


def _r_find_typed(c, dt):
  return lambda: dt.find(c.keys, return_exists=True, out_dtype=c.torch.float16)


def _r_find_field(c, dt):
  return lambda: dt.find(c.keys, return_exists=True, field=1)


def _r_find_missed(c, dt):
  torch = c.torch
  scored = any(sc for t, sc in c.tables if t is dt)
  return (lambda: dt.find_missed(c.keys, return_exists=True, return_scores=scored, sync=False),
          lambda o: [o[0]] + _listed(torch, o[1], N, o[3], o[2]) + list(o[4:]))


def _r_contains(c, dt):
  return lambda: dt.contains(c.keys)


def _r_find_unique(c, dt):
  return (lambda: dt.find_unique(c.rep, return_exists=True),
          lambda o: [o[0], o[4], o[3], o[1][o[2].long()]])      # rows, exists, count, unique[idx] (== the ids)


def _r_find_n(c, dt):
  count = c.T(np.array([300], np.int64))
  out = c.torch.zeros((N, DIM), device="cuda")
  return lambda: dt.find_n(c.keys, count, out=out, return_exists=True)


def _r_find_combine(c, dt):
  return lambda: [dt.find_combine(c.rep, c.seg, c.w, cb, ROWS) for cb in (0, 1, 2)]


def _r_find_combine_typed(c, dt):
  return lambda: dt.find_combine_typed(c.rep, c.seg, c.w, 1, ROWS, out_dtype=c.torch.bfloat16)


def _r_find_combine_ragged(c, dt):
  fill = int(KEYS[3])
  return lambda: [dt.find_combine_ragged(c.splits, c.rep, c.w, 1), dt.find_combine_ragged(c.splits, c.rep, c.w, 0, prune=True, fill_id=fill),
                  dt.find_combine_ragged(c.splits, c.rep, None, 2, out_dtype=c.torch.float16)]


def _r_weight_grad(c, dt):
  return lambda: dt.find_combine_weight_grad(c.rep, c.seg, c.w, 1, c.grad_out)


def _r_ragged_weight_grad(c, dt):
  return lambda: dt.find_combine_ragged_weight_grad(c.splits, c.rep, c.w, 2, c.grad_out)


def _r_fetch_planned(c, dt):
  torch = c.torch
  plan = _plan(c, c.rep)

  def post(o):
    keys, fields, gsum, count = o
    return _listed(torch, count, N, keys, *([f for f in fields if f is not None] + [gsum]))
  return (lambda: dt.fetch_planned(plan, grads=c.grads)), post


def _r_export(c, dt):
  torch = c.torch
  return (lambda: dt.export_all(with_scores=True)), (lambda o: _by(torch, *o))


def _r_export_if(c, dt):
  torch = c.torch
  return (lambda: [dt.export_if(1100, "ge"), dt.count_if(1100, "lt")]), (lambda o: [_by(torch, *o[0]), o[1]])


def _r_size(c, dt):
  return lambda: [dt.size_device(), dt.size_host(), dt.slot_census()["live"], dt.check_errors()]


def _r_save(c, dt):
  os.makedirs(c.tmp, exist_ok=True)
  prefix = os.path.join(c.tmp, "saved")

  def post(o):
    k = np.fromfile(prefix + "-keys", np.int64)
    v = np.fromfile(prefix + "-values", np.float32).reshape(-1, DIM)
    order = np.argsort(k)
    return [o[0], o[1], o[2], k[order].tobytes(), v[order].tobytes(), os.path.getsize(prefix + "_delta-keys")]
  return (lambda: [dt.save(prefix), dt.save(prefix + "_f1", field=1), dt.save_if(prefix + "_delta", 1100, "ge")]), post


# name -> (reader, kwargs of the table)
WAR = {
    "find": (_r_find, {}),
    "find-f16": (_r_find, {"f16": True}),
    "find_typed": (_r_find_typed, {}),
    "find_field": (_r_find_field, {"aux": 2}),
    "find_missed": (_r_find_missed, {}),
    "find_missed-scores": (_r_find_missed, {"scored": True}),
    "contains": (_r_contains, {}),
    "find_unique": (_r_find_unique, {}),
    "find_n": (_r_find_n, {}),
    "find_combine": (_r_find_combine, {}),
    "find_combine-f16": (_r_find_combine, {"f16": True}),
    "find_combine_typed": (_r_find_combine_typed, {}),
    "find_combine_ragged": (_r_find_combine_ragged, {}),
    "find_combine_weight_grad": (_r_weight_grad, {}),
    "find_combine_ragged_weight_grad": (_r_ragged_weight_grad, {}),
    "fetch_planned": (_r_fetch_planned, {"aux": 2}),
    "fetch_planned-f16": (_r_fetch_planned, {"aux": 2, "f16": True}),
    "export-scores": (_r_export, {"scored": True}),
    "export_if": (_r_export_if, {"scored": True}),
    "size": (_r_size, {}),
    "save": (_r_save, {"scored": True, "aux": 1}),
}


@pytest.mark.parametrize("name", sorted(WAR))
def test_write_after_read(env, streams, tmp_path, name):
  """The reader must return the rows from BEFORE the write (and the 128 keys the write adds as misses)."""
  reader, kw = WAR[name]

  def case(c):
    dtype = c.torch.float16 if kw.get("f16") else None
    scored = bool(kw.get("scored"))
    dt = c.table("t", dtype, aux=kw.get("aux", 0), scored=scored)
    r = reader(c, dt)
    read, post = r if isinstance(r, tuple) else (r, None)
    new, sc = c.rows(KEYS, 9, dtype), (c.scores(3000) if scored else None)
    write = lambda: dt.upsert(c.keys, new, scores=sc, unique_keys=True)
    return [((0, read, post) if post else (0, read)), (1, write)]
  _check(env, streams, case, tmp_path)


def test_write_after_grouped_reads(env, streams, tmp_path):
  """find_combine_many, find_combine_ragged_many (untyped and typed) and both grouped weight gradients over three tables, each
  delayed on A; on B new rows go into all three tables."""
  from tfra_amd.dynamic_embedding import table_ops as to
  f16 = env[0].float16
  readers = {
      "many": lambda c, ts: to.find_combine_many([(t, c.rep, c.seg, c.w, i % 3, ROWS) for i, t in enumerate(ts)]),
      "many_typed": lambda c, ts: to.find_combine_many([(t, c.rep, c.seg, c.w, i % 3, ROWS) for i, t in enumerate(ts)], out_dtype=f16),
      "ragged_many": lambda c, ts: to.find_combine_ragged_many([(t, c.splits, c.rep, c.w, i % 3) for i, t in enumerate(ts)]),
      "ragged_many_typed": lambda c, ts: to.find_combine_ragged_many([(t, c.splits, c.rep, c.w, i % 3) for i, t in enumerate(ts)], out_dtype=f16),
      "wgrad_many": lambda c, ts: to.find_combine_weight_grad_many([(t, c.rep, c.seg, c.w, i % 3, c.grad_out) for i, t in enumerate(ts)]),
      "ragged_wgrad_many": lambda c, ts: to.find_combine_ragged_weight_grad_many([(t, c.splits, c.rep, c.w, i % 3, c.grad_out)
                                                                                 for i, t in enumerate(ts)]),
  }
  for name, reader in readers.items():
    def case(c, reader=reader):
      tabs = [c.table("m%d" % i, c.torch.float16 if i == 2 else None) for i in range(3)]
      new = [c.rows(KEYS, 9 + i, t.value_dtype) for i, t in enumerate(tabs)]
      return [(0, lambda: reader(c, tabs)), (1, lambda: [t.upsert(c.keys, v, unique_keys=True) for t, v in zip(tabs, new)])]
    _check(env, streams, case, tmp_path / name)


# ---- 3. write after write -----------------------------------------------------------------------------------------------------------
def _ww_apply_then_insert(c):
  dt = c.table("t", aux=2)
  p, v = _params(c.de, "adam"), c.rows(KEYS[:256], 7)
  return [(0, lambda: dt.apply_sparse(p, c.rep, c.grads, c.default)), (1, lambda: dt.upsert(c.keys[:256], v))]


def _ww_insert_then_apply(c):
  dt = c.table("t", aux=2)
  p, v = _params(c.de, "adam"), c.rows(KEYS, 7)
  return [(0, lambda: dt.upsert(c.keys, v)), (1, lambda: dt.apply_sparse(p, c.rep, c.grads, c.default))]


def _ww_find_or_insert_then_assign(c):
  dt = c.table("t")
  init, v = c.rows(KEYS, 2), c.rows(KEYS, 7)
  return [(0, lambda: dt.find_or_insert(c.keys, init_values=init, return_exists=True)), (1, lambda: dt.assign(c.keys, v, return_found=True))]


def _ww_clear_then_insert(c):
  dt = c.table("t")
  v = c.rows(KEYS[:256], 7)
  return [(0, lambda: dt.clear_all()), (1, lambda: dt.upsert(c.keys[:256], v))]


WAW = {"apply_sparse-insert_or_assign": _ww_apply_then_insert, "insert_or_assign-apply_sparse": _ww_insert_then_apply,
       "find_or_insert-assign": _ww_find_or_insert_then_assign, "clear-insert": _ww_clear_then_insert}


@pytest.mark.parametrize("name", sorted(WAW))
def test_write_after_write(env, streams, tmp_path, name):
  _check(env, streams, WAW[name], tmp_path)


# ---- 4. three streams ---------------------------------------------------------------------------------------------------------------
def test_three_streams_chain_through_the_last_one(env, streams, tmp_path):
  """A writes (delayed), B reads and writes, C reads: the table remembers only the LAST stream, and that carries the order from A
  through B to C."""
  def case(c):
    dt = c.table("t", aux=1)
    v2, v3 = c.rows(KEYS, 2), c.rows(KEYS[:256], 3)
    return [(0, lambda: dt.upsert(c.keys, v2)),
            (1, lambda: dt.find(c.keys, return_exists=True)),
            (1, lambda: dt.upsert(c.keys[:256], v3, field=1)),
            (2, lambda: [dt.find(c.keys, return_exists=True), dt.find(c.keys, field=1), dt.size_device()])]
  _check(env, streams, case, tmp_path)


# ---- 5. tiers -----------------------------------------------------------------------------------------------------------------------
def _found(o):
  """(rows, where) -> [rows, found or not]: which tier held a key follows the LRU victims (module docstring)"""
  return [o[0], o[1] != 0]


def _batch():
  """64 keys: 32 that went through the tier, 32 never seen"""
  return np.concatenate([KEYS[100:132], KEYS[SEEN + 10:SEEN + 42]])


def _tier_reads(c, tier):
  return lambda: [tier.find(c.keys), tier.find_combine(c.rep, c.seg, c.w, 1, ROWS), tier.find_combine_ragged(c.splits, c.rep, c.w, 0),
                  tier.find_combine_weight_grad(c.rep, c.seg, c.w, 1, c.grad_out),
                  tier.find_combine_ragged_weight_grad(c.splits, c.rep, c.w, 2, c.grad_out)]


def _t_find_or_insert_then_reads(c):
  _, _, tier = c.tier("t")
  b = _batch()
  kb, init = c.T(b), c.rows(b, 2)
  return [(0, lambda: tier.find_or_insert(kb, init_values=init, return_where=True), _found), (1, _tier_reads(c, tier))]


def _t_find_combine_then_insert(c):
  _, _, tier = c.tier("t")
  b = _batch()
  kb, v = c.T(b), c.rows(b, 7)
  return [(0, _tier_reads(c, tier)), (1, lambda: tier.insert(kb, v))]


def _t_planned_then_apply_on_the_cache(c):
  up, _, tier = c.tier("t")
  b = _batch()
  ids = np.concatenate([b, b[::3]])
  plan, init = _plan(c, c.T(ids)), c.rows(ids, 2)
  p, g = _params(c.de, "adam"), c.grads[:ids.size].contiguous()
  return [(0, lambda: tier.find_or_insert_planned(plan, init_values=init, return_where=True), _found),
          (1, lambda: up.apply_planned(p, plan, g, c.default))]


def _t_grouped_admission_then_grouped_read(c):
  from tfra_amd.dynamic_embedding import table_ops as to
  tiers = [c.tier("g%d" % i)[2] for i in range(3)]
  b = _batch()
  kb = c.T(b)
  reqs = [(t, kb, c.rows(b, 2 + i)) for i, t in enumerate(tiers)]
  return [(0, lambda: to.tier_find_or_insert_many(reqs), lambda o: [_found(x) for x in o]),
          (1, lambda: [to.find_combine_many([(t, c.rep, c.seg, c.w, i % 3, ROWS) for i, t in enumerate(tiers)]),
                       to.find_combine_ragged_many([(t, c.splits, c.rep, c.w, i % 3) for i, t in enumerate(tiers)]),
                       to.find_combine_weight_grad_many([(t, c.rep, c.seg, c.w, 1, c.grad_out) for t in tiers])])]


def _t_lower_write_then_tier_read(c):
  _, lo, tier = c.tier("t")
  new = KEYS[SEEN:]                       # never seen by the tier: only the lower table can hold them, so the read is determined
  kn, v = c.T(new), c.rows(new, 7)
  return [(0, lambda: lo.upsert(kn, v, unique_keys=True)), (1, _tier_reads(c, tier))]


TIER = {"find_or_insert-reads": _t_find_or_insert_then_reads, "reads-insert": _t_find_combine_then_insert,
        "find_or_insert_planned-apply_planned": _t_planned_then_apply_on_the_cache,
        "tier_find_or_insert_many-grouped_reads": _t_grouped_admission_then_grouped_read,
        "lower_write-tier_reads": _t_lower_write_then_tier_read}


@pytest.mark.parametrize("name", sorted(TIER))
def test_tiers(env, streams, tmp_path, name):
  _check(env, streams, TIER[name], tmp_path)
