"""GPU: tfra_table_find_or_insert — the lookup that admits never-seen keys with the rows it returns for them.

The reference of every case is the two-call twin the header names: find(return_exists) followed by the unique upsert of
where(exists, resident row, init row) on the locked route (owner tags off).  The call must return what that find returns and leave the
table as that upsert leaves it — keys, rows, slot vectors, scores — on a growing table that grows under the calls, on crafted overflow
chains (tests/test_gpu_probe_chains.py, placement against tests/probe_model.py) and on the eviction scene at max_capacity
(tests/test_gpu_eviction.py: Scene.evict says which residents leave, Scene.check runs after every call).  Everything is compared bit
for bit."""
import numpy as np
import pytest

from tests import probe_model as pm
from tests.test_gpu_eviction import DIM, F_CALL1, F_CALL2, N_PAIRS, Ages, Scene, _distinct_scores
from tests.test_gpu_probe_chains import SLOTS, Scn, _a_locked, _build, _census, _kt, _nb, _sorted_export, _table, _vals, _vt

pytestmark = pytest.mark.gpu

EMPTY_KEY, LOCKED_KEY = -(1 << 63), -(1 << 63) + 1
SENT = 0x5A


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _rows(keys, ver, dt, dim):
  """rows that are a closed-form function of (key, version), in any of the value dtypes"""
  k = np.asarray(keys, np.int64).astype(np.uint64)
  j = np.arange(dim, dtype=np.uint64)
  with np.errstate(over="ignore"):
    x = (k[:, None] * np.uint64(2654435761) + j[None, :] * np.uint64(40503) + np.uint64(ver * 7919)) % np.uint64(65521)
  if dt == "int8":
    return ((x % np.uint64(251)).astype(np.int16) - 125).astype(np.int8)
  return (x.astype(np.float32) / np.float32(65521.0) - np.float32(0.5)).astype({"float32": np.float32, "float16": np.float16}[dt])


def _same(torch, a, b, tag):
  for x, y in zip(a, b):
    assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), tag


def _raw(tbl, n, keys, init, full, out, found, count=None, scores=None):
  """tfra_table_find_or_insert itself on buffers of the test (any of them None = NULL)"""
  import torch
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  try:
    _capi.call("tfra_table_find_or_insert", tbl._h, n, _ptr(count), _ptr(keys), _ptr(init), int(full), _ptr(scores), _ptr(out),
               _ptr(found), _stream(tbl.device))
  finally:
    torch.cuda.synchronize()


def _twin_upsert(tbl, keys, vals, scores=None):
  """the plain unique upsert on the locked route"""
  tbl.set_owner_tags(False)
  try:
    tbl.upsert(keys, vals, scores=scores, unique_keys=True)
  finally:
    tbl.set_owner_tags(True)


# ---- 1. against the two-call twin, on a table that grows -----------------------------------------------------------------------------
SHAPES = [("float32", 8, 0), ("float16", 6, 0), ("int8", 3, 0), ("float32", 72, 2)]
AUX_INIT = (0.5, 0.25, 0.0, 0.0)
N_SEED, N_CALL, N_SLOTTED = 8000, 1000, 150


@pytest.mark.parametrize("full", [True, False], ids=["init-full", "init-row"])
@pytest.mark.parametrize("dt,dim,aux", SHAPES, ids=["f32-8", "f16-6", "i8-3", "f32-72-aux2"])
def test_equals_find_then_upsert(env, dt, dim, aux, full):
  """Three calls of 1000 unique keys, a third of them resident, EMPTY_KEY and LOCKED_KEY among them, on tables seeded with 8000 keys
  at init_capacity 8192 (729 buckets, growth past 8201 keys): the table grows under the calls, by the second call's size read or at
  the third call's hard bound.  The slot vectors of 150 seeded keys are written beforehand (more would grow the table while
  seeding); 50 hits of every call are among them."""
  torch, _ = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  tdt = getattr(torch, dt)
  default = torch.full((dim,), 3, dtype=tdt)

  def mk(name):
    return _DeviceTable(torch.int64, tdt, default, name, "cuda:0", dim=dim, aux_fields=aux, init_capacity=8192, aux_init=AUX_INIT)

  a, b = mk("foi_twin_a_%s_%d_%d" % (dt, dim, full)), mk("foi_twin_b_%s_%d_%d" % (dt, dim, full))
  rng = np.random.default_rng(dim)
  pool = np.unique(rng.integers(-2**62, 2**62, size=N_SEED + 3 * N_CALL + 100, dtype=np.int64))
  rng.shuffle(pool)
  seed, never = pool[:N_SEED], pool[N_SEED:]
  slotted = seed[:N_SLOTTED]
  for t in (a, b):
    t.upsert(_kt(torch, seed), _vt(torch, _rows(seed, 1, dt, dim)))
    for f in range(1, aux + 1):
      t.upsert(_kt(torch, slotted), _vt(torch, _rows(slotted, 10 + f, dt, dim)), field=f)
    assert t.growth_stats()["growths"] == 0
  resident = list(seed[N_SLOTTED:])
  used = 0
  for call in range(3):
    n_hit = N_CALL // 3
    hits = np.concatenate([rng.choice(np.array(resident, np.int64), size=n_hit - 50, replace=False), rng.choice(slotted, size=50, replace=False)])
    special = [EMPTY_KEY, LOCKED_KEY]                       # never seen in call 0, hits from then on
    fresh = never[used:used + N_CALL - n_hit - (2 if call == 0 else 0)]
    used += fresh.size
    if call > 0:
      hits[:2] = special
    keys = np.concatenate([hits, fresh] + ([np.array(special, np.int64)] if call == 0 else []))
    rng.shuffle(keys)
    assert keys.size == N_CALL == np.unique(keys).size
    kt = _kt(torch, keys)
    init = _vt(torch, _rows(keys, 2 + call, dt, dim)) if full else _vt(torch, _rows([77], 2 + call, dt, dim)[0])
    hit_t = _kt(torch, hits)
    aux_before = [a.find(hit_t, field=f) for f in range(1, aux + 1)]
    # B: the two calls
    rows_b, ex_b = b.find(kt, dynamic_default_values=init, return_exists=True)
    want = torch.where(ex_b[:, None], rows_b, init if full else init[None, :].expand(N_CALL, dim))
    _twin_upsert(b, kt, want.contiguous())
    # A: the one call
    rows_a, ex_a = a.find_or_insert(kt, init, return_exists=True)
    torch.cuda.synchronize()
    assert int(ex_b.sum()) == n_hit, call
    assert torch.equal(ex_a, ex_b), call
    _same(torch, [rows_a], [want], "values_out, call %d" % call)
    ea, eb = _sorted_export(torch, a), _sorted_export(torch, b)
    _same(torch, ea, eb, "exports differ after call %d" % call)
    for f in range(1, aux + 1):
      _same(torch, [a.find(hit_t, field=f)], [aux_before[f - 1]], "slot vector %d of a hit was written" % f)
      new = kt[~ex_a]
      assert bool((a.find(new, field=f) == AUX_INIT[f - 1]).all()), "slot vector %d of a new key is not at aux_init" % f
      _same(torch, [a.find(ea[0], field=f)], [b.find(eb[0], field=f)], "slot vectors %d differ" % f)
    resident = sorted(set(resident) | ({int(k) for k in keys} - set(special) - set(slotted.tolist())))
  for t in (a, b):
    t.check_errors()
    assert t.size_host() == N_SEED + 3 * N_CALL - 3 * (N_CALL // 3)
    assert t.growth_stats()["growths"] >= 1, "no call grew the table"


# ---- 2. the count on the device, NULL outputs ---------------------------------------------------------------------------------------
def test_device_count_and_null_outputs(env):
  torch, _ = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  dim, n = 8, 1000
  mk = lambda name: _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), name, "cuda:0", dim=dim, init_capacity=8192)
  a, c, d = mk("foi_dn_a"), mk("foi_dn_c"), mk("foi_dn_d")
  keys = np.arange(1, n + 1, dtype=np.int64) * 7919
  old = keys[::3]
  for t in (a, c, d):
    t.upsert(_kt(torch, old), _vt(torch, _rows(old, 1, "float32", dim)))
  kt, init = _kt(torch, keys), _vt(torch, _rows(keys, 2, "float32", dim))
  # *d_n = n // 2
  out8 = torch.full((n * dim * 4,), SENT, dtype=torch.uint8, device="cuda")
  found = torch.full((n,), SENT, dtype=torch.uint8, device="cuda")
  _raw(a, n, kt, init, 1, out8, found, count=torch.tensor([n // 2], dtype=torch.int64, device="cuda"))
  h = n // 2
  is_old = np.isin(keys, old)
  want = np.where(is_old[:, None], _rows(keys, 1, "float32", dim), _rows(keys, 2, "float32", dim))
  np.testing.assert_array_equal(out8.view(torch.float32).reshape(n, dim)[:h].cpu().numpy(), want[:h])
  np.testing.assert_array_equal(found[:h].cpu().numpy(), is_old[:h].astype(np.uint8))
  assert bool((out8[h * dim * 4:] == SENT).all()) and bool((found[h:] == SENT).all()), "written beyond the count"
  _, ex = a.find(kt, return_exists=True)
  np.testing.assert_array_equal(ex.cpu().numpy(), is_old | (np.arange(n) < h))
  a.check_errors()
  # values_out == NULL and found == NULL: the same table as the full call
  _raw(c, n, kt, init, 1, None, None)
  rows_d, ex_d = d.find_or_insert(kt, init, return_exists=True)
  np.testing.assert_array_equal(rows_d.cpu().numpy(), want)
  np.testing.assert_array_equal(ex_d.cpu().numpy(), is_old)
  _same(torch, _sorted_export(torch, c), _sorted_export(torch, d), "admit-only and full call differ")
  assert c.size_host() == d.size_host() == n


# ---- 3. collision chains ------------------------------------------------------------------------------------------------------------
def _bucket_keys(torch, tbl, b):
  """the keys bucket b holds: export_batch over its 15 slots"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  counter = torch.zeros(1, dtype=torch.int64, device="cuda")
  k = torch.empty(SLOTS, dtype=torch.int64, device="cuda")
  _capi.call("tfra_table_export_batch", tbl._h, SLOTS, b * SLOTS, _ptr(counter), _ptr(k), None, None, _stream(tbl.device))
  return set(k[:int(counter.item())].cpu().numpy().tolist())


@pytest.mark.parametrize("kind", ["mid", "wrap"])
def test_on_collision_chains(env, kind):
  """The chain of tests/test_gpu_probe_chains.py (11 buckets deep; "wrap": over the last bucket) with holes in its buckets 0 and 2.
  One call carries the keys at the chain's end (hits), bystanders (hits), 20 new keys of the pair and 8 more: the hits come back
  with their rows, the new keys fill the holes — every chain bucket holds as many keys as the sequential model's, the new keys sit
  in the model's buckets, the census is the model's and the flags do not move."""
  torch, _ = env
  tbl = _table(env, "foi_chain_" + kind)
  scn = Scn(_nb(tbl), kind)
  ref, model = {}, pm.FirstFit(scn.nb)
  _build(env, tbl, scn, _a_locked, "float32", ref, model, None, exact=True)
  holes = np.concatenate([scn.chain[0:15], scn.chain[30:45]])
  tbl.erase(_kt(torch, holes))
  for k in holes:
    model.erase(k)
    del ref[int(k)]
  flags = tbl.slot_census()
  deep = np.concatenate([scn.chain[75:90], scn.chain[150:160]])
  assert sorted({model.depth_of(k) for k in deep}) == [5, 10]
  new = np.concatenate([scn.extra, scn.absent[:8]])
  keys = np.concatenate([deep, scn.by[:40], new])
  np.random.default_rng(5).shuffle(keys)
  init = _vals(keys, 2)
  rows, ex = tbl.find_or_insert(_kt(torch, keys), _vt(torch, init), return_exists=True)
  torch.cuda.synchronize()
  tbl.check_errors()
  is_new = np.isin(keys, new)
  np.testing.assert_array_equal(ex.cpu().numpy(), ~is_new)
  want = np.stack([init[i] if is_new[i] else ref[int(k)] for i, k in enumerate(keys)])
  np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint8), want.view(np.uint8))
  for k in new:
    assert model.insert(k)
  assert {model.bucket_of(k) for k in new} == {scn.chain_buckets[0], scn.chain_buckets[2]}
  on_device = {b: _bucket_keys(torch, tbl, b) for b in range(scn.nb)}
  for b in scn.chain_buckets:       # (elsewhere the racing batches of the build decide which pile key went to which of its b1)
    assert len(on_device[b]) == SLOTS - model.slots[b].count(None), ("bucket", b)
  where = {k: b for b, ks in on_device.items() for k in ks}
  assert {where[int(k)] for k in new} == {model.bucket_of(k) for k in new}
  c = _census(tbl, model, False, "after find_or_insert")
  assert (c["ovf0"], c["ovf1"]) == (flags["ovf0"], flags["ovf1"])
  ref.update({int(k): init[i] for i, k in enumerate(keys) if is_new[i]})
  everything = np.concatenate([scn.resident(), scn.absent, scn.extra])
  got, ex = tbl.find(_kt(torch, everything), return_exists=True)
  np.testing.assert_array_equal(ex.cpu().numpy(), np.array([int(k) in ref for k in everything]))
  wrows = np.stack([ref.get(int(k), tbl._default_value.cpu().numpy()) for k in everything])
  np.testing.assert_array_equal(got.cpu().numpy().view(np.uint8), wrows.view(np.uint8))
  assert tbl.size_host() == len(ref) and tbl.growth_stats()["growths"] == 0


# ---- 4. at max_capacity -------------------------------------------------------------------------------------------------------------
def _foi(scn, keys, init, score):
  """find_or_insert on the scene's table -> (rows, found) as numpy"""
  torch = scn.env[0]
  sc = None if score is None else _kt(torch, np.array([score[int(k)] for k in keys], np.int64))
  rows, ex = scn.tbl.find_or_insert(_kt(torch, keys), _vt(torch, init), scores=sc, return_exists=True)
  torch.cuda.synchronize()
  return rows.cpu().numpy(), ex.cpu().numpy()


def _twin(b, keys, vals, score):
  torch = b.env[0]
  sc = None if score is None else _kt(torch, np.array([score[int(k)] for k in keys], np.int64))
  _twin_upsert(b.tbl, _kt(torch, keys), _vt(torch, vals), sc)
  torch.cuda.synchronize()


@pytest.mark.parametrize("strategy", ["CUSTOMIZED", "LRU"])
def test_at_max_capacity(env, strategy):
  """CUSTOMIZED: test_victim_set_customized's two calls (F = 1, 4, 15, 30 fresh keys for the four pairs, then rotated), scores above
  every resident's, and in every pair that keeps residents its two highest-scoring ones as hits, with new caller scores above
  everything.  LRU (residents in six calls of five): every F a whole number of calls, the hits a whole call's residents, which
  become the youngest.  The residents that leave are the model's; a hit returns its row, keeps it and takes the score of an assign;
  the table is byte-identical to a twin scene given the plain unique upsert of where(found, row, init) on the locked route (LRU:
  everything but the device clocks)."""
  lru = strategy == "LRU"
  mk = lambda name: (Scene(env, name, "LRU", groups=(5,) * 6) if lru else Scene(env, name, "CUSTOMIZED", score=_distinct_scores(1)))
  a, b = mk("foi_cap_a_" + strategy), mk("foi_cap_b_" + strategy)
  ages = Ages(a) if lru else None
  used = [0] * N_PAIRS
  lru_hits = [(0, 0, None, 0), (4, 4, None, None)]      # per call and pair: the group of residents (a call of five) that is hit
  for call, fs in enumerate(((5, 10, 30, 15), (10, 5, 0, 30)) if lru else (F_CALL1, F_CALL2)):
    fresh = [a.fresh[i][used[i]:used[i] + f] for i, f in enumerate(fs)]
    fkeys = np.concatenate(fresh)
    if lru:
      hits = [int(k) for i in range(N_PAIRS) if lru_hits[call][i] is not None
              for k in a.res[i][5 * lru_hits[call][i]:5 * lru_hits[call][i] + 5]]
    else:
      hits = [k for i in range(N_PAIRS) if fs[i] < 30 for k in a.order(i)[-2:]]
    assert hits and all(k in a.present for k in hits)
    keys = np.concatenate([fkeys, np.array(hits, np.int64)])
    np.random.default_rng(call).shuffle(keys)
    is_hit = np.isin(keys, hits)
    init = a.rows(keys, 2 + call)
    row_before = {k: a.present[k][0].copy() for k in hits}
    want = np.stack([row_before[int(k)] if is_hit[j] else init[j] for j, k in enumerate(keys)])
    before = set(a.present)
    if lru:
      score = None
      gone = ages.call(hits, fkeys, 2 + call)
      for k in hits:                                   # (Ages.call models an assign of new rows: a hit keeps its row)
        a.present[k][0] = row_before[k]
    else:
      score = {int(k): 5000 * (call + 1) + j for j, k in enumerate(fkeys)}
      score.update({k: 5000 * (call + 1) + 1000 + j for j, k in enumerate(hits)})   # (below the next call's fresh scores)
      for k in hits:
        a.present[k][1] = score[k]                     # CUSTOMIZED: an assign takes the caller's score
      gone = []
      for i, f in enumerate(fresh):
        gone += a.evict(i, f, [score[int(k)] for k in f], [score[int(k)] for k in f], 2 + call)
    for i, f in enumerate(fresh):
      used[i] += f.size
    assert not set(gone) & set(hits)
    b.present = {x: [r[0].copy(), r[1]] for x, r in a.present.items()}
    rows, found = _foi(a, keys, init, score)
    _twin(b, keys, want, score)
    np.testing.assert_array_equal(found, is_hit)
    np.testing.assert_array_equal(rows.view(np.uint8), want.view(np.uint8))
    a.check("find_or_insert, call %d" % call)
    b.check("twin, call %d" % call)
    assert before - set(a.snap()[0].cpu().numpy().tolist()) == set(gone)
    sa, sb = a.snap(), b.snap()
    a.same(sa[:2] if lru else sa, sb[:2] if lru else sb, "the two tables differ after call %d" % call)


def test_at_max_capacity_device_count_and_one_init_row(env):
  """The three ways phase 2 gets its rows, each on a batch of fresh keys that all evict: one init row per key with the count on the
  device (four more keys lie beyond the count: they stay out, outputs beyond it keep their sentinel); ONE init row with values_out
  (phase 2 reads the rows phase 1 put there); one init row with values_out == NULL and found == NULL (phase 1 leaves the deferred
  keys' rows in the table's scratch)."""
  torch = env[0]
  scn = Scene(env, "foi_cap_dn", "CUSTOMIZED", score=_distinct_scores(1))
  used = [0] * N_PAIRS

  def batch(call, fs):
    fresh = [scn.fresh[i][used[i]:used[i] + f] for i, f in enumerate(fs)]
    keys = np.concatenate(fresh)
    score = {int(k): 5000 * (call + 1) + j for j, k in enumerate(keys)}
    for i, f in enumerate(fresh):
      scn.evict(i, f, [score[int(k)] for k in f], [score[int(k)] for k in f], 2 + call)
      used[i] += f.size
    return keys, score

  # one init row per key, the count on the device
  keys, score = batch(0, (1, 4, 15, 10))
  pad = np.array([scn.fresh[i][44] for i in range(N_PAIRS)], np.int64)
  buf = np.concatenate([keys, pad])
  score.update({int(k): 9000 + i for i, k in enumerate(pad)})
  n, m = buf.size, keys.size
  init = scn.rows(buf, 2)
  out8 = torch.full((n * DIM * 4,), SENT, dtype=torch.uint8, device="cuda")
  found = torch.full((n,), SENT, dtype=torch.uint8, device="cuda")
  _raw(scn.tbl, n, _kt(torch, buf), _vt(torch, init), 1, out8, found, count=torch.tensor([m], dtype=torch.int64, device="cuda"),
       scores=_kt(torch, np.array([score[int(k)] for k in buf], np.int64)))
  np.testing.assert_array_equal(out8.view(torch.float32).reshape(n, DIM)[:m].cpu().numpy(), init[:m])
  assert not bool(found[:m].any())
  assert bool((out8[m * DIM * 4:] == SENT).all()) and bool((found[m:] == SENT).all()), "written beyond the count"
  scn.check("device count")          # (a key beyond the count that got in would be resident and not expected)
  # ONE init row, values_out given
  keys, score = batch(1, (10, 1, 4, 15))
  row = scn.rows([123], 7)
  for k in keys:
    scn.present[int(k)][0] = row[0]
  rows, ex = _foi(scn, keys, row[0], score)
  assert not ex.any()
  np.testing.assert_array_equal(rows, np.repeat(row, keys.size, axis=0))
  scn.check("one init row")
  # ONE init row, no outputs
  keys, score = batch(2, (4, 10, 1, 4))
  row = scn.rows([456], 8)
  for k in keys:
    scn.present[int(k)][0] = row[0]
  _raw(scn.tbl, keys.size, _kt(torch, keys), _vt(torch, row[0]), 0, None, None,
       scores=_kt(torch, np.array([score[int(k)] for k in keys], np.int64)))
  scn.check("one init row, no outputs")


def test_below_the_minimum_is_not_admitted(env):
  """One fresh key per pair scoring minimum - 1, next to one hit per pair: found = 0 and the init row for the fresh keys, which stay
  out; nothing of the table changes but the hits' scores."""
  scn = Scene(env, "foi_refused", "CUSTOMIZED", aux=1, aux_init=(0.5, 0.0, 0.0, 0.0), score=_distinct_scores(2))
  mins = [scn.order(i)[0] for i in range(N_PAIRS)]
  lo = [scn.present[m][1] for m in mins]
  fresh = np.array([scn.fresh[i][0] for i in range(N_PAIRS)], np.int64)
  hits = [scn.order(i)[-1] for i in range(N_PAIRS)]
  keys = np.concatenate([fresh, np.array(hits, np.int64)])
  score = {int(x): lo[i] - 1 for i, x in enumerate(fresh)}
  score.update({k: 30000 + i for i, k in enumerate(hits)})
  init = scn.rows(keys, 2)
  before = scn.snap()
  rows, found = _foi(scn, keys, init, score)
  np.testing.assert_array_equal(found, np.array([False] * N_PAIRS + [True] * N_PAIRS))
  want = np.concatenate([init[:N_PAIRS], np.stack([scn.present[k][0] for k in hits])])
  np.testing.assert_array_equal(rows.view(np.uint8), want.view(np.uint8))
  for k in hits:
    scn.present[k][1] = score[k]
  scn.check("below the minimum")
  after = scn.snap()
  scn.same([before[0], before[1], before[3]], [after[0], after[1], after[3]], "keys, rows or slot vectors changed")
  changed = (before[2] != after[2]).cpu().numpy()
  assert set(after[0].cpu().numpy()[changed].tolist()) == set(hits)


def test_lfu_hit_counts_like_an_assign(env):
  """LFU: a hit adds the caller's score to the resident's count, as an assign does; a fresh key at exactly the minimum is admitted
  and starts a new life with its own score."""
  scn = Scene(env, "foi_lfu", "LFU", score=_distinct_scores(2))
  hits = [scn.order(i)[-1] for i in range(N_PAIRS)]
  mins = [scn.order(i)[0] for i in range(N_PAIRS)]
  fresh = np.array([scn.fresh[i][0] for i in range(N_PAIRS)], np.int64)
  keys = np.concatenate([np.array(hits, np.int64), fresh])
  score = {k: 7 + i for i, k in enumerate(hits)}
  score.update({int(x): scn.present[mins[i]][1] for i, x in enumerate(fresh)})
  row_before = [scn.present[k][0].copy() for k in hits]
  for k in hits:
    scn.present[k][1] += score[k]
  for i, x in enumerate(fresh):
    assert scn.evict(i, [x], [score[int(x)]], [score[int(x)]], 2) == [mins[i]]
  init = scn.rows(keys, 2)
  rows, found = _foi(scn, keys, init, score)
  np.testing.assert_array_equal(found, np.array([True] * N_PAIRS + [False] * N_PAIRS))
  np.testing.assert_array_equal(rows.view(np.uint8), np.concatenate([np.stack(row_before), init[N_PAIRS:]]).view(np.uint8))
  scn.check("LFU")


# ---- 5. refusals and the empty call -------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_call(env):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _stream
  tbl = _table(env, "foi_refuse")
  old = np.arange(1, 301, dtype=np.int64) * 104729
  tbl.upsert(_kt(torch, old), _vt(torch, _vals(old, 1)))
  before = _sorted_export(torch, tbl)
  new = _kt(torch, np.arange(1, 9, dtype=np.int64) * 15485863)
  init = _vt(torch, _vals(new.cpu().numpy(), 2))
  out = torch.full((8, DIM), -9.0, device="cuda")
  for k, i in ((None, init), (new, None)):
    with pytest.raises(_capi.TfraError) as e:
      _raw(tbl, 8, k, i, 1, out, None)
    assert e.value.code == -1 and "tfra_table_find_or_insert" in str(e.value)
  assert bool((out == -9.0).all())
  _same(torch, before, _sorted_export(torch, tbl), "a refused call changed the table")
  tbl.check_errors()
  assert tbl.size_host() == 300
  # n == 0
  _capi.call("tfra_table_find_or_insert", tbl._h, 0, None, None, None, 0, None, None, None, _stream(tbl.device))
  rows, ex = tbl.find_or_insert(new[:0], init[:0], return_exists=True)
  assert tuple(rows.shape) == (0, DIM) and ex.numel() == 0
  torch.cuda.synchronize()
  _same(torch, before, _sorted_export(torch, tbl), "an empty call changed the table")
  # the table's default row when no init rows are given; the wrappers
  rows, ex = tbl.find_or_insert(new[:4], return_exists=True)
  assert not bool(ex.any()) and torch.equal(rows, tbl._default_value[None, :].expand(4, DIM))
  rows, ex = tbl.find_or_insert(new[:4], init[:4], return_exists=True)
  assert bool(ex.all()) and torch.equal(rows, tbl._default_value[None, :].expand(4, DIM))
  tbl.check_errors()
  assert tbl.size_host() == 304
