"""GPU: tfra_table_insert_and_evict — the insert that hands back what it displaces.

The scene, the model and the conditions after every call are those of tests/test_gpu_eviction.py (class Scene: a table of 15 * 89 slots
at max_capacity, four full bucket pairs, bystanders that keep it in the dense regime; Scene.evict says from the scores the test wrote
which resident leaves; Scene.check runs after every call under test).  On top of them: the call reports exactly the entries the
model says leave, each with the row and the score the scene recorded before the call; a key that is not admitted comes back with
the caller's row and its compare score; the table ends byte-identical to a twin that received the plain unique upsert on the locked
route (owner tags off); counter and cap follow export_batch_if's rules; off max_capacity nothing is reported.  Everything is compared
bit for bit."""
import numpy as np
import pytest

from tests.test_gpu_eviction import (CAP, DIM, F_CALL1, F_CALL2, N_PAIRS, Ages, Scene, _assign, _distinct_scores, _word)
from tests.test_gpu_probe_chains import _kt, _sorted_export, _vals, _vt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _call(scn, keys, vals, score, **kw):
  """one upsert_and_evict on the scene's table -> (counter, keys, rows, scores): the counter as the device wrote it, the buffers
  trimmed to min(counter, their length)"""
  torch = scn.env[0]
  keys = np.asarray(keys, np.int64)
  sc = None if score is None else _kt(torch, np.array([score[int(k)] for k in keys], np.int64))
  cnt, k, v, s = scn.tbl.upsert_and_evict(_kt(torch, keys), _vt(torch, vals), scores=sc, sync=False, **kw)
  torch.cuda.synchronize()
  n = int(cnt.item())
  m = min(n, k.numel())
  return n, k[:m].cpu().numpy(), v[:m].cpu().numpy(), s[:m].cpu().numpy()


def _entries(k, v, s):
  """{key: (row bytes, score)} of a reported list; no key twice"""
  assert np.unique(k).size == k.size, "a key is reported twice"
  return {int(x): (v[i].tobytes(), int(s[i])) for i, x in enumerate(k)}


def _rows_now(scn, keys, whole):
  """{key: bytes}: the row the scene recorded for each of `keys`; whole rows: followed by the slot vectors as find(field=f) reports
  them now (a find changes nothing)"""
  torch = scn.env[0]
  keys = [int(k) for k in keys]
  parts = [np.stack([scn.present[k][0] for k in keys])]
  if whole:
    parts += [scn.tbl.find(_kt(torch, np.array(keys, np.int64)), field=f).cpu().numpy() for f in range(1, scn.aux + 1)]
  full = np.concatenate(parts, axis=1)
  return {k: full[i].tobytes() for i, k in enumerate(keys)}


def _write_slots(scn):
  """every resident's slot vector f = rows of version 30 + f (a field insert sets a CUSTOMIZED score to 1: the residents are written
  again with their scores afterwards)"""
  torch = scn.env[0]
  res = np.concatenate(scn.res)
  for f in range(1, scn.aux + 1):
    scn.tbl.upsert(_kt(torch, res), _vt(torch, scn.rows(res, 30 + f)), field=f)
  sc = np.array([scn.present[int(k)][1] for k in res], np.int64)
  scn.tbl.upsert(_kt(torch, res), _vt(torch, scn.rows(res, 1)), scores=_kt(torch, sc), unique_keys=True)
  torch.cuda.synchronize()
  scn.check("slot vectors written")
  for f in range(1, scn.aux + 1):
    np.testing.assert_array_equal(scn.tbl.find(_kt(torch, res), field=f).cpu().numpy(), scn.rows(res, 30 + f))


# ---- 1. victims come back ----------------------------------------------------------------------------------------------------------------
SHAPES = [("float32", 8, 0, False), ("float16", 6, 0, False), ("float32", 72, 2, True)]


@pytest.mark.parametrize("dt,dim,aux,whole", SHAPES, ids=["f32-8", "f16-6", "f32-72-aux2-whole"])
def test_victims_come_back(env, dt, dim, aux, whole):
  """test_victim_set_customized's two calls: the reported key set is exactly what Scene.evict says leaves, each entry with the row
  (whole rows: and the slot vectors) and the score it had before the call; the counter is the list's length."""
  scn = Scene(env, "ie_victims_%s_%d" % (dt, dim), "CUSTOMIZED", dt=dt, dim=dim, aux=aux, aux_init=(0.5, 0.25, 0.0, 0.0), score=_distinct_scores(1))
  if aux:
    _write_slots(scn)
  used = [0] * N_PAIRS
  for call, fs in enumerate((F_CALL1, F_CALL2)):
    fresh = [scn.fresh[i][used[i]:used[i] + f] for i, f in enumerate(fs)]
    keys = np.concatenate(fresh)
    score = {int(k): 5000 * (call + 1) + j for j, k in enumerate(keys)}
    resident = sorted(scn.present)
    rows_before = _rows_now(scn, resident, whole)
    score_before = {k: scn.present[k][1] for k in resident}
    gone = []
    for i, f in enumerate(fresh):
      gone += scn.evict(i, f, [score[int(k)] for k in f], [score[int(k)] for k in f], 2 + call)
      used[i] += f.size
    n, k, v, s = _call(scn, keys, scn.rows(keys, 2 + call), score, whole_rows=whole)
    scn.check("victims, call %d" % call)
    got = _entries(k, v, s)
    assert n == len(gone) == len(got), (n, len(gone), len(got))
    assert sorted(got) == sorted(gone)
    for x in gone:
      assert got[x] == (rows_before[x], score_before[x]), (call, scn.pair_of(x))


# ---- 2. the same table as the plain call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["CUSTOMIZED", "LRU"])
def test_same_table_as_the_plain_call(env, strategy):
  """A twin scene receives the same batches through the plain unique upsert on the locked route: byte-identical tables after each
  call (LRU: everything but the device-clock scores).  LRU: residents in six calls of five, every F a whole number of calls."""
  lru = strategy == "LRU"
  mk = lambda name: (Scene(env, name, "LRU", groups=(5,) * 6) if lru else Scene(env, name, "CUSTOMIZED", score=_distinct_scores(1)))
  a, b = mk("ie_same_a_" + strategy), mk("ie_same_b_" + strategy)
  ages = Ages(a) if lru else None
  used = [0] * N_PAIRS
  for call, fs in enumerate(((5, 10, 30, 15), (25, 5, 0, 30)) if lru else (F_CALL1, F_CALL2)):
    fresh = [a.fresh[i][used[i]:used[i] + f] for i, f in enumerate(fs)]
    keys = np.concatenate(fresh)
    score = None if lru else {int(k): 5000 * (call + 1) + j for j, k in enumerate(keys)}
    if lru:
      gone = ages.call([], keys, 2 + call)
    else:
      gone = []
      for i, f in enumerate(fresh):
        gone += a.evict(i, f, [score[int(k)] for k in f], [score[int(k)] for k in f], 2 + call)
    for i, f in enumerate(fresh):
      used[i] += f.size
    b.present = {x: list(r) for x, r in a.present.items()}
    n, k, _, _ = _call(a, keys, a.rows(keys, 2 + call), score)
    _assign(b, "notags", keys, 2 + call, score)
    a.check("captured, call %d" % call)
    b.check("plain, call %d" % call)
    sa, sb = a.snap(), b.snap()
    a.same(sa[:2] if lru else sa, sb[:2] if lru else sb, "the two tables differ after call %d" % call)
    assert n == len(gone) and sorted(k.tolist()) == sorted(gone)


# ---- 3. keys that are not admitted -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["CUSTOMIZED", "LFU", "EPOCHLFU"])
def test_refused_keys_are_reported(env, strategy):
  """One fresh key per pair scoring minimum - 1: the table is byte-identical, the four entries are the caller's keys, rows (slot
  vectors at aux_init) and compare scores.  The same keys at exactly the minimum: the four minima come back, no fresh key does."""
  epoch = 5
  scn = Scene(env, "ie_refused_" + strategy, strategy, aux=1, aux_init=(0.5, 0.0, 0.0, 0.0), score=_distinct_scores(2),
              epochs=[epoch, epoch] if strategy == "EPOCHLFU" else None)
  mins = [scn.order(i)[0] for i in range(N_PAIRS)]
  lo = [scn.present[m][1] & 0xffffffff for m in mins]
  assert lo == [1000] * N_PAIRS
  keys = np.array([scn.fresh[i][0] for i in range(N_PAIRS)], np.int64)
  before = scn.snap()
  n, k, v, s = _call(scn, keys, scn.rows(keys, 2), {int(x): lo[i] - 1 for i, x in enumerate(keys)}, whole_rows=True)
  scn.same(before, scn.snap(), "below the minimum")
  scn.check("below the minimum")
  got = _entries(k, v, s)
  assert n == 4 and sorted(got) == sorted(keys.tolist())
  aux = np.full(DIM, 0.5, np.float32).tobytes()
  for i, x in enumerate(keys.tolist()):
    assert got[x] == (scn.rows([x], 2)[0].tobytes() + aux, _word(strategy, epoch, lo[i] - 1)), scn.pair_of(x)
  # exactly the minimum: admitted, the minimum goes
  rows_before = _rows_now(scn, mins, True)
  score_before = {m: scn.present[m][1] for m in mins}
  for i, x in enumerate(keys):
    w = _word(strategy, epoch, lo[i])
    assert scn.evict(i, [x], [w], [w], 3) == [mins[i]]
  n, k, v, s = _call(scn, keys, scn.rows(keys, 3), {int(x): lo[i] for i, x in enumerate(keys)}, whole_rows=True)
  scn.check("equal to the minimum")
  got = _entries(k, v, s)
  assert n == 4 and sorted(got) == sorted(mins)
  for m in mins:
    assert got[m] == (rows_before[m], score_before[m]), scn.pair_of(m)


# ---- 4. nothing is lost inside one launch -------------------------------------------------------------------------------------------------
def _interleave(fresh, fillers):
  """rounds of 16 positions: one fresh key of each pair at positions 0, 4, 8, 12, fillers between them — two keys of one pair are
  16 positions apart, so their evictions run in different blocks"""
  per = len(fresh[0])
  assert all(len(f) == per for f in fresh) and len(fillers) == 12 * per
  out, it = [], iter(fillers)
  for r in range(per):
    for i in range(N_PAIRS):
      out += [int(fresh[i][r])] + [int(next(it)) for _ in range(3)]
  return np.array(out, np.int64)


def _conserved(scn, keys, ver_of, score, own_score, expect_reports):
  """the call, then conservation: {resident before} U {batch} = {resident after} + {reported}, no key twice, every reported entry
  with its own row (the batch's for batch keys) and, where the test knows it, its own score.  -> the export after the call"""
  torch = scn.env[0]
  kb = scn.snap()[0].cpu().numpy()
  vals = np.stack([scn.rows([k], ver_of[int(k)])[0] for k in keys])
  n, k, v, s = _call(scn, keys, vals, score)
  scn.tbl.check_errors()
  got = _entries(k, v, s)
  ka, _, sa = _sorted_export(torch, scn.tbl, with_scores=True)
  ka = ka.cpu().numpy()
  assert n == len(got) == expect_reports, (n, len(got), expect_reports)
  assert np.unique(ka).size == ka.size == scn.tbl.size_host() == scn.n_live
  assert not set(ka.tolist()) & set(got), "a reported key is still resident"
  assert set(kb.tolist()) | set(keys.tolist()) == set(ka.tolist()) | set(got)
  for x, (row, sc) in got.items():
    assert row == scn.rows([x], ver_of.get(x, 1))[0].tobytes(), ("row of", scn.pair_of(x))
    if x in own_score:
      assert sc == own_score[x], ("score of", scn.pair_of(x), sc, own_score[x])
  return ka, sa.cpu().numpy()


def test_nothing_is_lost_customized(env):
  """Eight fresh keys per pair scoring between the residents, interleaved with hits that rewrite the same row and score (the twelve
  highest residents of each pair, bystanders).  Which fresh key ends resident is a race; every one of the 32 reports exactly one
  entry (itself, or what it replaced), and nothing is lost."""
  scn = Scene(env, "ie_cons_c", "CUSTOMIZED", score=_distinct_scores(4))
  fresh = [scn.fresh[i][:8] for i in range(N_PAIRS)]
  own_score = {k: r[1] for k, r in scn.present.items()}
  own_score.update({int(k): 1 for k in scn.by})
  ver_of = {}
  for i in range(N_PAIRS):
    for j, k in enumerate(fresh[i].tolist()):
      own_score[k] = 1000 + 3 * (2 + 3 * j) + 1      # between two resident scores (1000 + 3 p)
      ver_of[k] = 2
  hits = [k for i in range(N_PAIRS) for k in scn.order(i)[-12:]] + scn.by[:48].tolist()
  np.random.default_rng(0).shuffle(hits)
  keys = _interleave(fresh, hits)
  for k in hits:
    ver_of[int(k)] = 1
  ka, _ = _conserved(scn, keys, ver_of, {int(k): own_score[int(k)] for k in keys}, own_score, 32)
  isby = np.isin(ka, scn.by)
  scn.present = {x: [scn.rows([x], ver_of.get(x, 1))[0], own_score[x]] for x in ka[~isby].tolist()}
  scn.check("conservation, CUSTOMIZED")


def test_nothing_is_lost_lru(env):
  """Thirty fresh keys per pair on an LRU table, interleaved with hits on bystanders: every resident of the pairs comes back with
  the row and the clock it had, every fresh key is resident.  (The hit bystanders' clocks move forward: the only change the scene's
  bystander snapshot is told of.)"""
  torch = env[0]
  scn = Scene(env, "ie_cons_l", "LRU")
  fresh = [scn.fresh[i][:30] for i in range(N_PAIRS)]
  ver_of = {int(k): 2 for f in fresh for k in f}
  hits = scn.by[:360]
  ver_of.update({int(k): 1 for k in hits})
  keys = _interleave(fresh, hits.tolist())
  kb, _, sb = scn.snap()[:3]
  own_score = dict(zip(kb.cpu().numpy().tolist(), sb.cpu().numpy().tolist()))
  ka, sa = _conserved(scn, keys, ver_of, None, own_score, 120)
  isby = np.isin(ka, scn.by)
  assert np.array_equal(ka[isby], scn.by_snap[0].cpu().numpy())
  old, new = scn.by_snap[2].cpu().numpy(), sa[isby]
  hit = np.isin(ka[isby], hits)
  assert (new[hit] > old[hit]).all() and np.array_equal(new[~hit], old[~hit])
  scn.by_snap = (scn.by_snap[0], scn.by_snap[1], torch.from_numpy(new).cuda())
  scn.present = {x: [scn.rows([x], ver_of.get(x, 1))[0], None] for x in ka[~isby].tolist()}
  assert sorted(scn.present) == sorted(int(k) for f in fresh for k in f)
  scn.check("conservation, LRU")


# ---- 5. counter and cap ------------------------------------------------------------------------------------------------------------------
SENT = 0x5A


def _raw(scn, keys, vals, score, flags, cap, ek, ev, es):
  """tfra_table_insert_and_evict itself, on buffers of the test -> the counter"""
  torch = scn.env[0]
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  kt, vt = _kt(torch, keys), _vt(torch, vals)
  st = _kt(torch, np.array([score[int(k)] for k in keys], np.int64))
  counter = torch.zeros(1, dtype=torch.int64, device="cuda")
  try:
    _capi.call("tfra_table_insert_and_evict", scn.tbl._h, kt.numel(), _ptr(kt), _ptr(vt), _ptr(st), flags, _ptr(counter), cap, _ptr(ek),
               _ptr(ev), _ptr(es), _stream(scn.tbl.device))
  finally:
    torch.cuda.synchronize()
  return int(counter.item())


def test_cap_and_count_only(env):
  """cap = half the expected count, buffers pre-filled with a sentinel: the counter is the full count, exactly cap entries are
  written (distinct, each one of the expected, each correct), every byte behind them is still the sentinel; the table equals an
  uncapped twin.  evicted_keys == NULL: the full count, nothing else.  NULL keys with non-NULL values: TFRA_ERR_INVALID, nothing
  changes."""
  torch = env[0]
  from tfra_amd import _capi
  a, b = [Scene(env, "ie_cap_" + x, "CUSTOMIZED", score=_distinct_scores(1)) for x in "ab"]
  used = [0] * N_PAIRS

  def batch(call, fs):
    fresh = [a.fresh[i][used[i]:used[i] + f] for i, f in enumerate(fs)]
    keys = np.concatenate(fresh)
    score = {int(k): 5000 * (call + 1) + j for j, k in enumerate(keys)}
    before = {x: (r[0].tobytes(), r[1]) for x, r in a.present.items()}
    gone = []
    for i, f in enumerate(fresh):
      gone += a.evict(i, f, [score[int(k)] for k in f], [score[int(k)] for k in f], 2 + call)
      used[i] += f.size
    b.present = {x: list(r) for x, r in a.present.items()}
    return keys, score, before, gone

  # capped
  keys, score, before, gone = batch(0, F_CALL1)
  n, cap = keys.size, len(gone) // 2
  assert len(gone) == 50 and cap == 25
  ek8, ev8, es8 = [torch.full((n * w,), SENT, dtype=torch.uint8, device="cuda") for w in (8, DIM * 4, 8)]
  count = _raw(a, keys, a.rows(keys, 2), score, 0, cap, ek8, ev8, es8)
  assert count == len(gone)
  k, v, s = ek8.view(torch.int64).cpu().numpy(), ev8.view(torch.float32).reshape(n, DIM).cpu().numpy(), es8.view(torch.int64).cpu().numpy()
  got = _entries(k[:cap], v[:cap], s[:cap])
  assert len(got) == cap and set(got) <= set(gone)
  for x, e in got.items():
    assert e == before[x], a.pair_of(x)
  for buf, w in ((ek8, 8), (ev8, DIM * 4), (es8, 8)):
    assert bool((buf[cap * w:] == SENT).all()), "written at or beyond cap"
  n_b, k_b, _, _ = _call(b, keys, b.rows(keys, 2), score)
  assert n_b == len(gone) and sorted(k_b.tolist()) == sorted(gone)
  a.check("capped")
  b.check("uncapped twin")
  a.same(a.snap(), b.snap(), "capped and uncapped tables differ")
  # count only
  keys, score, before, gone = batch(1, F_CALL2)
  assert _raw(a, keys, a.rows(keys, 3), score, 0, 0, None, None, None) == len(gone)
  n_b, k_b, _, _ = _call(b, keys, b.rows(keys, 3), score)
  assert n_b == len(gone) and sorted(k_b.tolist()) == sorted(gone)
  a.check("count only")
  b.check("twin of count only")
  a.same(a.snap(), b.snap(), "count-only and reporting tables differ")
  # NULL keys with a values buffer
  snap = a.snap()
  more = np.array([a.fresh[i][0] for i in range(N_PAIRS)], np.int64)
  with pytest.raises(_capi.TfraError) as e:
    _raw(a, more, a.rows(more, 4), {int(x): 9000 for x in more}, 0, 4, None, ev8, None)
  assert e.value.code == -1 and "tfra_table_insert_and_evict" in str(e.value)
  with pytest.raises(_capi.TfraError) as e:
    _raw(a, more, a.rows(more, 4), {int(x): 9000 for x in more}, 2, 4, ek8, ev8, es8)       # an unknown flag bit
  assert e.value.code == -1
  a.same(snap, a.snap(), "a refused call changed the table")
  a.check("refused")


# ---- 6. off max_capacity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["cuckoo", "hkv"])
def test_off_max_capacity_nothing_is_reported(env, flavour):
  """A growing table (no strategy) and an Hkv table below its capacity: the call is the unique upsert, the counter stays 0, the
  table equals a twin written through upsert(unique_keys=True)."""
  torch, de = env
  default = torch.full((DIM,), 0.125)

  def mk(name):
    if flavour == "cuckoo":
      return de.CuckooHashTable(torch.int64, torch.float32, default, device="cuda:0", dim=DIM, init_size=1024, name=name)._table
    return de.HkvHashTable(torch.int64, torch.float32, default, init_capacity=1024, max_capacity=1 << 16, device="cuda:0", dim=DIM,
                           evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, name=name)._table

  a, b = mk("ie_off_a_" + flavour), mk("ie_off_b_" + flavour)
  scored = flavour == "hkv"
  for call in range(3):     # the third call rewrites half of the second's keys
    keys = (np.arange(700, dtype=np.int64) + (0, 700, 1050)[call]) * 7919 + 1
    kt, vt = _kt(torch, keys), _vt(torch, _vals(keys, call + 1))
    sc = _kt(torch, np.arange(keys.size, dtype=np.int64) + 100 * call) if scored else None
    cnt, _, _, _ = a.upsert_and_evict(kt, vt, scores=sc, sync=False)
    b.upsert(kt, vt, scores=sc, unique_keys=True)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0
    ea, eb = _sorted_export(torch, a, with_scores=scored), _sorted_export(torch, b, with_scores=scored)
    for x, y in zip(ea, eb):
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), call
  a.check_errors()
  assert a.size_host() == 1750


# ---- 7. the Python surface -----------------------------------------------------------------------------------------------------------------
def test_hkv_insert_and_evict(env):
  """HkvHashTable.insert_and_evict on an LRU scene (residents in six calls of five): five fresh keys per pair bring back the oldest
  call's residents with their rows."""
  torch = env[0]
  scn = Scene(env, "ie_py_hkv", "LRU", groups=(5,) * 6)
  ages = Ages(scn)
  keys = np.concatenate([scn.fresh[i][:5] for i in range(N_PAIRS)])
  gone = ages.call([], keys, 2)
  k, v, s = scn.t.insert_and_evict(_kt(torch, keys), _vt(torch, scn.rows(keys, 2)))
  torch.cuda.synchronize()
  scn.check("HkvHashTable.insert_and_evict")
  assert k.dtype == torch.int64 and v.shape == (len(gone), DIM) and s.shape == (len(gone),)
  got = _entries(k.cpu().numpy(), v.cpu().numpy(), s.cpu().numpy())
  assert sorted(got) == sorted(gone) == sorted(int(x) for i in range(N_PAIRS) for x in scn.res[i][:5])
  for x in gone:
    assert got[x][0] == scn.rows([x], 1)[0].tobytes()


def _exported(torch, k, v):
  k = k.cpu().numpy().astype(np.int64)
  assert np.unique(k).size == k.size
  return dict(zip(k.tolist(), [r.tobytes() for r in v.cpu().numpy()]))


def test_variable_upsert_and_evict(env):
  """A bounded variable of two shards (both on this GPU): what the call returns is what left either shard — nothing lost, nothing
  twice, every entry with its own row."""
  torch, de = env
  v = de.get_variable("ie_py_var", key_dtype=torch.int64, value_dtype=torch.float32, initializer=0.0, dim=DIM, init_size=CAP,
                      devices=["cuda:0", "cuda:0"],
                      kv_creator=de.HkvHashTableCreator(config=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, max_hbm_for_values=1 << 22,
                                                                                     evict_strategy=de.HkvEvictStrategy.LRU)))
  rows = lambda keys: _vt(torch, _vals(keys, 1))
  old = np.arange(1, 2401, dtype=np.int64) * 104729
  for lo in range(0, old.size, 400):
    v.upsert(_kt(torch, old[lo:lo + 400]), rows(old[lo:lo + 400]))
  before = _exported(torch, *v.export())
  new = np.arange(1, 601, dtype=np.int64) * 15485863 + 5
  ek, ev, es = v.upsert_and_evict(_kt(torch, new), rows(new))
  torch.cuda.synchronize()
  for t in v.tables:
    t._table.check_errors()
  after = _exported(torch, *v.export())
  got = _exported(torch, ek, ev)
  assert ek.device == ev.device == es.device == torch.device("cuda", 0) and es.shape == ek.shape
  assert len(got) > 100, "the shards were not full: nothing to report"
  assert not set(got) & set(after)
  assert set(before) | set(new.tolist()) == set(after) | set(got)
  for x, row in got.items():
    assert row == _vals(np.array([x]), 1)[0].tobytes()
  for x in new.tolist():
    assert after[x] == _vals(np.array([x]), 1)[0].tobytes()


def test_int32_keys_and_the_unsynchronised_form(env):
  """An int32-key table reports int32 keys (as export does).  sync=False: a device count, the untrimmed buffers and no host read;
  the count is the number of entries that left."""
  torch, de = env
  t = de.HkvHashTable(torch.int32, torch.float32, torch.zeros(DIM), init_capacity=CAP, max_capacity=CAP, device="cuda:0", dim=DIM,
                      evict_strategy=de.HkvEvictStrategy.LRU, name="ie_py_i32")._table
  k32 = lambda keys: torch.from_numpy(np.asarray(keys, np.int32)).cuda()
  rows = lambda keys: _vt(torch, _vals(np.asarray(keys, np.int64), 1))
  old = np.arange(1, 1201, dtype=np.int64) * 7919
  for lo in range(0, old.size, 400):
    t.upsert(k32(old[lo:lo + 400]), rows(old[lo:lo + 400]), unique_keys=True)
  for call, sync in enumerate((True, False)):
    before = _exported(torch, *t.export_all()[:2])
    new = np.arange(1, 301, dtype=np.int64) * 10007 + 3 + call
    out = t.upsert_and_evict(k32(new), rows(new), sync=sync)
    torch.cuda.synchronize()
    t.check_errors()
    after = _exported(torch, *t.export_all()[:2])
    left = (set(before) | set(new.tolist())) - set(after)
    assert len(left) > 50
    if sync:
      ek, ev, es = out
      assert ek.dtype == torch.int32 and ek.numel() == len(left)
    else:
      cnt, ek, ev, es = out
      assert cnt.is_cuda and cnt.dtype == torch.int64 and tuple(cnt.shape) == (1,) and ek.numel() == new.size
      assert int(cnt.item()) == len(left)
      ek, ev, es = ek[:len(left)], ev[:len(left)], es[:len(left)]
    got = _exported(torch, ek, ev)
    assert set(got) == left
    for x, row in got.items():
      assert row == _vals(np.array([x]), 1)[0].tobytes()
