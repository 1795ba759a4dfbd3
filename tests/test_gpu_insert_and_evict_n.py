"""GPU: tfra_table_insert_and_evict_n — insert_and_evict with the key count on the device and whole co-located rows in.

The tables are twins of 15 * 89 slots at max_capacity under CUSTOMIZED scores, built like the scene of tests/test_gpu_eviction.py: four
full bucket pairs (crafted keys whose two home buckets are exactly the pair, distinct scores), bystanders that keep the table in the
dense regime and never fill a bucket.  A fresh pair key that scores above every resident replaces the lowest-scoring resident of its
pair, so the victims are determined by the scores, whatever the order in which the keys of a call arrive.  Everything is compared
bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import probe_model as pm
from tests.test_gpu_eviction import CAP, N_PAIRS, SLOTS, _pairs

pytestmark = pytest.mark.gpu

SHAPES = [("float32", 8, 2), ("float16", 20, 1), ("int64", 3, 0)]   # (float16 x 20: a 40-byte field, the 8-byte granule)
IDS = ["f32-8-aux2", "f16-20-aux1", "i64-3-aux0"]
AUX_INIT = (0.5, 0.25, 0.0, 0.0)
_SCENES = {}


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _rows(keys, ver, dt, width):
  """[n, width] rows of dtype dt, a closed-form function of (key, version)"""
  k = np.asarray(keys, np.int64).astype(np.uint64)
  j = np.arange(width, dtype=np.uint64)
  with np.errstate(over="ignore"):
    x = (k[:, None] * np.uint64(2654435761) + j[None, :] * np.uint64(40503) + np.uint64(ver * 7919)) % np.uint64(65521)
  if dt == "int64":
    return x.astype(np.int64) - 30000
  return (x.astype(np.float32) / np.float32(65521.0) - np.float32(0.5)).astype(dt)


def _t(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Twin:
  """One table of the module docstring.  res[i] / fresh[i]: pair i's 30 residents and its further keys; score_of: resident -> score.
  A resident's embedding is version 1 and its slot vector f version 30 + f."""

  def __init__(self, env, name, dt, dim, aux):
    torch, de = env
    self.torch, self.dt, self.dim, self.aux = torch, dt, dim, aux
    tdt = getattr(torch, dt)
    self.t = de.HkvHashTable(torch.int64, tdt, torch.zeros(dim, dtype=tdt), init_capacity=CAP, max_capacity=CAP, device="cuda:0", dim=dim,
                             evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, step_per_epoch=0, aux_fields=aux, aux_init=AUX_INIT, name=name)
    tbl = self.tbl = self.t._table
    nb = self.nb = (tbl.capacity() - 2) // SLOTS
    assert nb * SLOTS <= CAP < 2 * nb * SLOTS          # at max_capacity: it cannot double
    if nb not in _SCENES:
      _SCENES[nb] = pm.pair_scene(nb, _pairs(nb))
    keys, self.by = _SCENES[nb]
    self.res = [k[:30] for k in keys]
    self.fresh = [k[30:] for k in keys]
    perm = [np.random.default_rng(1 + i).permutation(30) for i in range(N_PAIRS)]
    self.score_of = {int(k): 1000 + 3 * int(perm[i][r]) for i in range(N_PAIRS) for r, k in enumerate(self.res[i])}
    for lo in (0, 15):    # the first call fills every pair's b0, the second its b1
      self._put(np.concatenate([r[lo:lo + 15] for r in self.res]))
    tbl.upsert(_t(torch, self.by), _t(torch, _rows(self.by, 1, dt, dim)), scores=_t(torch, np.ones(self.by.size, np.int64)), unique_keys=True)
    torch.cuda.synchronize()
    for _ in range(3):     # the host learns the density from asynchronous size reads: give it calls to complete in
      s = self.by[:16]
      tbl.upsert(_t(torch, s), _t(torch, _rows(s, 1, dt, dim)), scores=_t(torch, np.ones(16, np.int64)), unique_keys=True)
      torch.cuda.synchronize()
    allres = np.concatenate(self.res)
    for f in range(1, aux + 1):
      tbl.upsert(_t(torch, allres), _t(torch, _rows(allres, 30 + f, dt, dim)), field=f)
    if aux:                # (a field insert sets a CUSTOMIZED score to 1: the residents are written again with their scores)
      self._put(allres)
    assert tbl.size_host() == 30 * N_PAIRS + self.by.size > 0.6 * nb * SLOTS

  def _put(self, ks):
    sc = np.array([self.score_of[int(k)] for k in ks], np.int64)
    self.tbl.upsert(_t(self.torch, ks), _t(self.torch, _rows(ks, 1, self.dt, self.dim)), scores=_t(self.torch, sc), unique_keys=True)
    self.torch.cuda.synchronize()

  def whole(self, keys, ver_emb, ver_slot0):
    """whole rows: embedding of version ver_emb, slot vector f of version ver_slot0 + f"""
    return np.concatenate([_rows(keys, ver_emb, self.dt, self.dim)] + [_rows(keys, ver_slot0 + f, self.dt, self.dim) for f in range(1, self.aux + 1)],
                          axis=1)

  def state(self):
    """the whole table sorted by key: keys, embedding rows, scores, slot vectors"""
    torch = self.torch
    k, v, s = self.tbl.export_all(with_scores=True)
    o = torch.argsort(k)
    k, v, s = k[o], v[o], s[o]
    return [k, v, s] + [self.tbl.find(k, field=f) for f in range(1, self.aux + 1)]

  def victims(self, pair, f, gone=()):
    """the f lowest-scoring residents of a pair that are still there"""
    left = [int(k) for k in self.res[pair] if int(k) not in gone]
    return sorted(left, key=lambda k: self.score_of[k])[:f]


def _same(torch, a, b, tag):
  assert len(a) == len(b)
  for x, y in zip(a, b):
    assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), tag


def _triples(torch, out):
  """what a sync=False upsert_and_evict reported -> (count, {key: (row bytes, score)})"""
  cnt, k, v, s = out
  torch.cuda.synchronize()
  n = int(cnt.item())
  assert n <= k.numel()
  k, v, s = k[:n].cpu().numpy(), v[:n].cpu().numpy(), s[:n].cpu().numpy()
  assert np.unique(k).size == n, "a key is reported twice"
  return n, {int(x): (v[i].tobytes(), int(s[i])) for i, x in enumerate(k)}


def _batch(tw, fs, base_score=5000):
  """fs[i] fresh keys of pair i -> keys, scores"""
  keys = np.concatenate([tw.fresh[i][:f] for i, f in enumerate(fs)])
  return keys, base_score + np.arange(keys.size, dtype=np.int64)


POISON_KEY_OFFSET = 30     # the poisoned tail's keys: further fresh pair keys (a pair has 45), which WOULD evict if they were read


def _poisoned(tw, keys, rows, scores, extra):
  """the buffers with `extra` poisoned entries behind them"""
  pk = np.concatenate([tw.fresh[i][POISON_KEY_OFFSET:POISON_KEY_OFFSET + (extra + N_PAIRS - 1) // N_PAIRS] for i in range(N_PAIRS)])[:extra]
  prow = np.full((extra, rows.shape[1]), -77, rows.dtype)
  return (np.concatenate([keys, pk]), np.concatenate([rows, prow]), np.concatenate([scores, np.full(extra, 99999, np.int64)]), pk)


# ---- 1. the count on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,dim,aux", SHAPES, ids=IDS)
def test_counted_call_equals_the_parent(env, dt, dim, aux):
  """Twin a takes insert_and_evict of m keys, twin b the _n call on buffers of n > m entries with d_n = m and poisoned tails: the
  same resident keys, rows, slot vectors and scores, the same reported triples (whole rows), and nothing of the poison anywhere.
  Without TFRA_INSERT_WHOLE_ROWS: the bytes written are the parent's."""
  torch, _ = env
  a, b = Twin(env, "ien_a_" + dt, dt, dim, aux), Twin(env, "ien_b_" + dt, dt, dim, aux)
  _same(torch, a.state(), b.state(), "the twins differ before the call")
  fs = (5, 10, 1, 14)
  keys, scores = _batch(a, fs)
  rows = _rows(keys, 2, dt, dim)
  m = keys.size
  bk, br, bs, pk = _poisoned(b, keys, rows, scores, 37)
  na, ta = _triples(torch, a.tbl.upsert_and_evict(_t(torch, keys), _t(torch, rows), scores=_t(torch, scores), whole_rows=True, sync=False))
  nb_, tb = _triples(torch, b.tbl.upsert_and_evict(_t(torch, bk), _t(torch, br), scores=_t(torch, bs), whole_rows=True, sync=False,
                                                  count=torch.tensor([m], dtype=torch.int64, device="cuda")))
  a.tbl.check_errors()
  b.tbl.check_errors()
  want = sorted(x for i, f in enumerate(fs) for x in a.victims(i, f))
  assert na == nb_ == m and sorted(ta) == sorted(tb) == want
  assert ta == tb
  before = dict(zip(np.concatenate(a.res).tolist(), a.whole(np.concatenate(a.res), 1, 30)))
  for x in want:
    assert tb[x] == (before[x].tobytes(), a.score_of[x])
  sa, sb = a.state(), b.state()
  _same(torch, sa, sb, "the twins differ after the call")
  resident = set(sb[0].tolist())
  assert set(keys.tolist()) <= resident and not (set(pk.tolist()) & (resident | set(tb)))
  assert not bool((sb[1] == -77).any())


@pytest.mark.parametrize("count", [0, -5])
def test_a_zero_or_negative_count_changes_nothing(env, count):
  torch, _ = env
  dt, dim, aux = SHAPES[0]
  b = Twin(env, "ien_zero", dt, dim, aux)
  before = b.state()
  keys, scores = _batch(b, (5, 5, 5, 5))
  out = b.tbl.upsert_and_evict(_t(torch, keys), _t(torch, _rows(keys, 2, dt, dim)), scores=_t(torch, scores), sync=False,
                               count=torch.tensor([count], dtype=torch.int64, device="cuda"))
  n, t = _triples(torch, out)
  assert n == 0 and not t
  b.tbl.check_errors()
  _same(torch, before, b.state(), "a call that serves no key changed the table")


def test_a_count_beyond_the_buffers_serves_the_buffers(env):
  torch, _ = env
  dt, dim, aux = SHAPES[0]
  a, b = Twin(env, "ien_over_a", dt, dim, aux), Twin(env, "ien_over_b", dt, dim, aux)
  keys, scores = _batch(a, (3, 0, 17, 9))
  rows = _rows(keys, 2, dt, dim)
  na, ta = _triples(torch, a.tbl.upsert_and_evict(_t(torch, keys), _t(torch, rows), scores=_t(torch, scores), sync=False))
  nb_, tb = _triples(torch, b.tbl.upsert_and_evict(_t(torch, keys), _t(torch, rows), scores=_t(torch, scores), sync=False,
                                                  count=torch.tensor([keys.size + 100], dtype=torch.int64, device="cuda")))
  assert na == nb_ == keys.size and ta == tb
  _same(torch, a.state(), b.state(), "d_n > n")


# ---- 2. whole rows in ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,dim,aux", SHAPES, ids=IDS)
def test_whole_rows_in(env, dt, dim, aux):
  """One call with keys of every kind: fresh keys that replace a victim, fresh keys that take an empty slot (two residents of pair 0
  are erased first), residents, and one fresh key that scores below its pair's minimum and is not admitted.  Every admitted key
  holds the caller's embedding AND slot vectors; the victims come back with the whole rows they held; the refused key comes back
  with the caller's whole row and its score."""
  torch, _ = env
  b = Twin(env, "ien_whole_" + dt, dt, dim, aux)
  tbl = b.tbl
  order0 = sorted((int(k) for k in b.res[0]), key=lambda k: b.score_of[k])
  erased = order0[10:12]                                   # neither among the lowest nor among the highest
  tbl.erase(_t(torch, np.array(erased, np.int64)))
  fs = (5, 4, 0, 7)
  fresh, fscores = _batch(b, fs)
  stay = np.array([sorted((int(k) for k in b.res[i]), key=lambda k: b.score_of[k])[-1] for i in range(N_PAIRS)], np.int64)   # each pair's top scorer
  refused = b.fresh[2][:1]                                 # pair 2 takes no other fresh key: its minimum is 1000
  keys = np.concatenate([fresh, stay, refused])
  scores = np.concatenate([fscores, np.array([b.score_of[int(k)] + 1 for k in stay], np.int64), np.array([999], np.int64)])
  rows = b.whole(keys, 2, 40)
  assert rows.shape[1] == dim * (1 + aux)
  out = tbl.upsert_and_evict(_t(torch, keys), _t(torch, rows), scores=_t(torch, scores), whole_rows=True, whole_rows_in=True, sync=False)
  n, got = _triples(torch, out)
  tbl.check_errors()
  # pair 0: two of its five fresh keys take the erased slots, three replace a victim
  want = b.victims(0, 3, gone=erased) + b.victims(1, 4) + b.victims(3, 7)
  assert n == len(want) + 1 and sorted(got) == sorted(want + [int(refused[0])])
  allres = np.concatenate(b.res)
  before = dict(zip(allres.tolist(), b.whole(allres, 1, 30)))
  for x in want:
    assert got[x] == (before[x].tobytes(), b.score_of[x]), "a victim did not come back with the whole row it held"
  assert got[int(refused[0])] == (rows[-1].tobytes(), 999), "the refused key did not come back with the caller's whole row"
  # the table: every admitted key of the call with the caller's fields and score
  admitted = keys[:-1]
  kt = _t(torch, admitted)
  assert bool(tbl.contains(kt).all()) and not bool(tbl.contains(_t(torch, refused)).any())
  assert not bool(tbl.contains(_t(torch, np.array(want, np.int64))).any())
  for f in range(aux + 1):
    got_f = tbl.find(kt, field=f).cpu().numpy()
    assert got_f.tobytes() == np.ascontiguousarray(rows[:-1, f * dim:(f + 1) * dim]).tobytes(), "field %d is not the caller's" % f
  k, _, s = tbl.export_all(with_scores=True)
  sc = dict(zip(k.tolist(), s.tolist()))
  assert [sc[int(x)] for x in admitted] == scores[:-1].tolist()
  # everything else is as it was
  others = np.array([x for x in allres.tolist() if x not in set(want) | set(erased) | set(stay.tolist())], np.int64)
  for f in range(aux + 1):
    ver = 1 if f == 0 else 30 + f
    assert tbl.find(_t(torch, others), field=f).cpu().numpy().tobytes() == _rows(others, ver, dt, dim).tobytes()
  assert tbl.size_host() == 30 * N_PAIRS + b.by.size


# ---- 3. refusals, and a table that is not at max_capacity -------------------------------------------------------------------------
def test_off_max_capacity_the_counter_is_untouched(env):
  """A bounded table that can still grow displaces nothing: the keys are inserted (whole rows: with the caller's slot vectors), the
  counter keeps the value the caller left in it and the output buffers are not written."""
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  dim, aux = 8, 2
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=1024, max_capacity=1 << 20, device="cuda:0", dim=dim,
                      evict_strategy=de.HkvEvictStrategy.LRU, aux_fields=aux, aux_init=AUX_INIT, name="ien_growing")
  tbl = t._table
  n, m = 500, 300
  keys = np.arange(1, n + 1, dtype=np.int64) * 7919
  rows = np.concatenate([_rows(keys, 2, "float32", dim)] + [_rows(keys, 40 + f, "float32", dim) for f in (1, 2)], axis=1)
  counter = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
  ek = torch.full((n,), -7, dtype=torch.int64, device="cuda")
  ev = torch.full((n, dim * 3), -7.0, device="cuda")
  kt, vt = _t(torch, keys), _t(torch, rows)
  cnt = torch.tensor([m], dtype=torch.int64, device="cuda")
  _capi.call("tfra_table_insert_and_evict_n", tbl._h, n, _ptr(cnt), _ptr(kt), _ptr(vt), None, _capi.EVICT_WHOLE_ROWS | _capi.INSERT_WHOLE_ROWS,
             _ptr(counter), n, _ptr(ek), _ptr(ev), None, _stream(tbl.device))
  torch.cuda.synchronize()
  tbl.check_errors()
  assert int(counter.item()) == 12345 and bool((ek == -7).all()) and bool((ev == -7).all())
  assert tbl.size_host() == m
  ex = tbl.contains(kt)
  assert bool(ex[:m].all()) and not bool(ex[m:].any())
  for f in range(aux + 1):
    assert tbl.find(kt[:m], field=f).cpu().numpy().tobytes() == np.ascontiguousarray(rows[:m, f * dim:(f + 1) * dim]).tobytes()


def test_refusals_name_the_function(env):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  dt, dim, aux = SHAPES[0]
  b = Twin(env, "ien_refuse", dt, dim, aux)
  before = b.state()
  keys, scores = _batch(b, (2, 2, 2, 2))
  kt, vt = _t(torch, keys), _t(torch, _rows(keys, 2, dt, dim))
  counter = torch.zeros(1, dtype=torch.int64, device="cuda")
  ev = torch.empty((keys.size, dim), device="cuda")
  s = _stream(b.tbl.device)
  lib = _capi.lib()
  cases = [
      (b.tbl._h, keys.size, None, _ptr(kt), _ptr(vt), None, 4, _ptr(counter), 0, None, None, None, s),              # an unknown flag bit
      (b.tbl._h, keys.size, None, None, _ptr(vt), None, 0, _ptr(counter), 0, None, None, None, s),                  # no keys
      (b.tbl._h, keys.size, None, _ptr(kt), _ptr(vt), None, 0, None, 0, None, None, None, s),                       # no counter
      (b.tbl._h, keys.size, None, _ptr(kt), _ptr(vt), None, 0, _ptr(counter), 0, None, _ptr(ev), None, s),          # rows without keys
      (b.tbl._h, 1 << 31, None, _ptr(kt), _ptr(vt), None, 0, _ptr(counter), 0, None, None, None, s),                # too many keys
  ]
  for args in cases:
    assert lib.tfra_table_insert_and_evict_n(*args) == -1
    assert "tfra_table_insert_and_evict_n" in lib.tfra_last_error().decode()
  torch.cuda.synchronize()
  assert int(counter.item()) == 0
  _same(torch, before, b.state(), "a refused call changed the table")
