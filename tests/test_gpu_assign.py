"""GPU: tfra_table_assign — the write that only hits — and tfra_table_contains.

References are exact: a tensor of the last row written per resident key, the Python set of what was inserted, and for the scores a
twin table that received upsert(hit subset, same rows, same scores, unique_keys=True).  Everything is compared bit for bit."""
import numpy as np
import pytest

from tests.test_gpu_eviction import N_PAIRS, Scene
from tests.test_gpu_find_missed import ABS, GRID, NS, RES, _rows, make_table
from tests.test_gpu_probe_chains import _kt, _sorted_export, _vt

pytestmark = pytest.mark.gpu

EMPTY = -2**63


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _more(count, seed):
  rng = np.random.default_rng(seed)
  u = np.unique(rng.integers(-2**62, 2**62, size=count + 64, dtype=np.int64))
  u = u[~np.isin(u, np.concatenate([RES, ABS]))]
  rng.shuffle(u)
  return u[:count]


RES2 = np.concatenate([RES, _more(700, 21)])      # 2200 resident, 2200 absent: unique batches of up to 4099 keys
ABS2 = np.concatenate([ABS, _more(700, 22)])


def _batch(n, seed):
  """n unique keys, about half of them resident, shuffled -> keys, index into RES2 (-1: absent)"""
  rng = np.random.default_rng(seed)
  h = min(n // 2, RES2.size)
  ri = rng.permutation(RES2.size)[:h]
  keys = np.concatenate([RES2[ri], ABS2[rng.permutation(ABS2.size)[:n - h]]])
  idx = np.concatenate([ri, np.full(n - h, -1)])
  o = rng.permutation(n)
  return keys[o], idx[o]


# ---- 1. hits are written, misses change nothing ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,dim", GRID, ids=["%s-%d" % g for g in GRID])
def test_hits_and_misses(env, dt, dim):
  torch, _ = env
  tbl = make_table(torch, dt, dim, "as_%s_%d" % (dt, dim), resident=RES2)
  rt = _kt(torch, RES2)
  ref = _rows(torch, RES2, dt, dim)
  size, cap, census = tbl.size_host(), tbl.capacity(), tbl.slot_census()
  assert size == RES2.size
  for n in NS:
    keys, idx = _batch(n, n)
    kt = _kt(torch, keys)
    vals = _rows(torch, keys, dt, dim, ver=n)
    hit = torch.from_numpy(idx >= 0).cuda()
    exists = tbl.find(kt, return_exists=True)[1]
    assert torch.equal(tbl.contains(kt), exists) and torch.equal(exists, hit)
    found = tbl.assign(kt, vals, return_found=True)
    assert torch.equal(found, hit), n
    ref[torch.from_numpy(idx[idx >= 0]).cuda()] = vals[hit]
    rows, ex = tbl.find(kt, return_exists=True)
    assert torch.equal(ex, hit), n                                                    # absent keys are still absent
    assert torch.equal(rows[hit].view(torch.uint8), vals[hit].view(torch.uint8)), n
    assert torch.equal(tbl.find(rt).view(torch.uint8), ref.view(torch.uint8)), n    # every other resident row as it was
    tbl.check_errors()
    assert (tbl.size_host(), tbl.capacity(), tbl.slot_census()) == (size, cap, census), n
  assert np.array_equal(np.sort(tbl.export_all()[0].cpu().numpy()), np.sort(RES2))
  assert tbl.assign(kt, vals) is None                                                 # found may be NULL


# ---- 2. a table at max_capacity: nothing is evicted ----------------------------------------------------------------------------------
def test_at_max_capacity_nothing_is_evicted(env):
  torch, _ = env
  scn = Scene(env, "as_scene", "CUSTOMIZED", score=lambda i, r: 10 + r)
  tbl = scn.tbl
  res, fresh = np.concatenate(scn.res), np.concatenate(scn.fresh)
  keys = np.concatenate([res[::2], fresh, scn.by[:7]])          # fresh: absent keys whose home buckets are full of residents
  np.random.default_rng(3).shuffle(keys)
  kt = _kt(torch, keys)
  census, size, cap = tbl.slot_census(), tbl.size_host(), tbl.capacity()
  hit = np.isin(keys, np.concatenate([res, scn.by]))
  assert np.array_equal(tbl.contains(kt).cpu().numpy(), hit)
  sc = 7000 + np.arange(keys.size)
  found = tbl.assign(kt, _vt(torch, scn.rows(keys, 2)), scores=_kt(torch, sc), return_found=True)
  assert np.array_equal(found.cpu().numpy(), hit)
  assert (tbl.slot_census(), tbl.size_host(), tbl.capacity()) == (census, size, cap)
  got, ex = tbl.find(kt, return_exists=True)
  assert np.array_equal(ex.cpu().numpy(), hit)
  np.testing.assert_array_equal(got.cpu().numpy()[hit], scn.rows(keys, 2)[hit])
  for j, k in enumerate(keys.tolist()):
    if k in scn.present:
      scn.present[k] = [scn.rows([k], 2)[0], int(sc[j])]
  # the seven bystanders were written on purpose: put them back, then the scene's conditions hold as a whole
  b = scn.by[:7]
  tbl.assign(_kt(torch, b), _vt(torch, scn.rows(b, 1)), scores=_kt(torch, np.ones(7, np.int64)))
  scn.check("after assign")


# ---- 3. slot vectors stay -------------------------------------------------------------------------------------------------------------
def test_slot_vectors_are_not_written(env):
  torch, _ = env
  tbl = make_table(torch, "float32", 6, "as_aux", resident=RES[:300], aux_fields=2, aux_init=(0.5, 0.25, 0.0, 0.0))
  rt = _kt(torch, RES[:300])
  for f in (1, 2):
    tbl.upsert(rt, _rows(torch, RES[:300], "float32", 6, ver=10 + f), field=f)
  keys = np.concatenate([RES[:200], ABS[:100]])
  found = tbl.assign(_kt(torch, keys), _rows(torch, keys, "float32", 6, ver=3), return_found=True)
  assert found.cpu().numpy().tolist() == [True] * 200 + [False] * 100
  for f in (1, 2):
    assert torch.equal(tbl.find(rt, field=f), _rows(torch, RES[:300], "float32", 6, ver=10 + f))
  assert torch.equal(tbl.find(rt[:200]), _rows(torch, RES[:200], "float32", 6, ver=3))
  assert torch.equal(tbl.find(rt[200:]), _rows(torch, RES[200:300], "float32", 6, ver=1))


# ---- 4. scores: as insert_or_assign touches them on an assign ------------------------------------------------------------------------
def _hkv(env, strategy, name):
  torch, de = env
  return de.HkvHashTable(torch.int64, torch.float32, torch.zeros(8), init_capacity=15 * 89, max_capacity=15 * 89, device="cuda:0", dim=8,
                         evict_strategy=de.HkvEvictStrategy[strategy], step_per_epoch=2, name=name)._table


@pytest.mark.parametrize("strategy", ["CUSTOMIZED", "LFU", "EPOCHLFU"])
def test_scores_match_the_upsert_twin(env, strategy):
  torch, _ = env
  a, b = _hkv(env, strategy, "as_sc_a_" + strategy), _hkv(env, strategy, "as_sc_b_" + strategy)
  res = np.concatenate([RES[:500], [EMPTY]])
  for t in (a, b):
    t.upsert(_kt(torch, res), _rows(torch, res, "float32", 8), scores=_kt(torch, 50 + np.arange(res.size)), unique_keys=True)
  for call in range(4):          # step_per_epoch = 2: the epoch moves under these calls, once per call for both tables
    keys = np.concatenate([res[call * 60:call * 60 + 150], ABS[call * 40:call * 40 + 90], res[-1:]])
    np.random.default_rng(call).shuffle(keys)
    hit = np.isin(keys, res)
    sc = 900 * (call + 1) + np.arange(keys.size)
    vals = _rows(torch, keys, "float32", 8, ver=2 + call)
    found = a.assign(_kt(torch, keys), vals, scores=_kt(torch, sc), return_found=True)
    assert np.array_equal(found.cpu().numpy(), hit)
    ht = torch.from_numpy(hit).cuda()
    b.upsert(_kt(torch, keys[hit]), vals[ht], scores=_kt(torch, sc[hit]), unique_keys=True)
    for x, y in zip(_sorted_export(torch, a, with_scores=True), _sorted_export(torch, b, with_scores=True)):
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), (strategy, call)
  assert a.size_host() == res.size


def test_lru_scores_of_hits_rise(env):
  torch, _ = env
  t = _hkv(env, "LRU", "as_sc_lru")
  t.upsert(_kt(torch, RES[:500]), _rows(torch, RES[:500], "float32", 8), unique_keys=True)
  k0, _, s0 = _sorted_export(torch, t, with_scores=True)
  keys = np.concatenate([RES[:200], ABS[:100]])
  t.assign(_kt(torch, keys), _rows(torch, keys, "float32", 8, ver=2))
  k1, _, s1 = _sorted_export(torch, t, with_scores=True)
  assert torch.equal(k0, k1)
  touched = torch.from_numpy(np.isin(k0.cpu().numpy(), RES[:200])).cuda()
  assert bool((s1[touched] > s0[touched]).all()) and torch.equal(s1[~touched], s0[~touched])


# ---- 5. refusals on a live table -------------------------------------------------------------------------------------------------------
def test_argument_refusals(env):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr
  lib = _capi.lib()
  tbl = make_table(torch, "float32", 4, "as_refuse", resident=RES[:10])
  k, v = _kt(torch, RES[:4]), _rows(torch, RES[:4], "float32", 4)
  e = torch.zeros(4, dtype=torch.uint8, device="cuda")
  c = torch.zeros(1, dtype=torch.int64, device="cuda")
  big = 2**31            # the count is checked before any of these four-entry buffers is read
  cases = [
      ("tfra_table_assign", (tbl._h, 4, None, None, _ptr(v), None, None, None)),
      ("tfra_table_assign", (tbl._h, 4, None, _ptr(k), None, None, None, None)),
      ("tfra_table_assign", (tbl._h, big, None, _ptr(k), _ptr(v), None, None, None)),
      ("tfra_table_contains", (tbl._h, 4, None, None, _ptr(e), None)),
      ("tfra_table_contains", (tbl._h, 4, None, _ptr(k), None, None)),
      ("tfra_table_contains", (tbl._h, big, None, _ptr(k), _ptr(e), None)),
      ("tfra_table_find_missed", (tbl._h, 4, None, None, _ptr(v), None, None, _ptr(v), 0, _ptr(c), 4, None, None, None)),
      ("tfra_table_find_missed", (tbl._h, 4, None, _ptr(k), _ptr(v), None, None, None, 0, _ptr(c), 4, None, None, None)),
      ("tfra_table_find_missed", (tbl._h, big, None, _ptr(k), _ptr(v), None, None, _ptr(v), 0, _ptr(c), 4, None, None, None)),
  ]
  for name, args in cases:
    assert getattr(lib, name)(*args) == -1, name
    assert name in lib.tfra_last_error().decode()
  for name, args in cases:      # n == 0: TFRA_OK, nothing touched
    assert getattr(lib, name)(*((args[0], 0) + args[2:])) == 0
  torch.cuda.synchronize()
  assert int(c.item()) == 0 and tbl.size_host() == 10
  assert torch.equal(tbl.find(k), v)
