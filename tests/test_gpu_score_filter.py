"""GPU: score-filtered export, count, erase and save (tfra_table_export_batch_if / _erase_if / _save_if and their Python forms).

The yardstick of every case is code that predates them: `export_all(with_scores=True)` taken before the call, filtered in NumPy on
the scores as uint64, compared as sets of (key, score, row bytes) — sorted by key, rows bit for bit.  CUSTOMIZED tables are filled
through `upsert(keys, values, scores=...)` with scores the test chooses: a small range (so every threshold meets ties) plus a few
scores above 2^63 (an int64 compare would order them below everything).  Tables: 1024 slots (68 buckets: one 64-bucket block and
a tail) and 3000 slots (200 buckets), filled to at most half; the sequential placement model (tests/probe_model.py) confirms per
table that every key finds a slot within the four buckets a bounded table may use, so nothing evicts."""
import ctypes
import os

import numpy as np
import pytest

from tests import probe_model as pm

pytestmark = pytest.mark.gpu

SLOTS = 15
I64_MIN = -2**63
RESERVED = np.array([I64_MIN, I64_MIN + 1], np.int64)
HIGH = 2**63            # scores from here up are negative as int64
GE, LT = 0, 1


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _nb(tbl):
  return (tbl.capacity() - 2) // SLOTS


def _np_dt(torch, dt):
  return {torch.float32: np.float32, torch.float16: np.float16, torch.int8: np.int8}[dt]


def _rows(torch, keys, dim, dt, ver=1):
  """rows that are a closed-form function of (key, version), in the table's dtype"""
  k = np.asarray(keys, np.int64).astype(np.uint64)
  j = np.arange(dim, dtype=np.uint64)
  with np.errstate(over="ignore"):
    x = (k[:, None] * np.uint64(2654435761) + j[None, :] * np.uint64(40503) + np.uint64(ver * 7919)) % np.uint64(65521)
  if dt == torch.int8:
    return (x % np.uint64(251)).astype(np.int64).astype(np.int8)
  return (x.astype(np.float32) / np.float32(65521.0) - np.float32(0.5)).astype(_np_dt(torch, dt))


def _scores(rng, n):
  """uint64 scores: 10..59 with many ties, both ends present, four above 2^63"""
  s = rng.integers(10, 60, size=n).astype(np.uint64)
  s[0], s[1] = 10, 59
  s[2:6] = np.uint64(HIGH) + np.arange(4, dtype=np.uint64)
  return s


def _t(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _st(torch, s):
  return _t(torch, np.asarray(s, np.uint64).view(np.int64))


def _fits(nb, keys):
  """the sequential model places every key within b0, b1, b1 + 1, b1 + 2: a bounded table takes it without evicting"""
  m = pm.FirstFit(nb)
  for k in keys:
    m.insert(k)
  return max(m.depth_of(k) for k in keys) <= 3


def _hkv(env, name, dt, dim, slots, strategy="CUSTOMIZED", aux=0, key_dtype=None):
  torch, de = env
  return de.HkvHashTable(key_dtype or torch.int64, dt, torch.zeros(dim, dtype=dt), init_capacity=slots, max_capacity=slots,
                         device="cuda:0", dim=dim, evict_strategy=getattr(de.HkvEvictStrategy, strategy), aux_fields=aux, name=name)


def _filled(env, name, dt, dim, slots, n, seed, reserved=True, aux=0):
  """a CUSTOMIZED table of `slots` slots holding n random keys (+ the two reserved keys) -> (HkvHashTable, keys, uint64 scores)"""
  torch, _ = env
  t = _hkv(env, name, dt, dim, slots, aux=aux)
  tbl = t._table
  rng = np.random.default_rng(seed)
  keys = np.unique(rng.integers(-2**62, 2**62, size=n + 8, dtype=np.int64))[:n]
  rng.shuffle(keys)
  assert keys.size == n and n * 2 <= _nb(tbl) * SLOTS and _fits(_nb(tbl), keys)
  sc = _scores(rng, n)
  tbl.upsert(_t(torch, keys), _t(torch, _rows(torch, keys, dim, dt)), scores=_st(torch, sc), unique_keys=True)
  if reserved:
    tbl.upsert(_t(torch, RESERVED), _t(torch, _rows(torch, RESERVED, dim, dt)), scores=_st(torch, [20, 30]), unique_keys=True)
  tbl.check_errors()
  assert tbl.size_host() == n + (2 if reserved else 0)
  return t, keys, sc


def _snap(tbl, field=0):
  """the whole table through the existing export: keys, rows as bytes, scores as uint64, sorted by key"""
  import torch
  k, v, s = tbl.export_all(with_scores=True)
  if field:
    v = tbl.find(k, field=field)
  o = np.argsort(k.cpu().numpy(), kind="stable")
  k, s = k.cpu().numpy()[o], s.cpu().numpy().view(np.uint64)[o]
  v = v.contiguous().view(torch.uint8).cpu().numpy()[o]
  assert np.unique(k).size == k.size
  return k, v, s


def _mask(s, thr, pred):
  return s >= np.uint64(thr) if pred in ("ge", GE) else s < np.uint64(thr)


def _want(snap, thr, pred):
  k, v, s = snap
  m = _mask(s, thr, pred)
  return k[m], v[m], s[m]


def _sorted(torch, k, v, s):
  k = k.cpu().numpy()
  o = np.argsort(k, kind="stable")
  v = None if v is None else v.contiguous().view(torch.uint8).cpu().numpy()[o]
  s = None if s is None else s.cpu().numpy().view(np.uint64)[o]
  return k[o], v, s


def _same(got, want, tag=""):
  for g, w, what in zip(got, want, ("keys", "rows", "scores")):
    if g is not None:
      np.testing.assert_array_equal(g, w, err_msg="%s %s" % (tag, what))


def _thresholds(s):
  """0, the minimum, a tied middle score, the maximum, the maximum + 1 of the resident non-reserved scores, and 2^64 - 1"""
  real = s[s != np.uint64(2**64 - 1)]
  mid = int(np.sort(real)[real.size // 2])
  assert (real == np.uint64(mid)).sum() > 1
  return [0, int(real.min()), mid, int(real.max()), int(real.max()) + 1, 2**64 - 1]


def _raw_export(env, tbl, pred, thr, n, offset, cap, nbuf, values=True, scores=True, count_only=False, guard=0):
  """tfra_table_export_batch_if into buffers of nbuf entries pre-filled with a guard pattern -> (count, keys, rows, scores)"""
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  counter = torch.zeros(1, dtype=torch.int64, device="cuda")
  k = torch.full((nbuf,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
  v = torch.full((nbuf, tbl.dim * tbl._default_value.element_size()), 0xA5, dtype=torch.uint8, device="cuda") if values else None
  s = torch.full((nbuf,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda") if scores else None
  if count_only:
    _capi.call("tfra_table_export_batch_if", tbl._h, pred, thr, n, offset, _ptr(counter), cap, None, None, None, _stream(tbl.device))
  else:
    _capi.call("tfra_table_export_batch_if", tbl._h, pred, thr, n, offset, _ptr(counter), cap, _ptr(k), _ptr(v), _ptr(s),
               _stream(tbl.device))
  return int(counter.item()), k, v, s


def _untouched(k, v, s, start):
  assert bool((k[start:] == 0x5A5A5A5A5A5A5A5A).all())
  if v is not None:
    assert bool((v[start:] == 0xA5).all())
  if s is not None:
    assert bool((s[start:] == 0x3C3C3C3C3C3C3C3C).all())


# ---- 1. thresholds and predicates, per value type ------------------------------------------------------------------------------------
CASES = [("float32", 4, 1024, 500), ("float32", 64, 3000, 1400), ("float16", 128, 1024, 480), ("int8", 3, 3000, 1300)]
_RO = {}


def _ro(env, case):
  """one read-only table per case, its snapshot taken once"""
  if case not in _RO:
    torch, _ = env
    dt, dim, slots, n = case
    t, keys, sc = _filled(env, "sf_%s_%d" % (dt, dim), getattr(torch, dt), dim, slots, n, seed=CASES.index(case) + 1)
    _RO[case] = (t, _snap(t._table))
  return _RO[case]


@pytest.mark.parametrize("case", CASES, ids=["%s-d%d-%d" % c[:3] for c in CASES])
def test_thresholds_and_predicates(env, case):
  torch, _ = env
  t, snap = _ro(env, case)
  tbl = t._table
  assert _nb(tbl) == case[2] // SLOTS and _nb(tbl) > 64
  for thr in _thresholds(snap[2]):
    for pred in ("ge", "lt"):
      want = _want(snap, thr, pred)
      tag = "%s %d" % (pred, thr)
      c = tbl.count_if(thr, pred)
      assert tuple(c.shape) == (1,) and c.dtype == torch.int64 and c.is_cuda and int(c.item()) == want[0].size, tag
      k, v, s = tbl.export_if(thr, pred)
      assert v.dtype == getattr(torch, case[0]) and tuple(v.shape) == (want[0].size, case[1])
      _same(_sorted(torch, k, v, s), want, tag)
      k, v, s = tbl.export_if(thr, pred, with_scores=False, values=False)
      assert v is None and s is None
      _same(_sorted(torch, k, None, None), want, tag + " keys only")
  # the reserved keys: under every GE, under no LT
  for thr in (0, 59, 2**64 - 1):
    ge = tbl.export_if(thr, "ge")[0].cpu().numpy()
    lt = tbl.export_if(thr, "lt")[0].cpu().numpy()
    assert np.isin(RESERVED, ge).all() and not np.isin(RESERVED, lt).any(), thr
  assert int(tbl.count_if(2**64 - 1, "ge").item()) == 2
  _same(_snap(tbl), snap, "the table is unchanged")


# ---- 2. windows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=["float32-d4-1024", "int8-d3-3000"])
def test_windows(env, case):
  torch, _ = env
  t, snap = _ro(env, case)
  tbl = t._table
  cap = tbl.capacity()
  nb = _nb(tbl)
  assert cap == nb * SLOTS + 2
  thr = _thresholds(snap[2])[2]
  for pred in (GE, LT):
    want = _want(snap, thr, pred)
    # disjoint windows that begin and end inside buckets, the last one holding the two reserved slots
    cuts = [0, 7, 7, 100, 64 * SLOTS - 3, 64 * SLOTS + 8, nb * SLOTS - 1, nb * SLOTS + 1, cap]
    parts, total = [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
      c, k, v, s = _raw_export(env, tbl, pred, thr, b - a, a, b - a, max(b - a, 1))
      assert c <= b - a
      _untouched(k, v, s, c)
      parts.append((k[:c], v[:c], s[:c]))
      total += c
    assert total == want[0].size
    got = _sorted(torch, torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]))
    _same(got, want, "union of windows, pred %d" % pred)
    # only the reserved slots; then windows that are empty or lie past the end
    c, k, v, s = _raw_export(env, tbl, pred, thr, 2, nb * SLOTS, 2, 2)
    assert c == (2 if pred == GE else 0)
    if c:
      assert sorted(k.cpu().numpy().tolist()) == RESERVED.tolist() and bool((s == -1).all())
    for n, off in ((0, 5), (10, cap), (10, cap + 100)):
      c, k, v, s = _raw_export(env, tbl, pred, thr, n, off, 10, 10)
      assert c == 0
      _untouched(k, v, s, 0)
    # a window far longer than the table is the whole table
    c, k, v, s = _raw_export(env, tbl, pred, thr, cap * 3, 0, cap, cap)
    _same(_sorted(torch, k[:c], v[:c], s[:c]), want, "long window")


# ---- 3. the cap ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=["float32-d4-1024", "float32-d64-3000"])
def test_cap(env, case):
  torch, _ = env
  t, snap = _ro(env, case)
  tbl = t._table
  cap = tbl.capacity()
  thr = _thresholds(snap[2])[2]
  want = _want(snap, thr, GE)
  m = want[0].size
  assert m > 100
  # count only: the count, nothing written (cap is ignored)
  for c_arg in (0, 5, m):
    c, k, v, s = _raw_export(env, tbl, GE, thr, cap, 0, c_arg, 4, count_only=True)
    assert c == m
    _untouched(k, v, s, 0)
  # cap == matches: everything
  c, k, v, s = _raw_export(env, tbl, GE, thr, cap, 0, m, m + 16)
  assert c == m
  _untouched(k, v, s, m)
  _same(_sorted(torch, k[:m], v[:m], s[:m]), want, "cap == matches")
  # cap == matches - 1: the counter still says matches; exactly cap entries, all of them matches; nothing behind cap
  c, k, v, s = _raw_export(env, tbl, GE, thr, cap, 0, m - 1, m + 16)
  assert c == m
  _untouched(k, v, s, m - 1)
  gk, gv, gs = _sorted(torch, k[:m - 1], v[:m - 1], s[:m - 1])
  assert np.unique(gk).size == m - 1
  at = np.minimum(np.searchsorted(want[0], gk), m - 1)
  np.testing.assert_array_equal(want[0][at], gk)
  np.testing.assert_array_equal(want[1][at], gv)
  np.testing.assert_array_equal(want[2][at], gs)
  # a cap that cuts inside a block's run, and one without values / scores
  c, k, v, s = _raw_export(env, tbl, GE, thr, cap, 0, 37, m + 16, values=False, scores=False)
  assert c == m and bool(np.isin(k[:37].cpu().numpy(), want[0]).all()) and np.unique(k[:37].cpu().numpy()).size == 37
  _untouched(k, None, None, 37)
  # cap == 0 with buffers given: nothing
  c, k, v, s = _raw_export(env, tbl, GE, thr, cap, 0, 0, 8)
  assert c == m
  _untouched(k, v, s, 0)


# ---- 4. erase ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots,n", [(1024, 500), (3000, 1400)])
def test_erase_if(env, slots, n):
  torch, _ = env
  dt, dim = torch.float32, 4
  t, keys, sc = _filled(env, "sf_erase_%d" % slots, dt, dim, slots, n, seed=7)
  tbl = t._table
  snap = _snap(tbl)
  thr = _thresholds(snap[2])[2]
  gone = _want(snap, thr, "lt")
  stay = _want(snap, thr, "ge")
  assert gone[0].size > 50 and stay[0].size > 50 and np.isin(RESERVED, stay[0]).all()
  size = tbl.size_host()
  e = tbl.erase_if(thr, "lt")
  assert tuple(e.shape) == (1,) and e.dtype == torch.int64 and int(e.item()) == gone[0].size
  assert tbl.size_host() == size - gone[0].size
  _, ex = tbl.find(_t(torch, gone[0]), return_exists=True)
  assert not bool(ex.any())
  rows, ex = tbl.find(_t(torch, stay[0]), return_exists=True)
  assert bool(ex.all())
  np.testing.assert_array_equal(rows.contiguous().view(torch.uint8).reshape(stay[0].size, -1).cpu().numpy(), stay[1])
  _same(_snap(tbl), stay, "survivors")
  c = tbl.slot_census()
  assert c["live"] == stay[0].size - 2 and c["locked"] == 0
  assert int(tbl.erase_if(thr, "lt").item()) == 0                # a second identical call
  assert tbl.size_host() == stay[0].size
  # an erased key comes back with the score of its new upsert
  back = gone[0][:40]
  tbl.upsert(_t(torch, back), _t(torch, _rows(torch, back, dim, dt, ver=2)), scores=_st(torch, np.full(40, 5, np.uint64)), unique_keys=True)
  tbl.check_errors()
  k, v, s = _sorted(torch, *tbl.export_if(thr, "lt"))
  np.testing.assert_array_equal(k, np.sort(back))
  assert bool((s == np.uint64(5)).all())
  np.testing.assert_array_equal(v, _rows(torch, np.sort(back), dim, dt, ver=2).view(np.uint8).reshape(40, -1))
  assert tbl.size_host() == stay[0].size + 40
  # the reserved keys stay under every LT, and go — with everything else — under GE 0
  assert int(tbl.erase_if(2**64 - 1, "lt").item()) == stay[0].size + 40 - 2
  assert sorted(tbl.export_all()[0].cpu().numpy().tolist()) == RESERVED.tolist() and tbl.size_host() == 2
  tbl.upsert(_t(torch, keys[:100]), _t(torch, _rows(torch, keys[:100], dim, dt)), scores=_st(torch, sc[:100]), unique_keys=True)
  assert int(tbl.erase_if(0, "ge").item()) == 102
  assert tbl.size_host() == 0 and int(tbl.count_if(0, "ge").item()) == 0
  c = tbl.slot_census()
  assert c["live"] == 0 and c["locked"] == 0
  _, ex = tbl.find(_t(torch, np.concatenate([RESERVED, keys[:100]])), return_exists=True)
  assert not bool(ex.any())
  # erase_if without a counter (the C call takes NULL)
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _stream
  tbl.upsert(_t(torch, keys[:30]), _t(torch, _rows(torch, keys[:30], dim, dt)), scores=_st(torch, sc[:30]), unique_keys=True)
  _capi.call("tfra_table_erase_if", tbl._h, GE, 0, None, _stream(tbl.device))
  assert tbl.size_host() == 0


def test_erase_if_on_overflow_chains(env):
  """A scored table below max_capacity (it places keys first-fit along the whole probe sequence) with the crafted chains of
  tests/test_gpu_probe_chains.py: a chain 11 buckets deep that wraps over the last bucket, a pile on the last bucket.  erase_if
  empties chain buckets 0 and 2 and a scattering of other slots; every survivor behind a hole is still found."""
  torch, de = env
  from tests.test_gpu_probe_chains import Scn, N_CHAIN
  dim = 8
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=600, max_capacity=SLOTS * 89 * 16, device="cuda:0",
                      dim=dim, evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, name="sf_chains")
  tbl = t._table
  scn = Scn(_nb(tbl), "wrap")
  model = pm.FirstFit(scn.nb)
  score = {}
  rng = np.random.default_rng(5)
  low = set(scn.chain[0:15].tolist()) | set(scn.chain[30:45].tolist()) | set(scn.pile[::3].tolist()) | set(scn.by[::4].tolist())
  for b in scn.batches():
    sc = np.array([rng.integers(1, 50) if int(k) in low else rng.integers(50, 100) for k in b], np.uint64)
    tbl.upsert(_t(torch, b), _t(torch, _rows(torch, b, dim, torch.float32)), scores=_st(torch, sc), unique_keys=True)
    score.update({int(k): int(s) for k, s in zip(b, sc)})
    for k in b:
      model.insert(k)
  c = tbl.slot_census()
  assert tbl.growth_stats()["growths"] == 0 and c["ovf1"] >= 9 and c["live"] == len(score), c
  assert {model.bucket_of(k) for k in scn.chain[0:15]} == {scn.chain_buckets[0]}
  assert {model.bucket_of(k) for k in scn.chain[30:45]} == {scn.chain_buckets[2]}
  assert max(model.depth_of(k) for k in scn.chain) == 10
  snap = _snap(tbl)
  np.testing.assert_array_equal(snap[2], np.array([score[int(k)] for k in snap[0]], np.uint64))
  gone, stay = _want(snap, 50, "lt"), _want(snap, 50, "ge")
  assert sorted(gone[0].tolist()) == sorted(low)
  assert int(tbl.erase_if(50, "lt").item()) == len(low)
  assert tbl.size_host() == stay[0].size
  everything = np.concatenate([scn.resident(), scn.absent])
  rows, ex = tbl.find(_t(torch, everything), return_exists=True)
  np.testing.assert_array_equal(ex.cpu().numpy(), np.isin(everything, stay[0]))
  deep = scn.chain[75:N_CHAIN]                      # chain buckets 5..10, behind both holes
  assert np.isin(deep, stay[0]).all() and min(model.depth_of(k) for k in deep) == 5
  got = tbl.find(_t(torch, deep))
  np.testing.assert_array_equal(got.cpu().numpy(), _rows(torch, deep, dim, torch.float32))
  _same(_snap(tbl), stay, "survivors on chains")
  after = tbl.slot_census()
  assert (after["ovf0"], after["ovf1"]) == (c["ovf0"], c["ovf1"]) and after["live"] == stay[0].size and after["locked"] == 0
  # the holes are refilled by new keys of the pair before the chain grows
  tbl.upsert(_t(torch, scn.extra), _t(torch, _rows(torch, scn.extra, dim, torch.float32)), scores=_st(torch, np.full(scn.extra.size, 7, np.uint64)),
             unique_keys=True)
  assert tbl.slot_census()["ovf1"] == c["ovf1"]
  k, _, s = _sorted(torch, *tbl.export_if(50, "lt"))
  np.testing.assert_array_equal(k, np.sort(scn.extra))
  assert tbl.growth_stats()["growths"] == 0


# ---- 5. LRU and EPOCHLRU: the filter is the NumPy filter of the full export, whatever the clock says ---------------------------------
@pytest.mark.parametrize("strategy", ["LRU", "EPOCHLRU"])
def test_clock_scores(env, strategy):
  torch, _ = env
  from tfra_amd import _capi
  dim = 4
  t = _hkv(env, "sf_" + strategy, torch.float32, dim, 3000, strategy=strategy)
  tbl = t._table
  rng = np.random.default_rng(9)
  keys = np.unique(rng.integers(-2**62, 2**62, size=1208, dtype=np.int64))[:1200]
  rng.shuffle(keys)
  assert _fits(_nb(tbl), keys)
  a, b = keys[:700], keys[500:]                      # 200 keys of A are touched again by B
  if strategy == "EPOCHLRU":
    _capi.call("tfra_table_set_global_epoch", tbl._h, 3)
  t.insert(_t(torch, a), _t(torch, _rows(torch, a, dim, torch.float32)))
  after_a = _snap(tbl)
  boundary = int(after_a[2].max()) + 1
  if strategy == "EPOCHLRU":
    _capi.call("tfra_table_set_global_epoch", tbl._h, 4)
    boundary = 4 << 32
  t.insert(_t(torch, b), _t(torch, _rows(torch, b, dim, torch.float32, ver=2)))
  tbl.check_errors()
  snap = _snap(tbl)
  assert snap[0].size == 1200
  for thr in (boundary, int(snap[2].min()), int(np.sort(snap[2])[600])):
    for pred in ("ge", "lt"):
      want = _want(snap, thr, pred)
      assert int(t.size_if(thr, pred).item()) == want[0].size
      _same(_sorted(torch, *t.export_if(thr, pred)), want, "%s %s %d" % (strategy, pred, thr))
  # expiry: what the filter calls older than the boundary goes, the rest stays as it is
  stay = _want(snap, boundary, "ge")
  assert int(t.remove_if(boundary, "lt").item()) == 1200 - stay[0].size
  _same(_snap(tbl), stay, strategy + " after expiry")


# ---- 6. co-located state fields ------------------------------------------------------------------------------------------------------
def test_aux_fields(env, tmp_path):
  torch, _ = env
  dt, dim = torch.float32, 8
  t, keys, sc = _filled(env, "sf_aux", dt, dim, 1024, 400, seed=11, reserved=False, aux=2)
  tbl = t._table
  for f in (1, 2):
    tbl.upsert(_t(torch, keys), _t(torch, _rows(torch, keys, dim, dt, ver=20 + f)), field=f)
  tbl.upsert(_t(torch, keys), _t(torch, _rows(torch, keys, dim, dt)), scores=_st(torch, sc), unique_keys=True)   # the scores once more
  tbl.check_errors()
  snap = [_snap(tbl, field=f) for f in range(3)]
  np.testing.assert_array_equal(snap[0][2], np.asarray(sc, np.uint64)[np.argsort(keys)])
  thr = _thresholds(snap[0][2])[2]
  # save_if(field=1): the matching keys with field 1's bytes
  prefix = str(tmp_path / "aux1")
  want = _want(snap[1], thr, "ge")
  assert tbl.save_if(prefix, thr, "ge", field=1) == want[0].size
  fk = np.fromfile(prefix + "-keys", dtype=np.int64)
  fv = np.fromfile(prefix + "-values", dtype=np.uint8).reshape(fk.size, -1)
  o = np.argsort(fk)
  np.testing.assert_array_equal(fk[o], want[0])
  np.testing.assert_array_equal(fv[o], want[1])
  assert not np.array_equal(want[1], _want(snap[0], thr, "ge")[1])
  assert not os.path.exists(prefix + "-scores")
  # erase_if takes the slot with the row: every field misses
  gone = _want(snap[0], thr, "lt")[0]
  assert int(tbl.erase_if(thr, "lt").item()) == gone.size
  for f in range(3):
    _, ex = tbl.find(_t(torch, gone), return_exists=True, field=f)
    assert not bool(ex.any()), f
    _same(_snap(tbl, field=f), _want(snap[f], thr, "ge"), "field %d survivors" % f)


# ---- 7. save and load ----------------------------------------------------------------------------------------------------------------
def _read_kv(prefix, key_np=np.int64):
  k = np.fromfile(prefix + "-keys", dtype=key_np)
  v = np.fromfile(prefix + "-values", dtype=np.uint8).reshape(k.size, -1) if k.size else np.zeros((0, 0), np.uint8)
  o = np.argsort(k, kind="stable")
  return k[o], v[o]


@pytest.mark.parametrize("key_dtype", ["int64", "int32"])
def test_save_if_and_load_over_a_base(env, tmp_path, key_dtype):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  dt, dim = torch.float32, 4
  kdt = getattr(torch, key_dtype)
  knp = np.int32 if key_dtype == "int32" else np.int64
  t = _hkv(env, "sf_save_" + key_dtype, dt, dim, 1024, key_dtype=kdt)
  tbl = t._table
  rng = np.random.default_rng(13)
  if key_dtype == "int32":
    keys = np.unique(rng.integers(-2**31, 2**31, size=508, dtype=np.int64))[:500]
  else:
    keys = np.concatenate([np.unique(rng.integers(-2**62, 2**62, size=506, dtype=np.int64))[:498], RESERVED])
  rng.shuffle(keys)
  assert _fits(_nb(tbl), keys[keys > I64_MIN + 1])
  sc = _scores(rng, keys.size)
  tbl.upsert(_t(torch, keys.astype(knp)), _t(torch, _rows(torch, keys, dim, dt, ver=2)), scores=_st(torch, sc), unique_keys=True)
  tbl.check_errors()
  snap = _snap(tbl)
  assert snap[0].size == 500
  thr = _thresholds(snap[2])[2]
  want = _want(snap, thr, "ge")
  rest = _want(snap, thr, "lt")
  assert 50 < want[0].size < 450
  # many windows (7 slots each) and one window: the same entries on disk
  p7, p1 = str(tmp_path / "delta7"), str(tmp_path / "delta1")
  assert tbl.save_if(p7, thr, "ge", buffer_size=7) == want[0].size
  assert tbl.save_if(p1, thr, "ge") == want[0].size
  assert os.path.getsize(p1 + "-keys") == want[0].size * np.dtype(knp).itemsize
  for p in (p7, p1):
    fk, fv = _read_kv(p, knp)
    np.testing.assert_array_equal(fk, want[0])
    np.testing.assert_array_equal(fv, want[1])
    assert not os.path.exists(p + "-scores") and not os.path.exists(p + "-keys.tmp")
  # the delta over an older base: base overwritten by the delta, nothing else
  base_keys = np.concatenate([keys[:300], (np.arange(40, dtype=np.int64) * 7919 + 11)])
  base = _DeviceTable(kdt, dt, torch.zeros(dim), "sf_base_" + key_dtype, "cuda:0", dim=dim, init_capacity=4096)
  base.upsert(_t(torch, base_keys.astype(knp)), _t(torch, _rows(torch, base_keys, dim, dt, ver=1)))
  expect = {int(k): r.tobytes() for k, r in zip(base_keys, _rows(torch, base_keys, dim, dt, ver=1))}
  expect.update({int(k): r.tobytes() for k, r in zip(want[0], want[1])})
  assert base.load(p7) == want[0].size
  bk, bv = base.export_all()[:2]
  bk, bv = bk.cpu().numpy(), bv.cpu().numpy()
  assert bk.size == len(expect) and {int(k): r.tobytes() for k, r in zip(bk, bv)} == expect
  # append the complement on top of the delta: the file holds the whole table
  assert tbl.save_if(p1, thr, "lt", append_to_file=True) == rest[0].size
  fk, fv = _read_kv(p1, knp)
  np.testing.assert_array_equal(fk, snap[0])
  np.testing.assert_array_equal(fv, snap[1])
  # a filter nothing matches writes empty files
  pe = str(tmp_path / "empty")
  assert tbl.save_if(pe, 0, "lt") == 0
  assert os.path.getsize(pe + "-keys") == 0 and os.path.getsize(pe + "-values") == 0
  _same(_snap(tbl), snap, "save_if changes nothing")


# ---- 8. the Python surface -----------------------------------------------------------------------------------------------------------
def test_hkv_table_and_variable_surface(env, tmp_path, monkeypatch):
  torch, de = env
  monkeypatch.delenv("TFRA_SAVED_KV", raising=False)
  dim = 4
  score_of = lambda k: (k.abs() % 97 + 1)
  cfg = de.HkvHashTableConfig(init_capacity=1024, max_capacity=1024, evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, gen_scores_fn=score_of)
  var = de.Variable(dim=dim, name="sf_var", devices=["cuda:0", "cuda:0"], kv_creator=de.HkvHashTableCreator(cfg), initializer=0.0)
  rng = np.random.default_rng(17)
  keys = np.unique(rng.integers(1, 2**40, size=608, dtype=np.int64))[:600]
  var.upsert(_t(torch, keys), _t(torch, _rows(torch, keys, dim, torch.float32)))
  shards = [_snap(t._table) for t in var.tables]
  assert all(s[0].size > 200 for s in shards) and sum(s[0].size for s in shards) == 600
  for s in shards:
    np.testing.assert_array_equal(s[2], (np.abs(s[0]) % 97 + 1).astype(np.uint64))
  thr = 49
  for pred in ("ge", "lt"):
    per = [_want(s, thr, pred) for s in shards]
    for t, w in zip(var.tables, per):
      _same(_sorted(torch, *t.export_if(thr, pred)), w, "HkvHashTable.export_if " + pred)
      c = t.size_if(thr, pred)
      assert tuple(c.shape) == (1,) and int(c.item()) == w[0].size
    k, v, s = var.export_if(thr, pred)
    assert k.numel() == sum(w[0].size for w in per)
    np.testing.assert_array_equal(np.sort(k.cpu().numpy()[:per[0][0].size]), per[0][0])      # shard by shard, as export
    o = np.argsort(np.concatenate([w[0] for w in per]))
    _same(_sorted(torch, k, v, s), tuple(np.concatenate([w[i] for w in per])[o] for i in range(3)), "Variable.export_if " + pred)
    assert int(var.size_if(thr, pred).item()) == k.numel()
  # delta files: save_to_file_system's names; each loads into a base through the existing load
  d = str(tmp_path / "delta")
  per = [_want(s, thr, "ge") for s in shards]
  assert var.save_delta(d, thr) == sum(w[0].size for w in per)
  assert sorted(os.listdir(d)) == sorted("sf_var_mht_%dof2-%s" % (i, x) for i in (1, 2) for x in ("keys", "values"))
  for i, w in enumerate(per):
    fk, fv = _read_kv(os.path.join(d, "sf_var_mht_%dof2" % (i + 1)))
    np.testing.assert_array_equal(fk, w[0])
    np.testing.assert_array_equal(fv, w[1])
  d1 = str(tmp_path / "one")
  assert var.tables[0].save_delta_to_file_system(d1, thr, "lt", file_name="x", dirpath_env=None) == _want(shards[0], thr, "lt")[0].size
  assert var.tables[0].save_delta_to_file_system(d1, thr, "ge", file_name="x", dirpath_env=None, append_to_file=True) == per[0][0].size
  np.testing.assert_array_equal(_read_kv(os.path.join(d1, "x"))[0], shards[0][0])
  fresh = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=1024, max_capacity=1024, device="cuda:0", dim=dim,
                          evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, gen_scores_fn=score_of, name="x")
  assert fresh.load_from_file_system(d1, dirpath_env=None) == shards[0][0].size
  _same(_snap(fresh._table)[:2], shards[0][:2], "load_from_file_system of a delta file")
  # bad arguments: before any launch
  for obj in (var, var.tables[0], var.tables[0]._table):
    for call in ("export_if", "size_if" if obj is not var.tables[0]._table else "count_if"):
      with pytest.raises(ValueError):
        getattr(obj, call)(1, "gt")
      with pytest.raises(ValueError):
        getattr(obj, call)(-1, "ge")
      with pytest.raises(ValueError):
        getattr(obj, call)(2**64, "ge")
  with pytest.raises(ValueError):
    var.remove_if(1, pred="le")
  # remove_if: the per-shard counts, summed
  gone = sum(_want(s, thr, "lt")[0].size for s in shards)
  assert int(var.remove_if(thr).item()) == gone
  assert int(var.size().item()) == 600 - gone
  for t, s in zip(var.tables, shards):
    _same(_snap(t._table), _want(s, thr, "ge"), "Variable.remove_if")


def test_a_variable_without_scores_refuses(env, tmp_path):
  torch, de = env
  var = de.Variable(dim=4, name="sf_cuckoo", devices=["cuda:0", "cuda:0"], initializer=0.0)
  keys = np.arange(1, 301, dtype=np.int64) * 104729
  var.upsert(_t(torch, keys), _t(torch, _rows(torch, keys, 4, torch.float32)))
  before = var.export()
  for call, args in (("export_if", (5,)), ("remove_if", (5,)), ("size_if", (5,)), ("save_delta", (str(tmp_path / "no"), 5))):
    with pytest.raises(NotImplementedError, match="NONE"):
      getattr(var, call)(*args)
  assert not os.path.exists(str(tmp_path / "no"))
  after = var.export()
  ob, oa = torch.argsort(before[0]), torch.argsort(after[0])          # (the order of an export is unspecified)
  assert torch.equal(before[0][ob], after[0][oa]) and torch.equal(before[1][ob], after[1][oa])
  assert int(var.size().item()) == 300


# ---- 9. refusals at the C level ------------------------------------------------------------------------------------------------------
def test_c_level_refusals(env, tmp_path):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _ptr, _stream
  lib = _capi.lib()
  err = lambda: lib.tfra_last_error().decode()
  grow = _DeviceTable(torch.int64, torch.float32, torch.zeros(4), "sf_growing", "cuda:0", dim=4, init_capacity=1024)
  keys = np.arange(1, 201, dtype=np.int64) * 15485863
  grow.upsert(_t(torch, keys), _t(torch, _rows(torch, keys, 4, torch.float32)))
  st = _stream(grow.device)
  counter = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
  kbuf = torch.full((256,), -7, dtype=torch.int64, device="cuda")
  # a growing table has no score line: UNSUPPORTED, nothing enqueued, nothing written
  assert lib.tfra_table_export_batch_if(grow._h, GE, 0, grow.capacity(), 0, _ptr(counter), 256, _ptr(kbuf), None, None, st) == _capi.ERR_UNSUPPORTED
  assert "tfra_table_export_batch_if" in err()
  assert lib.tfra_table_export_batch_if(grow._h, GE, 0, grow.capacity(), 0, _ptr(counter), 0, None, None, None, st) == _capi.ERR_UNSUPPORTED
  assert lib.tfra_table_erase_if(grow._h, GE, 0, _ptr(counter), st) == _capi.ERR_UNSUPPORTED
  assert "tfra_table_erase_if" in err()
  prefix = str(tmp_path / "refused")
  n_saved = ctypes.c_size_t(777)
  assert lib.tfra_table_save_if(grow._h, 0, GE, 0, prefix.encode(), 0, 0, st, ctypes.byref(n_saved)) == _capi.ERR_UNSUPPORTED
  assert "tfra_table_save_if" in err()
  assert os.listdir(str(tmp_path)) == [] and n_saved.value == 777
  torch.cuda.synchronize()
  assert int(counter.item()) == 12345 and bool((kbuf == -7).all())
  assert grow.size_host() == 200
  with pytest.raises(_capi.TfraError):
    grow.count_if(0)
  # a scored table: an unknown predicate, and count-only with a values or a scores buffer
  t, _, _ = _filled(env, "sf_refuse", torch.float32, 4, 1024, 100, seed=19)
  tbl = t._table
  vbuf = torch.zeros((256, 4), device="cuda")
  sbuf = torch.zeros(256, dtype=torch.int64, device="cuda")
  for pred in (2, -1, 7):
    assert lib.tfra_table_export_batch_if(tbl._h, pred, 0, tbl.capacity(), 0, _ptr(counter), 256, _ptr(kbuf), None, None, st) == -1
    assert "tfra_table_export_batch_if" in err()
    assert lib.tfra_table_erase_if(tbl._h, pred, 0, _ptr(counter), st) == -1
    assert lib.tfra_table_save_if(tbl._h, 0, pred, 0, prefix.encode(), 0, 0, st, None) == -1
  assert lib.tfra_table_export_batch_if(tbl._h, GE, 0, tbl.capacity(), 0, _ptr(counter), 256, None, _ptr(vbuf), None, st) == -1
  assert "tfra_table_export_batch_if" in err()
  assert lib.tfra_table_export_batch_if(tbl._h, GE, 0, tbl.capacity(), 0, _ptr(counter), 256, None, None, _ptr(sbuf), st) == -1
  assert lib.tfra_table_export_batch_if(tbl._h, GE, 0, tbl.capacity(), 0, None, 256, _ptr(kbuf), None, None, st) == -1
  assert lib.tfra_table_save_if(tbl._h, 3, GE, 0, prefix.encode(), 0, 0, st, None) == -1       # no such field
  torch.cuda.synchronize()
  assert int(counter.item()) == 12345 and bool((kbuf == -7).all()) and os.listdir(str(tmp_path)) == []
  assert tbl.size_host() == 102
