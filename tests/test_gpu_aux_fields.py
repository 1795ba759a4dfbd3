"""GPU: co-located state fields (tables created with aux_fields = S > 0) through every table entry point, byte-exact against
the row model of tests/field_model.py.  A row holds 1 + S vectors of `dim` elements, its stride rounded up to 16 bytes; the
shapes below make each copy granule (1, 2, 4, 8, 16 bytes) and each branch of the aux initialisation (4-byte words, single
bytes) the deciding one, and aux_init gives every aux field a pattern of its own.

What the tests found out about a field insert (tfra_table_insert_field, field != 0) of ABSENT keys on a bounded table at
max_capacity: it never evicts.  A key whose home buckets have a free slot is created (field 0 zeros, the other aux fields
aux_init); a key whose home buckets are full is dropped and counted, check_errors() reports exactly those keys; no resident
row changes (test_bounded_field_insert_of_absent_keys)."""
import os
import zlib

import numpy as np
import pytest

from tests import field_model as fm

pytestmark = pytest.mark.gpu

AUX = (0.1, -2.75, 3.0, 0.0)
IMIN = np.iinfo(np.int64).min
SLOTS = 15

# dtype, dim, S            field bytes, row bytes -> stride
SHAPES = [
    ("int8", 3, 4),        # 3, 15 -> 16      granule 1, per-byte init
    ("float16", 1, 2),     # 2, 6 -> 16       granule 2
    ("bfloat16", 3, 3),    # 6, 24 -> 32      per-byte init, elem_bytes 2
    ("float32", 3, 2),     # 12, 36 -> 48     granule 4
    ("float32", 6, 1),     # 24, 48           granule 8: the field offset clamps 16 -> 8
    ("float16", 20, 4),    # 40, 200 -> 208   padded row
    ("float32", 64, 2),    # 256, 768         the optimizer's own shape, as control
    ("int64", 5, 1),       # 40, 80           8-byte exception
    ("float64", 2, 2),     # 16, 48           8-byte exception
    ("int32", 4, 4),       # 16, 80           integer truncation of aux_init
]


def _sid(s):
  return "%s-%d-S%d" % s


def _seed(*parts):
  return zlib.crc32(repr(parts).encode())


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _tdt(torch, name):
  return getattr(torch, name)


def _dev(torch, shape, arr):
  """rows of the storage dtype [n, dim] -> device tensor of the table's dtype (through their bytes: bit patterns survive)"""
  b = np.ascontiguousarray(fm.as_bytes(arr))
  return torch.from_numpy(b.copy()).view(_tdt(torch, shape[0])).cuda()


def _bytes(t):
  import torch
  return t.contiguous().cpu().view(torch.uint8).numpy()


def _bits(rng, shape, n):
  """random bit patterns: NaN payloads, -0.0, denormals must survive every copy"""
  st = fm.STORAGE[shape[0]]
  es = np.dtype(st).itemsize
  return rng.integers(0, 256, size=(n, shape[1] * es), dtype=np.uint8).view(st).reshape(n, shape[1])


def _finite(rng, shape, n):
  return fm.from_float(shape[0], rng.integers(-50, 50, size=(n, shape[1])).astype(np.float32) * 0.37)


def _kt(torch, keys):
  return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).cuda()


def _universe(lo, n):
  return np.arange(lo + 1, lo + n + 1, dtype=np.int64) * 104723 - 77


def _table(env, shape, name, init_size=64):
  torch, de = env
  dt = _tdt(torch, shape[0])
  t = de.CuckooHashTable(torch.int64, dt, torch.zeros(shape[1], dtype=dt), device="cuda:0", dim=shape[1], init_size=init_size,
                         aux_fields=shape[2], aux_init=AUX, name=name)
  return t, fm.FieldModel(shape[0], shape[1], shape[2], AUX)


def _fill(env, shape, t, m, rng, n=2400, lo=0, bits=True):
  """n keys (both sentinel key values among them) by unique-key upserts of 800: the table grows in front of them"""
  torch, _ = env
  keys = np.concatenate([_universe(lo, n - 2), [IMIN, IMIN + 1]]).astype(np.int64)
  rng.shuffle(keys)
  vals = _bits(rng, shape, n) if bits else _finite(rng, shape, n)
  for a in range(0, n, 800):
    t._table.upsert(_kt(torch, keys[a:a + 800]), _dev(torch, shape, vals[a:a + 800]), unique_keys=True)
    m.insert_or_assign(keys[a:a + 800], vals[a:a + 800])
  return keys


def _scribble(env, shape, t, m, rng, keys):
  """distinctive bytes into every aux field of `keys` (resident)"""
  torch, _ = env
  for f in range(1, shape[2] + 1):
    v = _bits(rng, shape, keys.size)
    t._table.upsert(_kt(torch, keys), _dev(torch, shape, v), unique_keys=True, field=f)
    m.insert_field(f, keys, v)


def _check(env, shape, t, m, keys, tag=""):
  """every field of `keys`, rows and exists flags, against the model"""
  torch, _ = env
  zero = np.zeros(shape[1], m.st)
  kt = _kt(torch, keys)
  for f in range(shape[2] + 1):
    got, ex = t._table.find(kt, _dev(torch, shape, zero[None])[0], return_exists=True, field=f)
    want, wex = m.find_field(f, keys, zero)
    np.testing.assert_array_equal(ex.cpu().numpy(), wex, err_msg="%s exists, field %d" % (tag, f))
    np.testing.assert_array_equal(_bytes(got), fm.as_bytes(want), err_msg="%s field %d" % (tag, f))
  assert t._table.size_host() == m.size(), tag
  t._table.check_errors()
  assert t._table.slot_census()["locked"] == 0


def _own_takes(t, n):
  """the route of a unique-key call of n keys (own_upsert_unique, csrc/tfra_own.hip): the ownership pass while the expected
  number of keys sharing a home bucket, 2 n^2 / buckets, stays below 2048; a bulk load takes the locked kernels"""
  return 2.0 * n * n / ((t._table.capacity() - 2) // SLOTS) < 2048.0


# ---- the insert paths: each takes (env, shape, table, model, rng, pool of absent unique keys) and inserts some of them ------------
def _p_own(env, shape, t, m, rng, pool):
  torch, _ = env
  k, v = pool[:128], _bits(rng, shape, 128)
  t._table.upsert(_kt(torch, k), _dev(torch, shape, v), unique_keys=True)
  assert _own_takes(t, 128)
  m.insert_or_assign(k, v)
  return k


def _p_bulk(env, shape, t, m, rng, pool):
  torch, _ = env
  n = min(pool.size, 1200)
  k, v = pool[:n], _bits(rng, shape, n)
  t._table.upsert(_kt(torch, k), _dev(torch, shape, v), unique_keys=True)
  assert not _own_takes(t, n)          # insert_unique_kernel
  m.insert_or_assign(k, v)
  return k


def _dups(rng, pool, nu, n):
  ids = pool[:nu][rng.integers(0, nu, size=n)]
  ids[:nu] = pool[:nu]                   # every key at least once
  rng.shuffle(ids)
  return ids


def _p_dups(env, shape, t, m, rng, pool):
  torch, _ = env
  ids = _dups(rng, pool, 300, 900)
  v = _bits(rng, shape, ids.size)
  t._table.upsert(_kt(torch, ids), _dev(torch, shape, v))      # no flag: locate / write, the last occurrence wins
  m.insert_or_assign(ids, v)
  return pool[:300]


def _p_upsert_n(env, shape, t, m, rng, pool):
  torch, _ = env
  k, v = pool[:256], _bits(rng, shape, 256)
  cnt = torch.tensor([130], dtype=torch.int64, device="cuda")
  t._table.upsert_n(_kt(torch, k), cnt, _dev(torch, shape, v))   # raises unless the ownership pass takes the call
  m.insert_or_assign(k[:130], v[:130])
  return k                                                         # (the keys beyond the count must stay absent)


def _p_sparse(env, shape, t, m, rng, pool):
  torch, _ = env
  ids = _dups(rng, pool, 300, 900)
  v = _bits(rng, shape, ids.size)
  t._table.upsert_sparse(_kt(torch, ids), _dev(torch, shape, v))
  m.insert_or_assign(ids, v)
  return pool[:300]


def _p_planned(env, shape, t, m, rng, pool):
  torch, _ = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  ids = _dups(rng, pool, 300, 900)
  v = _bits(rng, shape, ids.size)
  plan = SparsePlan("cuda:0", 0).build(_kt(torch, ids))
  t._table.upsert_planned(plan, _dev(torch, shape, v))
  torch.cuda.synchronize()
  m.insert_or_assign(ids, v)
  return pool[:300]


def _accum(tags, unique):
  def run(env, shape, t, m, rng, pool):
    torch, _ = env
    t._table.set_owner_tags(tags)
    k = pool[:160]
    ex = np.zeros(160, bool)
    ex[128:] = True                      # absent & exists: nothing
    o = rng.permutation(160)
    k, ex = k[o], ex[o]
    v = _finite(rng, shape, 160)
    t._table.accum_or_assign(_kt(torch, k), _dev(torch, shape, v), torch.from_numpy(ex).cuda(), unique_keys=unique)
    if unique and tags:
      assert _own_takes(t, 160)          # (rows of 16-byte granules: the ownership pass; other widths: the locked kernels)
    m.accum_or_assign(k, v, ex)
    t._table.set_owner_tags(True)
    return k
  return run


PATHS = {"own": _p_own, "bulk": _p_bulk, "dups": _p_dups, "upsert_n": _p_upsert_n, "sparse": _p_sparse, "planned": _p_planned,
         "accum_tags": _accum(True, True), "accum_notags": _accum(False, True), "accum_dups": _accum(True, False)}


# ---- 1. new rows on every insert path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_new_rows_start_at_aux_init(env, shape, path):
  rng = np.random.default_rng(_seed(shape, path, 1))
  t, m = _table(env, shape, "aux_new_%s_%s" % (_sid(shape), path))
  pool = _universe(100_000, 1200)
  pool[:2] = [IMIN, IMIN + 1]
  if path == "bulk":       # a bulk load into the small table itself
    used = PATHS[path](env, shape, t, m, rng, pool)
    resident = np.zeros(0, np.int64)
  else:
    resident = _fill(env, shape, t, m, rng)
    resident = resident[(resident != IMIN) & (resident != IMIN + 1)]
    t._table.erase(_kt(env[0], [IMIN, IMIN + 1]))
    m.erase([IMIN, IMIN + 1])
    assert t._table.growth_stats()["growths"] >= 2
    _scribble(env, shape, t, m, rng, resident[:600])
    used = PATHS[path](env, shape, t, m, rng, pool)
  assert m.size() > resident.size
  _check(env, shape, t, m, np.concatenate([used, resident, pool[-50:]]), tag=path)


# ---- 2. field isolation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_field_isolation(env, shape):
  torch, _ = env
  rng = np.random.default_rng(7 + shape[1])
  t, m = _table(env, shape, "aux_iso_" + _sid(shape))
  keys = _fill(env, shape, t, m, rng)
  assert t._table.growth_stats()["growths"] >= 2
  kt = _kt(torch, keys)
  for f in list(range(1, shape[2] + 1)) + [0]:
    for unique in (True, False):
      sub = keys[rng.permutation(keys.size)[:1500]] if unique else keys[rng.integers(0, keys.size, size=1500)]
      v = _bits(rng, shape, sub.size)
      t._table.upsert(_kt(torch, sub), _dev(torch, shape, v), unique_keys=unique, field=f)
      m.insert_field(f, sub, v)
      _check(env, shape, t, m, keys, tag="upsert field %d unique %s" % (f, unique))
  # accumulate on present keys: field 0 only, one add per element
  base = _finite(rng, shape, keys.size)
  t._table.upsert(kt, _dev(torch, shape, base), unique_keys=True)
  m.insert_or_assign(keys, base)
  for unique, n in ((True, 128), (True, 2000), (False, 1500)):
    sub = keys[rng.permutation(keys.size)[:n]] if unique else keys[rng.integers(0, keys.size, size=n)]
    d = _finite(rng, shape, n)
    ex = rng.random(n) < 0.7
    t._table.accum_or_assign(_kt(torch, sub), _dev(torch, shape, d), torch.from_numpy(ex).cuda(), unique_keys=unique)
    m.accum_or_assign(sub, d, ex)
    _check(env, shape, t, m, keys, tag="accum unique %s n %d" % (unique, n))


# ---- 3. find(field=f) defaults ----------------------------------------------------------------------------------------------------
def _at_offset(torch, x, k):
  buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=x.device)
  v = buf[k: k + x.numel()].view(x.shape)
  v.copy_(x)
  return v


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_find_field_defaults(env, shape):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  rng = np.random.default_rng(11 + shape[1])
  t, m = _table(env, shape, "aux_find_" + _sid(shape))
  keys = _fill(env, shape, t, m, rng)
  _scribble(env, shape, t, m, rng, keys)
  look = np.concatenate([keys[:700], _universe(500_000, 700)])
  rng.shuffle(look)
  n = look.size
  kt = _kt(torch, look)
  tbl = t._table
  for f in range(shape[2] + 1):
    d1, dn = _bits(rng, shape, 1)[0], _bits(rng, shape, n)
    for d, k in ((d1, 0), (dn, 0), (d1, 1), (dn, 1)):
      dd = _dev(torch, shape, d.reshape(-1, shape[1])).reshape(d.shape)
      if k:
        dd = _at_offset(torch, dd, k)
      want, wex = m.find_field(f, look, d)
      got, ex = tbl.find(kt, dd, return_exists=True, field=f)
      np.testing.assert_array_equal(ex.cpu().numpy(), wex)
      np.testing.assert_array_equal(_bytes(got), fm.as_bytes(want), err_msg="field %d offset %d full %s" % (f, k, d is dn))
      got2 = tbl.find(kt, dd, field=f)          # without exists
      np.testing.assert_array_equal(_bytes(got2), fm.as_bytes(want))
    # the output rows at an element offset (the pointer is not 16-byte aligned), guard elements around them untouched
    buf = torch.from_numpy(np.full((n * shape[1] + 8) * np.dtype(m.st).itemsize, 0xA5, np.uint8)).view(_tdt(torch, shape[0])).cuda()
    out = buf[1: 1 + n * shape[1]].view(n, shape[1])
    exb = torch.empty(n, dtype=torch.bool, device="cuda")
    dd = _dev(torch, shape, dn)
    if f:
      _capi.call("tfra_table_find_field", tbl._h, f, n, _ptr(kt), _ptr(out), _ptr(exb), _ptr(dd), 1, _stream(tbl.device))
    else:
      _capi.call("tfra_table_find", tbl._h, n, _ptr(kt), _ptr(out), _ptr(exb), _ptr(dd), 1, _stream(tbl.device))
    want, wex = m.find_field(f, look, dn)
    np.testing.assert_array_equal(_bytes(out), fm.as_bytes(want), err_msg="field %d, out at offset" % f)
    np.testing.assert_array_equal(exb.cpu().numpy(), wex)
    bb = _bytes(buf)
    es = np.dtype(m.st).itemsize
    assert (bb[:es] == 0xA5).all() and (bb[(1 + n * shape[1]) * es:] == 0xA5).all()


# ---- 4. no stale state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(PATHS) + ["clear_all"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_reinserted_keys_start_at_aux_init_again(env, shape, path):
  torch, _ = env
  rng = np.random.default_rng(_seed(shape, path, 4))
  t, m = _table(env, shape, "aux_stale_%s_%s" % (_sid(shape), path))
  keys = _fill(env, shape, t, m, rng)
  _scribble(env, shape, t, m, rng, keys)
  if path == "clear_all":
    t._table.clear_all()
    m.clear()
    gone, kept = keys, np.zeros(0, np.int64)
    PATHS["bulk"](env, shape, t, m, rng, gone)
  else:
    pos = np.concatenate([np.flatnonzero(keys == IMIN), np.flatnonzero(keys == IMIN + 1)])
    rest = np.setdiff1d(np.arange(keys.size), pos)
    gone = np.concatenate([keys[pos], keys[rest[:1198]]])       # half of the keys, the sentinel values first
    kept = keys[rest[1198:]]
    t._table.erase(_kt(torch, gone))
    m.erase(gone)
    _check(env, shape, t, m, keys, tag="after erase")
    PATHS[path](env, shape, t, m, rng, gone)
  assert m.size() > kept.size
  _check(env, shape, t, m, keys, tag=path)


# ---- 5. insert_field of absent keys -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unique", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_insert_field_of_absent_keys(env, shape, unique):
  torch, _ = env
  rng = np.random.default_rng(13 + shape[1] + unique)
  t, m = _table(env, shape, "aux_absent_%s_%d" % (_sid(shape), unique))
  resident = _fill(env, shape, t, m, rng, n=1200)
  _scribble(env, shape, t, m, rng, resident)
  seen = [resident]
  for f in range(1, shape[2] + 1):
    new = _universe(200_000 + 10_000 * f, 700)
    ids = np.concatenate([new, resident[:100]])      # ... and some resident keys in the same call
    if not unique:
      ids = np.concatenate([ids, new[:200]])          # repeats: the last occurrence wins
    rng.shuffle(ids)
    v = _bits(rng, shape, ids.size)
    t._table.upsert(_kt(torch, ids), _dev(torch, shape, v), unique_keys=unique, field=f)
    m.insert_field(f, ids, v)
    seen.append(new)
    zero = np.zeros(shape[1], m.st)
    for k in new[:5].tolist():
      assert not m.rows[k][0].any()
      for g in range(1, shape[2] + 1):
        if g != f:
          assert np.array_equal(m.rows[k][g], np.full(shape[1], m.aux[g - 1], m.st))
    _check(env, shape, t, m, np.concatenate(seen), tag="field %d" % f)
  assert t._table.size_host() == m.size()


# ---- 6. bounded table at capacity -------------------------------------------------------------------------------------------------
BOUNDED = [("float32", 6, 1), ("float16", 20, 4)]
CAP = 2048 * SLOTS      # 2048 buckets; 200 fresh keys a call: the tenth of a key per bucket of tests/test_gpu_accum_own.py


def _bounded(env, shape, name, rng):
  """A full LRU table whose resident rows hold distinctive bytes in every field -> (table, {key: [1 + S, dim] rows})"""
  torch, de = env
  dt = _tdt(torch, shape[0])
  t = de.HkvHashTable(torch.int64, dt, torch.zeros(shape[1], dtype=dt), init_capacity=CAP, max_capacity=CAP, device="cuda:0",
                      dim=shape[1], evict_strategy=de.HkvEvictStrategy.LRU, aux_fields=shape[2], aux_init=AUX, name=name)
  tbl = t._table
  fill = np.arange(1, CAP + CAP // 4 + 1, dtype=np.int64) * 7919
  for a in range(0, fill.size, 4096):
    k = fill[a:a + 4096]
    tbl.upsert(_kt(torch, k), _dev(torch, shape, _bits(rng, shape, k.size)), unique_keys=True)
  rk = np.sort(tbl.export_all()[0].cpu().numpy())
  assert rk.size > 0.8 * CAP
  for f in range(shape[2] + 1):
    tbl.upsert(_kt(torch, rk), _dev(torch, shape, _bits(rng, shape, rk.size)), unique_keys=True, field=f)
  tbl.check_errors()
  assert tbl.size_host() == rk.size      # present keys: nothing was created, nothing dropped
  return t, rk, _read_all(env, shape, tbl, rk)[0]


def _read_all(env, shape, tbl, keys):
  torch, _ = env
  zero = torch.zeros(shape[1], dtype=_tdt(torch, shape[0]), device="cuda")
  rows, ex = [], None
  for f in range(shape[2] + 1):
    r, ex = tbl.find(_kt(torch, keys), zero, return_exists=True, field=f)
    rows.append(_bytes(r))
  return np.stack(rows, 1), ex.cpu().numpy()      # [n, 1 + S, field bytes]


def _aux_bytes(shape):
  m = fm.FieldModel(shape[0], shape[1], shape[2], AUX)
  return fm.as_bytes(m.new_row())[1:]


def _old_rows_unchanged(env, shape, tbl, rk, before, tag):
  after, ex = _read_all(env, shape, tbl, rk)
  np.testing.assert_array_equal(after[ex], before[ex], err_msg=tag)
  return ex


@pytest.mark.parametrize("owner_tags", [True, False])
@pytest.mark.parametrize("shape", BOUNDED, ids=_sid)
def test_bounded_fresh_keys_evict_into_clean_rows(env, shape, owner_tags):
  torch, _ = env
  rng = np.random.default_rng(17 + shape[1])
  t, rk, before = _bounded(env, shape, "aux_bnd_%s_%d" % (_sid(shape), owner_tags), rng)
  tbl = t._table
  tbl.set_owner_tags(owner_tags)
  aux = _aux_bytes(shape)
  for step, how in enumerate(["upsert", "accum", "upsert", "accum"]):
    fresh = np.arange(10**9 + step * 5000, 10**9 + step * 5000 + 200, dtype=np.int64)
    v = _finite(rng, shape, fresh.size)
    if how == "upsert":
      tbl.upsert(_kt(torch, fresh), _dev(torch, shape, v), unique_keys=True)
    else:
      tbl.accum_or_assign(_kt(torch, fresh), _dev(torch, shape, v), torch.zeros(fresh.size, dtype=torch.bool, device="cuda"), unique_keys=True)
    assert _own_takes(t, fresh.size)      # (upsert: the ownership pass; accumulate on rows that are no multiple of 16 bytes: locked)
    got, ex = _read_all(env, shape, tbl, fresh)
    assert ex.all(), (how, int((~ex).sum()))                     # every fresh key is resident
    np.testing.assert_array_equal(got[:, 0], fm.as_bytes(v), err_msg=how)
    for f in range(1, shape[2] + 1):                             # ... with its aux fields at aux_init, not a victim's
      np.testing.assert_array_equal(got[:, f], np.broadcast_to(aux[f - 1], got[:, f].shape), err_msg="%s field %d" % (how, f))
    ex_old = _old_rows_unchanged(env, shape, tbl, rk, before, how)
    assert ex_old.sum() >= rk.size - 200 * (step + 1)
    assert tbl.size_host() <= tbl.capacity()
    tbl.check_errors()
    assert tbl.slot_census()["locked"] == 0


@pytest.mark.parametrize("unique", [True, False])
@pytest.mark.parametrize("shape", BOUNDED, ids=_sid)
def test_bounded_field_insert_of_absent_keys(env, shape, unique):
  """A field insert never evicts: at max_capacity an absent key is created where its home buckets have room and is dropped and
  counted where they have none.  No resident row changes either way."""
  torch, _ = env
  from tfra_amd._capi import TfraError
  rng = np.random.default_rng(19 + shape[1])
  t, rk, before = _bounded(env, shape, "aux_bndf_%s_%d" % (_sid(shape), unique), rng)
  tbl = t._table
  aux = _aux_bytes(shape)
  f = shape[2]
  fresh = np.arange(3 * 10**9, 3 * 10**9 + 200, dtype=np.int64)
  v = _bits(rng, shape, fresh.size)
  size0 = tbl.size_host()
  tbl.upsert(_kt(torch, fresh), _dev(torch, shape, v), unique_keys=unique, field=f)
  got, ex = _read_all(env, shape, tbl, fresh)
  ex_old = _old_rows_unchanged(env, shape, tbl, rk, before, "field insert")
  assert ex_old.all()                                             # nothing was evicted
  assert tbl.slot_census()["locked"] == 0
  n_in = int(ex.sum())
  np.testing.assert_array_equal(got[ex][:, f], fm.as_bytes(v)[ex])
  assert not got[ex][:, 0].any()                                  # field 0 = zeros
  for g in range(1, shape[2] + 1):
    if g != f:
      np.testing.assert_array_equal(got[ex][:, g], np.broadcast_to(aux[g - 1], got[ex][:, g].shape))
  if n_in == fresh.size:
    tbl.check_errors()
  else:
    with pytest.raises(TfraError) as e:
      tbl.check_errors()
    assert ("%d keys could not be placed" % (fresh.size - n_in)) in str(e.value), str(e.value)   # exactly the keys that are not resident
    tbl.check_errors()                                            # (reported once)
  assert tbl.size_host() == size0 + n_in <= tbl.capacity()        # (a pending error count makes the size read raise: after the check)


# ---- 7. readers on strided rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_readers_on_strided_rows(env, shape):
  torch, de = env
  rng = np.random.default_rng(23 + shape[1])
  t, m = _table(env, shape, "aux_read_" + _sid(shape))
  keys = _fill(env, shape, t, m, rng, bits=False)
  _scribble(env, shape, t, m, rng, keys)
  tbl = t._table
  # export: field 0 only, several windows
  ek, ev, _ = tbl.export_all(split_size=257)
  ek, evb = ek.cpu().numpy(), _bytes(ev)
  assert ek.size == np.unique(ek).size
  assert {int(k): evb[i].tobytes() for i, k in enumerate(ek)} == m.items_field(0)
  # find_unique / find_n = find on field 0
  look = np.concatenate([keys[rng.integers(0, keys.size, size=900)], _universe(700_000, 300)])
  rng.shuffle(look)
  kt = _kt(torch, look)
  d1n = _finite(rng, shape, 1)
  d1 = _dev(torch, shape, d1n)[0]
  want, wex = tbl.find(kt, d1, return_exists=True)
  mw, mex = m.find_field(0, look, d1n[0])
  np.testing.assert_array_equal(wex.cpu().numpy(), mex)
  np.testing.assert_array_equal(_bytes(want), fm.as_bytes(mw))
  rows, uniq, idx, cnt, ex = tbl.find_unique(kt, d1, return_exists=True)
  assert torch.equal(rows.view(torch.uint8), want.view(torch.uint8)) and torch.equal(ex, wex)
  u = int(cnt.item())
  assert u == np.unique(look).size and torch.equal(uniq[:u][idx.long()], kt)
  cntd = torch.tensor([777], dtype=torch.int64, device="cuda")
  out = torch.from_numpy(np.full((look.size, shape[1] * np.dtype(m.st).itemsize), 0xA5, np.uint8)).view(_tdt(torch, shape[0])).cuda()
  want0 = tbl.find(kt, return_exists=False)
  got, exn = tbl.find_n(kt, cntd, out=out, return_exists=True)
  assert torch.equal(got[:777].view(torch.uint8), want0[:777].view(torch.uint8)) and torch.equal(exn[:777], wex[:777])
  assert (_bytes(got[777:]) == 0xA5).all()                         # rows beyond the count are left as they are
  # find_combine (float rows, dim % 4 == 0) = find + the segment combination of the found rows, bit for bit
  if shape[0] in ("float32", "float16", "bfloat16") and shape[1] % 4 == 0:
    seg = torch.from_numpy(np.sort(rng.integers(0, 200, size=look.size)).astype(np.int64)).cuda()
    w = torch.from_numpy((rng.integers(1, 8, size=look.size) * 0.25).astype(np.float32)).cuda()
    idx = torch.arange(look.size, dtype=torch.int32, device="cuda")
    for comb, cname in enumerate(("sum", "mean", "sqrtn")):
      for wt in (None, w):
        got = tbl.find_combine(kt, seg, wt, comb, 200, default_row=d1)
        exp = de.device_ops.sparse_segment_combine(want, idx, seg, wt, cname, 200)
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (cname, wt is not None)
  _check(env, shape, t, m, keys, tag="readers changed nothing")
  # the step driver: rows with optimizer slots go one op after the other (reason bit 8)
  drv = de.OverlapAssignStep(t)
  old = keys[:1500]
  batches = [np.concatenate([old[rng.integers(0, old.size, size=500)], _universe(800_000 + 1000 * s, 150), _universe(800_000, 50)])
             for s in range(5)]
  for b in batches:
    rng.shuffle(b)
  bt = [_kt(torch, b) for b in batches]
  vals = [_bits(rng, shape, b.size) for b in batches]
  vt = [_dev(torch, shape, v) for v in vals]
  drv.prime(bt[0])
  zero = np.zeros(shape[1], m.st)
  for s in range(4):
    out, ex = drv.step(vt[s], bt[s + 1], None, return_exists=True)
    wrows, wex = m.find_field(0, batches[s], zero)
    np.testing.assert_array_equal(ex.cpu().numpy(), wex, err_msg="step %d" % s)
    np.testing.assert_array_equal(_bytes(out), fm.as_bytes(wrows), err_msg="step %d" % s)
    m.insert_or_assign(batches[s], vals[s])
  drv.flush()
  st = drv.stats()
  assert st["overlapped"] == 0 and st["why_sequential"] & 8, st
  _check(env, shape, t, m, np.concatenate([keys] + batches[:4]), tag="after the steps")


# ---- 8. field files ---------------------------------------------------------------------------------------------------------------
def _files(prefix, m):
  k = np.fromfile(prefix + "-keys", dtype=np.int64)
  v = np.fromfile(prefix + "-values", dtype=np.uint8).reshape(k.size, -1) if k.size else np.zeros((0, 0), np.uint8)
  return k, v


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_field_files(env, shape, tmp_path):
  torch, _ = env
  from tfra_amd._capi import TfraError
  rng = np.random.default_rng(29 + shape[1])
  t, m = _table(env, shape, "aux_io_" + _sid(shape))
  keys = _fill(env, shape, t, m, rng, n=1000)
  _scribble(env, shape, t, m, rng, keys)
  tbl = t._table
  n, S = keys.size, shape[2]
  for bs in (n - 337, n, n + 1):
    for f in range(S + 1):
      p = str(tmp_path / ("bs%d_f%d" % (bs, f)))
      assert tbl.save(p, buffer_size=bs, field=f) == n
      k, v = _files(p, m)
      assert np.array_equal(np.sort(k), np.sort(keys))          # the same key set for every field
      want, wex = m.find_field(f, k, np.zeros(shape[1], m.st))
      assert wex.all()
      np.testing.assert_array_equal(v, fm.as_bytes(want), err_msg="save bs %d field %d" % (bs, f))
  # load: field 0, then every aux field, with a ragged last chunk
  t2, _ = _table(env, shape, "aux_io2_" + _sid(shape))
  for f in range(S + 1):
    assert t2._table.load(str(tmp_path / ("bs%d_f%d" % (n, f))), buffer_size=300, field=f) == n
  _check(env, shape, t2, m, np.concatenate([keys, _universe(900_000, 20)]), tag="loaded")
  # load of an aux field into an EMPTY table: the keys are created, field 0 zeros, the other aux fields aux_init
  for f in range(1, S + 1):
    t3, m3 = _table(env, shape, "aux_io3_%s_%d" % (_sid(shape), f))
    p = str(tmp_path / ("bs%d_f%d" % (n, f)))
    assert t3._table.load(p, buffer_size=300, field=f) == n
    k, v = _files(p, m)
    m3.insert_field(f, k, v.view(m.st).reshape(n, shape[1]))
    assert not m3.rows[int(k[0])][0].any()
    _check(env, shape, t3, m3, keys, tag="field %d into an empty table" % f)
  # append twice: both files double
  p = str(tmp_path / "app")
  for _ in range(2):
    assert tbl.save(p, buffer_size=n, append_to_file=True, field=S) == n
  k, v = _files(p, m)
  assert k.size == 2 * n and v.shape[0] == 2 * n
  for h in (slice(0, n), slice(n, 2 * n)):            # each half: the table's field S (the order within a save is not fixed)
    want, wex = m.find_field(S, k[h], np.zeros(shape[1], m.st))
    assert wex.all() and np.unique(k[h]).size == n
    np.testing.assert_array_equal(v[h], fm.as_bytes(want))
  assert os.path.getsize(p + "-values") == 2 * n * shape[1] * np.dtype(m.st).itemsize
  # a bad field raises and changes nothing
  kt = _kt(torch, keys[:10])
  vv = _dev(torch, shape, _bits(rng, shape, 10))
  for bad in (-1, S + 1):
    with pytest.raises(TfraError):
      tbl.find(kt, field=bad)
    with pytest.raises(TfraError):
      tbl.upsert(kt, vv, field=bad)
    with pytest.raises(TfraError):
      tbl.save(str(tmp_path / "bad"), field=bad)
    with pytest.raises(TfraError):
      tbl.load(str(tmp_path / ("bs%d_f0" % n)), field=bad)
  assert not os.path.exists(str(tmp_path / "bad") + "-keys") and not os.path.exists(str(tmp_path / "bad") + "-keys.tmp")
  _check(env, shape, t, m, keys, tag="after the bad calls")
