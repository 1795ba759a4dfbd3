"""GPU: the fused lookup + insert_or_assign step drivers and the row gathers at every row width, byte for byte.

Every other step test writes 256-byte rows that are constant across the row: exactly one pass of the kernels' row loops (16 lanes x
16 B), and a kernel that copied chunk 0 into every chunk, or served a forwarded row at the wrong 16-byte offset, would pass them.
Here the rows are seeded random BYTES viewed as the table's dtype (prefill, step values, default rows) and every column of every row
is compared through uint8 views against a host model of the reference's semantics — a dict from key to the row's bytes,
insert_or_assign's last occurrence wins, lookup i+1 sees every write of step i, a miss returns the default row (or that position's
default row).  Widths: 16-byte multiples from 16 to 4096 B (narrower than a pass, a pass plus one granule, many passes) take the
overlapped launch; other widths (6, 8, 24, 260 B) must fall back to the ops one after the other (why_sequential bit 2).
Reference: K/hkv_hashtable_op_gpu.cu.cc:182-290 (Find shared / Insert exclusive), K/cuckoo_hashtable_op.cc:111-150."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IMIN = np.iinfo(np.int64).min
ESIZE = {"float32": 4, "float16": 2, "bfloat16": 2, "int8": 1, "int64": 8}
# (dtype, dim): row bytes 16 16 32 48 64 128 144 240 256 272 512 1040 4096 — the overlapped launch
OVL = [("float32", 4), ("int8", 16), ("bfloat16", 16), ("float32", 12), ("float32", 16), ("float32", 32), ("int64", 18), ("float16", 120),
       ("float32", 64), ("float32", 68), ("float32", 128), ("float32", 260), ("float32", 1024)]
# row bytes 6 8 24 260 — not a 16-byte multiple: the sequential fallback
SEQ = [("float16", 3), ("int64", 1), ("float32", 6), ("float32", 65)]
WIDTHS = OVL + SEQ


def _wid(w):
  return "%s_x%d_%dB" % (w[0], w[1], ESIZE[w[0]] * w[1])


def _rb(w):
  return ESIZE[w[0]] * w[1]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  from tfra_amd import _capi
  return torch, de, _capi


def _rand(torch, rng, shape, dtype):
  """seeded random bytes on cuda:0 viewed as `dtype` (any bit pattern: NaNs included — compare bytes only)"""
  nel = int(np.prod(shape))
  b = rng.integers(0, 256, size=nel * torch.empty((), dtype=dtype).element_size(), dtype=np.uint8)
  return torch.from_numpy(b).cuda().view(dtype).reshape(shape)


def _b(t):
  """host byte view [rows, row bytes] (or [bytes] of a vector)"""
  import torch
  u = t.contiguous()
  u = u.view(torch.uint8) if u.dtype != torch.uint8 else u
  return u.reshape(t.shape[0], -1).cpu().numpy() if t.dim() > 1 else u.reshape(-1).cpu().numpy()


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class ByteModel:
  """The reference's table semantics on the host: key -> the row's bytes (every key that can appear is known up front)."""

  def __init__(self, keys, rb, default):
    self.keys = np.unique(np.asarray(keys, np.int64))
    self.rows = np.zeros((self.keys.size, rb), np.uint8)
    self.present = np.zeros(self.keys.size, bool)
    self.default = default

  def idx(self, ids):
    i = np.searchsorted(self.keys, ids)
    assert np.all(i < self.keys.size) and np.array_equal(self.keys[np.minimum(i, self.keys.size - 1)], ids), "key unknown to the model"
    return i

  def assign(self, ids, rows):
    """insert_or_assign of a batch: the last occurrence of a key wins"""
    i = self.idx(ids)
    u, first_rev = np.unique(i[::-1], return_index=True)
    self.rows[u] = rows[i.size - 1 - first_rev]
    self.present[u] = True

  def lookup(self, ids, defaults=None):
    """rows and exists flags; a miss reads the default row, or its own position's row of `defaults` [n, rb]"""
    i = self.idx(ids)
    ex = self.present[i]
    dflt = np.broadcast_to(self.default, (i.size, self.rows.shape[1])) if defaults is None else defaults
    return np.where(ex[:, None], self.rows[i], dflt), ex

  def check_export(self, ek, ev, exact):
    ekn = ek.cpu().numpy()
    assert np.unique(ekn).size == ekn.size
    i = self.idx(ekn)
    assert self.present[i].all()
    np.testing.assert_array_equal(_b(ev), self.rows[i])
    if exact:
      assert ekn.size == int(self.present.sum())
    else:   # (a dense table evicts now and then: never more than a handful)
      assert ekn.size >= 0.99 * int(self.present.sum())


def _check_model(model, ids, ob, exn, exact, defaults=None, tag=""):
  """one lookup's row bytes `ob` / exists flags against the model: exactly on a table that never evicts; on a dense bounded table a key
  the model holds may be gone (counted; it reads the default), never the other way round"""
  want, want_ex = model.lookup(ids.cpu().numpy(), defaults)
  if exact:
    np.testing.assert_array_equal(exn, want_ex, err_msg=str(tag))
    np.testing.assert_array_equal(ob, want, err_msg=str(tag))
    return 0
  assert not np.any(exn & ~want_ex), tag
  np.testing.assert_array_equal(ob[exn], want[exn], err_msg=str(tag))
  dflt = np.broadcast_to(model.default, ob.shape) if defaults is None else defaults
  np.testing.assert_array_equal(ob[~exn], dflt[~exn], err_msg=str(tag))
  return int(np.sum(~exn & want_ex))


def _check_rows(tbl, model, ids, out, ex, exact, defaults=None, tag=""):
  """a step's rows / exists flags: equal to a plain find of the table right after the call (the write-back of the previous batch is
  complete, this batch's has not started), byte for byte, and to the model"""
  ref, rex = tbl.find(ids, dynamic_default_values=defaults, return_exists=True)
  exn = ex.cpu().numpy()
  np.testing.assert_array_equal(exn, rex.cpu().numpy(), err_msg="exists vs find %s" % (tag,))
  ob = _b(out)
  np.testing.assert_array_equal(ob, _b(ref), err_msg="rows vs find %s" % (tag,))
  return _check_model(model, ids, ob, exn, exact, None if defaults is None else _b(defaults), tag)


def _cap_for(rb):
  """about 10^5 slots; fewer for wide rows (the model holds every row on the host)"""
  return int(min(120_000, max(32_768, (48 << 20) // rb)))


def _dense(torch, de, w, cap, keys, rows, default, name):
  """bounded LRU table at max_capacity, pre-filled with `rows`, known to the host as dense (runs step_k_u2)"""
  dtype = getattr(torch, w[0])
  t = de.HkvHashTable(torch.int64, dtype, default, init_capacity=cap, max_capacity=cap, device="cuda:0", dim=w[1],
                      evict_strategy=de.HkvEvictStrategy.LRU, name=name)
  k = torch.from_numpy(keys).cuda()
  for lo in range(0, k.numel(), 20000):
    t._table.upsert(k[lo:lo + 20000], rows[lo:lo + 20000], unique_keys=True)
    torch.cuda.synchronize()
  for _ in range(3):   # the host learns the density from an asynchronous size read: give it calls to complete in
    t._table.upsert(k[:16], rows[:16], unique_keys=True)
    torch.cuda.synchronize()
  return t


def _growing(torch, de, w, keys, rows, default, name):
  """CuckooHashTable: grows, never evicts (runs step_k_gen); starts at 8192 slots' worth"""
  t = de.CuckooHashTable(torch.int64, getattr(torch, w[0]), default, device="cuda:0", dim=w[1], name=name)
  t._table.upsert(torch.from_numpy(keys).cuda(), rows, unique_keys=True)
  torch.cuda.synchronize()
  return t


def _draw(rng, universe, n, sentinels=True, fresh=None):
  """Zipf ids over `universe` with a hot id, repeats, the two sentinel key values and (fresh) never-seen keys"""
  ids = universe[(rng.zipf(1.15, size=n) * 37 + rng.integers(0, 50, size=n)) % universe.size].astype(np.int64)
  if sentinels:
    ids[rng.integers(0, n, size=max(1, n // 100))] = IMIN
    ids[rng.integers(0, n, size=max(1, n // 130))] = IMIN + 1
  ids[: n // 6] = universe[7]
  if fresh is not None:
    ids[rng.choice(n, size=fresh.size, replace=False)] = fresh
  rng.shuffle(ids)
  return ids


def _setup(torch, de, w, kind, seed, n, nsteps, new_share=None):
  """table + model + batches: 'dense' = bounded LRU at capacity, 62 % of the slots used, the last 1 % of the universe entering through
  the steps (and `new_share` of every batch never-seen keys, default none); 'growing' = a cuckoo table pre-filled with 6000 keys,
  `new_share` (default 0.3) of every batch never-seen keys: it grows"""
  rng = np.random.default_rng(seed)
  dtype, dim, rb = getattr(torch, w[0]), w[1], _rb(w)
  default = _rand(torch, rng, (dim,), dtype)
  if kind == "dense":
    cap = _cap_for(rb)
    universe = rng.permutation(np.arange(1, int(cap * 0.62) + 1, dtype=np.int64)) * 7919 + 3
    resident = universe[: int(universe.size * 0.99)]
    new_share = new_share or 0.0
  else:
    universe = rng.permutation(np.arange(1, 6001, dtype=np.int64)) * 7919 + 3
    resident = universe
    new_share = 0.3 if new_share is None else new_share
  m = int(n * new_share)
  fresh = [np.arange(10_000_000 + s * m, 10_000_000 + (s + 1) * m, dtype=np.int64) * 31 + 5 if m else None for s in range(nsteps + 2)]
  pre = _rand(torch, rng, (resident.size, dim), dtype)
  name = "rw_%s_%s_%d" % (kind, _wid(w), seed)
  t = _dense(torch, de, w, cap, resident, pre, default, name) if kind == "dense" else _growing(torch, de, w, resident, pre, default, name)
  batches = [_draw(rng, universe, n, fresh=fresh[s]) for s in range(nsteps + 2)]
  allk = np.concatenate([universe, np.array([IMIN, IMIN + 1], np.int64)] + [f for f in fresh if f is not None])
  model = ByteModel(allk, rb, _b(default))
  model.assign(resident, _b(pre))
  vals = [_rand(torch, rng, (n, dim), dtype) for _ in range(nsteps + 1)]
  return t, model, [torch.from_numpy(b).cuda() for b in batches], vals


def _assert_path(st, w, nsteps_total):
  if w in SEQ:
    assert st["overlapped"] == 0 and st["why_sequential"] & 2, st
  else:
    # (the host learns that a bounded table is dense from asynchronous size reads: the first steps may run one op after the other)
    assert st["overlapped"] + st["sequential"] == nsteps_total and st["sequential"] <= 3, st
    assert st["why_sequential"] in (0, 32), st


# ---- 1. the overlapped step, dictionary-exact ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "growing"])
@pytest.mark.parametrize("w", WIDTHS, ids=_wid)
def test_overlap_step_every_byte_at_every_width(env, w, kind):
  """Next ids announced two ahead, one ahead and not at all; a hot id, repeats, both sentinel keys; a random default row.  The
  growing table grows in front of a launch during the run."""
  torch, de, _ = env
  n, nsteps = 3000, 10
  t, model, batches, vals = _setup(torch, de, w, kind, 1000 + _rb(w), n, nsteps)
  tbl = t._table
  cap0 = tbl.capacity()
  drv = de.OverlapAssignStep(t).prime(batches[0])
  evicted = 0
  for s in range(nsteps):
    nxt = batches[s + 1] if s % 4 != 3 else None                 # every fourth step: the next ids are NOT announced
    nx2 = batches[s + 2] if (nxt is not None and s % 5 != 2) else None   # ... and not always two ahead
    out, ex = drv.step(vals[s], nxt, nx2, return_exists=True)
    if nxt is None:
      drv.prime(batches[s + 1])
    evicted += _check_rows(tbl, model, batches[s], out, ex, kind == "growing", tag=(_wid(w), kind, s))
    model.assign(batches[s].cpu().numpy(), _b(vals[s]))
  assert evicted <= nsteps * n // 100, evicted
  drv.flush()
  _assert_path(drv.stats(), w, nsteps + 1)
  if kind == "growing":
    assert tbl.capacity() > cap0              # it really grew while the steps ran
  model.check_export(*t.export(), exact=kind == "growing")
  tbl.check_errors()
  assert tbl.slot_census()["locked"] == 0


# ---- 2. the tail's corrections at width ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [("float32", 4), ("float32", 68), ("float32", 128)], ids=_wid)
def test_overlap_corrections_at_width(env, w):
  """A table at capacity; a third of every batch never-seen ids (each evicts the oldest entry of its home buckets), a third the OLDEST
  resident keys — the likely victims: the write-back keeps evicting keys the next lookup asks for, and the tail copies their rows
  again (tfra_step_impl.h, the tail's correction loop).  Every returned row, corrected ones included, equals a plain find right after
  the call in full; every present key holds the bytes of its last write."""
  torch, de, _ = env
  dtype, dim, rb = getattr(torch, w[0]), w[1], _rb(w)
  cap, n, nsteps = 60_000, 3000, 30
  rng = np.random.default_rng(5 + rb)
  fill = np.arange(1, cap + 1, dtype=np.int64) * 104729 + 11
  fresh_all = np.arange(10_000_000, 10_000_000 + (nsteps + 3) * (n // 3), dtype=np.int64) * 31 + 5
  default = _rand(torch, rng, (dim,), dtype)
  pre = _rand(torch, rng, (cap, dim), dtype)
  t = _dense(torch, de, w, cap, fill, pre, default, "rw_corr_%d" % rb)
  tbl = t._table
  model = ByteModel(np.concatenate([fill, fresh_all]), rb, _b(default))
  model.assign(fill, _b(pre))
  last_write = {int(k): -1 for k in fill}
  hot = fill[rng.integers(0, cap, size=400)]
  nfresh = [0]

  def make_batch():
    a = hot[rng.zipf(1.2, size=n // 3) % hot.size]
    b = fresh_all[nfresh[0]: nfresh[0] + n // 3]
    nfresh[0] += n // 3
    oldest = np.array(sorted(last_write, key=last_write.get)[: 4 * n], np.int64)
    c = oldest[rng.integers(0, oldest.size, size=n - a.size - b.size)]
    ids = np.concatenate([a, b, c])
    rng.shuffle(ids)
    return ids

  drv = de.OverlapAssignStep(t)
  ids_np = make_batch()
  drv.prime(torch.from_numpy(ids_np).cuda())
  keep, nxt2_np, nxt2_t, prev_keys = [], None, None, None
  for s in range(nsteps):
    ids = torch.from_numpy(ids_np).cuda()
    vals = _rand(torch, rng, (n, dim), dtype)
    for k in ids_np.tolist():
      last_write[k] = s
    if s == 0:
      nxt_np = make_batch()
      nxt_t = torch.from_numpy(nxt_np).cuda()
    else:
      nxt_np, nxt_t = nxt2_np, nxt2_t
    nxt2_np = make_batch()
    nxt2_t = torch.from_numpy(nxt2_np).cuda()
    keep.append((ids, nxt_t, nxt2_t, vals))
    out, ex = drv.step(vals, nxt_t, nxt2_t, return_exists=True)
    _check_rows(tbl, model, ids, out, ex, False, tag=("corr", rb, s))
    if prev_keys is not None:
      again = np.isin(ids_np, prev_keys)
      assert again.any() and ex.cpu().numpy()[again].all()   # written one step ago: present
    model.assign(ids_np, _b(vals))
    prev_keys = np.unique(ids_np)
    ids_np = nxt_np
  drv.flush()
  st = drv.stats()
  assert st["overlapped"] + st["sequential"] == nsteps + 1 and st["overlapped"] >= nsteps - 8, st
  assert st["rows_corrected"] > 0 and st["victims_noted"] > 0, st     # the tail's correction copy really ran
  ek, ev = t.export()
  ekn = ek.cpu().numpy()
  assert np.unique(ekn).size == ekn.size == int(t.size().item()) <= tbl.capacity()
  i = model.idx(ekn)
  assert model.present[i].all()
  np.testing.assert_array_equal(_b(ev), model.rows[i])
  tbl.check_errors()
  assert tbl.slot_census()["locked"] == 0


# ---- 3. many steps per host call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [("float32", 4), ("int64", 18), ("float32", 128)], ids=_wid)
def test_make_run_equals_single_steps_bytewise(env, w):
  """tfra_table_steps_overlap (make_run): 8 steps from ONE host call on one table, the same steps one by one on its twin (growing
  tables: nothing is evicted, so the twins agree exactly) — outputs and exports byte-equal, and equal to the model."""
  torch, de, _ = env
  dtype, dim, rb = getattr(torch, w[0]), w[1], _rb(w)
  n, m = 4000, 8
  rng = np.random.default_rng(9 + rb)
  universe = rng.permutation(np.arange(1, 20001, dtype=np.int64)) * 6151 + 1
  default = _rand(torch, rng, (dim,), dtype)
  pre = _rand(torch, rng, (universe.size, dim), dtype)
  tabs = [_growing(torch, de, w, universe, pre, default, "rw_run_%d_%d" % (rb, i)) for i in range(2)]
  ids = [torch.from_numpy(_draw(rng, universe, n, sentinels=False)).cuda() for _ in range(m + 1)]
  vals = [_rand(torch, rng, (n, dim), dtype) for _ in range(m)]
  outs = [torch.empty((n, dim), dtype=dtype, device="cuda") for _ in range(m)]
  d0 = de.OverlapAssignStep(tabs[0])
  run = d0.make_run(ids[:m], vals, outs, ids_after=ids[m])
  run()
  d0.flush()
  d1 = de.OverlapAssignStep(tabs[1]).prime(ids[0])
  model = ByteModel(universe, rb, _b(default))
  model.assign(universe, _b(pre))
  for k in range(m):
    o = d1.step(vals[k], ids[k + 1])
    ob = _b(o)
    np.testing.assert_array_equal(_b(outs[k]), ob, err_msg="step %d" % k)
    want, _ = model.lookup(ids[k].cpu().numpy())
    np.testing.assert_array_equal(ob, want, err_msg="step %d" % k)
    model.assign(ids[k].cpu().numpy(), _b(vals[k]))
  d1.flush()
  assert d0.stats()["overlapped"] == m + 1 and d1.stats()["overlapped"] == m + 1, (d0.stats(), d1.stats())
  ex = []
  for t in tabs:
    k, v = t.export()
    o = torch.argsort(k)
    ex.append((k[o], v[o]))
    model.check_export(k, v, exact=True)
  assert torch.equal(ex[0][0], ex[1][0])
  np.testing.assert_array_equal(_b(ex[0][1]), _b(ex[1][1]))


# ---- 4. per-position defaults (default_is_full = 1) ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "growing"])
@pytest.mark.parametrize("w", [("float32", 4), ("float32", 68), ("float32", 260)], ids=_wid)
def test_overlap_step_per_position_defaults(env, w, kind):
  """tfra_table_step_overlap called with default_is_full = 1 (the argument order of OverlapAssignStep.step): every miss returns ITS
  position's row of the [n, dim] defaults, in the lookup role and in the tail's corrections alike."""
  torch, de, capi = env
  from tfra_amd.dynamic_embedding.table_ops import _stream
  n, nsteps = 3000, 8
  dtype, dim = getattr(torch, w[0]), w[1]
  t, model, batches, vals = _setup(torch, de, w, kind, 2000 + _rb(w), n, nsteps, new_share=0.02 if kind == "dense" else None)
  tbl = t._table
  rng = np.random.default_rng(7 + _rb(w))
  drv = de.OverlapAssignStep(t)
  fn, h = drv._fn, drv._h
  keep, prev, misses = [], None, 0      # (keep: the buffers the enqueued launches read)
  for s in range(nsteps):
    ids = batches[s]
    out = torch.empty((n, dim), dtype=dtype, device="cuda")
    ex = torch.empty(n, dtype=torch.bool, device="cuda")
    dfl = _rand(torch, rng, (n, dim), dtype)
    nxt = batches[s + 1]
    nx2 = batches[s + 2] if s % 3 != 1 else None
    capi.check(fn(h, n, _ptr(ids), _ptr(out), _ptr(ex), _ptr(dfl), 1, _ptr(prev), None, nxt.numel(), _ptr(nxt),
                  0 if nx2 is None else nx2.numel(), _ptr(nx2), _stream(torch.device("cuda:0"))))
    keep.append((ids, out, ex, dfl, prev, nxt, nx2))
    prev = vals[s]
    _check_rows(tbl, model, ids, out, ex, kind == "growing", defaults=dfl, tag=("full", _wid(w), kind, s))
    misses += int((~ex).sum())
    model.assign(ids.cpu().numpy(), _b(vals[s]))
  capi.call("tfra_table_step_overlap_flush", h, _ptr(prev), None, _stream(torch.device("cuda:0")))
  torch.cuda.synchronize()
  assert misses > nsteps          # (sentinels and never-seen ids: misses in every step)
  _assert_path(drv.stats(), w, nsteps + 1)
  model.check_export(*t.export(), exact=kind == "growing")
  tbl.check_errors()


def test_steps_overlap_struct_per_position_defaults(env):
  """The same through the tfra_overlap_step struct of the many-steps call: default_is_full = 1 and a defaults array per step."""
  torch, de, _ = env
  w = ("float32", 68)
  dtype, dim = getattr(torch, w[0]), w[1]
  n, m = 3000, 6
  t, model, batches, vals = _setup(torch, de, w, "growing", 3000, n, m)
  rng = np.random.default_rng(3)
  dfl = [_rand(torch, rng, (n, dim), dtype) for _ in range(m)]
  outs = [torch.empty((n, dim), dtype=dtype, device="cuda") for _ in range(m)]
  drv = de.OverlapAssignStep(t)
  run = drv.make_run(batches[:m], vals[:m], outs, ids_after=batches[m])
  arr = run._keep[0]
  for k in range(m):
    arr[k].default_is_full = 1
    arr[k].defaults = dfl[k].data_ptr()
  run()
  drv.flush()
  torch.cuda.synchronize()
  for k in range(m):
    ids_np = batches[k].cpu().numpy()
    want, want_ex = model.lookup(ids_np, _b(dfl[k]))
    assert (~want_ex).sum() > 0
    np.testing.assert_array_equal(_b(outs[k]), want, err_msg="step %d" % k)
    model.assign(ids_np, _b(vals[k]))
  assert drv.stats()["overlapped"] == m + 1, drv.stats()
  model.check_export(*t.export(), exact=True)


# ---- 5. the look-ahead and routed drivers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS, ids=_wid)
def test_prefetch_assign_step_every_byte(env, w):
  """PrefetchAssignStep: lookup(i) then insert_or_assign(i) per call, the next batch's plan built on a second stream."""
  torch, de, _ = env
  n, nsteps = 3000, 8
  t, model, batches, vals = _setup(torch, de, w, "dense", 4000 + _rb(w), n, nsteps)
  tbl = t._table
  ps = de.PrefetchAssignStep(t).prime(batches[0])
  evicted = 0
  for s in range(nsteps):
    ref, rex = tbl.find(batches[s], return_exists=True)     # (in stream order in front of the step: what its lookup must return)
    out = ps.step(vals[s], batches[s + 1])
    ob = _b(out)
    np.testing.assert_array_equal(ob, _b(ref), err_msg="step %d" % s)
    evicted += _check_model(model, batches[s], ob, rex.cpu().numpy(), False, tag=("prefetch", _wid(w), s))
    model.assign(batches[s].cpu().numpy(), _b(vals[s]))
  torch.cuda.synchronize()
  assert evicted <= nsteps * n // 100
  model.check_export(*t.export(), exact=False)
  tbl.check_errors()


@pytest.mark.parametrize("w", WIDTHS, ids=_wid)
def test_routed_assign_step_local_every_byte(env, w):
  """RoutedAssignStep(transport='local'): one rank THROUGH the route driver — rows and values move through the row gathers, the owner
  runs the overlapped step (or, at a width it cannot serve, the ops one after the other)."""
  torch, de, _ = env
  from tfra_amd.dynamic_embedding.distributed import RoutedAssignStep
  n, nsteps = 3000, 8
  t, model, batches, vals = _setup(torch, de, w, "dense", 5000 + _rb(w), n, nsteps)
  tbl = t._table
  rs = RoutedAssignStep(t, transport="local", max_batch=1 << 14)
  assert not rs.identity
  for k in range(3):
    rs.feed(batches[k])
  prev, evicted = None, 0
  for s in range(nsteps):
    out = rs.step(prev)
    if s + 3 < nsteps:
      rs.feed(batches[s + 3])
    torch.cuda.synchronize()
    ref, rex = tbl.find(batches[s], return_exists=True)     # the table right now = what this lookup had to reflect
    ob = _b(out)
    np.testing.assert_array_equal(ob, _b(ref), err_msg="step %d" % s)
    evicted += _check_model(model, batches[s], ob, rex.cpu().numpy(), False, tag=("routed", _wid(w), s))
    prev = vals[s]
    model.assign(batches[s].cpu().numpy(), _b(vals[s]))
  rs.flush(prev)
  torch.cuda.synchronize()
  assert evicted <= nsteps * n // 100
  st = rs.stats()
  assert st["steps"] == nsteps, st
  if w in SEQ:
    assert st["owner_overlapped"] == 0, st
  else:
    assert st["owner_overlapped"] >= nsteps - 2, st
  model.check_export(*t.export(), exact=False)
  tbl.check_errors()
  rs.close()


# ---- 6. row gathers --------------------------------------------------------------------------------------------------------------
GATHER_N = [4095, 4096, 4097, 131_073]
GATHER_CASES = [(w, n) for w in WIDTHS for n in GATHER_N if n * _rb(w) <= (160 << 20)]


@pytest.mark.parametrize("w,n", GATHER_CASES, ids=lambda x: _wid(x) if isinstance(x, tuple) else str(x))
def test_gather_scatter_rows_every_width(env, w, n):
  """device_ops.gather_rows / scatter_rows against numpy fancy indexing: at n >= 4096 a 16-byte-granule gather takes
  gather_rows16_kernel (4 rows per lane group; n not a multiple of 4 exercises its tail)."""
  torch, de, _ = env
  from tfra_amd.dynamic_embedding import device_ops
  dtype, dim = getattr(torch, w[0]), w[1]
  rng = np.random.default_rng(n + _rb(w))
  m = 3000
  src = _rand(torch, rng, (m, dim), dtype)
  idx = rng.integers(0, m, size=n).astype(np.int32)
  out = device_ops.gather_rows(src, torch.from_numpy(idx).cuda())
  np.testing.assert_array_equal(_b(out), _b(src)[idx])
  rows = _rand(torch, rng, (n, dim), dtype)
  perm = rng.permutation(n + 77)[:n].astype(np.int32)
  sc = device_ops.scatter_rows(rows, torch.from_numpy(perm).cuda(), n + 77)
  np.testing.assert_array_equal(_b(sc)[perm], _b(rows))


@pytest.mark.parametrize("side", ["in", "out"])
@pytest.mark.parametrize("off", [8, 4, 2, 1])
@pytest.mark.parametrize("w", WIDTHS, ids=_wid)
def test_gather_scatter_rows_at_byte_offsets(env, w, off, side):
  """Input or output buffer `off` bytes past an aligned address: the kernels' granule drops to 8, 4, 2, 1 bytes (move_rows).  The
  output goes into a pre-allocated view of a guarded buffer: the bytes just before and after it must be unchanged, and so must the
  rows a scatter does not address."""
  torch, de, capi = env
  from tfra_amd.dynamic_embedding import device_ops
  from tfra_amd.dynamic_embedding.table_ops import _stream
  rb = _rb(w)
  rng = np.random.default_rng(off * 100 + rb)
  n, m, guard = 4097, 3000, 64
  st = _stream(torch.device("cuda:0"))
  o_in, o_out = (off, 0) if side == "in" else (0, off)

  def place(nrows, o):   # a guarded random byte buffer and the [nrows, rb] uint8 view `o` bytes past its 16-aligned interior
    buf = _rand(torch, rng, (guard + nrows * rb + guard,), torch.uint8)
    return buf, buf[guard + o: guard + o + nrows * rb].view(nrows, rb)

  # gather
  sbuf, src = place(m, o_in)
  obuf, outv = place(n, o_out)
  before = obuf.cpu().numpy()
  idx = rng.integers(0, m, size=n).astype(np.int32)
  if side == "in":
    got = device_ops.gather_rows(src, torch.from_numpy(idx).cuda())     # (the wrapper takes an input view as it is)
    np.testing.assert_array_equal(got.cpu().numpy(), src.cpu().numpy()[idx])
  idx_t = torch.from_numpy(idx).cuda()
  capi.call("tfra_gather_rows", n, rb, _ptr(src), _ptr(idx_t), _ptr(outv), st)
  after = obuf.cpu().numpy()
  np.testing.assert_array_equal(after[guard + o_out: guard + o_out + n * rb].reshape(n, rb), src.cpu().numpy()[idx])
  np.testing.assert_array_equal(after[: guard + o_out], before[: guard + o_out])
  np.testing.assert_array_equal(after[guard + o_out + n * rb:], before[guard + o_out + n * rb:])
  # scatter: n rows into n + 77 (the rows not addressed keep their bytes)
  rbuf, rows = place(n, o_in)
  obuf, outv = place(n + 77, o_out)
  before = obuf.cpu().numpy()
  perm = rng.permutation(n + 77)[:n].astype(np.int32)
  perm_t = torch.from_numpy(perm).cuda()
  capi.call("tfra_scatter_rows", n, rb, _ptr(rows), _ptr(perm_t), _ptr(outv), st)
  after = obuf.cpu().numpy()
  want = before[guard + o_out: guard + o_out + (n + 77) * rb].reshape(n + 77, rb).copy()
  want[perm] = rows.cpu().numpy()
  np.testing.assert_array_equal(after[guard + o_out: guard + o_out + (n + 77) * rb].reshape(n + 77, rb), want)
  np.testing.assert_array_equal(after[: guard + o_out], before[: guard + o_out])
  np.testing.assert_array_equal(after[guard + o_out + (n + 77) * rb:], before[guard + o_out + (n + 77) * rb:])


# ---- 7. offset buffers through the table and the step ----------------------------------------------------------------------------
def _at_offset(torch, x, k):
  """a copy of x in a buffer of its dtype, k elements past the start: same values, a (k * element size)-byte offset"""
  buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=x.device)
  v = buf[k: k + x.numel()].view(x.shape)
  v.copy_(x)
  return v


# 272-byte rows, at a 4-byte (fp32, one element) and a 2-byte (fp16, one element) offset
OFFSET_CASES = [(("float32", 68), 1), (("float16", 136), 1)]


@pytest.mark.parametrize("w,k", OFFSET_CASES, ids=["f32_4B", "f16_2B"])
def test_table_ops_with_offset_buffers(env, w, k):
  """upsert / upsert_sparse values, find defaults (one row and per position) and find's output as views at a 4- or 2-byte offset:
  byte-equal to the same calls with aligned buffers on a twin table, and to the model."""
  torch, de, capi = env
  from tfra_amd.dynamic_embedding.table_ops import _stream
  dtype, dim, rb = getattr(torch, w[0]), w[1], _rb(w)
  assert (k * ESIZE[w[0]]) % 16 != 0 and rb % 16 == 0
  rng = np.random.default_rng(rb + k)
  default = _rand(torch, rng, (dim,), dtype)
  tabs = [de.HkvHashTable(torch.int64, dtype, default, init_capacity=1 << 15, max_capacity=1 << 20, device="cuda:0", dim=dim,
                          evict_strategy=de.HkvEvictStrategy.LRU, name="rw_off_%s_%d" % (w[0], i)) for i in range(2)]
  keys = rng.permutation(np.arange(1, 8001, dtype=np.int64)) * 7919 + 3
  model = ByteModel(np.concatenate([keys, np.arange(1, 40, dtype=np.int64) * -3]), rb, _b(default))
  kt = torch.from_numpy(keys).cuda()
  v1 = _rand(torch, rng, (keys.size, dim), dtype)
  tabs[0]._table.upsert(kt, v1, unique_keys=True)
  tabs[1]._table.upsert(kt, _at_offset(torch, v1, k), unique_keys=True)
  model.assign(keys, _b(v1))
  ids2 = np.concatenate([keys[rng.integers(0, 3000, size=3500)], np.arange(1, 40, dtype=np.int64) * -3])
  rng.shuffle(ids2)
  i2 = torch.from_numpy(ids2).cuda()
  v2 = _rand(torch, rng, (ids2.size, dim), dtype)
  tabs[0]._table.upsert_sparse(i2, v2)
  tabs[1]._table.upsert_sparse(i2, _at_offset(torch, v2, k))
  model.assign(ids2, _b(v2))
  v3 = _rand(torch, rng, (2000, dim), dtype)   # a plain upsert, not flagged unique
  i3 = torch.from_numpy(keys[rng.choice(keys.size, size=2000, replace=False)]).cuda()
  tabs[0]._table.upsert(i3, v3)
  tabs[1]._table.upsert(i3, _at_offset(torch, v3, k))
  model.assign(i3.cpu().numpy(), _b(v3))
  q = np.concatenate([keys[rng.integers(0, keys.size, size=3000)], np.arange(100, 400, dtype=np.int64) * 13 + 1000_000_001])
  model_keys = np.union1d(model.keys, q)
  m2 = ByteModel(model_keys, rb, model.default)
  m2.assign(model.keys[model.present], model.rows[model.present])
  qt = torch.from_numpy(q).cuda()
  dfl_full = _rand(torch, rng, (q.size, dim), dtype)
  dfl_row = _rand(torch, rng, (dim,), dtype)
  for dfl in (None, dfl_row, dfl_full):
    a, ea = tabs[0]._table.find(qt, dynamic_default_values=dfl, return_exists=True)
    b, eb = tabs[1]._table.find(qt, dynamic_default_values=None if dfl is None else _at_offset(torch, dfl, k), return_exists=True)
    assert torch.equal(ea, eb)
    np.testing.assert_array_equal(_b(a), _b(b))
    dfb = None if dfl is None else (_b(dfl) if dfl.dim() == 2 else np.broadcast_to(_b(dfl), (q.size, rb)))
    want, want_ex = m2.lookup(q, dfb)
    np.testing.assert_array_equal(ea.cpu().numpy(), want_ex)
    np.testing.assert_array_equal(_b(a), want)
    # find's output at the offset too (the op allocates its own: the C entry point with a pre-allocated view)
    outv = _at_offset(torch, torch.zeros((q.size, dim), dtype=dtype, device="cuda"), k)
    exv = torch.empty(q.size, dtype=torch.bool, device="cuda")
    d = tabs[1]._table._default_value if dfl is None else _at_offset(torch, dfl, k)
    capi.call("tfra_table_find", tabs[1]._table._h, q.size, _ptr(qt), _ptr(outv), _ptr(exv), _ptr(d), int(dfl is not None and dfl.dim() == 2),
              _stream(torch.device("cuda:0")))
    np.testing.assert_array_equal(_b(outv), want)
    np.testing.assert_array_equal(exv.cpu().numpy(), want_ex)
  for t in tabs:
    model.check_export(*t.export(), exact=True)
    t._table.check_errors()


@pytest.mark.parametrize("w,k", OFFSET_CASES, ids=["f32_4B", "f16_2B"])
def test_overlap_step_with_offset_values_falls_back(env, w, k):
  """OverlapAssignStep with `values` at a 4- or 2-byte offset: not 16-byte aligned, so a step that writes them back does not take the
  overlapped launch (why_sequential bit 2) — and the results are the model's all the same."""
  torch, de, _ = env
  n, nsteps = 3000, 6
  t, model, batches, vals = _setup(torch, de, w, "growing", 6000 + _rb(w) + k, n, nsteps)
  drv = de.OverlapAssignStep(t).prime(batches[0])
  keep = []
  for s in range(nsteps):
    v = _at_offset(torch, vals[s], k)
    keep.append(v)
    out, ex = drv.step(v, batches[s + 1], batches[s + 2], return_exists=True)
    _check_rows(t._table, model, batches[s], out, ex, True, tag=("offset", s))
    model.assign(batches[s].cpu().numpy(), _b(vals[s]))
  drv.flush()
  st = drv.stats()
  # (the first call has nothing to write back — a lookup-only launch; every call that writes offset values back runs sequentially)
  assert st["overlapped"] == 1 and st["sequential"] == nsteps and st["why_sequential"] & 2, st
  model.check_export(*t.export(), exact=True)
  t._table.check_errors()
