"""GPU: tfra_multi_unique / device_ops.unique_many — many id lists' tf.unique in one call.

Expected values: oracle.frontends.unique, the first-occurrence model tests/test_gpu_frontend.py uses; every list is also compared
byte for byte with device_ops.unique_no_sync on the same ids (uniq[:cnt], idx, cnt).  The shapes are the smallest at which the
kernels can go wrong: the insert block edge (512), the scatter tile edge (1024), a look-back over several tiles behind other
lists' tiles, lists without blocks, INT64_MIN (the sets' sentinel) in several lists of one call, layouts that change from call to
call over the two self-emptying sets, the staging ring's reuse, the parity and the generation."""
import ctypes

import numpy as np
import pytest

from oracle import frontends as ofe

pytestmark = pytest.mark.gpu

IMIN = np.iinfo(np.int64).min
SENT = -7          # what the raw calls' output buffers hold before the call
EDGES = [1, 511, 512, 513, 1023, 1024, 1025, 4097]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ids(rng, n, spread=None):
  """n ids with repeats (about two positions per distinct id) around zero"""
  hi = max(1, (n // 4) if spread is None else spread)
  return rng.integers(-hi, hi + 1, size=n).astype(np.int64)


def _check(torch, de, got, ids, tag=""):
  """one member (uniq, idx or None, cnt) against the model and against unique_no_sync"""
  uniq, idx, cnt = got
  eu, eidx = ofe.unique(ids)
  c = int(cnt.item())
  assert c == eu.size, (tag, c, eu.size)
  assert uniq.numel() == ids.size
  np.testing.assert_array_equal(uniq[:c].cpu().numpy(), eu, err_msg=str(tag))
  su, sidx, scnt = de.device_ops.unique_no_sync(T(torch, ids))
  assert int(scnt.item()) == c and torch.equal(su[:c], uniq[:c]), tag
  if idx is not None:
    assert idx.dtype == torch.int32
    np.testing.assert_array_equal(idx.cpu().numpy(), eidx, err_msg=str(tag))
    assert torch.equal(sidx, idx), tag


def _many(torch, de, lists, **kw):
  res = de.device_ops.unique_many([T(torch, a) for a in lists], **kw)
  out = res[0] if kw.get("return_launches") else res
  assert len(out) == len(lists)
  return res


class Raw:
  """tfra_multi_unique itself over buffers of the test's own, filled with SENT first"""

  def __init__(self, torch, de, lists, want=None, n_says=None, ids_t=None):
    from tfra_amd import _capi
    from tfra_amd.dynamic_embedding import _args
    self.torch, self.capi, self.args, self.de = torch, _capi, _args, de
    self.lists = lists
    want = [True] * len(lists) if want is None else want
    self.ids = ids_t if ids_t is not None else [T(torch, a) for a in lists]
    self.uniq = [torch.full((max(1, a.size),), SENT, dtype=torch.int64, device="cuda") for a in lists]
    self.idx = [torch.full((max(1, a.size),), SENT, dtype=torch.int32, device="cuda") for a in lists]
    self.cnt = torch.full((len(lists),), SENT, dtype=torch.int64, device="cuda")
    self.descs = (_capi.UniqueDesc * len(lists))()
    for k, a in enumerate(lists):
      e = self.descs[k]
      e.struct_size, e.flags = ctypes.sizeof(_capi.UniqueDesc), 0
      e.n = a.size if n_says is None else n_says[k]
      e.ids, e.unique_out = (self.ids[k].data_ptr(), self.uniq[k].data_ptr()) if a.size else (None, None)
      e.idx_out = self.idx[k].data_ptr() if (want[k] and a.size) else None
      e.d_num_unique = self.cnt[k:].data_ptr()
    self.want = want

  def call(self):
    dev = self.torch.device("cuda", self.torch.cuda.current_device())
    launches = ctypes.c_uint32(99)
    rc = self.capi.lib().tfra_multi_unique(self.de.device_ops._workspace(dev), len(self.lists), ctypes.c_void_p(ctypes.addressof(self.descs)),
                                           ctypes.byref(launches), self.args._stream(dev))
    return rc, launches.value, self.capi.lib().tfra_last_error().decode()

  def untouched(self):
    self.torch.cuda.synchronize()
    return all(bool((b == SENT).all()) for b in self.uniq + self.idx + [self.cnt])

  def check(self, tag=""):
    for k, a in enumerate(self.lists):
      idx = self.idx[k][:a.size] if self.want[k] else None
      if a.size == 0:
        assert int(self.cnt[k].item()) == 0, (tag, k)            # written: the buffer held SENT
        assert bool((self.uniq[k] == SENT).all()) and bool((self.idx[k] == SENT).all())
        continue
      _check(self.torch, self.de, (self.uniq[k][:a.size], idx, self.cnt[k]), a, (tag, k))
      if not self.want[k]:
        assert bool((self.idx[k] == SENT).all()), (tag, k, "an index was written where none was asked for")


# ---- boundaries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["last", "first", "twice"])
def test_block_and_tile_edges_with_empty_members(env, where):
  torch, de = env
  rng = np.random.default_rng(11)
  lists = [_ids(rng, n) for n in EDGES]
  empty = np.zeros(0, np.int64)
  lists = {"last": lists + [empty], "first": [empty] + lists, "twice": lists[:4] + [empty, empty] + lists[4:]}[where]
  r = Raw(torch, de, lists)
  rc, launches, msg = r.call()
  assert rc == 0 and launches == 3, msg
  r.check(where)


def test_a_call_of_empty_lists_only_writes_their_counts(env):
  torch, de = env
  r = Raw(torch, de, [np.zeros(0, np.int64)] * 3)
  rc, launches, msg = r.call()
  assert rc == 0 and launches <= 1, msg
  r.check("empty")
  res = _many(torch, de, [np.zeros(0, np.int64), np.array([5, 5, 4], np.int64)])
  assert int(res[0][2].item()) == 0 and res[0][0].numel() == 0 and res[0][1].numel() == 0
  _check(torch, de, res[1], np.array([5, 5, 4], np.int64))


# ---- independence ----------------------------------------------------------------------------------------------------------------
def test_lists_are_independent(env):
  torch, de = env
  rng = np.random.default_rng(12)
  base = _ids(rng, 2000)
  lists = [base, base[::-1].copy(), rng.permutation(base)]
  for got, a in zip(_many(torch, de, lists), lists):
    _check(torch, de, got, a, "same ids")
  # two descriptors that read ONE ids buffer
  shared = T(torch, base)
  r = Raw(torch, de, [base, base], ids_t=[shared, shared])
  rc, launches, msg = r.call()
  assert rc == 0 and launches == 3, msg
  r.check("shared ids")
  # ids that agree in their low 20 bits, the same ones in every list
  lists = [(rng.integers(0, 700, size=n).astype(np.int64) << 20) for n in (1500, 1024, 700)]
  for got, a in zip(_many(torch, de, lists), lists):
    _check(torch, de, got, a, "low bits")


def test_the_sentinel_value_is_an_id_of_each_list(env):
  torch, de = env
  rng = np.random.default_rng(13)
  a, b, c = _ids(rng, 1500), _ids(rng, 1100), _ids(rng, 600)
  a[0] = IMIN; a[700:720] = IMIN; a[-1] = IMIN; a[5] = 0; a[6] = -1
  b[-1] = IMIN; b[0] = -1; b[1] = 0
  c[300] = IMIN; c[301] = IMIN
  d = np.full(3, IMIN, np.int64)
  lists = [a, b, _ids(rng, 900), c, d]
  for k, (got, x) in enumerate(zip(_many(torch, de, lists), lists)):
    _check(torch, de, got, x, ("sentinel", k))


def test_repeats(env):
  torch, de = env
  rng = np.random.default_rng(14)
  lists = [np.full(3000, 42, np.int64), rng.permutation(3000).astype(np.int64) - 1500,
           (rng.zipf(1.2, size=8192 * 4) % 1_000_000).astype(np.int64)]
  for k, (got, x) in enumerate(zip(_many(torch, de, lists), lists)):
    _check(torch, de, got, x, ("repeats", k))
  assert int(_many(torch, de, lists)[0][2].item()) == 1


# ---- state across calls ------------------------------------------------------------------------------------------------------------
def test_layouts_change_from_call_to_call(env):
  """X, then Y (more lists, other lengths), then X: every call exact — the other set is emptied through absolute slots —, with
  tfra_unique and tfra_table_find_unique of the same workspace and stream in between."""
  torch, de = env
  rng = np.random.default_rng(15)
  X = [_ids(rng, n) for n in (3000, 17, 1025)]
  Y = [_ids(rng, n) for n in (5, 2100, 640, 1, 4097, 333, 1024)]
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(4), device="cuda:0", dim=4, name="um_fu")
  t._table.upsert(torch.arange(50, device="cuda"), torch.ones(50, 4, device="cuda"), unique_keys=True)
  for step, lists in enumerate((X, Y, X, X, Y, Y, X)):
    for k, (got, a) in enumerate(zip(_many(torch, de, lists), lists)):
      _check(torch, de, got, a, ("layouts", step, k))          # (unique_no_sync on the same stream: inside _check)
    probe = _ids(rng, 900, spread=40)
    rows, uniq, idx, cnt = t._table.find_unique(T(torch, probe))
    c = int(cnt.item())
    assert c == np.unique(probe).size
    np.testing.assert_array_equal(uniq[:c].cpu().numpy()[idx.cpu().numpy()], probe)


def test_forty_calls_back_to_back(env):
  """nothing read in between: the staging ring's slots come round five times, parity and generation step every call"""
  torch, de = env
  rng = np.random.default_rng(16)
  shapes = [(700, 1030), (5, 2100, 640), (1024,), (1, 1, 3000, 12)]
  calls = []
  for step in range(40):
    lists = [_ids(rng, n) for n in shapes[step % len(shapes)]]
    calls.append((lists, _many(torch, de, lists, want_idx=(step % 3 != 0))))
  for lists, res in calls[-3:]:
    for k, (got, a) in enumerate(zip(res, lists)):
      _check(torch, de, got, a, ("forty", k))


# ---- want_idx ----------------------------------------------------------------------------------------------------------------------
def test_without_the_inverse_index(env):
  torch, de = env
  rng = np.random.default_rng(17)
  lists = [_ids(rng, n) for n in (1500, 513, 2049)]
  with_idx, l3 = _many(torch, de, lists, return_launches=True)
  without, l2 = _many(torch, de, lists, want_idx=False, return_launches=True)
  assert (l3, l2) == (3, 2)
  for k, (a, b, x) in enumerate(zip(with_idx, without, lists)):
    assert b[1] is None and a[1] is not None
    _check(torch, de, a, x, ("idx", k))
    _check(torch, de, b, x, ("no idx", k))
  many = [_ids(rng, 300 + 7 * k) for k in range(26)]
  res, launches = _many(torch, de, many, return_launches=True)
  assert launches == 3
  for k, (got, x) in enumerate(zip(res, many)):
    _check(torch, de, got, x, ("26", k))
  assert _many(torch, de, many, want_idx=False, return_launches=True)[1] == 2
  # some members with an index, some without: the buffers beside the NULL members stay as they were
  r = Raw(torch, de, lists, want=[True, False, True])
  rc, launches, msg = r.call()
  assert rc == 0 and launches == 3, msg
  r.check("mixed")


def test_int32_ids_keep_their_dtype(env):
  torch, de = env
  rng = np.random.default_rng(18)
  lists = [_ids(rng, n) for n in (1500, 33, 1024)]
  wide = de.device_ops.unique_many([T(torch, a) for a in lists])
  narrow = de.device_ops.unique_many([T(torch, a.astype(np.int32)) for a in lists[:2]] + [T(torch, lists[2])])
  assert [r[0].dtype for r in narrow] == [torch.int32, torch.int32, torch.int64]
  for k, (w, n, a) in enumerate(zip(wide, narrow, lists)):
    c = int(w[2].item())
    assert int(n[2].item()) == c and torch.equal(n[0][:c].to(torch.int64), w[0][:c]) and torch.equal(n[1], w[1])
    _check(torch, de, w, a, ("wide", k))
    su, sidx, scnt = de.device_ops.unique_no_sync(T(torch, a.astype(np.int32)) if k < 2 else T(torch, a))
    assert su.dtype == n[0].dtype and torch.equal(su[:c], n[0][:c])


def test_lists_on_two_devices_are_refused(env):
  torch, de = env
  with pytest.raises(ValueError):
    de.device_ops.unique_many([torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64)])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["struct_size", "flags", "null_ids", "null_count", "overlap", "long_list", "total"])
def test_a_refused_call_writes_nothing(env, what):
  torch, de = env
  rng = np.random.default_rng(19)
  lists = [_ids(rng, n) for n in (600, 1025, 40)]
  n_says, at = None, 1
  if what == "long_list":                      # the descriptor's n says so, over small buffers: refused before any access
    n_says = [600, (1 << 20) + 1, 40]
  if what == "total":
    lists = [_ids(rng, 64) for _ in range(6)]
    n_says, at = [1 << 20] * 4 + [1, 64], 4    # 2^22 fits; one id more does not
  r = Raw(torch, de, lists, n_says=n_says)
  if what == "struct_size":
    r.descs[1].struct_size -= 8
  elif what == "flags":
    r.descs[1].flags = 1
  elif what == "null_ids":
    r.descs[1].ids = None
  elif what == "null_count":
    r.descs[1].d_num_unique = None
  elif what == "overlap":
    at = 2
    r.descs[2].unique_out = r.uniq[0][560:].data_ptr()       # its 40 ids' range lies inside list 0's
  rc, launches, msg = r.call()
  assert rc == -1 and launches == 0, (rc, launches, msg)
  assert "multi_unique" in msg and "descriptor %d" % at in msg, msg
  assert r.untouched()
  lists = [_ids(rng, n) for n in (600, 1025, 40)]
  ok = Raw(torch, de, lists)
  rc, launches, msg = ok.call()
  assert rc == 0 and launches == 3, msg
  ok.check("after " + what)
