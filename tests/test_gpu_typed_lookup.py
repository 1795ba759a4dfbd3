"""GPU: the typed lookups at the C-call level, through table_ops (tfra_table_find_typed, tfra_table_find_combine_typed,
tfra_table_find_combine_ragged_typed and the two grouped forms; include/tfra_mi355x.h, tfra_rows_out).

The contract under test: a typed call equals its untyped twin followed by the elementwise conversion of the twin's output, BIT FOR
BIT.  The conversion is the NumPy model of tests/typed_out_model.py (checked without a GPU by tests/test_typed_out_model.py); the
comparison rule is numeric_edges.assert_bits': expected not NaN -> equal bits, expected NaN -> a NaN.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from tests import numeric_edges as ne
from tests import probe_model as pm
from tests import typed_out_model as tom
from tests.sparse_helpers import COMB, T

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
DTYPES = ("float32", "float16", "bfloat16")
HALVES = ("float16", "bfloat16")
CANARY = 0x5a


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  from tfra_amd import _capi
  assert (_capi.lib().tfra_abi_version(), INVALID) == (1, -1)
  return torch, de


def _dt(torch, name):
  return getattr(torch, name)


def _dev_table(torch, vdtype, dim, name, default=0.375, **kw):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  dt = _dt(torch, vdtype)
  return _DeviceTable(torch.int64, dt, torch.full((dim,), default, dtype=dt), name, "cuda:0", dim=dim, **kw)


def _expect(torch, twin_out, out_dtype):
  """The model applied to the twin's output -> a CPU tensor of the output type."""
  return tom.convert_tensor(torch, twin_out, _dt(torch, out_dtype))


def _check(torch, got, twin_out, out_dtype, what):
  assert got.dtype == _dt(torch, out_dtype) and tuple(got.shape) == tuple(twin_out.shape), (what, got.dtype, tuple(got.shape))
  ne.assert_bits(torch, got, _expect(torch, twin_out, out_dtype), what)


# ---- 1. the storage set through find ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def storage_table(env):
  """A float32 table whose 9 120 rows of dim 64 hold numeric_edges.storage_values() (583 680 values), and its keys."""
  torch, de = env
  rows = ne.pack_rows(ne.storage_values(), 64)
  assert rows.shape == (9120, 64)
  keys = ne.row_keys(rows.shape[0])
  t = _dev_table(torch, "float32", 64, "typed_storage")
  t.upsert(T(torch, keys), T(torch, rows))
  assert t.size_host() == rows.shape[0]
  return t, T(torch, keys), rows


@pytest.mark.parametrize("out", HALVES)
def test_storage_set_through_find(env, storage_table, out):
  torch, _ = env
  t, keys, rows = storage_table
  got = t.find(keys, out_dtype=_dt(torch, out))
  assert got.dtype == _dt(torch, out)
  want = tom.narrow_bits(rows, out)
  bad = tom.bits_mismatch(got.cpu().view(torch.int16).numpy().view(np.uint16), want, out)
  assert not bad.any(), "%d of %d values differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[:4].tolist())
  # and the same against the twin's own output
  _check(torch, got, t.find(keys), out, "find float32 -> " + out)


@pytest.fixture(scope="module")
def half_tables(env):
  """A float16 and a bfloat16 table, each holding all 65 536 bit patterns of its type in 1 024 rows of dim 64."""
  torch, _ = env
  bits16 = np.arange(65536, dtype=np.uint16).reshape(1024, 64)
  keys = T(torch, ne.row_keys(1024, stride=104729, base=-5))
  out = {}
  for vd in HALVES:
    t = _dev_table(torch, vd, 64, "typed_allbits_" + vd)
    t.upsert(keys, T(torch, bits16.view(np.int16)).view(_dt(torch, vd)))
    out[vd] = t
  return out, keys, bits16


@pytest.mark.parametrize("vd", HALVES)
def test_every_half_pattern_read_out_as_float32_and_as_the_other_half(env, half_tables, vd):
  torch, _ = env
  tabs, keys, bits16 = half_tables
  t = tabs[vd]
  stored = t.find(keys)
  assert np.array_equal(stored.cpu().view(torch.int16).numpy().view(np.uint16), bits16)   # (the twin stores and returns the patterns)
  up = t.find(keys, out_dtype=torch.float32)
  assert up.dtype == torch.float32
  want = tom.widen_bits(bits16, vd)
  bad = tom.bits_mismatch(up.cpu().numpy().view(np.uint32), want.view(np.uint32), "float32")
  assert not bad.any(), "up-cast of %s: %d patterns differ" % (vd, bad.sum())
  other = HALVES[1 - HALVES.index(vd)]
  cross = t.find(keys, out_dtype=_dt(torch, other))
  bad = tom.bits_mismatch(cross.cpu().view(torch.int16).numpy().view(np.uint16), tom.narrow_bits(want, other), other)
  assert not bad.any(), "%s read out as %s: %d patterns differ" % (vd, other, bad.sum())


# ---- 2. the storage set through the pooled calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", HALVES)
@pytest.mark.parametrize("form", ["tuple", "ragged"])
def test_storage_set_through_the_pooled_calls(env, storage_table, form, out):
  """One entry per row, weight 1, sum: the twin's float32 output is acc = 0 + 1 * x (whatever that does to a -0.0 is the twin's)."""
  torch, _ = env
  t, keys, rows = storage_table
  n = keys.numel()
  od = _dt(torch, out)
  if form == "tuple":
    seg = torch.arange(n, dtype=torch.int64, device="cuda")
    twin = t.find_combine(keys, seg, None, COMB["sum"], n)
    got = t.find_combine_typed(keys, seg, None, COMB["sum"], n, out_dtype=od)
  else:
    rs = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    twin = t.find_combine_ragged(rs, keys, None, COMB["sum"])
    got = t.find_combine_ragged(rs, keys, None, COMB["sum"], out_dtype=od)
  assert twin.dtype == torch.float32
  _check(torch, got, twin, out, "%s pooled storage set -> %s" % (form, out))


# ---- 3. find shapes ---------------------------------------------------------------------------------------------------------------
_FIND_TABLES = {}


def _find_table(torch, vd, dim):
  """200 resident keys with random rows (finite; edge values are section 1's business), default row 0.375."""
  if (vd, dim) not in _FIND_TABLES:
    t = _dev_table(torch, vd, dim, "typed_find_%s_%d" % (vd, dim))
    keys = np.arange(200, dtype=np.int64) * 7919 - 700_000
    g = torch.Generator(device="cuda").manual_seed(dim + len(vd))
    t.upsert(T(torch, keys), (torch.randn((200, dim), generator=g, device="cuda") * 3).to(_dt(torch, vd)))
    _FIND_TABLES[(vd, dim)] = (t, keys)
  return _FIND_TABLES[(vd, dim)]


PAIRS = [(i, o) for i in DTYPES for o in DTYPES if i != o]


@pytest.mark.parametrize("dim", [4, 8, 64, 68, 128, 132, 256])
@pytest.mark.parametrize("vd,out", PAIRS)
def test_find_shapes(env, vd, out, dim):
  torch, _ = env
  t, resident = _find_table(torch, vd, dim)
  od, vdt = _dt(torch, out), _dt(torch, vd)
  rng = np.random.default_rng(dim)
  for n in (1, 15, 16, 17, 67):
    keys = np.where(rng.random(n) < 0.7, rng.choice(resident, n), rng.integers(1, 1 << 40, n)).astype(np.int64)   # hits, repeats, misses
    kt = T(torch, keys)
    # one default row
    twin, ex_t = t.find(kt, return_exists=True)
    got, ex = t.find(kt, return_exists=True, out_dtype=od)
    _check(torch, got, twin, out, "find %s -> %s dim %d n %d" % (vd, out, dim, n))
    assert torch.equal(ex, ex_t) and bool(ex.any()) == bool(np.isin(keys, resident).any())
    # full defaults: one row per key, in the table's value dtype
    d = (torch.randn((n, dim), device="cuda") * 5).to(vdt)
    _check(torch, t.find(kt, d, out_dtype=od), t.find(kt, d), out, "find %s -> %s dim %d n %d, full defaults" % (vd, out, dim, n))


@pytest.mark.parametrize("vd,out", PAIRS)
def test_find_typed_device_count_keeps_the_canary_beyond_it(env, vd, out):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  torch, _ = env
  dim, n, served = 68, 67, 41
  t, resident = _find_table(torch, vd, dim)
  od = _dt(torch, out)
  kt = T(torch, np.resize(resident, n))
  rows = torch.full((n, dim), 0, dtype=od, device="cuda")
  rows.view(torch.uint8).fill_(CANARY)
  exists = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
  cnt = torch.tensor([served], dtype=torch.int64, device="cuda")
  ro = _capi.RowsOut(rows.data_ptr(), {"float32": 0, "float16": 1, "bfloat16": 2}[out], 0)
  _capi.call("tfra_table_find_typed", t._h, n, _ptr(cnt), _ptr(kt), ctypes.byref(ro), _ptr(exists), _ptr(t._default_value), 0,
             _stream(t.device))
  twin = t.find(kt[:served])
  _check(torch, rows[:served], twin, out, "find_typed with a device count")
  assert bool((rows[served:].contiguous().view(torch.uint8) == CANARY).all()) and bool((exists[served:] == 7).all())
  assert bool((exists[:served] == 1).all())


@pytest.mark.parametrize("vd,out", [("float32", "bfloat16"), ("float16", "float32"), ("bfloat16", "float16")])
def test_find_typed_on_a_bounded_table_near_capacity(env, vd, out):
  """A bounded table at its capacity holding > 60 % of its slots: find_impl's rule then puts both home-bucket lines of a key in
  flight (the PF1 instantiations)."""
  torch, de = env
  dim, cap = 64, 8192
  dt = _dt(torch, vd)
  t = de.HkvHashTable(torch.int64, dt, torch.full((dim,), 0.25, dtype=dt), name="typed_dense_%s" % vd, init_capacity=cap,
                      max_capacity=cap, max_hbm_for_values=1 << 28, evict_strategy=de.HkvEvictStrategy.LRU, dim=dim)
  keys = np.arange(1, 7601, dtype=np.int64) * 104729
  g = torch.Generator(device="cuda").manual_seed(3)
  for a in range(0, keys.size, 1900):   # several calls: the asynchronous size read that sets the flag completes between them
    t.insert(T(torch, keys[a:a + 1900]), torch.randn((1900, dim), generator=g, device="cuda").to(dt))
    torch.cuda.synchronize()
  probe = T(torch, np.concatenate([keys[::3], -keys[:500]]))
  for _ in range(2):
    twin, ex_t = t._table.find(probe, return_exists=True)
    got, ex = t._table.find(probe, return_exists=True, out_dtype=_dt(torch, out))
  _check(torch, got, twin, out, "find on a dense bounded table %s -> %s" % (vd, out))
  assert torch.equal(ex, ex_t) and bool(ex.any()) and not bool(ex.all())


def test_find_typed_on_crafted_home_bucket_collisions(env):
  """60 keys that share one (b0, b1) pair: an overflow chain four buckets deep, read through the typed find."""
  torch, _ = env
  dim = 8
  t = _dev_table(torch, "float32", dim, "typed_chain", init_capacity=1000)
  nb = (t.capacity() - 2) // pm.SLOTS
  pair = pm.craft(nb, b0=nb // 4, b1=nb // 2, count=70)
  keys, absent = pair[:60], pair[60:]
  g = torch.Generator(device="cuda").manual_seed(11)
  t.upsert(T(torch, keys), torch.randn((60, dim), generator=g, device="cuda"), unique_keys=True)
  assert (t.capacity() - 2) // pm.SLOTS == nb and t.slot_census()["ovf1"] > 0   # it did not grow: the chain is there
  probe = T(torch, np.concatenate([keys, absent]))
  twin, ex_t = t.find(probe, return_exists=True)
  for out in HALVES:
    got, ex = t.find(probe, return_exists=True, out_dtype=_dt(torch, out))
    _check(torch, got, twin, out, "find over an overflow chain -> " + out)
    assert torch.equal(ex, ex_t) and int(ex.sum()) == 60


# ---- 4. pooled shapes -------------------------------------------------------------------------------------------------------------
def _pooled_case(resident, n_rows, per_row, weighted, seed):
  """(ids, row_splits, seg, w): every row has `per_row` entries but the middle one (when there are three or more), which is empty."""
  rng = np.random.default_rng(seed)
  counts = np.full(n_rows, per_row)
  if n_rows >= 3:
    counts[n_rows // 2] = 0
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  nnz = int(rs[-1])
  ids = np.where(rng.random(nnz) < 0.8, rng.choice(resident, nnz), rng.integers(1, 1 << 40, nnz)).astype(np.int64)
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  w = None
  if weighted:
    w = rng.standard_normal(nnz).astype(np.float32)
    w[rng.random(nnz) < 0.3] = 0.0      # PRUNE has something to prune; a row may lose every member
    if nnz:
      w[:per_row] = -1.0                # row 0: no member under PRUNE (FILL's business)
  return ids, rs, seg, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("dim", [4, 64, 68, 128, 132, 256])
def test_pooled_shapes(env, dim, combiner, weighted):
  torch, _ = env
  c = COMB[combiner]
  for vd in DTYPES:
    t, resident = _find_table(torch, vd, dim)
    fill_hit, fill_miss = int(resident[3]), 987654321
    for n_rows in (1, 5, 37):
      for per_row in (0, 1, 3, 17, 40):
        ids, rs, seg, w = _pooled_case(resident, n_rows, per_row, weighted, dim * 100 + n_rows * 7 + per_row)
        it, rt, st = T(torch, ids), T(torch, rs), T(torch, seg)
        wt = None if w is None else T(torch, w)
        twin = t.find_combine(it, st, wt, c, n_rows)
        twins = {(False, None): t.find_combine_ragged(rt, it, wt, c)}
        if per_row in (0, 17):   # the safe kernels: PRUNE, FILL (hit and miss of the fill id) and both; FILL is the second store site
          for key in ((True, None), (False, fill_hit), (False, fill_miss), (True, fill_hit)):
            twins[key] = t.find_combine_ragged(rt, it, wt, c, prune=key[0], fill_id=key[1])
        for out in HALVES:
          od = _dt(torch, out)
          what = "%s -> %s dim %d rows %d x %d %s%s" % (vd, out, dim, n_rows, per_row, combiner, " weighted" if weighted else "")
          _check(torch, t.find_combine_typed(it, st, wt, c, n_rows, out_dtype=od), twin, out, "find_combine " + what)
          for (prune, fill), tw in twins.items():
            got = t.find_combine_ragged(rt, it, wt, c, prune=prune, fill_id=fill, out_dtype=od)
            _check(torch, got, tw, out, "find_combine_ragged prune=%s fill=%s %s" % (prune, fill, what))


def test_fill_row_keeps_a_negative_zero(env):
  torch, _ = env
  t = _dev_table(torch, "float32", 8, "typed_negzero", default=-0.0)
  t.upsert(T(torch, np.array([5], np.int64)), torch.full((1, 8), -0.0, device="cuda"))
  rs = torch.zeros(4, dtype=torch.int64, device="cuda")
  empty = torch.zeros(0, dtype=torch.int64, device="cuda")
  for fill in (5, 6):   # hit, and a miss that takes the default row
    for out in HALVES:
      got = t.find_combine_ragged(rs, empty, None, COMB["mean"], fill_id=fill, out_dtype=_dt(torch, out))
      assert bool((got.view(torch.int16) == -32768).all()), (fill, out)   # 0x8000


# ---- 5. grouped -------------------------------------------------------------------------------------------------------------------
GROUP = [("float32", 64), ("float32", 64), ("float16", 128), ("bfloat16", 4), ("float32", 256), ("bfloat16", 132), ("float16", 68)]


def _group_requests(torch, ragged):
  reqs = []
  for i, (vd, dim) in enumerate(GROUP):
    t, resident = _find_table(torch, vd, dim)            # (members 0 and 1: the same table stands twice)
    n_rows = 0 if i == 3 else 5 + 3 * i                  # member 3: n_rows == 0, skipped
    ids, rs, seg, w = _pooled_case(resident, n_rows, 3 + i, i % 2 == 0, 900 + i)
    it, wt = T(torch, ids), (None if w is None else T(torch, w))
    if ragged:
      reqs.append((t, T(torch, rs), it, wt, i % 3, i % 2 == 0, (int(resident[0]) if i in (2, 5) else None)))
    else:
      reqs.append((t, it, T(torch, seg), wt, i % 3, n_rows))
  return reqs


@pytest.mark.parametrize("ragged", [False, True])
def test_grouped_equals_the_single_typed_calls(env, ragged):
  from tfra_amd.dynamic_embedding import table_ops
  torch, _ = env
  reqs = _group_requests(torch, ragged)
  many = table_ops.find_combine_ragged_many if ragged else table_ops.find_combine_many

  def single(r, od):
    if ragged:
      return r[0].find_combine_ragged(r[1], r[2], r[3], r[4], prune=r[5], fill_id=r[6], out_dtype=od)
    return r[0].find_combine_typed(r[1], r[2], r[3], r[4], r[5], out_dtype=od)

  _, untyped_launches = many(reqs, return_launches=True)
  for od in (torch.bfloat16, torch.float16):            # one output type for the list: the twin's launch count
    outs, launches = many(reqs, return_launches=True, out_dtype=od)
    assert launches == untyped_launches
    for i, (r, o) in enumerate(zip(reqs, outs)):
      assert o.dtype == od
      assert torch.equal(o.view(torch.int16), single(r, od).view(torch.int16)), "member %d" % i
  mixed = [torch.bfloat16, torch.float32, torch.float16, torch.bfloat16, None, torch.float16, torch.bfloat16]
  outs = many(reqs, out_dtype=mixed)
  for i, (r, o, od) in enumerate(zip(reqs, outs, mixed)):
    want = single(r, od)
    assert o.dtype == (od or torch.float32) == want.dtype
    assert torch.equal(o.view(torch.uint8), want.view(torch.uint8)), "member %d of the mixed list" % i


# ---- 6. refusals: nothing is written --------------------------------------------------------------------------------------------------
def _canary(torch, nbytes):
  buf = torch.full((nbytes + 64,), CANARY, dtype=torch.uint8, device="cuda")
  assert buf.data_ptr() % 16 == 0
  return buf


def _intact(buf):
  return bool((buf == CANARY).all())


def _raw_single(torch, which, t, ro, n_rows, ids, rs_or_seg, ws=True):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  L, dev = _capi.lib(), t.device
  ro_p = ctypes.byref(ro) if ro is not None else None
  if which == "find":
    rc = L.tfra_table_find_typed(t._h, ids.numel(), None, _ptr(ids), ro_p, None, _ptr(t._default_value), 0, _stream(dev))
  elif which == "tuple":
    rc = L.tfra_table_find_combine_typed(t._h, _workspace(dev), ids.numel(), _ptr(ids), _ptr(rs_or_seg), None, 0, n_rows,
                                         _ptr(t._default_value), ro_p, _stream(dev))
  else:
    rc = L.tfra_table_find_combine_ragged_typed(t._h, n_rows, _ptr(rs_or_seg), ids.numel(), _ptr(ids), None, 0, 0, 0,
                                                _ptr(t._default_value), ro_p, _stream(dev))
  return rc, L.tfra_last_error().decode()


def _twin_code(torch, which, t, out_ptr, n_rows, ids, rs_or_seg):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  L, dev = _capi.lib(), t.device
  if which == "tuple":
    return L.tfra_table_find_combine(t._h, _workspace(dev), ids.numel(), _ptr(ids), _ptr(rs_or_seg), None, 0, n_rows,
                                     _ptr(t._default_value), ctypes.c_void_p(out_ptr), _stream(dev))
  return L.tfra_table_find_combine_ragged(t._h, n_rows, _ptr(rs_or_seg), ids.numel(), _ptr(ids), None, 0, 0, 0,
                                          _ptr(t._default_value), ctypes.c_void_p(out_ptr), _stream(dev))


@pytest.mark.parametrize("which", ["find", "tuple", "ragged"])
def test_single_calls_refuse_before_anything_is_written(env, which):
  from tfra_amd import _capi
  torch, _ = env
  dim, n = 64, 6
  t, resident = _find_table(torch, "float32", dim)
  ids = T(torch, resident[:n].copy())
  aux = torch.arange(n + 1, dtype=torch.int64, device="cuda") if which == "ragged" else torch.arange(n, dtype=torch.int64, device="cuda")
  name = {"find": "find_typed", "tuple": "find_combine_typed", "ragged": "find_combine_ragged_typed"}[which]
  buf = _canary(torch, n * dim * 4)
  p = buf.data_ptr()
  cases = [
      (_capi.RowsOut(p, _capi.TFRA_BF16, 1), INVALID, "reserved"),
      (_capi.RowsOut(p, _capi.TFRA_I8, 0), INVALID, "dtype"),
      (_capi.RowsOut(p, 7, 0), INVALID, "dtype"),
      (_capi.RowsOut(p + 4, _capi.TFRA_BF16, 0), UNSUPPORTED, "misaligned"),     # 4 but not 8 bytes
      (_capi.RowsOut(p + 4, _capi.TFRA_F16, 0), UNSUPPORTED, "misaligned"),
      (_capi.RowsOut(p + 8, _capi.TFRA_F32, 0), UNSUPPORTED, "misaligned"),      # 8 but not 16 bytes
      (_capi.RowsOut(None, _capi.TFRA_BF16, 0), INVALID, "null"),                # NULL rows with rows to write
      (None, INVALID, "null"),
  ]
  for ro, code, word in cases:
    rc, msg = _raw_single(torch, which, t, ro, n, ids, aux)
    assert rc == code and name in msg and word in msg, (rc, msg, code, word)
    torch.cuda.synchronize()
    assert _intact(buf), msg
  # a table outside the limits: the twin's code (dim 6: dim % 4 != 0)
  t6 = _dev_table(torch, "float32", 6, "typed_dim6_" + which)
  ro = _capi.RowsOut(p, _capi.TFRA_BF16, 0)
  rc, msg = _raw_single(torch, which, t6, ro, n, ids, aux)
  assert rc == UNSUPPORTED and name in msg and "dim % 4" in msg, (rc, msg)
  if which != "find":
    assert _twin_code(torch, which, t6, p, n, ids, aux) == rc                   # the twin refuses the same table with the same code
    # a twin-side check: a misaligned ids pointer
    bad_ids = torch.zeros(n + 1, dtype=torch.int64, device="cuda").view(torch.int32)[1:2 * n + 1].view(torch.uint8)
    assert bad_ids.data_ptr() % 8 == 4
    from tfra_amd.dynamic_embedding.device_ops import _workspace
    from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
    L = _capi.lib()
    if which == "tuple":
      rc = L.tfra_table_find_combine_typed(t._h, _workspace(t.device), n, _ptr(bad_ids), _ptr(aux), None, 0, n, _ptr(t._default_value),
                                           ctypes.byref(ro), _stream(t.device))
      rc_t = L.tfra_table_find_combine(t._h, _workspace(t.device), n, _ptr(bad_ids), _ptr(aux), None, 0, n, _ptr(t._default_value),
                                       ctypes.c_void_p(p), _stream(t.device))
    else:
      rc = L.tfra_table_find_combine_ragged_typed(t._h, n, _ptr(aux), n, _ptr(bad_ids), None, 0, 0, 0, _ptr(t._default_value),
                                                  ctypes.byref(ro), _stream(t.device))
      rc_t = L.tfra_table_find_combine_ragged(t._h, n, _ptr(aux), n, _ptr(bad_ids), None, 0, 0, 0, _ptr(t._default_value),
                                              ctypes.c_void_p(p), _stream(t.device))
    assert rc == rc_t == UNSUPPORTED
  torch.cuda.synchronize()
  assert _intact(buf)


@pytest.mark.parametrize("ragged", [False, True])
def test_grouped_calls_refuse_the_whole_list(env, ragged):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _stream
  torch, _ = env
  dim, n = 64, 5
  t, resident = _find_table(torch, "float32", dim)
  t6 = _dev_table(torch, "float32", 6, "typed_dim6_many_%d" % ragged)
  ids = T(torch, resident[:n].copy())
  aux = torch.arange(n + 1, dtype=torch.int64, device="cuda")
  D = _capi.FindCombineRaggedTypedDesc if ragged else _capi.FindCombineTypedDesc
  fn = _capi.lib().tfra_multi_find_combine_ragged_typed if ragged else _capi.lib().tfra_multi_find_combine_typed
  name = "multi_find_combine_ragged_typed" if ragged else "multi_find_combine_typed"
  bufs = [_canary(torch, n * dim * 4) for _ in range(3)]

  def descs(bad):
    arr = (D * 3)()
    for i, e in enumerate(arr):
      e.struct_size, e.combiner, e.table = ctypes.sizeof(D), 0, t._h.value
      e.nnz, e.ids, e.weights, e.n_rows, e.default_row = n, ids.data_ptr(), None, n, t._default_value.data_ptr()
      if ragged:
        e.row_splits, e.flags, e.reserved, e.fill_id = aux.data_ptr(), 0, 0, 0
      else:
        e.seg = aux.data_ptr()
      e.out = _capi.RowsOut(bufs[i].data_ptr(), (_capi.TFRA_BF16, _capi.TFRA_F32, _capi.TFRA_F16)[i], 0)
    bad(arr[1])
    return arr

  def reserved(e): e.out.reserved = 3
  def dtype(e): e.out.dtype = _capi.TFRA_I64
  def half_misaligned(e): e.out = _capi.RowsOut(bufs[1].data_ptr() + 4, _capi.TFRA_F16, 0)
  def f32_misaligned(e): e.out = _capi.RowsOut(bufs[1].data_ptr() + 8, _capi.TFRA_F32, 0)
  def null_rows(e): e.out.rows = None
  def size(e): e.struct_size = ctypes.sizeof(D) - 8
  def dim6(e): e.table = t6._h.value

  for bad, code, word in ((reserved, INVALID, "reserved"), (dtype, INVALID, "dtype"), (half_misaligned, UNSUPPORTED, "misaligned"),
                          (f32_misaligned, UNSUPPORTED, "misaligned"), (null_rows, INVALID, "null"), (size, INVALID, "size"),
                          (dim6, UNSUPPORTED, "dim % 4")):
    arr = descs(bad)
    launches = ctypes.c_uint32(99)
    rc = fn(_workspace(t.device), 3, ctypes.c_void_p(ctypes.addressof(arr)), ctypes.c_void_p(ctypes.addressof(launches)), _stream(t.device))
    msg = _capi.lib().tfra_last_error().decode()
    assert rc == code and name in msg and "descriptor 1" in msg and word in msg, (bad.__name__, rc, msg)
    assert launches.value == 0
    torch.cuda.synchronize()
    assert all(_intact(b) for b in bufs), bad.__name__   # every descriptor's output, the good ones' too


# ---- 7. forwarding ----------------------------------------------------------------------------------------------------------------
def test_own_dtype_forwards_byte_identically(env):
  from tfra_amd.dynamic_embedding import table_ops
  torch, _ = env
  for vd in DTYPES:
    t, resident = _find_table(torch, vd, 68)
    keys = T(torch, np.concatenate([resident[:40], [12345]]))
    a, b = t.find(keys), t.find(keys, out_dtype=_dt(torch, vd))
    assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    ids, rs, seg, w = _pooled_case(resident, 9, 5, True, 4)
    it, rt, st, wt = T(torch, ids), T(torch, rs), T(torch, seg), T(torch, w)
    a, b = t.find_combine(it, st, wt, 1, 9), t.find_combine_typed(it, st, wt, 1, 9, out_dtype=torch.float32)
    assert b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    a = t.find_combine_ragged(rt, it, wt, 2, prune=True, fill_id=int(resident[1]))
    b = t.find_combine_ragged(rt, it, wt, 2, prune=True, fill_id=int(resident[1]), out_dtype=torch.float32)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    (a,), la = table_ops.find_combine_many([(t, it, st, wt, 1, 9)], return_launches=True)
    (b,), lb = table_ops.find_combine_many([(t, it, st, wt, 1, 9)], return_launches=True, out_dtype=torch.float32)
    assert la == lb and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_out_dtype_is_checked(env):
  torch, _ = env
  t, resident = _find_table(torch, "float32", 64)
  keys = T(torch, resident[:4].copy())
  with pytest.raises(TypeError):
    t.find(keys, out_dtype=torch.int32)
  with pytest.raises(TypeError):
    t.find_combine_typed(keys, torch.arange(4, device="cuda"), None, 0, 4, out_dtype=torch.float64)
  with pytest.raises(ValueError):
    t.find(keys, field=1, out_dtype=torch.bfloat16)
