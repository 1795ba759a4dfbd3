"""GPU: float16 / bfloat16 grad_out in the weight gradients of the pooled lookups — the single typed calls
tfra_table_find_combine[_ragged]_backprop_weights_typed, tfra_tier_find_combine[_ragged]_backprop_weights_typed and the chain twin
tfra_sparse_segment_combine_backprop_weights_typed.

The contract: a typed call equals its untyped twin, BIT FOR BIT, given GO32[r, c] = f32(grad_out[r, c]) * s.  Every comparison
here is numeric_edges.assert_bits (expected not NaN: equal bits; expected NaN: a NaN).  GO32 comes from the NumPy model of the
record (tests/half_grads_model.py: g32), never from the code under test."""
import ctypes

import numpy as np
import pytest

from tests import half_grads_model as M
from tests import sparse_helpers as H
from tests.numeric_edges import assert_bits
from tests.sparse_helpers import COMB, T, bits, table
from tests.test_gpu_weight_grad import edge_batch, ragged_batch

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
PRUNE, FILL = 1, 2
COMBINERS = ["sum", "mean", "sqrtn"]
P = ctypes.c_void_p
f32 = np.float32


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def half(torch, bits16, fmt):
  """uint16 ndarray -> a device tensor of the format with exactly these bits."""
  return M.from_bits(torch, bits16, fmt).cuda()


def scale_of(torch, s):
  return None if s is None else torch.full((1,), float(s), dtype=torch.float32, device="cuda")


def pair(torch, tag, vdtype, dim, default=0.0):
  """A tier of two empty tables (the cache bounded), with the tables."""
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
  vd = getattr(torch, vdtype)
  d = torch.full((dim,), default, dtype=vd)
  upper = _DeviceTable(torch.int64, vd, d, "wgh_up_" + tag, "cuda:0", dim=dim, init_capacity=15 * 89, max_capacity=15 * 89, strategy=0)
  lower = _DeviceTable(torch.int64, vd, d, "wgh_lo_" + tag, "cuda:0", dim=dim)
  return _DeviceTier(upper, lower, 4096), upper, lower


# ---- 1. every stored pattern, alone ----------------------------------------------------------------------------------------------------
N_PAT = 65536
KEY = 12345
_PAT = {}


def pattern_setup(torch, de):
  """Once: a float32 table at dim 4 whose one key holds [1, 1, 1, 1], a tier whose upper table holds it, and the batch: one entry
  per row, every entry that key."""
  if not _PAT:
    t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(4), name="wgh_pat", dim=4)._table
    key = torch.tensor([KEY], dtype=torch.int64, device="cuda")
    t.upsert(key, torch.ones((1, 4), device="cuda"))
    tier, upper, _ = pair(torch, "pat", "float32", 4)
    upper.upsert(key, torch.ones((1, 4), device="cuda"), unique_keys=True)
    ids = torch.full((N_PAT,), KEY, dtype=torch.int64, device="cuda")
    seg = torch.arange(N_PAT, dtype=torch.int64, device="cuda")
    rs = torch.arange(N_PAT + 1, dtype=torch.int64, device="cuda")
    _PAT["s"] = (t, tier, ids, seg, rs)
  return _PAT["s"]


@pytest.mark.parametrize("scale", [None, 1e-3, "subnormal"])
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_every_stored_pattern_alone(env, fmt, scale):
  """grad_out[r] = [pattern r, +0, +0, +0] against a row of ones, combiner sum: dw[r] = (((0 + GO32 * 1) + 0) + 0) + 0 and the
  group's reduction adds +0 fifteen times — exact, so each of the 65 536 patterns is visible on its own, non-finite ones included.
  Odd rows of a dim-4 half matrix start at 8 mod 16 bytes."""
  torch, de = env
  s = M.SUBNORMAL_SCALE if scale == "subnormal" else (None if scale is None else f32(scale))
  t, tier, ids, seg, rs = pattern_setup(torch, de)
  pat = M.all_patterns()
  with np.errstate(all="ignore"):
    go32 = M.g32(pat, fmt, s)
    zero = M.g32(np.zeros(1, np.uint16), fmt, s)[0] * f32(1)          # a +0 column's product: +0
    want = (((f32(0) + go32 * f32(1)) + zero) + zero) + zero
    for _ in range(4):                                                  # the xor-shuffles: the other lanes hold +0
      want = want + f32(0)
  want_t = torch.from_numpy(want.astype(f32))
  sc = scale_of(torch, s)
  ctx = lambda i: "pattern %04x of %s, scale %r" % (i, fmt, s)
  for dim in (4, 3):                                                    # 4: every vector arm; 3: the chain twin's element-wise arm
    g = np.zeros((N_PAT, dim), np.uint16)
    g[:, 0] = pat
    G = half(torch, g, fmt)
    assert G.data_ptr() % 16 == 0 and G.is_contiguous()
    rows = torch.ones((1, dim), device="cuda")
    idx = torch.zeros(N_PAT, dtype=torch.int32, device="cuda")
    got = de.device_ops.sparse_segment_combine_weight_grad(rows, idx, G, seg, None, "sum", grad_scale=sc)
    assert_bits(torch, got, want_t, "chain twin, dim %d" % dim, ctx)
    if dim == 4:
      assert_bits(torch, t.find_combine_weight_grad_typed(ids, seg, None, 0, G, grad_scale=sc), want_t, "table, tuple form", ctx)
      assert_bits(torch, t.find_combine_ragged_weight_grad_typed(rs, ids, None, 0, G, grad_scale=sc), want_t, "table, ragged form", ctx)
      assert_bits(torch, tier.find_combine_weight_grad_typed(ids, seg, None, 0, G, grad_scale=sc), want_t, "tier, tuple form", ctx)
      assert_bits(torch, tier.find_combine_ragged_weight_grad_typed(rs, ids, None, 0, G, grad_scale=sc), want_t, "tier, ragged form", ctx)
  t.check_errors()


# ---- 2. every lane, chunk and batch boundary, against the twin ------------------------------------------------------------------------
def random_half_bits(n_rows, dim, fmt, seed):
  """Finite random gradients of the format, as bits; a few subnormals, zeros of both signs and large values among them."""
  import torch
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((n_rows, dim)).astype(f32)
  x[rng.random((n_rows, dim)) < 0.02] *= f32(1e-6)
  x[rng.random((n_rows, dim)) < 0.02] *= f32(3e3)
  x[rng.random((n_rows, dim)) < 0.01] = f32(-0.0)
  return M.bits_of(torch, torch.from_numpy(x).to(getattr(torch, fmt)))


@pytest.mark.parametrize("vdtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("dim", [4, 60, 64, 68, 128, 192, 256])   # one lane; a partial chunk; a full one; one lane in a second; NCH 2, 4 (partial), 4
def test_typed_equals_the_twin_on_go32(env, dim, vdtype):
  torch, de = env
  t = table(torch, de, "cuckoo", vdtype, dim)._table
  ids_t, seg_t, w_t = edge_batch(torch)                       # rows of 0, 1, 3, 4, 5, 15, 16, 17 and 33 entries, misses among the ids
  ids_x = torch.cat([ids_t, ids_t[:5]])                       # five entries in no row at the tail
  seg_x = torch.cat([seg_t, torch.tensor([37, 40, 99, 1000, 5000], dtype=torch.int64, device="cuda")])   # (n_rows is 37)
  w_x = torch.cat([w_t, w_t[:5]])
  rs, w, rs_t, rids_t, rw_t, rseg_t = ragged_batch(torch)
  rw_clean = torch.where(torch.isnan(rw_t), torch.ones_like(rw_t), rw_t)
  # a tier whose cache is empty: every resident key is only below (every other id of the batch: the default row)
  tier, _, lower = pair(torch, "%s_%d" % (vdtype, dim), vdtype, dim, default=0.25)
  uniq = torch.unique(ids_t)
  lower.upsert(uniq[::2].contiguous(), t.find(uniq[::2].contiguous()))
  for k, (fmt, s) in enumerate((("float16", None), ("bfloat16", 1e-3), ("bfloat16", None), ("float16", 1e-3))):
    sc = scale_of(torch, s)
    for (n_rows, tag) in ((37, "edge"), (40, "ragged")):
      b16 = random_half_bits(n_rows, dim, fmt, 100 * dim + 10 * k + n_rows)
      G, G32 = half(torch, b16, fmt), T(torch, M.g32(b16, fmt, s))   # GO32 carries the scale per element
      assert G.dtype == getattr(torch, fmt) and G32.dtype == torch.float32
      for combiner in COMBINERS:
        c = COMB[combiner]
        what = "%s %s scale %r %s" % (tag, fmt, s, combiner)
        if tag == "edge":
          for wt in (w_x, None):
            assert_bits(torch, t.find_combine_weight_grad_typed(ids_x, seg_x, wt, c, G, grad_scale=sc),
                        t.find_combine_weight_grad(ids_x, seg_x, wt, c, G32), "table tuple " + what)
            assert_bits(torch, tier.find_combine_weight_grad_typed(ids_x, seg_x, wt, c, G, grad_scale=sc),
                        tier.find_combine_weight_grad(ids_x, seg_x, wt, c, G32), "tier tuple " + what)
            rows = t.find(ids_x).to(torch.float32)
            idx = torch.arange(ids_x.numel(), dtype=torch.int32, device="cuda")
            chain = de.device_ops.sparse_segment_combine_weight_grad(rows, idx, G, seg_x, wt, combiner, grad_scale=sc)
            assert_bits(torch, chain, de.device_ops.sparse_segment_combine_weight_grad(rows, idx, G32, seg_x, wt, combiner),
                        "chain twin " + what)
            # the two routes give the same bits for the same rows, for half gradients too
            assert_bits(torch, chain, t.find_combine_weight_grad_typed(ids_x, seg_x, wt, c, G, grad_scale=sc), "routes " + what)
        else:
          for wt, prune, fill in ((rw_clean, False, None), (None, False, None), (rw_t, True, None), (rw_t, True, int(rids_t[0])),
                                  (rw_clean, False, 777)):
            for owner, name in ((t, "table"), (tier, "tier")):
              assert_bits(torch, owner.find_combine_ragged_weight_grad_typed(rs_t, rids_t, wt, c, G, prune=prune, fill_id=fill,
                                                                             grad_scale=sc),
                          owner.find_combine_ragged_weight_grad(rs_t, rids_t, wt, c, G32, prune=prune, fill_id=fill),
                          "%s ragged prune %d fill %r %s" % (name, prune, fill, what))
  t.check_errors()


# ---- 3. the scale is read on the stream ----------------------------------------------------------------------------------------------
def test_the_scale_is_read_on_the_stream(env):
  torch, de = env
  dim = 64
  t = table(torch, de, "cuckoo", "float32", dim)._table
  ids_t, seg_t, w_t = edge_batch(torch)
  b16 = random_half_bits(37, dim, "float16", 3)
  G = half(torch, b16, "float16")
  want = {s: t.find_combine_weight_grad(ids_t, seg_t, w_t, 1, T(torch, M.g32(b16, "float16", s))) for s in (0.25, 3.0)}
  rows = t.find(ids_t).to(torch.float32)
  idx = torch.arange(ids_t.numel(), dtype=torch.int32, device="cuda")
  torch.cuda.synchronize()
  scale = torch.zeros(1, dtype=torch.float32, device="cuda")
  got = []
  for s in (0.25, 3.0):           # a torch kernel fills the scale on the call's stream, directly before the call: no synchronisation
    scale.fill_(s)
    got.append((s, "table", t.find_combine_weight_grad_typed(ids_t, seg_t, w_t, 1, G, grad_scale=scale)))
    scale.fill_(s)
    got.append((s, "chain", de.device_ops.sparse_segment_combine_weight_grad(rows, idx, G, seg_t, w_t, "mean", grad_scale=scale)))
  for s, name, dw in got:
    assert_bits(torch, dw, want[s], "%s with the scale %r written on the stream" % (name, s))


# ---- 4. forwarding and 5. refusals: the C calls themselves -----------------------------------------------------------------------------
def _grads(g_ptr, dtype, reserved=0, scale_ptr=None):
  from tfra_amd import _capi
  return _capi.Grads(g_ptr, dtype, reserved, scale_ptr)


def raw_calls(torch, t, tier, a):
  """name -> f(tfra_grads or None, **overrides) -> code: the five single typed calls over the arguments `a` (a dict)."""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  lib = _capi.lib()
  ws, st = _workspace(t._device), _stream(t._device)

  def ref(g):
    return None if g is None else ctypes.byref(g)

  def args(kw):
    x = dict(a)
    x.update(kw)
    return x

  def tup(f, h):
    def call(g, **kw):
      x = args(kw)
      return f(h, ws, x["nnz"], x["ids"], x["seg"], x["w"], x["combiner"], x["n_rows"], x["default_row"], ref(g), x["dw"], st)
    return call

  def rag(f, h):
    def call(g, **kw):
      x = args(kw)
      return f(h, x["n_rows"], x["rs"], x["nnz"], x["ids"], x["w"], x["combiner"], x["flags"], 0, x["default_row"], ref(g), x["dw"], st)
    return call

  def chain(g, **kw):
    x = args(kw)
    return lib.tfra_sparse_segment_combine_backprop_weights_typed(ws, x["nnz"], x["dim"], x["rows"], x["idx"], ref(g), x["seg"], x["w"],
                                                                  x["combiner"], x["n_rows"], x["dw"], st)

  return {"find_combine_backprop_weights_typed": tup(lib.tfra_table_find_combine_backprop_weights_typed, t._h),
          "find_combine_ragged_backprop_weights_typed": rag(lib.tfra_table_find_combine_ragged_backprop_weights_typed, t._h),
          "tfra_tier_find_combine_backprop_weights_typed": tup(lib.tfra_tier_find_combine_backprop_weights_typed, tier._h),
          "tfra_tier_find_combine_ragged_backprop_weights_typed": rag(lib.tfra_tier_find_combine_ragged_backprop_weights_typed, tier._h),
          "segment_combine_backprop_weights_typed": chain}


_RAW = {}


def raw_setup(torch, de):
  if not _RAW:
    from tfra_amd import _capi
    dim, nnz, n_rows = 8, 6, 2
    owner = de.HkvHashTable(torch.int64, torch.float32, torch.full((dim,), 0.5), name="wgh_raw", init_capacity=8192, max_capacity=8192,
                            max_hbm_for_values=1 << 28, evict_strategy=de.HkvEvictStrategy.LRU, dim=dim)
    keys = torch.arange(0, 40, 2, dtype=torch.int64, device="cuda")
    vals = torch.randn((keys.numel(), dim), generator=torch.Generator(device="cuda").manual_seed(8), device="cuda")
    owner.insert(keys, vals)
    t = owner._table
    tier, upper, lower = pair(torch, "raw", "float32", dim, default=0.5)
    upper.upsert(keys[:10].contiguous(), vals[:10].contiguous(), unique_keys=True)
    lower.upsert(keys, vals)
    k = type("Raw", (), {})()
    k.owner, k.t, k.tier, k.upper, k.lower, k.dim, k.nnz, k.n_rows = owner, t, tier, upper, lower, dim, nnz, n_rows
    k.ids = T(torch, np.array([0, 2, 5, 4, 38, 7], dtype=np.int64))
    k.seg = T(torch, np.array([0, 0, 0, 1, 1, 1], dtype=np.int64))
    k.rs = T(torch, np.array([0, 3, 6], dtype=np.int64))
    k.w = T(torch, np.array([0.5, 1.5, -1.0, 2.0, 0.25, 1.0], dtype=f32))
    k.rows = t.find(k.ids).to(torch.float32).contiguous()
    k.idx = torch.arange(nnz, dtype=torch.int32, device="cuda")
    k.default_row = t._default_value
    b16 = random_half_bits(n_rows + 1, dim, "bfloat16", 9)
    k.b16 = b16[:n_rows]
    k.Gbuf = half(torch, b16, "bfloat16")              # one spare row: a pointer 2 bytes in still lies inside the allocation
    k.G32 = T(torch, M.g32(k.b16, "bfloat16", None))
    k.scale = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
    k.BF16, k.F16, k.F32 = _capi.TFRA_BF16, _capi.TFRA_F16, _capi.TFRA_F32
    _RAW["k"] = k
  return _RAW["k"]


def raw_args(k, dw):
  from tfra_amd.dynamic_embedding.table_ops import _ptr
  return dict(nnz=k.nnz, ids=P(k.ids.data_ptr()), seg=P(k.seg.data_ptr()), rs=P(k.rs.data_ptr()), w=P(k.w.data_ptr()), combiner=1,
              n_rows=k.n_rows, default_row=_ptr(k.default_row), dw=P(dw.data_ptr()), flags=0, dim=k.dim, rows=P(k.rows.data_ptr()),
              idx=P(k.idx.data_ptr()))


def test_float32_without_a_scale_forwards_to_the_untyped_call(env):
  torch, de = env
  k = raw_setup(torch, de)
  want_table = k.t.find_combine_weight_grad(k.ids, k.seg, k.w, 1, k.G32)
  want_tier = k.tier.find_combine_weight_grad(k.ids, k.seg, k.w, 1, k.G32, k.default_row)
  want_chain = de.device_ops.sparse_segment_combine_weight_grad(k.rows, k.idx, k.G32, k.seg, k.w, "mean")
  for name, call in raw_calls(torch, k.t, k.tier, {}).items():
    dw = torch.full((k.nnz,), 7.0, device="cuda")
    assert call(_grads(k.G32.data_ptr(), k.F32), **raw_args(k, dw)) == 0, name
    want = want_chain if name.startswith("segment") else want_tier if "tier" in name else want_table
    assert_bits(torch, dw, want, name + " on TFRA_F32 without a scale")
    # and the half matrix through the same raw call gives the same bits: GO32 of these bits is G32
    dw = torch.full((k.nnz,), 7.0, device="cuda")
    assert call(_grads(k.Gbuf.data_ptr(), k.BF16), **raw_args(k, dw)) == 0, name
    assert_bits(torch, dw, want, name + " on bfloat16")


def test_refusals_write_nothing_and_leave_the_table_untouched(env):
  torch, de = env
  from tfra_amd import _capi
  k = raw_setup(torch, de)

  def state():
    out = []
    for tab, scored in ((k.t, True), (k.upper, True), (k.lower, False)):
      kk, v, s = tab.export_all(with_scores=scored)
      o = torch.argsort(kk)
      out += [kk[o], bits(torch, v[o])] + ([s[o]] if s is not None else []) + [tab.size_device().reshape(-1)]
    return out

  before = state()
  g_ptr = k.Gbuf.data_ptr()
  ok = _grads(g_ptr, k.BF16)
  # (the record, code, text): the record's refusals, in every call
  record = [(_grads(g_ptr + 2, k.F16), UNSUPPORTED, "8-B aligned"),
            (_grads(k.G32.data_ptr(), k.F32, 0, k.scale.data_ptr()), UNSUPPORTED, "float32 gradients take no scale"),
            (_grads(g_ptr, k.BF16, 1), INVALID, "reserved"),
            (_grads(g_ptr, 3), INVALID, "dtype"),
            (None, INVALID, "null gradients")]
  # the twins' own refusals behind a good record: (override, code, text, the calls it applies to)
  twin = [(dict(combiner=3), INVALID, "", None),
          (dict(default_row=P(k.default_row.data_ptr() + 4)), UNSUPPORTED, "misaligned buffer", "find_combine"),
          (dict(ids=None), INVALID, "null buffer", "find_combine"),
          (dict(rows=None), INVALID, "null buffer", "segment"),
          (dict(dw=None), INVALID, "null", None),
          (dict(nnz=1 << 31), None, "too large", None),
          (dict(flags=4), INVALID, "unknown flag bits", "ragged"),
          (dict(w=P(k.w.data_ptr() + 2)), UNSUPPORTED, "misaligned", None)]
  for name, call in raw_calls(torch, k.t, k.tier, {}).items():
    for g, code, text in record:
      dw = torch.full((k.nnz,), 7.0, device="cuda")
      assert call(g, **raw_args(k, dw)) == code, (name, text)
      msg = _capi.lib().tfra_last_error().decode()
      assert msg.startswith(name) and text in msg, msg
      torch.cuda.synchronize()
      assert bool((dw == 7.0).all()), (name, text)
    for kw, code, text, only in twin:
      if only is not None and only not in name:
        continue
      dw = torch.full((k.nnz,), 7.0, device="cuda")
      a = raw_args(k, dw)
      a.update(kw)
      rc = call(ok, **a)
      assert rc != 0 and (code is None or rc == code), (name, kw, rc)
      msg = _capi.lib().tfra_last_error().decode()
      assert msg.startswith(name) and text in msg, msg
      torch.cuda.synchronize()
      assert bool((dw == 7.0).all()), (name, kw)
  # what only the table can get wrong: a dim that is no multiple of 4 names the typed call and the chain route
  t6 = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(6), name="wgh_dim6", dim=6)._table
  G6 = torch.zeros((2, 6), dtype=torch.bfloat16, device="cuda")
  dw = torch.full((k.nnz,), 7.0, device="cuda")
  a = raw_args(k, dw)
  a["default_row"] = P(t6._default_value.data_ptr())
  call = raw_calls(torch, t6, k.tier, {})["find_combine_backprop_weights_typed"]
  assert call(_grads(G6.data_ptr(), k.BF16), **a) == UNSUPPORTED
  msg = _capi.lib().tfra_last_error().decode()
  assert msg.startswith("find_combine_backprop_weights_typed (out = grad_out): ") and "dim % 4 == 0" in msg, msg
  torch.cuda.synchronize()
  assert bool((dw == 7.0).all())
  # good calls are reads too
  for name, call in raw_calls(torch, k.t, k.tier, {}).items():
    dw = torch.full((k.nnz,), 7.0, device="cuda")
    assert call(ok, **raw_args(k, dw)) == 0, name
  after = state()
  assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after))
  k.t.check_errors()
