"""GPU: the gradient of the pooled lookup's weights over a tier (tfra_tier_find_combine_backprop_weights and its ragged form), on the
setup of tests/test_gpu_tier_pooled.py — an upper LRU table of 15 * 89 slots at max_capacity over a growing lower table, 3000 keys
written through the tier, a batch of about 2000 entries (max_batch = 512) drawn after the fill with >= 100 entries each in upper,
only below and in neither, stale copies below promoted keys, both sentinel key values, entries outside every row, and rows of
0 / 1 / 3 / 4 / 5 / 16 / 17 / 33 entries.

Every comparison is bit for bit.  The references are code that does not read two tables in one launch: tier.find of the unique
ids (in calls of at most max_batch) + device_ops.sparse_segment_combine_weight_grad, and find_combine_weight_grad on a roomy twin
table that holds every key's newest row.  After every call both tables and the tier's statistics are what they were."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_tier_pooled import COMB, INVALID, MAX_BATCH, UNSUPPORTED, _unchanged, bits, setup_of

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
TUPLE, RAGGED = "tfra_tier_find_combine_backprop_weights", "tfra_tier_find_combine_ragged_backprop_weights"


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


_EXTRA = {}


def extra_of(torch, s, dim, vdtype):
  """What these tests add to the forward's setup, once per (dim, value dtype), without a call that counts in the tier's statistics:
  grad_out; the rows tier.find returned for the batch (the setup fetched them in calls of at most max_batch) as ONE row per unique
  id, with torch.unique's inverse as their index; and which entries of the rows have their key only below."""
  if (dim, vdtype) not in _EXTRA:
    x = type("Extra", (), {})()
    g = torch.Generator(device="cuda").manual_seed(1000 + dim)
    x.G = torch.randn((s.n_rows, dim), generator=g, device="cuda", dtype=torch.float32)
    uniq, x.inv = torch.unique(s.ids, return_inverse=True)
    x.rows = torch.zeros((uniq.numel(), dim), dtype=torch.float32, device="cuda")
    x.rows[x.inv] = s.found.to(torch.float32)                 # (every position of one id holds the same row)
    assert uniq.numel() < s.ids.numel() and torch.equal(bits(torch, x.rows[x.inv]), bits(torch, s.found.to(torch.float32)))
    up, lo = s.upper.contains(s.ids), s.lower.contains(s.ids)
    in_rows = (s.seg >= 0) & (s.seg < s.n_rows)
    x.below = ~up & lo & in_rows
    for kind in (up & in_rows, x.below, ~up & ~lo & in_rows):
      assert int(kind.sum()) >= 100
    _unchanged(torch, s)
    _EXTRA[(dim, vdtype)] = x
  return _EXTRA[(dim, vdtype)]


def cover_of(splits, nnz):
  """how many rows claim each entry, by the kernel's clamp: b = clamp(lo, 0, nnz), e = clamp(hi, b, nnz)"""
  cover = np.zeros(nnz, dtype=np.int64)
  for lo, hi in zip(splits[:-1], splits[1:]):
    b = min(max(int(lo), 0), nnz)
    cover[b:min(max(int(hi), b), nnz)] += 1
  return cover


@pytest.mark.parametrize("weights", ["none", "random", "mixed"])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("vdtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("dim", [8, 72, 256])
def test_weight_grad_sees_both_tiers_bitwise(env, dim, vdtype, combiner, weights):
  torch, de = env
  s = setup_of(torch, dim, vdtype)
  x = extra_of(torch, s, dim, vdtype)
  c, w, n, G = COMB[combiner], s.weights[weights], s.n_rows, x.G
  assert s.ids.numel() > s.tier.max_batch                    # no staging: the batch is not limited by max_batch
  # ---- 1. the tuple form: the chain over tier.find's rows, and the one-table call on the twin
  got = s.tier.find_combine_weight_grad(s.ids, s.seg, w, c, G, s.default_row)
  _unchanged(torch, s)
  assert got.dtype == torch.float32 and tuple(got.shape) == (s.ids.numel(),)
  chain = de.device_ops.sparse_segment_combine_weight_grad(x.rows, x.inv, G, s.seg, w, combiner)
  assert torch.equal(bits(torch, got), bits(torch, chain))
  twin = s.twin.find_combine_weight_grad(s.ids, s.seg, w, c, G, s.default_row)
  assert torch.equal(bits(torch, got), bits(torch, twin))
  assert not bool(bits(torch, got[:s.front]).any()) and not bool(bits(torch, got[-s.back:]).any())    # entries in no row
  assert bool(torch.isfinite(got).all())
  # ---- 3. the second view is read: the cache alone answers the entries that are only below with the default row
  cache = s.upper.find_combine_weight_grad(s.ids, s.seg, w, c, G, s.default_row)
  differ = (bits(torch, got) != bits(torch, cache)) & x.below
  assert int(differ.sum()) >= 100, int(differ.sum())
  # ---- 2. the ragged form on the same rows (the entries outside [0, n_rows) are in no row)
  a, b = s.front, s.ids.numel() - s.back
  ids_in, w_in = s.ids[a:b], (None if w is None else w[a:b])
  rag = s.tier.find_combine_ragged_weight_grad(s.splits, ids_in, w_in, c, G, default_row=s.default_row)
  _unchanged(torch, s)
  assert torch.equal(bits(torch, rag), bits(torch, got[a:b]))
  # PRUNE: an entry with weight <= 0 gets exactly 0, the rest are the twin's
  pruned = s.tier.find_combine_ragged_weight_grad(s.splits, ids_in, w_in, c, G, prune=True, default_row=s.default_row)
  _unchanged(torch, s)
  if w is None:
    assert torch.equal(bits(torch, pruned), bits(torch, rag))
  else:
    keep = w_in > 0
    assert not bool(bits(torch, pruned[~keep]).any())
    want = s.twin.find_combine_ragged_weight_grad(s.splits, ids_in, w_in, c, G, prune=True, default_row=s.default_row)
    assert torch.equal(bits(torch, pruned), bits(torch, want))
    compact = s.tier.find_combine_weight_grad(ids_in[keep], s.seg[a:b][keep], w_in[keep], c, G, s.default_row)
    assert torch.equal(bits(torch, pruned[keep]), bits(torch, compact))
  # FILL: a row without members gives 0 for all its entries, wherever the fill id is; the other rows are unchanged
  for kind, fill in s.fill.items():
    filled = s.tier.find_combine_ragged_weight_grad(s.splits, ids_in, w_in, c, G, prune=True, fill_id=fill, default_row=s.default_row)
    _unchanged(torch, s)
    assert torch.equal(bits(torch, filled), bits(torch, pruned)), kind
    if weights == "mixed":
      lo, hi = int(s.splits[5]), int(s.splits[6])               # row 5: 16 entries, every weight 0
      assert hi - lo == 16 and not bool(bits(torch, filled[lo:hi]).any()), kind
    plain = s.tier.find_combine_ragged_weight_grad(s.splits, ids_in, w_in, c, G, fill_id=fill, default_row=s.default_row)
    assert torch.equal(bits(torch, plain), bits(torch, rag)), kind
  # row_splits that are negative, decreasing or beyond nnz are clamped: an entry outside the clamped cover gets 0, an entry that
  # exactly one row claims is what the one-table kernel gives (an entry two rows claim is written by both, in no order)
  nnz_in = ids_in.numel()
  base = s.splits.cpu().numpy()
  bad_a, bad_b = base.copy(), base.copy()
  bad_a[0], bad_a[10], bad_a[-1] = -7, base[9] - 2, nnz_in - 3          # negative; decreasing; the last 3 entries in no row
  bad_b[20] = nnz_in + 1000                                              # row 19 runs to the end of ids
  for bad in (bad_a, bad_b):
    cover = cover_of(bad, nnz_in)
    one = torch.from_numpy(cover == 1).cuda()
    assert int(one.sum()) >= 100
    bad_t = torch.from_numpy(bad).cuda()
    clamped = s.tier.find_combine_ragged_weight_grad(bad_t, ids_in, w_in, c, G, default_row=s.default_row)
    _unchanged(torch, s)
    want = s.twin.find_combine_ragged_weight_grad(bad_t, ids_in, w_in, c, G, default_row=s.default_row)
    assert torch.equal(bits(torch, clamped[one]), bits(torch, want[one]))
    assert not bool(bits(torch, clamped[torch.from_numpy(cover == 0).cuda()]).any())
    assert bool(torch.isfinite(clamped).all())
  assert (cover_of(bad_a, nnz_in) == 0).sum() == 3 and (cover_of(bad_a, nnz_in) == 2).sum() == 2


def test_nothing_to_read(env):
  torch, _ = env
  s = setup_of(torch, 8, "float32")
  x = extra_of(torch, s, 8, "float32")
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  z = torch.zeros(6, dtype=torch.int64, device="cuda")
  for c in (0, 1, 2):
    assert tuple(s.tier.find_combine_weight_grad(none, none, None, c, x.G[:5], s.default_row).shape) == (0,)       # nnz == 0
    assert tuple(s.tier.find_combine_ragged_weight_grad(z, none, None, c, x.G[:5], default_row=s.default_row).shape) == (0,)
  # entries but no rows: every entry is in no row
  ids = s.ids[:5]
  assert not bool(bits(torch, s.tier.find_combine_weight_grad(ids, torch.zeros_like(ids), None, 1, x.G[:0], s.default_row)).any())
  assert not bool(bits(torch, s.tier.find_combine_ragged_weight_grad(z[:1], ids, None, 1, x.G[:0], default_row=s.default_row)).any())
  _unchanged(torch, s)


def _pair(torch, tag, vd, dim):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
  upper = _DeviceTable(torch.int64, vd, torch.zeros(dim, dtype=vd), "twg_up_" + tag, "cuda:0", dim=dim, init_capacity=15 * 89,
                       max_capacity=15 * 89, strategy=0)
  lower = _DeviceTable(torch.int64, vd, torch.zeros(dim, dtype=vd), "twg_lo_" + tag, "cuda:0", dim=dim)
  return _DeviceTier(upper, lower, MAX_BATCH)


def test_refusals_by_code_and_name(env):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  ids = torch.arange(8, dtype=torch.int64, device="cuda")
  seg = torch.arange(8, dtype=torch.int64, device="cuda") // 2
  splits = torch.arange(0, 9, 2, dtype=torch.int64, device="cuda")
  # what the Python layer cannot see: the table's dim and value dtype; the hint names the chain route over a tier
  for tag, vd, dim, what in (("dim6", torch.float32, 6, "dim % 4 == 0"), ("int32", torch.int32, 8, "value_dtype must be")):
    tier = _pair(torch, tag, vd, dim)
    G = torch.zeros((4, dim), dtype=torch.float32, device="cuda")
    for name, call in ((TUPLE, lambda: tier.find_combine_weight_grad(ids, seg, None, 1, G)),
                       (RAGGED, lambda: tier.find_combine_ragged_weight_grad(splits, ids, None, 1, G))):
      with pytest.raises(_capi.TfraError) as e:
        call()
      assert e.value.code == UNSUPPORTED and name + ":" in str(e.value) and what in str(e.value)
      if tag == "dim6":
        assert "tfra_tier_find + tfra_sparse_segment_combine_backprop_weights" in str(e.value)
  s = setup_of(torch, 8, "float32")
  lib, dev = _capi.lib(), s.upper.device
  ws, st, d = _workspace(dev), _stream(dev), _ptr(s.default_row)
  G = torch.ones(4 * 8 + 4, dtype=torch.float32, device="cuda")
  dw = torch.full((12,), 7.0, dtype=torch.float32, device="cuda")
  g, o = P(G.data_ptr()), P(dw.data_ptr())
  tup = lambda tier=s.tier._h, combiner=1, grad=g, out=o: lib.tfra_tier_find_combine_backprop_weights(
      tier, ws, 8, _ptr(ids), _ptr(seg), None, combiner, 4, d, grad, out, st)
  rag = lambda tier=s.tier._h, combiner=1, flags=0, grad=g, out=o: lib.tfra_tier_find_combine_ragged_backprop_weights(
      tier, 4, _ptr(splits), 8, _ptr(ids), None, combiner, flags, 0, d, grad, out, st)

  def refused(call, name, code, what, **kw):
    assert call(**kw) == code, (name, kw)
    msg = lib.tfra_last_error().decode()
    assert msg.startswith(name + ":") and what in msg, msg

  for call, name in ((tup, TUPLE), (rag, RAGGED)):
    refused(call, name, INVALID, "null tier", tier=None)
    refused(call, name, INVALID, "bad argument", combiner=3)
    refused(call, name, INVALID, "null dw_out", out=None)
    refused(call, name, UNSUPPORTED, "misaligned dw_out", out=P(dw.data_ptr() + 2))
    refused(call, name, UNSUPPORTED, "misaligned buffer", grad=P(G.data_ptr() + 4))
  refused(rag, RAGGED, INVALID, "unknown flag bits", flags=4)
  torch.cuda.synchronize()
  assert bool((dw == 7.0).all())                              # nothing was enqueued
  # the same operands, accepted: the 8 entries are written, the guard behind them is not
  assert tup(combiner=0) == 0
  torch.cuda.synchronize()
  first = dw.clone()
  assert bool((first[8:] == 7.0).all()) and not bool((first[:8] == 7.0).any())
  dw.fill_(7.0)
  assert rag(combiner=0) == 0
  torch.cuda.synchronize()
  assert torch.equal(bits(torch, dw), bits(torch, first))
  # nnz == 0 and n_rows == 0 return OK, dw_out may be NULL when there is no entry
  assert lib.tfra_tier_find_combine_backprop_weights(s.tier._h, ws, 0, None, None, None, 1, 4, d, g, None, st) == 0
  assert lib.tfra_tier_find_combine_ragged_backprop_weights(s.tier._h, 4, _ptr(splits), 0, None, None, 1, 0, 0, d, g, None, st) == 0
  assert lib.tfra_tier_find_combine_backprop_weights(s.tier._h, ws, 8, _ptr(ids), _ptr(seg), None, 1, 0, d, None, o, st) == 0
  assert lib.tfra_tier_find_combine_ragged_backprop_weights(s.tier._h, 0, None, 8, _ptr(ids), None, 1, 0, 0, d, None, o, st) == 0
  torch.cuda.synchronize()
  assert not bool(bits(torch, dw[:8]).any()) and bool((dw[8:] == 7.0).all())   # entries without a row: 0
  _unchanged(torch, s)
