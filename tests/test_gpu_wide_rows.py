"""GPU: the wide-row pooled lookup and weight gradient (tfra_table_find_combine_wide, its ragged form and their
*_backprop_weights_wide forms; the `wide_rows` keyword of the sparse lookups), for variables of 256 < dim <= 1024.

One crafted batch: rows of LENS entries — an empty first row, every boundary of the wave's four-entry batch and of its 64-entry load
batch, a row over two batches —, ids from 80 values of which the 40 even ones are resident.  The wide forward must equal today's
route (the same public function with wide_rows=False: unique, find, segment combine) BIT FOR BIT, the wide gradient a lookup of the
rows plus device_ops.sparse_segment_combine_weight_grad, and both are held to the float64 NumPy reference of
tests/test_gpu_long_rows.py under its bound of recursive summation per element: (L + 2) 2^-24 sum_p |w_p x_p| / |den| for the
forward, (L + dim + 4) 2^-24 M_p for the gradient."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls, T, bits

pytestmark = pytest.mark.gpu

LENS = [0, 1, 3, 4, 5, 63, 64, 65, 130]
U24 = 2.0 ** -24
ZERO_ROW = 4          # its weights are all 0: weight sum 0, and under PRUNE a row whose members are all pruned
CLASSES = [("float32", 260), ("float32", 512), ("float16", 768), ("bfloat16", 1024)]   # 260: one lane alone in the second chunk
FORMS = {"tuple": None, "ragged": None, "safe_fill_hit": 2, "safe_fill_miss": 3}   # form -> fill id
C_FORWARD = {"tuple": "tfra_table_find_combine_wide"}


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  rng = np.random.default_rng(41)
  rs = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
  seg = np.repeat(np.arange(len(LENS)), LENS).astype(np.int64)
  ids = rng.integers(0, 80, size=seg.size).astype(np.int64)
  w = rng.uniform(0.25, 2.0, size=seg.size).astype(np.float32)
  w[seg == ZERO_ROW] = 0.0
  wp = w.copy()                                          # the PRUNE form's weights: a fifth of them <= 0
  wp[rng.random(seg.size) < 0.2] = -0.5
  wp[rng.random(seg.size) < 0.05] = 0.0
  tables = {}
  for vdtype, dim in CLASSES:
    dt = getattr(torch, vdtype)
    var = de.Variable(dim=dim, name="wr_%s_%d" % (vdtype, dim), value_dtype=dt, initializer=0.375)
    rows = torch.randn((40, dim), generator=torch.Generator(device="cuda").manual_seed(dim), device="cuda").to(dt)
    var.upsert(T(torch, np.arange(0, 80, 2, dtype=np.int64)), rows)
    x = np.full((80, dim), 0.375)
    x[0::2] = rows.to(torch.float32).cpu().numpy()
    g = torch.randn((len(LENS), dim), generator=torch.Generator(device="cuda").manual_seed(dim + 1), device="cuda")
    tables[(vdtype, dim)] = (var, x, g)
  return torch, de, rs, seg, ids, w, wp, tables


def reference(x, G, seg, ids, w, member, combiner, fill):
  """float64 (out, its bound, dw, its bound) over the member entries; a row without members is x[fill] (zeros for None)."""
  n, dim = len(LENS), x.shape[1]
  w = w.astype(np.float64) * member
  E, L = x[ids], np.bincount(seg, weights=member, minlength=n)
  acc, mag = np.zeros((n, dim)), np.zeros((n, dim))
  np.add.at(acc, seg, E * w[:, None])
  np.add.at(mag, seg, np.abs(E * w[:, None]))
  ws = np.bincount(seg, weights=w * w if combiner == "sqrtn" else w, minlength=n)
  den = np.ones(n) if combiner == "sum" else (np.sqrt(ws) if combiner == "sqrtn" else ws)
  ok = den != 0
  safe = np.where(ok, den, 1)
  out, bound = np.where(ok[:, None], acc / safe[:, None], 0), (L + 2)[:, None] * U24 * mag / np.abs(safe)[:, None]
  if fill is not None:
    out[L == 0] = x[fill]
  d, D = (E * G[seg]).sum(1), np.abs(E * G[seg]).sum(1)
  s, S = np.bincount(seg, weights=w * d, minlength=n)[seg], np.bincount(seg, weights=np.abs(w) * D, minlength=n)[seg]
  W, okp = safe[seg], ok[seg] & (member > 0)
  if combiner == "sum":
    dw, M = d, D
  elif combiner == "mean":
    dw, M = (d - s / W) / W, (D + S / np.abs(W)) / np.abs(W)
  else:
    dw, M = (d - (s / ws[seg].clip(1e-300)) * w) / W, (D + (S / ws[seg].clip(1e-300)) * np.abs(w)) / W
  return out, bound, np.where(okp, dw, 0), (L[seg] + dim + 4) * U24 * np.where(okp, M, 0)


def lookup(torch, de, form, var, rs, seg, ids, w, combiner, fill, **kw):
  from tfra_amd.dynamic_embedding import ragged_embedding_ops as ragged
  if form == "tuple":
    return de.embedding_lookup_sparse(var, (T(torch, seg), T(torch, ids)), w, combiner=combiner, num_rows=len(LENS), **kw)
  if form == "ragged":
    return ragged.embedding_lookup_sparse(var, (T(torch, rs), T(torch, ids)), w, combiner=combiner, **kw)
  return ragged.safe_embedding_lookup_sparse(var, (T(torch, rs), T(torch, ids)), w, combiner=combiner, default_id=fill, **kw)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("vdtype,dim", CLASSES)
def test_wide_forms_equal_todays_route_and_the_float64_reference(env, monkeypatch, vdtype, dim, combiner, weighted, form):
  torch, de, rs, seg, ids, w, wp, tables = env
  from tfra_amd.dynamic_embedding import device_ops
  var, x, g = tables[(vdtype, dim)]
  safe, fill = form.startswith("safe"), FORMS[form]
  wn = (wp if safe else w) if weighted else None
  w_t = None if wn is None else T(torch, wn)
  prune = safe and weighted and combiner != "sum"   # (the safe forms prune by weight unless the combiner is "sum")
  # 1. the forward: the wide call, no unique pass, today's bits
  exp = lookup(torch, de, form, var, rs, seg, ids, w_t, combiner, fill)
  calls = Calls(monkeypatch)
  got = lookup(torch, de, form, var, rs, seg, ids, w_t, combiner, fill, wide_rows=True)
  assert calls[C_FORWARD.get(form, "tfra_table_find_combine_ragged_wide")] == 1 and calls["tfra_unique"] == 0
  assert got.dtype == torch.float32 and tuple(got.shape) == (len(LENS), dim)
  assert torch.equal(bits(torch, got), bits(torch, exp))
  # 2. the gradient: a lookup of the kept entries' rows plus the chain's weight gradient, 0 for a pruned entry
  wv = np.ones(ids.size, np.float32) if wn is None else wn
  member = (wv > 0).astype(np.float64) if prune else np.ones(ids.size)
  kept = T(torch, np.flatnonzero(member))
  ids_t, seg_t = T(torch, ids), T(torch, seg)
  rows = var.lookup(ids_t[kept]).to(torch.float32)
  chain = device_ops.sparse_segment_combine_weight_grad(rows, torch.arange(kept.numel(), device="cuda", dtype=torch.int32), g, seg_t[kept],
                                                        None if w_t is None else w_t[kept], combiner)
  dw_exp = torch.zeros(ids.size, device="cuda").index_copy_(0, kept, chain)
  if form == "tuple":
    dw = var.lookup_combined_weight_grad_wide(ids_t, seg_t, w_t, combiner, g)
  else:
    dw = var.lookup_combined_ragged_weight_grad_wide(T(torch, rs), ids_t, w_t, combiner, g, prune=prune, fill_id=fill)
  assert torch.equal(bits(torch, dw), bits(torch, dw_exp))
  if weighted:   # through a training lookup's wrapper: the chain's wrapper, whose weights_grad takes the wide call
    _, tw0 = lookup(torch, de, form, var, rs, seg, ids, w_t, combiner, fill, return_trainable=True)
    _, tw = lookup(torch, de, form, var, rs, seg, ids, w_t, combiner, fill, return_trainable=True, wide_rows=True)
    calls.n.clear()
    via = tw.weights_grad(g)
    assert calls["tfra_table_find_combine_backprop_weights_wide"] == 1 and calls["tfra_table_find"] == 0
    assert torch.equal(bits(torch, via), bits(torch, tw0.weights_grad(g))) and torch.equal(bits(torch, via), bits(torch, dw))
  # 3. both within the float64 reference's bound
  out, bound, dwr, dbound = reference(x, g.cpu().numpy().astype(np.float64), seg, ids, wv, member, combiner, fill)
  assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - out) <= bound)
  assert np.all(np.abs(dw.cpu().numpy().astype(np.float64) - dwr) <= dbound)
  var._tables[0]._table.check_errors()


@pytest.mark.parametrize("dim", [256, 1028, 258])
def test_other_widths_are_refused_and_nothing_is_written(env, dim):
  torch, de = env[:2]
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(dim), name="wr_dim%d" % dim, dim=dim)
  dev = t._table.device
  h, ws, st, d = t._table._h, _workspace(dev), _stream(dev), _ptr(t._default_value)
  ids, rs = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.tensor([0, 2], dtype=torch.int64, device="cuda")
  g, out, dw = torch.zeros(1, dim, device="cuda"), torch.full((1, dim), 7.0, device="cuda"), torch.full((2,), 7.0, device="cuda")
  lib = _capi.lib()
  for rc in (lib.tfra_table_find_combine_wide(h, ws, 2, _ptr(ids), _ptr(ids), None, 0, 1, d, _ptr(out), st),
             lib.tfra_table_find_combine_ragged_wide(h, 1, _ptr(rs), 2, _ptr(ids), None, 0, 0, 0, d, _ptr(out), st),
             lib.tfra_table_find_combine_backprop_weights_wide(h, ws, 2, _ptr(ids), _ptr(ids), None, 0, 1, d, _ptr(g), _ptr(dw), st),
             lib.tfra_table_find_combine_ragged_backprop_weights_wide(h, 1, _ptr(rs), 2, _ptr(ids), None, 0, 0, 0, d, _ptr(g), _ptr(dw), st)):
    msg = lib.tfra_last_error().decode()
    assert rc == _capi.ERR_UNSUPPORTED and "256 < dim <= 1024" in msg and "tfra_table_find_combine" in msg   # (names the twins)
  assert bool((out == 7.0).all()) and bool((dw == 7.0).all())


def test_the_keyword_changes_nothing_where_the_wide_calls_do_not_serve(env, monkeypatch):
  torch, de, rs, seg, ids, w = env[:6]
  from tests.sparse_helpers import filled_var
  var = filled_var(torch, de, "wr_dim64", initializer=0.5)
  seg_t, ids_t, w_t = T(torch, seg), T(torch, ids * 37), T(torch, w)
  clipped, _, _ = env[7][("float32", 512)]
  calls = Calls(monkeypatch)
  for v, kw in ((var, {}), (var, {"max_norm": 1.0}), (clipped, {"max_norm": 1.0})):
    run = lambda **more: de.embedding_lookup_sparse(v, (seg_t, ids_t), w_t, combiner="mean", num_rows=len(LENS), **kw, **more)
    calls.n.clear()
    a = run(wide_rows=True)
    with_keyword = dict(calls.n)
    calls.n.clear()
    b = run()
    assert with_keyword == calls.n and not any(name.endswith("_wide") for name in with_keyword)
    assert torch.equal(bits(torch, a), bits(torch, b))
  with pytest.raises(ValueError):
    de.embedding_lookup_sparse(clipped, (seg_t, ids_t), w_t, num_rows=len(LENS), wide_rows=True, long_rows=True)
  with pytest.raises(ValueError):
    de.safe_embedding_lookup_sparse(clipped, (seg_t, ids_t), w_t, num_rows=len(LENS), wide_rows=True, mixed_rows=True)


@pytest.mark.parametrize("fill", [None, 2, 3])
def test_no_entries_give_zero_rows_or_fill_rows(env, fill):
  torch, de = env[:2]
  var, x, g = env[7][("float16", 768)]
  none, rs_t = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
  want = np.zeros((3, 768)) if fill is None else np.tile(x[fill], (3, 1))
  got = var.lookup_combined_ragged_wide(rs_t, none, None, "mean", fill_id=fill)
  assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
  assert var.lookup_combined_ragged_weight_grad_wide(rs_t, none, None, "mean", g[:3], fill_id=fill).numel() == 0
  if fill is None:
    assert not var.lookup_combined_wide(none, none, None, "mean", 3).any()
    assert var.lookup_combined_weight_grad_wide(none, none, None, "mean", g[:3]).numel() == 0
