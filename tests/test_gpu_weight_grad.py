"""GPU: the gradient of the pooled lookup with respect to its weights (tfra_table_find_combine_backprop_weights, its ragged form,
the chain twin tfra_sparse_segment_combine_backprop_weights; Variable.lookup_combined_weight_grad; SparseTrainableWrapper.weights_grad).

The table kernels and the chain twin call the same device functions (csrc/tfra_combine_device.h: wgrad_*) in one evaluation order,
so the two routes must agree BIT FOR BIT: those comparisons are torch.equal on int32 views.  Against float64 the tolerance is the
forward error bound of the computation, per entry: |got - exp| <= (dim + cnt_r + 8) * 2^-23 * T_p with T_p the float64 sum of
the absolute values of all terms of dw_p (tests/wgrad_model.py, checked against torch.autograd in tests/test_weight_grad_abi.py)."""
import numpy as np
import pytest

import oracle
from tests import sparse_helpers as H
from tests.sparse_helpers import COMB, T, batch, bits, table
from tests.wgrad_model import bounds_of, chain_autograd, wgrad_model

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
PRUNE, FILL = 1, 2
COMBINERS = ["sum", "mean", "sqrtn"]
EDGE_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 33]   # either side of the U = 4 step and of the 16-entry batch


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def chain(torch, de, t, ids_t, seg_t, w_t, combiner, G):
  """The chain route: find, then the chain twin over idx = arange."""
  rows = t._table.find(ids_t).to(torch.float32)
  idx = torch.arange(ids_t.numel(), dtype=torch.int32, device="cuda")
  return de.device_ops.sparse_segment_combine_weight_grad(rows, idx, G, seg_t, w_t, combiner)


def grad_of(torch, n_rows, dim, seed=0):
  g = torch.Generator(device="cuda").manual_seed(1000 + 7 * dim + seed)
  return torch.randn((n_rows, dim), generator=g, device="cuda")


# ---- 1. the table route equals the chain route, bit for bit ------------------------------------------------------------------------
_EDGE = {}


def edge_batch(torch):
  """37 rows (a partial last wave) of the EDGE_LENGTHS, ids with misses, weights with zeros and negatives."""
  if not _EDGE:
    rng = np.random.default_rng(37)
    counts = np.array([EDGE_LENGTHS[i % len(EDGE_LENGTHS)] for i in range(37)])
    seg = np.repeat(np.arange(37, dtype=np.int64), counts)
    keys, _ = H._universe()
    ids = keys[(rng.zipf(1.2, size=seg.size) - 1) % H.POOL_UNIVERSE]
    w = rng.standard_normal(seg.size).astype(np.float32)
    w[rng.random(seg.size) < 0.05] = 0.0
    _EDGE["b"] = (T(torch, ids), T(torch, seg), T(torch, w))
  return _EDGE["b"]


@pytest.mark.parametrize("dim", [4, 64, 132, 256])    # one active lane, a full chunk, NCH = 4 with a partial chunk, full width
@pytest.mark.parametrize("vdtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("kind", ["cuckoo", "hkv"])
def test_table_route_equals_chain_route_bitwise(env, kind, vdtype, dim):
  torch, de = env
  t = table(torch, de, kind, vdtype, dim)
  _, _, _, ids_t, seg_t, w_t = batch(torch, 20000, 1400)
  for (i_t, s_t, ww_t), n_rows in (((ids_t, seg_t, w_t), 1400), (edge_batch(torch), 37)):
    G = grad_of(torch, n_rows, dim)
    for combiner in COMBINERS:
      for wt in (ww_t, None):
        got = t._table.find_combine_weight_grad(i_t, s_t, wt, COMB[combiner], G)
        exp = chain(torch, de, t, i_t, s_t, wt, combiner, G)
        assert got.dtype == torch.float32 and tuple(got.shape) == (i_t.numel(),)
        assert torch.equal(bits(torch, got), bits(torch, exp)), (n_rows, combiner, wt is not None)
    if n_rows == 1400:
      assert not bool(got[-4:].any())     # the four entries whose row lies outside [0, n_rows)
  t._table.check_errors()


# ---- 2. exact known answers --------------------------------------------------------------------------------------------------------
# weight lists whose sum is a power of two <= 32 (mean: every quotient is exact), lengths on the batch boundaries
MEAN_ROWS = [[1.0], [0.5, 0.5], [1.0, 0.5, 0.5], [0.5] * 4, [2.0] + [0.5] * 4, [2.0] * 2 + [1.0] * 11 + [0.5] * 2, [1.0] * 16, [2.0] * 16,
             [0.5] * 16, [1.0] * 15 + [0.5] * 2, [1.0] * 31 + [0.5] * 2, []]
SQRTN_ROWS = [[1.0] * 4, [1.0] * 16, [2.0] * 4, [2.0] * 16, [], [1.0] * 4, [2.0] * 16]   # sqrt(S) = 2, 4, 4, 8


def exact_eval(E, G, bounds, w, combiner, dt, reverse):
  """The closed form evaluated in `dt` with every sum sequential: columns and entries ascending, or both descending."""
  E, G, w = E.astype(dt), G.astype(dt), w.astype(dt)
  dw = np.zeros(w.size, dt)
  dim = E.shape[1]
  for r, (b, e) in enumerate(bounds):
    if b >= e:
      continue
    d = np.zeros(e - b, dt)
    for c in (range(dim - 1, -1, -1) if reverse else range(dim)):
      d = d + E[b:e, c] * G[r, c]
    s, ws = dt(0), dt(0)
    for p in (range(e - b - 1, -1, -1) if reverse else range(e - b)):
      s = s + w[b + p] * d[p]
      ws = ws + (w[b + p] * w[b + p] if combiner == "sqrtn" else w[b + p])
    if combiner == "sum":
      dw[b:e] = d
    elif combiner == "mean":
      dw[b:e] = (d - s / ws) / ws
    else:
      dw[b:e] = (d - (s / ws) * w[b:e]) / np.sqrt(ws)
  assert dw.dtype == dt
  return dw


@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("dim", [4, 64, 256])
def test_exact_known_answers(env, dim, combiner):
  torch, de = env
  rng = np.random.default_rng(dim + COMB[combiner])
  lists = SQRTN_ROWS if combiner == "sqrtn" else MEAN_ROWS
  w = np.concatenate([rng.permutation(np.array(x, np.float32)) for x in lists]).astype(np.float32)
  counts = np.array([len(x) for x in lists])
  assert counts.max() <= 33 and set(np.unique(w)) <= {0.5, 1.0, 2.0}
  n_rows = counts.size
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), counts)
  bounds = bounds_of(seg, n_rows)
  ids = rng.integers(0, 60, size=seg.size).astype(np.int64)            # odd ids miss: the default row, all ones
  resident = np.arange(0, 60, 2, dtype=np.int64)
  rows = rng.integers(-2, 3, size=(resident.size, dim)).astype(np.float32)
  G = rng.integers(-2, 3, size=(n_rows, dim)).astype(np.float32)
  E = np.where((ids % 2 == 0)[:, None], rows[ids // 2], np.float32(1.0)).astype(np.float32)
  # the inputs are exact: float64 and float32 in two summation orders give the same numbers
  e64 = exact_eval(E, G, bounds, w, combiner, np.float64, False)
  a32, b32 = exact_eval(E, G, bounds, w, combiner, np.float32, False), exact_eval(E, G, bounds, w, combiner, np.float32, True)
  assert np.array_equal(a32, b32) and np.array_equal(a32.astype(np.float64), e64)
  np.testing.assert_allclose(e64, wgrad_model(E, G, bounds, w, combiner)[0], rtol=0, atol=1e-9)
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.ones(dim), name="wgx_%s_%d" % (combiner, dim), dim=dim)
  t.insert(T(torch, resident), T(torch, rows))
  ids_t, seg_t, w_t, G_t = T(torch, ids), T(torch, seg), T(torch, w), T(torch, G)
  exp = T(torch, a32)
  got = t._table.find_combine_weight_grad(ids_t, seg_t, w_t, COMB[combiner], G_t)
  assert torch.equal(got, exp)
  assert torch.equal(chain(torch, de, t, ids_t, seg_t, w_t, combiner, G_t), exp)
  rs_t = T(torch, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
  assert torch.equal(t._table.find_combine_ragged_weight_grad(rs_t, ids_t, w_t, COMB[combiner], G_t), exp)


# ---- 3. random values against float64 ----------------------------------------------------------------------------------------------
def assert_within_bound(got, exp, Tp, cnt, dim, what):
  err = np.abs(np.asarray(got, np.float64) - exp)
  bound = (dim + cnt + 8) * 2.0 ** -23 * Tp
  ratio = np.max(err / np.maximum(bound, 1e-300))
  print("%s: max |got - exp| = %.3e, max err / bound = %.3f" % (what, err.max() if err.size else 0.0, ratio if err.size else 0.0))
  assert np.all(err <= bound), what


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("dim", [4, 64, 256])
def test_matches_the_float64_closed_form(env, dim, combiner, weighted):
  torch, de = env
  rng = np.random.default_rng(dim * 7 + COMB[combiner] * 2 + weighted)
  n_rows = 300
  counts = rng.integers(0, 7, size=n_rows)
  counts[[0, 5, n_rows - 1]] = 0
  counts[3] = 40
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), counts)
  ids = rng.integers(0, 40, size=seg.size).astype(np.int64)
  w = rng.uniform(0.1, 2.0, size=seg.size).astype(np.float32) if weighted else None     # the weight sums do not cancel
  resident = np.arange(0, 40, 2, dtype=np.int64)           # odd ids miss
  rows = rng.standard_normal((resident.size, dim)).astype(np.float32)
  G = rng.standard_normal((n_rows, dim)).astype(np.float32)
  var = de.Variable(dim=dim, name="wgo_%s_%d_%d" % (combiner, weighted, dim), initializer=0.5)
  var.upsert(T(torch, resident), T(torch, rows))
  tab = oracle.CpuTable(dim)
  tab.insert(resident, rows)
  E = tab.find(ids, np.full(dim, 0.5, np.float32))
  exp, Tp, cnt = wgrad_model(E, G, bounds_of(seg, n_rows), w, combiner)
  wt = None if w is None else T(torch, w)
  got = var.lookup_combined_weight_grad(T(torch, ids), T(torch, seg), wt, combiner, T(torch, G))
  assert got.dtype == torch.float32 and tuple(got.shape) == (seg.size,)
  assert_within_bound(got.cpu().numpy(), exp, Tp, cnt, dim, "table route")
  t = var._tables[0]
  assert torch.equal(bits(torch, chain(torch, de, t, T(torch, ids), T(torch, seg), wt, combiner, T(torch, G))), bits(torch, got))


# ---- 4. ragged -----------------------------------------------------------------------------------------------------------------------
ROW_ALL_PRUNED, ROW_ENDS_PRUNED, NAN_ROW = 10, 11, 9
_RAGGED = {}


def ragged_batch(torch):
  """40 rows: the EDGE_LENGTHS and a 70-entry row; row 10: 6 entries, every weight <= 0; row 11: first and last pruned; rows of
  0..24 entries; ~15 % of the weights 0 or negative, one NaN (row 9)."""
  if not _RAGGED:
    rng = np.random.default_rng(5)
    counts = np.array(EDGE_LENGTHS + [70, 6, 8, 0] + list(rng.integers(0, 25, size=26)) + [0])
    assert counts.size == 40
    rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nnz = int(rs[-1])
    keys, _ = H._universe()
    ids = keys[(rng.zipf(1.2, size=nnz) - 1) % H.POOL_UNIVERSE]
    w = rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)
    bad = rng.random(nnz) < 0.15
    w[bad] = np.where(rng.random(int(bad.sum())) < 0.5, 0.0, -rng.uniform(0.1, 1.0, size=int(bad.sum()))).astype(np.float32)
    w[rs[ROW_ALL_PRUNED]:rs[ROW_ALL_PRUNED + 1]] = [0.0, -1.0, -0.0, -2.5, 0.0, -0.125]
    w[rs[ROW_ENDS_PRUNED]:rs[ROW_ENDS_PRUNED + 1]] = [-1.0, 0.5, 1.5, 0.25, 2.0, 1.0, 0.75, 0.0]
    w[rs[NAN_ROW] + 20] = np.nan
    seg = np.repeat(np.arange(40, dtype=np.int64), counts)
    _RAGGED["b"] = (rs, w, T(torch, rs), T(torch, ids), T(torch, w), T(torch, seg))
  return _RAGGED["b"]


@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("kind,vdtype,dim", [("cuckoo", "float32", 64), ("hkv", "bfloat16", 132), ("cuckoo", "float16", 256),
                                             ("hkv", "float32", 4)])
def test_ragged_equals_the_seg_call_prunes_and_fills(env, kind, vdtype, dim, combiner):
  torch, de = env
  t = table(torch, de, kind, vdtype, dim)._table
  rs, w, rs_t, ids_t, w_t, seg_t = ragged_batch(torch)
  c = COMB[combiner]
  G = grad_of(torch, 40, dim, 4)
  w_clean = torch.where(torch.isnan(w_t), torch.ones_like(w_t), w_t)
  # the ragged call is the seg call on the row ids the splits stand for (int32 splits are widened)
  for wt in (w_clean, None):
    plain = t.find_combine_ragged_weight_grad(rs_t, ids_t, wt, c, G)
    assert torch.equal(bits(torch, plain), bits(torch, t.find_combine_weight_grad(ids_t, seg_t, wt, c, G)))
    assert torch.equal(bits(torch, t.find_combine_ragged_weight_grad(rs_t.to(torch.int32), ids_t, wt, c, G)), bits(torch, plain))
    # FILL without PRUNE changes nothing: a row without members has no entries
    assert torch.equal(bits(torch, t.find_combine_ragged_weight_grad(rs_t, ids_t, wt, c, G, fill_id=12345)), bits(torch, plain))
  # PRUNE: weight 0, negative or NaN -> exactly 0; the members' values are those of the compacted list
  keep = w_t > 0
  assert int((~keep).sum()) > 20 and not bool(keep[rs[NAN_ROW] + 20])
  pruned = t.find_combine_ragged_weight_grad(rs_t, ids_t, w_t, c, G, prune=True)
  assert not bool(bits(torch, pruned[~keep]).any())
  compact = t.find_combine_weight_grad(ids_t[keep], seg_t[keep], w_t[keep], c, G)
  assert torch.equal(bits(torch, pruned[keep]), bits(torch, compact))
  # FILL: the entries of a row without members get 0 (they do already), the other rows are unchanged
  filled = t.find_combine_ragged_weight_grad(rs_t, ids_t, w_t, c, G, prune=True, fill_id=int(ids_t[0]))
  assert torch.equal(bits(torch, filled), bits(torch, pruned))
  assert not bool(bits(torch, filled[rs[ROW_ALL_PRUNED]:rs[ROW_ALL_PRUNED + 1]]).any())
  # PRUNE without weights is ignored
  assert torch.equal(bits(torch, t.find_combine_ragged_weight_grad(rs_t, ids_t, None, c, G, prune=True)), bits(torch, plain))
  t.check_errors()


def _raw_ragged(torch, t, n_rows, rs_ptr, nnz, ids_ptr, w_ptr, combiner, flags, fill_id, g_ptr, dw_ptr):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  return _capi.lib().tfra_table_find_combine_ragged_backprop_weights(t._h, n_rows, rs_ptr, nnz, ids_ptr, w_ptr, combiner, flags, fill_id,
                                                                     _ptr(t._default_value), g_ptr, dw_ptr, _stream(t.device))


def _raw_seg(torch, t, nnz, ids_ptr, seg_ptr, w_ptr, combiner, n_rows, g_ptr, dw_ptr):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  return _capi.lib().tfra_table_find_combine_backprop_weights(t._h, _workspace(t.device), nnz, ids_ptr, seg_ptr, w_ptr, combiner, n_rows,
                                                              _ptr(t._default_value), g_ptr, dw_ptr, _stream(t.device))


def clamped(rs, nnz):
  out = []
  for lo, hi in zip(rs[:-1], rs[1:]):
    b = min(max(int(lo), 0), nnz)
    out.append((b, min(max(int(hi), b), nnz)))
  return out


MALFORMED = {"decreasing": [0, 12, 8, 20, 20, 15, 30, 38], "negative": [-7, 5, -3, -1, 12, 20, 30, 36],
             "too_large": [4, 10, 14, 1 << 40, 20, 64, 30, 36]}


@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_row_splits_are_clamped(env, case, combiner):
  """nnz = 40 of buffers that hold 16 + 64 + 16 elements: every index the splits name lies inside an allocation; an entry
  outside the clamped cover gets 0, an entry in exactly one row what that row alone gives, and the guards stay as they were.
  (An entry that two rows claim is written by both groups: its value is one of theirs or a mix, never a fault.)"""
  torch, de = env
  import ctypes
  dim, GUARD, nnz = 64, 16, 40
  t = table(torch, de, "cuckoo", "float32", dim)._table
  rng = np.random.default_rng(len(case))
  keys, _ = H._universe()
  ids = T(torch, keys[rng.integers(0, H.POOL_UNIVERSE, size=GUARD + 64 + GUARD)])
  w = T(torch, rng.uniform(0.1, 2.0, size=GUARD + 64 + GUARD).astype(np.float32))
  ids0, w0 = ids.clone(), w.clone()
  rs = np.array(MALFORMED[case], dtype=np.int64)
  rs_t = T(torch, rs)
  n_rows = rs.size - 1
  G = grad_of(torch, n_rows, dim, 9)
  dw = torch.full((GUARD + 64 + GUARD,), 7.0, device="cuda")
  P = ctypes.c_void_p
  rc = _raw_ragged(torch, t, n_rows, P(rs_t.data_ptr()), nnz, P(ids.data_ptr() + 8 * GUARD), P(w.data_ptr() + 4 * GUARD), COMB[combiner],
                   0, 0, P(G.data_ptr()), P(dw.data_ptr() + 4 * GUARD))
  assert rc == 0
  torch.cuda.synchronize()
  assert bool((dw[:GUARD] == 7.0).all()) and bool((dw[GUARD + nnz:] == 7.0).all())
  assert torch.equal(ids, ids0) and torch.equal(bits(torch, w), bits(torch, w0))
  got = dw[GUARD:GUARD + nnz]
  ids_n, w_n = ids[GUARD:GUARD + nnz].contiguous(), w[GUARD:GUARD + nnz].contiguous()
  bounds = clamped(rs, nnz)
  cover = np.zeros(nnz, dtype=np.int64)
  for b, e in bounds:
    cover[b:e] += 1
  assert (cover == 0).any() and (cover == 1).any()
  assert not bool(bits(torch, got[T(torch, cover == 0)]).any())
  for r, (b, e) in enumerate(bounds):
    if b < e:
      one = t.find_combine_ragged_weight_grad(torch.tensor([b, e], device="cuda"), ids_n, w_n, COMB[combiner], G[r:r + 1])
      m = T(torch, (cover == 1) & (np.arange(nnz) >= b) & (np.arange(nnz) < e))
      assert torch.equal(bits(torch, got[m]), bits(torch, one[m])), r
  assert bool(torch.isfinite(got).all())
  t.check_errors()


def test_empty_calls_succeed(env):
  torch, de = env
  t = table(torch, de, "cuckoo", "float32", 64)._table
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  z = torch.zeros(6, dtype=torch.int64, device="cuda")
  G = grad_of(torch, 5, 64)
  for combiner in (0, 1, 2):
    assert tuple(t.find_combine_ragged_weight_grad(z, none, None, combiner, G).shape) == (0,)
    assert tuple(t.find_combine_weight_grad(none, none, None, combiner, G).shape) == (0,)
  # entries but no rows: every entry is in no row
  ids = torch.arange(5, device="cuda")
  assert not bool(t.find_combine_weight_grad(ids, torch.zeros_like(ids), None, 1, G[:0]).any())
  assert not bool(t.find_combine_ragged_weight_grad(z[:1], ids, None, 1, G[:0]).any())
  t.check_errors()


# ---- 5. the wrapper ------------------------------------------------------------------------------------------------------------------
N_W, DIM_W, DEFAULT_ID = 50, 8, 4


def _wrapper_case(torch):
  """50 rows of 0..8 entries over resident (even) keys; rows 0, 7 and 49 empty, row 3 pruned away entirely; ~25 % of the weights
  not > 0."""
  rng = np.random.default_rng(77)
  counts = rng.integers(1, 9, size=N_W)
  counts[[0, 7, N_W - 1]] = 0
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  seg = np.repeat(np.arange(N_W, dtype=np.int64), counts)
  ids = ((rng.zipf(1.3, size=seg.size) % 1500) * 2).astype(np.int64)
  w = rng.uniform(0.1, 2.0, size=seg.size).astype(np.float32)
  w[rng.random(seg.size) < 0.25] *= -1.0
  w[seg == 3] = 0.0
  G = rng.standard_normal((N_W, DIM_W)).astype(np.float32)
  return rs, seg, ids, w, G


def _lookup(de, var, form, safe, rs_t, seg_t, ids_t, w_t, combiner, **kw):
  if form == "ragged":
    f = de.ragged_embedding_ops.safe_embedding_lookup_sparse if safe else de.ragged_embedding_ops.embedding_lookup_sparse
    if safe:
      kw["default_id"] = DEFAULT_ID
    return f(var, (rs_t, ids_t), w_t, combiner=combiner, return_trainable=True, **kw)
  if safe:
    return de.safe_embedding_lookup_sparse(var, (seg_t, ids_t), w_t, combiner=combiner, default_id=DEFAULT_ID, return_trainable=True,
                                           num_rows=N_W, **kw)
  return de.embedding_lookup_sparse(var, (seg_t, ids_t), w_t, combiner=combiner, return_trainable=True, num_rows=N_W, **kw)


@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("form", ["tuple", "ragged"])
def test_wrapper_weights_grad(env, monkeypatch, form, safe, combiner):
  torch, de = env
  rs, seg, ids, w, G = _wrapper_case(torch)
  if not safe:
    w = np.abs(w) + np.float32(0.1)     # the plain forms prune nothing: keep the weight sums away from 0
  tag = "%s_%d_%s" % (form, safe, combiner)
  pooled = H.filled_var(torch, de, "wgw_p_" + tag, dim=DIM_W, initializer=0.5)
  called = H.filled_var(torch, de, "wgw_c_" + tag, dim=DIM_W, initializer=lambda shape: torch.full(tuple(shape), 0.5))
  shards = H.filled_var(torch, de, "wgw_s_" + tag, dim=DIM_W, initializer=0.5, devices=["cuda:0", "cuda:0"])
  assert pooled.can_lookup_combined() and not called.can_lookup_combined() and not shards.can_lookup_combined()
  rs_t, seg_t, ids_t, w_t, G_t = T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w), T(torch, G)
  # float64 autograd of the reference's chain on the entries the lookup keeps
  keep = (w > 0) if (safe and combiner != "sum") else np.ones(w.size, dtype=bool)
  E = pooled.lookup(ids_t).cpu().numpy().astype(np.float64)
  exp = np.zeros(w.size)
  exp[keep] = chain_autograd(E[keep], G, seg[keep], w[keep], combiner, N_W)
  model, Tk, ck = wgrad_model(E[keep], G, bounds_of(seg[keep], N_W), w[keep], combiner)
  np.testing.assert_allclose(model, exp[keep], rtol=0, atol=1e-12)
  Tp, cnt = np.zeros(w.size), np.zeros(w.size)
  Tp[keep], cnt[keep] = Tk, ck
  calls = H.Calls(monkeypatch)
  got = {}
  for name, var in (("pooled", pooled), ("callable", called), ("shards", shards)):
    out, tw = _lookup(de, var, form, safe, rs_t, seg_t, ids_t, w_t, combiner)
    assert tuple(out.shape) == (N_W, DIM_W)
    dw = tw.weights_grad(G_t)
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (w.size,)          # the caller's length and order
    assert not bool(bits(torch, dw[T(torch, ~keep)]).any())                    # 0 at pruned entries
    assert_within_bound(dw.cpu().numpy(), exp, Tp, cnt, DIM_W, name)
    got[name] = dw
    if name == "pooled":
      assert calls["tfra_table_find_combine_backprop_weights"] == 1 and calls["tfra_sparse_segment_combine_backprop_weights"] == 0
  assert calls["tfra_table_find_combine_backprop_weights"] == 1 and calls["tfra_sparse_segment_combine_backprop_weights"] == 2
  assert torch.equal(bits(torch, got["pooled"]), bits(torch, got["callable"]))  # same rows: same bits on both routes
  # the answer does not depend on whether the wrapper has resolved its unique ids
  out, tw = _lookup(de, pooled, form, safe, rs_t, seg_t, ids_t, w_t, combiner)
  assert tw.ids.numel() > 0
  assert torch.equal(bits(torch, tw.weights_grad(G_t)), bits(torch, got["pooled"]))
  with pytest.raises(ValueError):
    tw.weights_grad(G_t[:-1])
  with pytest.raises(ValueError):
    tw.weights_grad(G_t.reshape(-1))
  with pytest.raises(ValueError):
    _lookup(de, pooled, form, safe, rs_t, seg_t, ids_t, None, combiner)[1].weights_grad(G_t)
  if form == "tuple":
    with pytest.raises(ValueError):
      _lookup(de, pooled, form, safe, rs_t, seg_t, ids_t, w_t, combiner, max_norm=1.0)[1].weights_grad(G_t)


# ---- 6. the table is untouched -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cuckoo", "hkv"])
def test_the_table_is_untouched(env, kind):
  torch, de = env
  t = table(torch, de, kind, "float32", 64)._table
  rs, w, rs_t, ids_t, w_t, seg_t = ragged_batch(torch)
  G = grad_of(torch, 40, 64)

  def state():
    k, v, s = t.export_all(with_scores=kind == "hkv")
    o = torch.argsort(k)          # (an export's order is not part of its contract)
    return [k[o], bits(torch, v[o])] + ([s[o]] if s is not None else []) + [t.size_device().reshape(-1)]

  before = state()
  for c in (0, 1, 2):
    t.find_combine_weight_grad(ids_t, seg_t, w_t, c, G)
    t.find_combine_ragged_weight_grad(rs_t, ids_t, w_t, c, G, prune=True, fill_id=int(ids_t[0]))
  after = state()
  assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
  t.check_errors()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["int8", "float64", "dim6", "dim260", "misaligned_grad_out", "combiner3", "flags"])
def test_refusals_write_nothing(env, why):
  torch, de = env
  import ctypes
  P = ctypes.c_void_p
  dim = {"dim6": 6, "dim260": 260}.get(why, 8)
  dt = {"int8": torch.int8, "float64": torch.float64}.get(why, torch.float32)
  t = de.CuckooHashTable(torch.int64, dt, torch.zeros(dim, dtype=dt), name="wgr_" + why, dim=dim)._table
  nnz, n_rows = 6, 2
  ids = torch.arange(nnz, device="cuda")
  seg = T(torch, np.array([0, 0, 0, 1, 1, 1], dtype=np.int64))
  rs = T(torch, np.array([0, 3, 6], dtype=np.int64))
  Gbuf = torch.ones(n_rows * dim + 4, device="cuda")
  g_ptr = Gbuf.data_ptr() + (4 if why == "misaligned_grad_out" else 0)
  dw = torch.full((nnz,), 7.0, device="cuda")
  combiner = 3 if why == "combiner3" else 1
  expect = INVALID if why in ("combiner3", "flags") else UNSUPPORTED
  if why != "flags":
    assert _raw_seg(torch, t, nnz, P(ids.data_ptr()), P(seg.data_ptr()), None, combiner, n_rows, P(g_ptr), P(dw.data_ptr())) == expect
  assert _raw_ragged(torch, t, n_rows, P(rs.data_ptr()), nnz, P(ids.data_ptr()), None, combiner, 4 if why == "flags" else 0, 0, P(g_ptr),
                     P(dw.data_ptr())) == expect
  torch.cuda.synchronize()
  assert bool((dw == 7.0).all())
  if why in ("int8", "dim6"):
    from tfra_amd import _capi
    with pytest.raises(_capi.TfraError) as e:
      t.find_combine_weight_grad(ids, seg, None, 1, Gbuf[:n_rows * dim].reshape(n_rows, dim))
    assert e.value.code == UNSUPPORTED
