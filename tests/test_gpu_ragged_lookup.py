"""GPU: the ragged pooled lookup (tfra_table_find_combine_ragged / tfra_multi_find_combine_ragged; Variable.lookup_combined_ragged;
de.ragged_embedding_ops).

The ragged kernels compile find_combine_row — the body of tfra_table_find_combine — with the row's bounds read from row_splits
and, for the safe semantics, with pruned entries skipped in the weight sum and the accumulation and the default row probed by
the group that owns an empty row.  So they must agree BIT FOR BIT with the tuple form on the derived row ids and with the chain
safe_embedding_lookup_sparse runs (prune by boolean mask, find_combine, a lookup of default_id, torch.where): those comparisons
are torch.equal on int32 views, no tolerance.  The float64 model is tests/test_ragged_lookup_abi.py's."""
import ctypes

import numpy as np
import pytest

from tests import sparse_helpers as H
from tests.sparse_helpers import Calls, T, _export_state, bits
from tests.test_ragged_lookup_abi import ragged_bounds, ragged_model

pytestmark = pytest.mark.gpu

IMIN = np.iinfo(np.int64).min
COMB = {"sum": 0, "mean": 1, "sqrtn": 2}
INVALID, UNSUPPORTED = -1, -6
PRUNE, FILL = 1, 2


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


# ---- shared fixtures: tables of 2 000 keys, one batch ---------------------------------------------------------------------------
UNIVERSE = 2500            # distinct keys the ids are drawn from; every fifth one is never inserted (~20 % misses)
FILL_KEY = 777_777_777     # resident, its row holds a -0.0
MISS_KEY = 888_888_888     # never inserted


def _universe():
  rng = np.random.default_rng(99)
  keys = rng.permutation(np.arange(1, UNIVERSE + 1, dtype=np.int64) * 7919 - 9_000_000)   # negative keys too
  return keys, keys[np.arange(UNIVERSE) % 5 != 0]


_TABLES = {}


def table(torch, de, kind, vdtype, dim):
  """A table of `kind` ("cuckoo": growing; "hkv": bounded LRU, filled past its capacity) holding 2 000 keys of the universe,
  INT64_MIN (its side row; INT64_MIN + 1 is not resident) and FILL_KEY, whose row has a -0.0."""
  key = (kind, vdtype, dim)
  if key not in _TABLES:
    dt = getattr(torch, vdtype)
    default = torch.full((dim,), 0.375, dtype=dt)
    if kind == "cuckoo":
      t = de.CuckooHashTable(torch.int64, dt, default, name="rg_c_%s_%d" % (vdtype, dim), dim=dim)
    else:
      t = de.HkvHashTable(torch.int64, dt, default, name="rg_h_%s_%d" % (vdtype, dim), init_capacity=2048, max_capacity=2048,
                          max_hbm_for_values=1 << 26, evict_strategy=de.HkvEvictStrategy.LRU, dim=dim)
      filler = torch.arange(1, 601, device="cuda") * 104729 + 5_000_000_000   # evicted first
      t.insert(filler, torch.ones((filler.numel(), dim), device="cuda").to(dt))
    _, inserted = _universe()
    keys = np.concatenate([inserted, [IMIN, FILL_KEY]])
    g = torch.Generator(device="cuda").manual_seed(dim)
    rows = torch.randn((keys.size, dim), generator=g, device="cuda").to(dt)
    rows[-1, 1] = -0.0
    rows[-1, 2] = 1.5
    t.insert(T(torch, keys), rows)
    _TABLES[key] = t
  return _TABLES[key]


# the lengths that hit every boundary of the walk (16 entries per batch of the group, 4 per inner step), then the prune cases
LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 70, 600]
ROW_ALL_PRUNED, ROW_ENDS_PRUNED, ROW_LATE_SURVIVOR = 13, 14, 15
NAN_ROW = 11
N_ROWS = 40


def _batch():
  """(row_splits, ids, w): rows 0..12 of LENGTHS; row 13: 6 entries, every weight <= 0; row 14: 8 entries, first and last
  pruned; row 15: 40 entries, the only survivor at position 25; row 16 empty; rows 17..38 of 0..24 entries; row 39 empty.
  ids: ~20 % never-inserted keys and both reserved key values.  w: mostly in (0.1, 2), ~12 % zeros / negatives, one NaN (row 11)."""
  rng = np.random.default_rng(4)
  keys, _ = _universe()
  counts = LENGTHS + [6, 8, 40, 0] + list(rng.integers(0, 25, size=22)) + [0]
  assert len(counts) == N_ROWS
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  nnz = int(rs[-1])
  ids = keys[(rng.zipf(1.2, size=nnz) - 1) % UNIVERSE]
  ids[rs[12] + 5], ids[rs[12] + 300], ids[rs[8] + 2], ids[rs[12] + 599] = IMIN, IMIN, IMIN + 1, IMIN + 1
  w = rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)
  bad = rng.random(nnz) < 0.12
  w[bad] = np.where(rng.random(int(bad.sum())) < 0.5, 0.0, -rng.uniform(0.1, 1.0, size=int(bad.sum()))).astype(np.float32)
  w[rs[ROW_ALL_PRUNED]:rs[ROW_ALL_PRUNED + 1]] = [0.0, -1.0, -0.0, -2.5, 0.0, -0.125]
  w[rs[ROW_ENDS_PRUNED]:rs[ROW_ENDS_PRUNED + 1]] = [-1.0, 0.5, 1.5, 0.25, 2.0, 1.0, 0.75, 0.0]
  w[rs[ROW_LATE_SURVIVOR]:rs[ROW_LATE_SURVIVOR + 1]] = -0.5
  w[rs[ROW_LATE_SURVIVOR] + 25] = 1.25
  w[rs[NAN_ROW] + 20] = np.nan
  return rs, ids, w


_BATCH = {}


def batch(torch):
  if not _BATCH:
    rs, ids, w = _batch()
    seg = np.repeat(np.arange(N_ROWS, dtype=np.int64), np.diff(rs))
    _BATCH["b"] = (rs, ids, w, T(torch, rs), T(torch, ids), T(torch, w), T(torch, seg))
  return _BATCH["b"]


def safe_chain(torch, t, seg_t, ids_t, w_t, combiner, n, prune, fill_id):
  """What safe_embedding_lookup_sparse runs today, written out on the device table: prune by boolean mask, the pooled lookup of
  the compacted list, a lookup of the fill id and torch.where over the rows left empty."""
  if prune and w_t is not None:
    keep = w_t > 0
    seg_t, ids_t, w_t = seg_t[keep], ids_t[keep], w_t[keep]
  res = t._table.find_combine(ids_t, seg_t, w_t, COMB[combiner], n)
  if fill_id is not None:
    empty = torch.ones(n, dtype=torch.bool, device="cuda")
    empty[seg_t] = False
    d = t._table.find(torch.tensor([fill_id], dtype=torch.int64, device="cuda")).to(torch.float32)
    res = torch.where(empty[:, None], d, res)
  return res


# ---- 1. bitwise against the tuple form and against the safe chain ------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("dim", [4, 64, 128, 256])
@pytest.mark.parametrize("vdtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("kind", ["cuckoo", "hkv"])
def test_ragged_equals_the_tuple_form_and_the_safe_chain_bitwise(env, kind, vdtype, dim, combiner, weighted):
  torch, de = env
  rs, ids, w, rs_t, ids_t, w_t, seg_t = batch(torch)
  t = table(torch, de, kind, vdtype, dim)
  wt = w_t if weighted else None
  c = COMB[combiner]
  got = t._table.find_combine_ragged(rs_t, ids_t, wt, c)
  assert got.dtype == torch.float32 and tuple(got.shape) == (N_ROWS, dim)
  assert torch.equal(bits(torch, got), bits(torch, t._table.find_combine(ids_t, seg_t, wt, c, N_ROWS)))
  assert not bool(got[0].any()) and not bool(got[16].any()) and not bool(got[N_ROWS - 1].any())
  assert torch.equal(bits(torch, t._table.find_combine_ragged(rs_t.to(torch.int32), ids_t, wt, c)), bits(torch, got))
  # prune alone (without weights the flag changes nothing): the all-pruned row is zeros
  got = t._table.find_combine_ragged(rs_t, ids_t, wt, c, prune=True)
  assert torch.equal(bits(torch, got), bits(torch, safe_chain(torch, t, seg_t, ids_t, wt, combiner, N_ROWS, True, None)))
  if weighted:
    assert not bool(got[ROW_ALL_PRUNED].any())
    assert bool(torch.isfinite(got).all())               # the NaN weight is no member
  # the fill row, in turn: resident with a -0.0, a miss, a reserved key that is resident, a reserved key that is not
  for fill_id in (FILL_KEY, MISS_KEY, int(IMIN), int(IMIN) + 1):
    for prune in (False, True):
      got = t._table.find_combine_ragged(rs_t, ids_t, wt, c, prune=prune, fill_id=fill_id)
      exp = safe_chain(torch, t, seg_t, ids_t, wt, combiner, N_ROWS, prune, fill_id)
      assert torch.equal(bits(torch, got), bits(torch, exp)), (fill_id, prune)
      frow = t._table.find(torch.tensor([fill_id], device="cuda")).to(torch.float32)[0]
      assert torch.equal(bits(torch, got[0]), bits(torch, frow)) and torch.equal(bits(torch, got[16]), bits(torch, frow))
      if weighted and prune:
        assert torch.equal(bits(torch, got[ROW_ALL_PRUNED]), bits(torch, frow))
      else:
        assert torch.equal(bits(torch, got[ROW_ALL_PRUNED]), bits(torch, t._table.find_combine(ids_t, seg_t, wt, c, N_ROWS)[ROW_ALL_PRUNED]))
  if kind == "cuckoo":   # (a bounded table may have evicted the key; the chain comparison above holds either way)
    got = t._table.find_combine_ragged(rs_t, ids_t, wt, c, fill_id=FILL_KEY)
    assert float(got[0, 2]) == 1.5 and float(got[0, 1]) == 0.0 and bool(torch.signbit(got[0, 1]))   # -0.0 survived
  miss = t._table.find_combine_ragged(rs_t, ids_t, wt, c, fill_id=MISS_KEY)
  assert bool((miss[0] == 0.375).all())
  t._table.check_errors()


# ---- 2. against the float64 model ------------------------------------------------------------------------------------------------
def assert_close_to_model(got, exp, den, amp, emax, max_left_out):
  """|got - exp| <= 1e-6 (1 + sum |w| / |den| max |E|) per row — the error of a row's float32 sums scales with sum |w| / |sum w|.
  A row may be left out only if |den| < 1e-3 sum |w| (its weights cancel), and at most `max_left_out` rows."""
  nan = np.isnan(exp).any(1)
  assert np.isnan(got[nan]).all()
  cancel = (~nan) & (np.abs(den) < 1e-3 * amp)
  assert int(cancel.sum()) <= max_left_out, "the batch leaves out %d rows" % int(cancel.sum())
  ok = ~nan & ~cancel
  tol = 1e-6 * (1 + (amp / np.where(den != 0, np.abs(den), 1))[:, None] * emax)
  err = np.abs(got[ok] - exp[ok])
  assert np.all(err <= np.broadcast_to(tol, exp.shape)[ok]), float((err / np.broadcast_to(tol, exp.shape)[ok]).max())


@pytest.mark.parametrize("mode", ["plain", "prune", "prune_fill", "fill"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("vdtype,dim", [("float32", 4), ("float32", 64), ("float32", 256), ("float16", 128), ("bfloat16", 64)])
def test_ragged_matches_the_model(env, vdtype, dim, combiner, weighted, mode):
  torch, de = env
  rs, ids, w, rs_t, ids_t, w_t, seg_t = batch(torch)
  t = table(torch, de, "cuckoo", vdtype, dim)
  E = t._table.find(ids_t).to(torch.float32).cpu().numpy().astype(np.float64)     # half rows up-cast exactly
  prune, fill_id = mode.startswith("prune"), (FILL_KEY if mode.endswith("fill") else None)
  fill_row = None if fill_id is None else t._table.find(torch.tensor([fill_id], device="cuda")).to(torch.float32)[0].cpu().numpy()
  wn = w if weighted else None
  exp, den, amp = ragged_model(rs, ids.size, E, wn, combiner, prune=prune, fill_row=fill_row)
  got = t._table.find_combine_ragged(rs_t, ids_t, w_t if weighted else None, COMB[combiner], prune=prune, fill_id=fill_id)
  assert_close_to_model(got.cpu().numpy().astype(np.float64), exp, den, amp, np.abs(E).max(), int(0.02 * N_ROWS))


# ---- 3. malformed row_splits: memory-safe by construction ------------------------------------------------------------------------
def _raw_single(torch, t, n_rows, rs_ptr, nnz, ids_t, w_t, combiner, flags, fill_id, out, ids_ptr=None):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  dev = t._table.device
  return _capi.lib().tfra_table_find_combine_ragged(t._table._h, n_rows, rs_ptr, nnz, _ptr(ids_t) if ids_ptr is None else ids_ptr,
                                                    _ptr(w_t), combiner, flags, fill_id, _ptr(t._default_value), _ptr(out),
                                                    _stream(dev))


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("dim", [64, 256])
def test_malformed_row_splits_are_clamped(env, dim, combiner):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import _ptr
  rng = np.random.default_rng(dim)
  keys, _ = _universe()
  ids = keys[rng.integers(0, UNIVERSE, size=64)]              # buffers of 64 entries, nnz = 40 passed: every index the
  w = rng.uniform(0.1, 2.0, size=64).astype(np.float32)       # splits name lies inside an allocation
  rs = np.array([-5, 3, 10, 7, 20, 64, 30, 50, 41, 64, 12, -1, 40, 39], dtype=np.int64)
  n_rows, nnz = rs.size - 1, 40
  assert ragged_bounds(rs, nnz)[:6] == [(0, 3), (3, 10), (10, 10), (7, 20), (20, 40), (40, 40)]
  t = table(torch, de, "cuckoo", "float32", dim)
  ids_t, w_t, rs_t = T(torch, ids), T(torch, w), T(torch, rs)
  E = t._table.find(ids_t).cpu().numpy().astype(np.float64)
  fill = t._table.find(torch.tensor([FILL_KEY], device="cuda"))[0].cpu().numpy()
  for flags, prune, fill_row in ((0, False, None), (PRUNE | FILL, True, fill)):
    out = torch.full((n_rows, dim), 7.0, device="cuda")
    assert _raw_single(torch, t, n_rows, _ptr(rs_t), nnz, ids_t, w_t, COMB[combiner], flags, FILL_KEY, out) == 0
    exp, den, amp = ragged_model(rs, nnz, E, w, combiner, prune=prune, fill_row=fill_row)
    assert_close_to_model(out.cpu().numpy().astype(np.float64), exp, den, amp, np.abs(E).max(), 0)
    # and bit for bit what the clamped splits give row by row
    for r, (b, e) in enumerate(ragged_bounds(rs, nnz)):
      one = t._table.find_combine_ragged(torch.tensor([b, e], device="cuda"), ids_t, w_t, COMB[combiner], prune=prune,
                                         fill_id=FILL_KEY if flags else None)
      assert torch.equal(bits(torch, out[r]), bits(torch, one[0])), r
  t._table.check_errors()


# ---- 4. launch counts ------------------------------------------------------------------------------------------------------------
def filled_var(torch, de, name, **kw):
  return H.filled_var(torch, de, name, scale=3, **kw)


def sparse_case(rng, n_rows=200):
  """(row_splits, seg, ids, w): rows of 0..8 entries, three empty ones; ~25 % of the weights not > 0."""
  counts = rng.integers(0, 9, size=n_rows)
  counts[[0, 7, n_rows - 1]] = 0
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = (rng.zipf(1.3, size=seg.size) % 3000).astype(np.int64)
  w = rng.uniform(0.1, 2.0, size=seg.size).astype(np.float32)
  w[rng.random(seg.size) < 0.25] *= -1.0
  w[seg == 3] = 0.0
  return rs, seg, ids, w


def test_the_ragged_forward_is_one_call_and_the_safe_form_never_masks(env, monkeypatch):
  torch, de = env
  from tfra_amd.dynamic_embedding import ragged_embedding_ops as reo
  from tfra_amd.dynamic_embedding import variable as tuple_form
  rs, seg, ids, w = sparse_case(np.random.default_rng(5))
  var = filled_var(torch, de, "rgl_calls", initializer=0.5)
  rs_t, seg_t, ids_t, w_t = T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w)
  exp = de.safe_embedding_lookup_sparse(var, (seg_t, ids_t), w_t, combiner="mean", default_id=4, num_rows=200)
  calls = Calls(monkeypatch)
  out = var.lookup_combined_ragged(rs_t, ids_t, w_t, "mean")
  assert calls["tfra_table_find_combine_ragged"] == 1 and sum(calls.n.values()) == 1

  def boom(*a, **k):
    raise AssertionError("the safe ragged forward must not run _safe_sparse_args")

  monkeypatch.setattr(reo, "_safe_sparse_args", boom)
  monkeypatch.setattr(tuple_form, "_safe_sparse_args", boom)
  got = reo.safe_embedding_lookup_sparse(var, (rs_t, ids_t), w_t, combiner="mean", default_id=4)
  assert calls["tfra_table_find_combine_ragged"] == 2 and sum(calls.n.values()) == 2
  assert calls["tfra_table_find_combine"] == 0 and calls["tfra_unique"] == 0 and calls["tfra_sparse_segment_combine"] == 0
  assert calls["tfra_table_find"] == 0
  assert torch.equal(bits(torch, got), bits(torch, exp))
  assert torch.equal(bits(torch, out), bits(torch, var.lookup_combined(ids_t, seg_t, w_t, "mean", 200)))


# ---- 5. grouped ------------------------------------------------------------------------------------------------------------------
def _group_requests(torch, de):
  """Six descriptors over four tables, two dtypes, three row-width classes: (float32, 64) twice — once safe, once with a PRUNE
  that changes nothing —, (float32, 128) plain and with n_rows == 0, (bfloat16, 64) fill only, (float32, 256) nnz == 0 with fill."""
  rs, ids, w, rs_t, ids_t, w_t, seg_t = batch(torch)
  a, b = table(torch, de, "cuckoo", "float32", 64), table(torch, de, "hkv", "float32", 128)
  c, d = table(torch, de, "cuckoo", "bfloat16", 64), table(torch, de, "cuckoo", "float32", 256)
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  zeros5 = torch.zeros(6, dtype=torch.int64, device="cuda")
  return [(a, rs_t, ids_t, w_t, 1, True, FILL_KEY), (b, rs_t, ids_t, w_t, 2, False, None), (c, rs_t, ids_t, None, 0, False, int(IMIN)),
          (a, rs_t, ids_t, None, 1, True, None), (d, zeros5, none, None, 1, False, MISS_KEY),
          (b, torch.zeros(1, dtype=torch.int64, device="cuda"), none, None, 0, False, FILL_KEY)]


def test_grouped_call_equals_the_single_calls_with_one_launch_per_class(env, monkeypatch):
  torch, de = env
  from tfra_amd.dynamic_embedding import table_ops
  reqs = _group_requests(torch, de)
  singles = [r[0]._table.find_combine_ragged(r[1], r[2], r[3], r[4], prune=r[5], fill_id=r[6]) for r in reqs]
  calls = Calls(monkeypatch)
  outs, launches = table_ops.find_combine_ragged_many(reqs, return_launches=True)
  assert calls["tfra_multi_find_combine_ragged"] == 1 and sum(calls.n.values()) == 1
  # (f32, NCH 1, safe), (f32, NCH 2, plain), (bf16, NCH 1, safe), (f32, NCH 1, plain), (f32, NCH 4, safe); the sixth is dropped
  assert launches == 5
  for i, (o, s) in enumerate(zip(outs, singles)):
    assert tuple(o.shape) == tuple(s.shape) and torch.equal(bits(torch, o), bits(torch, s)), i
  assert tuple(outs[5].shape) == (0, 128) and bool((outs[4] == 0.375).all())
  outs2 = table_ops.find_combine_ragged_many(reqs)      # back to back: the staging ring
  for o, s in zip(outs2, singles):
    assert torch.equal(bits(torch, o), bits(torch, s))


@pytest.mark.parametrize("fault", ["flag_bits", "null_row_splits", "misaligned_row_splits", "reserved", "combiner"])
def test_grouped_call_refuses_a_faulty_descriptor_like_the_single_call(env, fault):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  reqs = _group_requests(torch, de)[:5]
  n = len(reqs)
  descs = (_capi.FindCombineRaggedDesc * n)()
  keep, outs = [], []
  for i, (t, rs_t, ids_t, w_t, comb, prune, fill_id) in enumerate(reqs):
    rs_a, ids_a, w_a, flags, fill, dflt, _ = t._table._find_combine_ragged_args(rs_t, ids_t, w_t, prune, fill_id, None)
    out = torch.full((rs_a.numel() - 1, t._table._dim), 7.0, device="cuda")
    keep.append((rs_a, ids_a, w_a, dflt))
    outs.append(out)
    e = descs[i]
    e.struct_size, e.combiner, e.table = ctypes.sizeof(_capi.FindCombineRaggedDesc), comb, t._table._h.value
    e.n_rows, e.row_splits, e.nnz, e.ids = rs_a.numel() - 1, rs_a.data_ptr(), ids_a.numel(), ids_a.data_ptr()
    e.weights, e.flags, e.reserved, e.fill_id = (w_a.data_ptr() if w_a is not None else None), flags, 0, fill
    e.default_row, e.out = dflt.data_ptr(), out.data_ptr()
  e = descs[2]
  t = reqs[2][0]
  single = dict(n_rows=e.n_rows, rs=e.row_splits, flags=e.flags, combiner=e.combiner)
  if fault == "flag_bits":
    e.flags = single["flags"] = 4 | FILL
  elif fault == "null_row_splits":
    e.row_splits = single["rs"] = None
  elif fault == "misaligned_row_splits":
    e.row_splits = single["rs"] = e.row_splits + 4
  elif fault == "reserved":
    e.reserved = 1
  else:
    e.combiner = single["combiner"] = 3
  dev = t._table.device
  lib = _capi.lib()
  launches = ctypes.c_uint32(99)
  rc = lib.tfra_multi_find_combine_ragged(_workspace(dev), n, ctypes.c_void_p(ctypes.addressof(descs)),
                                          ctypes.c_void_p(ctypes.addressof(launches)), _stream(dev))
  msg = lib.tfra_last_error().decode()
  assert rc == (UNSUPPORTED if fault == "misaligned_row_splits" else INVALID) and launches.value == 0
  assert msg.startswith("multi_find_combine_ragged: descriptor 2: "), msg
  if fault != "reserved":      # (the single call has no such field)
    lone = torch.full((reqs[2][1].numel() - 1, t._table._dim), 7.0, device="cuda")
    rc1 = _raw_single(torch, t, single["n_rows"], single["rs"], e.nnz, keep[2][1], None, single["combiner"], single["flags"],
                      e.fill_id, lone)
    msg1 = lib.tfra_last_error().decode()
    assert rc1 == rc and msg1.startswith("find_combine_ragged: ")
    assert msg1[len("find_combine_ragged: "):] == msg[len("multi_find_combine_ragged: descriptor 2: "):]
    outs.append(lone)
  else:
    assert "reserved" in msg
  torch.cuda.synchronize()
  for o in outs:
    assert bool((o == 7.0).all())
  for r in reqs:
    r[0]._table.check_errors()


def test_single_call_argument_errors_and_empty_calls(env):
  torch, de = env
  from tfra_amd import _capi
  t = table(torch, de, "cuckoo", "float32", 64)
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  z = torch.zeros(6, dtype=torch.int64, device="cuda")
  out = t._table.find_combine_ragged(z, none, None, 1)
  assert tuple(out.shape) == (5, 64) and not bool(out.any())                    # nnz == 0 without FILL: zeros
  out = t._table.find_combine_ragged(z, none, None, 1, fill_id=MISS_KEY)
  assert bool((out == 0.375).all())                                             # with FILL: every row is the fill row
  assert tuple(t._table.find_combine_ragged(z[:1], none, None, 0).shape) == (0, 64)
  t8 = de.CuckooHashTable(torch.int64, torch.int8, torch.zeros(8, dtype=torch.int8), name="rg_i8", dim=8)
  with pytest.raises(_capi.TfraError) as e:
    t8._table.find_combine_ragged(z, none, None, 0)
  assert e.value.code == UNSUPPORTED
  with pytest.raises(ValueError):
    t._table.find_combine_ragged(z, torch.arange(4, device="cuda"), torch.ones(3, device="cuda"), 0)
  with pytest.raises(TypeError):
    t._table.find_combine_ragged(z.to(torch.float32), none, None, 0)
  t._table.check_errors()


# ---- 6. the public functions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", [False, True])          # int32 keys and int32 row_splits
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_public_functions_equal_the_tuple_forms(env, combiner, narrow):
  torch, de = env
  reo = de.ragged_embedding_ops
  rs, seg, ids, w = sparse_case(np.random.default_rng(COMB[combiner]))
  n = 200
  kd = torch.int32 if narrow else torch.int64
  va = filled_var(torch, de, "rgp_a_%s_%d" % (combiner, narrow), key_dtype=kd, initializer=0.5)
  vb = filled_var(torch, de, "rgp_b_%s_%d" % (combiner, narrow), dim=128, key_dtype=kd, value_dtype=torch.bfloat16, initializer=0.25)
  rs_t = T(torch, rs.astype(np.int32) if narrow else rs)
  ids_t = T(torch, ids.astype(np.int32) if narrow else ids)
  seg_t, w_t = T(torch, seg), T(torch, w)
  for wt in (w_t, None):
    for var in (va, vb):
      got = reo.embedding_lookup_sparse(var, (rs_t, ids_t), wt, combiner=combiner)
      assert torch.equal(got, de.embedding_lookup_sparse(var, (seg_t, ids_t), wt, combiner=combiner, num_rows=n))
      for default_id in (None, 4, 5):                       # 4 resident, 5 a miss
        got = reo.safe_embedding_lookup_sparse(var, (rs_t, ids_t), wt, combiner=combiner, default_id=default_id)
        exp = de.safe_embedding_lookup_sparse(var, (seg_t, ids_t), wt, combiner=combiner, default_id=default_id, num_rows=n)
        assert torch.equal(bits(torch, got), bits(torch, exp))
    got = reo.embedding_lookup_sparse_many([va, vb, va], [(rs_t, ids_t)] * 3, [wt, wt, None], combiner=[combiner, "sum", "mean"])
    exp = de.embedding_lookup_sparse_many([va, vb, va], [(seg_t, ids_t)] * 3, [wt, wt, None], combiner=[combiner, "sum", "mean"],
                                          num_rows=n)
    assert len(got) == 3 and all(torch.equal(bits(torch, g), bits(torch, x)) for g, x in zip(got, exp))
    got = reo.safe_embedding_lookup_sparse_many([va, vb, va], [(rs_t, ids_t)] * 3, [wt, wt, None], combiner=[combiner, "sum", "mean"],
                                                default_id=[4, None, 5])
    exp = de.safe_embedding_lookup_sparse_many([va, vb, va], [(seg_t, ids_t)] * 3, [wt, wt, None], combiner=[combiner, "sum", "mean"],
                                               default_id=[4, None, 5], num_rows=n)
    assert len(got) == 3 and all(torch.equal(bits(torch, g), bits(torch, x)) for g, x in zip(got, exp))


@pytest.mark.parametrize("why", ["shards2", "dim6", "callable_init", "bp_v2", "int8"])
def test_ineligible_variables_take_the_tuple_form(env, monkeypatch, why):
  torch, de = env
  reo = de.ragged_embedding_ops
  rs, seg, ids, w = sparse_case(np.random.default_rng(3))
  n = 200
  dim = 6 if why == "dim6" else 8
  kw = dict(initializer=0.5)
  if why == "shards2":
    kw["devices"] = ["cuda:0", "cuda:0"]
  if why == "callable_init":
    kw["initializer"] = lambda shape: torch.full(tuple(shape), 0.5)
  if why == "bp_v2":
    kw["bp_v2"] = True
  if why == "int8":
    kw = dict(initializer=3, value_dtype=torch.int8)
  var = filled_var(torch, de, "rgi_" + why, dim=dim, **kw)
  good = filled_var(torch, de, "rgi_good_" + why, initializer=0.5)
  rs_t, seg_t, ids_t, w_t = T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w)
  calls = Calls(monkeypatch)
  got = reo.embedding_lookup_sparse(var, (rs_t, ids_t), w_t, combiner="mean")
  assert calls["tfra_table_find_combine_ragged"] == 0 and calls["tfra_unique"] == 1 and calls["tfra_sparse_segment_combine"] == 1
  assert torch.equal(bits(torch, got), bits(torch, de.embedding_lookup_sparse(var, (seg_t, ids_t), w_t, combiner="mean", num_rows=n)))
  got = reo.safe_embedding_lookup_sparse(var, (rs_t, ids_t), w_t, combiner="sqrtn", default_id=4)
  exp = de.safe_embedding_lookup_sparse(var, (seg_t, ids_t), w_t, combiner="sqrtn", default_id=4, num_rows=n)
  assert torch.equal(bits(torch, got), bits(torch, exp))
  got = reo.safe_embedding_lookup_sparse_many([good, var], [(rs_t, ids_t)] * 2, [w_t, w_t], combiner="mean", default_id=[5, 4])
  exp = de.safe_embedding_lookup_sparse_many([good, var], [(seg_t, ids_t)] * 2, [w_t, w_t], combiner="mean", default_id=[5, 4],
                                             num_rows=n)
  assert all(torch.equal(bits(torch, g), bits(torch, x)) for g, x in zip(got, exp))
  got = reo.embedding_lookup_sparse_many([good, var], [(rs_t, ids_t)] * 2, None, combiner="sum")
  exp = de.embedding_lookup_sparse_many([good, var], [(seg_t, ids_t)] * 2, None, combiner="sum", num_rows=n)
  assert all(torch.equal(bits(torch, g), bits(torch, x)) for g, x in zip(got, exp))


# ---- 7. training -----------------------------------------------------------------------------------------------------------------
def _train_case(torch):
  """128 rows, duplicates within and across rows, two empty rows, ~20 % of the weights not > 0."""
  rng = np.random.default_rng(31)
  counts = rng.integers(1, 12, size=128)
  counts[[5, 127]] = 0
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  seg = np.repeat(np.arange(128), counts).astype(np.int64)
  ids = (rng.zipf(1.3, size=seg.size) % 300).astype(np.int64)
  ids[1] = ids[0]
  w = rng.uniform(0.1, 2.0, size=seg.size).astype(np.float32)
  w[rng.random(seg.size) < 0.2] *= -1.0
  G = (rng.standard_normal((128, 64)) * 0.01).astype(np.float32)
  return T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w), T(torch, G)


def _twins(torch, de, tag, n):
  opt = de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  va = [de.Variable(dim=64, name="rgt_a_%s_%d" % (tag, i), initializer=0.5, **kw) for i in range(n)]
  vb = [de.Variable(dim=64, name="rgt_b_%s_%d" % (tag, i), initializer=0.5, **kw) for i in range(n)]
  return opt, va, vb, de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)


def _same_state(torch, de, opt, da, db, va, vb):
  for a, b in zip(va, vb):
    sa, sb = _export_state(torch, de, da, opt, a), _export_state(torch, de, db, opt, b)
    assert len(sa) == len(sb) == 2 + len(opt.slots) and sa[0].numel() > 0
    for x, y in zip(sa, sb):
      assert torch.equal(x, y)


@pytest.mark.parametrize("safe", [False, True])
def test_training_through_the_ragged_forward_matches_the_tuple_form(env, safe):
  torch, de = env
  reo = de.ragged_embedding_ops
  rs_t, seg_t, ids_t, w_t, G = _train_case(torch)
  opt, (va,), (vb,), da, db = _twins(torch, de, "s%d" % safe, 1)
  for step in range(2):
    if safe:
      out_a, twa = reo.safe_embedding_lookup_sparse(va, (rs_t, ids_t), w_t, combiner="mean", default_id=7, return_trainable=True)
      out_b, twb = de.safe_embedding_lookup_sparse(vb, (seg_t, ids_t), w_t, combiner="mean", default_id=7, return_trainable=True,
                                                   num_rows=128)
    else:
      out_a, twa = reo.embedding_lookup_sparse(va, (rs_t, ids_t), w_t, combiner="sqrtn", return_trainable=True)
      out_b, twb = de.embedding_lookup_sparse(vb, (seg_t, ids_t), w_t, combiner="sqrtn", return_trainable=True, num_rows=128)
    assert isinstance(twa, de.SparseTrainableWrapper)
    assert torch.equal(bits(torch, out_a), bits(torch, out_b))
    da.apply_combined_gradients([(G, twa)])
    db.apply_combined_gradients([(G, twb)])
    _same_state(torch, de, opt, da, db, [va], [vb])


@pytest.mark.parametrize("safe", [False, True])
def test_training_through_the_grouped_ragged_forward_matches_the_tuple_form(env, safe):
  torch, de = env
  reo = de.ragged_embedding_ops
  rs_t, seg_t, ids_t, w_t, G = _train_case(torch)
  opt, va, vb, da, db = _twins(torch, de, "m%d" % safe, 3)
  ws = [w_t, None, w_t]
  combs = ["mean", "sum", "sqrtn"]
  for step in range(2):
    if safe:
      ra = reo.safe_embedding_lookup_sparse_many(va, [(rs_t, ids_t)] * 3, ws, combiner=combs, default_id=[7, None, 9],
                                                 return_trainable=True)
      rb = de.safe_embedding_lookup_sparse_many(vb, [(seg_t, ids_t)] * 3, ws, combiner=combs, default_id=[7, None, 9],
                                                return_trainable=True, num_rows=128)
    else:
      ra = reo.embedding_lookup_sparse_many(va, [(rs_t, ids_t)] * 3, ws, combiner=combs, return_trainable=True)
      rb = de.embedding_lookup_sparse_many(vb, [(seg_t, ids_t)] * 3, ws, combiner=combs, return_trainable=True, num_rows=128)
    for (oa, _), (ob, _) in zip(ra, rb):
      assert torch.equal(bits(torch, oa), bits(torch, ob))
    da.apply_combined_gradients_many([(G, tw) for _, tw in ra])
    db.apply_combined_gradients_many([(G, tw) for _, tw in rb])
    _same_state(torch, de, opt, da, db, va, vb)
