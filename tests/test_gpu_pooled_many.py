"""GPU: the grouped pooled lookup (tfra_multi_find_combine; table_ops.find_combine_many; embedding_lookup_sparse_many and
safe_embedding_lookup_sparse_many).

The reference of every case is the single-table call (tfra_table_find_combine / embedding_lookup_sparse), itself pinned to the
oracle by tests/test_gpu_pooled_lookup.py.  Both forms run one device function (find_combine_row, csrc/tfra_pool.hip), so they
must agree BIT FOR BIT: every comparison is torch.equal on int32 views, no tolerance."""
import ctypes

import numpy as np
import pytest

from tests import sparse_helpers as H

pytestmark = pytest.mark.gpu

COMB = H.COMB
INVALID, UNSUPPORTED = -1, -6
T, bits, _raw, _desc = H.T, H.bits, H._raw, H._desc


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def many(de, reqs, **kw):
  from tfra_amd.dynamic_embedding import table_ops
  return table_ops.find_combine_many(reqs, **kw)


def single(req):
  t = req[0]
  return getattr(t, "_table", t).find_combine(*req[1:])


def assert_same(torch, got, reqs):
  assert len(got) == len(reqs)
  for i, (g, req) in enumerate(zip(got, reqs)):
    exp = single(req)
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(exp.shape), i
    assert torch.equal(bits(torch, g), bits(torch, exp)), "descriptor %d differs from its single call" % i


def head(torch, n_rows, spill=20):
  """The 20 000-entry batch cut after its rows < n_rows + spill: the tail's seg values lie outside [0, n_rows)."""
  ids, seg, w, ids_t, seg_t, w_t = H.batch(torch, 20000, 1400)
  k = int(np.searchsorted(seg, n_rows + spill))
  return ids_t[:k], seg_t[:k], w_t[:k]


# ---- 1. a mixed list -----------------------------------------------------------------------------------------------------------
def test_mixed_list_equals_the_single_calls_bitwise(env):
  torch, de = env
  ids, seg, w, ids_t, seg_t, w_t = H.batch(torch, 20000, 1400)
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  c = lambda vd, dim: H.table(torch, de, "cuckoo", vd, dim)
  i16, s16, w16 = head(torch, 16)
  i17, s17, w17 = head(torch, 17)
  i300, s300, w300 = head(torch, 300)
  reqs = [
      (c("float32", 4), ids_t[3000:3001], torch.zeros(1, dtype=torch.int64, device="cuda"), w_t[3000:3001], COMB["sum"], 1),
      (c("float32", 64), i16, s16, None, COMB["mean"], 16),
      (c("float32", 128), i17, s17, w17, COMB["sqrtn"], 17),
      (c("float32", 256), i300, s300, None, COMB["sum"], 300),
      (c("float16", 64), ids_t, seg_t, w_t, COMB["mean"], 1400),          # the 2 000-entry row
      (c("bfloat16", 128), i300, s300, w300, COMB["sqrtn"], 300),
      (H.table(torch, de, "hkv", "float32", 64), i17, s17, w17, COMB["mean"], 17),
      (c("float32", 64), none, none, None, COMB["mean"], 40),            # nnz == 0: zeros
      (c("float32", 128), i16, s16, w16, COMB["sum"], 0),                # n_rows == 0: skipped
  ]
  got, launches = many(de, reqs, return_launches=True)
  assert_same(torch, got, reqs)
  assert tuple(got[7].shape) == (40, 64) and not bool(got[7].any())
  assert tuple(got[8].shape) == (0, 128)
  assert got[4][3].any() and not bool(got[4][0].any())                  # the long row is there, an empty row is zeros
  # bounds + float32 NCH 1 / 2 / 4 + float16 NCH 1 + bfloat16 NCH 2
  assert launches == 1 + 5
  for r in reqs:
    r[0]._table.check_errors()


# ---- 2. neighbours do not leak ---------------------------------------------------------------------------------------------------
def test_adjacent_descriptors_of_one_class_do_not_read_each_other(env):
  torch, de = env
  ids, seg, w, ids_t, seg_t, w_t = H.batch(torch, 20000, 1400)
  seg_a = np.array([0, 0, 1, 3, 3, 3, 5, 5], dtype=np.int64)              # ends with 5 ...
  seg_b = np.array([5, 5, 5, 6, 7, 7], dtype=np.int64)                    # ... and the next one begins with 5
  seg_all = T(torch, np.concatenate([seg_a, seg_b]))
  ids_all = ids_t[100:100 + seg_all.numel()].clone()                      # one allocation, adjacent slices
  w_all = w_t[100:100 + seg_all.numel()].clone()
  na = seg_a.size
  ta, tb = H.table(torch, de, "cuckoo", "float32", 64), H.table(torch, de, "cuckoo", "float32", 4)   # both float32, NCH 1
  for comb in COMB.values():
    reqs = [(ta, ids_all[:na], seg_all[:na], w_all[:na], comb, 8), (tb, ids_all[na:], seg_all[na:], w_all[na:], comb, 8)]
    assert ids_all[na:].data_ptr() == ids_all.data_ptr() + 8 * na
    got = many(de, reqs)
    assert_same(torch, got, reqs)
    assert not bool(got[0][6].any()) and not bool(got[1][4].any())      # rows without entries


# ---- 3. the same table twice ------------------------------------------------------------------------------------------------------
def test_one_table_in_two_descriptors(env):
  torch, de = env
  t = H.table(torch, de, "cuckoo", "float32", 64)
  i16, s16, w16 = head(torch, 16)
  i300, s300, w300 = head(torch, 300)
  d1 = torch.full((64,), -2.5, device="cuda")
  d2 = torch.full((64,), 9.0, device="cuda")
  reqs = [(t, i16, s16, w16, COMB["mean"], 16, d1), (t, i300, s300, None, COMB["sum"], 300, d2),
          (H.table(torch, de, "cuckoo", "float32", 128), i16, s16, None, COMB["sqrtn"], 16)]
  got, launches = many(de, reqs, return_launches=True)    # returns: the table is locked once
  assert_same(torch, got, reqs)
  assert launches == 3
  assert not torch.equal(got[1], single((t, i300, s300, None, COMB["sum"], 300, d1)))   # the default row is the descriptor's own
  t._table.check_errors()


# ---- 4. 26 tables -----------------------------------------------------------------------------------------------------------------
def _small_tables(torch, de, tag, dims, vdtype="float32"):
  dt = getattr(torch, vdtype)
  keys = torch.arange(0, 3000, 2, device="cuda")
  out = []
  for j, dim in enumerate(dims):
    t = de.CuckooHashTable(torch.int64, dt, torch.full((dim,), 0.125 * (j + 1), dtype=dt), name="pm_%s_%d" % (tag, j), dim=dim)
    g = torch.Generator(device="cuda").manual_seed(100 + j)
    t.insert(keys, torch.randn((keys.numel(), dim), generator=g, device="cuda").to(dt))
    out.append(t)
  return out


def _small_reqs(torch, tables, seed, n_rows=64):
  rng = np.random.default_rng(seed)
  reqs = []
  for j, t in enumerate(tables):
    n = n_rows + j % 3                                                   # 64, 65, 66 rows: the block edge at 16 rows per block
    counts = rng.integers(0, 17, size=n)
    counts[[0, n - 1]] = 0
    seg = np.repeat(np.arange(n), counts).astype(np.int64)
    ids = (rng.zipf(1.3, size=seg.size) % 3000).astype(np.int64)
    w = rng.standard_normal(seg.size).astype(np.float32) if j % 2 else None
    reqs.append((t, T(torch, ids), T(torch, seg), None if w is None else T(torch, w), j % 3, n))
  return reqs


def test_26_tables_in_three_launches(env):
  torch, de = env
  tables = _small_tables(torch, de, "t26", [(16, 32, 64, 128)[j % 4] for j in range(26)])
  reqs = _small_reqs(torch, tables, 26)
  assert 400 <= np.mean([r[1].numel() for r in reqs]) <= 600
  got, launches = many(de, reqs, return_launches=True)
  assert_same(torch, got, reqs)
  assert launches == 1 + 2                                               # bounds, NCH 1 (dims 16 / 32 / 64), NCH 2 (dim 128)
  half = _small_tables(torch, de, "t26h", [64], "float16")
  reqs2 = reqs + _small_reqs(torch, half, 27)
  got, launches = many(de, reqs2, return_launches=True)
  assert_same(torch, got, reqs2)
  assert launches == 4
  for r in reqs2:
    r[0]._table.check_errors()


# ---- 5. back to back --------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_and_a_table_that_grew(env):
  torch, de = env
  tables = _small_tables(torch, de, "b2b", [64, 16, 128, 32, 64, 256])
  r = _small_reqs(torch, tables, 5) + _small_reqs(torch, tables, 6, n_rows=130)
  lists = [r[0:4], [r[11], r[2], r[7], r[5], r[9], r[1], r[4]], [r[10], r[3]]]
  exp = [[single(q) for q in l] for l in lists]
  torch.cuda.synchronize()
  got = [many(de, l) for l in lists]          # three calls enqueued with nothing waited for in between
  torch.cuda.synchronize()
  for g, e in zip(got, exp):
    assert len(g) == len(e)
    for x, y in zip(g, e):
      assert torch.equal(bits(torch, x), bits(torch, y))
  # a growing table doubles: the next call must read it where it is now
  t = tables[0]
  cap0 = t._table.capacity()
  extra = torch.arange(10_000_000, 10_000_000 + 2 * cap0, device="cuda")
  t.insert(extra, torch.ones((extra.numel(), 64), device="cuda"))
  assert t._table.capacity() > cap0
  ids = torch.cat([r[0][1], extra[:50]])
  seg = torch.cat([r[0][2], torch.full((50,), r[0][5] - 1, dtype=torch.int64, device="cuda")])
  reqs = [(t, ids, seg, None, COMB["mean"], r[0][5]), r[1]]
  got4 = many(de, reqs)
  assert_same(torch, got4, reqs)
  assert got4[0][r[0][5] - 1].any()           # the new keys are found
  for t in tables:
    t._table.check_errors()


# ---- 6. all or nothing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["dim6", "int8", "misaligned_out", "null_table", "struct_size", "combiner3"])
def test_one_bad_descriptor_and_nothing_is_written(env, bad):
  torch, de = env
  from tfra_amd import _capi
  good = [H.table(torch, de, "cuckoo", "float32", 64), H.table(torch, de, "cuckoo", "float32", 128),
          H.table(torch, de, "cuckoo", "float32", 64), H.table(torch, de, "cuckoo", "float16", 64)]
  third = good[2]
  if bad in ("dim6", "int8"):
    dim, dt = (6, torch.float32) if bad == "dim6" else (8, torch.int8)
    third = de.CuckooHashTable(torch.int64, dt, torch.zeros(dim, dtype=dt), name="pm_bad_" + bad, dim=dim)
  tabs = [good[0], good[1], third, good[3]]
  ids_t = torch.arange(8, device="cuda")
  seg_t = torch.arange(8, device="cuda") // 2
  outs = [torch.full((4, t._table.dim + 4), 7.0, device="cuda") for t in tabs]
  descs = (_capi.FindCombineDesc * 4)()
  for e, t, o in zip(descs, tabs, outs):
    _desc(e, t, ids_t, seg_t, 4, o)
  want = UNSUPPORTED
  if bad == "misaligned_out":
    descs[2].out = outs[2].data_ptr() + 4
  elif bad == "null_table":
    descs[2].table, want = None, INVALID
  elif bad == "struct_size":
    descs[2].struct_size, want = ctypes.sizeof(_capi.FindCombineDesc) - 8, INVALID
  elif bad == "combiner3":
    descs[2].combiner, want = 3, INVALID
  launches = ctypes.c_uint32(99)
  rc, msg = _raw(torch, descs, launches=launches)
  assert rc == want
  assert "descriptor 2" in msg
  assert launches.value == 0
  torch.cuda.synchronize()
  for o in outs:
    assert bool((o == 7.0).all())
  # the same code as the single call's, where the single call can be made
  if bad in ("dim6", "int8", "combiner3"):
    comb = 3 if bad == "combiner3" else 0
    assert H._raw_find_combine(torch, de, third, 8, ids_t, seg_t, 4, outs[2], combiner=comb) == want


def test_empty_lists_are_ok(env):
  torch, de = env
  from tfra_amd import _capi
  assert _raw(torch, None, n=0)[0] == 0
  assert _raw(torch, None, n=2)[0] == INVALID                              # null descs with n_tables > 0
  t = H.table(torch, de, "cuckoo", "float32", 64)
  ids_t = torch.arange(8, device="cuda")
  seg_t = torch.arange(8, device="cuda") // 2
  out = torch.full((4, 64), 7.0, device="cuda")
  descs = (_capi.FindCombineDesc * 3)()
  for e in descs:
    _desc(e, t, ids_t, seg_t, 0, out)
  launches = ctypes.c_uint32(99)
  assert _raw(torch, descs, launches=launches)[0] == 0 and launches.value == 0
  torch.cuda.synchronize()
  assert bool((out == 7.0).all())
  assert many(de, []) == []


# ---- 7. the public functions ------------------------------------------------------------------------------------------------------
def _five_vars(torch, de, tag):
  return [H.filled_var(torch, de, "pmv_a_" + tag, dim=64, initializer=0.5),
          H.filled_var(torch, de, "pmv_b_" + tag, dim=128, value_dtype=torch.bfloat16, initializer=0.25),
          H.filled_var(torch, de, "pmv_c_" + tag, dim=32, key_dtype=torch.int32, initializer=0.5),
          H.filled_var(torch, de, "pmv_d_" + tag, dim=6, initializer=0.5),                                # ineligible: dim % 4
          H.filled_var(torch, de, "pmv_e_" + tag, dim=8, initializer=lambda shape: torch.full(tuple(shape), 0.5))]   # callable


def _five_cases(torch, vs, seed):
  rng = np.random.default_rng(seed)
  sp, ws, ns = [], [], []
  for j, v in enumerate(vs):
    n = 200 + 7 * j
    seg, ids, w = H.sparse_case(rng, n, weighted=j != 1)
    ids_t = T(torch, ids.astype(np.int32) if v.key_dtype == torch.int32 else ids)
    sp.append((T(torch, seg), ids_t))
    ws.append(None if w is None else T(torch, w))
    ns.append(n)
  return sp, ws, ns


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_embedding_lookup_sparse_many_equals_the_single_form(env, monkeypatch, combiner):
  torch, de = env
  vs = _five_vars(torch, de, combiner)
  sp, ws, ns = _five_cases(torch, vs, COMB[combiner])
  exp = [de.embedding_lookup_sparse(v, s, w, combiner=combiner, num_rows=n) for v, s, w, n in zip(vs, sp, ws, ns)]
  calls = H.Calls(monkeypatch)
  got = de.embedding_lookup_sparse_many(vs, sp, ws, combiner=combiner, num_rows=ns)
  assert calls["tfra_multi_find_combine"] == 1 and calls["tfra_table_find_combine"] == 0
  assert calls["tfra_unique"] == 2 and calls["tfra_sparse_segment_combine"] == 2      # the two ineligible ones: today's chain
  monkeypatch.undo()
  assert len(got) == 5
  for g, e in zip(got, exp):
    assert torch.equal(bits(torch, g), bits(torch, e))
  # per-table combiners, row counts from the ids (one host read for the grouped three)
  combs = ["sum", "mean", "sqrtn", "mean", "sum"]
  got = de.embedding_lookup_sparse_many(vs, sp, ws, combiner=combs)
  for v, s, w, c, g in zip(vs, sp, ws, combs, got):
    assert torch.equal(bits(torch, g), bits(torch, de.embedding_lookup_sparse(v, s, w, combiner=c)))


@pytest.mark.parametrize("default_id", [None, 4, 5])     # 4 resident, 5 a miss
def test_safe_embedding_lookup_sparse_many_rank2_and_rank3(env, monkeypatch, default_id):
  torch, de = env
  vs = _five_vars(torch, de, "s%s" % default_id)[:4]
  rng = np.random.default_rng(40)
  n_rows = 200
  sp2, sp3, ws = [], [], []
  for v in vs:
    seg, ids, w = H.sparse_case(rng, n_rows)
    ids_t = T(torch, ids.astype(np.int32) if v.key_dtype == torch.int32 else ids)
    col = np.concatenate([np.arange(c) for c in np.bincount(seg, minlength=n_rows)]).astype(np.int64)
    sp2.append((T(torch, seg), ids_t, [n_rows, 9]))
    sp3.append((T(torch, np.stack([seg // 20, seg % 20, col], 1)), ids_t, [10, 20, 9]))
    ws.append(T(torch, w))
  for sp in (sp2, sp3):
    exp = [de.safe_embedding_lookup_sparse(v, s, w, combiner="mean", default_id=default_id) for v, s, w in zip(vs, sp, ws)]
    calls = H.Calls(monkeypatch)
    got = de.safe_embedding_lookup_sparse_many(vs, sp, ws, combiner="mean", default_id=default_id)
    assert calls["tfra_multi_find_combine"] == 1 and calls["tfra_table_find_combine"] == 0
    monkeypatch.undo()
    for g, e in zip(got, exp):
      assert tuple(g.shape) == tuple(e.shape)
      assert torch.equal(bits(torch, g), bits(torch, e))
  assert tuple(got[0].shape) == (10, 20, 64)
  # row counts from the ids when nothing gives them
  sp = [(s[0], s[1]) for s in sp2]
  got = de.safe_embedding_lookup_sparse_many(vs, sp, ws, combiner="sqrtn", default_id=default_id)
  for v, s, w, g in zip(vs, sp, ws, got):
    assert torch.equal(bits(torch, g), bits(torch, de.safe_embedding_lookup_sparse(v, s, w, combiner="sqrtn", default_id=default_id)))


# ---- 8. training through it -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_training_through_the_grouped_lookup_matches_the_single_form(env, monkeypatch, name):
  torch, de = env
  rng = np.random.default_rng(31)
  dims, n_rows = [64, 32, 128], 512
  mk = {"sgd": lambda: de.optimizers.SGD(0.1), "adam": lambda: de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)}[name]
  opt = mk()
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  va = [de.Variable(dim=d, name="pmt_a_%s_%d" % (name, d), initializer=0.5, **kw) for d in dims]
  vb = [de.Variable(dim=d, name="pmt_b_%s_%d" % (name, d), initializer=0.5, **kw) for d in dims]
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  sp, ws, Gs = [], [], []
  for d in dims:
    seg = np.repeat(np.arange(n_rows, dtype=np.int64), 8)
    ids = (rng.zipf(1.2, size=seg.size) % 100000).astype(np.int64)
    w = rng.uniform(0.0, 2.0, size=seg.size).astype(np.float32)
    w[seg == 3] = 0.0
    sp.append((T(torch, seg), T(torch, ids)))
    ws.append(T(torch, w))
    Gs.append(T(torch, (rng.standard_normal((n_rows, d)) * 0.01).astype(np.float32)))
  for step in range(2):
    calls = H.Calls(monkeypatch)
    res = de.embedding_lookup_sparse_many(va, sp, ws, combiner="mean", return_trainable=True, num_rows=n_rows)
    for (out, tw), G in zip(res, Gs):
      assert isinstance(tw, de.SparseTrainableWrapper)
      da.apply_combined_gradients([(G, tw)])
    assert calls["tfra_multi_find_combine"] == 1 and calls["tfra_table_find_combine"] == 0 and calls["tfra_unique"] == 0
    monkeypatch.undo()
    for j in range(len(dims)):
      out_b, twb = de.embedding_lookup_sparse(vb[j], sp[j], ws[j], combiner="mean", return_trainable=True, num_rows=n_rows)
      db.apply_combined_gradients([(Gs[j], twb)])
      assert torch.equal(bits(torch, res[j][0]), bits(torch, out_b))
      sa, sb = H._export_state(torch, de, da, opt, va[j]), H._export_state(torch, de, db, opt, vb[j])
      assert len(sa) == len(sb) == 2 + len(opt.slots)
      for x, y in zip(sa, sb):
        assert torch.equal(x, y)
