"""GPU: the grouped plan build (tfra_multi_sparse_plan_build; table_ops.build_plans_many; the plans of
embedding_lookup_sparse_many(plan_writeback=True) and of apply_combined_gradients_many).

A grouped build runs the single build's device functions (csr_tile_body / csr_bucket_body / csr_scatter_body, csrc/tfra_csr.hip)
with the block's index inside its plan, so plan d must hold the CSR a single build holds.  WHERE a key's records land inside the
plan's buffers differs from run to run (atomic cursors), so plans are compared on `canon`: the content of tfra_sparse_plan_read per
key — keys, counts, each key's positions ascending, the hot / cold split, no build errors — against a twin plan built by
SparsePlan.build over the same ids and against numpy; tables written back through the plans are compared bit for bit.  No tolerance."""
import ctypes

import numpy as np
import pytest

from tests import sparse_helpers as H
from tests.sparse_helpers import Calls, T

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6

@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops
  return torch, de, table_ops


def dev_of(torch):
  return "cuda:%d" % torch.cuda.current_device()


def zipf(rng, n):
  return (rng.zipf(1.2, size=n) % 1_000_003).astype(np.int64) * 7919 - 5


def _in_key_order(keys, cnt, pos):
  """(keys ascending, their counts, the positions lists concatenated in that key order)"""
  cnt = cnt.astype(np.int64)
  order = np.argsort(keys, kind="stable")
  off = np.concatenate([[0], np.cumsum(cnt)])
  c = cnt[order]
  start = np.concatenate([[0], np.cumsum(c)])[:-1]
  idx = np.repeat(off[order], c) + (np.arange(int(c.sum())) - np.repeat(start, c))
  return keys[order], c, pos.astype(np.int64)[idx]


def canon(plan):
  """plan.read() per key, in key order: (keys, counts, positions), the number of hot keys and of cold keys; the build reported no
  error and the hot keys (more than 8 occurrences) come first."""
  counts, keys, cnt, pos = plan.read()
  assert counts["errors"] == 0, counts
  many, few = counts["many"], counts["few"]
  assert many + few == keys.size
  assert np.all(cnt[:many] > 8) and np.all(cnt[many:] <= 8)
  return _in_key_order(keys, cnt, pos) + (many, few)


def canon_np(ids):
  uk, uc = np.unique(ids, return_counts=True)
  pos = np.argsort(ids, kind="stable")   # grouped by key ascending, each key's positions ascending
  many = int((uc > 8).sum())
  return uk, uc.astype(np.int64), pos.astype(np.int64), many, uk.size - many


def same(a, b):
  return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def plans_for(torch, table_ops, dims):
  return [table_ops.SparsePlan(dev_of(torch), d) for d in dims]


def check_against_twins_and_numpy(torch, table_ops, ids_list, dims, numpy_too=True):
  plans, twins = plans_for(torch, table_ops, dims), plans_for(torch, table_ops, dims)
  dev_ids = [T(torch, a) for a in ids_list]
  _, launches = table_ops.build_plans_many(plans, dev_ids, return_launches=True)
  for tw, t in zip(twins, dev_ids):
    tw.build(t)
  for i, (pl, tw, a) in enumerate(zip(plans, twins, ids_list)):
    c = canon(pl)
    assert same(c, canon(tw)), ("twin", i, a.size)
    if numpy_too:
      assert same(c, canon_np(a)), ("numpy", i, a.size)
  return launches


def hot_bucket_ids(rng, n):
  """Hot keys that all hash into ONE merge bucket and occur in every tile: the bucket holds more descriptors than one pass takes
  (100 keys x 79 tiles > 512) and is merged in several hash-split passes from the region and the overflow list (the generator of
  tests/test_gpu_frontend.py, restated)."""
  from bench import fmix64_np
  P = 64
  while P < 2048 and P * 128 < n:
    P *= 2
  cand = rng.integers(1, 2**62, size=200000).astype(np.int64)
  h = fmix64_np(cand.astype(np.uint64))
  bucket = ((h >> np.uint64(32)).astype(np.uint64) * np.uint64(P)) >> np.uint64(32)
  hot = cand[bucket == 7][:100]
  assert hot.size == 100
  ids = np.concatenate([np.tile(hot, n // 100), hot[: n % 100]])
  rng.shuffle(ids)
  return ids


# ---- 1. a mixed list ---------------------------------------------------------------------------------------------------------------
def test_mixed_list_equals_the_single_builds(env):
  torch, de, table_ops = env
  rng = np.random.default_rng(1)
  ids = [zipf(rng, n) for n in (1, 511, 512, 513, 8192, 8193)]       # 8192: 64 merge buckets, 8193: 128
  ids.append(zipf(rng, 40000))
  ids.append(np.full(5000, -77, np.int64))                          # one key: 9 full 512-entry bins + a remainder
  edge = np.concatenate([np.repeat(np.arange(100, 160, dtype=np.int64), 8), np.repeat(np.arange(200, 260, dtype=np.int64), 9)])
  rng.shuffle(edge)
  ids.append(edge)                                                  # exactly 8 (cold) and exactly 9 (hot) occurrences
  ids.append(rng.permutation(4096).astype(np.int64) - 2000)          # all distinct
  dims = [(16, 64, 128, 256)[i % 4] for i in range(len(ids))]
  assert check_against_twins_and_numpy(torch, table_ops, ids, dims) == 3
  c = canon_np(edge)
  assert (c[3], c[4]) == (60, 60)


# ---- 2. both pass sizes in one call ------------------------------------------------------------------------------------------------
def test_both_cm_classes_in_one_call(env):
  torch, de, table_ops = env
  rng = np.random.default_rng(2)
  ids = [zipf(rng, 131072), zipf(rng, 700), zipf(rng, 3000), zipf(rng, 131073)]   # 256 tiles (cm 512) ... 257 tiles (cm 1024)
  assert check_against_twins_and_numpy(torch, table_ops, ids, [64, 16, 128, 32]) == 4
  assert check_against_twins_and_numpy(torch, table_ops, ids[:3], [64, 16, 128], numpy_too=False) == 3


# ---- 3. the bucket overflow path inside a list ---------------------------------------------------------------------------------
def test_bucket_overflow_between_two_ordinary_plans(env):
  torch, de, table_ops = env
  rng = np.random.default_rng(77)
  ids = [zipf(rng, 20000), hot_bucket_ids(rng, 40064), zipf(rng, 5000)]
  assert check_against_twins_and_numpy(torch, table_ops, ids, [64, 8, 32]) == 3


# ---- 4. neighbours ------------------------------------------------------------------------------------------------------------------
def test_neighbours_do_not_touch_each_other(env):
  torch, de, table_ops = env
  rng = np.random.default_rng(4)
  sizes = (513, 1, 1023)
  rounds = [[rng.integers(-50, 50, size=n).astype(np.int64) * (r + 1) for n in sizes] for r in range(5)]
  dev = [[T(torch, a) for a in r] for r in rounds]
  plans = plans_for(torch, table_ops, [64, 64, 64])
  torch.cuda.synchronize()
  for r in range(5):
    table_ops.build_plans_many(plans, dev[r])
  for pl, a in zip(plans, rounds[-1]):
    assert same(canon(pl), canon_np(a)), a.size


# ---- 5. rebuilds with another layout -------------------------------------------------------------------------------------------
def test_rebuild_with_another_layout_and_mixed_with_single_builds(env):
  torch, de, table_ops = env
  rng = np.random.default_rng(5)
  a, b = plans_for(torch, table_ops, [64, 32])
  other = plans_for(torch, table_ops, [16])[0]
  b.build(T(torch, zipf(rng, 3000)))                                  # b: first built by the single call
  for n in (8192, 20000, 100):                                       # a: 64 merge buckets, 256 (the memsets run), back to 64
    ia, ib, io = zipf(rng, n), zipf(rng, n // 2 + 1), zipf(rng, 777)
    table_ops.build_plans_many([a, b, other], [T(torch, ia), T(torch, ib), T(torch, io)])
    for pl, ids in ((a, ia), (b, ib), (other, io)):
      assert same(canon(pl), canon_np(ids)), (n, ids.size)
  ia = zipf(rng, 9000)
  a.build(T(torch, ia))                                               # built grouped, rebuilt by the single call
  assert same(canon(a), canon_np(ia))
  ia = zipf(rng, 600)
  table_ops.build_plans_many([a, other], [T(torch, ia), T(torch, ia)])   # ... and grouped again
  assert same(canon(a), canon_np(ia)) and same(canon(other), canon_np(ia))


# ---- 6. the launch count does not grow with the list -------------------------------------------------------------------------------
def test_26_plans_take_3_launches_and_52_the_same_3(env):
  torch, de, table_ops = env
  rng = np.random.default_rng(6)
  ids = [zipf(rng, 8192 * 4) for _ in range(52)]
  dims = [(16, 32, 64, 128)[i % 4] for i in range(52)]
  assert check_against_twins_and_numpy(torch, table_ops, ids[:26], dims[:26], numpy_too=False) == 3
  assert check_against_twins_and_numpy(torch, table_ops, ids, dims, numpy_too=False) == 3


# ---- 7. the plans work -------------------------------------------------------------------------------------------------------------
def test_tables_written_back_through_grouped_plans_equal_the_single_builds(env):
  torch, de, table_ops = env
  adam = H.opt_of(de, "adam")
  shapes = [(32, "float32"), (64, "float32"), (128, "float32"), (64, "float16")]
  cases = [H.Case(torch, de, adam, "pm7_%d" % i, d, vdtype=vd, seed=70 + i) for i, (d, vd) in enumerate(shapes)]

  def twin_request(c, step):
    t = c.table(True)
    return (t._table, c.plan_t, c.G(torch, step), c.seg, c.w, c.comb, t._default_value.to(torch.float32))

  for step, p in ((1, adam.params(1)), (2, H.opt_of(de, "sgd").params(2))):
    table_ops.build_plans_many([c.plan for c in cases], [c.ids for c in cases])   # set a: grouped
    for c in cases:
      c.plan_t.build(c.ids)                                                       # set b: one by one
    H.many([c.request(torch, step, build=False) for c in cases], p)
    H.many([twin_request(c, step) for c in cases], p)
  H.assert_twins(torch, de, adam, cases)
  # one plan of each set consumed by apply_planned on a dense [n, dim] gradient
  c = cases[1]
  table_ops.build_plans_many([cases[0].plan, c.plan], [cases[0].ids, c.ids])
  c.plan_t.build(c.ids)
  g = torch.randn((c.ids.numel(), c.dim), generator=torch.Generator(device="cuda").manual_seed(7), device="cuda") * 0.01
  p = adam.params(3)
  for twin, plan in ((False, c.plan), (True, c.plan_t)):
    t = c.table(twin)
    t._table.apply_planned(p, plan, g, t._default_value.to(torch.float32))
  H.assert_twins(torch, de, adam, cases)


# ---- 8. one bad descriptor and nothing is built ----------------------------------------------------------------------------------
def desc_of(plan, ids, dim=None):
  from tfra_amd import _capi
  e = _capi.PlanBuildDesc()
  e.struct_size = ctypes.sizeof(_capi.PlanBuildDesc)
  e.plan, e.n, e.ids, e.dim = plan._h.value, ids.numel(), ids.data_ptr(), plan._dim if dim is None else dim
  return e


def raw_many(torch, descs, n=None):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _stream
  arr = (_capi.PlanBuildDesc * max(1, len(descs)))(*descs)
  launches = ctypes.c_uint32(77)
  dev = torch.device("cuda", torch.cuda.current_device())
  rc = _capi.lib().tfra_multi_sparse_plan_build(_workspace(dev), len(descs) if n is None else n, ctypes.c_void_p(ctypes.addressof(arr)),
                                                ctypes.c_void_p(ctypes.addressof(launches)), _stream(dev))
  return rc, int(launches.value), _capi.lib().tfra_last_error().decode()


def raw_single(torch, plan_handle, n, ids_ptr, dim):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _stream
  dev = torch.device("cuda", torch.cuda.current_device())
  rc = _capi.lib().tfra_sparse_plan_build(plan_handle, n, ids_ptr, dim, _stream(dev))
  return rc, _capi.lib().tfra_last_error().decode()


BAD = ["null_plan", "null_ids", "dim_6", "dim_260", "dim_0", "too_many_ids", "struct_size", "same_plan_twice"]


@pytest.mark.parametrize("what", BAD)
def test_one_bad_descriptor_and_nothing_is_built(env, what):
  torch, de, table_ops = env
  rng = np.random.default_rng(8)
  plans = plans_for(torch, table_ops, [64, 32, 128])
  prev = [zipf(rng, n) for n in (700, 2000, 513)]
  table_ops.build_plans_many(plans, [T(torch, a) for a in prev])
  new = [T(torch, zipf(rng, n)) for n in (900, 100, 5000)]
  descs = [desc_of(pl, t) for pl, t in zip(plans, new)]
  bad, expect, names, single = descs[1], INVALID, ["descriptor 1"], None
  scratch = plans_for(torch, table_ops, [32])[0]
  keep = []
  if what == "null_plan":
    bad.plan = None
    single = (None, 100, new[1].data_ptr(), 32)
  elif what == "null_ids":
    bad.ids = None
    single = (scratch._h, 100, None, 32)
  elif what in ("dim_6", "dim_260"):
    bad.dim, expect = int(what[4:]), UNSUPPORTED
    single = (scratch._h, 100, new[1].data_ptr(), bad.dim)
  elif what == "dim_0":
    bad.dim, expect = 0, UNSUPPORTED
  elif what == "too_many_ids":
    big = torch.zeros((1 << 18) + 1, dtype=torch.int64, device="cuda")
    keep.append(big)
    bad.n, bad.ids, expect = big.numel(), big.data_ptr(), UNSUPPORTED
    single = (scratch._h, big.numel(), big.data_ptr(), 32)
  elif what == "struct_size":
    bad.struct_size -= 8
  elif what == "same_plan_twice":
    descs[2].plan = descs[0].plan
    names = ["descriptor 0", "descriptor 2"]
  torch.cuda.synchronize()
  rc, launches, msg = raw_many(torch, descs)
  assert rc == expect, (rc, msg)
  assert launches == 0
  assert msg.startswith("multi_sparse_plan_build: ") and all(nm in msg for nm in names), msg
  if single is not None:
    rc1, msg1 = raw_single(torch, *single)
    assert rc1 == expect and msg1.startswith("sparse_plan_build: "), (rc1, msg1)
    assert msg == "multi_sparse_plan_build: descriptor 1: " + msg1[len("sparse_plan_build: "):]
  for pl, a in zip(plans, prev):     # every plan of the list still holds its previous build
    assert same(canon(pl), canon_np(a)), a.size


def test_null_descs_and_null_workspace_are_refused(env):
  torch, de, table_ops = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _stream
  dev = torch.device("cuda", torch.cuda.current_device())
  rc = _capi.lib().tfra_multi_sparse_plan_build(None, 1, None, None, _stream(dev))
  assert rc == INVALID and "null argument" in _capi.lib().tfra_last_error().decode()


# ---- 9. empty lists -----------------------------------------------------------------------------------------------------------------
def test_empty_list_and_list_of_empty_batches(env):
  torch, de, table_ops = env
  assert table_ops.build_plans_many([], [], return_launches=True) == ([], 0)
  rc, launches, _ = raw_many(torch, [])
  assert rc == 0 and launches == 0
  plans = plans_for(torch, table_ops, [64, 16])
  table_ops.build_plans_many(plans, [T(torch, np.arange(600, dtype=np.int64)), T(torch, np.arange(9, dtype=np.int64))])
  empty = torch.empty(0, dtype=torch.int64, device="cuda")
  _, launches = table_ops.build_plans_many(plans, [empty, empty], return_launches=True)
  assert launches == 0
  for pl in plans:
    counts, keys, cnt, pos = pl.read()
    assert pl.n == 0 and keys.size == 0 and not any(counts.values())
  # ... and an empty batch beside a real one takes no blocks
  ids = np.arange(1000, dtype=np.int64) % 37
  _, launches = table_ops.build_plans_many(plans, [empty, T(torch, ids)], return_launches=True)
  assert launches == 3 and plans[0].n == 0 and same(canon(plans[1]), canon_np(ids))


# ---- 10. a build on a side stream next to a grouped lookup on the main stream -------------------------------------------------------
def test_side_stream_build_beside_grouped_lookups(env):
  """Each stream has a workspace of its own (device_ops._workspace is keyed by the current stream): the two grouped calls never
  share a staging ring or scratch."""
  torch, de, table_ops = env
  rng = np.random.default_rng(10)
  sgd = H.opt_of(de, "sgd")
  dims = [64, 32, 128]
  cases = [H.Case(torch, de, sgd, "pm10_%d" % i, d, seed=100 + i) for i, d in enumerate(dims)]
  reqs = []
  for c in cases:
    t = c.table()
    reqs.append((t._table, c.ids, c.seg, c.w, c.comb, c.n_rows, t._default_value))
  quiet = [o.clone() for o in table_ops.find_combine_many(reqs)]
  rounds = [[zipf(rng, n) for n in (9000, 513, 30000)] for _ in range(10)]
  dev = [[T(torch, a) for a in r] for r in rounds]
  plans = plans_for(torch, table_ops, dims)
  side = torch.cuda.Stream()
  torch.cuda.synchronize()
  outs = []
  for r in range(10):
    with torch.cuda.stream(side):
      table_ops.build_plans_many(plans, dev[r])
    outs.append(table_ops.find_combine_many(reqs))
  torch.cuda.synchronize()
  for r in range(10):
    for o, q in zip(outs[r], quiet):
      assert torch.equal(H.bits(torch, o), H.bits(torch, q)), r
  for pl, a in zip(plans, rounds[-1]):
    assert same(canon(pl), canon_np(a)), a.size


# ---- 11. the Python surface ------------------------------------------------------------------------------------------------------
ROWS = 8192   # x 1 id per row = PLAN_AT_LOOKUP_MIN_IDS entries


def sparse_inputs(torch, seed, empty_row=None):
  rng = np.random.default_rng(seed)
  rank = (rng.zipf(1.2, size=ROWS) - 1) % H.UNIVERSE
  seg = np.arange(ROWS, dtype=np.int64)
  if empty_row is not None:
    seg[empty_row] = empty_row - 1   # row `empty_row` has no entry, the row before has two
  w = rng.uniform(0.1, 2.0, size=ROWS).astype(np.float32)
  return (T(torch, seg), T(torch, H.key_of(rank))), T(torch, w)


def variables(torch, de, opt, tag):
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  dev = dev_of(torch)
  vs = [H.make_var(torch, de, opt, "pm11%s_%d" % (tag, i), d) for i, d in enumerate((64, 32, 128))]
  return vs + [de.Variable(dim=32, name="pm11%s_s" % tag, initializer=0.5, devices=[dev, dev], **kw)]


def pools_are_full(vs):
  return all(len(v._plan_pool["free"]) == v._plan_pool["made"] for v in vs if getattr(v, "_plan_pool", None) is not None)


@pytest.mark.parametrize("safe", [False, True])
def test_python_surface_one_grouped_build_per_step(env, monkeypatch, safe):
  torch, de, table_ops = env
  from tfra_amd.dynamic_embedding import variable as V
  assert ROWS >= V.PLAN_AT_LOOKUP_MIN_IDS
  opt = H.opt_of(de, "adam")
  tag = "s" if safe else "p"
  va, vb = variables(torch, de, opt, tag + "a"), variables(torch, de, opt, tag + "b")
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  sps, ws = zip(*[sparse_inputs(torch, 110 + i, empty_row=(77 if safe else None)) for i in range(4)])
  sps, ws = list(sps), list(ws)

  def lookups(vs, plan_writeback):
    if safe:
      res = de.safe_embedding_lookup_sparse_many(vs, sps, ws, combiner="mean", default_id=int(H.key_of(np.array([3]))[0]),
                                                 return_trainable=True, num_rows=ROWS, plan_writeback=plan_writeback)
    else:
      res = de.embedding_lookup_sparse_many(vs, sps, ws, combiner="mean", return_trainable=True, num_rows=ROWS,
                                            plan_writeback=plan_writeback)
    return [tw for _, tw in res]

  for step, plan_writeback in ((1, True), (2, False)):
    Gs = [H.grad(torch, 110 + i, ROWS, v.dim, step) for i, v in enumerate(va)]
    db.apply_combined_gradients(list(zip(Gs, lookups(vb, False))))
    calls = Calls(monkeypatch)
    tws = lookups(va, plan_writeback)
    if plan_writeback:   # the three eligible members' plans: one grouped build at lookup time
      assert calls["tfra_multi_sparse_plan_build"] == 1 and calls["tfra_sparse_plan_build"] == 0
      assert all(tw.entry_plan is not None for tw in tws[:3]) and tws[3].entry_plan is None
    else:
      assert calls["tfra_multi_sparse_plan_build"] == 0 and calls["tfra_sparse_plan_build"] == 0
      assert all(tw.entry_plan is None for tw in tws)
    da.apply_combined_gradients_many(list(zip(Gs, tws)))
    assert calls["tfra_multi_sparse_plan_build"] == 1 and calls["tfra_sparse_plan_build"] == 0
    assert calls["tfra_multi_apply_planned_combined"] == 1 and calls["tfra_table_apply_planned_combined"] == 0
    monkeypatch.undo()
    del tws
    assert pools_are_full(va[:3])
  assert da.iterations == db.iterations == 2
  for a, b in zip(va, vb):
    for x, y in zip(H._export_state(torch, de, da, opt, a), H._export_state(torch, de, db, opt, b)):
      assert torch.equal(x, y)


def test_a_group_of_one_keeps_the_single_build(env, monkeypatch):
  torch, de, table_ops = env
  opt = H.opt_of(de, "sgd")
  v = H.make_var(torch, de, opt, "pm12", 64)
  deo = de.DynamicEmbeddingOptimizer(opt)
  sp, w = sparse_inputs(torch, 120)
  for plan_writeback in (True, False):
    calls = Calls(monkeypatch)
    (_, tw), = de.embedding_lookup_sparse_many([v], [sp], [w], combiner="sum", return_trainable=True, num_rows=ROWS,
                                               plan_writeback=plan_writeback)
    assert (tw.entry_plan is not None) == plan_writeback
    deo.apply_combined_gradients_many([(H.grad(torch, 120, ROWS, 64), tw)])
    assert calls["tfra_sparse_plan_build"] == 1 and calls["tfra_multi_sparse_plan_build"] == 0
    monkeypatch.undo()
