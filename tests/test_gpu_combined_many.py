"""GPU: the grouped combined write-back (tfra_multi_apply_planned_combined; table_ops.apply_planned_combined_many;
DynamicEmbeddingOptimizer.apply_combined_gradients_many).

The reference of every case is a TWIN table driven through the single call (tfra_table_apply_planned_combined) on the same inputs.
Both forms run the same device functions (hot_sums_body / apply_csr_body, csrc/tfra_apply_device.h; comb_den_row / comb_ent_one,
csrc/tfra_combine_device.h), so they must agree BIT FOR BIT: every comparison is torch.equal on the bit patterns of the key-sorted
exported rows and of every slot, after two steps (the second one updates rows the first one wrote).  No tolerance."""

import numpy as np
import pytest

from tests.sparse_helpers import (COMB, N_ROWS, Calls, Case, T, _export_state, assert_twins, desc_of, grad, key_of, make_var, many,
                                  opt_of, raw_many, writeback_batch as batch)

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def two_steps(torch, de, opt, cases, expect_launches=None):
  for step in (1, 2):
    p = opt.params(step)
    launches = many([c.request(torch, step) for c in cases], p)
    if expect_launches is not None:
      assert launches == expect_launches, "launches %d, the header's formula gives %d" % (launches, expect_launches)
    for c in cases:
      c.single(torch, p, step)
  assert_twins(torch, de, opt, cases)


# ---- 1. a mixed list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sgd", "adam", "adagrad", "ftrl"])
def test_mixed_list_equals_the_single_calls_bitwise(env, rule):
  torch, de = env
  opt = opt_of(de, rule)
  n = "cm1_" + rule
  cases = [
      Case(torch, de, opt, n + "a", 16, comb="sum", seed=1),
      Case(torch, de, opt, n + "b", 64, comb="mean", weighted=False, seed=2),
      Case(torch, de, opt, n + "c", 128, comb="sqrtn", seed=3),
      Case(torch, de, opt, n + "d", 192, comb="mean", seed=4),             # hot_sums NCH 3
      Case(torch, de, opt, n + "e", 256, comb="sum", weighted=False, seed=5),
      Case(torch, de, opt, n + "f", 64, "float16", comb="sqrtn", seed=6),
      Case(torch, de, opt, n + "g", 128, "bfloat16", comb="mean", seed=7),
  ]
  # 3 (bounds, denominators, entry records) + NCH 1, 2, 3, 4 + one rule x (float32, float16, bfloat16); no table at max_capacity
  two_steps(torch, de, opt, cases, expect_launches=3 + 4 + 3)
  k, v = cases[0].var.export()
  assert k.numel() > 400 and bool(torch.isfinite(v).all())           # keys entered from the default row


# ---- 2. neighbours of one class ---------------------------------------------------------------------------------------------------
def test_adjacent_descriptors_of_one_class_do_not_touch_each_other(env):
  """Plans of 1, 17 and 257 distinct keys (block-boundary cases of the 16-lane-group mapping: 16 keys per 256-thread block) and a
  descriptor with an empty plan between them."""
  torch, de = env
  opt = opt_of(de, "adam")
  rng = np.random.default_rng(5)
  cases = []
  for j, nkeys in enumerate([1, 17, 0, 257]):
    n_rows = max(1, (nkeys * 2 + 3) // 4)
    rank = np.concatenate([np.arange(nkeys), np.arange(nkeys)])            # every key twice
    rng.shuffle(rank)
    seg = np.sort(rng.integers(0, n_rows, size=rank.size)).astype(np.int64)
    if nkeys:
      seg[-1] = n_rows - 1
    w = rng.uniform(0.5, 1.5, size=rank.size).astype(np.float32)
    inputs = (T(torch, key_of(rank + 100 * j)), T(torch, seg), T(torch, w))
    cases.append(Case(torch, de, opt, "cm2_%d" % j, 64, comb=["sum", "mean", "sqrtn", "mean"][j], seed=20 + j, inputs=inputs,
                      n_rows=n_rows))
  two_steps(torch, de, opt, cases, expect_launches=3 + 1 + 1)
  before = _export_state(torch, de, de.DynamicEmbeddingOptimizer(opt), opt, make_var(torch, de, opt, "cm2_ref", 64))
  after = _export_state(torch, de, de.DynamicEmbeddingOptimizer(opt), opt, cases[2].var)
  for x, y in zip(before, after):
    assert torch.equal(x, y)                                              # the empty plan's table is as it was filled


# ---- 3. the launch count does not grow with the list -------------------------------------------------------------------------
@pytest.mark.parametrize("n_tables", [26, 52])
def test_26_tables_6_launches_52_tables_the_same_6(env, n_tables):
  torch, de = env
  opt = opt_of(de, "adam")
  cases = []
  for i in range(n_tables):
    inputs = batch(torch, 300 + i, n_rows=64, per_row=4, planted=0)
    cases.append(Case(torch, de, opt, "cm3_%d_%d" % (n_tables, i), [16, 32, 64, 128][i % 4], comb="mean", seed=300 + i, inputs=inputs,
                      n_rows=64))
  two_steps(torch, de, opt, cases, expect_launches=3 + 2 + 1)


# ---- 4. one bad descriptor and nothing is written --------------------------------------------------------------------------------
BAD = ["int8_table", "misaligned_grad_out", "null_plan", "struct_size", "combiner_3", "plan_of_another_dim", "adam_without_slots",
       "same_table_twice", "same_plan_twice"]


@pytest.mark.parametrize("what", BAD)
def test_one_bad_descriptor_and_nothing_is_written(env, what):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  opt = opt_of(de, "adam")
  p = opt.params(1)
  cases = [Case(torch, de, opt, "cm4_%s_%d" % (what, i), 64, seed=40 + i) for i in range(3)]
  reqs = [c.request(torch, 1) for c in cases]
  keep = []
  descs = [desc_of(torch, r, p) for r in reqs]
  bad, expect, names = descs[2], INVALID, ["descriptor 2"]
  if what == "int8_table":
    t8 = de.CuckooHashTable(torch.int64, torch.int8, torch.zeros(64, dtype=torch.int8), name="cm4_i8", dim=64, aux_fields=2)
    keep.append(t8)
    bad.table, expect = t8._table._h.value, UNSUPPORTED
  elif what == "misaligned_grad_out":
    G = torch.zeros(N_ROWS * 64 + 4, device="cuda")[1:1 + N_ROWS * 64].view(N_ROWS, 64)
    keep.append(G)
    bad.grad_out, expect = G.data_ptr(), UNSUPPORTED
    assert G.data_ptr() % 16 == 4
  elif what == "null_plan":
    bad.plan = None
  elif what == "struct_size":
    bad.struct_size -= 8
  elif what == "combiner_3":
    bad.combiner = 3
  elif what == "plan_of_another_dim":
    pl = SparsePlan(cases[2].var._primary, 32).build(cases[2].ids)
    keep.append(pl)
    bad.plan = pl._h.value
  elif what == "adam_without_slots":
    bare = make_var(torch, de, opt_of(de, "sgd"), "cm4_bare", 64)
    keep.append(bare)
    bad.table = bare._tables[0]._table._h.value
  elif what == "same_table_twice":
    pl = SparsePlan(cases[2].var._primary, 64).build(cases[2].ids)
    keep.append(pl)
    bad.table, bad.plan, names = descs[0].table, pl._h.value, ["descriptor 0", "descriptor 2"]
  elif what == "same_plan_twice":
    bad.plan, names = descs[1].plan, ["descriptor 1", "descriptor 2"]
  deo = de.DynamicEmbeddingOptimizer(opt)
  before = [_export_state(torch, de, deo, opt, c.var) for c in cases]
  torch.cuda.synchronize()
  rc, launches, msg = raw_many(torch, descs)
  assert rc == expect, (rc, msg)
  assert launches == 0
  for nm in names:
    assert nm in msg, msg
  torch.cuda.synchronize()
  for c, b in zip(cases, before):
    for x, y in zip(b, _export_state(torch, de, deo, opt, c.var)):
      assert torch.equal(x, y)
  # the same list without the bad descriptor goes through
  assert raw_many(torch, descs[:2])[:2] == (0, 3 + 1 + 1)
  assert raw_many(torch, [])[:2] == (0, 0)


# ---- 5. empty lists ---------------------------------------------------------------------------------------------------------------
def test_empty_lists_are_ok(env):
  torch, de = env
  opt = opt_of(de, "sgd")
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  assert many([], opt.params(1)) == 0
  assert raw_many(torch, [])[:2] == (0, 0)
  cases = [Case(torch, de, opt, "cm5_%d" % i, 64, seed=50, inputs=(none, none, torch.empty(0, device="cuda")), n_rows=1)
           for i in range(2)]
  deo = de.DynamicEmbeddingOptimizer(opt)
  before = [_export_state(torch, de, deo, opt, c.var) for c in cases]
  assert many([c.request(torch, 1) for c in cases], opt.params(1)) == 0
  for c, b in zip(cases, before):
    for x, y in zip(b, _export_state(torch, de, deo, opt, c.var)):
      assert torch.equal(x, y)


# ---- 6. a table that grows inside the call ----------------------------------------------------------------------------------------
def test_a_table_that_grows_inside_the_call(env):
  torch, de = env
  opt = opt_of(de, "adam")
  rng = np.random.default_rng(6)
  nnz = 4096
  rank = rng.permutation(np.arange(600, 600 + nnz))                        # never-seen keys, all distinct
  seg = np.repeat(np.arange(nnz // 8, dtype=np.int64), 8)
  inputs = (T(torch, key_of(rank)), T(torch, seg), T(torch, rng.uniform(0.5, 1.5, size=nnz).astype(np.float32)))
  cases = [Case(torch, de, opt, "cm6_a", 64, seed=61),
           Case(torch, de, opt, "cm6_g", 64, seed=62, inputs=inputs, n_rows=nnz // 8, init_size=1024),
           Case(torch, de, opt, "cm6_b", 32, seed=63)]
  cap0 = cases[1].table()._table.capacity()
  two_steps(torch, de, opt, cases, expect_launches=3 + 1 + 1)
  assert cases[1].table()._table.capacity() > cap0, "the batch did not carry the table over its load factor"
  assert int(cases[1].var.size()) >= nnz


# ---- 7. a full bounded table in the list ---------------------------------------------------------------------------------------------
def test_a_full_bounded_table_in_the_list(env):
  """What tests/test_gpu_hkv.py::test_fused_optimizer_evicts_on_full_bounded_table holds for the single call, for a bounded table
  inside a grouped call: the size stays within max_capacity (var.size() raises if a key could neither be placed nor evict), every
  key of the step is resident after its write-back and holds the value of the reference sequence, nothing is duplicated.  Victim
  choice is not pinned between runs, so the bounded table has no twin; the model of its values is an unbounded table seeded with
  what the bounded one held."""
  torch, de = env
  opt = opt_of(de, "sgd")
  dim = 64
  grow = [Case(torch, de, opt, "cm7_a", 64, seed=71), Case(torch, de, opt, "cm7_b", 64, seed=72)]
  hkv = de.get_variable("cm7_hkv", key_dtype=torch.int64, value_dtype=torch.float32, initializer=0.25, dim=dim, init_size=1024,
                        kv_creator=de.HkvHashTableCreator(config=de.HkvHashTableConfig(
                            init_capacity=1024, max_capacity=1024, max_hbm_for_values=1 << 20,
                            evict_strategy=de.HkvEvictStrategy.LRU)))
  for lo in range(0, 3000, 500):   # fill beyond capacity: the table is now as full as it gets
    k = np.arange(lo, lo + 500, dtype=np.int64)
    hkv.upsert(T(torch, k), T(torch, np.tile(k[:, None] * 1e-3, (1, dim)).astype(np.float32)))
  assert 900 < int(hkv.size()) <= 1024
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  rng = np.random.default_rng(7)
  plan, plan_m = SparsePlan(hkv._primary, dim), SparsePlan(hkv._primary, dim)
  fresh_base = 10**6
  for step in (1, 2):
    p = opt.params(step)
    rk, rv = hkv.export()
    model = de.Variable(dim=dim, name="cm7_model_%d" % step, initializer=0.25)
    model.upsert(rk, rv)
    resident = rng.choice(rk.cpu().numpy(), size=100, replace=False)
    fresh = np.arange(fresh_base, fresh_base + 150, dtype=np.int64)
    fresh_base += 150
    ids = np.concatenate([resident, resident[:40], fresh, fresh[:30]])
    rng.shuffle(ids)
    ids_t = T(torch, ids)
    seg = T(torch, np.repeat(np.arange(ids.size // 4, dtype=np.int64), 4))
    G = grad(torch, 70, ids.size // 4, dim, step)
    t = hkv._tables[0]
    reqs = [grow[0].request(torch, step), (t._table, plan.build(ids_t), G, seg, None, COMB["sum"], t._default_value.to(torch.float32)),
            grow[1].request(torch, step)]
    launches = many(reqs, p)
    assert launches == 3 + 1 + 1 + 1                                        # ... + the eviction-phase launch of the class
    for c in grow:
      c.single(torch, p, step)
    m = model._tables[0]
    m._table.apply_planned_combined(p, plan_m.build(ids_t), G, seg, None, COMB["sum"], m._default_value.to(torch.float32))
    assert int(hkv.size()) <= 1024
    uniq = T(torch, np.unique(ids))
    got, ex = hkv.lookup(uniq, return_exists=True)
    assert bool(ex.all()), "step %d: keys of the step not resident after its write-back" % step
    np.testing.assert_allclose(got.cpu().numpy(), model.lookup(uniq).cpu().numpy(), rtol=2e-6, atol=2e-6)
  k = hkv.export()[0].cpu().numpy()
  assert len(np.unique(k)) == len(k) == int(hkv.size())
  assert_twins(torch, de, opt, grow)


# ---- 8. back-to-back calls ---------------------------------------------------------------------------------------------------------
def test_ten_calls_back_to_back_without_synchronisation(env):
  """More calls in flight than the staging ring has slots (8)."""
  torch, de = env
  opt = opt_of(de, "adam")
  cases = [Case(torch, de, opt, "cm8_%d" % i, [64, 32, 128][i], seed=80 + i) for i in range(3)]
  reqs = [[c.request(torch, r, build=(r == 1)) for c in cases] for r in range(1, 11)]
  ps = [opt.params(r) for r in range(1, 11)]
  torch.cuda.synchronize()
  for r in range(10):
    many(reqs[r], ps[r])
  for r in range(10):
    for c in cases:
      c.single(torch, ps[r], r + 1, build=(r == 0))
  assert_twins(torch, de, opt, cases)


# ---- 9. the optimizer's method ---------------------------------------------------------------------------------------------------
def sparse_inputs(torch, seed, n_rows=128):
  ids, seg, w = batch(torch, seed, n_rows=n_rows, per_row=4, planted=0)
  seg = torch.repeat_interleave(torch.arange(n_rows, device="cuda"), 4)
  return (seg, ids), w


def lookups(torch, de, vs, sps, ws, rows=128):
  res = de.embedding_lookup_sparse_many(vs, sps, ws, combiner="mean", return_trainable=True, num_rows=rows)
  return [tw for _, tw in res]


@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_apply_combined_gradients_many_equals_the_loop(env, monkeypatch, rule):
  torch, de = env
  opt = opt_of(de, rule)
  dims = [64, 32, 128]
  va = [make_var(torch, de, opt, "cm9a_%s_%d" % (rule, i), d) for i, d in enumerate(dims)]
  vb = [make_var(torch, de, opt, "cm9b_%s_%d" % (rule, i), d) for i, d in enumerate(dims)]
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  sps, ws = zip(*[sparse_inputs(torch, 90 + i) for i in range(3)])
  for step in (1, 2):
    Gs = [grad(torch, 90 + i, 128, d, step) for i, d in enumerate(dims)]
    db.apply_combined_gradients(list(zip(Gs, lookups(torch, de, vb, sps, ws))))
    tws = lookups(torch, de, va, sps, ws)
    calls = Calls(monkeypatch)
    da.apply_combined_gradients_many(list(zip(Gs, tws)))
    assert calls["tfra_multi_apply_planned_combined"] == 1
    assert calls["tfra_table_apply_planned_combined"] == 0 and calls["tfra_unique"] == 0
    monkeypatch.undo()
    assert da.iterations == db.iterations == step
  for a, b in zip(va, vb):
    for x, y in zip(_export_state(torch, de, da, opt, a), _export_state(torch, de, db, opt, b)):
      assert torch.equal(x, y)


def test_apply_combined_gradients_many_mixed_lists(env, monkeypatch):
  """The same variable twice (two grouped calls, in the list's order) and an ineligible pair in the middle (two shards on one
  device: the per-pair path), against apply_combined_gradients over the same list; a max_norm wrapper is refused first."""
  torch, de = env
  opt = opt_of(de, "adam")
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  dev = "cuda:%d" % torch.cuda.current_device()

  def variables(tag):
    vs = [make_var(torch, de, opt, "cm10%s_0" % tag, 64),
          de.Variable(dim=32, name="cm10%s_1" % tag, initializer=0.5, devices=[dev, dev], **kw),
          make_var(torch, de, opt, "cm10%s_2" % tag, 128)]
    return vs + [vs[0]]                                                    # the first variable again, with other ids

  va, vb = variables("a"), variables("b")
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  sps, ws = zip(*[sparse_inputs(torch, 95 + i) for i in range(4)])
  Gs = [grad(torch, 95 + i, 128, v.dim) for i, v in enumerate(va)]
  db.apply_combined_gradients(list(zip(Gs, lookups(torch, de, vb, sps, ws))))
  tws = lookups(torch, de, va, sps, ws)
  calls = Calls(monkeypatch)
  da.apply_combined_gradients_many(list(zip(Gs, tws)))
  assert calls["tfra_multi_apply_planned_combined"] == 2 and calls["tfra_table_apply_planned_combined"] == 0
  monkeypatch.undo()
  assert da.iterations == db.iterations == 1
  for a, b in zip(va[:3], vb[:3]):
    for x, y in zip(_export_state(torch, de, da, opt, a), _export_state(torch, de, db, opt, b)):
      assert torch.equal(x, y)
  # max_norm: ValueError before any table changes (and before the step advances)
  before = [_export_state(torch, de, da, opt, v) for v in va[:3]]
  tws = lookups(torch, de, va[:1], sps[:1], ws[:1])
  _, clipped = de.embedding_lookup_sparse(va[2], sps[2], ws[2], combiner="mean", max_norm=1.0, return_trainable=True, num_rows=128)
  with pytest.raises(ValueError):
    da.apply_combined_gradients_many([(Gs[0], tws[0]), (Gs[2], clipped)])
  assert da.iterations == 1
  for v, b in zip(va[:3], before):
    for x, y in zip(b, _export_state(torch, de, da, opt, v)):
      assert torch.equal(x, y)
