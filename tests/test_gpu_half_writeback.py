"""GPU: the planned / sparse write-back (tfra_table_apply_sparse, _apply_planned, _apply_planned_combined, the step drivers)
on float16 and bfloat16 tables.

"Twin" = a second table of the same options driven through tfra_reduce_by_key + tfra_table_apply_optimizer, the route half
tables took before the planned kernels served them.  Both routes sum a key's gradients with the same tree, evaluate the same
fp32 rule under -ffp-contract=off and round once, so on a table that is not evicting they must leave THE SAME BYTES: the
comparisons below are torch.equal on int16 views (NaN patterns count), no tolerance."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VDTYPES = ["float16", "bfloat16"]
KINDS = ["sgd", "adam", "adagrad", "ftrl"]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_opt(de, kind):
  return {"sgd": de.optimizers.SGD(0.1), "adam": de.optimizers.Adam(0.01, 0.9, 0.999, 1e-7),
          "adagrad": de.optimizers.Adagrad(0.05, 0.1), "ftrl": de.optimizers.Ftrl(0.05, -0.5, 0.1, 1e-3, 1e-3)}[kind]


_serial = [0]


def make_var(torch, de, opt, vdtype, dim, tag, bounded=None, cap=0):
  """A one-shard half variable with the optimizer's slots; bounded = an HkvEvictStrategy for a bounded table of `cap` slots."""
  _serial[0] += 1
  name = "hw_%s_%s_%d_%d" % (tag, vdtype, dim, _serial[0])
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  dt = getattr(torch, vdtype)
  if bounded is None:
    return de.Variable(dim=dim, name=name, value_dtype=dt, initializer=0.25, **kw)
  return de.get_variable(name, key_dtype=torch.int64, value_dtype=dt, initializer=0.25, dim=dim, init_size=cap,
                         kv_creator=de.HkvHashTableCreator(config=de.HkvHashTableConfig(
                             init_capacity=cap, max_capacity=cap, max_hbm_for_values=1 << 28, evict_strategy=bounded)), **kw)


def dev_table(var):
  return var.tables[0]._table


def default_row(torch, var):
  return var.tables[0]._default_value.to(torch.float32)


def twin_apply(torch, de, var, p, ids, g):
  """reduce_by_key + apply_optimizer: the unchanged route."""
  uniq, gsum, cnt = de.device_ops.reduce_by_key(ids, g)
  dev_table(var).apply_optimizer(p, uniq, gsum, default_row(torch, var), n_dev=cnt)


def state(torch, de, opt, var, keys=None):
  """(sorted keys, rows, slot fields ...) as int16 bit patterns; keys=None: every key of the table."""
  if keys is None:
    k, v = var.export()
    o = torch.argsort(k)
    k, v = k[o], v[o]
  else:
    k = keys
    v = var.lookup(k)
  deo = de.DynamicEmbeddingOptimizer(opt)
  out = [k, v.contiguous().view(torch.int16)]
  for s in opt.slots:
    out.append(deo.get_slot(var, s).lookup(k).contiguous().view(torch.int16))
  return out


def assert_same_state(torch, a, b, what):
  assert torch.equal(a[0], b[0]), "%s: key sets differ (%d vs %d keys)" % (what, a[0].numel(), b[0].numel())
  for f, (x, y) in enumerate(zip(a[1:], b[1:])):
    assert torch.equal(x, y), "%s: field %d differs in %d elements" % (what, f, int((x != y).sum()))


def batches(rng, dim, steps=5, B=4096, n_keys=500, big=131072):
  out = []
  for _ in range(steps):   # heavy repeats: ~8 occurrences per key and more, hot partial sums
    out.append((rng.integers(0, n_keys, size=B).astype(np.int64), (rng.standard_normal((B, dim)) * 0.1).astype(np.float32)))
  if big:
    ids = (rng.zipf(1.2, size=big) % 1_000_003).astype(np.int64) * 7919 - 5
    out.append((ids, (rng.standard_normal((big, dim)) * 0.1).astype(np.float32)))
  return out


# ---- 1 / 2: the one-call and the planned form against the twin ------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 128])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_apply_sparse_equals_reduce_then_apply_bytewise(env, kind, vdtype, dim):
  """tfra_table_apply_sparse on a half table (growing): after every step the exported keys, the rows and every slot field equal
  the twin's, bit for bit.  (Before the planned kernels took half rows the call returned TFRA_ERR_UNSUPPORTED.)"""
  torch, de = env
  opt = make_opt(de, kind)
  va, vb = make_var(torch, de, opt, vdtype, dim, "one_a"), make_var(torch, de, opt, vdtype, dim, "one_b")
  rng = np.random.default_rng(100 + dim)
  for step, (ids, g) in enumerate(batches(rng, dim), 1):
    p = opt.params(step)
    it, gt = T(torch, ids), T(torch, g)
    dev_table(va).apply_sparse(p, it, gt, default_row(torch, va))
    twin_apply(torch, de, vb, p, it, gt)
    assert_same_state(torch, state(torch, de, opt, va), state(torch, de, opt, vb), "step %d" % step)
  dev_table(va).check_errors()


@pytest.mark.parametrize("dim", [32, 128])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_apply_planned_equals_apply_sparse_bytewise(env, kind, vdtype, dim):
  """plan.build(ids) on a side stream, then apply_planned: the bytes of the one-call form after every step."""
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  opt = make_opt(de, kind)
  va, vb = make_var(torch, de, opt, vdtype, dim, "pl_a"), make_var(torch, de, opt, vdtype, dim, "pl_b")
  rng = np.random.default_rng(100 + dim)
  plan = SparsePlan("cuda:0", dim)
  side = torch.cuda.Stream(device="cuda:0")
  for step, (ids, g) in enumerate(batches(rng, dim), 1):
    p = opt.params(step)
    it, gt = T(torch, ids), T(torch, g)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      plan.build(it)
    dev_table(va).apply_planned(p, plan, gt, default_row(torch, va))
    dev_table(vb).apply_sparse(p, it, gt, default_row(torch, vb))
    assert_same_state(torch, state(torch, de, opt, va), state(torch, de, opt, vb), "step %d" % step)
  dev_table(va).check_errors()


# ---- 3: against the NumPy rules -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["apply_sparse", "plan_at_lookup"])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_half_writeback_against_numpy_rules(env, kind, vdtype, form):
  """deo.apply_sparse, and embedding_lookup(plan_writeback=True) + apply_gradients, against oracle/optimizers.py applied to the
  up-cast rows with one rounding per step — the comparison and the bound of test_fused_optimizers_on_half_tables
  (0.999-quantile <= 2 storage ulp, max <= 4 ulp), taken over unchanged."""
  torch, de = env
  from oracle import optimizers as oopt
  from tfra_amd.dynamic_embedding.variable import PLAN_AT_LOOKUP_MIN_IDS
  dt = getattr(torch, vdtype)
  dim, n_keys, B = 32, 500, max(8192, PLAN_AT_LOOKUP_MIN_IDS)
  opt = make_opt(de, kind)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = make_var(torch, de, opt, vdtype, dim, "np_" + form)
  rng = np.random.default_rng(3)

  def cast(x):   # float32 -> storage type -> float32, round to nearest even like the kernel
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dt).to(torch.float32).numpy()

  ulp = 2.0 ** -10 if vdtype == "float16" else 2.0 ** -7
  init_acc = 0.1
  state_ = {}
  for step in range(1, 5):
    ids = rng.integers(0, n_keys, size=B).astype(np.int64)
    g = (rng.standard_normal((B, dim)) * 0.1).astype(np.float32)
    if form == "apply_sparse":
      deo.apply_sparse(var, T(torch, ids), T(torch, g))
    else:
      emb, tw = de.embedding_lookup(var, T(torch, ids), return_trainable=True, plan_writeback=True)
      assert emb.dtype == dt
      assert tw.plan is not None   # the write-back of this batch is the planned one
      deo.apply_gradients([(T(torch, g), tw)])
    uniq, gsum, _ = oopt.segment_sum_by_key(ids, g)
    for k, gs in zip(uniq.tolist(), gsum):
      # a new row starts from the float32 default / initial slot values (not from their rounded images)
      p, s1, s2 = state_.get(k, [np.full(dim, 0.25, np.float32), np.full(dim, init_acc if kind in ("adagrad", "ftrl") else 0.0, np.float32),
                                 np.zeros(dim, np.float32)])
      if kind == "sgd":
        p = oopt.sgd(p, gs, 0.1)
      elif kind == "adam":
        p, s1, s2 = oopt.adam(p, s1, s2, gs, 0.01, 0.9, 0.999, 1e-7, step)
      elif kind == "adagrad":
        p, s1 = oopt.adagrad(p, s1, gs, 0.05)
      else:
        p, s1, s2 = oopt.ftrl(p, s1, s2, gs, 0.05, 1e-3, 1e-3)
      state_[k] = [cast(p), cast(s1), cast(s2)]
  keys = np.array(sorted(state_), np.int64)
  got = var.lookup(T(torch, keys)).to(torch.float32).cpu().numpy()
  want = np.stack([state_[k][0] for k in keys.tolist()])
  err = np.abs(got - want) / np.maximum(np.abs(want), 2.0 ** -14)
  print("half write-back vs numpy (%s %s %s): q999 %.3g max %.3g ulp %.3g" % (kind, vdtype, form, float(np.quantile(err, 0.999)), float(err.max()), ulp))
  assert float(np.quantile(err, 0.999)) <= 2 * ulp and float(err.max()) <= 4 * ulp, (float(err.max()), ulp)
  assert var.size() == keys.size


# ---- 4: combined write-back ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_combined_writeback_on_half_rows_bytewise(env, monkeypatch, kind, vdtype, combiner):
  """embedding_lookup_sparse(return_trainable) + apply_combined_gradients on a half variable == sparse_segment_combine_backprop
  + the twin route, bit for bit (weights, one row without entries, one row of weight 0), and the fused branch is the one that ran."""
  torch, de = env
  dim, n_rows, per_row = 64, 2048, 8
  opt = make_opt(de, kind)
  va, vb = make_var(torch, de, opt, vdtype, dim, "cb_a"), make_var(torch, de, opt, vdtype, dim, "cb_b")
  da = de.DynamicEmbeddingOptimizer(opt)
  rng = np.random.default_rng(17)
  backprop = de.device_ops.sparse_segment_combine_backprop
  for step in range(1, 4):
    ids = (rng.zipf(1.2, size=n_rows * per_row) % 200_000).astype(np.int64)
    seg = np.repeat(np.arange(n_rows, dtype=np.int64), per_row)
    w = rng.uniform(0.1, 2.0, size=ids.size).astype(np.float32)
    keep = seg != 7                       # row 7 has no entries
    ids, seg, w = ids[keep], seg[keep], w[keep]
    w[seg == 3] = 0.0                     # row 3: weight sum 0
    G = T(torch, (rng.standard_normal((n_rows, dim)) * 0.1).astype(np.float32))
    st, it, wt = T(torch, seg), T(torch, ids), T(torch, w)
    eg = backprop(G, st, wt, combiner)
    twin_apply(torch, de, vb, opt.params(step), it, eg)
    _, tw = de.embedding_lookup_sparse(va, (st, it), wt, combiner=combiner, return_trainable=True, num_rows=n_rows,
                                       plan_writeback=(step % 2 == 0))

    def boom(*a, **k):
      raise AssertionError("apply_combined_gradients wrote the entry gradients out: the fused branch did not run")
    with monkeypatch.context() as m:
      m.setattr(de.device_ops, "sparse_segment_combine_backprop", boom)
      da.apply_combined_gradients([(G, tw)])
    assert_same_state(torch, state(torch, de, opt, va), state(torch, de, opt, vb), "step %d" % step)
  dev_table(va).check_errors()


# ---- 5: bounded tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["LRU", "EPOCHLFU"])
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_bounded_table_below_capacity_bytewise(env, kind, vdtype, strategy):
  """A bounded table with max_capacity = 4x the keys ever inserted never evicts: bytes equal to the twin, no errors."""
  torch, de = env
  dim = 32
  opt = make_opt(de, kind)
  strat = getattr(de.HkvEvictStrategy, strategy)
  rng = np.random.default_rng(29)
  bs = batches(rng, dim, big=0)
  ids = (rng.zipf(1.2, size=16384) % 5000).astype(np.int64) + 1000
  bs.append((ids, (rng.standard_normal((ids.size, dim)) * 0.1).astype(np.float32)))
  inserted = np.unique(np.concatenate([b[0] for b in bs])).size
  cap = 32768
  assert cap >= 4 * inserted
  va, vb = make_var(torch, de, opt, vdtype, dim, "bb_a", strat, cap), make_var(torch, de, opt, vdtype, dim, "bb_b", strat, cap)
  for step, (ids, g) in enumerate(bs, 1):
    p = opt.params(step)
    it, gt = T(torch, ids), T(torch, g)
    dev_table(va).apply_sparse(p, it, gt, default_row(torch, va))
    twin_apply(torch, de, vb, p, it, gt)
    assert_same_state(torch, state(torch, de, opt, va), state(torch, de, opt, vb), "step %d" % step)
  dev_table(va).check_errors()
  dev_table(vb).check_errors()
  assert int(va.size()) == inserted


@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_bounded_table_at_capacity_new_rows(env, kind, vdtype):
  """LRU table filled to its capacity, then ONE batch of all-distinct never-seen keys, a quarter of the capacity: every key of the
  batch takes the eviction path (PHASE2).  size() == capacity before and after (capacity = every slot an ordinary key can take:
  tfra_table_capacity also counts the slots reserved for the sentinel keys, so "at capacity" is asserted as no empty slot in the
  census and size() == the census' live slots == capacity - those reserved slots), no errors, and every batch key resident afterwards
  holds exactly round(rule(default row, aux_init, g)) — what the twin's apply_kernel writes for the same key on a scratch table (a
  new row's result does not depend on which victim it replaced).
  Share of batch keys that must be resident: ALL of them.  That is what the fp32 at-capacity test of the planned apply requires
  (tests/test_gpu_frontend.py, test_prefetch_step_driver_matches_eager part (b): `ex.all()` after batches of 1500 on 4096 slots),
  and it follows from LRU: a new key's score is the device clock of this write-back, above every score written earlier, so a
  batch key could only be chosen as a victim if all 30 slots of another batch key's two home buckets held batch keys."""
  torch, de = env
  dim, cap = 32, 8192
  opt = make_opt(de, kind)
  var = make_var(torch, de, opt, vdtype, dim, "cap", de.HkvEvictStrategy.LRU, cap)
  scratch = make_var(torch, de, opt, vdtype, dim, "cap_scratch")
  dt = getattr(torch, vdtype)
  capacity = dev_table(var).capacity()
  old = -np.arange(1, 4 * capacity + 1, dtype=np.int64)
  for part in np.array_split(old, 8):
    var.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=dt))
  census = dev_table(var).slot_census()
  slots = census["live"]
  assert census["empty"] == 0 and census["locked"] == 0 and int(var.size()) == slots
  assert capacity - 16 <= slots <= capacity   # (the difference: slots reserved for the sentinel keys)
  rng = np.random.default_rng(31)
  B = slots // 4
  ids = np.arange(B, dtype=np.int64) * 7919 + 13
  rng.shuffle(ids)
  g = (rng.standard_normal((B, dim)) * 0.1).astype(np.float32)
  it, gt = T(torch, ids), T(torch, g)
  p = opt.params(1)
  dev_table(var).apply_sparse(p, it, gt, default_row(torch, var))
  twin_apply(torch, de, scratch, p, it, gt)
  dev_table(var).check_errors()
  census = dev_table(var).slot_census()
  assert census["empty"] == 0 and census["locked"] == 0 and census["live"] == slots and int(var.size()) == slots
  rows, ex = var.lookup(it, return_exists=True)
  assert bool(ex.all()), "%d of %d batch keys are not resident" % (int((~ex).sum()), B)
  assert_same_state(torch, state(torch, de, opt, var, it), state(torch, de, opt, scratch, it), "new rows")


# ---- 6: the step drivers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_prefetch_step_on_half_variable(env, kind, vdtype):
  """PrefetchStep, 6 steps with rotating plans: the returned rows have the variable's dtype and are var.lookup(ids) taken before
  the step; the final table equals a twin driven by apply_sparse, bit for bit."""
  torch, de = env
  dim, B = 64, 16384
  dt = getattr(torch, vdtype)
  opt = make_opt(de, kind)
  va, vb = make_var(torch, de, opt, vdtype, dim, "ps_a"), make_var(torch, de, opt, vdtype, dim, "ps_b")
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  rng = np.random.default_rng(37)
  bs = [((rng.zipf(1.2, size=B) % 50_000).astype(np.int64) * 31 + 7, (rng.standard_normal((B, dim)) * 0.1).astype(np.float32)) for _ in range(6)]
  ps = de.PrefetchStep(va, da).prime(T(torch, bs[0][0]))
  for i, (ids, g) in enumerate(bs):
    it = T(torch, ids)
    before = va.lookup(it)
    rows = ps.step(T(torch, g), T(torch, bs[i + 1][0]) if i + 1 < len(bs) else None)
    assert rows.dtype == dt and tuple(rows.shape) == (B, dim)
    assert torch.equal(rows.view(torch.int16), before.view(torch.int16)), "step %d" % i
    db.apply_sparse(vb, it, T(torch, g))
  torch.cuda.synchronize()
  assert_same_state(torch, state(torch, de, opt, va), state(torch, de, opt, vb), "after 6 steps")
  dev_table(va).check_errors()


@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_multi_table_prefetch_step_on_half_variables(env, kind, vdtype):
  """MultiTablePrefetchStep over a half and a float32 variable: rows come back in each variable's dtype, tables equal eager twins."""
  torch, de = env
  dims, B = (32, 64), 8192
  dt = getattr(torch, vdtype)
  opt = make_opt(de, kind)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  _serial[0] += 1
  vs_a = [make_var(torch, de, opt, vdtype, dims[0], "ms_a"), de.Variable(dim=dims[1], name="hw_ms_f32_a_%d" % _serial[0], initializer=0.25, **kw)]
  vs_b = [make_var(torch, de, opt, vdtype, dims[0], "ms_b"), de.Variable(dim=dims[1], name="hw_ms_f32_b_%d" % _serial[0], initializer=0.25, **kw)]
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  rng = np.random.default_rng(41)
  steps = [[((rng.zipf(1.2, size=B) % 20_000).astype(np.int64) + 5, (rng.standard_normal((B, d)) * 0.1).astype(np.float32)) for d in dims]
           for _ in range(4)]
  ms = de.MultiTablePrefetchStep(vs_a, da).prime([T(torch, x[0]) for x in steps[0]])
  for i, st in enumerate(steps):
    before = [v.lookup(T(torch, x[0])) for v, x in zip(vs_a, st)]
    torch.cuda.synchronize()
    outs = ms.step([T(torch, x[1]) for x in st], [T(torch, x[0]) for x in steps[i + 1]] if i + 1 < len(steps) else None)
    ms.synchronize()
    assert outs[0].dtype == dt and outs[1].dtype == torch.float32
    assert torch.equal(outs[0].view(torch.int16), before[0].view(torch.int16))
    assert torch.equal(outs[1], before[1])
    p = db.begin_step()
    for v, x in zip(vs_b, st):
      db.apply_sparse(v, T(torch, x[0]), T(torch, x[1]), p)
  ms.synchronize()
  torch.cuda.synchronize()
  for a, b in zip(vs_a, vs_b):
    # (state() views rows as int16; for the float32 variable that is two words per element, still a bit comparison)
    assert_same_state(torch, state(torch, de, opt, a), state(torch, de, opt, b), "dim %d" % a.dim)


@pytest.mark.parametrize("vdtype", VDTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_captured_train_step_on_half_variable(env, kind, vdtype):
  """CapturedTrainStep (one HIP graph, a single stream's chain) on a half variable: 3 replays == 3 eager steps."""
  torch, de = env
  dim, B = 64, 8192
  opt = make_opt(de, kind)
  rng = np.random.default_rng(43)
  bs = [(rng.zipf(1.2, size=B) % 30_000).astype(np.int64) * 3 + 1 for _ in range(3)]
  g = (rng.standard_normal((B, dim)) * 0.1).astype(np.float32)
  outs = []
  for mode in ("eager", "captured"):
    deo = de.DynamicEmbeddingOptimizer(opt)
    _serial[0] += 1
    v = de.Variable(dim=dim, name="hw_cap_%s_%s_%d" % (mode, vdtype, _serial[0]), value_dtype=getattr(torch, vdtype), initializer=0.25,
                    init_size=200000, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    looks = []
    if mode == "eager":
      for _ in range(2):   # the captured variant runs 2 eager warm-up steps on batch 0 ...
        deo.apply_sparse(v, T(torch, bs[0]), T(torch, g))
      deo.iterations += 1  # ... and spends one step number on the capture itself (not executed)
      for b in bs:
        looks.append(v.lookup(T(torch, b)).view(torch.int16).cpu())
        deo.apply_sparse(v, T(torch, b), T(torch, g))
    else:
      cap = de.CapturedTrainStep(v, deo, B)
      cap.grads.copy_(T(torch, g))
      cap.capture(warmup_ids=T(torch, bs[0]))
      for b in bs:
        looks.append(cap.step(T(torch, b)).view(torch.int16).cpu().clone())
      torch.cuda.synchronize()
      cap.close()
    outs.append((state(torch, de, opt, v), looks))
  assert_same_state(torch, outs[0][0], outs[1][0], "after 3 steps")
  for i, (a, b) in enumerate(zip(outs[0][1], outs[1][1])):
    assert torch.equal(a, b), "lookup of step %d" % i


# ---- 7: more than 2^18 ids -------------------------------------------------------------------------------------------------------
def test_apply_sparse_more_than_2_18_ids(env):
  """fp16, Adam, 600 000 ids over 50 000 keys (apply_sparse_big).  Byte equality was practical, so that is what is asserted: the
  twin is fed the per-key fp32 sums built the way apply_sparse_big documents — tfra_reduce_by_key per chunk of 2^18 ids, the chunk
  results concatenated, then a key's (at most three) chunk sums added in chunk order by a second tfra_reduce_by_key."""
  torch, de = env
  dim, n, n_keys, chunk = 32, 600_000, 50_000, 1 << 18
  opt = make_opt(de, "adam")
  va, vb = make_var(torch, de, opt, "float16", dim, "big_a"), make_var(torch, de, opt, "float16", dim, "big_b")
  rng = np.random.default_rng(47)
  for step in (1, 2):
    ids = rng.integers(0, n_keys, size=n).astype(np.int64) * 11 + 3
    g = (rng.standard_normal((n, dim)) * 0.1).astype(np.float32)
    it, gt = T(torch, ids), T(torch, g)
    p = opt.params(step)
    dev_table(va).apply_sparse(p, it, gt, default_row(torch, va))
    ks, ss = [], []
    for off in range(0, n, chunk):
      k, s, c = de.device_ops.reduce_by_key(it[off:off + chunk], gt[off:off + chunk])
      c = int(c.item())
      ks.append(k[:c])
      ss.append(s[:c])
    kc, sc = torch.cat(ks), torch.cat(ss)
    assert kc.numel() <= chunk
    twin_apply(torch, de, vb, p, kc, sc)
    assert_same_state(torch, state(torch, de, opt, va), state(torch, de, opt, vb), "step %d" % step)
  dev_table(va).check_errors()


# ---- 8: refusals stay refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", ["int8", "int32"])
def test_integer_tables_are_still_refused(env, vdtype):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  dim = 32
  dt = getattr(torch, vdtype)
  t = de.CuckooHashTable(torch.int64, dt, torch.zeros(dim, dtype=dt), device="cuda:0", dim=dim, name="hw_refuse_" + vdtype)
  ids = torch.arange(64, device="cuda", dtype=torch.int64)
  g = torch.ones((64, dim), device="cuda")
  p = make_opt(de, "sgd").params(1)
  with pytest.raises(_capi.TfraError) as e:
    t._table.apply_sparse(p, ids, g, torch.zeros(dim))
  assert e.value.code == -6 and "float32, float16 or bfloat16" in str(e.value)
  plan = SparsePlan("cuda:0", dim).build(ids)
  with pytest.raises(_capi.TfraError) as e:
    t._table.apply_planned(p, plan, g, torch.zeros(dim))
  assert e.value.code == -6 and "float32, float16 or bfloat16" in str(e.value)
  assert int(t.size().item()) == 0


@pytest.mark.parametrize("vdtype", VDTYPES)
def test_gradient_route_still_refuses_half_rows(env, vdtype):
  """tfra_route_create ships fp32 rows: a half table is refused by the C entry point and by NativeRoutedStep."""
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.distributed import NativeRoutedStep
  opt = make_opt(de, "sgd")
  var = make_var(torch, de, opt, vdtype, 32, "route")
  h = ctypes.c_void_p()
  with pytest.raises(_capi.TfraError) as e:
    _capi.call("tfra_route_create", dev_table(var)._h, None, 0, 1 << 16, _capi.ROUTE_NO_THREAD, ctypes.byref(h))
  assert e.value.code == -6
  with pytest.raises(ValueError):
    NativeRoutedStep(var, de.DynamicEmbeddingOptimizer(opt), transport=None, threaded=False)
