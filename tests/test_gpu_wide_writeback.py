"""GPU: the planned sparse write-back for wide rows (tfra_*_wide, 256 < dim <= 1024), one wave per key.

Every addition of the wide kernels is per column and in the plan's order, so the columns [a, b) of a wide table must end BIT FOR
BIT as a narrow table of those columns driven through the twin call with the same ids and that slice of the gradient (expected A).
All test data is dyadic — rows k/8, gradients k * 2^-6, weights and learning rate powers of two, a row's weights summing to 2 — so
every gradient sum is exact in float32: SGD must equal the float64 result rounded once to the row type with no tolerance (B), and
Adagrad / Adam on float32 rows the float64 rule at rtol = atol = 1e-6, the bound tests/test_gpu_csr.py holds the narrow write-back
to against its exactly-summed oracle (C; hyper-parameters enter the float64 rule as the float32 values the kernels receive)."""
import ctypes

import numpy as np
import pytest

from tests.sparse_helpers import Calls, T

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 8, 9, 16, 17, 600, 1, 1, 2, 3, 9, 19]   # occurrences per key: 13 = 4 * 3 + 1 keys, 688 = 4 * 172 entries
KEYS = (np.arange(len(COUNTS), dtype=np.int64) * 7919 - 20000)
RESIDENT = KEYS[::2]                                     # the others are never seen before the first step
N_ROWS, W_ROW = 172, np.array([1.0, 0.5, 0.25, 0.25], np.float32)
FORMS = ["sparse", "planned", "combined"]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def batch():
  rng = np.random.default_rng(5)
  ids = np.repeat(KEYS, COUNTS)
  rng.shuffle(ids)
  return ids, np.repeat(np.arange(N_ROWS, dtype=np.int64), 4), np.tile(W_ROW, N_ROWS)


def make_opt(de, rule):
  return {"sgd": lambda: de.optimizers.SGD(0.5), "adagrad": lambda: de.optimizers.Adagrad(0.05, 0.1),
          "adam": lambda: de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)}[rule]()


_serial = [0]


def make_var(torch, de, opt, vdtype, dim, rows, bounded=0):
  _serial[0] += 1
  kw = dict(de.DynamicEmbeddingOptimizer.variable_kwargs(opt), value_dtype=getattr(torch, vdtype), initializer=0.5, dim=dim)
  if bounded:
    cfg = de.HkvHashTableConfig(init_capacity=bounded, max_capacity=bounded, max_hbm_for_values=1 << 28,
                                evict_strategy=de.HkvEvictStrategy.LRU)
    return de.get_variable("ww_%d" % _serial[0], key_dtype=torch.int64, init_size=bounded, kv_creator=de.HkvHashTableCreator(config=cfg), **kw)
  var = de.Variable(name="ww_%d" % _serial[0], **kw)
  var.upsert(T(torch, RESIDENT), rows.to(var.value_dtype))
  return var


def state(torch, de, opt, var, keys=None):
  """[sorted keys, rows, slot fields ...] of the whole table, or of `keys`"""
  if keys is None:
    keys = torch.sort(var.export()[0])[0]
  deo = de.DynamicEmbeddingOptimizer(opt)
  return [keys, var.lookup(keys)] + [deo.get_slot(var, s).lookup(keys) for s in opt.slots]


def drive(torch, form, wide, var, p, ids, G, seg, w, comb):
  """one write-back through `form` of the wide calls or of their twins; G: the entry gradients, or grad_out for `combined`"""
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  t = var.tables[0]._table
  d = var.tables[0]._default_value.to(torch.float32)
  sfx = "_wide" if wide else ""
  if form == "sparse":
    return getattr(t, "apply_sparse" + sfx)(p, ids, G, d)
  plan = SparsePlan(var._primary, var.dim).build(ids)
  if form == "planned":
    return getattr(t, "apply_planned" + sfx)(p, plan, G, d)
  return getattr(t, "apply_planned_combined" + sfx)(p, plan, G, seg, w, comb, d)


def rule64(rule, opt, step, p, s, g):
  """the float64 rule on rows p, slots s and gradient sums g, hyper-parameters as the float32 values of tfra_opt_params"""
  f = lambda x: float(np.float32(x))
  if rule == "sgd":
    return p - f(opt.lr) * g, []
  if rule == "adagrad":
    a = s[0] + g * g
    return p - f(opt.lr) * g / np.sqrt(a), [a]
  m = s[0] + (g - s[0]) * (1.0 - f(opt.b1))
  v = s[1] + (g * g - s[1]) * (1.0 - f(opt.b2))
  return p - (m * f(opt._lr_t(step))) / (np.sqrt(v) + f(opt.eps)), [m, v]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("vdtype,dim", [("float32", 260), ("float32", 512), ("float16", 768), ("bfloat16", 1024)])
def test_wide_forms_against_the_narrow_kernels_and_float64(env, vdtype, dim, rule, form):
  torch, de = env
  opt = make_opt(de, rule)
  ids_np, seg_np, w_np = batch()
  ids, seg, w = T(torch, ids_np), T(torch, seg_np), T(torch, w_np)
  comb = 0 if rule == "sgd" else 1   # sum | mean (a row's weights sum to 2)
  g = torch.Generator(device="cuda").manual_seed(dim)
  rows = torch.randint(-8, 9, (RESIDENT.size, dim), generator=g, device="cuda").float() / 8
  cuts = [(a, min(a + 256, dim)) for a in range(0, dim, 256)]
  wide = make_var(torch, de, opt, vdtype, dim, rows)
  narrow = [make_var(torch, de, opt, vdtype, b - a, rows[:, a:b]) for a, b in cuts]
  # the float64 model: every key's row and slots as stored
  order = np.argsort(KEYS)
  P = np.full((KEYS.size, dim), 0.5)
  P[::2] = rows.cpu().numpy()
  S = [np.full((KEYS.size, dim), float(a)) for a in opt.aux_init()[:len(opt.slots)]]
  inv = np.searchsorted(KEYS, ids_np)
  dt = getattr(torch, vdtype)
  stored = lambda x: torch.from_numpy(x).to(torch.float32).to(dt).to(torch.float64).numpy()
  for step in (1, 2):
    n_g = N_ROWS if form == "combined" else ids_np.size
    G = torch.randint(-4, 5, (n_g, dim), generator=g, device="cuda").float() / 64
    p = opt.params(step)
    drive(torch, form, True, wide, p, ids, G, seg, w, comb)
    for (a, b), nv in zip(cuts, narrow):
      drive(torch, form, False, nv, p, ids, G[:, a:b].contiguous(), seg, w, comb)
    torch.cuda.synchronize()
    wide.tables[0]._table.check_errors()
    got = state(torch, de, opt, wide)
    assert int(wide.size()) == KEYS.size and torch.equal(got[0], T(torch, KEYS[order]))
    # A: every field, bit for bit, the narrow tables' columns
    parts = [state(torch, de, opt, nv) for nv in narrow]
    for f in range(1, len(got)):
      want = torch.cat([s[f] for s in parts], dim=1)
      assert torch.equal(got[f].view(torch.int32 if vdtype == "float32" else torch.int16),
                         want.view(torch.int32 if vdtype == "float32" else torch.int16)), (step, f)
    # B / C: the float64 rule on exact sums
    E = G.cpu().numpy().astype(np.float64)
    if form == "combined":
      E = E[seg_np] / (1.0 if comb == 0 else 2.0) * w_np[:, None].astype(np.float64)
    sums = np.zeros((KEYS.size, dim))
    np.add.at(sums, inv, E)
    P, S = rule64(rule, opt, step, P, S, sums)
    if rule == "sgd":
      P = stored(P)
      assert np.array_equal(got[1].to(torch.float64).cpu().numpy(), P[order]), step
    elif vdtype == "float32":
      for f, want in enumerate([P] + S):
        np.testing.assert_allclose(got[1 + f].cpu().numpy(), want[order], rtol=1e-6, atol=1e-6)
    else:
      continue   # (the half classes of Adagrad / Adam are held by A alone)
    P, S = stored(P), [stored(x) for x in S]   # (the next step reads what the table holds)


def test_bounded_table_at_capacity(env):
  """LRU table of 1024 slots at dim 512, filled beyond its capacity, then one wide write-back of 100 never-seen keys: all of them
  take the eviction phase (the second launch).  Every batch key ends resident with exactly the bits the two dim-256 slice tables,
  prepared and driven the same way through the narrow call, hold for it; the size does not move; no errors.  (WHICH old keys
  leave is not compared between tables: two groups that share one home bucket evict in execution order.)"""
  torch, de = env
  opt = make_opt(de, "adam")
  dim, cap = 512, 1024
  tables = [make_var(torch, de, opt, "float32", d, None, bounded=cap) for d in (dim, 256, 256)]
  old = T(torch, -np.arange(1, 4 * cap + 1, dtype=np.int64))
  for v in tables:
    v.upsert(old, torch.full((old.numel(), v.dim), 0.25, device="cuda"))
  size0 = int(tables[0].size())
  ids = T(torch, np.repeat(np.arange(100, dtype=np.int64) * 7919 + 13, 3))
  G = torch.randint(-4, 5, (ids.numel(), dim), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda").float() / 64
  p = opt.params(1)
  drive(torch, "sparse", True, tables[0], p, ids, G, None, None, 0)
  drive(torch, "sparse", False, tables[1], p, ids, G[:, :256].contiguous(), None, None, 0)
  drive(torch, "sparse", False, tables[2], p, ids, G[:, 256:].contiguous(), None, None, 0)
  tables[0].tables[0]._table.check_errors()
  keys = torch.unique(ids)
  assert bool(tables[0].lookup(keys, return_exists=True)[1].all()) and int(tables[0].size()) == size0
  got, lo, hi = (state(torch, de, opt, v, keys) for v in tables)
  for f in range(1, len(got)):
    assert torch.equal(got[f].view(torch.int32), torch.cat([lo[f], hi[f]], dim=1).view(torch.int32)), f


def raw(torch, name, *args):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _stream
  rc = getattr(_capi.lib(), name)(*args, _stream(torch.device("cuda", torch.cuda.current_device())))
  return rc, _capi.lib().tfra_last_error().decode()


def test_refusals_write_nothing(env):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan, _ptr
  torch, de = env
  opt = make_opt(de, "sgd")
  p = ctypes.byref(opt.params(1))
  ids, seg_np, w_np = batch()
  ids, seg, w = T(torch, ids), T(torch, seg_np), T(torch, w_np)
  U = _capi.ERR_UNSUPPORTED

  def refused(var, fragments, n=None, n_rows=N_ROWS, plan_dim=None):
    """the three write-backs (n: apply_sparse_wide alone; another n_rows: the combined call alone) refuse and write nothing"""
    t, d = var.tables[0]._table, var.tables[0]._default_value.to(torch.float32)
    G = torch.full((ids.numel(), var.dim), 7.0, device="cuda")
    plan = SparsePlan(var._primary, plan_dim or var.dim).build(ids)
    before = state(torch, de, opt, var)
    calls = []
    if n_rows == N_ROWS:
      calls.append(("tfra_table_apply_sparse_wide", (t._h, p, n or ids.numel(), _ptr(ids), _ptr(G), _ptr(d))))
    if n is None:
      calls.append(("tfra_table_apply_planned_combined_wide", (t._h, p, plan._h, _ptr(G), _ptr(seg), _ptr(w), 0, n_rows, _ptr(d))))
    if n is None and n_rows == N_ROWS:
      calls.append(("tfra_table_apply_planned_wide", (t._h, p, plan._h, _ptr(G), _ptr(d))))
    for name, args in calls:
      rc, msg = raw(torch, name, *args)
      assert rc == U and all(f in msg for f in fragments), (name, rc, msg)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state(torch, de, opt, var)))

  rows = lambda dim: torch.full((RESIDENT.size, dim), -3.0, device="cuda")   # sentinel rows
  plan = SparsePlan(torch.device("cuda", torch.cuda.current_device()), 512)
  for dim in (256, 258, 1028):
    rc, msg = raw(torch, "tfra_sparse_plan_build_wide", plan._h, ids.numel(), _ptr(ids), dim)
    assert rc == U and "256 < dim <= 1024" in msg and "tfra_sparse_plan_build" in msg
    refused(make_var(torch, de, opt, "float32", dim, rows(dim)), ["256 < dim <= 1024", "tfra_table_apply_"], plan_dim=256)
  sr = make_var(torch, de, opt, "bfloat16", 512, rows(512))
  sr.set_stochastic_rounding(11)
  refused(sr, ["round to nearest even"])
  big = make_var(torch, de, opt, "float32", 1024, rows(1024))
  refused(big, ["2^18"], n=(1 << 18) + 1)
  refused(big, ["n_rows * dim < 2^32"], n_rows=1 << 22)


def test_optimizer_routes(env, monkeypatch):
  torch, de = env
  ids_np, seg_np, w_np = batch()
  ids = T(torch, ids_np)

  def calls_of(opt, dim, **kw):
    """the C calls of one apply_sparse and one apply_combined_gradients over a fresh variable"""
    var = make_var(torch, de, opt, "float32", dim, torch.zeros((RESIDENT.size, dim), device="cuda"))
    deo = de.DynamicEmbeddingOptimizer(opt, **kw)
    out, tw = de.embedding_lookup_sparse(var, (T(torch, seg_np), ids), None, combiner="mean", return_trainable=True, num_rows=N_ROWS)
    c = Calls(monkeypatch)
    deo.apply_sparse(var, ids, torch.ones((ids.numel(), dim), device="cuda"))
    deo.apply_combined_gradients([(torch.ones_like(out), tw)])
    monkeypatch.undo()
    return {k: v for k, v in c.n.items() if "apply" in k or k in ("tfra_unique", "tfra_segment_sum") or "plan_build" in k}

  sgd = make_opt(de, "sgd")
  on = calls_of(sgd, 512, wide_rows=True)
  assert on["tfra_table_apply_sparse_wide"] == 1 and on["tfra_table_apply_planned_combined_wide"] == 1
  assert "tfra_unique" not in on and "tfra_segment_sum" not in on
  off = calls_of(sgd, 512)
  assert not any(k.endswith("_wide") for k in off) and off == calls_of(sgd, 512, wide_rows=False)
  assert calls_of(sgd, 64, wide_rows=True) == calls_of(sgd, 64)
  assert calls_of(sgd, 512, wide_rows=True, exact_order=True) == calls_of(sgd, 512, exact_order=True)
  generic = de.optimizers.Generic(update=lambda step, p, g: (p - 0.5 * g,))
  assert calls_of(generic, 512, wide_rows=True) == calls_of(generic, 512)
