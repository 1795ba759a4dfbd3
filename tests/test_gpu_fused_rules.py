"""GPU: the fused Momentum, Nesterov and RMSProp rules (TFRA_OPT_MOMENTUM / _NESTEROV / _RMSPROP: apply_one<4 / 5 / 6>, reached
through optimizers.Momentum(..., fused=True) / RMSProp(..., fused=True)) pinned to oracle/optimizers.py through every write-back
that instantiates them — apply_kernel / apply_evict_kernel (tfra_table_apply_optimizer) and apply_csr_body (the sparse, planned,
combined, grouped and step write-backs), float32 / float16 / bfloat16 rows, nearest-even and stochastic rounding.

Comparisons are bit for bit (tests/numeric_edges.py: assert_bits — equal bits, or a NaN where a NaN is expected), except the one
comparison of the combined write-back with backprop + apply_sparse, which has the tolerance tests/test_gpu_sparse_train.py uses for
the four earlier rules.  The inputs and references are built in tests/fused_rules_edges.py and checked without a GPU in
tests/test_fused_rules_model.py; the route drivers are those of tests/test_gpu_numeric_edges.py.

Why equality is the right bound: apply_one is IEEE add, multiply, divide and sqrt in a fixed order, compiled with
-ffp-contract=off, float32 subnormals kept; the oracle is one NumPy float32 operation per call in the same order."""
import numpy as np
import pytest

import oracle
from oracle import optimizers as oopt
from tests import fused_rules_edges as fe
from tests import numeric_edges as ne
from tests import stochastic_rounding_model as srm
from tests import test_gpu_numeric_edges as tg

pytestmark = pytest.mark.gpu

HALVES = ["float16", "bfloat16"]
SEED = 0x5EED0000C0FFEE11
T = tg.T


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


# ---- 1. the rules at their edges ----------------------------------------------------------------------------------------------------
def _rule_params():
  """(rule, vdtype, dim, route), the routes of one (rule, vdtype, dim) next to each other: they share one reference."""
  out = []
  for rule in fe.RULES:
    for vdtype, dims in (("float32", (4, 6, 68)), ("float16", (4, 68)), ("bfloat16", (4, 68))):   # float32 4: VEC4; 6: scalar
      for dim in dims:
        routes = ("apply_optimizer",) if dim % 4 else ("apply_optimizer", "apply_sparse", "apply_planned", "prefetch_step")
        out += [pytest.param(rule, vdtype, dim, r, id="%s-%s-%d-%s" % (rule, vdtype, dim, r)) for r in routes]
  return out


@pytest.mark.parametrize("rule,vdtype,dim,route", _rule_params())
def test_rules_at_their_edges(env, rule, vdtype, dim, route):
  """One write-back over the Cartesian edge grid of the rule (momentum / nesterov: g, p, accum in EDGE^3; rmsprop: g, p in EDGE, ms
  in NONNEG, mom in EDGE) against ONE call of oracle.optimizers.momentum / rmsprop and one conversion to the storage type: the
  parameter and every slot field of every key, bit for bit.  Resident rows hold the grid (rounded to the storage type first on half
  tables); in the sparse, planned and step routes ids repeat 1, 2 and 8 times and the expected sums are segment_sum_by_key's;
  never-seen keys of the same batch start from the FLOAT default 0.3 and the float aux_init (RMSProp: initial_rms 0.1, not a half
  value).  dim 4: one granule; 6: the scalar path of apply_kernel; 68: a second chunk with lanes past the row.  (PrefetchStep
  takes the default row from the variable, which keeps it in the storage type: its new rows start from that image of 0.3.)"""
  torch, de = env
  opt = fe.make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  default = ne.DEFAULT
  if route == "prefetch_step":
    default = float(ne.through_storage(torch, np.array([ne.DEFAULT], np.float32), vdtype)[0])
  c = fe.fused_case(torch, rule, vdtype, dim, route != "apply_optimizer", default)
  var = tg.make_var(torch, de, opt, vdtype, dim, "fr_" + route, default=ne.DEFAULT)
  tg.seed_rows(torch, de, deo, opt, var, c)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  tg.write_back(torch, de, route, var, deo, opt.params(1), 1, T(torch, c.ids), T(torch, c.grads), default_row)
  tg.check_rows(torch, deo, opt, var, T(torch, c.keys), (c.want_p, c.want_s1, c.want_s2), vdtype,
                "%s %s dim %d %s" % (rule, vdtype, dim, route), c.context)
  assert int(var.size()) == c.keys.size


# ---- 2. phase 2 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse"])
@pytest.mark.parametrize("vdtype", ["float32"] + HALVES)
@pytest.mark.parametrize("rule", fe.RULES)
def test_new_rows_of_a_bounded_table_at_capacity(env, rule, vdtype, route):
  """Phase 2 (apply_evict_kernel behind apply_optimizer, PHASE2 of apply_csr_body behind apply_sparse): an LRU table of 8192 slots
  filled to its capacity, then one batch of never-seen keys with the EDGE gradients.  Every batch key that is present afterwards
  holds exactly the new-row result: the rule on the float default 0.3 and the optimizer's initial slot values, converted once."""
  torch, de = env
  dim, cap = 32, 8192
  opt = fe.make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, vdtype, dim, "fr_cap_" + route, default=ne.DEFAULT, bounded_cap=cap)
  dt = getattr(torch, vdtype)
  capacity = tg.dev_table(var).capacity()
  old = -np.arange(1, 4 * capacity + 1, dtype=np.int64)
  for part in np.array_split(old, 8):
    var.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=dt))
  census = tg.dev_table(var).slot_census()
  assert census["empty"] == 0 and census["locked"] == 0   # at capacity: a never-seen key can only come in by eviction
  B = census["live"] // 4
  ids = ne.row_keys(B)
  np.random.default_rng(31).shuffle(ids)
  g = np.resize(ne.EDGE, B * dim).reshape(B, dim)   # (27 and 32 are coprime: every column meets every value)
  a1, a2 = fe.new_row_slots(rule)
  full = lambda x: np.full((B, dim), x, np.float32)
  gsum = g   # apply_optimizer takes a key's gradient as it is; the sparse route sums first (0 + g: a -0 becomes +0)
  if route == "apply_sparse":
    with np.errstate(all="ignore"):
      uniq, gsum, _ = oopt.segment_sum_by_key(ids, g)
    assert np.array_equal(uniq, ids)
  wants = fe.oracle_step(rule, gsum, full(ne.DEFAULT), full(a1), full(a2) if fe.n_slots(rule) >= 2 else None)
  it = T(torch, ids)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  tg.write_back(torch, de, route, var, deo, opt.params(1), 1, it, T(torch, g), default_row)
  ex = var.lookup(it, return_exists=True)[1].cpu()
  assert bool(ex.any())
  rows = torch.nonzero(ex).reshape(-1)
  tg.check_rows(torch, deo, opt, var, it, wants, vdtype, "%s %s %s" % (rule, vdtype, route),
                lambda i: "(%s, g %r, new row)" % (rule, float(g[int(rows[i // dim]), i % dim])), rows=rows)


# ---- 3. the combined write-back -------------------------------------------------------------------------------------------------------
COMB_ROWS, COMB_PER_ROW, COMB_KEYS = 128, 4, 160


def _state_bits(torch, deo, opt, var, keys):
  """[p, slot...] of `keys` as int32 bit patterns (float32 rows)."""
  return [f.cpu().contiguous().view(torch.int32) for f in
          [var.lookup(keys)] + [deo.get_slot(var, s).lookup(keys) for s in opt.slots]]


def test_combined_write_back_single_grouped_and_expanded(env, monkeypatch):
  """Three float32 variables — dim 4 with Momentum, 64 with Nesterov, 68 with RMSProp — and one sparse batch each of 128 rows x 4
  ids over 160 keys (ids repeat, half of the keys resident), combiner mean with weights.  Per variable four twins:
    A  apply_combined_gradients_many of its optimizer            (the grouped C call, one member)
    B  apply_combined_gradients                                   (the single C call)
    C  sparse_segment_combine_backprop + apply_sparse             (the expanded entry gradients)
    D  table_ops.apply_planned_combined_many over all three tables, each with its own rule, in ONE call
  A and D end bit-identical to B, parameter and slots; all three were served by grouped calls — counted C calls for A, the call's
  launch count for D; B equals C to rtol = atol = 1e-6 (the bound tests/test_gpu_sparse_train.py has for the four earlier rules)."""
  torch, de = env
  from tests.sparse_helpers import Calls
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan, apply_planned_combined_many
  rng = np.random.default_rng(64)
  members = []
  for rule, dim in zip(fe.RULES, (4, 64, 68)):
    opt = fe.make_opt(de, rule)
    seg = np.repeat(np.arange(COMB_ROWS, dtype=np.int64), COMB_PER_ROW)
    ids = rng.integers(0, COMB_KEYS, size=seg.size).astype(np.int64) * 31 + 5
    assert np.bincount((ids - 5) // 31).max() > 1
    w = (rng.random(seg.size) + 0.5).astype(np.float32)
    G = (rng.standard_normal((COMB_ROWS, dim)) * 0.1).astype(np.float32)
    res_keys = np.arange(0, COMB_KEYS, 2, dtype=np.int64) * 31 + 5
    res_rows = rng.standard_normal((res_keys.size, dim)).astype(np.float32)
    twins = {}
    for tag in "ABCD":
      v = tg.make_var(torch, de, opt, "float32", dim, "fr_comb_" + tag, default=ne.DEFAULT)
      v.upsert(T(torch, res_keys), T(torch, res_rows))
      twins[tag] = (v, de.DynamicEmbeddingOptimizer(opt))
    members.append(dict(rule=rule, dim=dim, opt=opt, seg=T(torch, seg), ids=T(torch, ids), w=T(torch, w), G=T(torch, G), twins=twins,
                        keys=T(torch, np.unique(ids))))

  def lookup(m, tag, many):
    v = m["twins"][tag][0]
    if many:
      return de.embedding_lookup_sparse_many([v], [(m["seg"], m["ids"])], [m["w"]], combiner="mean", return_trainable=True,
                                             num_rows=COMB_ROWS)[0][1]
    return de.embedding_lookup_sparse(v, (m["seg"], m["ids"]), m["w"], combiner="mean", return_trainable=True, num_rows=COMB_ROWS)[1]

  calls = Calls(monkeypatch)
  for m in members:
    m["twins"]["A"][1].apply_combined_gradients_many([(m["G"], lookup(m, "A", True))])
  assert calls["tfra_multi_apply_planned_combined"] == 3 and calls["tfra_table_apply_planned_combined"] == 0
  assert calls["tfra_table_apply_sparse"] == 0 and calls["tfra_table_apply_optimizer"] == 0   # no member dropped out of its group
  for m in members:
    m["twins"]["B"][1].apply_combined_gradients([(m["G"], lookup(m, "B", False))])
  assert calls["tfra_table_apply_planned_combined"] == 3 and calls["tfra_table_apply_sparse"] == 0
  monkeypatch.undo()
  for m in members:
    v, deo = m["twins"]["C"]
    eg = de.device_ops.sparse_segment_combine_backprop(m["G"], m["seg"], m["w"], "mean")
    deo.apply_sparse(v, m["ids"], eg)
  # D: one grouped call, three (rule, storage type) classes.  Launches: 3 in front (row bounds, denominators, entry records), the
  # sums by row chunks (dims 4 and 64: one class, 68: another) = 2, one update launch per rule = 3; no table is at max_capacity
  reqs, ps = [], []
  for m in members:
    v = m["twins"]["D"][0]
    reqs.append((tg.dev_table(v), SparsePlan("cuda:0", m["dim"]).build(m["ids"]), m["G"], m["seg"], m["w"], de.device_ops.COMBINERS["mean"],
                 torch.full((m["dim"],), ne.DEFAULT, device="cuda")))
    ps.append(m["opt"].params(1))
  assert [p.kind for p in ps] == [4, 5, 6]
  assert apply_planned_combined_many(reqs, ps) == 8
  torch.cuda.synchronize()
  for m in members:
    states = {}
    for tag, (v, deo) in m["twins"].items():
      tg.dev_table(v).check_errors()
      assert int(v.size()) == COMB_KEYS // 2 + int((~np.isin(m["keys"].cpu().numpy(), np.arange(0, COMB_KEYS, 2) * 31 + 5)).sum())
      states[tag] = _state_bits(torch, deo, m["opt"], v, m["keys"])
    for tag in "AD":
      for name, a, b in zip(("p",) + tuple(m["opt"].slots), states[tag], states["B"]):
        assert torch.equal(a, b), "%s dim %d: %s of twin %s differs from the single call's" % (m["rule"], m["dim"], name, tag)
    for name, b, c in zip(("p",) + tuple(m["opt"].slots), states["B"], states["C"]):
      np.testing.assert_allclose(b.view(torch.float32).numpy(), c.view(torch.float32).numpy(), rtol=1e-6, atol=1e-6,
                                 err_msg="%s dim %d: %s" % (m["rule"], m["dim"], name))


# ---- 4. five training steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", fe.RULES)
def test_five_training_steps_against_the_sparse_optimizer_oracle(env, monkeypatch, rule):
  """embedding_lookup(..., return_trainable=True, plan_writeback=True) + apply_gradients, dim 8, 64 ids per step over 40 keys (no
  id more than 8 times: the sums are strictly in input order), float32, against SparseOptimizerOracle over CpuTables: the looked-up
  rows, the parameter and every slot, bit for bit after every step.  (A batch this small is normally not worth a plan at lookup
  time: the threshold is lowered, as tests/test_gpu_find_or_insert_planned.py does, so that the plan route is the one that runs.)"""
  torch, de = env
  monkeypatch.setattr(de.variable, "PLAN_AT_LOOKUP_MIN_IDS", 1)
  dim, n_keys, n_ids = 8, 40, 64
  opt = fe.make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, "float32", dim, "fr_steps", default=ne.DEFAULT)
  S = fe.n_slots(rule)
  inits = (ne.DEFAULT,) + fe.new_row_slots(rule)[:S]
  tabs = [oracle.CpuTable(dim) for _ in range(1 + S)]
  ora = oopt.SparseOptimizerOracle(fe.ORACLE_KIND[rule], tabs[0], tabs[1:], fe.HYPER[rule], ne.DEFAULT)
  rng = np.random.default_rng(5 + len(rule))
  all_keys = np.arange(n_keys, dtype=np.int64) * 7919 - 100000
  seen = np.zeros(n_keys, bool)
  for step in range(5):
    while True:
      idx = rng.integers(0, n_keys, size=n_ids)
      if np.bincount(idx, minlength=n_keys).max() <= 8:
        break
    assert np.bincount(idx).max() >= 2
    ids = all_keys[idx]
    emb, tw = de.embedding_lookup(var, T(torch, ids), return_trainable=True, plan_writeback=True)
    assert tw.plan is not None   # the planned write-back: the plan was built at lookup time
    exp = tabs[0].find(ids, np.full(dim, ne.DEFAULT, np.float32))
    ne.assert_bits(torch, emb.reshape(n_ids, dim), torch.from_numpy(exp), "%s step %d: looked-up rows" % (rule, step))
    g = (rng.standard_normal((n_ids, dim)) * 0.5).astype(np.float32)
    deo.apply_gradients([(T(torch, g), tw)])
    ora.apply(ids, g)
    torch.cuda.synchronize()
    tg.dev_table(var).check_errors()
    seen[idx] = True
    keys = all_keys[seen]
    fields = [var.lookup(T(torch, keys))] + [deo.get_slot(var, s).lookup(T(torch, keys)) for s in opt.slots]
    for name, got, t, init in zip(("p",) + tuple(opt.slots), fields, tabs, inits):
      want, ex = t.find(keys, np.full(dim, init, np.float32), return_exists=True)
      assert np.asarray(ex).all()
      ne.assert_bits(torch, got, torch.from_numpy(np.ascontiguousarray(want, np.float32)), "%s step %d: %s" % (rule, step, name))
    assert int(var.size()) == int(seen.sum())


# ---- 5. stochastic rounding -----------------------------------------------------------------------------------------------------------
SR_KEYS, SR_RES, SR_DIM = 128, 64, 68


class StochBatch:
  """n_keys keys of dim `dim` (128 of 68), the first half resident with random rows and slots (storage values), the other half
  never seen (the float default 0.3 and the rule's aux_init); ids repeat 1, 2 and 8 times (`repeats`).  The attributes
  tg.seed_rows reads and the operands of the oracle's step."""

  def __init__(self, torch, rule, vdtype, repeats, n_keys=SR_KEYS, dim=SR_DIM):
    rng = np.random.default_rng(sum(map(ord, rule + vdtype)) + int(repeats))
    S = fe.n_slots(rule)
    a1, a2 = fe.new_row_slots(rule)
    self.n_res = n_res = n_keys // 2
    shape = (n_res, dim)
    self.keys = np.concatenate([ne.row_keys(n_res), -np.arange(1, n_keys - n_res + 1, dtype=np.int64) * 104729])
    st = lambda a: ne.through_storage(torch, a.astype(np.float32), vdtype)
    self.p0 = st(rng.standard_normal(shape) * 0.5)
    if rule == "rmsprop":
      self.s10, self.s20 = st(0.05 + rng.uniform(0, 1, shape)), st(rng.standard_normal(shape) * 0.1)
    else:
      self.s10, self.s20 = st(rng.standard_normal(shape) * 0.5), None
    G = (rng.standard_normal((n_keys, dim)) * 0.3).astype(np.float32)
    idx, occ = fe.batch_over(n_keys, repeats, 99 + int(repeats))
    self.grads = (G[idx] * ne.OCC_SCALE[occ][:, None]).astype(np.float32)
    self.ids = self.keys[idx]
    if repeats:
      uniq, gsum, _ = oopt.segment_sum_by_key(idx, self.grads)
      self.gsum = gsum[np.argsort(uniq)]
    else:
      self.gsum = G
    full = lambda v: np.full((n_keys - n_res, dim), v, np.float32)
    self.in_p = np.concatenate([self.p0, full(ne.DEFAULT)])
    self.in_s1 = np.concatenate([self.s10, full(a1)])
    self.in_s2 = np.concatenate([self.s20, full(a2)]) if S >= 2 else None


@pytest.mark.parametrize("route", ["apply_sparse", "apply_optimizer"])
@pytest.mark.parametrize("vdtype", HALVES)
@pytest.mark.parametrize("rule", ["momentum", "rmsprop"])
def test_stochastic_rounding_of_the_parameter_and_every_slot(env, rule, vdtype, route):
  """A half variable with a seed, one write-back: every stored bit of the parameter (field 0) and of each slot (fields 1, 2) is
  stochastic_rounding_model.stochastic_field of the oracle's float32 result for (SEED, call 0, key, element).  At least 20 % of
  each comparison differs from the nearest-even bits — checked on the CPU, from the model, before the GPU is asked — so that a
  kernel that ignores the option cannot pass."""
  torch, de = env
  c = StochBatch(torch, rule, vdtype, route == "apply_sparse")
  outs = fe.oracle_step(rule, c.gsum, c.in_p, c.in_s1, c.in_s2)
  outs = [o for o in outs if o is not None]
  bits = [srm.stochastic_field(o, vdtype, SEED, 0, c.keys, f) for f, o in enumerate(outs)]
  for f, (b, o) in enumerate(zip(bits, outs)):
    frac = srm.differing_fraction(b, o, vdtype)
    print("%s %s %s field %d: %.1f %% of %d elements differ from nearest even" % (rule, vdtype, route, f, 100 * frac, b.size))
    assert frac >= 0.20, "field %d: only %.1f %% of the elements tell the rounding modes apart" % (f, 100 * frac)
  opt = fe.make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, vdtype, SR_DIM, "fr_sr_" + route, default=ne.DEFAULT)
  tg.seed_rows(torch, de, deo, opt, var, c)
  var.set_stochastic_rounding(SEED)
  default_row = torch.full((SR_DIM,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  tg.write_back(torch, de, route, var, deo, opt.params(1), 1, T(torch, c.ids), T(torch, c.grads), default_row)
  keys = T(torch, c.keys)
  fields = [("p", var.lookup(keys))] + [(n, deo.get_slot(var, n).lookup(keys)) for n in opt.slots]
  for (name, got), b in zip(fields, bits):
    ne.assert_bits(torch, got.cpu(), srm.as_tensor(torch, b, vdtype).reshape(got.shape), "%s %s %s: %s" % (rule, vdtype, route, name))
  assert int(var.size()) == SR_KEYS


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def _refusal_cases(de):
  """(what, aux_fields of the table, the refused parameters)"""
  from tfra_amd import _capi
  p7 = de.optimizers.RMSProp(0.01, 0.9, 0.5, 1e-10, fused=True).params(1)
  p7.kind = 7
  return [("kind 7", 2, p7),
          ("Momentum on a table without slot fields", 0, de.optimizers.Momentum(0.05, 0.9, fused=True).params(1)),
          ("RMSProp on a table with one slot field", 1, de.optimizers.RMSProp(0.01, 0.9, 0.5, 1e-10, fused=True).params(1))]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_refusals_leave_the_table_as_it_was(env, case):
  """Kind 7, Momentum on aux_fields = 0 and RMSProp on aux_fields = 1: TFRA_ERR_INVALID through apply_optimizer, apply_planned and
  the grouped combined call, each of which leaves the table's size and an exported row unchanged."""
  torch, de = env
  from tfra_amd._capi import TfraError
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan, apply_planned_combined_many
  what, aux, p = _refusal_cases(de)[case]
  dim = 8
  tg._serial[0] += 1
  var = de.Variable(dim=dim, name="fr_refuse_%d_%d" % (case, tg._serial[0]), initializer=ne.DEFAULT, aux_fields=aux,
                    aux_init=(0.25, 0.0, 0.0, 0.0))
  t = tg.dev_table(var)
  keys = T(torch, ne.row_keys(16))
  rows = torch.arange(16 * dim, dtype=torch.float32, device="cuda").reshape(16, dim) / 8
  var.upsert(keys, rows)

  def snapshot():
    k, v = var.export()
    o = torch.argsort(k)
    return int(var.size()), k[o].cpu(), v[o].cpu().contiguous().view(torch.int32)

  before = snapshot()
  ids = torch.cat([keys[:8], T(torch, np.array([-5, -6, -5], np.int64))])   # resident and never-seen ids, one repeated
  grads = torch.ones((ids.numel(), dim), device="cuda")
  default_row = torch.full((dim,), ne.DEFAULT, device="cuda")
  uniq = torch.unique(ids)
  seg = torch.arange(ids.numel(), dtype=torch.int64, device="cuda")
  routes = {
      "apply_optimizer": lambda: t.apply_optimizer(p, uniq, grads[:uniq.numel()], default_row),
      "apply_planned": lambda: t.apply_planned(p, SparsePlan("cuda:0", dim).build(ids), grads, default_row),
      "grouped": lambda: apply_planned_combined_many([(t, SparsePlan("cuda:0", dim).build(ids), grads, seg, None, 0, default_row)], p),
  }
  for route, call in routes.items():
    with pytest.raises(TfraError) as e:
      call()
    assert e.value.code == -1, "%s through %s: %s" % (what, route, e.value)   # TFRA_ERR_INVALID
    torch.cuda.synchronize()
    t.check_errors()
    after = snapshot()
    assert after[0] == before[0] == 16 and torch.equal(after[1], before[1]) and torch.equal(after[2], before[2]), (what, route)


# ---- 7. existing behaviour ----------------------------------------------------------------------------------------------------------------
def test_plan_needs_the_fused_form(env):
  """The default Momentum stays on the Generic route, which has no plan; with fused=True `plan` returns one that apply_sparse
  consumes — and the rows are the oracle's."""
  torch, de = env
  dim = 8
  ids = T(torch, np.array([3, 4, 4, 5, 3, 3], np.int64))
  g = (np.random.default_rng(7).standard_normal((6, dim)) * 0.5).astype(np.float32)
  generic = de.optimizers.Momentum(0.05, 0.9)
  var = tg.make_var(torch, de, generic, "float32", dim, "fr_plan", default=ne.DEFAULT)
  with pytest.raises(ValueError, match="has no plan"):
    de.DynamicEmbeddingOptimizer(generic).plan(var, ids)
  opt = de.optimizers.Momentum(0.05, 0.9, fused=True)
  deo = de.DynamicEmbeddingOptimizer(opt)
  plan = deo.plan(var, ids)
  deo.apply_sparse(var, ids, T(torch, g), plan=plan)
  torch.cuda.synchronize()
  tg.dev_table(var).check_errors()
  uniq, gsum, _ = oopt.segment_sum_by_key(ids.cpu().numpy(), g)
  want_p, want_a = oopt.momentum(np.full((3, dim), ne.DEFAULT, np.float32), np.zeros((3, dim), np.float32), gsum, 0.05, 0.9)
  ne.assert_bits(torch, var.lookup(T(torch, uniq)), torch.from_numpy(want_p), "planned Momentum: p")
  ne.assert_bits(torch, deo.get_slot(var, "momentum").lookup(T(torch, uniq)), torch.from_numpy(want_a), "planned Momentum: accum")
  # ... and the variable continues through the Generic form: same slots, same rows
  de.DynamicEmbeddingOptimizer(generic).apply_sparse(var, ids, T(torch, g))
  want_p2, want_a2 = oopt.momentum(want_p, want_a, gsum, 0.05, 0.9)
  np.testing.assert_allclose(var.lookup(T(torch, uniq)).cpu().numpy(), want_p2, rtol=1e-6, atol=1e-6)
  np.testing.assert_allclose(deo.get_slot(var, "momentum").lookup(T(torch, uniq)).cpu().numpy(), want_a2, rtol=1e-6, atol=1e-6)


# ---- 8. the other routes of DynamicEmbeddingOptimizer ---------------------------------------------------------------------------------
W_KEYS, W_DIM = 48, 8


@pytest.mark.parametrize("route", ["exact_order", "two_shards", "multi_table_step"])
@pytest.mark.parametrize("rule", fe.RULES)
def test_wrapper_routes_with_the_fused_kinds(env, rule, route):
  """The branches of DynamicEmbeddingOptimizer that key on `opt.kind is None`, with the new kinds: exact_order=True (unique +
  segment_sum + apply_optimizer), a variable of two shards (reduce by key, then apply_optimizer per shard) and
  MultiTablePrefetchStep over two variables.  float32, dim 8, 48 keys (24 resident, 24 never seen), ids repeating 1, 2 and 8 times:
  the parameter and every slot are the oracle's one step, bit for bit."""
  torch, de = env
  opt = fe.make_opt(de, rule)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  c = StochBatch(torch, rule, "float32", True, n_keys=W_KEYS, dim=W_DIM)
  wants = fe.oracle_step(rule, c.gsum, c.in_p, c.in_s1, c.in_s2)
  deo = de.DynamicEmbeddingOptimizer(opt, exact_order=(route == "exact_order"))
  tg._serial[0] += 1
  n_vars = 2 if route == "multi_table_step" else 1
  devices = ["cuda:0"] * (2 if route == "two_shards" else 1)
  vs = [de.Variable(dim=W_DIM, devices=devices, name="fr_w_%s_%s_%d_%d" % (route, rule, i, tg._serial[0]), initializer=ne.DEFAULT, **kw)
        for i in range(n_vars)]
  for v in vs:
    tg.seed_rows(torch, de, deo, opt, v, c)
  ids, grads = T(torch, c.ids), T(torch, c.grads)
  if route == "multi_table_step":
    ms = de.MultiTablePrefetchStep(vs, deo).prime([ids, ids])
    rows = ms.step([grads, grads], None)
    ms.synchronize()
    for r in rows:   # the step's lookup half ran before its write-back
      ne.assert_bits(torch, r, torch.from_numpy(c.in_p[_index_of(c.keys, c.ids)]), "%s: rows of the step's lookup" % rule)
  else:
    deo.apply_sparse(vs[0], ids, grads)
  torch.cuda.synchronize()
  for v in vs:
    for t in v.tables:
      t._table.check_errors()
    tg.check_rows(torch, deo, opt, v, T(torch, c.keys), wants, "float32", "%s %s" % (rule, route), None)
    assert int(v.size()) == W_KEYS


def _index_of(keys, ids):
  """The position in `keys` of every id."""
  order = np.argsort(keys)
  return order[np.searchsorted(keys[order], ids)]


def test_a_tiered_init_on_lookup_variable_trains_like_its_roomy_twin(env):
  """tests/test_gpu_tier_variable.py at its shape with RMSProp(fused=True): init_on_lookup variables, one over a tier (an HBM cache
  of 1335 slots over a lower table) and one over a roomy table, 12 steps of embedding_lookup + apply_gradients over 3000 ids.  The
  write-backs land in the cache table, rows move between the tiers as they are: embedding and both slots of every key ever seen
  are bit for bit the twin's."""
  torch, de = env
  from tests import test_gpu_tier_variable as tv
  cfg = de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=tv.CAP, max_capacity=tv.CAP, evict_strategy=de.HkvEvictStrategy.LRU),
                                 max_batch=1024)

  def make(kind, creator):
    opt = fe.make_opt(de, "rmsprop")
    var = de.Variable(dim=tv.DIM, name="fr_tier_" + kind, initializer=tv._Init(torch), kv_creator=creator, init_on_lookup=True,
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    return var, de.DynamicEmbeddingOptimizer(opt)

  pair = [make("tiered", de.TieredHashTableCreator(cfg)), make("twin", de.CuckooHashTableCreator())]
  seen = tv._train(env, pair, *tv._batches(29))
  t = pair[0][0]._tables[0]
  t._table.check_errors()
  t._lower.check_errors()
  s = t._tier.stats()
  assert seen.numel() > tv.CAP and s["demoted"] > 0 and s["lower_hits"] > 100   # keys went down and came up again
  a, b = (tv._whole_rows(torch, v, seen).cpu().view(torch.int32) for v in (pair[0][0], pair[1][0]))
  assert a.shape == b.shape == (seen.numel(), tv.DIM * 3)
  bad = (a != b).any(1)
  assert not bool(bad.any()), "%d of %d keys differ from the twin (embedding or slots)" % (int(bad.sum()), seen.numel())
  ms = b.view(torch.float32)[:, tv.DIM:2 * tv.DIM]
  assert bool((ms != fe.INITIAL_RMS).any()) and bool((ms >= 0).all())   # the rule ran: ms moved from its initial value


@pytest.mark.parametrize("rule", fe.RULES)
def test_apply_sparse_beyond_2_18_ids(env, rule):
  """tfra_table_apply_sparse's path for more than 2^18 ids (chunk-wise sums, then every key once) with the new kinds: 300 000
  distinct never-seen ids of dim 4, each once, so that no sum's association is in play — the rows are the oracle's new-row step on
  0 + g, bit for bit."""
  torch, de = env
  n, dim = 300_000, 4
  assert n > (1 << 18)
  opt = fe.make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, "float32", dim, "fr_big", default=ne.DEFAULT)
  rng = np.random.default_rng(18)
  ids = ne.row_keys(n)
  rng.shuffle(ids)
  g = (rng.standard_normal((n, dim)) * 0.3).astype(np.float32)
  a1, a2 = fe.new_row_slots(rule)
  full = lambda x: np.full((n, dim), x, np.float32)
  wants = fe.oracle_step(rule, (np.float32(0) + g).astype(np.float32), full(ne.DEFAULT), full(a1), full(a2) if fe.n_slots(rule) >= 2 else None)
  it = T(torch, ids)
  deo.apply_sparse(var, it, T(torch, g))
  torch.cuda.synchronize()
  tg.dev_table(var).check_errors()
  tg.check_rows(torch, deo, opt, var, it, wants, "float32", "%s, %d ids" % (rule, n), None)
  assert int(var.size()) == n
