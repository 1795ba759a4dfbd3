"""GPU: TFRA_OPTION_STOCHASTIC_ROUNDING — what the fused optimizer write-backs store in float16 / bfloat16 rows with the option on,
against the NumPy model of tests/stochastic_rounding_model.py (checked without a GPU in tests/test_stochastic_rounding_model.py),
through every entry point that reaches the three kernels with a rounding axis: apply_kernel / apply_evict_kernel
(tfra_table_apply_optimizer) and apply_csr_body (the sparse, planned, combined, grouped and step write-backs).

Every comparison is with the model and has no tolerance (numeric_edges.assert_bits: equal bits, or a NaN where a NaN is expected),
and in every comparison at least 20 % of the compared elements differ from the nearest-even bits (`check`), so that a kernel that
ignores the option cannot pass.  The drivers of the routes are those of tests/test_gpu_numeric_edges.py."""
import numpy as np
import pytest

from tests import numeric_edges as ne
from tests import stochastic_rounding_model as srm
from tests import test_gpu_numeric_edges as tg

pytestmark = pytest.mark.gpu

HALVES = ["float16", "bfloat16"]
SEED = 0x5EED0000C0FFEE11
SEED_HIGH = 0xF00DF00DF00DF00D   # the top bit set: the option's value is an int64
T = tg.T


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def check(torch, got, want_bits, x, vdtype, what, context=None):
  """got (a tensor of the storage type) against the model's bits of the float32 results x, and the 20 % rule."""
  ne.assert_bits(torch, got.cpu(), srm.as_tensor(torch, want_bits, vdtype).reshape(got.shape), what, context)
  frac = srm.differing_fraction(want_bits, x, vdtype)
  print("%s: %.1f %% of %d elements differ from nearest even" % (what, 100 * frac, np.asarray(want_bits).size))
  assert frac >= 0.20, "%s: only %.1f %% of the elements tell the rounding modes apart" % (what, 100 * frac)


# ---- 1. storage: the SGD carrier through every route ----------------------------------------------------------------------------
def carrier(torch, de, vdtype, dim, tag, seed):
  """The SGD carrier of numeric_edges (lr 1, every key once, gradient -x, resident rows of 0) over the model's storage set packed
  into rows of `dim` -> var, optimizer, keys (NumPy, tensor), grads, the oracle's float32 result [n, dim]."""
  x = ne.pack_rows(srm.storage_values(), dim)
  res = ne.pack_rows(srm.sgd_carrier_result(), dim)
  opt = de.optimizers.SGD(1.0)
  var = tg.make_var(torch, de, opt, vdtype, dim, "sr_" + tag)
  keys_np = ne.row_keys(x.shape[0])
  keys = T(torch, keys_np)
  var.upsert(keys, torch.zeros((x.shape[0], dim), dtype=getattr(torch, vdtype), device="cuda"))   # (not a fused write-back: no call)
  if seed is not None:
    var.set_stochastic_rounding(seed)
  return var, opt, keys_np, keys, T(torch, -x), res


def carrier_context(dim):
  x = ne.pack_rows(srm.storage_values(), dim).reshape(-1)
  return lambda i: "x = %r / %08x, row %d column %d" % (float(x[i]), int(x[i:i + 1].view(np.uint32)[0]), i // dim, i % dim)


# every width on the unique-key path (6: not a multiple of 4, the element index crosses the granules) and on the one-call path;
# the planned, combined and step forms launch the same apply_csr_kernel through apply_planned_impl: two widths each, one for the step.
# 4: one granule; 8: two; 64: one full trip; 68: a second trip with 15 idle lanes; 256: four trips.
STORAGE_ROUTES = ([("apply_optimizer", d) for d in (4, 6, 8, 64, 68, 256)] + [("apply_sparse", d) for d in (4, 8, 64, 68, 256)] +
                  [("apply_planned", 8), ("apply_planned", 68), ("combined", 4), ("combined", 256), ("prefetch_step", 68)])


@pytest.mark.parametrize("vdtype", HALVES)
@pytest.mark.parametrize("route,dim", STORAGE_ROUTES)
def test_storage_rounding_through_the_write_back(env, route, dim, vdtype):
  """Every float32 value at which a rounding to the storage type can go wrong (every bfloat16 tie pattern, every float16 tie with
  its neighbours, the float16 subnormal range, the top interval, infinities, NaNs) and random low bits, carried through `route`
  unchanged: the row holds the model's bits for (SEED, call 0, its key, its element)."""
  torch, de = env
  var, opt, keys_np, keys, grads, res = carrier(torch, de, vdtype, dim, route, SEED)
  deo = de.DynamicEmbeddingOptimizer(opt)
  rows = tg.write_back(torch, de, route, var, deo, opt.params(1), 1, keys, grads, torch.zeros(dim, device="cuda"))
  if rows is not None:   # the step's lookup half ran before its write-back
    assert not bool(rows.view(torch.int16).any())
  want = srm.stochastic_field(res, vdtype, SEED, 0, keys_np, 0)
  check(torch, var.lookup(keys), want, res, vdtype, "%s %s dim %d" % (route, vdtype, dim), carrier_context(dim))
  assert int(var.size()) == keys.numel()


@pytest.mark.parametrize("vdtype", HALVES)
def test_storage_rounding_through_the_grouped_combined_write_back(env, monkeypatch, vdtype):
  """apply_combined_gradients_many over two variables, one with the option on and one without: ONE grouped C call, in which the
  member that rounds stochastically is served by the single call's launches; it holds the model's bits, and the other member
  ends bit-identical to a twin that is written back alone (and holds the nearest-even bits)."""
  torch, de = env
  from tests.sparse_helpers import Calls
  dim = 64
  on, opt, keys_np, keys, grads, res = carrier(torch, de, vdtype, dim, "many_on", SEED)
  off = carrier(torch, de, vdtype, dim, "many_off", None)[0]
  twin = carrier(torch, de, vdtype, dim, "many_twin", None)[0]
  n = keys.numel()
  sp = (torch.arange(n, dtype=torch.int64, device="cuda"), keys)   # one entry per output row, combiner sum: the entry's gradient is grad_out's row
  deo, deo_twin = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  tws = [tw for _, tw in de.embedding_lookup_sparse_many([on, off], [sp, sp], None, combiner="sum", return_trainable=True, num_rows=n)]
  calls = Calls(monkeypatch)
  deo.apply_combined_gradients_many([(grads, tws[0]), (grads, tws[1])])
  assert calls["tfra_multi_apply_planned_combined"] == 1 and calls["tfra_table_apply_planned_combined"] == 0
  monkeypatch.undo()
  _, tw = de.embedding_lookup_sparse(twin, sp, None, combiner="sum", return_trainable=True, num_rows=n)
  deo_twin.apply_combined_gradients([(grads, tw)])
  torch.cuda.synchronize()
  for v in (on, off, twin):
    tg.dev_table(v).check_errors()
  check(torch, on.lookup(keys), srm.stochastic_field(res, vdtype, SEED, 0, keys_np, 0), res, vdtype, "grouped, member on, %s" % vdtype,
        carrier_context(dim))
  got_off = off.lookup(keys).cpu()
  assert torch.equal(got_off.view(torch.int16), twin.lookup(keys).cpu().view(torch.int16))
  ne.assert_bits(torch, got_off, ne.to_storage(torch, res, vdtype), "grouped, member off, %s" % vdtype, carrier_context(dim))


# ---- 2. the rules: the parameter and every slot ------------------------------------------------------------------------------------
N_KEYS, N_RES, R_DIM = 512, 256, 8
# numeric_edges' hyper-parameters, but for Adam: with lr = 1e-3 and beta2 = 0.999 a resident parameter and v move by less than half
# a storage ulp per step — the case the mode exists for — so that few elements would tell the two roundings apart, and with
# eps = 1e-8 the first step of a new row is +-lr whatever the gradient.  These move every field by several ulps.
HYPER = dict(ne.HYPER, adam=dict(lr=0.05, beta1=0.9, beta2=0.95, eps=0.05))


def make_opt(de, rule):
  if rule == "adam":
    h = HYPER["adam"]
    return de.optimizers.Adam(h["lr"], h["beta1"], h["beta2"], h["eps"])
  return tg.make_opt(de, rule)


class RuleBatch:
  """512 keys of dim 8, the first 256 resident with random rows and slots (storage values), the other 256 never seen (they start
  from the float default 0.3 and the rule's initial slot values); ids repeat 1, 2 and 8 times (`repeats`), the expected sums are
  segment_sum_by_key's.  The attributes tg.seed_rows reads, and the operands of the oracle's step."""

  def __init__(self, torch, rule, vdtype, repeats):
    rng = np.random.default_rng(sum(map(ord, rule + vdtype)) + int(repeats))
    S = ne.n_slots(rule)
    a1, a2 = ne.new_row_slots(rule)
    shape = (N_RES, R_DIM)
    self.n_res = N_RES
    self.keys = np.concatenate([ne.row_keys(N_RES), -np.arange(1, N_KEYS - N_RES + 1, dtype=np.int64) * 104729])
    st = lambda a: ne.through_storage(torch, a.astype(np.float32), vdtype)
    self.p0 = st(rng.standard_normal(shape) * 0.5)
    if rule == "adam":
      self.s10, self.s20 = st(rng.standard_normal(shape) * 0.1), st(rng.uniform(1e-4, 1e-1, shape))
    elif rule == "ftrl":
      self.s10, self.s20 = st(0.1 + rng.uniform(0, 2, shape)), st(rng.standard_normal(shape) * 0.5)
    else:
      self.s10, self.s20 = (st(0.1 + rng.uniform(0, 2, shape)) if S else None), None
    G = (rng.standard_normal((N_KEYS, R_DIM)) * 0.3).astype(np.float32)
    idx = np.repeat(np.arange(N_KEYS), ne.repeat_counts(N_KEYS, repeats))
    rng.shuffle(idx)
    order = np.argsort(idx, kind="stable")
    occ = np.empty(idx.size, dtype=np.int64)
    occ[order] = np.arange(idx.size) - np.searchsorted(idx[order], idx[order], side="left")
    self.grads = (G[idx] * ne.OCC_SCALE[occ][:, None]).astype(np.float32)
    self.ids = self.keys[idx]
    if repeats:
      uniq, gsum, _ = oopt_sums(idx, self.grads)
      self.gsum = gsum[np.argsort(uniq)]
    else:
      self.gsum = G
    full = lambda v: np.full((N_KEYS - N_RES, R_DIM), v, np.float32)
    self.in_p = np.concatenate([self.p0, full(ne.DEFAULT)])
    self.in_s1 = np.concatenate([self.s10, full(a1)]) if S >= 1 else None
    self.in_s2 = np.concatenate([self.s20, full(a2)]) if S >= 2 else None


def oopt_sums(idx, grads):
  from oracle import optimizers as oopt
  return oopt.segment_sum_by_key(idx, grads)


def check_fields(torch, deo, opt, var, keys, keys_np, bits, outs, vdtype, what, rows=None):
  """The parameter and every slot field of `keys` against the model (rows: only these rows)."""
  fields = [("p", var.lookup(keys))] + [(n, deo.get_slot(var, n).lookup(keys)) for n in opt.slots]
  sel = (lambda a: a) if rows is None else (lambda a: a[rows])
  for (name, got), b, o in zip(fields, bits, outs):
    got = got.cpu()
    check(torch, got if rows is None else got[torch.from_numpy(rows)], sel(b), sel(o), vdtype, "%s: %s" % (what, name))


@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse"])
@pytest.mark.parametrize("vdtype", HALVES)
@pytest.mark.parametrize("rule,step", [r for r in ne.RULES if r[0] != "sgd"])
def test_rules_round_the_parameter_and_every_slot(env, rule, step, vdtype, route):
  """Adam (steps 1 and 1000), Adagrad with and without epsilon, FTRL: one write-back, the oracle's rule and then the model's
  rounding with field 0 for the parameter and 1, 2 for the slots.  apply_sparse: ids repeat 1, 2 and 8 times."""
  torch, de = env
  opt = make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  c = RuleBatch(torch, rule, vdtype, route == "apply_sparse")
  var = tg.make_var(torch, de, opt, vdtype, R_DIM, "sr_rule_" + route, default=ne.DEFAULT)
  tg.seed_rows(torch, de, deo, opt, var, c)
  var.set_stochastic_rounding(SEED)
  default_row = torch.full((R_DIM,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  tg.write_back(torch, de, route, var, deo, opt.params(step), step, T(torch, c.ids), T(torch, c.grads), default_row)
  bits, outs = srm.stochastic_step(rule, step, c.gsum, c.in_p, c.in_s1, c.in_s2, vdtype, SEED, 0, c.keys, HYPER[rule])
  check_fields(torch, deo, opt, var, T(torch, c.keys), c.keys, bits, outs, vdtype, "%s step %d %s %s" % (rule, step, vdtype, route))
  assert int(var.size()) == N_KEYS


@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse"])
@pytest.mark.parametrize("vdtype", HALVES)
@pytest.mark.parametrize("rule", ["adam", "adagrad", "adagrad_v2", "ftrl"])
def test_rules_on_a_bounded_table_at_capacity(env, rule, vdtype, route):
  """Phase 2 writes (apply_evict_kernel behind apply_optimizer, PHASE2 of apply_csr_body behind apply_sparse): an LRU table filled
  to its capacity, then the rule's batch, all of whose keys are never seen there.  Every batch key that is present afterwards
  holds the new-row result with the model's rounding."""
  torch, de = env
  cap = 8192
  opt = make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, vdtype, R_DIM, "sr_cap_" + route, default=ne.DEFAULT, bounded_cap=cap)
  dt = getattr(torch, vdtype)
  capacity = tg.dev_table(var).capacity()
  old = -np.arange(1, 4 * capacity + 1, dtype=np.int64) - (1 << 40)
  for part in np.array_split(old, 8):
    var.upsert(T(torch, part), torch.full((part.size, R_DIM), 0.5, device="cuda", dtype=dt))
  census = tg.dev_table(var).slot_census()
  assert census["empty"] == 0 and census["locked"] == 0   # at capacity: a never-seen key can only come in by eviction
  c = RuleBatch(torch, rule, vdtype, route == "apply_sparse")
  a1, a2 = ne.new_row_slots(rule)
  full = lambda v: np.full((N_KEYS, R_DIM), v, np.float32)
  var.set_stochastic_rounding(SEED)
  default_row = torch.full((R_DIM,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  tg.write_back(torch, de, route, var, deo, opt.params(1), 1, T(torch, c.ids), T(torch, c.grads), default_row)
  S = ne.n_slots(rule)
  bits, outs = srm.stochastic_step(rule, 1, c.gsum, full(ne.DEFAULT), full(a1) if S >= 1 else None, full(a2) if S >= 2 else None,
                                   vdtype, SEED, 0, c.keys, HYPER[rule])
  kt = T(torch, c.keys)
  ex = var.lookup(kt, return_exists=True)[1].cpu().numpy()
  assert ex.sum() >= N_KEYS // 2
  check_fields(torch, deo, opt, var, kt, c.keys, bits, outs, vdtype, "at capacity, %s %s %s" % (rule, vdtype, route), rows=np.nonzero(ex)[0])


# ---- 3. the call index ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", HALVES)
def test_call_index_advances_per_write_back_and_restarts_with_the_seed(env, vdtype):
  torch, de = env
  dim, n = 8, 1024
  x = (np.random.default_rng(5).standard_normal((n, dim)) * 3).astype(np.float32)
  k1, k2 = ne.row_keys(n), -ne.row_keys(n) - 1
  opt = de.optimizers.SGD(1.0)
  p = opt.params(1)
  var = tg.make_var(torch, de, opt, vdtype, dim, "sr_call")
  t = tg.dev_table(var)
  zero, g = torch.zeros(dim, device="cuda"), T(torch, -x)
  model = lambda keys, call: srm.stochastic_field(x, vdtype, SEED_HIGH, call, keys, 0)
  bits = lambda keys: var.lookup(T(torch, keys)).cpu().view(torch.int16).numpy().view(np.uint16)
  var.set_stochastic_rounding(SEED_HIGH)
  t.apply_sparse(p, T(torch, k1), g, zero)
  t.apply_sparse(p, T(torch, k2), g, zero)
  got1, got2 = bits(k1), bits(k2)
  check(torch, var.lookup(T(torch, k1)), model(k1, 0), x, vdtype, "first write-back, call 0")
  check(torch, var.lookup(T(torch, k2)), model(k2, 1), x, vdtype, "second write-back, call 1")
  assert np.mean(got1 != model(k1, 1)) > 0.2 and np.mean(got2 != model(k2, 0)) > 0.2   # and not the other way round
  # clear + the seed again: the first result comes back; the unique-key entry point stores the same bits for the same (seed, call, key)
  for route in ("apply_sparse", "apply_optimizer"):
    var.clear()
    var.set_stochastic_rounding(SEED_HIGH)
    getattr(t, route)(p, T(torch, k1), g, zero)
    assert np.array_equal(bits(k1), got1), route
  t.check_errors()


# ---- 4. off -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("had_it", [False, True])
@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse"])
@pytest.mark.parametrize("vdtype", HALVES)
def test_off_is_nearest_even(env, vdtype, route, had_it):
  """With the option at 0 (set back after a seed, or never set) the rows hold the nearest-even bits of numeric_edges."""
  torch, de = env
  dim = 8
  var, opt, keys_np, keys, grads, res = carrier(torch, de, vdtype, dim, "off_" + route, SEED if had_it else None)
  if had_it:
    var.set_stochastic_rounding(None)
  tg.write_back(torch, de, route, var, de.DynamicEmbeddingOptimizer(opt), opt.params(1), 1, keys, grads, torch.zeros(dim, device="cuda"))
  ne.assert_bits(torch, var.lookup(keys), ne.to_storage(torch, res, vdtype), "off, %s %s" % (route, vdtype), carrier_context(dim))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_a_float32_table_refuses_a_seed(env):
  torch, de = env
  from tfra_amd import _capi
  var = tg.make_var(torch, de, de.optimizers.SGD(1.0), "float32", 8, "sr_f32")
  with pytest.raises(_capi.TfraError, match="set_option") as e:
    var.set_stochastic_rounding(SEED)
  assert e.value.code == _capi.ERR_UNSUPPORTED
  var.set_stochastic_rounding(None)   # off is fine on every table
  with pytest.raises(_capi.TfraError):
    de.Variable(dim=8, name="sr_f32_ctor", stochastic_rounding=SEED)


@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse", "apply_planned", "combined", "prefetch_step"])
def test_a_capture_safe_table_refuses_the_write_back(env, route):
  """Both options on: TFRA_ERR_UNSUPPORTED naming the function, nothing enqueued, the table unchanged."""
  torch, de = env
  from tfra_amd import _capi
  dim, n = 8, 256
  opt = de.optimizers.SGD(1.0)
  var = tg.make_var(torch, de, opt, "bfloat16", dim, "sr_cs_" + route)
  keys = T(torch, ne.row_keys(n))
  rows = torch.full((n, dim), 0.3, dtype=torch.bfloat16, device="cuda")
  var.upsert(keys[:n // 2], rows[:n // 2])
  var.set_stochastic_rounding(SEED)
  t = tg.dev_table(var)
  deo = de.DynamicEmbeddingOptimizer(opt)
  g = torch.ones((n, dim), device="cuda")
  name = {"combined": "apply_planned_combined", "prefetch_step": "step_prefetch"}.get(route, route)
  t.set_capture_safe(True)
  try:
    with pytest.raises(_capi.TfraError, match=name + ": ") as e:
      tg.write_back(torch, de, route, var, deo, opt.params(1), 1, keys, g, torch.zeros(dim, device="cuda"))
    assert e.value.code == _capi.ERR_UNSUPPORTED
  finally:
    t.set_capture_safe(False)
  torch.cuda.synchronize()
  assert int(var.size()) == n // 2
  got, ex = var.lookup(keys, return_exists=True)
  assert torch.equal(ex.cpu(), torch.arange(n) < n // 2) and torch.equal(got[:n // 2].cpu(), rows[:n // 2].cpu())
  with pytest.raises(ValueError, match="stochastic_rounding"):
    de.CapturedTrainStep(var, deo, n)


# ---- 6. a tiered variable ------------------------------------------------------------------------------------------------------------------
def test_a_tiered_variable_rounds_like_its_roomy_twin(env):
  """tests/test_gpu_tier_variable.py at its shape, bfloat16 rows, the option on through the constructor: the write-backs land in the
  cache table, rows move between the tiers as they are, and embedding and slots of every key ever seen are bit for bit those of a
  roomy twin with the same seed — and not those of a twin that rounds to nearest even."""
  torch, de = env
  from tests import test_gpu_tier_variable as tv
  cfg = de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=tv.CAP, max_capacity=tv.CAP, evict_strategy=de.HkvEvictStrategy.LRU),
                                 max_batch=1024)

  def make(kind, creator, seed):
    opt = de.optimizers.Adam(1e-2)
    var = de.Variable(dim=tv.DIM, name="sr_tier_" + kind, value_dtype=torch.bfloat16, initializer=tv._Init(torch), kv_creator=creator,
                      init_on_lookup=True, stochastic_rounding=seed, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    return var, de.DynamicEmbeddingOptimizer(opt)

  pair = [make("tiered", de.TieredHashTableCreator(cfg), SEED), make("twin", de.CuckooHashTableCreator(), SEED)]
  nearest = [make("nearest", de.CuckooHashTableCreator(), None)]
  assert pair[0][0].stochastic_rounding == SEED and nearest[0][0].stochastic_rounding is None
  seen = tv._train(env, pair, *tv._batches(23))
  tv._train(env, nearest, *tv._batches(23))
  t = pair[0][0]._tables[0]
  t._table.check_errors()
  t._lower.check_errors()
  s = t._tier.stats()
  assert seen.numel() > tv.CAP and s["demoted"] > 0 and s["lower_hits"] > 100   # keys went down and came up again
  a, b, c = (tv._whole_rows(torch, v, seen).cpu().view(torch.int16) for v in (pair[0][0], pair[1][0], nearest[0][0]))
  assert a.shape == b.shape == c.shape == (seen.numel(), tv.DIM * 3)
  bad = (a != b).any(1)
  assert not bool(bad.any()), "%d of %d keys differ from the twin (embedding or slots)" % (int(bad.sum()), seen.numel())
  assert float((a != c).float().mean()) >= 0.20
