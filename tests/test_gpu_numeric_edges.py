"""GPU: the fused optimizer rules (apply_one<KIND>) and the half-row conversions (load_stored / to_stored and their four-element
forms, csrc/tfra_optim_device.h) pinned BIT FOR BIT — the rules to oracle/optimizers.py on a grid of numeric edges, the conversions
to torch's, exhaustively at the tie points — through every write-back that instantiates them: apply_kernel / apply_evict_kernel
(tfra_table_apply_optimizer) and apply_csr_body (the sparse, planned, combined, grouped and step write-backs).

The comparison rule, everywhere (tests/numeric_edges.py: assert_bits): where the expected value is not a NaN the stored bits are
equal; where it is a NaN the result is a NaN, payload free.  No tolerances.  The inputs and the references are built in
tests/numeric_edges.py and checked against each other without a GPU in tests/test_numeric_edges_model.py.

Why equality is the right bound: apply_one is IEEE add, multiply, divide and sqrt in a fixed order, compiled with
-ffp-contract=off, float32 subnormals kept; the oracle is one NumPy float32 operation per call in the same order.  (FTRL with a
general lr_power goes through powf and stays where it was, at 5e-6 in test_k13_fused_optimizer_matches_reference_sequence.)"""
import numpy as np
import pytest

from tests import numeric_edges as ne

pytestmark = pytest.mark.gpu

HALVES = ["float16", "bfloat16"]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_serial = [0]


def make_opt(de, rule):
  h = ne.HYPER[rule]
  if rule == "sgd":
    return de.optimizers.SGD(h["lr"])
  if rule == "adam":
    return de.optimizers.Adam(h["lr"], h["beta1"], h["beta2"], h["eps"])
  if rule in ("adagrad", "adagrad_v2"):
    return de.optimizers.Adagrad(h["lr"], ne.INIT_ACC, h["eps"])
  return de.optimizers.Ftrl(h["lr"], h["lr_power"], ne.INIT_ACC, h["l1"], h["l2"])


def make_var(torch, de, opt, vdtype, dim, tag, default=0.0, bounded_cap=0):
  """A one-shard variable with the optimizer's slots; bounded_cap: a bounded LRU table of that many slots."""
  _serial[0] += 1
  name = "ne_%s_%s_%d_%d" % (tag, vdtype, dim, _serial[0])
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  dt = getattr(torch, vdtype)
  if not bounded_cap:
    return de.Variable(dim=dim, name=name, value_dtype=dt, initializer=default, **kw)
  return de.get_variable(name, key_dtype=torch.int64, value_dtype=dt, initializer=default, dim=dim, init_size=bounded_cap,
                         kv_creator=de.HkvHashTableCreator(config=de.HkvHashTableConfig(
                             init_capacity=bounded_cap, max_capacity=bounded_cap, max_hbm_for_values=1 << 28,
                             evict_strategy=de.HkvEvictStrategy.LRU)), **kw)


def dev_table(var):
  return var.tables[0]._table


def write_back(torch, de, route, var, deo, p, step, ids, grads, default_row):
  """One write-back of (ids, grads) through `route`; prefetch_step returns the rows its lookup half handed back."""
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  t, rows = dev_table(var), None
  if route == "apply_optimizer":   # apply_kernel: each key once
    t.apply_optimizer(p, ids, grads, default_row)
  elif route == "apply_sparse":
    t.apply_sparse(p, ids, grads, default_row)
  elif route == "apply_planned":
    t.apply_planned(p, SparsePlan("cuda:0", var.dim).build(ids), grads, default_row)
  elif route == "combined":   # combiner sum, no weights, one entry per output row: the entry's gradient is grad_out / 1 * 1
    seg = torch.arange(ids.numel(), dtype=torch.int64, device="cuda")
    t.apply_planned_combined(p, SparsePlan("cuda:0", var.dim).build(ids), grads, seg, None, 0, default_row)
  elif route == "prefetch_step":
    deo.iterations = step - 1
    rows = de.PrefetchStep(var, deo).prime(ids).step(grads, None)
  else:
    raise ValueError(route)
  torch.cuda.synchronize()
  t.check_errors()
  return rows


# ---- 1. storage rounding through the write-back ---------------------------------------------------------------------------------
def carrier(torch, de, vdtype, dim, tag):
  """The SGD carrier (lr 1, every key once, gradient -x, resident rows of 0) over the storage set packed into rows of `dim`:
  -> var, optimizer, keys, grads [n, dim], the expected rows in the storage type (the oracle's result, converted ONCE on the CPU)."""
  x = ne.pack_rows(ne.storage_values(), dim)
  want = ne.to_storage(torch, ne.pack_rows(ne.sgd_carrier_result(), dim), vdtype)
  opt = de.optimizers.SGD(1.0)
  var = make_var(torch, de, opt, vdtype, dim, tag)
  keys = T(torch, ne.row_keys(x.shape[0]))
  var.upsert(keys, torch.zeros((x.shape[0], dim), dtype=getattr(torch, vdtype), device="cuda"))
  return var, opt, keys, T(torch, -x), want


def carrier_context(dim):
  x = ne.pack_rows(ne.storage_values(), dim).reshape(-1)
  return lambda i: "x = %r / %08x, column %d" % (float(x[i]), int(x[i:i + 1].view(np.uint32)[0]), i % dim)


STORAGE_ROUTES = ([("apply_optimizer", d) for d in (4, 6, 68)] +   # the scalar ST path; 6: not a multiple of 4
                  [(r, d) for r in ("apply_sparse", "apply_planned", "combined") for d in (4, 64, 68)] +   # one granule, one full
                  [("prefetch_step", 68)])                                        # trip of apply_csr_body, a second with 15 idle lanes


@pytest.mark.parametrize("vdtype", HALVES)
@pytest.mark.parametrize("route,dim", STORAGE_ROUTES)
def test_storage_rounding_through_the_write_back(env, route, dim, vdtype):
  """Every float32 value at which a rounding to the storage type can go wrong, carried through `route` unchanged and rounded by
  to_stored / to_stored4 on the way into the row: the row holds torch's conversion of it, bit for bit.  A truncating or
  double-rounding conversion, a lost carry into the exponent, a tie that goes the wrong way, two elements packed in the wrong
  order (from column 64 on too) — each fails here."""
  torch, de = env
  var, opt, keys, grads, want = carrier(torch, de, vdtype, dim, "st_" + route)
  deo = de.DynamicEmbeddingOptimizer(opt)
  rows = write_back(torch, de, route, var, deo, opt.params(1), 1, keys, grads, torch.zeros(dim, device="cuda"))
  if rows is not None:   # the step's lookup half ran before its write-back
    assert rows.dtype == want.dtype and not bool(rows.view(torch.int16).any())
  ne.assert_bits(torch, var.lookup(keys), want, "%s %s dim %d" % (route, vdtype, dim), carrier_context(dim))
  assert int(var.size()) == keys.numel()


@pytest.mark.parametrize("dim", [4, 68])
def test_storage_rounding_through_the_grouped_combined_write_back(env, dim):
  """apply_planned_combined_many: a float16 and a bfloat16 table in ONE call."""
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan, apply_planned_combined_many
  members = [carrier(torch, de, vdtype, dim, "st_many") for vdtype in HALVES]
  zero = torch.zeros(dim, device="cuda")
  reqs = []
  for var, opt, keys, grads, want in members:
    seg = torch.arange(keys.numel(), dtype=torch.int64, device="cuda")
    reqs.append((dev_table(var), SparsePlan("cuda:0", dim).build(keys), grads, seg, None, 0, zero))
  apply_planned_combined_many(reqs, members[0][1].params(1))
  torch.cuda.synchronize()
  for vdtype, (var, opt, keys, grads, want) in zip(HALVES, members):
    dev_table(var).check_errors()
    ne.assert_bits(torch, var.lookup(keys), want, "grouped combined %s dim %d" % (vdtype, dim), carrier_context(dim))


# ---- 2. exact up-cast on the read side -------------------------------------------------------------------------------------------
PAT_DIM, PAT_KEYS = 32, 2048


def pattern_rows(torch, vdtype):
  """All 65536 storage patterns as [2048, 32] rows of the storage type (CPU), written as raw bits."""
  bits = np.arange(65536, dtype=np.uint16).view(np.int16).reshape(PAT_KEYS, PAT_DIM)
  return torch.from_numpy(bits.copy()).view(getattr(torch, vdtype))


def pattern_table(torch, vdtype, tag, keys=None, **kw):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  _serial[0] += 1
  vd = getattr(torch, vdtype)
  t = _DeviceTable(torch.int64, vd, torch.zeros(PAT_DIM, dtype=vd), "ne_pat_%s_%s_%d" % (tag, vdtype, _serial[0]), "cuda:0",
                   dim=PAT_DIM, **kw)
  all_keys = T(torch, ne.row_keys(PAT_KEYS))
  sel = slice(None) if keys is None else keys
  t.upsert(all_keys[sel], pattern_rows(torch, vdtype).cuda()[sel], unique_keys=True)
  return t, all_keys


@pytest.fixture(scope="module")
def pattern_owners(env):
  """Per storage type: a table holding every pattern, and a tier with half of the keys in each of its tables.  Read-only."""
  torch, _ = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTier
  out = {}
  for vdtype in HALVES:
    table, keys = pattern_table(torch, vdtype, "all", init_capacity=4096)
    upper, _ = pattern_table(torch, vdtype, "up", keys=slice(0, PAT_KEYS, 2), init_capacity=8192, max_capacity=8192, strategy=0)
    lower, _ = pattern_table(torch, vdtype, "lo", keys=slice(1, PAT_KEYS, 2))
    ex_up, ex_lo = upper.find(keys, return_exists=True)[1], lower.find(keys, return_exists=True)[1]
    assert bool((ex_up ^ ex_lo).all()) and int(ex_up.sum()) == PAT_KEYS // 2   # each key in exactly one tier
    out[vdtype] = {"table": table, "tier": _DeviceTier(upper, lower, 1 << 16), "keys": keys, "keep": (upper, lower)}
  return out


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("owner", ["table", "tier"])
@pytest.mark.parametrize("vdtype", HALVES)
def test_upcast_of_every_storage_pattern_in_the_pooled_read(env, pattern_owners, vdtype, owner, weighted):
  """find_combine (combiner sum, one entry per row) over rows holding all 65536 patterns: exactly float32(0) + w * upcast(x) in
  NumPy float32 — load_stored4 through the pooled read, subnormals, infinities and NaNs included (-0 gives +0 on both sides)."""
  torch, _ = env
  s = pattern_owners[vdtype]
  w = np.resize(np.array([1.0, 0.5, 2.0, -1.0], np.float32), PAT_KEYS) if weighted else None
  up = ne.upcast_bits(pattern_rows(torch, vdtype).view(torch.int16).numpy(), vdtype)
  with np.errstate(all="ignore"):
    want = (np.float32(0) + (np.float32(1) if w is None else w[:, None]) * up).astype(np.float32)
  seg = torch.arange(PAT_KEYS, dtype=torch.int64, device="cuda")
  got = s[owner].find_combine(s["keys"], seg, None if w is None else T(torch, w), 0, PAT_KEYS)
  torch.cuda.synchronize()
  assert got.dtype == torch.float32
  ne.assert_bits(torch, got, torch.from_numpy(want), "find_combine %s %s" % (owner, vdtype),
                 lambda i: "pattern %04x, weight %r" % (i, 1.0 if w is None else float(w[i // PAT_DIM])))


@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse"])
@pytest.mark.parametrize("vdtype", HALVES)
def test_zero_gradient_step_leaves_every_storage_pattern(env, vdtype, route):
  """to_stored(load_stored(b)) == b: an SGD step with a zero gradient over rows holding all 65536 patterns leaves the bits of every
  pattern that is not a NaN, and every NaN a NaN (-0 stays -0: x - 1 * 0)."""
  torch, de = env
  t, keys = pattern_table(torch, vdtype, "zero_" + route, init_capacity=4096)
  p = de.optimizers.SGD(1.0).params(1)
  g = torch.zeros((PAT_KEYS, PAT_DIM), device="cuda")
  getattr(t, route)(p, keys, g, torch.zeros(PAT_DIM, device="cuda"))
  torch.cuda.synchronize()
  t.check_errors()
  ne.assert_bits(torch, t.find(keys), pattern_rows(torch, vdtype), "%s %s" % (route, vdtype), lambda i: "pattern %04x" % i)


# ---- 3. the rules at their edges --------------------------------------------------------------------------------------------------
def _rule_params():
  """(rule, step, vdtype, dim, route), the routes of one (rule, step, vdtype, dim) next to each other: they share one reference."""
  out = []
  for rule, step in ne.RULES:
    for vdtype, dims in (("float32", (4, 6, 68)), ("float16", (4, 68)), ("bfloat16", (4, 68))):   # float32 4: VEC4; 6: scalar
      for dim in dims:
        routes = ("apply_optimizer",) if dim % 4 else ("apply_optimizer", "apply_sparse", "apply_planned", "prefetch_step")
        out += [pytest.param(rule, step, vdtype, dim, r, id="%s-t%d-%s-%d-%s" % (rule, step, vdtype, dim, r)) for r in routes]
  return out


def seed_rows(torch, de, deo, opt, var, c):
  """The resident rows of a RuleCase: p through upsert, every slot field through get_slot(var, name).upsert."""
  dt = var.value_dtype
  kres = T(torch, c.keys[:c.n_res])
  var.upsert(kres, T(torch, c.p0).to(dt))   # (exact: the values are storage values already)
  for name, s in zip(opt.slots, (c.s10, c.s20)):
    deo.get_slot(var, name).upsert(kres, T(torch, s).to(dt))


def check_rows(torch, deo, opt, var, keys, wants, vdtype, what, context, rows=None):
  """The parameter AND every slot field of `keys` against the oracle's result converted once (rows: only these)."""
  sel = (lambda x: x) if rows is None else (lambda x: x[rows])
  fields = [("p", var.lookup(keys))] + [(n, deo.get_slot(var, n).lookup(keys)) for n in opt.slots]
  for (name, got), want in zip(fields, wants):
    ne.assert_bits(torch, sel(got.cpu()), sel(ne.to_storage(torch, want, vdtype)), "%s: %s" % (what, name), context)


@pytest.mark.parametrize("rule,step,vdtype,dim,route", _rule_params())
def test_rules_at_their_edges(env, rule, step, vdtype, dim, route):
  """One write-back over the Cartesian edge grid of the rule (tests/numeric_edges.py: EDGE, NONNEG, ftrl_linear_values) against ONE
  call of oracle.optimizers' rule and one conversion to the storage type: the parameter and every slot field, bit for bit.
  Resident rows hold the grid (rounded to the storage type first on half tables); in the sparse, planned and step routes ids repeat
  1, 2 and 8 times and the expected sums are segment_sum_by_key's (input order); never-seen keys of the same batch start from the
  FLOAT default 0.3 and initial accumulator 0.1, neither a bfloat16 / float16 value.  (PrefetchStep takes the default row from the
  variable, which keeps it in the storage type: its new rows start from that image of 0.3 — and still from the float 0.1.)"""
  torch, de = env
  opt = make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  default = ne.DEFAULT
  if route == "prefetch_step":
    default = float(ne.through_storage(torch, np.array([ne.DEFAULT], np.float32), vdtype)[0])
  c = ne.rule_case(torch, rule, step, vdtype, dim, route != "apply_optimizer", default)
  var = make_var(torch, de, opt, vdtype, dim, "rule_" + route, default=ne.DEFAULT)
  seed_rows(torch, de, deo, opt, var, c)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  write_back(torch, de, route, var, deo, opt.params(step), step, T(torch, c.ids), T(torch, c.grads), default_row)
  check_rows(torch, deo, opt, var, T(torch, c.keys), (c.want_p, c.want_s1, c.want_s2), vdtype,
             "%s step %d %s dim %d %s" % (rule, step, vdtype, dim, route), c.context)
  assert int(var.size()) == c.keys.size


@pytest.mark.parametrize("route", ["apply_optimizer", "apply_sparse"])
@pytest.mark.parametrize("vdtype", ["float32"] + HALVES)
@pytest.mark.parametrize("rule", ["sgd", "adam", "adagrad", "ftrl"])
def test_new_rows_of_a_bounded_table_at_capacity(env, rule, vdtype, route):
  """Phase 2 (apply_evict_kernel behind apply_optimizer, PHASE2 of apply_csr_body behind apply_sparse): the table shape of
  test_bounded_table_at_capacity_new_rows — an LRU table filled to its capacity, then one batch of never-seen keys with the EDGE
  gradients.  Every batch key that is present afterwards holds exactly the new-row result: the rule on the float default 0.3 and the
  optimizer's initial slot values, converted once.  (Which keys are evicted or admitted is pinned in test_gpu_eviction.py.)"""
  torch, de = env
  dim, cap = 32, 8192
  opt = make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = make_var(torch, de, opt, vdtype, dim, "cap_" + route, default=ne.DEFAULT, bounded_cap=cap)
  dt = getattr(torch, vdtype)
  capacity = dev_table(var).capacity()
  old = -np.arange(1, 4 * capacity + 1, dtype=np.int64)
  for part in np.array_split(old, 8):
    var.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=dt))
  census = dev_table(var).slot_census()
  assert census["empty"] == 0 and census["locked"] == 0   # at capacity: a never-seen key can only come in by eviction
  B = census["live"] // 4
  ids = ne.row_keys(B)
  np.random.default_rng(31).shuffle(ids)
  g = np.resize(ne.EDGE, B * dim).reshape(B, dim)   # (27 and 32 are coprime: every column meets every value)
  a1, a2 = ne.new_row_slots(rule)
  full = lambda x: np.full((B, dim), x, np.float32)
  gsum = g   # apply_optimizer takes a key's gradient as it is; the sparse route sums first (0 + g: a -0 becomes +0)
  if route == "apply_sparse":
    from oracle import optimizers as oopt
    with np.errstate(all="ignore"):
      uniq, gsum, _ = oopt.segment_sum_by_key(ids, g)
    assert np.array_equal(uniq, ids)
  wants = ne.oracle_step(rule, 1, gsum, full(ne.DEFAULT), full(a1), full(a2))
  it = T(torch, ids)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  write_back(torch, de, route, var, deo, opt.params(1), 1, it, T(torch, g), default_row)
  ex = var.lookup(it, return_exists=True)[1].cpu()
  assert bool(ex.any())
  rows = torch.nonzero(ex).reshape(-1)
  check_rows(torch, deo, opt, var, it, wants, vdtype, "%s %s %s" % (rule, vdtype, route),
             lambda i: "(%s, g %r, new row)" % (rule, float(g[int(rows[i // dim]), i % dim])), rows=rows)
