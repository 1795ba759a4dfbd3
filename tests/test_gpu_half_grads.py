"""GPU: float16 / bfloat16 gradients in the fused sparse write-backs (tfra_table_apply_sparse_typed, tfra_table_apply_planned_typed,
tfra_reduce_by_key_typed; the GradHalf pack member of hot_sums_body, add_rows and gather_csr_kernel).

The contract (include/tfra_mi355x.h): a typed call equals its untyped twin given G32[e] = f32(grads[e]) * s.  Every comparison
here is bit for bit (tests/numeric_edges.py: assert_bits — equal bits, or a NaN where a NaN is expected): the up-cast is exact and
the scale one IEEE multiplication, so the float matrix the kernels form in registers is the one tests/half_grads_model.py forms on
the host, and everything behind it is the twin's code."""
import ctypes
import types

import numpy as np
import pytest

from oracle import optimizers as oopt
from tests import fused_rules_edges as fe
from tests import half_grads_model as hm
from tests import numeric_edges as ne
from tests import test_gpu_numeric_edges as tg

pytestmark = pytest.mark.gpu

T = tg.T
SEED = 0x5EED0000C0FFEE11
TYPED = {"apply_sparse": "tfra_table_apply_sparse_typed", "apply_planned": "tfra_table_apply_planned_typed",
         "reduce": "tfra_reduce_by_key_typed"}
UNTYPED = {r: n[:-len("_typed")] for r, n in TYPED.items()}
NESTED_RULES = ["sgd", "adam", "adagrad", "ftrl"] + fe.RULES   # the seven fused rules


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture
def calls(monkeypatch):
  from tests.sparse_helpers import Calls
  return Calls(monkeypatch)


def make_opt(de, rule):
  return fe.make_opt(de, rule) if rule in fe.RULES else tg.make_opt(de, rule)


def half_tensor(torch, bits16, fmt):
  """uint16 ndarray -> device tensor of the format with exactly these bits."""
  return hm.from_bits(torch, bits16, fmt).cuda()


def scale_tensor(torch, scale):
  return None if scale is None else torch.full((1,), float(scale), dtype=torch.float32, device="cuda")


def write_back(torch, de, route, var, p, ids, grads, default_row, grad_scale=None):
  """One write-back through the Python table layer: float32 `grads` reach the untyped C call, a contiguous half matrix the typed."""
  from tfra_amd.dynamic_embedding import device_ops
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  t = tg.dev_table(var)
  if route == "apply_sparse":
    t.apply_sparse(p, ids, grads, default_row, grad_scale=grad_scale)
  elif route == "apply_planned":
    t.apply_planned(p, SparsePlan("cuda:0", var.dim).build(ids), grads, default_row, grad_scale=grad_scale)
  else:
    keys, sums, cnt = device_ops.reduce_by_key(ids, grads, grad_scale=grad_scale)
    t.apply_optimizer(p, keys, sums, default_row, n_dev=cnt)
  torch.cuda.synchronize()
  t.check_errors()


def fields(torch, deo, opt, var, keys):
  return [("p", var.lookup(keys))] + [(n, deo.get_slot(var, n).lookup(keys)) for n in opt.slots]


def assert_twins(torch, de, opt, twins, keys, what):
  """Twin B (typed) against twin A (float32): the size, the parameter and every slot field of every key, as bits."""
  (va, da), (vb, db) = twins
  assert int(va.size()) == int(vb.size()), what
  for (name, a), (_, b) in zip(fields(torch, da, opt, va, keys), fields(torch, db, opt, vb, keys)):
    ne.assert_bits(torch, b.cpu(), a.cpu(), "%s: %s" % (what, name))


# ---- 1. every pattern through every load site -------------------------------------------------------------------------------------
ARRANGEMENTS = {"once": (64, 1024, 1), "hot_8_8": (64, 1024, 16), "hot_16_two_chunks": (128, 512, 16)}


@pytest.mark.parametrize("scale", [None, 1e-3], ids=["noscale", "scale1e-3"])
@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_every_pattern_through_every_load_site(env, calls, fmt, arrangement, scale):
  """A float32 table, SGD with lr = 1, default row 0: the 65 536 patterns of the format are the gradient matrix of never-seen keys.
  once: every key occurs once (add_rows' `grads` arm, one row); hot_8_8: every key 16 times, the pattern at its first occurrence and
  +0 rows at the others (hot_sums' 8 + 8 form at dim 64); hot_16_two_chunks: dim 128, so the 16-in-flight form and a second chunk.
  Expected p = 0 - G32 summed as oopt.segment_sum_by_key sums it, G32 from the model."""
  torch, de = env
  dim, n_keys, occ = ARRANGEMENTS[arrangement]
  bits = hm.all_patterns().reshape(n_keys, dim)
  keys = ne.row_keys(n_keys)
  ids = np.tile(keys, occ)
  gbits = np.concatenate([bits, np.zeros(((occ - 1) * n_keys, dim), np.uint16)])
  s32 = None if scale is None else np.float32(scale)
  with np.errstate(all="ignore"):
    uniq, gsum, _ = oopt.segment_sum_by_key(ids, hm.g32(gbits, fmt, s32))
    want = oopt.sgd(np.zeros((n_keys, dim), np.float32), gsum, 1.0)
  assert np.array_equal(uniq, keys)
  opt = de.optimizers.SGD(1.0)
  var = tg.make_var(torch, de, opt, "float32", dim, "hg_pat_" + arrangement, default=0.0)
  write_back(torch, de, "apply_sparse", var, opt.params(1), T(torch, ids), half_tensor(torch, gbits, fmt),
             torch.zeros(dim, dtype=torch.float32, device="cuda"), scale_tensor(torch, s32))
  assert calls[TYPED["apply_sparse"]] == 1 and calls[UNTYPED["apply_sparse"]] == 0
  flat = bits.reshape(-1)
  ne.assert_bits(torch, var.lookup(T(torch, keys)).cpu(), torch.from_numpy(want), "%s %s scale %r" % (fmt, arrangement, scale),
                 lambda i: "pattern %04x" % flat[i])
  assert int(var.size()) == n_keys


# ---- 2. twin write-backs at the rules' edges ----------------------------------------------------------------------------------------
REPEATS = (1, 2, 8, 9, 17, 600)   # 8: the last cold list length; 9: the first hot one; 17 crosses an item; 600 a 512-entry bin


def edge_batch(torch, fmt, dim, vdtype):
  """Resident rows and one batch for the twins: per repeat count two resident keys and one never-seen key (600: one and one), ids
  shuffled; the gradients are ne.EDGE through the half format, three neighbouring values per key and column over its occurrences,
  so that most sums are finite and depend on their order.  -> (case for tg.seed_rows, ids, gradient bits [n, dim])."""
  rng = np.random.default_rng(dim)
  counts, resident = [], []
  for r in REPEATS:
    for res in ((True, False) if r == 600 else (True, True, False)):
      counts.append(r)
      resident.append(res)
  resident = np.array(resident)
  keys = ne.row_keys(len(counts), stride=104729, base=7)
  order = np.argsort(~resident, kind="stable")   # resident keys first, as tg.seed_rows takes them
  keys_sorted, counts_sorted = keys[order], np.array(counts)[order]
  n_res = int(resident.sum())
  idx = np.repeat(np.arange(len(counts)), counts_sorted)
  rng.shuffle(idx)
  o = np.argsort(idx, kind="stable")
  occ = np.empty(idx.size, dtype=np.int64)
  occ[o] = np.arange(idx.size) - np.searchsorted(idx[o], idx[o], side="left")
  edge = hm.bits_of(torch, ne.to_storage(torch, ne.EDGE, fmt))
  gbits = edge[(idx[:, None] * 5 + np.arange(dim)[None, :] + (occ % 3)[:, None]) % edge.size]
  state = lambda lo: ne.through_storage(torch, (rng.random((n_res, dim)) * 2 + lo).astype(np.float32), vdtype)
  c = types.SimpleNamespace(keys=keys_sorted, n_res=n_res, p0=state(-1.0), s10=state(0.0), s20=state(0.0))
  return c, keys_sorted[idx], np.ascontiguousarray(gbits)


def _twin_params():
  out = []
  for rule in NESTED_RULES:
    for dim in ((4, 68, 256) if rule in ("sgd", "adam") else (68,)):
      for vdtype in ("float32", "float16", "bfloat16"):
        for fmt in hm.FORMATS:
          out.append(pytest.param(rule, dim, vdtype, fmt, id="%s-%d-%s-grads_%s" % (rule, dim, vdtype, fmt)))
  return out


def run_twins(torch, de, rule, dim, vdtype, fmt, route, scale, tag, stochastic=False):
  opt = make_opt(de, rule)
  c, ids, gbits = edge_batch(torch, fmt, dim, vdtype)
  s32 = None if scale is None else np.float32(scale)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  twins = []
  for which in "AB":
    var = tg.make_var(torch, de, opt, vdtype, dim, "hg_%s_%s" % (tag, which), default=ne.DEFAULT)
    deo = de.DynamicEmbeddingOptimizer(opt)
    tg.seed_rows(torch, de, deo, opt, var, c)
    if stochastic:
      var.set_stochastic_rounding(SEED)
    if which == "A":
      write_back(torch, de, route, var, opt.params(1), T(torch, ids), T(torch, hm.g32(gbits, fmt, s32)), default_row)
    else:
      write_back(torch, de, route, var, opt.params(1), T(torch, ids), half_tensor(torch, gbits, fmt), default_row, scale_tensor(torch, s32))
    twins.append((var, deo))
  assert_twins(torch, de, opt, twins, T(torch, c.keys), "%s dim %d %s rows, %s gradients, %s, scale %r" % (rule, dim, vdtype, fmt, route, scale))
  assert int(twins[0][0].size()) == c.keys.size


@pytest.mark.parametrize("rule,dim,vdtype,fmt", _twin_params())
def test_twin_write_backs_at_the_rules_edges(env, calls, rule, dim, vdtype, fmt):
  """Two variables with the same seeded rows; twin A gets the float32 call with G32 built on the host by the model, twin B the typed
  call with the half matrix and the scale on the device — through apply_sparse, apply_planned and reduce_by_key + apply_optimizer,
  without a scale and with 1/1024.  Ids repeat 1, 2, 8, 9, 17 and 600 times and include never-seen keys.  The full rule set at dim
  68, SGD and Adam also at 4 and 256 (as tests/test_gpu_fused_rules.py prunes its grid)."""
  torch, de = env
  for route in TYPED:
    for k, scale in enumerate((None, 1.0 / 1024), 1):
      run_twins(torch, de, rule, dim, vdtype, fmt, route, scale, route)
      assert calls[TYPED[route]] == k and calls[UNTYPED[route]] == k, route   # twin A took the untyped call, twin B the typed one


@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_twins_round_stochastically_alike(env, calls, fmt):
  """Both twins with stochastic_rounding = SEED on bfloat16 rows, Adam: the hash takes the write-back index, the same on both."""
  torch, de = env
  run_twins(torch, de, "adam", 68, "bfloat16", fmt, "apply_sparse", 1.0 / 1024, "sr", stochastic=True)
  assert calls[TYPED["apply_sparse"]] == 1


# ---- 3. more than 2^18 ids ------------------------------------------------------------------------------------------------------------
def test_more_than_2_18_ids(env, calls):
  """2^18 + 1000 ids at dim 4, Adam, one id occurring in both chunks: apply_sparse_big's route with the typed reduce as its first
  stage, against the float32 call on a twin."""
  torch, de = env
  n, dim, fmt, scale = (1 << 18) + 1000, 4, "bfloat16", np.float32(1.0 / 1024)
  rng = np.random.default_rng(18)
  ids = rng.integers(0, 200000, size=n).astype(np.int64) * 3 + 1
  ids[5] = ids[(1 << 18) + 10] = 777777777   # in both chunks, and nowhere else
  edge = hm.bits_of(torch, ne.to_storage(torch, ne.EDGE[np.isfinite(ne.EDGE)], fmt))
  gbits = edge[rng.integers(0, edge.size, size=(n, dim))]
  opt = make_opt(de, "adam")
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  twins = []
  for which in "AB":
    var = tg.make_var(torch, de, opt, "float32", dim, "hg_big_" + which, default=ne.DEFAULT)
    g = T(torch, hm.g32(gbits, fmt, scale)) if which == "A" else half_tensor(torch, gbits, fmt)
    write_back(torch, de, "apply_sparse", var, opt.params(1), T(torch, ids), g, default_row, None if which == "A" else scale_tensor(torch, scale))
    twins.append((var, de.DynamicEmbeddingOptimizer(opt)))
  assert calls[TYPED["apply_sparse"]] == 1 and calls[UNTYPED["apply_sparse"]] == 1
  assert_twins(torch, de, opt, twins, T(torch, np.unique(ids)), "2^18 + 1000 ids")


# ---- 4. phase 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", hm.FORMATS)
@pytest.mark.parametrize("vdtype", ["float32", "bfloat16"])
def test_new_rows_of_a_bounded_table_at_capacity(env, calls, vdtype, fmt):
  """Phase 2 of apply_csr_body behind the typed call (the table shape of tests/test_gpu_numeric_edges.py): an LRU table of 8192
  slots filled to its capacity, then one batch of never-seen keys with the EDGE gradients in the half format and a scale.  Every
  batch key present afterwards holds the new-row result — Adam on the float default 0.3, the initial slots and the key's G32 sum —
  and at least half of the batch keys are present (an LRU table admits every new key; collisions inside the batch lose some: the
  float32 call on the same G32 leaves 2047 of 2047 present on this shape, and so does the typed call)."""
  torch, de = env
  dim, cap, rule, scale = 32, 8192, "adam", np.float32(1.0 / 1024)
  opt = make_opt(de, rule)
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, vdtype, dim, "hg_cap", default=ne.DEFAULT, bounded_cap=cap)
  capacity = tg.dev_table(var).capacity()
  old = -np.arange(1, 4 * capacity + 1, dtype=np.int64)
  for part in np.array_split(old, 8):
    var.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=getattr(torch, vdtype)))
  census = tg.dev_table(var).slot_census()
  assert census["empty"] == 0 and census["locked"] == 0
  B = census["live"] // 4
  ids = ne.row_keys(B)
  np.random.default_rng(31).shuffle(ids)
  edge = hm.bits_of(torch, ne.to_storage(torch, ne.EDGE, fmt))
  gbits = np.resize(edge, B * dim).reshape(B, dim)
  with np.errstate(all="ignore"):
    uniq, gsum, _ = oopt.segment_sum_by_key(ids, hm.g32(gbits, fmt, scale))
  assert np.array_equal(uniq, ids)
  a1, a2 = ne.new_row_slots(rule)
  full = lambda x: np.full((B, dim), x, np.float32)
  wants = ne.oracle_step(rule, 1, gsum, full(ne.DEFAULT), full(a1), full(a2))
  it = T(torch, ids)
  write_back(torch, de, "apply_sparse", var, opt.params(1), it, half_tensor(torch, gbits, fmt),
             torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda"), scale_tensor(torch, scale))
  assert calls[TYPED["apply_sparse"]] == 1
  ex = var.lookup(it, return_exists=True)[1].cpu()
  present = int(ex.sum())
  print("phase 2, %s rows, %s gradients: %d of %d batch keys present" % (vdtype, fmt, present, B))
  assert 2 * present >= B, "%d of %d batch keys present" % (present, B)
  rows = torch.nonzero(ex).reshape(-1)
  tg.check_rows(torch, deo, opt, var, it, wants, vdtype, "phase 2 %s %s" % (vdtype, fmt),
                lambda i: "(g bits %04x, new row)" % gbits[int(rows[i // dim]), i % dim], rows=rows)


# ---- 5. refusals and forwarding -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_alone(env):
  """A misaligned half pointer (a view offset by one element), reserved = 1, dtype 99, float32 with a scale: each is refused by
  all three calls with the contract's code and the function's name, and the table, its size and check_errors are unchanged."""
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import device_ops
  from tfra_amd.dynamic_embedding._args import _ptr, _stream
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  dim, n = 8, 64
  opt = make_opt(de, "adam")
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, "float32", dim, "hg_refuse", default=ne.DEFAULT)
  keys = T(torch, ne.row_keys(n))
  var.upsert(keys, torch.arange(n * dim, dtype=torch.float32, device="cuda").reshape(n, dim))
  before = [f.cpu().clone() for _, f in fields(torch, deo, opt, var, keys)]
  t = tg.dev_table(var)
  p = opt.params(1)
  lib, dev = _capi.lib(), t._device
  buf = torch.ones(n * dim + 4, dtype=torch.bfloat16, device="cuda")
  g32 = torch.ones((n, dim), dtype=torch.float32, device="cuda")
  one = torch.ones(1, dtype=torch.float32, device="cuda")
  d = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  plan = SparsePlan("cuda:0", dim).build(keys)
  ko, so, cnt = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty((n, dim), device="cuda"), torch.full((1,), -7, dtype=torch.int64, device="cuda")
  torch.cuda.synchronize()
  bad = {"misaligned": (_capi.Grads(buf[1:].data_ptr(), _capi.TFRA_BF16, 0, None), _capi.ERR_UNSUPPORTED, "8-B aligned"),
         "reserved": (_capi.Grads(buf.data_ptr(), _capi.TFRA_BF16, 1, None), -1, "reserved"),
         "dtype": (_capi.Grads(buf.data_ptr(), 99, 0, None), -1, "dtype"),
         "f32_scale": (_capi.Grads(g32.data_ptr(), _capi.TFRA_F32, 0, one.data_ptr()), _capi.ERR_UNSUPPORTED, "no scale")}
  assert buf[1:].data_ptr() % 8 == 2
  for what, (rec, code, text) in bad.items():
    ref = ctypes.byref(rec)
    for name, call in (("apply_sparse_typed", lambda: lib.tfra_table_apply_sparse_typed(t._h, ctypes.byref(p), n, _ptr(keys), ref, _ptr(d), _stream(dev))),
                       ("apply_planned_typed", lambda: lib.tfra_table_apply_planned_typed(t._h, ctypes.byref(p), plan._h, ref, _ptr(d), _stream(dev))),
                       ("reduce_by_key_typed", lambda: lib.tfra_reduce_by_key_typed(device_ops._workspace(dev), n, _ptr(keys), dim, ref, _ptr(ko), _ptr(so),
                                                                                   _ptr(cnt), _stream(dev)))):
      assert call() == code, (what, name)
      msg = lib.tfra_last_error().decode()
      assert msg.startswith(name + ": ") and text in msg, (what, msg)
  torch.cuda.synchronize()
  t.check_errors()
  assert int(var.size()) == n and int(cnt) == -7
  for f0, (name, f1) in zip(before, fields(torch, deo, opt, var, keys)):
    ne.assert_bits(torch, f1.cpu(), f0, "after the refusals: " + name)


def test_float32_without_a_scale_forwards_to_the_untyped_call(env):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding._args import _ptr, _stream
  dim, fmt = 68, "bfloat16"
  opt = make_opt(de, "adam")
  c, ids, gbits = edge_batch(torch, fmt, dim, "float32")
  g = T(torch, hm.g32(gbits, fmt, None))
  it = T(torch, ids)
  d = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  twins = []
  for which in "AB":
    var = tg.make_var(torch, de, opt, "float32", dim, "hg_fwd_" + which, default=ne.DEFAULT)
    deo = de.DynamicEmbeddingOptimizer(opt)
    tg.seed_rows(torch, de, deo, opt, var, c)
    t, p = tg.dev_table(var), opt.params(1)
    if which == "A":
      t.apply_sparse(p, it, g, d)
    else:
      rec = _capi.Grads(g.data_ptr(), _capi.TFRA_F32, 0, None)
      _capi.call("tfra_table_apply_sparse_typed", t._h, ctypes.byref(p), it.numel(), _ptr(it), ctypes.byref(rec), _ptr(d), _stream(t._device))
    torch.cuda.synchronize()
    t.check_errors()
    twins.append((var, deo))
  assert_twins(torch, de, opt, twins, T(torch, c.keys), "float32 through the typed call")


# ---- 6. the Python layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
def test_optimizer_apply_sparse_takes_half_gradients_and_a_scale(env, calls, shards):
  """DynamicEmbeddingOptimizer.apply_sparse with a bfloat16 gradient tensor and grad_scale equals the same call with
  grad.float() * scale, as bits: one shard through tfra_table_apply_sparse_typed, two through tfra_reduce_by_key_typed."""
  torch, de = env
  dim, fmt = 68, "bfloat16"
  opt = make_opt(de, "adam")
  c, ids, gbits = edge_batch(torch, fmt, dim, "float32")
  g, it = half_tensor(torch, gbits, fmt), T(torch, ids)
  scale = torch.full((1,), 1.0 / 1024, dtype=torch.float32, device="cuda")
  twins = []
  for which in "AB":
    var = de.Variable(dim=dim, devices=["cuda:0"] * shards, name="hg_py_%d_%s" % (shards, which), initializer=ne.DEFAULT,
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    deo = de.DynamicEmbeddingOptimizer(opt)
    tg.seed_rows(torch, de, deo, opt, var, c)
    if which == "A":
      deo.apply_sparse(var, it, g.float() * scale)
    else:
      deo.apply_sparse(var, it, g, grad_scale=scale)
    torch.cuda.synchronize()
    twins.append((var, deo))
  route = "apply_sparse" if shards == 1 else "reduce"
  assert calls[TYPED[route]] == 1 and calls[UNTYPED[route]] == 1
  assert_twins(torch, de, opt, twins, T(torch, c.keys), "%d shard(s)" % shards)


def test_generic_rule_accepts_a_scale_and_gives_the_upcast_result(env, calls):
  torch, de = env
  dim, fmt = 68, "bfloat16"
  opt = de.optimizers.Momentum(0.05, 0.9)   # unfused: the Generic route
  assert opt.kind is None
  c, ids, gbits = edge_batch(torch, fmt, dim, "float32")
  g, it = half_tensor(torch, gbits, fmt), T(torch, ids)
  scale = torch.full((1,), 1.0 / 1024, dtype=torch.float32, device="cuda")
  twins = []
  for which in "AB":
    var = tg.make_var(torch, de, opt, "float32", dim, "hg_gen_" + which, default=ne.DEFAULT)
    deo = de.DynamicEmbeddingOptimizer(opt)
    var.upsert(T(torch, c.keys[:c.n_res]), T(torch, c.p0))
    if which == "A":
      deo.apply_sparse(var, it, g.float() * scale)
    else:
      deo.apply_sparse(var, it, g, grad_scale=scale)
    torch.cuda.synchronize()
    twins.append((var, deo))
  assert sum(calls[n] for n in TYPED.values()) == 0   # the Generic route keeps the torch up-cast
  assert_twins(torch, de, opt, twins, T(torch, c.keys), "Generic")
