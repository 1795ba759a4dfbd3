"""GPU: float16 / bfloat16 grad_out in the combined sparse write-back (tfra_table_apply_planned_combined_typed; CombRows and GradHalf
in one pack of hot_sums_body and add_rows, csrc/tfra_apply_device.h).

The contract (include/tfra_mi355x.h): a typed combined call equals its untyped twin given GO32[r] = f32(grad_out[r]) * s, and the
product is formed BEFORE the combiner's backward — entry e's gradient is ((f32(g) * s) / den) * w.  Every comparison is bit for bit
(tests/numeric_edges.py: assert_bits): the float matrix the kernels form in registers is the one tests/half_grads_model.py forms
on the host, and everything behind it is the twin's code."""
import ctypes
import types

import numpy as np
import pytest

from oracle import optimizers as oopt
from tests import half_grads_model as hm
from tests import numeric_edges as ne
from tests import test_gpu_half_grads as hg
from tests import test_gpu_numeric_edges as tg
from tests.sparse_helpers import COMB, _export_state

pytestmark = pytest.mark.gpu

T = tg.T
f32 = np.float32
TYPED, UNTYPED = "tfra_table_apply_planned_combined_typed", "tfra_table_apply_planned_combined"
SCALE = f32(1e-3)


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture
def calls(monkeypatch):
  from tests.sparse_helpers import Calls
  return Calls(monkeypatch)


def combined(torch, var, p, ids, grad_out, seg, w, comb, default_row, grad_scale=None):
  """One combined write-back through the Python table layer: a float32 grad_out reaches the untyped C call, a contiguous half one
  the typed call."""
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  t = tg.dev_table(var)
  t.apply_planned_combined(p, SparsePlan("cuda:0", var.dim).build(ids), grad_out, seg, w, COMB[comb], default_row, grad_scale=grad_scale)
  torch.cuda.synchronize()
  t.check_errors()


# ---- 1. every pattern through every load site -------------------------------------------------------------------------------------
ARRANGEMENTS = {"once": (64, 1024, 1), "hot_8_8": (64, 1024, 16), "hot_16_two_chunks": (128, 512, 16)}


@pytest.mark.parametrize("scale", [None, SCALE], ids=["noscale", "scale1e-3"])
@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_every_pattern_through_every_load_site(env, calls, fmt, arrangement, scale):
  """A float32 table, SGD with lr = 1, default row 0, never-seen keys, combiner sum without weights, one entry per grad_out row: the
  65 536 patterns of the format are grad_out.  once: every key has one entry (add_rows' COMB + GH arm); hot_8_8: every key has 16
  entries in 16 different rows, the pattern row at its first entry and +0 rows at the others (hot_sums' 8 + 8 form at dim 64);
  hot_16_two_chunks: dim 128, the 16-in-flight form and a second chunk.  Expected p = 0 - GO32, GO32 from the model."""
  torch, de = env
  dim, n_keys, occ = ARRANGEMENTS[arrangement]
  bits = hm.all_patterns().reshape(n_keys, dim)
  keys = ne.row_keys(n_keys)
  ids = np.tile(keys, occ)
  gbits = np.concatenate([bits, np.zeros(((occ - 1) * n_keys, dim), np.uint16)])
  with np.errstate(all="ignore"):
    uniq, gsum, _ = oopt.segment_sum_by_key(ids, hm.g32(gbits, fmt, scale))
    want = oopt.sgd(np.zeros((n_keys, dim), f32), gsum, 1.0)
  assert np.array_equal(uniq, keys)
  opt = de.optimizers.SGD(1.0)
  var = tg.make_var(torch, de, opt, "float32", dim, "ch_pat_" + arrangement, default=0.0)
  combined(torch, var, opt.params(1), T(torch, ids), hg.half_tensor(torch, gbits, fmt), torch.arange(ids.size, device="cuda"), None, "sum",
           torch.zeros(dim, dtype=torch.float32, device="cuda"), hg.scale_tensor(torch, scale))
  assert calls[TYPED] == 1 and calls[UNTYPED] == 0
  flat = bits.reshape(-1)
  ne.assert_bits(torch, var.lookup(T(torch, keys)).cpu(), torch.from_numpy(want), "%s %s scale %r" % (fmt, arrangement, scale),
                 lambda i: "pattern %04x" % flat[i])
  assert int(var.size()) == n_keys


@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_the_scale_comes_before_the_combiner(env, calls, fmt):
  """Combiner mean with weights 0.3 / 0.7 / 1.1 over the three entries of every row (their sum is no power of two) and the scale
  1e-3, every key once: the expectation is ((g32 * s) / den) * w in NumPy float32, den summed in input order, so a kernel that
  divides before it scales, or contracts two of the steps, leaves other bits."""
  torch, de = env
  dim, n_rows = 64, 1024
  bits = hm.all_patterns().reshape(n_rows, dim)
  w3 = np.array([0.3, 0.7, 1.1], f32)
  den = f32(f32(w3[0] + w3[1]) + w3[2])
  keys = ne.row_keys(3 * n_rows)
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), 3)
  w = np.tile(w3, n_rows)
  with np.errstate(all="ignore"):
    go32 = (hm.upcast(bits, fmt) * SCALE).astype(f32)
    eg = ((go32[seg] / den).astype(f32) * w[:, None]).astype(f32)
    want = oopt.sgd(np.zeros((keys.size, dim), f32), eg, 1.0)
  opt = de.optimizers.SGD(1.0)
  var = tg.make_var(torch, de, opt, "float32", dim, "ch_order", default=0.0)
  combined(torch, var, opt.params(1), T(torch, keys), hg.half_tensor(torch, bits, fmt), T(torch, seg), T(torch, w), "mean",
           torch.zeros(dim, dtype=torch.float32, device="cuda"), hg.scale_tensor(torch, SCALE))
  assert calls[TYPED] == 1 and calls[UNTYPED] == 0
  flat = bits.reshape(-1)
  ne.assert_bits(torch, var.lookup(T(torch, keys)).cpu(), torch.from_numpy(want), "%s mean, weighted, scale 1e-3" % fmt,
                 lambda i: "pattern %04x, weight %r" % (flat[(i // dim // 3) * dim + i % dim], float(w3[(i // dim) % 3])))


# ---- 2. twins at the rules' edges -------------------------------------------------------------------------------------------------
REPEATS = (1, 2, 8, 9, 17, 600)   # 8: the last cold list length; 9: the first hot one; 17 crosses an item; 600 a 512-entry bin
PER_ROW = 4


def edge_batch(torch, fmt, dim, vdtype, weighted):
  """Resident rows and one sparse batch for the twins.  Per repeat count two resident keys and one never-seen key (600: one and
  one).  The entries of the keys with 9 and more occurrences come first (shuffled) and lie in grad_out rows of finite values of at
  most 3 in magnitude, so that their sums are finite and depend on their order; the entries of the other keys follow in rows that
  hold all of ne.EDGE (infinities and a NaN included), each value through the half format.  Four entries per row; with weights, one
  row's weights are all 0 and one row's cancel (the mean's denominator is 0).
  -> (case for tg.seed_rows, ids [nnz], seg [nnz], weights [nnz] or None, grad_out bits [n_rows, dim])."""
  rng = np.random.default_rng(dim)
  counts, resident = [], []
  for r in REPEATS:
    for res in ((True, False) if r == 600 else (True, True, False)):
      counts.append(r)
      resident.append(res)
  counts, resident = np.array(counts), np.array(resident)
  keys = ne.row_keys(counts.size, stride=104729, base=7)
  order = np.argsort(~resident, kind="stable")   # resident keys first, as tg.seed_rows takes them
  keys, counts = keys[order], counts[order]
  n_res = int(resident.sum())
  big = np.repeat(np.arange(counts.size), np.where(counts >= 9, counts, 0))
  small = np.repeat(np.arange(counts.size), np.where(counts < 9, counts, 0))
  rng.shuffle(big)
  rng.shuffle(small)
  idx = np.concatenate([big, small])
  nnz = idx.size
  n_rows = (nnz + PER_ROW - 1) // PER_ROW
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), PER_ROW)[:nnz]
  edge = hm.bits_of(torch, ne.to_storage(torch, ne.EDGE, fmt))
  tame = hm.bits_of(torch, ne.to_storage(torch, ne.EDGE[np.isfinite(ne.EDGE) & (np.abs(ne.EDGE) <= 3.0)], fmt))
  r, c = np.arange(n_rows)[:, None], np.arange(dim)[None, :]
  gbits = np.where(r < big.size // PER_ROW, tame[(r * 5 + c) % tame.size], edge[(r * 5 + c) % edge.size]).astype(np.uint16)
  w = None
  if weighted:
    w = rng.uniform(0.1, 2.0, size=nnz).astype(f32)
    w[seg == 3] = 0.0
    w[seg == n_rows - 2] = [1.0, -1.0, 0.5, -0.5]
  state = lambda lo: ne.through_storage(torch, (rng.random((n_res, dim)) * 2 + lo).astype(f32), vdtype)
  case = types.SimpleNamespace(keys=keys, n_res=n_res, p0=state(-1.0), s10=state(0.0), s20=state(0.0))
  return case, keys[idx], seg, w, np.ascontiguousarray(gbits)


def run_twins(torch, de, rule, dim, vdtype, fmt, comb, weighted, scale, tag, stochastic=False):
  """Twin A: the untyped call on GO32 formed on the host by the model.  Twin B: the typed call on the half bits and the device scale."""
  opt = hg.make_opt(de, rule)
  c, ids, seg, w, gbits = edge_batch(torch, fmt, dim, vdtype, weighted)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  wt = None if w is None else T(torch, w)
  twins = []
  for which in "AB":
    var = tg.make_var(torch, de, opt, vdtype, dim, "ch_%s_%s" % (tag, which), default=ne.DEFAULT)
    deo = de.DynamicEmbeddingOptimizer(opt)
    tg.seed_rows(torch, de, deo, opt, var, c)
    if stochastic:
      var.set_stochastic_rounding(hg.SEED)
    if which == "A":
      combined(torch, var, opt.params(1), T(torch, ids), T(torch, hm.g32(gbits, fmt, scale)), T(torch, seg), wt, comb, default_row)
    else:
      combined(torch, var, opt.params(1), T(torch, ids), hg.half_tensor(torch, gbits, fmt), T(torch, seg), wt, comb, default_row,
               hg.scale_tensor(torch, scale))
    twins.append((var, deo))
  hg.assert_twins(torch, de, opt, twins, T(torch, c.keys),
                  "%s dim %d %s rows, %s grad_out, %s%s, scale %r" % (rule, dim, vdtype, fmt, comb, ", weighted" if weighted else "", scale))
  assert int(twins[0][0].size()) == c.keys.size


def _twin_params():
  out = []
  for i, (rule, vdtype) in enumerate((r, v) for r in hg.NESTED_RULES for v in ("float32", "float16", "bfloat16")):
    out.append(pytest.param(i, rule, vdtype, hm.FORMATS[i % 2], id="%s-%s-grad_out_%s" % (rule, vdtype, hm.FORMATS[i % 2])))
  return out


@pytest.mark.parametrize("i,rule,vdtype,fmt", _twin_params())
def test_twins_at_the_rules_edges(env, calls, i, rule, vdtype, fmt):
  """The seven fused rules x the three row types at dim 68 (a second, partial chunk); the gradient's format alternates across the
  cases.  Each case runs the three combiners; with and without weights and with and without the scale alternate over the cases
  and the combiners, so that every pairing occurs for every combiner."""
  torch, de = env
  for k, comb in enumerate(("sum", "mean", "sqrtn")):
    weighted, scale = (i + k) % 2 == 0, (None, SCALE)[(i // 2 + k) % 2]
    run_twins(torch, de, rule, 68, vdtype, fmt, comb, weighted, scale, "tw")
    assert calls[TYPED] == k + 1 and calls[UNTYPED] == k + 1   # twin A took the untyped call, twin B the typed one


# ---- 3. a full bounded table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_phase_2_on_a_full_bounded_table(env, calls, fmt):
  """Two LRU tables of 8192 slots filled to capacity by the same calls, then one batch of never-seen keys (four entries per
  grad_out row, combiner mean, weights, scale): twin A the untyped call on GO32, twin B the typed call.  Both tables keep their
  size, admit the same batch keys, and every batch key present holds the same bits in the parameter and in every slot; as many old
  keys left one table as the other.  (WHICH old keys leave is not compared: an LRU score is the device clock of the thread that
  wrote it, so the order among the keys of one fill call — and with it the victim — is not the same on two tables, whichever call
  writes back.)"""
  torch, de = env
  dim, cap, rule, vdtype = 32, 8192, "adam", "bfloat16"
  opt = hg.make_opt(de, rule)
  rng = np.random.default_rng(31)
  twins, old = [], None
  for which in "AB":
    var = tg.make_var(torch, de, opt, vdtype, dim, "ch_cap_" + which, default=ne.DEFAULT, bounded_cap=cap)
    capacity = tg.dev_table(var).capacity()
    old = -np.arange(1, 4 * capacity + 1, dtype=np.int64)
    for part in np.array_split(old, 8):
      var.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=getattr(torch, vdtype)))
    census = tg.dev_table(var).slot_census()
    assert census["empty"] == 0 and census["locked"] == 0
    twins.append((var, de.DynamicEmbeddingOptimizer(opt), census["live"]))
  B = twins[0][2] // 4
  ids = ne.row_keys(B)
  rng.shuffle(ids)
  n_rows = (B + PER_ROW - 1) // PER_ROW
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), PER_ROW)[:B]
  w = rng.uniform(0.1, 2.0, size=B).astype(f32)
  edge = hm.bits_of(torch, ne.to_storage(torch, ne.EDGE, fmt))
  gbits = np.resize(edge, n_rows * dim).reshape(n_rows, dim)
  default_row = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  it = T(torch, ids)
  for which, (var, _, _) in zip("AB", twins):
    before = int(var.size())
    if which == "A":
      combined(torch, var, opt.params(1), it, T(torch, hm.g32(gbits, fmt, SCALE)), T(torch, seg), T(torch, w), "mean", default_row)
    else:
      combined(torch, var, opt.params(1), it, hg.half_tensor(torch, gbits, fmt), T(torch, seg), T(torch, w), "mean", default_row,
               hg.scale_tensor(torch, SCALE))
    assert int(var.size()) == before
  assert calls[TYPED] == 1 and calls[UNTYPED] == 1
  (va, da, _), (vb, db, _) = twins
  exa, exb = va.lookup(it, return_exists=True)[1].cpu(), vb.lookup(it, return_exists=True)[1].cpu()
  assert torch.equal(exa, exb), "the twins admitted different batch keys"
  assert 2 * int(exa.sum()) >= B
  rows = torch.nonzero(exa).reshape(-1)
  for (name, a), (_, b) in zip(hg.fields(torch, da, opt, va, it), hg.fields(torch, db, opt, vb, it)):
    ne.assert_bits(torch, b.cpu()[rows], a.cpu()[rows], "phase 2, %s grad_out: %s" % (fmt, name))
  ot = T(torch, old)
  left = [int((~v.lookup(ot, return_exists=True)[1]).sum()) for v in (va, vb)]
  assert left[0] == left[1] and left[0] >= int(exa.sum()), left


# ---- 4. stochastic rounding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_twins_round_stochastically_alike(env, calls, fmt):
  """Both twins with stochastic rounding of one seed on float16 rows, Adam: the hash takes the write-back index, the same on both."""
  torch, de = env
  run_twins(torch, de, "adam", 68, "float16", fmt, "mean", True, SCALE, "sr", stochastic=True)
  assert calls[TYPED] == 1 and calls[UNTYPED] == 1


# ---- 5. forwarding ----------------------------------------------------------------------------------------------------------------------
def raw_typed(torch, t, p, plan, rec, seg, w, comb, n_rows, d):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding._args import _ptr, _stream
  rc = _capi.lib().tfra_table_apply_planned_combined_typed(t._h, ctypes.byref(p), plan._h, ctypes.byref(rec) if rec is not None else None,
                                                           _ptr(seg), _ptr(w), COMB[comb], n_rows, _ptr(d), _stream(t._device))
  return rc, _capi.lib().tfra_last_error().decode()


def test_float32_without_a_scale_forwards_to_the_untyped_call(env):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  dim, fmt = 68, "bfloat16"
  opt = hg.make_opt(de, "adam")
  c, ids, seg, w, gbits = edge_batch(torch, fmt, dim, "float32", True)
  g, it, st, wt = T(torch, hm.g32(gbits, fmt, None)), T(torch, ids), T(torch, seg), T(torch, w)
  d = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  twins = []
  for which in "AB":
    var = tg.make_var(torch, de, opt, "float32", dim, "ch_fwd_" + which, default=ne.DEFAULT)
    deo = de.DynamicEmbeddingOptimizer(opt)
    tg.seed_rows(torch, de, deo, opt, var, c)
    t, p = tg.dev_table(var), opt.params(1)
    if which == "A":
      combined(torch, var, p, it, g, st, wt, "sqrtn", d)
    else:
      plan = SparsePlan("cuda:0", dim).build(it)
      rc, msg = raw_typed(torch, t, p, plan, _capi.Grads(g.data_ptr(), _capi.TFRA_F32, 0, None), st, wt, "sqrtn", g.shape[0], d)
      assert rc == 0, msg
      torch.cuda.synchronize()
      t.check_errors()
    twins.append((var, deo))
  hg.assert_twins(torch, de, opt, twins, T(torch, c.keys), "float32 through the typed call")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_alone(env):
  """A misaligned half grad_out, float32 with a scale, dtype 3, reserved = 1, NULL grads, and n_rows * dim = 2^32 (by n_rows alone,
  over a grad_out that is never read): each is refused with the contract's code and the function's name, and the table's export,
  its size and check_errors are unchanged."""
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  dim, n = 64, 64
  opt = hg.make_opt(de, "adam")
  deo = de.DynamicEmbeddingOptimizer(opt)
  var = tg.make_var(torch, de, opt, "float32", dim, "ch_refuse", default=ne.DEFAULT)
  keys = T(torch, ne.row_keys(n))
  var.upsert(keys, torch.arange(n * dim, dtype=torch.float32, device="cuda").reshape(n, dim))
  before = _export_state(torch, de, deo, opt, var)
  t, p = tg.dev_table(var), opt.params(1)
  buf = torch.ones(n * dim + 4, dtype=torch.bfloat16, device="cuda")
  g32 = torch.ones((n, dim), dtype=torch.float32, device="cuda")
  one = torch.ones(1, dtype=torch.float32, device="cuda")
  d = torch.full((dim,), ne.DEFAULT, dtype=torch.float32, device="cuda")
  seg = torch.arange(n, device="cuda")
  plan = SparsePlan("cuda:0", dim).build(keys)
  torch.cuda.synchronize()
  assert buf[1:].data_ptr() % 8 == 2
  U, I = _capi.ERR_UNSUPPORTED, -1
  bad = {"misaligned": (_capi.Grads(buf[1:].data_ptr(), _capi.TFRA_BF16, 0, None), n, U, "8-B aligned"),
         "f32_scale": (_capi.Grads(g32.data_ptr(), _capi.TFRA_F32, 0, one.data_ptr()), n, U, "no scale"),
         "dtype": (_capi.Grads(buf.data_ptr(), 3, 0, None), n, I, "dtype"),
         "reserved": (_capi.Grads(buf.data_ptr(), _capi.TFRA_BF16, 1, None), n, I, "reserved"),
         "null_grads": (_capi.Grads(None, _capi.TFRA_BF16, 0, None), n, I, "null gradients"),
         "null_record": (None, n, I, "null gradients"),
         "addressing": (_capi.Grads(buf.data_ptr(), _capi.TFRA_F16, 0, None), (1 << 32) // dim, U, "n_rows * dim < 2^32")}
  for what, (rec, n_rows, code, text) in bad.items():
    rc, msg = raw_typed(torch, t, p, plan, rec, seg, None, "sum", n_rows, d)
    assert rc == code, (what, rc, msg)
    assert msg.startswith("apply_planned_combined_typed: ") and text in msg, (what, msg)
  # one row fewer is inside the limit: the same record is then refused by nothing (not run: its grad_out would be read)
  torch.cuda.synchronize()
  t.check_errors()
  assert int(var.size()) == n
  for x, y in zip(before, _export_state(torch, de, deo, opt, var)):
    assert torch.equal(x, y)
  # and the plan still serves a good call
  rc, msg = raw_typed(torch, t, p, plan, _capi.Grads(buf.data_ptr(), _capi.TFRA_BF16, 0, one.data_ptr()), seg, None, "sum", n, d)
  assert rc == 0, msg
  torch.cuda.synchronize()
  t.check_errors()
