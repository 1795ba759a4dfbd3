"""GPU: float16 / bfloat16 gradients and grad_scale through DynamicEmbeddingOptimizer.apply_combined_gradients[_many] and the
lookups whose wrappers they take.

Every case holds a variable fed the half gradient (and the scale) against a twin variable fed `g_half.float() * scale` through the
signature without grad_scale: by the typed calls' contract the same bits, whichever route either takes.  `Calls` shows the route:
the fused one hands the halves to the typed C call, every other one up-casts first."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls, T, _export_state, bits, grad, writeback_batch as batch
from tests.test_gpu_ragged_lookup import _train_case

pytestmark = pytest.mark.gpu

TYPED, UNTYPED = "tfra_table_apply_planned_combined_typed", "tfra_table_apply_planned_combined"
MANY_TYPED, MANY_UNTYPED = "tfra_multi_apply_planned_combined_typed", "tfra_multi_apply_planned_combined"


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def adam(de):
  return de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)


def variables(torch, de, opt, tag, dim=64, n=1, **kw):
  """n variables with the rule's slots, holding the even ids below 300 (the others enter from the default row)."""
  out = []
  for i in range(n):
    v = de.Variable(dim=dim, name="chv_%s_%d" % (tag, i), initializer=0.5, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt), **kw)
    keys = torch.arange(0, 300, 2, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(dim + i)
    v.upsert(keys, torch.randn((keys.numel(), dim), generator=g, device="cuda"))
    out.append(v)
  return out


def same_state(torch, de, opt, da, db, va, vb):
  for a, b in zip(va, vb):
    sa, sb = _export_state(torch, de, da, opt, a), _export_state(torch, de, db, opt, b)
    assert len(sa) == len(sb) == 2 + len(opt.slots) and sa[0].numel() > 0
    for j, (x, y) in enumerate(zip(sa, sb)):
      assert torch.equal(x, y), "field %d differs from the twin fed the up-cast gradient" % j


def scale_of(torch, s=1.0 / 128):
  return torch.full((1,), s, dtype=torch.float32, device="cuda")


def half_grad(torch, G, fmt, scaled):
  """The gradient a half model hands back: G (times the loss scale) in the format."""
  return (G * 128.0 if scaled else G).to(getattr(torch, fmt))


# ---- a single variable --------------------------------------------------------------------------------------------------------------
def lookup(de, kind, var, case):
  rs, seg, ids, w, _ = case
  reo = de.ragged_embedding_ops
  if kind == "sparse":
    return de.embedding_lookup_sparse(var, (seg, ids), w, combiner="sqrtn", return_trainable=True, num_rows=128)[1]
  if kind == "safe":   # rows 5 and 127 are empty: they take default_id
    return de.safe_embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", default_id=7, return_trainable=True, num_rows=128)[1]
  if kind == "ragged":
    return reo.embedding_lookup_sparse(var, (rs, ids), w, combiner="mean", return_trainable=True)[1]
  assert kind == "ragged_safe", kind
  return reo.safe_embedding_lookup_sparse(var, (rs, ids), w, combiner="sum", default_id=7, return_trainable=True)[1]


@pytest.mark.parametrize("fmt,scaled", [("bfloat16", False), ("float16", True)])
@pytest.mark.parametrize("kind", ["sparse", "safe", "ragged", "ragged_safe"])
def test_one_variable_takes_the_typed_call(env, monkeypatch, kind, fmt, scaled):
  torch, de = env
  opt = adam(de)
  case = _train_case(torch)
  (va,), (vb,) = variables(torch, de, opt, "one_a_%s_%s" % (kind, fmt)), variables(torch, de, opt, "one_b_%s_%s" % (kind, fmt))
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  s = scale_of(torch) if scaled else None
  for step in range(2):
    g = half_grad(torch, case[4] * (step + 1), fmt, scaled)
    twa, twb = lookup(de, kind, va, case), lookup(de, kind, vb, case)
    calls = Calls(monkeypatch)
    da.apply_combined_gradients([(g, twa)], grad_scale=s)
    assert calls[TYPED] == 1 and calls[UNTYPED] == 0, calls.n
    monkeypatch.undo()
    db.apply_combined_gradients([(g.float() * s if scaled else g.float(), twb)])
  same_state(torch, de, opt, da, db, [va], [vb])


def test_field_wise_embedding_takes_a_three_dimensional_half_gradient(env, monkeypatch):
  torch, de = env
  from tests.test_gpu_field_layers import DIM, NSLOTS, _ids, slot_of
  opt = de.optimizers.Adam(0.01)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  layers = [de.layers.FieldWiseEmbedding(DIM, NSLOTS, slot_map_fn=slot_of(NSLOTS), combiner="mean", name="chv_fwl_" + which,
                                         initializer=0.25, **kw) for which in "ab"]
  deos = [de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)]
  for step in range(2):
    ids = _ids(torch, 50 + step, batch=30, universe=6000)
    g = torch.Generator(device="cuda").manual_seed(900 + step)
    grad_half = (torch.randn((30, NSLOTS, DIM), generator=g, device="cuda") * 0.01).to(torch.bfloat16)
    tws = [layer(ids, return_trainable=True)[1] for layer in layers]
    calls = Calls(monkeypatch)
    deos[0].apply_combined_gradients([(grad_half, tws[0])])
    assert calls[TYPED] == 1 and calls[UNTYPED] == 0, calls.n
    monkeypatch.undo()
    deos[1].apply_combined_gradients([(grad_half.float(), tws[1])])
  same_state(torch, de, opt, deos[0], deos[1], [layers[0].params], [layers[1].params])


# ---- what does not go down as halves -------------------------------------------------------------------------------------------------
def test_a_non_contiguous_half_gradient_is_upcast(env, monkeypatch):
  torch, de = env
  opt = adam(de)
  case = _train_case(torch)
  (va,), (vb,) = variables(torch, de, opt, "nc_a"), variables(torch, de, opt, "nc_b")
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  wide = torch.zeros((128, 128), dtype=torch.bfloat16, device="cuda")
  wide[:, :64] = case[4].to(torch.bfloat16)
  g = wide[:, :64]
  assert not g.is_contiguous()
  s = scale_of(torch)
  twa, twb = lookup(de, "sparse", va, case), lookup(de, "sparse", vb, case)
  calls = Calls(monkeypatch)
  da.apply_combined_gradients([(g, twa)], grad_scale=s)
  assert calls[TYPED] == 0 and calls[UNTYPED] == 1, calls.n
  monkeypatch.undo()
  db.apply_combined_gradients([(g.float() * s, twb)])
  same_state(torch, de, opt, da, db, [va], [vb])


@pytest.mark.parametrize("route", ["exact_order", "two_shards", "generic"])
def test_fallback_routes_honour_the_scale(env, monkeypatch, route):
  torch, de = env
  opt = de.optimizers.Momentum(0.05, 0.9) if route == "generic" else adam(de)
  if route == "generic":
    assert opt.kind is None
  case = _train_case(torch)
  dev = "cuda:%d" % torch.cuda.current_device()
  kw = dict(devices=[dev, dev]) if route == "two_shards" else {}
  (va,), (vb,) = variables(torch, de, opt, "fb_a_" + route, **kw), variables(torch, de, opt, "fb_b_" + route, **kw)
  mk = lambda: de.DynamicEmbeddingOptimizer(opt, exact_order=(route == "exact_order"))
  da, db = mk(), mk()
  g, s = half_grad(torch, case[4], "float16", True), scale_of(torch)
  twa, twb = lookup(de, "sparse", va, case), lookup(de, "sparse", vb, case)
  calls = Calls(monkeypatch)
  da.apply_combined_gradients([(g, twa)], grad_scale=s)
  assert calls[TYPED] == 0 and calls[UNTYPED] == 0 and calls[MANY_TYPED] == 0, calls.n
  monkeypatch.undo()
  db.apply_combined_gradients([(g.float() * s, twb)])
  same_state(torch, de, opt, da, db, [va], [vb])


# ---- many variables --------------------------------------------------------------------------------------------------------------------
def sparse_inputs(torch, seed, n_rows=128):
  ids, _, w = batch(torch, seed, n_rows=n_rows, per_row=4, planted=0)
  return (torch.repeat_interleave(torch.arange(n_rows, device="cuda"), 4), ids), w


def lookups(de, vs, sps, ws):
  return [tw for _, tw in de.embedding_lookup_sparse_many(vs, sps, ws, combiner="mean", return_trainable=True, num_rows=128)]


def many_vars(torch, de, opt, tag, dims):
  from tests.sparse_helpers import make_var
  return [make_var(torch, de, opt, "chv_%s_%d" % (tag, i), d) for i, d in enumerate(dims)]


def test_eight_variables_make_one_grouped_typed_call(env, monkeypatch):
  torch, de = env
  opt = adam(de)
  dims = [16, 32, 64, 128, 64, 16, 128, 32]
  va, vb = many_vars(torch, de, opt, "m8a", dims), many_vars(torch, de, opt, "m8b", dims)
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  sps, ws = zip(*[sparse_inputs(torch, 190 + i) for i in range(8)])
  s = scale_of(torch)
  for step in (1, 2):
    Gs = [half_grad(torch, grad(torch, 190 + i, 128, d, step), "float16" if i % 2 else "bfloat16", True) for i, d in enumerate(dims)]
    db.apply_combined_gradients(list(zip(Gs, lookups(de, vb, sps, ws))), grad_scale=s)   # the loop of single typed calls
    tws = lookups(de, va, sps, ws)
    calls = Calls(monkeypatch)
    da.apply_combined_gradients_many(list(zip(Gs, tws)), grad_scale=s)
    assert calls[MANY_TYPED] == 1 and calls[MANY_UNTYPED] == 0 and calls[TYPED] == 0 and calls[UNTYPED] == 0, calls.n
    monkeypatch.undo()
    assert da.iterations == db.iterations == step
  same_state(torch, de, opt, da, db, va, vb)
  # and both equal the variables fed the up-cast product through today's signature
  vc = many_vars(torch, de, opt, "m8c", dims)
  dc = de.DynamicEmbeddingOptimizer(opt)
  for step in (1, 2):
    Gs = [half_grad(torch, grad(torch, 190 + i, 128, d, step), "float16" if i % 2 else "bfloat16", True) for i, d in enumerate(dims)]
    tws = lookups(de, vc, sps, ws)
    calls = Calls(monkeypatch)
    dc.apply_combined_gradients_many([(g.float() * s, tw) for g, tw in zip(Gs, tws)])
    assert calls[MANY_UNTYPED] == 1 and calls[MANY_TYPED] == 0, calls.n
    monkeypatch.undo()
  same_state(torch, de, opt, da, dc, va, vc)


def test_a_variable_that_occurs_twice_flushes_in_list_order(env, monkeypatch):
  torch, de = env
  opt = adam(de)

  def vs(tag):
    v = many_vars(torch, de, opt, tag, [64, 32])
    return v + [v[0]]                                                       # the first variable again, with other ids

  va, vb = vs("twice_a"), vs("twice_b")
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  sps, ws = zip(*[sparse_inputs(torch, 195 + i) for i in range(3)])
  Gs = [half_grad(torch, grad(torch, 195 + i, 128, v.dim), "bfloat16", False) for i, v in enumerate(va)]
  db.apply_combined_gradients([(g.float(), tw) for g, tw in zip(Gs, lookups(de, vb, sps, ws))])
  tws = lookups(de, va, sps, ws)
  calls = Calls(monkeypatch)
  da.apply_combined_gradients_many(list(zip(Gs, tws)))
  assert calls[MANY_TYPED] == 2 and calls[MANY_UNTYPED] == 0, calls.n
  monkeypatch.undo()
  same_state(torch, de, opt, da, db, va[:2], vb[:2])


# ---- a tiered variable -------------------------------------------------------------------------------------------------------------------
def test_a_tiered_variable_trains_with_half_gradients_like_its_roomy_twin(env):
  """The training batches of tests/test_gpu_tier_sparse_variable.py (a cache of 15 * 89 slots under 3000 keys, so keys are demoted
  and come up again): the tiered variable gets bfloat16 gradients and a scale, its roomy twin their float32 product."""
  torch, de = env
  from tests import test_gpu_tier_sparse_variable as tsv
  universe, steps = tsv._batches(54)
  (tiered, dt), (twin, dw) = tsv._pair(env, "adam", "chv_half")
  s = scale_of(torch)
  seen = set()
  for step, (ids, seg, w, g) in enumerate(steps):
    tsv._no_saturation(ids)
    it, st, wt = (torch.from_numpy(x).cuda() for x in (ids, seg, w))
    gh = (torch.from_numpy(g).cuda() * 128.0).to(torch.bfloat16)
    combiner = ("mean", "sum", "sqrtn")[step % 3]
    _, tw = de.embedding_lookup_sparse(tiered, (st, it), wt, combiner=combiner, return_trainable=True, num_rows=g.shape[0])
    dt.apply_combined_gradients([(gh, tw)], grad_scale=s)
    _, tw = de.embedding_lookup_sparse(twin, (st, it), wt, combiner=combiner, return_trainable=True, num_rows=g.shape[0])
    dw.apply_combined_gradients([(gh.float() * s, tw)])
    seen.update(ids.tolist())
  t = tiered._tables[0]
  assert t._tier.stats()["demoted"] > 0
  seen_t = torch.from_numpy(np.fromiter(seen, np.int64, len(seen))).cuda()
  t._table.check_errors()
  t._lower.check_errors()
  a, b = tsv._whole_rows(torch, tiered, seen_t), tsv._whole_rows(torch, twin, seen_t)
  assert a.shape == b.shape and torch.equal(bits(torch, a), bits(torch, b))


# ---- unchanged defaults -----------------------------------------------------------------------------------------------------------------
def test_defaults_still_give_float32(env):
  torch, de = env
  from tfra_amd.dynamic_embedding import device_ops
  opt = adam(de)
  case = _train_case(torch)
  (var,) = variables(torch, de, opt, "dflt")
  tw = lookup(de, "sparse", var, case)
  gh = case[4].to(torch.bfloat16)
  g = tw.check_grad_out(gh)
  assert g.dtype == torch.float32 and g.is_contiguous() and torch.equal(g, gh.float())
  kept = tw.check_grad_out(gh, keep_half=True)
  assert kept.dtype == torch.bfloat16 and kept.shape == g.shape and kept.data_ptr() == gh.data_ptr()
  assert tw.check_grad_out(case[4], keep_half=True).dtype == torch.float32
  with pytest.raises(ValueError, match="shape"):
    tw.check_grad_out(gh[:5], keep_half=True)
  # grad_of and weights_grad read the float32 up-cast: what they gave for gh.float()
  assert torch.equal(bits(torch, tw.grad_of(gh)), bits(torch, tw.grad_of(gh.float())))
  assert torch.equal(bits(torch, tw.weights_grad(gh)), bits(torch, tw.weights_grad(gh.float())))
  eg = device_ops.sparse_segment_combine_backprop(gh.float(), tw.seg, tw.weights, tw.combiner)
  assert eg.dtype == torch.float32
