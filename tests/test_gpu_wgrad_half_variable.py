"""GPU: SparseTrainableWrapper.weights_grad and de.sparse_weights_grad_many on float16 / bfloat16 gradients: a
contiguous half grad_out and grad_scale go down as they are — the pooled route through the typed single call (a tiered variable:
the tier's), every other route through the typed chain twin, a list through ONE grouped typed call — and each result equals
weights_grad(GO32) bit for bit, GO32 = f32(grad_out) * s from the NumPy model (tests/half_grads_model.py).  Every other gradient
takes exactly the calls it took before."""
import numpy as np
import pytest

from tests import half_grads_model as M
from tests import sparse_helpers as H
from tests.numeric_edges import assert_bits
from tests.sparse_helpers import T, bits
from tests.test_gpu_tier_pooled_many import _side
from tests.test_gpu_weight_grad import DIM_W, N_W, _lookup, _wrapper_case
from tests.test_gpu_wgrad_half import half, random_half_bits, scale_of

pytestmark = pytest.mark.gpu

TABLE, TIER, CHAIN = ("tfra_table_find_combine_backprop_weights", "tfra_tier_find_combine_backprop_weights",
                      "tfra_sparse_segment_combine_backprop_weights")
GROUPED = "tfra_multi_find_combine_backprop_weights"
f32 = np.float32


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture(scope="module")
def variables(env):
  """name -> variable of dim 8 holding the even keys below 3000: pooled, callable initializer, two shards, tiered."""
  torch, de = env
  vs = {"pooled": H.filled_var(torch, de, "wghv_p", dim=DIM_W, initializer=0.5),
        "callable": H.filled_var(torch, de, "wghv_c", dim=DIM_W, initializer=lambda shape: torch.full(tuple(shape), 0.5)),
        "shards": H.filled_var(torch, de, "wghv_s", dim=DIM_W, initializer=0.5, devices=["cuda:0", "cuda:0"])}
  tiered = _side(de, "wghv", True)[0][0]
  assert tiered.dim == DIM_W and hasattr(tiered._tables[0], "_tier")
  keys = torch.arange(0, 3000, 2, device="cuda")
  g = torch.Generator(device="cuda").manual_seed(17)
  tiered.upsert(keys, torch.randn((keys.numel(), DIM_W), generator=g, device="cuda"))
  vs["tiered"] = tiered
  assert vs["pooled"].can_lookup_combined() and tiered.can_lookup_combined()
  assert not vs["callable"].can_lookup_combined() and not vs["shards"].can_lookup_combined()
  return vs


ROUTE = {"pooled": TABLE, "tiered": TIER, "callable": CHAIN, "shards": CHAIN}


def family(calls):
  """name -> count of the weight-gradient C calls made."""
  return {k: v for k, v in calls.n.items() if "backprop_weights" in k}


@pytest.mark.parametrize("fmt,scale", [("bfloat16", None), ("float16", 1e-3)])
@pytest.mark.parametrize("safe,combiner", [(False, "sum"), (True, "mean"), (True, "sqrtn")])
@pytest.mark.parametrize("form", ["tuple", "ragged"])
def test_weights_grad_takes_a_half_gradient_as_it_is(env, variables, monkeypatch, form, safe, combiner, fmt, scale):
  torch, de = env
  rs, seg, ids, w, _ = _wrapper_case(torch)
  if not safe:
    w = np.abs(w) + f32(0.1)
  rs_t, seg_t, ids_t, w_t = T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w)
  b16 = random_half_bits(N_W, DIM_W, fmt, 31)
  G, G32 = half(torch, b16, fmt), T(torch, M.g32(b16, fmt, scale))
  sc = scale_of(torch, scale)
  keep = (w > 0) if (safe and combiner != "sum") else np.ones(w.size, dtype=bool)
  for name, var in variables.items():
    _, tw = _lookup(de, var, form, safe, rs_t, seg_t, ids_t, w_t, combiner)
    want = tw.weights_grad(G32)                                     # the untyped route on GO32
    calls = H.Calls(monkeypatch)
    got = tw.weights_grad(G, grad_scale=sc)
    assert family(calls) == {ROUTE[name] + "_typed": 1}, (name, family(calls))      # one typed call, none of the untyped family
    monkeypatch.undo()
    assert got.dtype == torch.float32 and tuple(got.shape) == (w.size,)             # the caller's length and order
    assert_bits(torch, got, want, "%s %s %s" % (name, form, combiner))
    assert not bool(bits(torch, got[T(torch, ~keep)]).any()) and bool(got.any())   # exact zeros where the safe form pruned
  # the two routes give the same bits for the same rows, for half gradients too (pooled and callable hold the same rows)
  a = _lookup(de, variables["pooled"], form, safe, rs_t, seg_t, ids_t, w_t, combiner)[1].weights_grad(G, grad_scale=sc)
  b = _lookup(de, variables["callable"], form, safe, rs_t, seg_t, ids_t, w_t, combiner)[1].weights_grad(G, grad_scale=sc)
  assert_bits(torch, a, b, "pooled route against chain route")


def test_every_other_gradient_takes_the_calls_it_took(env, variables, monkeypatch):
  """float32; a half gradient that is not contiguous; float32 with a scale (multiplied in torch: the C call refuses that pair)."""
  torch, de = env
  rs, seg, ids, w, G = _wrapper_case(torch)
  rs_t, seg_t, ids_t, w_t, G_t = T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w), T(torch, G)
  b16 = random_half_bits(N_W, 2 * DIM_W, "bfloat16", 41)
  wide = half(torch, b16, "bfloat16")
  strided = wide[:, :DIM_W]                                           # every row's first half: not contiguous
  assert not strided.is_contiguous() and strided.dtype == torch.bfloat16
  s32 = T(torch, M.g32(b16[:, :DIM_W], "bfloat16", None))
  sc = scale_of(torch, 1e-3)
  scaled = T(torch, (G * f32(1e-3)).astype(f32))                     # what torch's float32 multiply gives
  for name, var in variables.items():
    _, tw = _lookup(de, var, "tuple", True, rs_t, seg_t, ids_t, w_t, "mean")
    base = tw.weights_grad(G_t)
    for what, g, kw, want in (("float32", G_t, {}, base), ("strided half", strided, {}, tw.weights_grad(s32)),
                              ("strided half with a scale", strided, dict(grad_scale=sc),
                               tw.weights_grad(T(torch, M.g32(b16[:, :DIM_W], "bfloat16", 1e-3)))),
                              ("float32 with a scale", G_t, dict(grad_scale=sc), tw.weights_grad(scaled))):
      calls = H.Calls(monkeypatch)
      got = tw.weights_grad(g, **kw)
      assert family(calls) == {ROUTE[name]: 1}, (name, what, family(calls))         # today's call, and only it
      monkeypatch.undo()
      assert_bits(torch, got, want, "%s: %s" % (name, what))


@pytest.mark.parametrize("scale", [None, 0.125])
def test_a_list_of_half_gradients_is_one_grouped_typed_call(env, variables, monkeypatch, scale):
  torch, de = env
  rs, seg, ids, w, G = _wrapper_case(torch)
  rs_t, seg_t, ids_t, w_t = T(torch, rs), T(torch, seg), T(torch, ids), T(torch, w)
  members = ["pooled", "tiered", "pooled", "shards"]
  fmts = ["bfloat16", "float16", "float32", "bfloat16"]
  sc = scale_of(torch, scale)
  pairs, want = [], []
  for k, (name, fmt) in enumerate(zip(members, fmts)):
    _, tw = _lookup(de, variables[name], "tuple", True, rs_t, seg_t, ids_t, w_t, ("mean", "sqrtn")[k % 2])
    if fmt == "float32":
      g = T(torch, np.random.default_rng(50 + k).standard_normal((N_W, DIM_W)).astype(f32))
      g32 = g if scale is None else g * sc
    else:
      b16 = random_half_bits(N_W, DIM_W, fmt, 50 + k)
      g, g32 = half(torch, b16, fmt), T(torch, M.g32(b16, fmt, scale))
    pairs.append((g, tw))
    want.append(tw.weights_grad(g32))
  calls = H.Calls(monkeypatch)
  got = de.sparse_weights_grad_many(pairs, grad_scale=sc)
  # the three pooled members — two halves and the float32 one riding along — in ONE grouped typed call; the two-shard one on its route
  assert family(calls) == {GROUPED + "_typed": 1, CHAIN + "_typed": 1}, family(calls)
  monkeypatch.undo()
  for k, (a, b) in enumerate(zip(got, want)):
    assert a.dtype == torch.float32 and tuple(a.shape) == (w.size,)
    assert_bits(torch, a, b, "member %d (%s, %s)" % (k, members[k], fmts[k]))
  # a list without a half member takes the untyped grouped call, as always
  floats = [(T(torch, G), tw) for _, tw in pairs[:3]]
  calls = H.Calls(monkeypatch)
  got = de.sparse_weights_grad_many(floats)
  assert family(calls) == {GROUPED: 1}, family(calls)
  monkeypatch.undo()
  for k, (a, (g, tw)) in enumerate(zip(got, floats)):
    assert_bits(torch, a, tw.weights_grad(g), "float member %d" % k)
