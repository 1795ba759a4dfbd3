"""GPU: the grouped typed weight gradients — tfra_multi_find_combine_backprop_weights_typed and
tfra_multi_find_combine_ragged_backprop_weights_typed over MIXED lists: float32, float16 and bfloat16 descriptors, with and without
a scale, plain tables and a tier, dims 16 / 64 / 128.  Each dw_out equals the single typed call on its descriptor bit for bit
(numeric_edges.assert_bits); *launches_out is

    (1 if any descriptor has nnz > 0) + the distinct (tiered or not, value dtype, NCH[, pruning or not], float-or-half) classes

among the descriptors with nnz > 0 and n_rows > 0; a refused list names the bad descriptor's index and writes nothing."""
import ctypes

import numpy as np
import pytest

from tests import half_grads_model as M
from tests.numeric_edges import assert_bits
from tests.sparse_helpers import T, table
from tests.test_gpu_weight_grad import edge_batch, ragged_batch
from tests.test_gpu_wgrad_half import half, pair, random_half_bits, scale_of

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
f32 = np.float32


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops
  return torch, de, table_ops


# (owner kind, value dtype, dim, gradient format, scale): all three formats, with and without a scale, NCH 1 and 2, a tier
MEMBERS = [("table", "float32", 16, "bfloat16", None), ("table", "float32", 64, "float16", 1e-3), ("table", "float16", 64, "float32", None),
           ("table", "bfloat16", 128, "bfloat16", 0.5), ("tier", "float32", 64, "float16", None), ("table", "float32", 128, "float32", 2.0),
           ("tier", "float32", 64, "float32", None), ("table", "float32", 64, "bfloat16", None), ("table", "float32", 16, "float32", None)]
_OWNERS = {}


def owner_of(torch, de, kind, vdtype, dim):
  if (kind, vdtype, dim) not in _OWNERS:
    t = table(torch, de, "cuckoo", vdtype, dim)._table
    if kind == "tier":
      tier, upper, lower = pair(torch, "many_%s_%d" % (vdtype, dim), vdtype, dim, default=0.25)
      ids_t = edge_batch(torch)[0]
      uniq = torch.unique(torch.cat([ids_t, ragged_batch(torch)[3]]))
      lower.upsert(uniq[::2].contiguous(), t.find(uniq[::2].contiguous()))
      upper.upsert(uniq[::6].contiguous(), t.find(uniq[::6].contiguous()), unique_keys=True)
      _OWNERS[(kind, vdtype, dim)] = tier
    else:
      _OWNERS[(kind, vdtype, dim)] = t
  return _OWNERS[(kind, vdtype, dim)]


def gradient(torch, n_rows, dim, fmt, seed):
  """(the tensor handed to the calls, its bits or None): float32 gradients are random normals."""
  if fmt == "float32":
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n_rows, dim), generator=g, device="cuda"), None
  b16 = random_half_bits(n_rows, dim, fmt, seed)
  return half(torch, b16, fmt), b16


def nch(dim):
  return 1 if dim <= 64 else 2 if dim <= 128 else 4


def expected_launches(classes):
  return (1 if classes else 0) + len(set(classes))


def build(torch, de, ragged, members=MEMBERS, prune_of=lambda i: False):
  """-> (requests, scales, classes, singles): the grouped call's requests, one scale per request, each request's launch class and
  the single typed call on it."""
  reqs, scales, classes, singles = [], [], [], []
  for i, (kind, vdtype, dim, fmt, s) in enumerate(members):
    owner = owner_of(torch, de, kind, vdtype, dim)
    sc = scale_of(torch, s)
    c = i % 3
    if ragged:
      rs, w, rs_t, ids_t, w_t, seg_t = ragged_batch(torch)
      G, _ = gradient(torch, 40, dim, fmt, 50 + i)
      prune = prune_of(i)
      wt = w_t if prune else (torch.where(torch.isnan(w_t), torch.ones_like(w_t), w_t) if i % 2 == 0 else None)
      reqs.append((owner, rs_t, ids_t, wt, c, G, prune, 777 if i % 4 == 1 else None))
      singles.append(lambda o=owner, a=(rs_t, ids_t, wt, c, G), p=prune, f=(777 if i % 4 == 1 else None), sc=sc:
                     o.find_combine_ragged_weight_grad_typed(*a, prune=p, fill_id=f, grad_scale=sc))
      classes.append((kind, vdtype, nch(dim), bool(prune and wt is not None), fmt != "float32"))
    else:
      ids_t, seg_t, w_t = edge_batch(torch)
      G, _ = gradient(torch, 37, dim, fmt, 10 + i)
      wt = w_t if i % 2 == 0 else None
      reqs.append((owner, ids_t, seg_t, wt, c, G))
      singles.append(lambda o=owner, a=(ids_t, seg_t, wt, c, G), sc=sc: o.find_combine_weight_grad_typed(*a, grad_scale=sc))
      classes.append((kind, vdtype, nch(dim), fmt != "float32"))
    scales.append(sc)
  return reqs, scales, classes, singles


@pytest.mark.parametrize("ragged", [False, True])
def test_a_mixed_list_equals_the_single_typed_calls(env, monkeypatch, ragged):
  torch, de, table_ops = env
  from tests.sparse_helpers import Calls
  reqs, scales, classes, singles = build(torch, de, ragged, prune_of=lambda i: i in (1, 3, 6))
  want = [f() for f in singles]
  calls = Calls(monkeypatch)
  many_f = table_ops.find_combine_ragged_weight_grad_many if ragged else table_ops.find_combine_weight_grad_many
  got, launches = many_f(reqs, return_launches=True, grad_scale=scales)
  name = "tfra_multi_find_combine_ragged_backprop_weights" if ragged else "tfra_multi_find_combine_backprop_weights"
  assert {k: v for k, v in calls.n.items() if "backprop_weights" in k} == {name + "_typed": 1}      # ONE grouped typed call
  assert launches == expected_launches(classes), (launches, classes)
  for i, (g, w) in enumerate(zip(got, want)):
    assert g.dtype == torch.float32 and g.shape == w.shape
    assert_bits(torch, g, w, "descriptor %d %r" % (i, MEMBERS[i]))
  # both axes are in the list: a float and a half class of one (owner, dtype, NCH), and more classes than the untyped call has
  assert len(set(classes)) > len(set(c[:-1] for c in classes))


@pytest.mark.parametrize("ragged", [False, True])
def test_launch_counts(env, ragged):
  torch, de, table_ops = env
  many_f = table_ops.find_combine_ragged_weight_grad_many if ragged else table_ops.find_combine_weight_grad_many
  halves = [m for m in MEMBERS if m[3] != "float32"]
  reqs, scales, classes, singles = build(torch, de, ragged, halves)
  got, launches = many_f(reqs, return_launches=True, grad_scale=scales)
  assert launches == expected_launches(classes)
  # an all-half list has the untyped call's count: the same requests on float32 gradients, through the untyped call
  as_float = [r[:5] + (r[5].to(torch.float32),) + r[6:] for r in reqs]
  _, untyped = many_f(as_float, return_launches=True)
  assert launches == untyped == 1 + len(set(c[:-1] for c in classes))
  # one float32 descriptor among the halves adds exactly its class
  extra = ("table", "float32", 64, "float32", None)
  assert any(c[:3] == ("table", "float32", 1) for c in classes)              # its (owner, dtype, NCH) is there already, as half
  reqs1, scales1, classes1, singles1 = build(torch, de, ragged, halves + [extra])
  got1, launches1 = many_f(reqs1, return_launches=True, grad_scale=scales1)
  assert launches1 == launches + 1 == expected_launches(classes1)
  assert_bits(torch, got1[-1], singles1[-1](), "the float32 descriptor among halves")
  for a, b in zip(got1[:-1], got):
    assert_bits(torch, a, b, "the halves beside it")
  # twice the list: the same classes, the same count
  _, twice = many_f(reqs + reqs, return_launches=True, grad_scale=scales + scales)
  assert twice == launches


def test_one_scale_for_all_equals_one_per_request(env):
  torch, de, table_ops = env
  members = [(k, v, d, f, None) for (k, v, d, f, _) in MEMBERS]
  reqs, _, _, _ = build(torch, de, False, members)
  sc = scale_of(torch, 1e-3)
  one = table_ops.find_combine_weight_grad_many(reqs, grad_scale=sc)
  per = table_ops.find_combine_weight_grad_many(reqs, grad_scale=[sc] * len(reqs))
  for i, (a, b) in enumerate(zip(one, per)):
    assert_bits(torch, a, b, "descriptor %d" % i)
    owner, ids_t, seg_t, wt, c, G = reqs[i]
    assert_bits(torch, a, owner.find_combine_weight_grad_typed(ids_t, seg_t, wt, c, G, grad_scale=sc), "single call %d" % i)
  rreqs, _, _, _ = build(torch, de, True, members)
  one = table_ops.find_combine_ragged_weight_grad_many(rreqs, grad_scale=sc)
  per = table_ops.find_combine_ragged_weight_grad_many(rreqs, grad_scale=[sc] * len(rreqs))
  for i, (a, b) in enumerate(zip(one, per)):
    assert_bits(torch, a, b, "ragged descriptor %d" % i)
  with pytest.raises(ValueError):
    table_ops.find_combine_weight_grad_many(reqs, grad_scale=[sc] * (len(reqs) - 1))


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("why", ["misaligned_half", "float32_with_scale", "reserved", "dtype3", "combiner3", "misaligned_default_row"])
def test_one_bad_descriptor_in_the_middle_refuses_the_list(env, ragged, why):
  """Three good descriptors, the middle one spoiled: the code is the single typed call's, the message names index 1 and every
  dw_out keeps its sentinel."""
  torch, de, table_ops = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _stream
  members = [("table", "float32", 64, "bfloat16", None), ("table", "float32", 16, "float16", None), ("tier", "float32", 64, "float32", None)]
  mirror = _capi.FindCombineRaggedWgradTypedDesc if ragged else _capi.FindCombineWgradTypedDesc
  descs = (mirror * 3)()
  keep, dws = [], []
  scale = scale_of(torch, 0.5)
  for i, (kind, vdtype, dim, fmt, _) in enumerate(members):
    owner = owner_of(torch, de, kind, vdtype, dim)
    up = owner._upper if kind == "tier" else owner
    e = descs[i]
    e.struct_size = ctypes.sizeof(mirror)
    e.combiner = 1
    e.table, e.tier = (None, owner._h.value) if kind == "tier" else (owner._h.value, None)
    if ragged:
      rs, w, rs_t, ids_t, w_t, seg_t = ragged_batch(torch)
      n_rows = 40
      e.n_rows, e.row_splits, e.flags, e.reserved, e.fill_id = n_rows, rs_t.data_ptr(), 0, 0, 0
    else:
      ids_t, seg_t, w_t = edge_batch(torch)
      n_rows = 37
      e.n_rows, e.seg = n_rows, seg_t.data_ptr()
    G, _ = gradient(torch, n_rows + 1, dim, fmt, 90 + i)          # one spare row: a pointer 2 bytes in stays inside the allocation
    d = up._default_value
    dw = torch.full((ids_t.numel(),), 7.0, device="cuda")
    e.nnz, e.ids, e.weights, e.default_row, e.dw_out = ids_t.numel(), ids_t.data_ptr(), None, d.data_ptr(), dw.data_ptr()
    e.grad_out = _capi.Grads(G.data_ptr(), {"float32": _capi.TFRA_F32, "float16": _capi.TFRA_F16, "bfloat16": _capi.TFRA_BF16}[fmt], 0, None)
    keep.append((G, d))
    dws.append(dw)
  dev = owner_of(torch, de, "table", "float32", 64)._device

  def run():
    launches = ctypes.c_uint32(99)
    f = getattr(_capi.lib(), "tfra_multi_find_combine_ragged_backprop_weights_typed" if ragged else
                "tfra_multi_find_combine_backprop_weights_typed")
    rc = f(_workspace(dev), 3, ctypes.c_void_p(ctypes.addressof(descs)), ctypes.c_void_p(ctypes.addressof(launches)), _stream(dev))
    return rc, _capi.lib().tfra_last_error().decode(), launches.value

  bad = descs[1]
  g0 = bad.grad_out.grads
  code, text = {
      "misaligned_half": (UNSUPPORTED, "8-B aligned"), "float32_with_scale": (UNSUPPORTED, "float32 gradients take no scale"),
      "reserved": (INVALID, "reserved"), "dtype3": (INVALID, "dtype"), "combiner3": (INVALID, "bad argument"),
      "misaligned_default_row": (UNSUPPORTED, "misaligned buffer")}[why]
  if why == "misaligned_half":
    bad.grad_out.grads = g0 + 2
  elif why == "float32_with_scale":
    bad.grad_out.dtype, bad.grad_out.d_scale = _capi.TFRA_F32, scale.data_ptr()
  elif why == "reserved":
    bad.grad_out.reserved = 1
  elif why == "dtype3":
    bad.grad_out.dtype = 3
  elif why == "combiner3":
    bad.combiner = 3
  else:
    bad.default_row = bad.default_row + 4
  rc, msg, launches = run()
  who = "multi_find_combine_ragged_backprop_weights_typed" if ragged else "multi_find_combine_backprop_weights_typed"
  assert rc == code and launches == 0, (rc, msg)
  assert msg.startswith(who + ": descriptor 1: ") and text in msg, msg
  torch.cuda.synchronize()
  for dw in dws:
    assert bool((dw == 7.0).all())
