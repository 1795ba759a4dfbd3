"""GPU: whole rows out and back for wide rows — tfra_table_fetch_planned_wide, tfra_table_store_rows_wide and the
optimizers' whole_rows route under DynamicEmbeddingOptimizer(wide_rows=True).  References are plain torch / NumPy: the rows the
test stored itself (up-cast), torch's CPU cast for the one rounding, float64 sums of the gradients — exact where the gradients
are k / 8, else within m * 2^-24 * sum|g| per element, the bound of a float32 sum of m terms in any order — and the narrow
tfra_table_fetch_planned on column slices for the summation tree."""
import ctypes

import numpy as np
import pytest

from tests.sparse_helpers import Calls, T

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 8, 9, 16, 17, 600, 1, 1, 2, 3, 9, 19]   # occurrences per key: 13 = 4 * 3 + 1 keys; 600: a hot key of the plan
KEYS = np.arange(len(COUNTS), dtype=np.int64) * 7919 - 20000
RESIDENT = KEYS[::2]                                     # the others are never seen
AUX_INIT, DEFAULT = (0.1, -1.7, 3.3, 0.7), 0.3           # no aux_init is a half value: the stored image is not the float
_serial = [0]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def make_table(torch, vdtype, dim, aux, strategy=-1, cap=0):
  """-> (table, [stored field f of RESIDENT]): random rows of the value dtype in every field of the resident keys (cap: none)"""
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  _serial[0] += 1
  dt = getattr(torch, vdtype)
  t = _DeviceTable(torch.int64, dt, torch.full((dim,), DEFAULT).to(dt), "grw_%d" % _serial[0], "cuda:0", dim=dim, aux_fields=aux,
                   init_capacity=cap or 8192, max_capacity=cap, strategy=strategy, aux_init=AUX_INIT)
  g = torch.Generator(device="cuda").manual_seed(dim + aux)
  rows = [(torch.randn((RESIDENT.size, dim), generator=g, device="cuda") * 3).to(dt) for _ in range(0 if cap else 1 + aux)]
  for f, r in enumerate(rows):
    t.upsert(T(torch, RESIDENT), r, unique_keys=True, field=f)
  return t, rows


def batch(torch, dim):
  """-> (ids, their plan, the KEYS index of every id)"""
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  ids = np.repeat(KEYS, COUNTS)
  np.random.default_rng(5).shuffle(ids)
  return T(torch, ids), SparsePlan("cuda:0", dim).build(T(torch, ids)), np.searchsorted(KEYS, ids)


def in_key_order(torch, keys, cnt, tensors):
  assert int(cnt) == KEYS.size
  o = torch.argsort(keys[:KEYS.size])
  assert torch.equal(keys[:KEYS.size][o].cpu(), torch.from_numpy(KEYS))
  return [None if x is None else x[:KEYS.size][o] for x in tensors]


@pytest.mark.parametrize("aux", [0, 2, 4])
@pytest.mark.parametrize("dim", [260, 512, 1024])
@pytest.mark.parametrize("vdtype", ["float32", "bfloat16", "float16"])
def test_fetch_then_store(env, vdtype, dim, aux):
  torch, de = env
  t, rows = make_table(torch, vdtype, dim, aux)
  ids, plan, inv = batch(torch, dim)
  default_row = torch.full((dim,), 0.6).to(t.value_dtype).cuda()   # not the table's own: the call's argument is what counts
  want = []   # float32 [13, dim] per field, in KEYS order: the stored field of a resident key, else default_row / the image of aux_init
  for f, r in enumerate(rows):
    miss = default_row if f == 0 else torch.full((dim,), AUX_INIT[f - 1]).to(t.value_dtype).cuda()
    want.append(miss.to(torch.float32).repeat(KEYS.size, 1))
    want[f][::2] = r.to(torch.float32)
  g = torch.Generator(device="cuda").manual_seed(dim)
  exact = torch.randint(-4, 5, (ids.numel(), dim), generator=g, device="cuda").float() / 8
  normal = torch.randn((ids.numel(), dim), generator=g, device="cuda")
  mask = [f != 1 for f in range(1 + aux)]                          # a field the caller does not want comes back None
  for G, fields in ((exact, None), (normal, mask)):
    keys, outs, gsum, cnt = t.fetch_planned_wide(plan, grads=G, fields=fields, default_row=default_row)
    outs = in_key_order(torch, keys, cnt, outs + [gsum])
    for f in range(1 + aux):
      assert (outs[f] is None) if fields and not fields[f] else torch.equal(outs[f], want[f]), f
    G64, sums, mag = G.double().cpu().numpy(), np.zeros((KEYS.size, dim)), np.zeros((KEYS.size, dim))
    np.add.at(sums, inv, G64)
    np.add.at(mag, inv, np.abs(G64))
    err = np.abs(outs[-1].double().cpu().numpy() - sums)
    assert np.all(err <= (0 if G is exact else np.array(COUNTS)[:, None] * 2.0**-24 * mag)), err.max()
  for a in range(0, dim if aux == 0 else 0, 256):   # the summation tree: bit for bit the narrow call on every slice of <= 256 columns
    b = min(a + 256, dim)
    nk, _, ngsum, ncnt = make_table(torch, vdtype, b - a, 0)[0].fetch_planned(batch(torch, b - a)[1], grads=normal[:, a:b].contiguous(), fields=[False])
    assert torch.equal(outs[-1][:, a:b].contiguous().view(torch.int32), in_key_order(torch, nk, ncnt, [ngsum])[0].view(torch.int32))
  t.check_errors()
  assert t.size_host() == RESIDENT.size, "a fetch inserts nothing"
  # the store: 11 of the 13 keys (count= on the device), field 1 not given; then a fetch without gradients
  order = np.random.default_rng(dim).permutation(KEYS.size)
  written = torch.from_numpy(order[:11]).cuda()
  new = [None if f == 1 else torch.randn((KEYS.size, dim), generator=g, device="cuda") * 3 for f in range(1 + aux)]
  t.store_rows_wide(T(torch, KEYS[order]), new, count=torch.full((1,), 11, dtype=torch.int64, device="cuda"))
  keys, outs, _, cnt = t.fetch_planned_wide(plan, default_row=default_row)
  for f, got in enumerate(in_key_order(torch, keys, cnt, outs)):
    if new[f] is not None:   # (a None field: a resident key keeps its bytes, a new key starts at aux_init — what `want` holds)
      want[f][written] = new[f][:11].cpu().to(t.value_dtype).cuda().to(torch.float32)   # one rounding: torch's cast on the CPU
    assert torch.equal(got.view(torch.int32), want[f].view(torch.int32)), f
  t.check_errors()
  assert t.size_host() == RESIDENT.size + int((order[:11] % 2 == 1).sum()), "the size grew by the never-seen keys that were written"


def test_store_into_a_full_lru_table(env):
  """A full 1024-slot LRU table at max_capacity and 100 never-seen unique keys: every one ends resident (LRU admits every new key) with its
  rounded row, field 1 at aux_init; the size does not move; no error.  (Which old keys leave depends on the order the groups run in.)"""
  torch, de = env
  dim, B = 260, 100
  t, _ = make_table(torch, "bfloat16", dim, 2, strategy=0, cap=1024)
  for part in np.array_split(-np.arange(1, 4 * t.capacity() + 1, dtype=np.int64), 8):   # (in parts, as tests/test_gpu_generic_rows.py fills its table)
    t.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=t.value_dtype), unique_keys=True)
  assert t.slot_census()["empty"] == 0
  size0 = t.size_host()
  keys = T(torch, np.arange(B, dtype=np.int64) * 7919 + 13)
  g = torch.Generator(device="cuda").manual_seed(1)
  fields = [torch.randn((B, dim), generator=g, device="cuda") * 3, None, torch.randn((B, dim), generator=g, device="cuda")]
  t.store_rows_wide(keys, fields)
  t.check_errors()
  assert t.size_host() == size0 and bool(t.contains(keys).all())
  for f, x in enumerate(fields):
    want = torch.full((B, dim), AUX_INIT[f - 1]).to(t.value_dtype) if x is None else x.cpu().to(t.value_dtype)
    assert torch.equal(t.find(keys, field=f).cpu().view(torch.int16), want.view(torch.int16)), f


def adamw(step, p, g, m, v):
  m = m * 0.9 + g * 0.1
  v = v * 0.999 + g * g * 0.001
  return p - 0.01 * (m / (v.sqrt() + 1e-8) + 0.01 * p), m, v


def train(torch, de, monkeypatch, rule, vdtype, dim, whole_rows, **kw):
  """three apply_sparse steps on exact-sum gradients over a fresh variable -> (C calls by name, [keys, rows, slots ...])"""
  opt = (de.optimizers.Momentum(0.05, 0.9, whole_rows=whole_rows) if rule == "momentum" else
         de.optimizers.Generic(slots=("m", "v"), slot_init=(0.0, 0.0), update=adamw, whole_rows=whole_rows))
  _serial[0] += 1
  var = de.Variable(dim=dim, name="grw_v%d" % _serial[0], value_dtype=getattr(torch, vdtype), initializer=DEFAULT,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
  var.upsert(T(torch, RESIDENT), torch.full((RESIDENT.size, dim), 0.25, device="cuda").to(var.value_dtype))
  deo = de.DynamicEmbeddingOptimizer(opt, **kw)
  ids = batch(torch, dim)[0]
  g = torch.Generator(device="cuda").manual_seed(dim)
  c = Calls(monkeypatch)
  for _ in range(3):
    deo.apply_sparse(var, ids, torch.randint(-4, 5, (ids.numel(), dim), generator=g, device="cuda").float() / 8)
  monkeypatch.undo()
  var.tables[0]._table.check_errors()
  keys = torch.sort(var.export()[0])[0]
  made = {k: v for k, v in c.n.items() if k.split("tfra_table_")[-1].startswith(("fetch", "store")) or "unique" in k or k == "tfra_segment_sum"}
  return made, [keys, var.lookup(keys)] + [deo.get_slot(var, s).lookup(keys) for s in opt.slots]


ROUTES = [(r, v, d, dict(wide_rows=True)) for v, d in (("float32", 260), ("bfloat16", 1024)) for r in ("momentum", "adamw")] + [
    ("momentum", "float32", d, kw) for d, kw in ((512, dict(wide_rows=False)), (64, dict(wide_rows=True)), (512, dict(wide_rows=True, exact_order=True)))]


@pytest.mark.parametrize("rule,vdtype,dim,kw", ROUTES)
def test_whole_rows_route_against_the_default_route(env, monkeypatch, rule, vdtype, dim, kw):
  """whole_rows=True with wide_rows=True on a wide variable: the two wide calls per step and nothing else; every other
  configuration: the calls it made before the wide row calls existed.  Rows and slots bit for bit those of whole_rows=False."""
  torch, de = env
  made, got = train(torch, de, monkeypatch, rule, vdtype, dim, True, **kw)
  if dim > 256 and kw == dict(wide_rows=True):
    assert made == {"tfra_table_fetch_planned_wide": 3, "tfra_table_store_rows_wide": 3}, made
  else:   # (wide_rows changed nothing for these: the calls of the same configuration without it)
    assert not any(k.endswith("_wide") for k in made), made
    assert made == train(torch, de, monkeypatch, rule, vdtype, dim, dim == 64, **dict(kw, wide_rows=False))[0]
  want = train(torch, de, monkeypatch, rule, vdtype, dim, False, **kw)[1]
  bits = torch.int32 if vdtype == "float32" else torch.int16
  assert len(got) == len(want) and all(torch.equal(a.view(bits), b.view(bits)) for a, b in zip(got[1:], want[1:]))
  assert torch.equal(got[0], want[0]) and got[0].numel() == KEYS.size


WIDTH = "256 < dim <= 1024 (dim <= 256: tfra_table_"
@pytest.mark.parametrize("dim,half,code,words", [(256, False, -6, WIDTH), (1028, False, -6, WIDTH), (512, True, -6, "half gradients are up-cast by the caller"),
                                                 (768, False, -1, "the plan was built for another dim")])
def test_refusals_leave_the_table_alone(env, dim, half, code, words):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding._args import _ptr, _stream
  lib, s = _capi.lib(), _stream(torch.device("cuda", 0))
  plan = batch(torch, 512)[1]
  t, rows = make_table(torch, "float32", dim, 0)
  keys, cnt = torch.empty(plan.n, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
  out, G = torch.full((plan.n, dim), -7.5, device="cuda"), torch.ones((plan.n, dim), device="cuda", dtype=torch.bfloat16 if half else torch.float32)
  rf, rec = t._row_fields([out]), _capi.Grads(G.data_ptr(), _capi.TFRA_BF16 if half else _capi.TFRA_F32, 0, None)
  torch.cuda.synchronize()
  calls = [("tfra_table_fetch_planned_wide", (t._h, plan._h, ctypes.byref(rec), _ptr(t._default_value), _ptr(keys), ctypes.byref(rf), _ptr(out), _ptr(cnt), s))]
  if dim in (256, 1028):
    calls.append(("tfra_table_store_rows_wide", (t._h, plan.n, None, _ptr(plan.ids), ctypes.byref(rf), s)))
  for name, args in calls:
    rc, msg = getattr(lib, name)(*args), lib.tfra_last_error().decode()
    assert rc == code and msg.startswith(name + ": ") and words in msg, (name, rc, msg)
  torch.cuda.synchronize()
  assert bool((out == -7.5).all()) and t.size_host() == RESIDENT.size and torch.equal(t.find(T(torch, RESIDENT)), rows[0])
