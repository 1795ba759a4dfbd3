"""GPU: whole rows out and back — tfra_table_fetch_planned, tfra_table_store_rows and the optimizers' whole_rows route.

Every comparison is bit for bit (tests/numeric_edges.py: assert_bits — equal bits, or a NaN where a NaN is expected) and is made
against entry points that existed before these calls: tfra_table_find_field and tfra_reduce_by_key[_typed] for the fetch,
tfra_table_insert_or_assign + tfra_table_insert_field on a twin table for the store, torch's CPU cast for the rounding, and the
default `Generic` route on a twin variable for the optimizer."""
import ctypes

import numpy as np
import pytest

from tests import numeric_edges as ne
from tests import probe_model as pm

pytestmark = pytest.mark.gpu

IMIN = -2**63
REPEATS = (1, 2, 8, 9, 17, 600)   # the plan's few / many boundary (8 | 9), a second item (17), a second 512-entry chunk (600)
AUX_INIT = (0.1, -1.7, 3.3, 0.7)  # none of them a float16 / bfloat16 value: the stored image is not the float
DEFAULT = 0.3
SENT = -7.5
VDTYPES = ["float32", "float16", "bfloat16"]
DIMS = [4, 68, 256]
AUXES = [0, 1, 2, 4]
LRU, LFU = 0, 1


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture
def calls(monkeypatch):
  from tests.sparse_helpers import Calls
  return Calls(monkeypatch)


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_serial = [0]


def make_table(torch, vdtype, dim, aux, tag, strategy=-1, cap=0, init=8192):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  _serial[0] += 1
  dt = getattr(torch, vdtype)
  return _DeviceTable(torch.int64, dt, torch.full((dim,), DEFAULT).to(dt), "gr_%s_%d" % (tag, _serial[0]), "cuda:0", dim=dim,
                      aux_fields=aux, init_capacity=cap or init, max_capacity=cap, strategy=strategy, aux_init=AUX_INIT)


def stored(torch, x, vdtype):
  """float32 device tensor -> the table's value dtype, ONE rounding to nearest even: torch's cast, computed on the CPU."""
  return x.detach().cpu().to(getattr(torch, vdtype)).cuda()


def aux_default(torch, t, f):
  """The table's stored image of aux_init[f - 1]: the FLOAT rounded to the value dtype once, one row."""
  return torch.full((t.dim,), AUX_INIT[f - 1], dtype=torch.float32).to(t.value_dtype).cuda()


def find_all(torch, t, keys, default_row=None):
  """Every field of `keys` through tfra_table_find / tfra_table_find_field with the defaults of the fetch's contract, up-cast."""
  out = []
  for f in range(1 + t._aux_fields):
    d = (t._default_value if default_row is None else default_row) if f == 0 else aux_default(torch, t, f)
    out.append(t.find(keys, d, field=f).to(torch.float32))
  return out


def table_state(torch, t):
  k, v, _ = t.export_all()
  o = torch.argsort(k)
  return t.size_host(), k[o].cpu(), v[o].cpu()


def assert_same_state(torch, t, before, what):
  torch.cuda.synchronize()
  t.check_errors()
  n, k, v = table_state(torch, t)
  assert n == before[0] and torch.equal(k, before[1]), what
  ne.assert_bits(torch, v, before[2], what + ": exported rows")


def rand_rows(torch, rng, n, dim, vdtype):
  return T(torch, ne.through_storage(torch, (rng.standard_normal((n, dim)) * 3).astype(np.float32), vdtype)).to(getattr(torch, vdtype))


def seed_table(torch, t, rng, keys, vdtype):
  """Resident rows: field 0 by insert_or_assign, every slot field by insert_field, random storage values."""
  kt = T(torch, keys)
  t.upsert(kt, rand_rows(torch, rng, keys.size, t.dim, vdtype), unique_keys=True)
  for f in range(1, 1 + t._aux_fields):
    t.upsert(kt, rand_rows(torch, rng, keys.size, t.dim, vdtype), unique_keys=True, field=f)


def repeat_batch(rng):
  """Per repeat count one resident and one never-seen key, and both reserved key values (INT64_MIN resident, INT64_MIN + 1 not,
  each twice) -> (resident keys, ids shuffled)."""
  res = ne.row_keys(len(REPEATS), stride=104729, base=7)
  absent = ne.row_keys(len(REPEATS), stride=15485863, base=-999)
  ids = np.concatenate([np.repeat(res, REPEATS), np.repeat(absent, REPEATS), np.array([IMIN, IMIN + 1] * 2, np.int64)])
  rng.shuffle(ids)
  return np.append(res, IMIN), ids


def raw_fetch(torch, t, plan, rec, default_row, want, with_sums):
  """tfra_table_fetch_planned into sentinel-filled buffers of the plan's n rows."""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding._args import _ptr, _stream
  n, dim = plan.n, t.dim
  keys = torch.full((n,), -7, dtype=torch.int64, device="cuda")
  bufs = [torch.full((n, dim), SENT, dtype=torch.float32, device="cuda") for _ in want]
  gsum = torch.full((n, dim), SENT, dtype=torch.float32, device="cuda")
  cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
  rf = t._row_fields([b if w else None for b, w in zip(bufs, want)])
  torch.cuda.synchronize()
  _capi.call("tfra_table_fetch_planned", t._h, plan._h, ctypes.byref(rec) if with_sums else None, _ptr(default_row), _ptr(keys),
             ctypes.byref(rf), _ptr(gsum) if with_sums else None, _ptr(cnt), _stream(t._device))
  torch.cuda.synchronize()
  return keys, bufs, gsum, int(cnt)


def gradient_kinds(torch, rng, n, dim):
  """(name, tensor, grad_scale): float32; bfloat16; float16 with a scale."""
  g = (rng.standard_normal((n, dim)) * 2).astype(np.float32)
  scale = torch.full((1,), 1.0 / 1024, dtype=torch.float32, device="cuda")
  return [("float32", T(torch, g), None), ("bfloat16", T(torch, g).to(torch.bfloat16), None),
          ("float16_scaled", T(torch, g * 512).to(torch.float16), scale)]


# ---- 1. the fetch against find_field and reduce_by_key -------------------------------------------------------------------------------
@pytest.mark.parametrize("aux", AUXES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("vdtype", VDTYPES)
def test_fetch_against_find_field_and_reduce_by_key(env, vdtype, dim, aux):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import device_ops
  from tfra_amd.dynamic_embedding._args import _grads_arg
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  rng = np.random.default_rng(dim * 10 + aux)
  t = make_table(torch, vdtype, dim, aux, "fetch")
  res, ids = repeat_batch(rng)
  seed_table(torch, t, rng, res, vdtype)
  before = table_state(torch, t)
  it = T(torch, ids)
  n, nf = ids.size, 1 + aux
  default_row = torch.full((dim,), 0.6).to(t.value_dtype).cuda()   # not the table's own default: the call's argument is what counts
  plan = SparsePlan("cuda:0", dim).build(it)
  U = np.unique(ids).size
  for name, g, scale in gradient_kinds(torch, rng, n, dim):
    what = "%s dim %d aux %d, %s gradients" % (vdtype, dim, aux, name)
    rkeys, rsums, rcnt = device_ops.reduce_by_key(it, g, grad_scale=scale)
    assert int(rcnt) == U
    typed, gt = _grads_arg(g, t._device, dim, scale)
    rec = typed if typed is not None else _capi.Grads(gt.data_ptr(), _capi.TFRA_F32, 0, None)
    keys, bufs, gsum, cnt = raw_fetch(torch, t, plan, rec, default_row, [True] * nf, True)
    assert cnt == U, what
    o = torch.argsort(keys[:U])
    ks = keys[:U][o]
    assert torch.equal(ks.cpu(), torch.from_numpy(np.unique(ids))), what
    ne.assert_bits(torch, gsum[:U][o], rsums[:U][torch.argsort(rkeys[:U])], what + ": gsum")
    for f, (got, want) in enumerate(zip(bufs, find_all(torch, t, ks, default_row))):
      ne.assert_bits(torch, got[:U][o], want, what + ": field %d" % f)
      assert bool((got[U:] == SENT).all()), what + ": rows at or beyond U keep the sentinel (field %d)" % f
    assert bool((gsum[U:] == SENT).all()) and bool((keys[U:] == -7).all()), what
  # NULL fields are neither read nor written; g == NULL fetches rows only
  for want in ([True] + [False] * aux, [False] * nf, [False] + [True] * aux):
    keys, bufs, gsum, cnt = raw_fetch(torch, t, plan, None, default_row, want, False)
    assert cnt == U and bool((gsum == SENT).all())
    o = torch.argsort(keys[:U])
    ref = find_all(torch, t, keys[:U][o], default_row)
    for f in range(nf):
      if want[f]:
        ne.assert_bits(torch, bufs[f][:U][o], ref[f], "rows only, mask %r: field %d" % (want, f))
      else:
        assert bool((bufs[f] == SENT).all()), "a NULL field's buffer keeps the sentinel (mask %r, field %d)" % (want, f)
  # the Python method: the same rows, gradients through _grads_arg
  name, g, scale = gradient_kinds(torch, rng, n, dim)[2]
  keys, outs, gsum, cnt = t.fetch_planned(plan, grads=g, grad_scale=scale, default_row=default_row)
  rkeys, rsums, _ = device_ops.reduce_by_key(it, g, grad_scale=scale)
  assert int(cnt) == U
  o = torch.argsort(keys[:U])
  assert torch.equal(keys[:U][o], torch.sort(rkeys[:U])[0])
  ne.assert_bits(torch, gsum[:U][o], rsums[:U][torch.argsort(rkeys[:U])], "fetch_planned: gsum")
  for f, want in enumerate(find_all(torch, t, keys[:U][o], default_row)):
    ne.assert_bits(torch, outs[f][:U][o], want, "fetch_planned: field %d" % f)
  assert_same_state(torch, t, before, "after the fetches")


def test_fetch_leaves_an_lru_table_alone(env):
  """Scores, size, rows and the error count of an LRU table are what they were."""
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  dim = 8
  tab = de.HkvHashTable(torch.int64, torch.float32, torch.full((dim,), DEFAULT), name="gr_lru", init_capacity=8192, max_capacity=8192,
                        max_hbm_for_values=1 << 26, evict_strategy=de.HkvEvictStrategy.LRU, device="cuda:0", dim=dim, aux_fields=1)
  rng = np.random.default_rng(5)
  res, ids = repeat_batch(rng)
  tab.insert(T(torch, res[:-1]), T(torch, rng.standard_normal((res.size - 1, dim)).astype(np.float32)))
  def scores():
    k, s = tab.export_keys_and_scores(4096)
    o = torch.argsort(k)
    return k[o].cpu(), s[o].cpu()
  before, k0 = table_state(torch, tab._table), scores()
  plan = SparsePlan("cuda:0", dim).build(T(torch, ids))
  keys, outs, gsum, cnt = tab.fetch_planned(plan, grads=T(torch, rng.standard_normal((ids.size, dim)).astype(np.float32)))
  assert int(cnt) == np.unique(ids).size and gsum is not None and len(outs) == 2
  assert_same_state(torch, tab._table, before, "LRU table after a fetch")
  k1 = scores()
  assert torch.equal(k0[0], k1[0]) and torch.equal(k0[1], k1[1]), "a fetch touches no score"


# ---- 2. the fetch on probe chains -----------------------------------------------------------------------------------------------------
def test_fetch_on_an_overflow_chain_with_a_hole(env):
  """52 keys that share both home buckets (A, B) fill A, B, B + 1 and reach B + 2; eight of those that sit in B are erased, which
  leaves a hole in the middle of the chain (the flags stay).  Every resident key's fields are found, every absent key of the same
  homes — the erased ones and twelve never inserted — gets the defaults."""
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  dim, aux, vdtype = 8, 2, "float32"
  t = make_table(torch, vdtype, dim, aux, "chain", init=1000)
  nb = (t.capacity() - 2) // pm.SLOTS
  a, b = 5, nb // 2
  crafted = pm.craft(nb, b0=a, b1=b, substituted=False, count=64)
  chain, never = crafted[:52], crafted[52:]
  rng = np.random.default_rng(9)
  model = pm.FirstFit(nb)
  for part in np.array_split(chain, chain.size):   # one key per call: in one launch the order of arrival is free, here the model's holds
    seed_table(torch, t, rng, part, vdtype)
    for k in part:
      model.insert(k)
  depth = np.array([model.depth_of(k) for k in chain])
  assert depth.max() >= 3, "the chain is several buckets deep"
  assert (t.capacity() - 2) // pm.SLOTS == nb, "the table has not grown"
  placed = find_all(torch, t, T(torch, chain))
  assert bool(t.find(T(torch, chain), return_exists=True)[1].all())
  # eight keys that sit in B, the second bucket of the chain
  hole = chain[depth == 1][:8]
  assert hole.size == 8
  t.erase(T(torch, hole))
  live = np.setdiff1d(chain, hole)
  absent = np.concatenate([hole, never])
  ids = np.concatenate([live, absent, live[:7]])
  rng.shuffle(ids)
  before = table_state(torch, t)
  plan = SparsePlan("cuda:0", dim).build(T(torch, ids))
  keys, outs, _, cnt = t.fetch_planned(plan)
  U = int(cnt)
  assert U == live.size + absent.size
  o = torch.argsort(keys[:U])
  ks = keys[:U][o]
  ref = find_all(torch, t, ks)
  is_live = torch.from_numpy(np.isin(ks.cpu().numpy(), live))
  for f in range(1 + aux):
    ne.assert_bits(torch, outs[f][:U][o], ref[f], "chain: field %d" % f)
    want_default = (t._default_value if f == 0 else aux_default(torch, t, f)).to(torch.float32).cpu()
    got = outs[f][:U][o].cpu()
    ne.assert_bits(torch, got[~is_live], want_default.expand(int((~is_live).sum()), dim), "chain: absent keys get the defaults (field %d)" % f)
    pos = {int(k): i for i, k in enumerate(chain)}
    rows = torch.tensor([pos[int(k)] for k in ks[is_live].cpu()])
    ne.assert_bits(torch, got[is_live], placed[f].cpu()[rows], "chain: resident keys keep their fields (field %d)" % f)
  assert_same_state(torch, t, before, "chain table after the fetch")


# ---- 3. the store against insert_or_assign + insert_field ------------------------------------------------------------------------------
def sequence(torch, t, keys, fields, vdtype):
  """The sequence of the store's contract through the entry points it names."""
  t.upsert(keys, stored(torch, fields[0], vdtype), unique_keys=True)
  for f in range(1, len(fields)):
    if fields[f] is not None:
      t.upsert(keys, stored(torch, fields[f], vdtype), unique_keys=True, field=f)


def assert_twin_tables(torch, a, b, keys, what):
  torch.cuda.synchronize()
  a.check_errors(); b.check_errors()
  sa, sb = table_state(torch, a), table_state(torch, b)
  assert sa[0] == sb[0] and torch.equal(sa[1], sb[1]), what + ": the same keys"
  ne.assert_bits(torch, sb[2], sa[2], what + ": exported rows")
  for f, (x, y) in enumerate(zip(find_all(torch, a, keys), find_all(torch, b, keys))):
    ne.assert_bits(torch, y, x, what + ": field %d" % f)


@pytest.mark.parametrize("aux", AUXES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("vdtype", VDTYPES)
def test_store_against_the_sequence_on_a_twin(env, vdtype, dim, aux):
  torch, de = env
  rng = np.random.default_rng(dim * 100 + aux)
  n = 300
  res = np.append(ne.row_keys(n // 2, stride=104729, base=7), IMIN)
  new = np.append(ne.row_keys(n // 2, stride=15485863, base=-999), IMIN + 1)
  keys = np.concatenate([res, new])
  rng.shuffle(keys)
  kt = T(torch, keys)
  twins = []
  for which in "AB":
    t = make_table(torch, vdtype, dim, aux, "store" + which)
    seed_table(torch, t, np.random.default_rng(1), res, vdtype)
    twins.append(t)
  a, b = twins
  rows = lambda: T(torch, (rng.standard_normal((keys.size, dim)) * 3).astype(np.float32))
  # all fields given
  fields = [rows() for _ in range(1 + aux)]
  sequence(torch, a, kt, fields, vdtype)
  b.store_rows(kt, fields)
  assert_twin_tables(torch, a, b, kt, "%s dim %d aux %d: all fields" % (vdtype, dim, aux))
  # NULL fields (a resident key keeps its bytes, a new key starts at aux_init), d_n smaller than n: nothing beyond it is written
  more = np.concatenate([keys[:100], ne.row_keys(100, stride=7919, base=5_000_000_007)])
  mt = T(torch, more)
  m = 150
  fields = [T(torch, (rng.standard_normal((more.size, dim)) * 3).astype(np.float32)) if f % 2 == 0 else None for f in range(1 + aux)]
  sequence(torch, a, mt[:m], [None if x is None else x[:m] for x in fields], vdtype)
  b.store_rows(mt, fields, count=torch.full((1,), m, dtype=torch.int64, device="cuda"))
  allk = T(torch, np.concatenate([keys, more]))
  assert_twin_tables(torch, a, b, allk, "%s dim %d aux %d: NULL fields, d_n = %d of %d" % (vdtype, dim, aux, m, more.size))
  assert not bool(b.contains(mt[m:]).any()), "keys beyond d_n are not written"
  # a negative count writes nothing
  before = table_state(torch, b)
  b.store_rows(mt, [x if x is not None else None for x in fields], count=torch.full((1,), -3, dtype=torch.int64, device="cuda"))
  assert_same_state(torch, b, before, "a negative d_n")


def test_store_counts_one_upsert_on_an_lfu_table(env):
  """The stated score difference: the sequence counts 1 + S upserts of a key, the store one."""
  torch, de = env
  dim, aux, vdtype = 8, 2, "float32"
  keys = T(torch, ne.row_keys(200))
  fields = [torch.rand((200, dim), device="cuda") for _ in range(1 + aux)]
  got = []
  for which in "AB":
    t = make_table(torch, vdtype, dim, aux, "lfu" + which, strategy=LFU, cap=1 << 16)
    for _ in range(2):   # new keys, then resident ones
      if which == "A":
        sequence(torch, t, keys, fields, vdtype)
      else:
        t.store_rows(keys, fields)
    torch.cuda.synchronize()
    t.check_errors()
    k, v, s = t.export_all(with_scores=True)
    got.append((k[torch.argsort(k)].cpu(), s.cpu()))
  assert torch.equal(got[0][0], got[1][0])
  assert bool((got[0][1] == 2 * (1 + aux)).all()), "the sequence: 1 + S per call"
  assert bool((got[1][1] == 2).all()), "the store: ONE upsert per call"


# ---- 4. the rounding of the store -------------------------------------------------------------------------------------------------------
def rounding_values(vdtype):
  """float32: the value of every one of the 65 536 stored patterns, then, with both signs, the midpoint of every pair of neighbouring
  finite magnitudes and of the largest one and the power of two above it (the tie that goes to infinity)."""
  pats = ne.upcast_bits(np.arange(65536, dtype=np.uint16), vdtype)
  top = 0x7c00 if vdtype == "float16" else 0x7f80
  mags = np.append(ne.upcast_bits(np.arange(top, dtype=np.uint16), vdtype).astype(np.float64), 2.0 ** (16 if vdtype == "float16" else 128))
  mid64 = (mags[:-1] + mags[1:]) / 2
  mid = mid64.astype(np.float32)
  assert np.array_equal(mid.astype(np.float64), mid64)   # one more significant bit than the format: exact in float32
  return np.concatenate([pats, mid, -mid])


@pytest.mark.parametrize("stochastic", [False, True], ids=["nearest", "stochastic_option_set"])
@pytest.mark.parametrize("vdtype", ["float16", "bfloat16"])
def test_store_rounds_once_to_nearest_even(env, vdtype, stochastic):
  torch, de = env
  dim = 64
  x = rounding_values(vdtype)
  rows = ne.pack_rows(x, dim, 0.0)
  t = make_table(torch, vdtype, dim, 0, "round")
  if stochastic:
    t.set_stochastic_rounding(0x5EED0000C0FFEE11)   # upserts keep nearest even
  keys = T(torch, ne.row_keys(rows.shape[0]))
  t.store_rows(keys, [T(torch, rows)])
  torch.cuda.synchronize()
  t.check_errors()
  want = torch.from_numpy(rows).to(getattr(torch, vdtype))   # torch's cast on the CPU
  flat = rows.reshape(-1)
  ne.assert_bits(torch, t.find(keys).cpu(), want, "%s store" % vdtype, lambda i: "x = %r / %08x" % (float(flat[i]), int(flat[i:i + 1].view(np.uint32)[0])))
  assert t.size_host() == rows.shape[0]


# ---- 5. a full table ------------------------------------------------------------------------------------------------------------------------
def test_store_into_a_full_lru_table(env):
  """An 8192-slot LRU table at max_capacity without an empty slot, and a batch of 2047 distinct never-seen keys: all of them are
  resident afterwards with the caller's fields (field 1 NULL: at aux_init), the size is unchanged, no error is counted, and their
  rows equal those of the twin written by the contract's sequence.  (Which old keys leave is LRU's choice by the device clock of
  each table: the twins are compared on the batch.)"""
  torch, de = env
  dim, aux, vdtype, cap = 32, 2, "bfloat16", 8192
  rng = np.random.default_rng(77)
  B = 2047
  ids = ne.row_keys(B)
  rng.shuffle(ids)
  it = T(torch, ids)
  fields = [T(torch, (rng.standard_normal((B, dim)) * 3).astype(np.float32)), None, T(torch, rng.standard_normal((B, dim)).astype(np.float32))]
  out = []
  for which in "AB":
    t = make_table(torch, vdtype, dim, aux, "full" + which, strategy=LRU, cap=cap)
    old = -np.arange(1, 4 * t.capacity() + 1, dtype=np.int64)
    for part in np.array_split(old, 8):
      t.upsert(T(torch, part), torch.full((part.size, dim), 0.5, device="cuda", dtype=t.value_dtype), unique_keys=True)
    census = t.slot_census()
    assert census["empty"] == 0 and census["locked"] == 0
    size0 = t.size_host()
    if which == "A":
      sequence(torch, t, it, fields, vdtype)
    else:
      t.store_rows(it, fields)
    torch.cuda.synchronize()
    t.check_errors()
    assert t.size_host() == size0, "a full table keeps its size"
    present = int(t.contains(it).sum())
    print("full table, twin %s: %d of %d batch keys present" % (which, present, B))
    assert present == B, "an LRU table admits every new key"
    out.append(find_all(torch, t, it))
  want = [stored(torch, fields[0], vdtype).float(), aux_default(torch, t, 1).float().expand(B, dim), stored(torch, fields[2], vdtype).float()]
  for f in range(1 + aux):
    ne.assert_bits(torch, out[1][f], want[f], "full table: field %d is the caller's" % f)
    ne.assert_bits(torch, out[1][f], out[0][f], "full table: field %d against the twin" % f)


# ---- 6. the optimizer -------------------------------------------------------------------------------------------------------------------
def four_slots(step, p, g, a, b, c, d):
  import torch
  a = a * 0.9 + g
  b = b + g * g
  c = torch.maximum(c, g.abs())
  d = d * 0.5 - a * 0.01
  return p - a * 0.05 / (b.sqrt() + 1e-3) + d, a, b, c, d


def no_slots(step, p, g):
  return (p - g * 0.07,)


def make_rule(de, rule, whole_rows):
  o = de.optimizers
  if rule == "momentum":
    return o.Momentum(0.05, 0.9, whole_rows=whole_rows)
  if rule == "nesterov":
    return o.Momentum(0.05, 0.9, use_nesterov=True, whole_rows=whole_rows)
  if rule == "rmsprop":
    return o.RMSProp(0.01, 0.9, 0.5, whole_rows=whole_rows)
  if rule == "four_slots":
    return o.Generic(slots=("a", "b", "c", "d"), slot_init=(0.0, 0.1, 0.0, 0.3), update=four_slots, whole_rows=whole_rows)
  return o.Generic(update=no_slots, whole_rows=whole_rows)


RULES = ["momentum", "nesterov", "rmsprop", "four_slots", "no_slots"]


def zipf_steps(rng, dim, steps=3, n=3000, universe=900):
  """Zipf-1.2 ids over `universe` keys (a third of them are first seen in a later step) and their gradients."""
  keys = rng.permutation(np.arange(1, universe + 1, dtype=np.int64) * 7919 - 3_000_000)
  out = []
  for s in range(steps):
    r = np.minimum(rng.zipf(1.2, size=n), universe // 3 * (s + 1)) - 1
    out.append((keys[r], (rng.standard_normal((n, dim)) * 0.5).astype(np.float32)))
  return keys, out


def var_state(torch, de, deo, var, keys):
  k, v = var.export()
  o = torch.argsort(k)
  kt = T(torch, keys)
  return [k[o].cpu(), v[o].cpu()] + [var.lookup(kt).cpu()] + [deo.get_slot(var, s).lookup(kt).cpu() for s in deo.opt.slots]


def assert_same_vars(torch, a, b, what):
  assert torch.equal(a[0], b[0]), what + ": the same keys"
  for i, (x, y) in enumerate(zip(a[1:], b[1:])):
    ne.assert_bits(torch, y, x, "%s: state %d" % (what, i))


def train(torch, de, calls, var, deo, batches, kind, watch):
  """Three steps of apply_sparse; -> the C calls made, by name."""
  scale = torch.full((1,), 1.0 / 256, dtype=torch.float32, device="cuda")
  n0 = {w: calls[w] for w in watch}
  for ids, g in batches:
    if kind == "float32":
      deo.apply_sparse(var, T(torch, ids), T(torch, g))
    else:
      deo.apply_sparse(var, T(torch, ids), T(torch, g * 256).to(torch.bfloat16), grad_scale=scale)
  torch.cuda.synchronize()
  return {w: calls[w] - n0[w] for w in watch}


WATCH = ("tfra_table_fetch_planned", "tfra_table_store_rows", "tfra_table_find_field", "tfra_table_insert_field", "tfra_table_find",
         "tfra_table_insert_or_assign", "tfra_reduce_by_key", "tfra_sparse_plan_build")


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("vdtype", VDTYPES)
def test_whole_rows_twin_variables(env, calls, vdtype, dim, rule):
  torch, de = env
  for kind in ("float32", "bfloat16_scaled"):
    keys, batches = zipf_steps(np.random.default_rng(dim), dim)
    states = []
    for whole in (False, True):
      opt = make_rule(de, rule, whole)
      _serial[0] += 1
      var = de.Variable(dim=dim, name="gr_opt_%d" % _serial[0], value_dtype=getattr(torch, vdtype), initializer=DEFAULT,
                        **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
      deo = de.DynamicEmbeddingOptimizer(opt)
      made = train(torch, de, calls, var, deo, batches, kind, WATCH)
      if whole:
        assert made["tfra_table_fetch_planned"] == 3 and made["tfra_table_store_rows"] == 3, made
        assert made["tfra_sparse_plan_build"] == 3, made
        assert all(made[w] == 0 for w in WATCH[2:7]), made
      else:
        assert made["tfra_table_fetch_planned"] == 0 and made["tfra_table_store_rows"] == 0, made
        assert made["tfra_table_find_field"] == 3 * len(opt.slots) and made["tfra_table_insert_field"] == 3 * len(opt.slots), made
      var.tables[0]._table.check_errors()
      states.append(var_state(torch, de, deo, var, keys))
    assert_same_vars(torch, states[0], states[1], "%s dim %d %s, %s gradients" % (vdtype, dim, rule, kind))


@pytest.mark.parametrize("how", ["two_shards", "tiered", "exact_order"])
def test_everything_else_keeps_the_old_route(env, calls, how):
  torch, de = env
  dim = 8
  keys, batches = zipf_steps(np.random.default_rng(3), dim)
  states = []
  for whole in (False, True):
    opt = make_rule(de, "rmsprop", whole)
    _serial[0] += 1
    kw = dict(dim=dim, name="gr_old_%s_%d" % (how, _serial[0]), initializer=DEFAULT, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    if how == "two_shards":
      kw["devices"] = ["cuda:0"] * 2
    if how == "tiered":
      kw["kv_creator"] = de.TieredHashTableCreator(de.TieredHashTableConfig(
          upper=de.HkvHashTableConfig(init_capacity=4096, max_capacity=4096, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=1 << 14))
    var = de.Variable(**kw)
    deo = de.DynamicEmbeddingOptimizer(opt, exact_order=(how == "exact_order"))
    made = train(torch, de, calls, var, deo, batches, "float32", WATCH)
    assert made["tfra_table_fetch_planned"] == 0 and made["tfra_table_store_rows"] == 0, made
    assert made["tfra_table_find_field"] > 0 and made["tfra_table_insert_field"] > 0, made
    states.append(var_state(torch, de, deo, var, keys))
  assert_same_vars(torch, states[0], states[1], how)


def test_the_wrappers_plan_is_consumed_and_returned(env, calls):
  """plan_writeback=True: the plan built at lookup time serves the fetch (no second build) and goes back to the variable's pool."""
  torch, de = env
  dim = 16
  keys, batches = zipf_steps(np.random.default_rng(4), dim, n=10000)   # (a plan at lookup time wants 8192 ids or more)
  states = []
  for whole in (False, True):
    opt = make_rule(de, "momentum", whole)
    _serial[0] += 1
    var = de.Variable(dim=dim, name="gr_plan_%d" % _serial[0], initializer=DEFAULT, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    deo = de.DynamicEmbeddingOptimizer(opt)
    for ids, g in batches:
      n0 = {w: calls[w] for w in WATCH}
      emb, tw = de.embedding_lookup(var, T(torch, ids), return_trainable=True, plan_writeback=True)
      had_plan = tw.plan is not None
      deo.apply_gradients([(T(torch, g), tw)])
      if whole:
        assert had_plan and tw.plan is None, "the wrapper's plan is taken"
        pool = var._plan_pool
        assert len(pool["free"]) == pool["made"] >= 1, "and returned to the pool"
        assert calls["tfra_sparse_plan_build"] - n0["tfra_sparse_plan_build"] == 1, "one build per step: the lookup's"
        assert calls["tfra_table_fetch_planned"] - n0["tfra_table_fetch_planned"] == 1
        assert calls["tfra_table_store_rows"] - n0["tfra_table_store_rows"] == 1
        assert calls["tfra_table_find_field"] == n0["tfra_table_find_field"] and calls["tfra_table_insert_field"] == n0["tfra_table_insert_field"]
    torch.cuda.synchronize()
    states.append(var_state(torch, de, deo, var, keys))
  assert_same_vars(torch, states[0], states[1], "plan_writeback")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_alone(env):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding._args import _ptr, _stream
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan, _DeviceTable
  lib = _capi.lib()
  dim, aux, n = 8, 1, 64
  t = make_table(torch, "float32", dim, aux, "refuse")
  rng = np.random.default_rng(2)
  keys = T(torch, ne.row_keys(n))
  seed_table(torch, t, rng, ne.row_keys(n), "float32")
  before = table_state(torch, t)
  s = _stream(t._device)
  plan = SparsePlan("cuda:0", dim).build(keys)
  set_plan = SparsePlan("cuda:0", 0).build(keys)
  other_dim = SparsePlan("cuda:0", 12).build(keys)
  never = SparsePlan("cuda:0", dim)
  ko = torch.empty(n, dtype=torch.int64, device="cuda")
  f0, f1 = torch.ones((n + 1, dim), device="cuda"), torch.ones((n + 1, dim), device="cuda")
  cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
  d = torch.full((dim + 4,), DEFAULT, device="cuda")
  g = torch.ones((n, dim), device="cuda")
  odd = f1.reshape(-1)[1:]
  assert odd.data_ptr() % 16 == 4
  ok = t._row_fields([f0, f1])
  def rf(n_fields=2, size=48, ptrs=None):
    r = _capi.RowFields()
    r.struct_size, r.n_fields = size, n_fields
    for i, p in enumerate(ptrs if ptrs is not None else [f0.data_ptr(), f1.data_ptr()][:n_fields]):
      r.field[i] = p
    return r
  i32 = _DeviceTable(torch.int64, torch.int32, torch.zeros(dim, dtype=torch.int32), "gr_i32", "cuda:0", dim=dim, aux_fields=1)
  dim6 = _DeviceTable(torch.int64, torch.float32, torch.zeros(6), "gr_dim6", "cuda:0", dim=6, aux_fields=1)
  torch.cuda.synchronize()
  grec = _capi.Grads(g.data_ptr(), _capi.TFRA_F32, 0, None)
  fetch = lambda tab=t, pl=plan, gr=None, dr=d, r=ok, gs=None: lib.tfra_table_fetch_planned(
      tab._h, pl._h, None if gr is None else ctypes.byref(gr), _ptr(dr), _ptr(ko), ctypes.byref(r), None if gs is None else _ptr(gs), _ptr(cnt), s)
  store = lambda tab=t, r=ok, nn=n, kk=keys: lib.tfra_table_store_rows(tab._h, nn, None, _ptr(kk), ctypes.byref(r), s)
  INVALID, UNSUPPORTED = -1, _capi.ERR_UNSUPPORTED
  cases = [
      ("fetch", fetch(pl=never), INVALID), ("fetch", fetch(pl=other_dim), INVALID), ("fetch", fetch(pl=set_plan), UNSUPPORTED),
      ("fetch", fetch(r=rf(n_fields=1)), INVALID), ("fetch", fetch(r=rf(size=40)), INVALID),
      ("fetch", fetch(r=rf(n_fields=1, ptrs=[f0.data_ptr(), f1.data_ptr()])), INVALID),
      ("fetch", fetch(r=rf(ptrs=[f0.data_ptr(), odd.data_ptr()])), UNSUPPORTED), ("fetch", fetch(dr=d[1:]), UNSUPPORTED),
      ("fetch", fetch(gr=grec), INVALID), ("fetch", fetch(gs=g), INVALID),
      ("fetch", fetch(gr=_capi.Grads(g.data_ptr(), _capi.TFRA_F32, 1, None), gs=g), INVALID),
      ("fetch", fetch(tab=i32), UNSUPPORTED), ("fetch", fetch(tab=dim6), UNSUPPORTED),
      ("store", store(r=rf(n_fields=1)), INVALID), ("store", store(r=rf(size=44)), INVALID),
      ("store", store(r=rf(ptrs=[None, f1.data_ptr()])), INVALID), ("store", store(r=rf(ptrs=[odd.data_ptr(), f1.data_ptr()])), UNSUPPORTED),
      ("store", store(nn=1 << 31), INVALID), ("store", store(tab=i32), UNSUPPORTED), ("store", store(tab=dim6), UNSUPPORTED),
  ]
  for i, (name, rc, code) in enumerate(cases):
    assert rc == code, (i, name, rc)
  # (the message of the last refusal of each call names it)
  assert fetch(pl=never) == INVALID and lib.tfra_last_error().decode().startswith("tfra_table_fetch_planned: ")
  assert store(r=rf(size=44)) == INVALID and lib.tfra_last_error().decode().startswith("tfra_table_store_rows: ")
  assert store(nn=0) == 0
  empty = SparsePlan("cuda:0", dim).build(keys[:0])
  assert fetch(pl=empty) == 0
  torch.cuda.synchronize()
  assert int(cnt) == 0, "a plan of 0 ids sets the count and does nothing else"
  assert_same_state(torch, t, before, "after the refusals")
  for x, y in zip(find_all(torch, t, keys), find_all(torch, t, keys)):
    ne.assert_bits(torch, x, y, "rows readable after the refusals")
