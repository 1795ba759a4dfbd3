"""GPU: the grouped weight gradients of the pooled lookups (tfra_multi_find_combine_backprop_weights and
tfra_multi_find_combine_ragged_backprop_weights) — ONE list whose members are plain tables of every launch class (float32 dims 8,
64, 72 and 132, float16 dim 128, bfloat16 dim 256), two tiers of tests/test_gpu_tier_pooled.py (`setup_of`: a full cache of
15 * 89 slots over a lower table that holds most keys alone), one table named twice and one tier's lower table named directly,
a descriptor with nnz == 0 and one with n_rows == 0.

Every member's batch has 35 rows (a block's last groups have no row) of 0, 1, 16, 17 and 40 entries (a second and a third batch
of 16 and a tail), absent ids, three entries in front of row 0 and four behind the last row.  Every dw_out is pre-filled with a
sentinel, and every comparison is bit for bit with the SINGLE call on that descriptor — a tier's with the tier call, a table's
with the table call.  Around the calls both tables of every tier and its statistics stay what they were."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_tier_pooled import COMB, INVALID, UNSUPPORTED, _unchanged, bits, setup_of
from tests.test_gpu_tier_weight_grad import cover_of

pytestmark = pytest.mark.gpu

COUNTS, CYCLES, FRONT, BACK = (0, 1, 16, 17, 40), 7, 3, 4
N_ROWS = len(COUNTS) * CYCLES                       # 35: three blocks of 16 row groups, the last with 3 rows
NNZ_IN = sum(COUNTS) * CYCLES                       # 518
NNZ = FRONT + NNZ_IN + BACK
SENTINEL = 12345.0
PLAIN = ((8, "float32"), (64, "float32"), (72, "float32"), (132, "float32"), (128, "float16"), (256, "bfloat16"))
TIERS = ((64, "float32"), (128, "float16"))
NAMES = {False: "tfra_multi_find_combine_backprop_weights", True: "tfra_multi_find_combine_ragged_backprop_weights"}
PRUNE, FILL = 1, 2


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


class Batch:
  pass


def _batch(torch, rng, ids, dim, vd):
  """A member's batch over `ids` (NNZ of them, as drawn by the caller); the ragged form reads the NNZ_IN entries in the rows."""
  b = Batch()
  counts = np.tile(np.array(COUNTS), CYCLES)
  seg = np.concatenate([np.full(FRONT, -1), np.repeat(np.arange(N_ROWS), counts), np.full(BACK, N_ROWS + 1)]).astype(np.int64)
  assert ids.size == seg.size == NNZ
  b.ids, b.seg = torch.from_numpy(ids).cuda(), torch.from_numpy(seg).cuda()
  b.splits_np = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  b.splits = torch.from_numpy(b.splits_np).cuda()
  w_rand = rng.uniform(0.1, 2.0, size=NNZ).astype(np.float32)
  w_mixed = rng.standard_normal(NNZ).astype(np.float32)
  w_mixed[rng.random(NNZ) < 0.2] = 0.0
  w_mixed[rng.random(NNZ) < 0.05] = np.nan
  w_mixed[seg == 2] = 0.0          # a row of 16 entries without a member under PRUNE, weight sum 0
  w_mixed[seg == 3] = -1.0         # a row of 17 entries, all negative
  assert np.isnan(w_mixed).sum() >= 5 and (w_mixed < 0).sum() >= 50 and (w_mixed == 0).sum() >= 50
  b.weights = {"none": None, "random": torch.from_numpy(w_rand).cuda(), "mixed": torch.from_numpy(w_mixed).cuda()}
  b.G = torch.from_numpy(rng.standard_normal((N_ROWS, dim)).astype(np.float32)).cuda()
  b.default_row = (0.5 + 0.25 * torch.arange(dim, dtype=torch.float32, device="cuda")).to(vd)
  return b


@pytest.fixture(scope="module")
def members(env):
  """[(owner, batch)]: six plain tables, two tiers, the first table again with another batch, the first tier's lower table; and the
  tiers' setups.  An owner has find_combine_weight_grad / find_combine_ragged_weight_grad, the single calls."""
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  rng = np.random.default_rng(2024)
  pool = np.unique(rng.integers(1, 2**40, size=800, dtype=np.int64))
  rng.shuffle(pool)
  keys, absent = pool[:600], pool[600:700]
  out = []
  for dim, vdtype in PLAIN:
    vd = getattr(torch, vdtype)
    t = _DeviceTable(torch.int64, vd, torch.zeros(dim), "wgm_%d_%s" % (dim, vdtype), "cuda:0", dim=dim, init_capacity=2048)
    t.upsert(torch.from_numpy(keys).cuda(), torch.from_numpy(rng.standard_normal((keys.size, dim)).astype(np.float32)).cuda().to(vd))
    t.check_errors()
    ids = np.where(rng.random(NNZ) < 0.85, rng.choice(keys, NNZ), rng.choice(absent, NNZ))
    out.append((t, _batch(torch, rng, ids, dim, vd)))
  setups = [setup_of(torch, dim, vdtype) for dim, vdtype in TIERS]
  for s, (dim, vdtype) in zip(setups, TIERS):
    b = _batch(torch, rng, s.ids[:NNZ].cpu().numpy(), dim, getattr(torch, vdtype))
    up, lo = s.upper.contains(b.ids), s.lower.contains(b.ids)      # (contains: a call that does not count in the tier's statistics)
    in_rows = (b.seg >= 0) & (b.seg < N_ROWS)
    for kind in (up & in_rows, ~up & lo & in_rows, ~up & ~lo & in_rows):
      assert int(kind.sum()) >= 60                                  # in the cache, only below, in neither
    out.append((s.tier, b))
  twice = _batch(torch, rng, out[0][1].ids.flip(0).cpu().numpy(), 8, torch.float32)
  out.append((out[0][0], twice))                                    # one table named twice
  out.append((setups[0].lower, out[len(PLAIN)][1]))                 # a tier's lower table named directly, the tier's batch
  _unchanged(torch, setups[0])
  return out, setups


def _tuple_req(owner, b, weights, c):
  return (owner, b.ids, b.seg, b.weights[weights], c, b.G, b.default_row)


def _ragged_req(owner, b, weights, c, prune=False, fill=None, splits=None):
  w = b.weights[weights]
  return (owner, b.splits if splits is None else splits, b.ids[FRONT:NNZ - BACK], None if w is None else w[FRONT:NNZ - BACK], c, b.G,
          prune, fill, b.default_row)


def _single(req, ragged):
  owner = req[0]
  if ragged:
    rs, ids, w, c, G, prune, fill, d = req[1:]
    return owner.find_combine_ragged_weight_grad(rs, ids, w, c, G, prune=prune, fill_id=fill, default_row=d)
  ids, seg, w, c, G, d = req[1:]
  return owner.find_combine_weight_grad(ids, seg, w, c, G, d)


def _extras(torch, members, ragged):
  """the two descriptors that enqueue no gradient: nnz == 0 (five rows) and n_rows == 0 (every entry is in no row)"""
  (p1, b1), (t0, bt) = members[1], members[len(PLAIN)]
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  if ragged:
    return [(p1, torch.zeros(6, dtype=torch.int64, device="cuda"), none, None, 1, b1.G[:5], False, None, b1.default_row),
            (t0, torch.zeros(1, dtype=torch.int64, device="cuda"), bt.ids, bt.weights["random"], 1, bt.G[:0], True, None, bt.default_row)]
  return [(p1, none, none, None, 1, b1.G[:5], b1.default_row),
          (t0, bt.ids, torch.zeros_like(bt.seg), bt.weights["random"], 1, bt.G[:0], bt.default_row)]


def _launches(torch, reqs, ragged):
  """the header's formula: (1 if any descriptor has nnz > 0) + the distinct classes among the descriptors with nnz > 0 and
  n_rows > 0 — (tiered or not, value dtype, NCH), ragged form: x (PRUNE with weights)"""
  from tfra_amd.dynamic_embedding import table_ops as T
  classes, any_nnz = set(), False
  for r in reqs:
    ids, w, G = (r[2] if ragged else r[1]), r[3], r[5]
    if ids.numel() == 0:
      continue
    any_nnz = True
    if G.shape[0] == 0:
      continue
    tier = T._device_tier(r[0])
    table = tier._upper if tier is not None else T._device_table(r[0])
    nch = 0 if table._dim <= 64 else 1 if table._dim <= 128 else 2
    classes.add((tier is not None, table._value_dtype, nch, bool(ragged and r[6] and w is not None)))
  return (1 if any_nnz else 0) + len(classes)


def _raw(torch, ragged, items):
  """One C call over descriptors made from `items`: dicts with req (a request as above), optionally dw (the tensor to write to
  instead of a sentinel-filled one of nnz floats) and over ({field: value} set last).  -> (code, message, launches, dws)"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import table_ops as T
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  desc_type = _capi.FindCombineRaggedWgradDesc if ragged else _capi.FindCombineWgradDesc
  descs = (desc_type * len(items))()
  keep, dws = [], []
  for e, it in zip(descs, items):
    e.struct_size = ctypes.sizeof(desc_type)
    table = T._pooled_owner(e, it["req"][0], True)
    if ragged:
      rs, ids, w, c, G, prune, fill, d = it["req"][1:]
      rs, ids, w, flags, fill_key, d, _ = table._find_combine_ragged_args(rs, ids, w, prune, fill, d)
      g = table._weight_grad_out(G, rs.numel() - 1)
      e.n_rows, e.row_splits, e.flags, e.reserved, e.fill_id = rs.numel() - 1, rs.data_ptr(), flags, 0, fill_key
      keep.append(rs)
    else:
      ids, seg, w, c, G, d = it["req"][1:]
      g = table._weight_grad_out(G, None)
      ids, seg, w, d, _ = table._find_combine_args(ids, seg, w, 0, d)
      e.n_rows, e.seg = g.shape[0], seg.data_ptr()
      keep.append(seg)
    dw = it["dw"] if "dw" in it else torch.full((ids.numel(),), SENTINEL, dtype=torch.float32, device="cuda")
    e.combiner, e.nnz, e.ids, e.weights = int(c), ids.numel(), ids.data_ptr(), (w.data_ptr() if w is not None else None)
    e.default_row, e.grad_out, e.dw_out = d.data_ptr(), g.data_ptr(), dw.data_ptr()
    for field, value in it.get("over", {}).items():
      setattr(e, field, value)
    keep += [ids, w, d, g]
    dws.append(dw)
  dev = torch.device("cuda:0")
  launches = ctypes.c_uint32(99)
  lib = _capi.lib()
  rc = getattr(lib, NAMES[ragged])(_workspace(dev), len(items), ctypes.c_void_p(ctypes.addressof(descs)),
                                   ctypes.c_void_p(ctypes.addressof(launches)), T._stream(dev))
  return rc, lib.tfra_last_error().decode(), launches.value, dws


def _sentinel(torch, n):
  return torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")


def _same(torch, many, reqs, ragged, what="", only=None):
  assert len(many) == len(reqs)
  for k, (got, req) in enumerate(zip(many, reqs)):
    want = _single(req, ragged)
    assert got.dtype == torch.float32 and got.shape == want.shape
    if only is None:
      assert torch.equal(bits(torch, got), bits(torch, want)), "descriptor %d %s" % (k, what)
    else:
      assert torch.equal(bits(torch, got[only]), bits(torch, want[only])), "descriptor %d %s" % (k, what)


def _run(torch, reqs, ragged, what="", only=None):
  """the raw call over `reqs` plus the two descriptors that enqueue no gradient, every dw_out pre-filled; -> the members' dws"""
  members_n = len(reqs)
  spare = _sentinel(torch, 16)                                       # handed to the nnz == 0 descriptor: it stays as it is
  extras = _extras_cache[ragged]
  items = [dict(req=r) for r in reqs] + [dict(req=extras[0], dw=spare), dict(req=extras[1])]
  rc, msg, launches, dws = _raw(torch, ragged, items)
  assert rc == 0, msg
  want = _launches(torch, reqs + extras, ragged)
  assert launches == want and launches < members_n, (launches, want)
  _same(torch, dws[:members_n], reqs, ragged, what, only)
  torch.cuda.synchronize()
  assert bool((spare == SENTINEL).all())                             # nnz == 0 writes nothing
  assert dws[-1].numel() == NNZ and not bool(bits(torch, dws[-1]).any())   # n_rows == 0 zero-fills dw_out
  return dws[:members_n]


_extras_cache = {}


@pytest.fixture(scope="module")
def listed(env, members):
  torch, _ = env
  ms, setups = members
  _extras_cache[False], _extras_cache[True] = _extras(torch, ms, False), _extras(torch, ms, True)
  return ms, setups


# ---- 1: bit identity per descriptor with the single call -------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["none", "random", "mixed"])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_every_descriptor_equals_its_single_call(env, listed, combiner, weights):
  torch, de = env
  T = de.table_ops
  ms, setups = listed
  c = COMB[combiner]
  reqs = [_tuple_req(o, b, weights, c) for o, b in ms]
  assert len(reqs) == 10
  dws = _run(torch, reqs, False)
  for dw in dws:                                                     # entries in no row: exactly 0, over the sentinel
    assert not bool(bits(torch, dw[:FRONT]).any()) and not bool(bits(torch, dw[-BACK:]).any())
  assert all(bool(dw.any()) for dw in dws)                           # (values were written)
  assert not torch.equal(bits(torch, dws[6]), bits(torch, dws[9]))   # the lower table alone is not the tier
  # the Python binding: fresh results, the same bits and the same count
  many, launches = T.find_combine_weight_grad_many(reqs + _extras_cache[False], return_launches=True)
  assert launches == 1 + 7 and tuple(many[-2].shape) == (0,) and not bool(many[-1].any())
  _same(torch, many[:len(reqs)], reqs, False, "python")
  # ---- the ragged form: PRUNE (zero, negative and NaN weights under "mixed"), FILL with any id
  some = int(ms[0][1].ids[5])
  for prune, fill in ((False, None), (True, None), (False, some), (True, -7)):
    reqs = [_ragged_req(o, b, weights, c, prune, fill) for o, b in ms]
    dws = _run(torch, reqs, True, "prune %s fill %s" % (prune, fill))
    if prune and weights == "mixed":
      for dw, (_, b) in zip(dws, ms):
        w_in = b.weights["mixed"][FRONT:NNZ - BACK]
        assert not bool(bits(torch, dw[~(w_in > 0)]).any())          # zero, negative and NaN weights: exactly 0
  # PRUNE differs by member: two classes where there was one
  reqs = [_ragged_req(o, b, weights, c, bool(j % 2), None) for j, (o, b) in enumerate(ms)]
  _run(torch, reqs, True, "prune by member")
  many, launches = T.find_combine_ragged_weight_grad_many(reqs + _extras_cache[True], return_launches=True)
  assert launches == _launches(torch, reqs + _extras_cache[True], True)
  _same(torch, many[:len(reqs)], reqs, True, "python")
  # row_splits that are negative, decreasing and beyond nnz are clamped: an entry outside the clamped cover gets 0, an entry that
  # exactly one row claims is the single call's (an entry two rows claim is written by both, in no order)
  bad_a, bad_b = ms[0][1].splits_np.copy(), ms[0][1].splits_np.copy()
  bad_a[0], bad_a[8], bad_a[-1] = -7, bad_a[7] - 2, NNZ_IN - 3       # negative; decreasing; the last 3 entries in no row
  bad_b[20] = NNZ_IN + 1000                                          # row 19 runs to the end of ids
  for bad in (bad_a, bad_b):
    cover = cover_of(bad, NNZ_IN)
    one, zero = torch.from_numpy(cover == 1).cuda(), torch.from_numpy(cover == 0).cuda()
    assert int(one.sum()) >= 100
    bad_t = torch.from_numpy(bad).cuda()
    reqs = [_ragged_req(o, b, weights, c, splits=bad_t) for o, b in ms]
    for dw in _run(torch, reqs, True, "clamped splits", only=one):
      assert not bool(bits(torch, dw[zero]).any())
  assert (cover_of(bad_a, NNZ_IN) == 0).sum() == 3 and (cover_of(bad_a, NNZ_IN) == 2).sum() >= 1
  for s in setups:
    _unchanged(torch, s)       # both tables' keys, rows and scores in key order, tier.stats(), check_errors()
  for o, _ in ms[:len(PLAIN)]:
    o.check_errors()


# ---- 2: launches_out -------------------------------------------------------------------------------------------------------------
def test_launches_count_the_classes_not_the_list(env, listed):
  torch, de = env
  T = de.table_ops
  ms, setups = listed
  reqs = [_tuple_req(o, b, "random", 1) for o, b in ms]
  # plain f32 NCH 1 / 2 / 4, plain f16 NCH 2, plain bf16 NCH 4, tier f32 NCH 1, tier f16 NCH 2 — and the ONE zero-fill + bounds launch
  for sub, classes in ((reqs, 7), (reqs[:2], 1), (reqs[:4], 3), (reqs[6:8], 2), (reqs[6:7] + reqs[9:], 2)):
    many, launches = T.find_combine_weight_grad_many(sub, return_launches=True)
    assert launches == classes + 1 == _launches(torch, sub, False)
    twice, launches2 = T.find_combine_weight_grad_many(sub + sub, return_launches=True)
    assert launches2 == launches and len(twice) == 2 * len(sub)
    assert all(torch.equal(bits(torch, a), bits(torch, b)) for a, b in zip(twice, many + many))
  ex = _extras_cache[False]
  assert T.find_combine_weight_grad_many([ex[0], ex[0]], return_launches=True)[1] == 0     # no entry anywhere: nothing is enqueued
  assert T.find_combine_weight_grad_many([ex[1]], return_launches=True)[1] == 1            # no rows: the zero-fill alone
  rag = [_ragged_req(o, b, "random", 1) for o, b in ms]
  pruning = [_ragged_req(o, b, "random", 1, prune=True) for o, b in ms[:2]]
  for sub, classes in ((rag, 7), (rag + pruning, 8), (pruning, 1), (rag[:1] + pruning[:1], 2)):
    _, launches = T.find_combine_ragged_weight_grad_many(sub, return_launches=True)
    assert launches == classes + 1 == _launches(torch, sub, True)
  # PRUNE without weights and FILL change nothing: the plain class
  same = [_ragged_req(ms[0][0], ms[0][1], "none", 1, prune=True), _ragged_req(ms[0][0], ms[0][1], "random", 1, fill=5), rag[0]]
  assert T.find_combine_ragged_weight_grad_many(same, return_launches=True)[1] == 2
  ex = _extras_cache[True]
  assert T.find_combine_ragged_weight_grad_many([ex[0]], return_launches=True)[1] == 0
  assert T.find_combine_ragged_weight_grad_many([ex[1]], return_launches=True)[1] == 1
  for s in setups:
    _unchanged(torch, s)


# ---- 3: the staging ring ---------------------------------------------------------------------------------------------------------
def test_ten_calls_back_to_back_share_the_ring(env, listed):
  torch, de = env
  T = de.table_ops
  ms, setups = listed
  calls = []
  for k in range(10):                                  # the ring has 8 slots; nothing is waited for between the calls
    c, weights = k % 3, ("none", "random", "mixed")[(k // 3) % 3]
    if k % 2:
      reqs = [_ragged_req(o, b, weights, c, prune=bool((j + k) % 3 == 0)) for j, (o, b) in enumerate(ms)]
      calls.append((True, reqs, T.find_combine_ragged_weight_grad_many(reqs)))
    else:
      reqs = [_tuple_req(o, b, weights, c) for o, b in (ms[k % 5:] + ms[:k % 5])]
      calls.append((False, reqs, T.find_combine_weight_grad_many(reqs)))
  for k, (ragged, reqs, dws) in enumerate(calls):
    _same(torch, dws, reqs, ragged, "call %d" % k)
  for s in setups:
    _unchanged(torch, s)


# ---- 4: refusals -----------------------------------------------------------------------------------------------------------------
def _single_refusal(torch, table, b, ragged, over):
  """(code, message tail) of the single table call with the same bad argument; nothing is written"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  lib, dev = _capi.lib(), torch.device("cuda:0")
  ids = b.ids[FRONT:FRONT + 8].contiguous()
  seg = torch.arange(8, dtype=torch.int64, device="cuda") // 2
  splits = torch.arange(0, 9, 2, dtype=torch.int64, device="cuda")
  dw = _sentinel(torch, 8)
  a = dict(grad_out=b.G.data_ptr(), dw_out=dw.data_ptr(), flags=0)
  a.update(over)
  if ragged:
    rc = lib.tfra_table_find_combine_ragged_backprop_weights(table._h, 4, _ptr(splits), 8, _ptr(ids), None, 1, a["flags"], 0,
                                                             _ptr(b.default_row), a["grad_out"], a["dw_out"], _stream(dev))
  else:
    rc = lib.tfra_table_find_combine_backprop_weights(table._h, _workspace(dev), 8, _ptr(ids), _ptr(seg), None, 1, 4, _ptr(b.default_row),
                                                      a["grad_out"], a["dw_out"], _stream(dev))
  msg = lib.tfra_last_error().decode()
  assert msg.startswith("find_combine_ragged_backprop_weights" if ragged else "find_combine_backprop_weights")
  torch.cuda.synchronize()
  assert bool((dw == SENTINEL).all())
  return rc, msg.split(": ", 1)[1]


@pytest.mark.parametrize("ragged", [False, True])
def test_a_bad_descriptor_refuses_the_whole_list(env, listed, ragged):
  torch, de = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  ms, setups = listed
  (p0, b0), (p1, b1), (t0, bt) = ms[0], ms[1], ms[len(PLAIN)]
  mk = (lambda o, b: _ragged_req(o, b, "random", 1)) if ragged else (lambda o, b: _tuple_req(o, b, "random", 1))
  six = _DeviceTable(torch.int64, torch.float32, torch.zeros(6), "wgm_dim6", "cuda:0", dim=6, init_capacity=1024)
  b6 = _batch(torch, np.random.default_rng(6), np.arange(1, NNZ + 1, dtype=np.int64), 6, torch.float32)
  who = NAMES[ragged][len("tfra_"):]
  size = ctypes.sizeof(_capi.FindCombineRaggedWgradDesc if ragged else _capi.FindCombineWgradDesc)
  # (the owner of descriptor 2, over for it, over for the single call or None, the code and tail where there is no single call)
  cases = [(p1, dict(struct_size=size - 8), None, (INVALID, "descriptor size mismatch")),
           (p1, dict(tier=t0._h.value), None, (INVALID, "exactly one of table / tier must be set")),
           (p1, dict(table=None), None, (INVALID, "exactly one of table / tier must be set")),
           (p1, dict(dw_out=None), dict(dw_out=None), None),
           (p1, dict(grad_out="misaligned"), dict(grad_out=b1.G.data_ptr() + 4), None),
           (six, {}, {}, None)]
  if ragged:
    cases.append((p1, dict(flags=4), dict(flags=4), None))
  for owner, over, single_over, fixed in cases:
    b = b6 if owner is six else b1
    dws = [_sentinel(torch, NNZ) for _ in range(4)]
    reqs = [mk(p0, b0), mk(t0, bt), mk(owner, b), mk(p1, b1)]
    over = dict(over)
    if over.get("grad_out") == "misaligned":
      over["grad_out"] = b.G.data_ptr() + 4
    items = [dict(req=r, dw=d) for r, d in zip(reqs, dws)]
    items[2]["over"] = over
    rc, msg, launches, _ = _raw(torch, ragged, items)
    want_rc, want_tail = fixed if fixed is not None else _single_refusal(torch, owner, b, ragged, single_over)
    assert want_rc in (INVALID, UNSUPPORTED) and rc == want_rc, (over, msg)
    assert msg.startswith("%s: descriptor 2: " % who) and msg.endswith(want_tail), (over, msg, want_tail)
    assert launches == 0
    torch.cuda.synchronize()
    assert all(bool((d == SENTINEL).all()) for d in dws), over        # no dw_out of any descriptor was written
  for s in setups:
    _unchanged(torch, s)
