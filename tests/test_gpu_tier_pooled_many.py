"""GPU: the grouped pooled lookups over tiers (tfra_multi_tier_find_combine, tfra_multi_tier_find_combine_ragged) — lists whose
members are tiers and plain tables, read in one call.

The tiers, their roomy twins and the batches are those of tests/test_gpu_tier_pooled.py (`setup_of`: an upper LRU table of
15 * 89 slots at max_capacity over a growing lower table, 3000 keys written through the tier, stale copies below promoted keys,
EMPTY_KEY stored below only, LOCKED_KEY absent, rows of (0, 1, 3, 4, 5, 16, 17, 33) entries, entries in front of row 0 and behind
the last row, at least 100 entries of each kind asserted from tier.find's `where`) — one tier per NCH class: dim 64 float32,
dim 128 float16, dim 256 bfloat16; the two plain tables are the twins of the first two.  Every class gets three descriptors: all
200 rows (13 blocks, the last one partly idle), the first 33 rows (the entries behind them are outside [0, n_rows)) and ONE row,
the 33-entry row 7 — so the block-prefix search and blockIdx.x - prefix[d] meet descriptors of 13, 3 and 1 blocks.

Every descriptor's result is compared bit for bit with the SINGLE call on that descriptor — a tier's with the tier call, a
table's with the table call —, and around the calls both tables of every tier and its statistics stay what they were."""
import ctypes

import numpy as np
import pytest

from tests import probe_model as pm
from tests.test_gpu_tier_pooled import CAP, COMB, COUNTS, INVALID, MAX_BATCH, N_KEYS, UNSUPPORTED, _unchanged, bits, setup_of

pytestmark = pytest.mark.gpu

TIERS = ((64, "float32"), (128, "float16"), (256, "bfloat16"))
VARIANTS = ((200, 0), (33, 0), (1, 7))   # (n_rows, the batch row that is the descriptor's row 0)
NAMES = {False: "tfra_multi_tier_find_combine", True: "tfra_multi_tier_find_combine_ragged"}


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture(scope="module")
def members(env):
  """[(owner, setup)]: the three tiers, then two plain tables; an owner has find_combine / find_combine_ragged, the single calls"""
  torch, _ = env
  setups = [setup_of(torch, dim, vd) for dim, vd in TIERS]
  return [(s.tier, s) for s in setups] + [(setups[0].twin, setups[0]), (setups[1].twin, setups[1])]


def _tuple_req(owner, s, weights, c, variant, flip=False):
  n, first = variant
  ids = s.ids.flip(0) if flip else s.ids            # (flipped: another batch over the same rows)
  return (owner, ids, s.seg - first, s.weights[weights], c, n, s.default_row)


def _ragged_req(owner, s, weights, c, variant, prune=False, fill=None):
  n, first = variant
  a, b = s.front, s.ids.numel() - s.back
  w = s.weights[weights]
  return (owner, s.splits[first:first + n + 1], s.ids[a:b], None if w is None else w[a:b], c, prune, fill, s.default_row)


def _single(req, ragged):
  owner, args = req[0], req[1:]
  if ragged:
    rs, ids, w, c, prune, fill, d = args
    return owner.find_combine_ragged(rs, ids, w, c, prune=prune, fill_id=fill, default_row=d)
  return owner.find_combine(*args)


def _same(torch, many, reqs, ragged, what=""):
  assert len(many) == len(reqs)
  for k, (got, req) in enumerate(zip(many, reqs)):
    want = _single(req, ragged)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(bits(torch, got), bits(torch, want)), "descriptor %d %s" % (k, what)


def _all_unchanged(torch, members):
  for _, s in members[:len(TIERS)]:
    _unchanged(torch, s)     # both tables' keys, rows and scores in key order, tier.stats(), check_errors()


# ---- 1: bit identity per descriptor with the single call -------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["none", "random", "mixed"])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_every_descriptor_equals_its_single_call(env, members, combiner, weights):
  torch, de = env
  T = de.table_ops
  c = COMB[combiner]
  reqs = [_tuple_req(o, s, weights, c, v) for o, s in members for v in VARIANTS]
  assert len(reqs) == 15 and reqs[0][1].numel() > MAX_BATCH           # no staging: a batch is not limited by max_batch
  many, launches = T.find_combine_many(reqs, return_launches=True)
  assert launches == 5 + 1                                            # five classes and the ONE bounds launch
  _same(torch, many, reqs, False)
  assert bool(many[2].any()) and tuple(many[2].shape) == (1, 64)      # the one-row descriptor: the 33-entry row
  for prune, fill in ((False, None), (True, None), (False, "up"), (False, "below"), (False, "absent"), (False, "sentinel"),
                      (True, "below")):
    reqs = [_ragged_req(o, s, weights, c, v, prune, None if fill is None else s.fill[fill]) for o, s in members for v in VARIANTS]
    many, launches = T.find_combine_ragged_many(reqs, return_launches=True)
    assert launches == 5                                              # one (tiered or not, dtype, NCH, safe or not) class per member
    _same(torch, many, reqs, True, "prune %s fill %s" % (prune, fill))
    if fill == "below":                                               # row 0 of the batch is empty: the LOWER table's row came back
      for k in (0, 3, 6):
        s = members[k // 3][1]
        assert torch.equal(bits(torch, many[k][0]), bits(torch, s.fill_rows["below"]))
  _all_unchanged(torch, members)


# ---- the descriptors by hand: what the Python layer cannot express ---------------------------------------------------------------
def _raw(torch, ragged, items):
  """One C call over descriptors made from `items`: dicts with owner, req (a request as above), optionally out (a tensor to write
  to instead of a fresh one) and over ({field: value} set last).  -> (code, message, launches, outs)"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import table_ops as T
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  desc_type = _capi.TierFindCombineRaggedDesc if ragged else _capi.TierFindCombineDesc
  descs = (desc_type * len(items))()
  keep, outs = [], []
  for e, it in zip(descs, items):
    e.struct_size = ctypes.sizeof(desc_type)
    table = T._pooled_owner(e, it["req"][0], True)
    if ragged:
      rs, ids, w, c, prune, fill, d = it["req"][1:]
      rs, ids, w, flags, fill_key, d, out = table._find_combine_ragged_args(rs, ids, w, prune, fill, d)
      e.n_rows, e.row_splits, e.flags, e.reserved, e.fill_id = rs.numel() - 1, rs.data_ptr(), flags, 0, fill_key
      keep.append(rs)
    else:
      ids, seg, w, c, n, d = it["req"][1:]
      ids, seg, w, d, out = table._find_combine_args(ids, seg, w, n, d)
      e.n_rows, e.seg = int(n), seg.data_ptr()
      keep.append(seg)
    out = it.get("out", out)
    e.combiner, e.nnz, e.ids, e.weights = int(c), ids.numel(), ids.data_ptr(), (w.data_ptr() if w is not None else None)
    e.default_row, e.out = d.data_ptr(), out.data_ptr()
    for field, value in it.get("over", {}).items():
      setattr(e, field, value)
    keep += [ids, w, d]
    outs.append(out)
  dev = torch.device("cuda:0")
  launches = ctypes.c_uint32(99)
  lib = _capi.lib()
  rc = getattr(lib, NAMES[ragged])(_workspace(dev), len(items), ctypes.c_void_p(ctypes.addressof(descs)),
                                   ctypes.c_void_p(ctypes.addressof(launches)), T._stream(dev))
  return rc, lib.tfra_last_error().decode(), launches.value, outs


def _nan(torch, n):
  return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


# ---- 2: one mixed list -----------------------------------------------------------------------------------------------------------
def test_one_mixed_list(env, members):
  torch, _ = env
  (t0, s0), (t1, s1), (t2, s2), (p0, _), (p1, _) = members
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  # tiers and plain tables; the first tier twice more, with another batch and another combiner; its LOWER table named directly
  reqs = [_tuple_req(t0, s0, "random", 1, VARIANTS[0]), _tuple_req(p0, s0, "mixed", 2, VARIANTS[1]),
          _tuple_req(t1, s1, "none", 0, VARIANTS[0]), _tuple_req(t0, s0, "mixed", 2, VARIANTS[1], flip=True),
          _tuple_req(s0.lower, s0, "random", 1, VARIANTS[0]), _tuple_req(t2, s2, "mixed", 1, VARIANTS[2]),
          _tuple_req(p1, s1, "none", 0, VARIANTS[2]), _tuple_req(s0.upper, s0, "none", 1, VARIANTS[1]),
          (t0, none, none, None, 1, 5, s0.default_row), (p0, none, none, None, 1, 6, s0.default_row)]      # nnz == 0: zeros
  skipped = _nan(torch, 64 * 4)
  items = [dict(req=r) for r in reqs] + [dict(req=_tuple_req(t0, s0, "none", 1, (0, 0)), out=skipped)]   # n_rows == 0: skipped
  rc, msg, launches, outs = _raw(torch, False, items)
  assert rc == 0, msg
  assert launches == 1 + 5     # bounds; plain f32 NCH 1, plain f16 NCH 2, tier f32 NCH 1, tier f16 NCH 2, tier bf16 NCH 4
  _same(torch, outs[:len(reqs)], reqs, False)
  assert not outs[8].any() and tuple(outs[8].shape) == (5, 64) and not outs[9].any()
  assert not torch.equal(bits(torch, outs[0][:33]), bits(torch, outs[4][:33]))     # the lower table alone is not the tier
  torch.cuda.synchronize()
  assert bool(torch.isnan(skipped).all())
  # the ragged form of the same list; nnz == 0 without FILL is zeros, with FILL the fill row — from BELOW for the tier
  zeros6 = torch.zeros(6, dtype=torch.int64, device="cuda")
  reqs = [_ragged_req(t0, s0, "random", 1, VARIANTS[0]), _ragged_req(p0, s0, "mixed", 2, VARIANTS[1], prune=True),
          _ragged_req(t1, s1, "none", 0, VARIANTS[0], fill=s1.fill["below"]), _ragged_req(t0, s0, "mixed", 2, VARIANTS[1], prune=True),
          _ragged_req(s0.lower, s0, "random", 1, VARIANTS[0]), _ragged_req(t2, s2, "mixed", 1, VARIANTS[2], fill=s2.fill["sentinel"]),
          _ragged_req(p1, s1, "none", 0, VARIANTS[2]), _ragged_req(s0.upper, s0, "none", 1, VARIANTS[1], fill=s0.fill["below"]),
          (t0, zeros6, none, None, 1, False, None, s0.default_row), (t0, zeros6, none, None, 1, False, s0.fill["below"], s0.default_row),
          (p0, zeros6, none, None, 1, False, s0.fill["below"], s0.default_row)]
  skipped = _nan(torch, 64 * 4)
  items = [dict(req=r) for r in reqs] + [dict(req=(t0, zeros6[:1], none, None, 1, False, s0.fill["up"], s0.default_row), out=skipped)]
  rc, msg, launches, outs = _raw(torch, True, items)
  assert rc == 0, msg
  _same(torch, outs[:len(reqs)], reqs, True)
  assert not outs[8].any()
  assert torch.equal(outs[9], s0.fill_rows["below"].expand(5, 64)) and torch.equal(outs[10], s0.fill_rows["below"].expand(5, 64))
  # the cache alone does not hold that key: the default row
  assert torch.equal(outs[7][0], s0.default_row.to(torch.float32))
  torch.cuda.synchronize()
  assert bool(torch.isnan(skipped).all())
  _all_unchanged(torch, members)


# ---- 3: launches_out -------------------------------------------------------------------------------------------------------------
def test_launches_count_the_classes_not_the_list(env, members):
  torch, de = env
  T = de.table_ops
  reqs = [_tuple_req(o, s, "random", 1, v) for o, s in members for v in VARIANTS]
  for sub, classes in ((reqs, 5), (reqs[:3], 1), (reqs[:3] + reqs[9:12], 2), (reqs[6:9], 1)):
    many, launches = T.find_combine_many(sub, return_launches=True)
    assert launches == classes + 1
    twice, launches2 = T.find_combine_many(sub + sub, return_launches=True)
    assert launches2 == launches and len(twice) == 2 * len(sub)
    assert all(torch.equal(bits(torch, a), bits(torch, b)) for a, b in zip(twice, many + many))
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  empty = [(o, none, none, None, 1, 4, s.default_row) for o, s in members]
  outs, launches = T.find_combine_many(empty, return_launches=True)
  assert launches == 5 and not any(bool(o.any()) for o in outs)        # no entry anywhere: no bounds launch
  outs, launches = T.find_combine_many(empty + reqs[:1], return_launches=True)
  assert launches == 5 + 1
  # the ragged form: safe or not is a class axis, and there is no bounds launch
  plain = [_ragged_req(o, s, "random", 1, v) for o, s in members for v in VARIANTS]
  safe = [_ragged_req(o, s, "random", 1, v, prune=True) for o, s in members[:2] for v in VARIANTS]
  for sub, classes in ((plain, 5), (plain + safe, 7), (safe, 2), (plain[:3] + safe[:3], 2)):
    _, launches = T.find_combine_ragged_many(sub, return_launches=True)
    assert launches == classes
    _, launches2 = T.find_combine_ragged_many(sub + sub, return_launches=True)
    assert launches2 == launches
  # PRUNE without weights changes nothing: the plain class
  _, launches = T.find_combine_ragged_many([_ragged_req(members[0][0], members[0][1], "none", 1, VARIANTS[0], prune=True), plain[0]],
                                           return_launches=True)
  assert launches == 1
  _all_unchanged(torch, members)


# ---- 5: refusals -----------------------------------------------------------------------------------------------------------------
def _single_refusal(torch, s, ragged, over):
  """(code, message tail) of the single tier call with the same bad argument"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  lib, dev = _capi.lib(), torch.device("cuda:0")
  ids = s.ids[:8].contiguous()
  seg = torch.arange(8, dtype=torch.int64, device="cuda") // 2
  splits = torch.arange(0, 9, 2, dtype=torch.int64, device="cuda")
  out = torch.zeros(4 * s.default_row.numel() + 4, dtype=torch.float32, device="cuda")
  a = dict(combiner=1, out=out.data_ptr(), ids=_ptr(ids), flags=0)
  a.update(over)
  if ragged:
    rc = lib.tfra_tier_find_combine_ragged(s.tier._h, 4, _ptr(splits), 8, a["ids"], None, a["combiner"], a["flags"], 0, _ptr(s.default_row),
                                           a["out"], _stream(dev))
    name = "tfra_tier_find_combine_ragged: "
  else:
    rc = lib.tfra_tier_find_combine(s.tier._h, _workspace(dev), 8, a["ids"], _ptr(seg), None, a["combiner"], 4, _ptr(s.default_row),
                                    a["out"], _stream(dev))
    name = "tfra_tier_find_combine: "
  msg = lib.tfra_last_error().decode()
  assert msg.startswith(name)
  torch.cuda.synchronize()
  assert not out.any()
  return rc, msg[len(name):]


@pytest.mark.parametrize("ragged", [False, True])
def test_a_bad_descriptor_refuses_the_whole_list(env, members, ragged):
  torch, _ = env
  (t0, s0), (t1, s1), _, (p0, _), _ = members
  mk = (lambda o, s, v: _ragged_req(o, s, "random", 1, v)) if ragged else (lambda o, s, v: _tuple_req(o, s, "random", 1, v))
  good = [mk(t0, s0, VARIANTS[1]), mk(p0, s0, VARIANTS[2]), mk(t1, s1, VARIANTS[1])]
  who = NAMES[ragged][len("tfra_"):]
  from tfra_amd import _capi
  size = ctypes.sizeof(_capi.TierFindCombineRaggedDesc if ragged else _capi.TierFindCombineDesc)
  # (over for the grouped descriptor, over for the single call or None, the code and tail where there is no single call)
  cases = [(dict(combiner=3), dict(combiner=3), None),
           (dict(out="misaligned"), dict(out="misaligned"), None),
           (dict(ids=None), dict(ids=None), None),
           (dict(struct_size=size - 8), None, (INVALID, "descriptor size mismatch")),
           (dict(table=s0.twin._h.value), None, (INVALID, "exactly one of table / tier must be set")),
           (dict(tier=None), None, (INVALID, "exactly one of table / tier must be set"))]
  if ragged:
    cases += [(dict(flags=4), dict(flags=4), None), (dict(reserved=1), None, (INVALID, "reserved must be 0"))]
  for over, single_over, fixed in cases:
    outs = [_nan(torch, 33 * 64), _nan(torch, 64), _nan(torch, 33 * 128), _nan(torch, 33 * 64 + 4)]
    items = [dict(req=r, out=o) for r, o in zip(good, outs)]
    over = dict(over)
    if over.get("out") == "misaligned":
      over["out"] = outs[3].data_ptr() + 4
      single_over = dict(out=None)      # filled below: the single call's own buffer, off by 4 bytes too
    items.append(dict(req=mk(t0, s0, VARIANTS[1]), out=outs[3], over=over))
    rc, msg, launches, _ = _raw(torch, ragged, items)
    if fixed is None:
      if "out" in single_over:
        buf = torch.zeros(4 * 64 + 4, dtype=torch.float32, device="cuda")
        single_over = dict(out=buf.data_ptr() + 4)
      want_rc, want_tail = _single_refusal(torch, s0, ragged, single_over)
    else:
      want_rc, want_tail = fixed
    assert want_rc in (INVALID, UNSUPPORTED) and rc == want_rc, (over, msg)
    assert msg == "%s: descriptor 3: %s" % (who, want_tail), over
    assert launches == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), over          # no out of any descriptor was written
  _all_unchanged(torch, members)


# ---- 6: growth -------------------------------------------------------------------------------------------------------------------
def test_a_lower_table_that_grew_is_read_where_it_is(env, members):
  torch, de = env
  T = de.table_ops
  dim = 64
  upper = T._DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "tpm_grow_up", "cuda:0", dim=dim, init_capacity=CAP, max_capacity=CAP,
                         strategy=0)
  lower = T._DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "tpm_grow_lo", "cuda:0", dim=dim, init_capacity=8192)
  tier = T._DeviceTier(upper, lower, MAX_BATCH)
  rng = np.random.default_rng(71)
  pool = np.unique(rng.integers(1, 2**40, size=70000, dtype=np.int64))
  rng.shuffle(pool)
  kt = torch.from_numpy(pool[:N_KEYS]).cuda()
  g = torch.Generator(device="cuda").manual_seed(72)
  rows = torch.randn((N_KEYS, dim), generator=g, device="cuda")
  for a in range(0, N_KEYS, 500):
    tier.insert(kt[a:a + 500], rows[a:a + 500])
  s = members[0][1]
  counts = np.tile(np.array(COUNTS), 25)
  ids = torch.from_numpy(rng.choice(pool[:N_KEYS + 300], int(counts.sum()))).cuda()
  assert int((~upper.contains(ids) & lower.contains(ids)).sum()) > 100
  splits = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda()
  seg = torch.from_numpy(np.repeat(np.arange(counts.size), counts).astype(np.int64)).cuda()
  other = _tuple_req(members[1][0], members[1][1], "random", 1, VARIANTS[1])
  other_r = _ragged_req(members[1][0], members[1][1], "random", 1, VARIANTS[1])

  def check():
    reqs = [(tier, ids, seg, None, 1, counts.size, s.default_row), other, (lower, ids, seg, None, 0, counts.size, s.default_row)]
    _same(torch, T.find_combine_many(reqs), reqs, False)
    reqs = [(tier, splits, ids, None, 1, False, int(pool[5]), s.default_row), other_r]
    _same(torch, T.find_combine_ragged_many(reqs), reqs, True)

  check()
  cap0 = lower.capacity()
  at = N_KEYS + 300
  for _ in range(16):                                  # insert below until the lower table has grown
    more = torch.from_numpy(pool[at:at + 4096]).cuda()
    lower.upsert(more, torch.zeros((more.numel(), dim), device="cuda"))
    at += 4096
    if lower.capacity() != cap0:
      break
  assert lower.capacity() != cap0
  check()
  want = tier.find(ids[:MAX_BATCH], s.default_row)
  one_per_row = torch.arange(MAX_BATCH, dtype=torch.int64, device="cuda")
  got = T.find_combine_many([(tier, ids[:MAX_BATCH], one_per_row, None, 0, MAX_BATCH, s.default_row)])[0]
  assert torch.equal(got, want)                        # the rows themselves, from where the lower table is now
  upper.check_errors()
  lower.check_errors()


# ---- 7: the staging ring ---------------------------------------------------------------------------------------------------------
def test_ten_calls_back_to_back_share_the_ring(env, members):
  torch, de = env
  T = de.table_ops
  calls = []
  for k in range(10):                                  # the ring has 8 slots; nothing is waited for between the calls
    c, weights = k % 3, ("none", "random", "mixed")[(k // 3) % 3]
    if k % 2:
      reqs = [_ragged_req(o, s, weights, c, VARIANTS[(k + j) % 3], prune=bool(j % 2)) for j, (o, s) in enumerate(members)]
      calls.append((True, reqs, T.find_combine_ragged_many(reqs)))
    else:
      reqs = [_tuple_req(o, s, weights, c, VARIANTS[(k + j) % 3]) for j, (o, s) in enumerate(members)]
      calls.append((False, reqs, T.find_combine_many(reqs)))
  for k, (ragged, reqs, outs) in enumerate(calls):
    _same(torch, outs, reqs, ragged, "call %d" % k)
  _all_unchanged(torch, members)


# ---- 8: the Variable layer -------------------------------------------------------------------------------------------------------
def _tier_cfg(de, max_batch=1024):
  return de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU),
                                  max_batch=max_batch)


@pytest.fixture(scope="module")
def variables(env):
  """[plain, tiered, plain, tiered] with a dim per class, 3000 rows each; (variables, keys, absent)"""
  torch, de = env
  rng = np.random.default_rng(83)
  pool = np.unique(rng.integers(1, 2**40, size=N_KEYS + 300, dtype=np.int64))
  rng.shuffle(pool)
  keys, absent = pool[:N_KEYS], pool[N_KEYS:N_KEYS + 100]
  out = []
  for k, (dim, tiered) in enumerate(((8, False), (16, True), (72, False), (256, True))):
    creator = de.TieredHashTableCreator(_tier_cfg(de)) if tiered else de.CuckooHashTableCreator()
    var = de.Variable(dim=dim, name="tpm_var%d" % k, initializer=0.5, kv_creator=creator)
    var.upsert(torch.from_numpy(keys).cuda(), torch.from_numpy(rng.standard_normal((N_KEYS, dim)).astype(np.float32)).cuda())
    assert var.can_lookup_combined()
    out.append(var)
  return out, keys, absent


def _sparse_batch(torch, rng, keys, absent, n_rows=120):
  counts = rng.integers(0, 9, size=n_rows)
  counts[[0, 7, n_rows - 1]] = 0
  counts[3] = 20
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = np.where(rng.random(seg.size) < 0.9, rng.choice(keys, seg.size), rng.choice(absent, seg.size))
  w = rng.standard_normal(seg.size).astype(np.float32)      # a third of the weights prune under the safe forms
  splits = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  return tuple(torch.from_numpy(x).cuda() for x in (seg, ids, w, splits)) + (n_rows,)


@pytest.fixture
def c_names(monkeypatch):
  from tfra_amd import _capi
  names, real = [], _capi.call

  def call(name, *args):
    names.append(name)
    return real(name, *args)

  monkeypatch.setattr(_capi, "call", call)
  return names


def test_the_grouped_forms_take_tiered_variables_in_one_call(env, variables, c_names):
  torch, de = env
  rag = de.ragged_embedding_ops
  vs, keys, absent = variables
  rng = np.random.default_rng(89)
  batches = [_sparse_batch(torch, rng, keys, absent) for _ in vs]
  n = batches[0][4]
  for v, b in zip(vs, batches):
    t = v._tables[0]
    if hasattr(t, "_tier"):
      assert int((~t._table.contains(b[1]) & t._lower.contains(b[1])).sum()) > 100      # full of keys that are only below
  below = vs[1]._tables[0]
  default_id = int(keys[(~below._table.contains(torch.from_numpy(keys).cuda())).cpu().numpy()][7])
  tup, rg, ws = [(b[0], b[1]) for b in batches], [(b[3], b[1]) for b in batches], [b[2] for b in batches]
  forms = (
      ("tfra_multi_tier_find_combine", lambda: de.embedding_lookup_sparse_many(vs, tup, ws, combiner="mean", num_rows=n),
       lambda v, i: de.embedding_lookup_sparse(v, tup[i], ws[i], combiner="mean", num_rows=n)),
      ("tfra_multi_tier_find_combine", lambda: de.safe_embedding_lookup_sparse_many(vs, tup, ws, combiner="sqrtn", num_rows=n),
       lambda v, i: de.safe_embedding_lookup_sparse(v, tup[i], ws[i], combiner="sqrtn", num_rows=n)),
      ("tfra_multi_tier_find_combine_ragged", lambda: rag.embedding_lookup_sparse_many(vs, rg, ws, combiner="sum"),
       lambda v, i: rag.embedding_lookup_sparse(v, rg[i], ws[i], combiner="sum")),
      ("tfra_multi_tier_find_combine_ragged", lambda: rag.safe_embedding_lookup_sparse_many(vs, rg, ws, combiner="mean", default_id=default_id),
       lambda v, i: rag.safe_embedding_lookup_sparse(v, rg[i], ws[i], combiner="mean", default_id=default_id)))
  for c_name, many, single in forms:
    del c_names[:]
    got = many()
    pooled = [x for x in c_names if "find_combine" in x]
    assert pooled == [c_name], pooled                       # ONE grouped call, and no tfra_tier_find_combine* beside it
    want = [single(v, i) for i, v in enumerate(vs)]
    assert all(torch.equal(bits(torch, a), bits(torch, b)) for a, b in zip(got, want)), c_name
    assert tuple(got[3].shape) == (n, 256) and bool(got[1][3].any())
  # a list with no tiered variable takes the calls it always took
  plain = [vs[0], vs[2]]
  del c_names[:]
  de.embedding_lookup_sparse_many(plain, [tup[0], tup[2]], [ws[0], ws[2]], combiner="mean", num_rows=n)
  rag.embedding_lookup_sparse_many(plain, [rg[0], rg[2]], [ws[0], ws[2]], combiner="mean")
  assert [x for x in c_names if "find_combine" in x] == ["tfra_multi_find_combine", "tfra_multi_find_combine_ragged"]


def test_a_tiered_owner_is_read_in_both_tiers(env, variables, c_names):
  torch, de = env
  vs, keys, _ = variables
  shard = vs[1]._tables[0]                                  # a TieredHashTable
  kt = torch.from_numpy(keys).cuda()
  only_below = kt[~shard._table.contains(kt) & shard._lower.contains(kt)][:200]
  assert only_below.numel() == 200
  one_per_row = torch.arange(200, dtype=torch.int64, device="cuda")
  want = shard._lower.find(only_below).to(torch.float32)
  assert not bool((want == 0.5).all(1).any())               # none of them is the default row
  splits = torch.arange(201, dtype=torch.int64, device="cuda")
  for owner in (shard, shard._tier):
    del c_names[:]
    got = de.table_ops.find_combine_many([(owner, only_below, one_per_row, None, 0, 200, shard._default_value)])[0]
    assert torch.equal(got, want)
    got = de.table_ops.find_combine_ragged_many([(owner, splits, only_below, None, 0, False, None, shard._default_value)])[0]
    assert torch.equal(got, want)
    assert [x for x in c_names if "find_combine" in x] == ["tfra_multi_tier_find_combine", "tfra_multi_tier_find_combine_ragged"]


# ---- 9: training -----------------------------------------------------------------------------------------------------------------
DIMS, STEPS, BATCH, UNIVERSE = (8, 16, 8), 6, 300, 3000       # [tiered, tiered, plain]


def _train_batches(seed):
  """per step and variable: entry ids (300, repeating), their rows (1 to 8 entries each), weights, the gradient of the result"""
  rng = np.random.default_rng(seed)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 50, dtype=np.int64))[:UNIVERSE]
  steps = []
  for _ in range(STEPS):
    per_var = []
    for dim in DIMS:
      counts = []
      while sum(counts) < BATCH:
        counts.append(min(int(rng.integers(1, 9)), BATCH - sum(counts)))
      seg = np.repeat(np.arange(len(counts)), counts).astype(np.int64)
      ids = rng.choice(universe, size=BATCH, replace=True)
      w = rng.uniform(0.1, 2.0, size=BATCH).astype(np.float32)
      g = rng.standard_normal((len(counts), dim)).astype(np.float32) * np.float32(0.1)
      per_var.append((ids, seg, w, g))
    steps.append(per_var)
  return universe, steps


def _no_saturation(entry_ids):
  b0, b1, _ = pm.homes(np.unique(entry_ids), 89)
  load = np.bincount(np.concatenate([b0, b1]), minlength=89)
  assert not bool(((load[b0] >= 15) & (load[b1] >= 15)).any())     # no batch saturates its own home buckets (a CPU precondition)


def _side(de, tag, tiered):
  opt = de.optimizers.Adam(1e-2)
  vs = []
  for k, dim in enumerate(DIMS):
    creator = de.TieredHashTableCreator(_tier_cfg(de)) if tiered and k < 2 else de.CuckooHashTableCreator()
    vs.append(de.Variable(dim=dim, name="tpm_train_%s_%d" % (tag, k), initializer=0.25, kv_creator=creator, init_on_lookup=True,
                          **de.DynamicEmbeddingOptimizer.variable_kwargs(opt)))
  return vs, de.DynamicEmbeddingOptimizer(opt)


def _whole_rows(torch, var, keys):
  """[n, (1 + aux) * dim]: embedding and slots of `keys`; a tiered variable is read through flush() plus its lower table"""
  t = var._tables[0]
  if hasattr(t, "flush"):
    t.flush()
    table = t._lower
  else:
    table = t._table
  assert bool(table.contains(keys).all())
  return torch.cat([table.find(keys, field=f) for f in range(var.aux_fields + 1)], dim=1)


@pytest.mark.parametrize("plan_writeback", [False, True])
def test_grouped_training_matches_roomy_twins_through_the_single_forms(env, c_names, monkeypatch, plan_writeback):
  torch, de = env
  if plan_writeback:
    monkeypatch.setattr(de.variable, "PLAN_AT_LOOKUP_MIN_IDS", 100)      # the batches are worth a plan at lookup time
  universe, steps = _train_batches(97)
  tag = "plan" if plan_writeback else "noplan"
  (vs, deo), (twins, deo_twin) = _side(de, tag, True), _side(de, tag + "_twin", False)
  assert [hasattr(v._tables[0], "_tier") for v in vs] == [True, True, False]
  # start from full caches: every variable holds the universe, most of a tiered one's keys are only below
  ut = torch.from_numpy(universe).cuda()
  for k, dim in enumerate(DIMS):
    rows = torch.from_numpy(np.random.default_rng(101 + k).standard_normal((UNIVERSE, dim)).astype(np.float32)).cuda()
    vs[k].upsert(ut, rows)
    twins[k].upsert(ut, rows)
  seen = [set(universe.tolist()) for _ in DIMS]
  for step, per_var in enumerate(steps):
    combiner = ("mean", "sum", "sqrtn")[step % 3]
    dev = [tuple(torch.from_numpy(x).cuda() for x in b) for b in per_var]
    for (ids, _, _, _), s in zip(per_var, seen):
      assert np.unique(ids).size <= ids.size <= 1024
      _no_saturation(ids)
      s.update(ids.tolist())
    del c_names[:]
    res = de.embedding_lookup_sparse_many(vs, [(b[1], b[0]) for b in dev], [b[2] for b in dev], combiner=combiner, return_trainable=True,
                                          num_rows=[b[3].shape[0] for b in dev], plan_writeback=plan_writeback)
    assert [x for x in c_names if "find_combine" in x] == ["tfra_multi_tier_find_combine"]
    assert c_names.count("tfra_tier_find_or_insert") == 2                    # one admission per tiered member: the read collapses
    if plan_writeback:
      assert all(tw.entry_plan is not None for _, tw in res)                 # from ONE grouped build
      assert c_names.count("tfra_multi_sparse_plan_build") == 1
    deo.apply_combined_gradients_many([(b[3], tw) for b, (_, tw) in zip(dev, res)])
    pairs = []
    for k, (twin, b) in enumerate(zip(twins, dev)):
      out, tw = de.embedding_lookup_sparse(twin, (b[1], b[0]), b[2], combiner=combiner, return_trainable=True, num_rows=b[3].shape[0],
                                           plan_writeback=plan_writeback)
      assert torch.equal(bits(torch, res[k][0]), bits(torch, out)), "step %d variable %d: the grouped forward is not the twin's" % (step, k)
      pairs.append((b[3], tw))
    deo_twin.apply_combined_gradients(pairs)        # one global step for the three pairs, as on the grouped side
  for k, (var, twin) in enumerate(zip(vs, twins)):
    t = var._tables[0]
    if hasattr(t, "_tier"):
      st = t._tier.stats()
      assert st["demoted"] > 0 and st["lower_hits"] > 0 and st["not_resident"] == 0    # keys went down and came up again
      t._lower.check_errors()
    t._table.check_errors()
    seen_t = torch.from_numpy(np.fromiter(seen[k], np.int64, len(seen[k]))).cuda()
    assert seen_t.numel() > CAP
    a, b = _whole_rows(torch, var, seen_t), _whole_rows(torch, twin, seen_t)
    assert a.shape == b.shape == (seen_t.numel(), DIMS[k] * 3)                         # embedding, m, v
    bad = (bits(torch, a) != bits(torch, b)).any(1)
    assert not bool(bad.any()), "variable %d: %d of %d keys differ from the twin (embedding, m or v)" % (k, int(bad.sum()), seen_t.numel())
    # the exports: a tiered shard's export does not depend on where a key lives
    (ka, va), (kb, vb) = var.export(), twin.export()
    oa, ob = torch.argsort(ka), torch.argsort(kb)
    assert torch.equal(ka[oa], kb[ob]) and torch.equal(bits(torch, va[oa]), bits(torch, vb[ob]))
    assert int(var.size()) == int(twin.size()) == seen_t.numel()


def test_a_member_over_max_batch_refuses_before_anything_is_admitted(env, c_names):
  torch, de = env
  rag = de.ragged_embedding_ops
  small = de.Variable(dim=8, name="tpm_big_a", initializer=0.25, kv_creator=de.TieredHashTableCreator(_tier_cfg(de, 64)))
  first = de.Variable(dim=8, name="tpm_big_b", initializer=0.25, kv_creator=de.TieredHashTableCreator(_tier_cfg(de, 1024)))
  plain = de.Variable(dim=8, name="tpm_big_c", initializer=0.25)
  vs = [first, plain, small]
  ids = torch.arange(1, 66, dtype=torch.int64, device="cuda")              # 65 entry ids > max_batch 64
  seg = torch.arange(65, dtype=torch.int64, device="cuda") // 4
  splits = torch.arange(0, 66, 5, dtype=torch.int64, device="cuda")
  del c_names[:]
  with pytest.raises(ValueError, match="max_batch"):
    de.embedding_lookup_sparse_many(vs, [(seg, ids)] * 3, None, combiner="sum", return_trainable=True, num_rows=17)
  with pytest.raises(ValueError, match="max_batch"):
    rag.safe_embedding_lookup_sparse_many(vs, [(splits, ids)] * 3, None, combiner="sum", return_trainable=True)
  assert not [x for x in c_names if "find_combine" in x or "find_or_insert" in x]       # nothing admitted, nothing read
  assert [int(v.size()) for v in vs] == [0, 0, 0]
  out = de.embedding_lookup_sparse_many(vs, [(seg, ids)] * 3, None, combiner="sum", num_rows=17)   # a read is not limited
  assert all(tuple(o.shape) == (17, 8) for o in out)
