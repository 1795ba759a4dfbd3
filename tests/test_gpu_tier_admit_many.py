"""GPU: the grouped admission over tiers (tfra_multi_tier_find_or_insert; table_ops.tier_find_or_insert_many / admit_many) — per
member it IS tfra_tier_find_or_insert: the same rows and `where`, the same invariant, the same statistics.

The tiers are those of tests/test_gpu_tier_driver.py: an upper LRU table of 15 * 89 slots at max_capacity in front of a growing
lower table, max_batch 512.  Which resident an LRU table evicts depends on device clocks, so nothing here asserts a victim.  What
is asserted per member after every call: the returned rows and `where` against `upper.contains` read just before the call and a
dictionary of whole rows (`Truth`, restated from that file for any value type, dim and number of slot vectors), the invariant —
every key ever written through the tier has its newest WHOLE row in the upper table if that contains the key, otherwise in the
lower one —, and the driver's statistics.  No batch saturates its own home buckets (`_saturated`, probe_model.homes, on the CPU),
so under VERIFY not_resident stays 0 and the whole batch is resident after the call."""
import collections
import ctypes

import numpy as np
import pytest

from tests import probe_model as pm

pytestmark = pytest.mark.gpu

CAP, NB, UNIVERSE, BATCH, MAX_BATCH = 15 * 89, 89, 4000, 300, 512
AUX_INIT = (0.5, 0.25, 0.0, 0.0)
SEED = 17

Spec = collections.namedtuple("Spec", "dtype dim aux full")      # full: the upper table is at max_capacity


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _tdt(torch, spec):
  return {"float32": torch.float32, "float16": torch.float16}[spec.dtype]


_count = [0]


def _tier(torch, spec, lower=None):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
  _count[0] += 1
  tag = "tam%d" % _count[0]
  dt = _tdt(torch, spec)
  upper = _DeviceTable(torch.int64, dt, torch.zeros(spec.dim, dtype=dt), "up_" + tag, "cuda:0", dim=spec.dim, aux_fields=spec.aux,
                       init_capacity=CAP, max_capacity=CAP if spec.full else 64 * CAP, strategy=0, aux_init=AUX_INIT)
  if lower is None:
    lower = _DeviceTable(torch.int64, dt, torch.zeros(spec.dim, dtype=dt), "lo_" + tag, "cuda:0", dim=spec.dim, aux_fields=spec.aux)
  return upper, lower, _DeviceTier(upper, lower, MAX_BATCH)


def _never_seen(keys, spec):
  """numpy [n, dim]: the init row of a key no tier holds yet, a function of the key (exact in float16 too)"""
  return ((keys[:, None] % 1000).astype(np.float32) * np.float32(0.5) + np.arange(spec.dim, dtype=np.float32)[None, :]).astype(spec.dtype)


def _fresh_whole(keys, spec):
  """the whole row a never-seen key starts with: its init row, then the slot vectors at aux_init"""
  return np.concatenate([_never_seen(keys, spec)] + [np.full((keys.size, spec.dim), AUX_INIT[f], spec.dtype) for f in range(spec.aux)], axis=1)


def _universe():
  """the key universe, prefill batches and lookup batches of tests/test_gpu_tier_driver.py (none of them saturates)"""
  rng = np.random.default_rng(SEED)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 50, dtype=np.int64))[:UNIVERSE]
  prefill = [rng.choice(universe, size=BATCH, replace=False) for _ in range(6)]
  batches = [rng.choice(universe, size=BATCH, replace=False) for _ in range(12)]
  return universe, prefill, batches


def _saturated(keys, nb):
  """batch keys with 15 or more batch keys homed at BOTH of their home buckets (probe_model.homes)"""
  b0, b1, _ = pm.homes(keys, nb)
  load = np.bincount(np.concatenate([b0, b1]), minlength=nb)
  return int(((load[b0] >= 15) & (load[b1] >= 15)).sum())


def _bits(torch, x):
  return x.contiguous().view(torch.uint8)


class Truth:
  """{key: whole row} of everything written through the tier, the set of keys the upper table held after the last call, and the
  running counts the driver's statistics must equal."""

  def __init__(self, torch, spec, upper, lower, tier):
    self.torch, self.spec, self.upper, self.lower, self.tier = torch, spec, upper, lower, tier
    self.rows, self.in_upper = {}, set()
    self.calls = self.missed = self.lower_hits = self.demoted = 0

  def seen(self):
    return np.fromiter(self.rows, np.int64, len(self.rows))

  def before_lookup(self, ids):
    """what the call must return for `ids` — (rows, where) — from the dictionary and upper.contains read now; counts the call's
    misses and lower hits and enters the never-seen keys into the dictionary"""
    spec = self.spec
    if not ids.size:
      return np.zeros((0, spec.dim), spec.dtype), np.zeros(0, np.uint8)
    up_before = self.upper.contains(self.torch.from_numpy(ids).cuda()).cpu().numpy()
    known = np.array([k in self.rows for k in ids.tolist()], bool)
    init = _never_seen(ids, spec)
    want_rows = np.stack([self.rows[k][:spec.dim] if k in self.rows else r for k, r in zip(ids.tolist(), init)])
    want_where = np.where(up_before, 1, np.where(known, 2, 0)).astype(np.uint8)
    self.missed += int((~up_before).sum())
    self.lower_hits += int((want_where == 2).sum())
    fresh = ids[~known]
    self.rows.update(zip(fresh.tolist(), _fresh_whole(fresh, spec)))
    return want_rows, want_where

  def after_call(self, batch, tag):
    """what left the upper table in the call that just ended; then the invariant and the statistics"""
    torch, upper, lower, spec = self.torch, self.upper, self.lower, self.spec
    seen = self.seen()
    self.calls += 1
    if not seen.size:      # (a call that served nothing on a tier that holds nothing)
      s = self.tier.stats()
      assert (s["calls"], s["missed"], s["lower_hits"], s["demoted"]) == (self.calls, 0, 0, 0), (tag, s)
      return
    st = torch.from_numpy(seen).cuda()
    up = upper.contains(st)
    now = set(seen[up.cpu().numpy()].tolist())
    self.demoted += len((self.in_upper | set(batch.tolist())) - now)
    self.in_upper = now
    want = torch.from_numpy(np.stack([self.rows[k] for k in seen.tolist()])).cuda()
    for f in range(spec.aux + 1):
      got = torch.where(up[:, None], upper.find(st, field=f), lower.find(st, field=f))
      bad = (_bits(torch, got) != _bits(torch, want[:, f * spec.dim:(f + 1) * spec.dim])).any(1)
      assert not bool(bad.any()), "%s: field %d of %d keys is not the newest (%d of them in the upper table)" % (
          tag, f, int(bad.sum()), int((bad & up).sum()))
    assert bool(lower.contains(st[~up]).all()), tag
    upper.check_errors()
    lower.check_errors()
    assert upper.size_host() <= upper.capacity()
    s = self.tier.stats()
    assert (s["calls"], s["missed"], s["lower_hits"], s["demoted"]) == (self.calls, self.missed, self.lower_hits, self.demoted), (tag, s)

  def prefill(self, ids, tag):
    torch, spec = self.torch, self.spec
    rows = (_never_seen(ids, spec).astype(np.float32) + np.float32(0.25)).astype(spec.dtype)
    self.tier.insert(torch.from_numpy(ids).cuda(), torch.from_numpy(rows).cuda())
    # (an insert writes the embedding: a key the upper table holds keeps its slot vectors, any other key's start at aux_init there)
    aux = _fresh_whole(ids, spec)[:, spec.dim:]
    for i, k in enumerate(ids.tolist()):
      if k in self.in_upper:
        aux[i] = self.rows[k][spec.dim:]
    self.rows.update(zip(ids.tolist(), np.concatenate([rows, aux], axis=1)))
    self.after_call(ids, tag)

  def train(self, ids, step):
    """new embedding AND new slot vectors for the batch, written into the upper table (every key of the batch is resident)"""
    torch, spec = self.torch, self.spec
    kt = torch.from_numpy(ids).cuda()
    old = np.stack([self.rows[k] for k in ids.tolist()])
    new = (old.astype(np.float32) * np.float32(0.5) + np.float32(step + 1)).astype(spec.dtype)
    for f in range(spec.aux + 1):
      self.upper.upsert(kt, torch.from_numpy(np.ascontiguousarray(new[:, f * spec.dim:(f + 1) * spec.dim])).cuda(), unique_keys=f == 0, field=f)
    self.rows.update(zip(ids.tolist(), new))


def _make(torch, spec, prefill=()):
  upper, lower, tier = _tier(torch, spec)
  truth = Truth(torch, spec, upper, lower, tier)
  for i, ids in enumerate(prefill):
    truth.prefill(ids, "prefill %d" % i)
  return truth


def _request(torch, truth, ids, want_rows=True, verify=True, count=None):
  return (truth.tier, torch.from_numpy(ids).cuda(), torch.from_numpy(_never_seen(ids, truth.spec)).cuda(), count, want_rows, verify)


def _grouped_step(torch, T, truths, batches, tag, verify=True, want_rows=None):
  """ONE grouped call over truths[i] with batches[i]; every member checked against its Truth.  -> the launches"""
  want_rows = [True] * len(truths) if want_rows is None else want_rows
  wants = [t.before_lookup(ids) for t, ids in zip(truths, batches)]
  outs, launches = T.tier_find_or_insert_many([_request(torch, t, ids, wr, verify) for t, ids, wr in zip(truths, batches, want_rows)],
                                              return_launches=True)
  for i, (t, ids, out, (rows, where)) in enumerate(zip(truths, batches, outs, wants)):
    if want_rows[i]:
      assert out[0].cpu().numpy().tobytes() == rows.tobytes(), "%s member %d: a lookup returned an old row" % (tag, i)
      assert np.array_equal(out[1].cpu().numpy(), where), "%s member %d: where" % (tag, i)
    else:
      assert out is None
    t.after_call(ids, "%s member %d" % (tag, i))
    if verify:
      assert t.tier.stats()["not_resident"] == 0 and bool(t.upper.contains(torch.from_numpy(ids).cuda()).all()), (tag, i)
  return launches


# ---- 1: a heterogeneous list ------------------------------------------------------------------------------------------------------
HETERO = [Spec("float32", 8, 2, True), Spec("float32", 4, 0, True), Spec("float16", 4, 1, True), Spec("float32", 2, 2, True),
          Spec("float32", 8, 2, False)]


def test_a_heterogeneous_list(env):
  torch, de = env
  T = de.table_ops
  _, prefill, batches = _universe()
  assert all(_saturated(ids, NB) == 0 for ids in batches)
  truths = [_make(torch, spec, prefill) for spec in HETERO]
  for t in truths[:4]:
    assert t.upper.size_host() > 0.9 * CAP and len(t.rows) > CAP        # prefilled past capacity: what overflowed is below
  assert truths[4].upper.capacity() > len(truths[4].rows) and truths[4].demoted == 0   # the fifth cache still grows
  for step in range(8):
    mine = [batches[(step + j) % 8] for j in range(len(truths))]      # (the members look different batches up)
    launches = _grouped_step(torch, T, truths, mine, "step %d" % step)
    # one launch per stage and class (granules of 16 and 8 bytes here; a dense cache is a class of its own), never one per tier:
    # begin + 5 stages of at least the two granules + verify; at most the call's bound
    assert 1 + 5 * 2 + 1 <= launches <= 30, launches
    for j, t in enumerate(truths):
      t.train(mine[j], step)
  for t in truths[:4]:
    s = t.tier.stats()
    assert s["demoted"] > CAP // 4 and s["lower_hits"] > 100             # keys did go down and come up again, slot vectors and all
  assert truths[4].tier.stats()["demoted"] == 0                          # no phase 2, nothing demoted


# ---- 2: shapes at the block and prefix edges --------------------------------------------------------------------------------------
def test_shapes_at_the_block_and_prefix_edges(env):
  torch, de = env
  T = de.table_ops
  spec = HETERO[0]
  universe, _, _ = _universe()
  rng = np.random.default_rng(23)
  pool = rng.permutation(universe)
  sizes = [1, 255, 0, 256, 257, 300, 300]
  # member:   0 n = 1 | 1 n = 255, admission only | 2 n = 0 (skipped) | 3 n = 256, all hits | 4 n = 257, all misses |
  #           5 n = 300, d_n = 200 | 6 n = 300, d_n = 0
  truths = [_make(torch, spec) for _ in sizes]
  keys, at = [], 0
  for n in sizes:
    keys.append(np.ascontiguousarray(pool[at:at + n]))
    at += n
  assert all(_saturated(k, NB) == 0 for k in keys if k.size)
  truths[3].prefill(keys[3], "prefill")                                 # every key of member 3 is resident: an EMPTY miss list
  want_rows = [True, False, True, True, True, True, True]
  counts = [None, None, None, None, None, torch.tensor([200], dtype=torch.int64, device="cuda"),
            torch.tensor([0], dtype=torch.int64, device="cuda")]
  served = [k[:{5: 200, 6: 0}.get(i, k.size)] for i, k in enumerate(keys)]
  wants = [t.before_lookup(s) for t, s in zip(truths, served)]
  sentinel = [torch.full((k.size, spec.dim), -9.0, device="cuda") for k in keys]
  reqs = [_request(torch, t, k, wr, True, c) + (o,) for t, k, wr, c, o in zip(truths, keys, want_rows, counts, sentinel)]
  stats2 = truths[2].tier.stats()
  outs, launches = T.tier_find_or_insert_many(reqs, return_launches=True)
  assert launches == 7 and len(outs) == len(sizes)
  assert outs[1] is None and not bool(wants[3][1].tolist().count(0)) and set(wants[4][1].tolist()) == {0}
  for i, (t, k, s, out, (rows, where)) in enumerate(zip(truths, keys, served, outs, wants)):
    if i == 2:
      assert t.tier.stats() == stats2 and stats2["calls"] == 0 and tuple(out[0].shape) == (0, spec.dim)   # skipped: no call counted
      continue
    if want_rows[i]:
      m = s.size
      assert out[0].data_ptr() == sentinel[i].data_ptr()
      assert out[0][:m].cpu().numpy().tobytes() == rows.tobytes(), i
      assert np.array_equal(out[1][:m].cpu().numpy(), where), i
      assert bool((out[0][m:] == -9.0).all()) and not bool(out[1][m:].any()), "member %d: an entry beyond d_n was served" % i
    t.after_call(s, "member %d" % i)
    assert t.tier.stats()["not_resident"] == 0
    if s.size:
      assert bool(t.upper.contains(torch.from_numpy(s).cuda()).all())
    beyond = torch.from_numpy(k[s.size:]).cuda()
    assert not bool(t.upper.contains(beyond).any()) and not bool(t.lower.contains(beyond).any())
  assert truths[6].tier.stats()["calls"] == 1 and truths[6].upper.size_host() == 0     # d_n == 0: a call that serves nothing


# ---- 3: a long list ---------------------------------------------------------------------------------------------------------------
def test_a_long_list_takes_the_launches_of_a_short_one(env):
  torch, de = env
  T = de.table_ops
  spec = Spec("float32", 4, 0, True)
  universe, _, _ = _universe()
  truths = [_make(torch, spec) for _ in range(33)]
  rng = np.random.default_rng(29)
  got = {}
  for verify in (True, False):
    for n_tiers in (33, 4):
      batches = [rng.choice(universe, size=40 + j, replace=False) for j in range(n_tiers)]
      got[n_tiers, verify] = _grouped_step(torch, T, truths[:n_tiers], batches, "%d tiers" % n_tiers, verify=verify)
  assert got == {(33, True): 7, (4, True): 7, (33, False): 6, (4, False): 6}, got
  assert all(t.tier.stats()["calls"] == (4 if j < 4 else 2) for j, t in enumerate(truths))


# ---- 4: parity with the single call -----------------------------------------------------------------------------------------------
def test_parity_with_the_single_call(env):
  torch, de = env
  T = de.table_ops
  specs = [Spec("float32", 8, 2, True), Spec("float16", 4, 1, True), Spec("float32", 4, 0, True)]
  universe, prefill, batches = _universe()
  rng = np.random.default_rng(31)
  fresh = np.setdiff1d(np.unique(rng.integers(2**41, 2**42, size=400, dtype=np.int64)), universe)[:300]
  sets = [[_make(torch, spec, prefill[:1]) for spec in specs] for _ in range(2)]      # 300 keys: far below capacity, nothing evicted

  def both(step_batches, tag, full):
    wants = [[t.before_lookup(ids) for t, ids in zip(s, step_batches)] for s in sets]
    many = T.tier_find_or_insert_many([_request(torch, t, ids) for t, ids in zip(sets[0], step_batches)])
    single = [t.tier.find_or_insert(torch.from_numpy(ids).cuda(), torch.from_numpy(_never_seen(ids, t.spec)).cuda(), return_where=True,
                                    verify=True) for t, ids in zip(sets[1], step_batches)]
    for j, (a, b) in enumerate(zip(many, single)):
      assert torch.equal(_bits(torch, a[0]), _bits(torch, b[0])) and torch.equal(a[1], b[1]), "%s member %d" % (tag, j)
      assert a[0].cpu().numpy().tobytes() == wants[0][j][0].tobytes() and np.array_equal(a[1].cpu().numpy(), wants[0][j][1])
    for s in sets:
      for t, ids in zip(s, step_batches):
        t.after_call(ids, tag)
    for a, b in zip(*sets):      # (how many keys a FULL cache displaces depends on which it holds — device clocks; each set's
      sa, sb = a.tier.stats(), b.tier.stats()      # `demoted` is checked against its own upper table in after_call)
      names = ("calls", "missed", "lower_hits", "not_resident") + (() if full else ("demoted",))
      assert [sa[x] for x in names] == [sb[x] for x in names], (tag, sa, sb)

  # below capacity every outcome is a function of the calls alone: hits, never-seen keys, three members of three shapes
  roomy = [np.unique(np.concatenate([prefill[0][j * 100:j * 100 + 100], batches[j][:150]])) for j in range(3)]   # (unique keys)
  both(roomy, "roomy", False)
  assert all(t.demoted == 0 and t.missed > 0 for s in sets for t in s)
  for s in sets:
    for t, ids in zip(s, roomy):
      t.train(ids, 0)
  # past capacity: which keys stay above depends on device clocks.  The overflow is made of keys nobody has seen (an insert of a
  # key that is only below restarts its slot vectors, so a re-inserted key would read differently where the sets disagree on it),
  # and a lookup batch holds the keys both sets agree on, plus never-seen ones
  overflow = [np.arange(2**43 + i * 1000, 2**43 + i * 1000 + 300, dtype=np.int64) * 7919 for i in range(5)]
  for s in sets:
    for t in s:
      for i, ids in enumerate(overflow):
        t.prefill(ids, "overflow %d" % i)
  for step in range(2):
    step_batches = []
    for j in range(3):
      ids = np.unique(np.concatenate([batches[3 + step * 3 + j][:150], overflow[(step + j) % 5][:80], roomy[j][:40]]))
      assert _saturated(np.concatenate([ids, fresh[step * 100 + j * 30:step * 100 + j * 30 + 30]]), NB) == 0
      kt = torch.from_numpy(ids).cuda()
      agree = (sets[0][j].upper.contains(kt) == sets[1][j].upper.contains(kt)).cpu().numpy()
      step_batches.append(np.concatenate([ids[agree], fresh[step * 100 + j * 30:step * 100 + j * 30 + 30]]))
      assert step_batches[-1].size > 150
    both(step_batches, "full %d" % step, True)
    for s in sets:
      for t, ids in zip(s, step_batches):
        t.train(ids, step + 1)
  assert all(t.tier.stats()["demoted"] > 0 and t.tier.stats()["lower_hits"] > 0 for t in sets[0])
  # afterwards: every key ever written reads the same on both sets, all fields, wherever it lives
  for a, b in zip(*sets):
    assert a.rows.keys() == b.rows.keys()
    st = torch.from_numpy(a.seen()).cuda()
    for at in range(0, st.numel(), MAX_BATCH):
      chunk = st[at:at + MAX_BATCH]
      assert torch.equal(_bits(torch, a.tier.find(chunk)), _bits(torch, b.tier.find(chunk)))
    for f in range(a.spec.aux + 1):
      rows = [torch.where(t.upper.contains(st)[:, None], t.upper.find(st, field=f), t.lower.find(st, field=f)) for t in (a, b)]
      assert torch.equal(_bits(torch, rows[0]), _bits(torch, rows[1])), f


# ---- 5: refusals, each leaving everything as it was -----------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(env):
  torch, de = env
  from tfra_amd import _capi
  T = de.table_ops
  spec = HETERO[0]
  _, prefill, batches = _universe()
  a, b = _make(torch, spec, prefill[:2]), _make(torch, spec, prefill[:2])
  up_c, _, tier_c = _tier(torch, spec, lower=a.lower)                  # a second tier over a's lower table
  probe = torch.from_numpy(np.concatenate([prefill[0][:100], batches[0][:100]])).cuda()
  ids = batches[0]
  kt = torch.from_numpy(ids).cuda()
  init = torch.from_numpy(_never_seen(ids, spec)).cuda()
  big = torch.arange(1, MAX_BATCH + 2, dtype=torch.int64, device="cuda")
  big_init = torch.zeros((MAX_BATCH + 1, spec.dim), device="cuda")
  out = [torch.full((ids.size, spec.dim), -9.0, device="cuda") for _ in range(2)]
  where = [torch.full((ids.size,), 77, dtype=torch.uint8, device="cuda") for _ in range(2)]

  def state():
    s = []
    for t in (a, b):
      s += [t.tier.stats(), t.upper.size_host(), t.lower.size_host(), t.upper.contains(probe), t.lower.contains(probe)]
      s += [_bits(torch, x.find(probe, field=f)) for x in (t.upper, t.lower) for f in range(spec.aux + 1)]
    return s + [tier_c.stats(), up_c.size_host()]

  def desc(tier, keys=kt, init_values=init, j=0, flags=0, reserved=0, size=None):
    d = _capi.TierFindOrInsertDesc()
    d.struct_size = ctypes.sizeof(_capi.TierFindOrInsertDesc) if size is None else size
    d.flags, d.tier, d.n, d.d_n, d.keys = flags, tier._h.value, keys.numel(), None, keys.data_ptr()
    d.init_values, d.init_is_full, d.reserved = init_values.data_ptr(), 1, reserved
    d.values_out, d.where = out[j].data_ptr(), where[j].data_ptr()
    return d

  def raw(ds):
    arr = (_capi.TierFindOrInsertDesc * len(ds))(*ds)
    launches = ctypes.c_uint32(5)
    try:
      _capi.call("tfra_multi_tier_find_or_insert", T._workspace(torch.device("cuda:0")), len(ds), ctypes.c_void_p(ctypes.addressof(arr)),
                 ctypes.c_void_p(ctypes.addressof(launches)), T._stream(torch.device("cuda:0")))
    finally:
      assert launches.value == 0
  cases = [
      ("the same tier twice", lambda: raw([desc(a.tier), desc(a.tier, j=1)]), "descriptor 1: the same tier as descriptor 0"),
      ("two tiers over one lower table", lambda: raw([desc(a.tier), desc(tier_c, j=1)]), "descriptor 1: a table of this tier stands in descriptor 0"),
      ("n > max_batch in the LAST descriptor", lambda: raw([desc(a.tier), desc(b.tier, big, big_init, j=1)]),
       "descriptor 1: more keys than the tier's max_batch"),
      ("unknown flag bits", lambda: raw([desc(a.tier), desc(b.tier, j=1, flags=2)]), "descriptor 1: unknown flag bits"),
      ("a wrong struct_size", lambda: raw([desc(a.tier), desc(b.tier, j=1, size=64)]), "descriptor 1: descriptor size mismatch"),
      ("a non-zero reserved", lambda: raw([desc(a.tier), desc(b.tier, j=1, reserved=1)]), "descriptor 1: reserved must be 0"),
      ("through the Python call", lambda: T.tier_find_or_insert_many([(a.tier, kt, init), (b.tier, big, big_init)]),
       "descriptor 1: more keys than the tier's max_batch"),
  ]
  before = state()
  for name, call, text in cases:
    with pytest.raises(_capi.TfraError) as e:
      call()
    assert e.value.code == -1, name
    assert "multi_tier_find_or_insert: " + text in str(e.value), (name, str(e.value))
    after = state()
    for x, y in zip(before, after):
      assert torch.equal(x, y) if torch.is_tensor(x) else x == y, "%s: a refused list changed something" % name
    assert all(bool((o == -9.0).all()) for o in out) and all(bool((w == 77).all()) for w in where), name
  # the single call's wording behind the prefix
  with pytest.raises(_capi.TfraError) as e:
    b.tier.find_or_insert(big, big_init)
  assert "tfra_tier_find_or_insert: more keys than the tier's max_batch" in str(e.value) and e.value.code == -1
  # and the same descriptors, once the list is sound, are served
  raw_ok = [desc(a.tier), desc(b.tier, j=1)]
  wants = [t.before_lookup(ids) for t in (a, b)]
  arr = (_capi.TierFindOrInsertDesc * 2)(*raw_ok)
  launches = ctypes.c_uint32(0)
  _capi.call("tfra_multi_tier_find_or_insert", T._workspace(torch.device("cuda:0")), 2, ctypes.c_void_p(ctypes.addressof(arr)),
             ctypes.c_void_p(ctypes.addressof(launches)), T._stream(torch.device("cuda:0")))
  assert launches.value == 6
  for j, t in enumerate((a, b)):
    assert out[j].cpu().numpy().tobytes() == wants[j][0].tobytes() and np.array_equal(where[j].cpu().numpy(), wants[j][1])
    t.after_call(ids, "served %d" % j)


# ---- 6: through the variable layer ------------------------------------------------------------------------------------------------
DIMS, STEPS, V_BATCH, V_UNIVERSE = (8, 16, 4, 8), 6, 300, 3000       # [tiered, tiered, tiered, plain]


def _tier_cfg(de):
  return de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU),
                                  max_batch=1024)


def _train_batches(seed):
  """per step and variable: entry ids (300, repeating), their rows (1 to 8 entries each), weights, the gradient of the result"""
  rng = np.random.default_rng(seed)
  universe = np.unique(rng.integers(1, 2**40, size=V_UNIVERSE + 50, dtype=np.int64))[:V_UNIVERSE]
  steps = []
  for _ in range(STEPS):
    per_var = []
    for dim in DIMS:
      counts = []
      while sum(counts) < V_BATCH:
        counts.append(min(int(rng.integers(1, 9)), V_BATCH - sum(counts)))
      seg = np.repeat(np.arange(len(counts)), counts).astype(np.int64)
      ids = rng.choice(universe, size=V_BATCH, replace=True)
      w = rng.uniform(0.1, 2.0, size=V_BATCH).astype(np.float32)
      g = rng.standard_normal((len(counts), dim)).astype(np.float32) * np.float32(0.1)
      per_var.append((ids, seg, w, g))
    steps.append(per_var)
  return universe, steps


def _side(de, tag, tiered):
  opt = de.optimizers.Adam(1e-2)
  vs = []
  for k, dim in enumerate(DIMS):
    creator = de.TieredHashTableCreator(_tier_cfg(de)) if tiered and k < 3 else de.CuckooHashTableCreator()
    vs.append(de.Variable(dim=dim, name="tam_train_%s_%d" % (tag, k), initializer=0.25, kv_creator=creator, init_on_lookup=True,
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


@pytest.fixture
def c_names(monkeypatch):
  from tfra_amd import _capi
  names, real = [], _capi.call

  def call(name, *args):
    names.append(name)
    return real(name, *args)

  monkeypatch.setattr(_capi, "call", call)
  return names


@pytest.mark.parametrize("form", ["tuple", "safe_ragged"])
def test_grouped_training_admits_in_one_call_and_matches_roomy_twins(env, c_names, form):
  torch, de = env
  rag = de.ragged_embedding_ops
  universe, steps = _train_batches(103)
  (vs, deo), (twins, deo_twin) = _side(de, form, True), _side(de, form + "_twin", False)
  assert [hasattr(v._tables[0], "_tier") for v in vs] == [True, True, True, False]
  ut = torch.from_numpy(universe).cuda()
  for k, dim in enumerate(DIMS):      # start from full caches: most of a tiered variable's keys are only below
    rows = torch.from_numpy(np.random.default_rng(107 + k).standard_normal((V_UNIVERSE, dim)).astype(np.float32)).cuda()
    vs[k].upsert(ut, rows)
    twins[k].upsert(ut, rows)
  seen = [set(universe.tolist()) for _ in DIMS]
  for step, per_var in enumerate(steps):
    combiner = ("mean", "sum", "sqrtn")[step % 3]
    dev = [tuple(torch.from_numpy(x).cuda() for x in b) for b in per_var]
    splits = [torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(b[1]))]).astype(np.int64)).cuda() for b in per_var]
    for (ids, _, _, _), s in zip(per_var, seen):
      b0, b1, _ = pm.homes(np.unique(ids), NB)
      load = np.bincount(np.concatenate([b0, b1]), minlength=NB)
      assert not bool(((load[b0] >= 15) & (load[b1] >= 15)).any())     # no batch saturates its own home buckets (a CPU precondition)
      s.update(ids.tolist())
    del c_names[:]
    if form == "tuple":
      res = de.embedding_lookup_sparse_many(vs, [(b[1], b[0]) for b in dev], [b[2] for b in dev], combiner=combiner, return_trainable=True,
                                            num_rows=[b[3].shape[0] for b in dev])
    else:
      res = rag.safe_embedding_lookup_sparse_many(vs, [(sp, b[0]) for sp, b in zip(splits, dev)], [b[2] for b in dev], combiner=combiner,
                                                  return_trainable=True)
    assert c_names.count("tfra_multi_tier_find_or_insert") == 1 and c_names.count("tfra_tier_find_or_insert") == 0, c_names
    deo.apply_combined_gradients_many([(b[3], tw) for b, (_, tw) in zip(dev, res)])
    pairs = []
    for k, (twin, b) in enumerate(zip(twins, dev)):
      if form == "tuple":
        out, tw = de.embedding_lookup_sparse(twin, (b[1], b[0]), b[2], combiner=combiner, return_trainable=True, num_rows=b[3].shape[0])
      else:
        out, tw = rag.safe_embedding_lookup_sparse(twin, (splits[k], b[0]), b[2], combiner=combiner, return_trainable=True)
      assert torch.equal(_bits(torch, res[k][0]), _bits(torch, out)), "step %d variable %d: the grouped forward is not the twin's" % (step, k)
      pairs.append((b[3], tw))
    deo_twin.apply_combined_gradients(pairs)
  for k, (var, twin) in enumerate(zip(vs, twins)):
    t = var._tables[0]
    if hasattr(t, "_tier"):
      st = t._tier.stats()
      assert st["calls"] >= STEPS and st["demoted"] > 0 and st["lower_hits"] > 0      # keys went down and came up again
      t._lower.check_errors()
    t._table.check_errors()
    seen_t = torch.from_numpy(np.fromiter(seen[k], np.int64, len(seen[k]))).cuda()
    a, b = _whole_rows(torch, var, seen_t), _whole_rows(torch, twin, seen_t)
    assert a.shape == b.shape == (seen_t.numel(), DIMS[k] * 3)                         # embedding, m, v
    bad = (_bits(torch, a) != _bits(torch, b)).any(1)
    assert not bool(bad.any()), "variable %d: %d of %d keys differ from the twin (embedding, m or v)" % (k, int(bad.sum()), seen_t.numel())


def test_the_same_variable_twice_trains_as_the_loop_of_single_lookups(env, c_names):
  torch, de = env
  universe, steps = _train_batches(109)
  sides = []
  for tag in ("many", "loop"):
    opt = de.optimizers.Adam(1e-2)
    vs = [de.Variable(dim=DIMS[k], name="tam_twice_%s_%d" % (tag, k), initializer=0.25, kv_creator=de.TieredHashTableCreator(_tier_cfg(de)),
                      init_on_lookup=True, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt)) for k in range(3)]
    sides.append((vs, de.DynamicEmbeddingOptimizer(opt)))
  seen = [set(), set(), set()]
  for step, per_var in enumerate(steps[:3]):
    dev = [tuple(torch.from_numpy(x).cuda() for x in b) for b in per_var]      # dims 8, 16, 4, 8
    for k, b in zip((0, 1, 2, 0), per_var):
      seen[k].update(b[0].tolist())
    (vs, deo), (ls, deo_loop) = sides
    order = [vs[0], vs[1], vs[2], vs[0]]                                # the first variable stands twice
    del c_names[:]
    res = de.embedding_lookup_sparse_many(order, [(b[1], b[0]) for b in dev], [b[2] for b in dev], combiner="sum", return_trainable=True,
                                          num_rows=[b[3].shape[0] for b in dev])
    # the three distinct tiers in ONE grouped call, the second occurrence by the single call behind it
    assert c_names.count("tfra_multi_tier_find_or_insert") == 1 and c_names.count("tfra_tier_find_or_insert") == 1, c_names
    assert c_names.index("tfra_multi_tier_find_or_insert") < c_names.index("tfra_tier_find_or_insert")
    want = [de.embedding_lookup_sparse(v, (b[1], b[0]), b[2], combiner="sum", return_trainable=True, num_rows=b[3].shape[0])
            for v, b in zip([ls[0], ls[1], ls[2], ls[0]], dev)]
    for k in range(4):
      assert torch.equal(_bits(torch, res[k][0]), _bits(torch, want[k][0])), (step, k)
    deo.apply_combined_gradients([(b[3], tw) for b, (_, tw) in zip(dev, res)])
    deo_loop.apply_combined_gradients([(b[3], tw) for b, (_, tw) in zip(dev, want)])
  for k, (a, b) in enumerate(zip(sides[0][0], sides[1][0])):
    assert a._tables[0]._tier.stats()["calls"] == b._tables[0]._tier.stats()["calls"]      # every occurrence was admitted, once
    keys = torch.from_numpy(np.fromiter(seen[k], np.int64, len(seen[k]))).cuda()
    assert keys.numel() > 300
    assert torch.equal(_bits(torch, _whole_rows(torch, a, keys)), _bits(torch, _whole_rows(torch, b, keys)))


def test_a_list_of_two_tiers_keeps_the_single_calls(env, c_names):
  """below variable.ADMIT_MANY_MIN_TIERS distinct tiers the loop of single admissions stays (tests/test_gpu_tier_pooled_many.py
  holds it for its two tiered members); the grouped call is what a list of three takes"""
  torch, de = env
  assert de.variable.ADMIT_MANY_MIN_TIERS == 3
  _, steps = _train_batches(113)
  opt = de.optimizers.Adam(1e-2)
  vs = [de.Variable(dim=DIMS[k], name="tam_short_%d" % k, initializer=0.25, kv_creator=de.TieredHashTableCreator(_tier_cfg(de)),
                    init_on_lookup=True, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt)) for k in range(3)]
  dev = [tuple(torch.from_numpy(x).cuda() for x in b) for b in steps[0][:3]]
  for n, names in ((2, ["tfra_tier_find_or_insert"] * 2), (3, ["tfra_multi_tier_find_or_insert"]), (1, ["tfra_tier_find_or_insert"])):
    del c_names[:]
    de.embedding_lookup_sparse_many(vs[:n], [(b[1], b[0]) for b in dev[:n]], [b[2] for b in dev[:n]], combiner="sum", return_trainable=True,
                                    num_rows=[b[3].shape[0] for b in dev[:n]])
    assert [x for x in c_names if "find_or_insert" in x] == names, (n, c_names)
