"""GPU: the tier driver (tfra_tier_*) — an upper LRU table of 15 * 89 slots at max_capacity in front of a growing lower table.

Which resident an LRU table evicts depends on device clocks, so nothing here asserts a victim.  What is asserted after every call is
the invariant — every key ever written through the tier has its newest WHOLE row (embedding and both slot vectors, bit for bit) in
the upper table if that contains the key, otherwise in the lower one — and conservation: the driver's statistics against a
dictionary of whole rows that is the truth."""
import numpy as np
import pytest

from tests import probe_model as pm

pytestmark = pytest.mark.gpu

DIM, AUX, CAP, UNIVERSE, BATCH, STEPS, MAX_BATCH = 8, 2, 15 * 89, 4000, 300, 12, 512
AUX_INIT = (0.5, 0.25, 0.0, 0.0)
SEED = 17


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _tables(torch, tag, dim=DIM, aux=AUX, lower_dim=None, upper_strategy=0):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  upper = _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "tier_up_" + tag, "cuda:0", dim=dim, aux_fields=aux, init_capacity=CAP,
                       max_capacity=CAP, strategy=upper_strategy, aux_init=AUX_INIT)
  ld = dim if lower_dim is None else lower_dim
  lower = _DeviceTable(torch.int64, torch.float32, torch.zeros(ld), "tier_lo_" + tag, "cuda:0", dim=ld, aux_fields=aux)
  return upper, lower


def _tier(torch, tag, **kw):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTier
  upper, lower = _tables(torch, tag, **kw)
  return upper, lower, _DeviceTier(upper, lower, MAX_BATCH)


def _never_seen(keys):
  """numpy [n, DIM]: the init row of a key no tier holds yet, a function of the key"""
  return ((keys[:, None] % 1000).astype(np.float32) * np.float32(0.5) + np.arange(DIM, dtype=np.float32)[None, :])


def _fresh_whole(keys):
  """the whole row a never-seen key starts with: its init row, then the slot vectors at aux_init"""
  return np.concatenate([_never_seen(keys)] + [np.full((keys.size, DIM), AUX_INIT[f], np.float32) for f in range(AUX)], axis=1)


def _universe():
  rng = np.random.default_rng(SEED)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 50, dtype=np.int64))[:UNIVERSE]
  prefill = [rng.choice(universe, size=BATCH, replace=False) for _ in range(6)]
  batches = [rng.choice(universe, size=BATCH, replace=False) for _ in range(STEPS)]
  return universe, prefill, batches


def _saturated(keys, nb):
  """batch keys with 15 or more batch keys homed at BOTH of their home buckets (probe_model.homes)"""
  b0, b1, _ = pm.homes(keys, nb)
  load = np.bincount(np.concatenate([b0, b1]), minlength=nb)
  return int(((load[b0] >= 15) & (load[b1] >= 15)).sum())


class Truth:
  """{key: whole row} of everything written through the tier, the set of keys the upper table held after the last call, and the
  running counts the driver's statistics must equal."""

  def __init__(self, torch, upper, lower, tier):
    self.torch, self.upper, self.lower, self.tier = torch, upper, lower, tier
    self.rows, self.in_upper = {}, set()
    self.calls = self.missed = self.lower_hits = self.demoted = 0

  def seen(self):
    return np.fromiter(self.rows, np.int64, len(self.rows))

  def after_call(self, batch, tag):
    """what left the upper table in the call that just ended; then the invariant and the statistics"""
    torch, upper, lower = self.torch, self.upper, self.lower
    seen = self.seen()
    st = torch.from_numpy(seen).cuda()
    up = upper.contains(st)
    now = set(seen[up.cpu().numpy()].tolist())
    self.demoted += len((self.in_upper | set(batch.tolist())) - now)
    self.in_upper = now
    self.calls += 1
    want = torch.from_numpy(np.stack([self.rows[k] for k in seen.tolist()])).cuda()
    for f in range(AUX + 1):
      got = torch.where(up[:, None], upper.find(st, field=f), lower.find(st, field=f))
      bad = (got.view(torch.int32) != want[:, f * DIM:(f + 1) * DIM].contiguous().view(torch.int32)).any(1)
      assert not bool(bad.any()), "%s: field %d of %d keys is not the newest (%d of them in the upper table)" % (
          tag, f, int(bad.sum()), int((bad & up).sum()))
    assert bool(lower.contains(st[~up]).all()), tag
    upper.check_errors()
    lower.check_errors()
    assert upper.size_host() <= upper.capacity()
    s = self.tier.stats()
    assert (s["calls"], s["missed"], s["lower_hits"], s["demoted"]) == (self.calls, self.missed, self.lower_hits, self.demoted), (tag, s)


def test_lookup_loop_keeps_whole_rows(env):
  torch, _ = env
  upper, lower, tier = _tier(torch, "loop")
  nb = (upper.capacity() - 2) // 15
  assert nb == 89
  _, prefill, batches = _universe()
  truth = Truth(torch, upper, lower, tier)
  # fill the upper table to capacity through the tier (what overflows goes down)
  for i, ids in enumerate(prefill):
    rows = _never_seen(ids) + np.float32(0.25)
    tier.insert(torch.from_numpy(ids).cuda(), torch.from_numpy(rows).cuda())
    # (an insert writes the embedding; the slot vectors of a new key start at aux_init, and nothing has written another value yet)
    truth.rows.update(zip(ids.tolist(), np.concatenate([rows, _fresh_whole(ids)[:, DIM:]], axis=1)))
    truth.after_call(ids, "prefill %d" % i)
  assert upper.size_host() > 0.9 * CAP and len(truth.rows) > CAP
  for step, ids in enumerate(batches):
    assert _saturated(ids, nb) == 0
    kt = torch.from_numpy(ids).cuda()
    up_before = upper.contains(kt).cpu().numpy()
    known = np.array([k in truth.rows for k in ids.tolist()])
    rows, where = tier.find_or_insert(kt, init_values=torch.from_numpy(_never_seen(ids)).cuda(), return_where=True, verify=True)
    want_rows = np.stack([truth.rows[k][:DIM] if k in truth.rows else r for k, r in zip(ids.tolist(), _never_seen(ids))])
    assert rows.cpu().numpy().tobytes() == want_rows.tobytes(), "step %d: a lookup returned an old row" % step
    want_where = np.where(up_before, 1, np.where(known, 2, 0)).astype(np.uint8)
    assert np.array_equal(where.cpu().numpy(), want_where), "step %d: where" % step
    truth.missed += int((~up_before).sum())
    truth.lower_hits += int((want_where == 2).sum())
    fresh = ids[~known]
    truth.rows.update(zip(fresh.tolist(), _fresh_whole(fresh)))
    truth.after_call(ids, "step %d, lookup" % step)
    assert tier.stats()["not_resident"] == 0 and bool(upper.contains(kt).all())
    # "training": new embedding AND new slot vectors, written into the upper table
    old = np.stack([truth.rows[k] for k in ids.tolist()])
    new = old * np.float32(0.5) + np.float32(step + 1)
    for f in range(AUX + 1):      # (every key of the batch is resident: a field insert claims nothing)
      upper.upsert(kt, torch.from_numpy(np.ascontiguousarray(new[:, f * DIM:(f + 1) * DIM])).cuda(), unique_keys=f == 0, field=f)
    truth.rows.update(zip(ids.tolist(), new))
  s = tier.stats()
  never_seen = len(truth.rows) - len({k for b in prefill for k in b.tolist()})
  assert s["missed"] == s["lower_hits"] + never_seen and never_seen > 0
  assert s["demoted"] > CAP // 2 and s["lower_hits"] > 100      # keys did go down and come up again, slot vectors and all


def test_find_is_a_read(env):
  """tier.find with repeated keys equals torch.where(upper.contains, upper.find, lower.find) and changes neither table"""
  torch, _ = env
  upper, lower, tier = _tier(torch, "find")
  universe, prefill, _ = _universe()
  for ids in prefill:
    tier.insert(torch.from_numpy(ids).cuda(), torch.from_numpy(_never_seen(ids)).cuda())
  rng = np.random.default_rng(3)
  ids = rng.choice(universe, size=400, replace=True)
  ids[100:200] = ids[0:100]                        # repeats, resident or not
  kt = torch.from_numpy(ids).cuda()
  default = torch.full((DIM,), -3.0, device="cuda")

  def export(t):
    k, v, s = t.export_all(with_scores=True)
    o = torch.argsort(k)
    return [k[o], v[o], s[o]] + [t.find(k[o], field=f) for f in range(1, AUX + 1)]

  before = export(upper), export(lower)
  up, lo = upper.contains(kt), lower.contains(kt)
  want = torch.where(up[:, None], upper.find(kt, default), lower.find(kt, default))
  rows, where = tier.find(kt, default, return_where=True)
  assert torch.equal(rows, want)
  assert torch.equal(where, torch.where(up, 1, torch.where(lo, 2, 0)).to(torch.uint8))
  assert bool((where == 0).any()) and bool((where == 1).any()) and bool((where == 2).any())
  full = torch.from_numpy(_never_seen(ids)).cuda()     # one default row per position
  rows2 = tier.find(kt, full)
  assert torch.equal(rows2, torch.where(up[:, None], upper.find(kt, full), lower.find(kt, full)))
  after = export(upper), export(lower)
  for b, a in zip(before, after):
    for x, y in zip(b, a):
      assert torch.equal(x, y), "a read changed a table"
  s = tier.stats()      # both reads listed every position the upper table missed, repeats included
  assert (s["calls"], s["missed"], s["lower_hits"]) == (len(prefill) + 2, 2 * int((~up).sum()), 2 * int((where == 2).sum()))


def test_counts_on_the_device(env):
  """d_n forms: the leading `m` entries are served, the poisoned tails are neither read as keys nor written"""
  torch, _ = env
  upper, lower, tier = _tier(torch, "dn")
  rng = np.random.default_rng(5)
  keys = np.unique(rng.integers(1, 2**40, size=600, dtype=np.int64))[:400]
  n, m = 400, 250
  poison = np.arange(2**41, 2**41 + n - m, dtype=np.int64)
  buf = np.concatenate([keys[:m], poison])
  cnt = torch.tensor([m], dtype=torch.int64, device="cuda")
  bt = torch.from_numpy(buf).cuda()
  tier.insert(bt, torch.from_numpy(_never_seen(buf)).cuda(), count=cnt)
  pt = torch.from_numpy(poison).cuda()
  assert not bool(upper.contains(pt).any()) and not bool(lower.contains(pt).any())
  assert upper.size_host() == m
  # a lookup of 150 known and 100 new keys, then 150 poisoned entries
  buf2 = np.concatenate([keys[100:250], keys[250:350], poison])
  out = torch.full((n, DIM), -9.0, device="cuda")
  rows, where = tier.find_or_insert(torch.from_numpy(buf2).cuda(), init_values=torch.from_numpy(_never_seen(buf2) + np.float32(1)).cuda(),
                                    return_where=True, count=cnt, out=out, verify=True)
  want = np.concatenate([_never_seen(keys[100:250]), _never_seen(keys[250:350]) + np.float32(1)])
  assert rows[:m].cpu().numpy().tobytes() == want.tobytes()
  assert bool((rows[m:] == -9.0).all()) and bool((where[m:] == 0).all())
  assert where[:m].tolist() == [1] * 150 + [0] * 100
  assert not bool(upper.contains(pt).any()) and not bool(lower.contains(pt).any())
  assert upper.size_host() == 350 and bool(upper.contains(torch.from_numpy(keys[:350]).cuda()).all())
  snap = out.clone()
  rows3, where3 = tier.find(torch.from_numpy(buf2).cuda(), torch.full((DIM,), -3.0, device="cuda"), return_where=True,
                            count=torch.tensor([-4], dtype=torch.int64, device="cuda"), out=out)
  assert torch.equal(rows3, snap) and not bool(where3.any())     # a negative count serves nothing
  s = tier.stats()
  assert (s["calls"], s["missed"], s["lower_hits"], s["demoted"], s["not_resident"]) == (3, 100, 0, 0, 0)
  upper.check_errors()
  lower.check_errors()


def test_refusals_name_the_function(env):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTier
  upper, lower, tier = _tier(torch, "refuse")
  keys = torch.arange(1, MAX_BATCH + 2, dtype=torch.int64, device="cuda")
  rows = torch.zeros((MAX_BATCH + 1, DIM), device="cuda")
  for name, call in (("tfra_tier_find_or_insert", lambda: tier.find_or_insert(keys, rows)), ("tfra_tier_find", lambda: tier.find(keys)),
                     ("tfra_tier_insert", lambda: tier.insert(keys, rows))):
    with pytest.raises(_capi.TfraError, match=name) as e:
      call()
    assert e.value.code == -1
  assert upper.size_host() == 0 and lower.size_host() == 0 and tier.stats()["calls"] == 0
  up16, lo8 = _tables(torch, "mismatch", dim=16, lower_dim=8)
  with pytest.raises(_capi.TfraError, match="tfra_tier_create") as e:
    _DeviceTier(up16, lo8, MAX_BATCH)
  assert e.value.code == -1
  with pytest.raises(_capi.TfraError, match="tfra_tier_create") as e:
    _DeviceTier(upper, upper, MAX_BATCH)
  assert e.value.code == -1
  lfu, lo = _tables(torch, "lfu", upper_strategy=1)
  with pytest.raises(_capi.TfraError, match="tfra_tier_create") as e:
    _DeviceTier(lfu, lo, MAX_BATCH)
  assert e.value.code == _capi.ERR_UNSUPPORTED
  with pytest.raises(_capi.TfraError, match="tfra_tier_create") as e:
    _DeviceTier(upper, lfu, MAX_BATCH)            # a lower table that forgets
  assert e.value.code == _capi.ERR_UNSUPPORTED
  for bad in (0, 1 << 31):
    with pytest.raises(_capi.TfraError, match="tfra_tier_create") as e:
      _DeviceTier(upper, lower, bad)
    assert e.value.code == -1


def test_a_batch_that_saturates_its_own_buckets(env):
  """32 keys of ONE (b0, b1) pair in one lookup: the pair has 30 slots, so at least two of them cannot stay in the upper table.
  TFRA_TIER_VERIFY counts them; their whole rows are below, every key's row is where the invariant says, and no error is counted."""
  torch, _ = env
  upper, lower, tier = _tier(torch, "saturate")
  nb = (upper.capacity() - 2) // 15
  _, prefill, _ = _universe()
  for ids in prefill:       # a dense upper table: a new key is placed in its two home buckets only
    tier.insert(torch.from_numpy(ids).cuda(), torch.from_numpy(_never_seen(ids)).cuda())
    torch.cuda.synchronize()
  assert upper.size_host() > 0.9 * CAP
  b0, b1 = nb // 3, nb // 3 + 5
  keys = pm.craft(nb, b0=b0, b1=b1, count=32)
  assert _saturated(keys, nb) == 32
  kt = torch.from_numpy(keys).cuda()
  s0 = tier.stats()
  rows, where = tier.find_or_insert(kt, init_values=torch.from_numpy(_never_seen(keys)).cuda(), return_where=True, verify=True)
  assert rows.cpu().numpy().tobytes() == _never_seen(keys).tobytes() and not bool(where.any())
  s = tier.stats()
  up = upper.contains(kt)
  assert s["not_resident"] == int((~up).sum()) >= 2
  assert s["demoted"] - s0["demoted"] >= s["not_resident"] and s["missed"] - s0["missed"] == 32 and s["lower_hits"] == s0["lower_hits"]
  assert bool(lower.contains(kt[~up]).all())
  want = torch.from_numpy(_fresh_whole(keys)).cuda()
  for f in range(AUX + 1):
    got = torch.where(up[:, None], upper.find(kt, field=f), lower.find(kt, field=f))
    assert torch.equal(got, want[:, f * DIM:(f + 1) * DIM])
  upper.check_errors()
  lower.check_errors()
  # the next lookup of the same keys finds the rest below
  rows2, where2 = tier.find_or_insert(kt, return_where=True)
  assert torch.equal(rows2, rows) and where2.tolist() == torch.where(up, 1, 2).tolist()
