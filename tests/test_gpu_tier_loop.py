"""GPU, end to end: a two-tier embedding store on find_missed / insert_and_evict / assign / contains.

`upper` is a bounded LRU table at max_capacity that stands in front of `lower`, a growing table that holds everything else.  A step
looks its ids up in `upper`, fetches the misses from `lower`, promotes them (what that displaces goes down), trains (rows + 1) and
writes back with `assign`; keys the step's own promotion displaced are not resident any more and go to `lower`.  A dict holds every
key's newest row: after every step each key ever seen has it in the tier that `contains` names."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, CAP, UNIVERSE, BATCH, STEPS = 8, 15 * 89, 4000, 300, 12


def _never_seen(torch, keys):
  """the row of a key no tier holds yet: a function of the key"""
  return ((keys[:, None] % 1000).to(torch.float32) * 0.5 + torch.arange(DIM, device=keys.device)[None, :]).contiguous()


def test_two_tier_loop():
  import torch
  import tfra_amd.dynamic_embedding as de
  upper_t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(DIM), init_capacity=CAP, max_capacity=CAP, device="cuda:0", dim=DIM,
                            evict_strategy=de.HkvEvictStrategy.LRU, name="tier_upper")
  lower_t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(DIM), name="tier_lower", device="cuda:0", dim=DIM)
  upper, lower = upper_t._table, lower_t._table
  rng = np.random.default_rng(17)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 50, dtype=np.int64))[:UNIVERSE]
  truth = {}
  displaced_by_own_step = 0
  for step in range(STEPS):
    ids_np = rng.choice(universe, size=BATCH, replace=False)
    ids = torch.from_numpy(ids_np).cuda()
    resident = upper.contains(ids)
    # 1. look up in the upper tier; its misses come back as (key, position)
    rows, mk, mi = upper.find_missed(ids)
    assert sorted(mk.tolist()) == sorted(ids[~resident].tolist()) and torch.equal(mk, ids[mi.long()])
    assert torch.equal(rows[resident], upper.find(ids)[resident])
    # 2. the lower tier has them, or nobody has: a never-seen key's row is a function of the key
    fetched, had = lower.find(mk, dynamic_default_values=_never_seen(torch, mk), return_exists=True)
    assert set(mk[had].tolist()) == {k for k in mk.tolist() if k in truth}
    # 3. into place
    rows[mi.long()] = fetched
    for k, r in zip(ids_np.tolist(), rows.cpu().numpy()):
      if k in truth:
        np.testing.assert_array_equal(r, truth[k], err_msg="step %d: key %d read an old row" % (step, k))
    # 4. promote; what leaves the upper tier goes down
    ek, ev, _ = upper.upsert_and_evict(mk, fetched)
    if ek.numel():
      lower.upsert(ek, ev, unique_keys=True)
    # 5. train
    new_rows = rows + 1
    # 6. write back: only what is (still) resident
    found = upper.assign(ids, new_rows, return_found=True)
    # 7. the keys this step's own promotion displaced
    if not bool(found.all()):
      lower.upsert(ids[~found], new_rows[~found], unique_keys=True)
      displaced_by_own_step += int((~found).sum())
    truth.update(zip(ids_np.tolist(), new_rows.cpu().numpy()))
    # after every step
    upper.check_errors()
    assert upper.size_host() <= upper.capacity()
    seen = torch.from_numpy(np.fromiter(truth, np.int64, len(truth))).cuda()
    up = upper.contains(seen)
    got = torch.where(up[:, None], upper.find(seen), lower.find(seen))
    want = torch.from_numpy(np.stack([truth[k] for k in seen.tolist()])).cuda()
    assert torch.equal(got, want), "step %d: %d keys do not hold their newest row" % (step, int((got != want).any(1).sum()))
    assert bool(lower.contains(seen[~up]).all())
  assert len(truth) > CAP            # the upper tier overflowed: the loop did evict
  assert upper.size_host() > 0.6 * CAP
