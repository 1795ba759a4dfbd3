"""The placement model of tests/probe_model.py pinned to hand-computed cases (no GPU)."""
import numpy as np
import pytest

from tests import probe_model as pm


def _py_homes(key, nb):
  """bucket0 / bucket1 of csrc/tfra_device.h in plain Python integers"""
  m64, m32 = (1 << 64) - 1, (1 << 32) - 1
  k = key & m64
  k ^= k >> 33; k = k * 0xff51afd7ed558ccd & m64
  k ^= k >> 33; k = k * 0xc4ceb9fe1a85ec53 & m64
  k ^= k >> 33
  b0 = ((k >> 32) * nb) >> 32
  x = (k & m32) ^ 0x9e3779b9
  x ^= x >> 16; x = x * 0x85ebca6b & m32
  x ^= x >> 13; x = x * 0xc2b2ae35 & m32
  x ^= x >> 16
  b1 = (x * nb) >> 32
  sub = b1 == b0
  if sub:
    b1 = 0 if b1 + 1 == nb else b1 + 1
  return b0, b1, sub


def test_fmix64_known_values():
  # murmur3's 64-bit finaliser: 0 is its fixed point, 1 -> 0xb456bcfc34c2cb2c (the published test vector)
  assert int(pm.fmix64(np.array([0], np.int64))[0]) == 0
  assert int(pm.fmix64(np.array([1], np.int64))[0]) == 0xb456bcfc34c2cb2c


@pytest.mark.parametrize("nb", [2, 3, 64, 89, 729, (1 << 32) - 2])
def test_homes_match_integer_arithmetic(nb):
  rng = np.random.default_rng(nb % 1000)
  keys = np.concatenate([rng.integers(-2**63, 2**63 - 1, size=2000, dtype=np.int64), np.array([0, 1, -1, 2**63 - 1, -2**63 + 2], np.int64)])
  b0, b1, sub = pm.homes(keys, nb)
  for i, k in enumerate(keys.tolist()):
    assert (int(b0[i]), int(b1[i]), bool(sub[i])) == _py_homes(k, nb), k
  assert ((0 <= b0) & (b0 < nb) & (0 <= b1) & (b1 < nb) & (b0 != b1)).all()


def test_craft_filters_and_is_deterministic():
  a = pm.craft(64, b0=20, b1=40, count=212)
  b0, b1, _ = pm.homes(a, 64)
  assert a.size == 212 and np.unique(a).size == 212 and (b0 == 20).all() and (b1 == 40).all()
  assert np.array_equal(a, pm.craft(64, b0=20, b1=40, count=212))
  assert np.array_equal(a[:50], pm.craft(64, b0=20, b1=40, count=50))
  w = pm.craft(64, b0=63, substituted=True, count=46)       # the substitute at the last bucket wraps to 0
  b0, b1, sub = pm.homes(w, 64)
  assert (b0 == 63).all() and (b1 == 0).all() and sub.all()
  n = pm.craft(64, b0=63, b1=0, substituted=False, count=10)
  assert not pm.homes(n, 64)[2].any()
  assert pm.craft(2, b0=0, count=5000).size == 5000 and pm.craft(3, b0=1, b1=2, count=5000).size == 5000


def test_craft_raises_when_starved():
  with pytest.raises(ValueError):
    pm.craft(729, b0=5, b1=6, count=160)          # ~8 keys of a pair in the stream at the default table's nb
  with pytest.raises(ValueError):
    pm.craft(64, b0=5, b1=5, count=1)             # b1 never equals b0


@pytest.mark.parametrize("n,ovf0,ovf1", [(15, 0, 0), (16, 1, 0), (30, 1, 0), (31, 1, 1), (46, 1, 2)])
def test_one_pair_fills_bucket_after_bucket(n, ovf0, ovf1):
  keys = pm.craft(64, b0=20, b1=40, count=n)
  m = pm.FirstFit(64)
  for k in keys:
    assert m.insert(k)
  assert m.census() == {"live": n, "empty": 64 * 15 - n, "ovf0": ovf0, "ovf1": ovf1}
  chain = [20, 40, 41, 42]
  for i, k in enumerate(keys):                     # key i sits in chain bucket i // 15, at that depth
    assert m.bucket_of(k) == chain[i // 15] and m.depth_of(k) == i // 15 and m.find(k) == chain[i // 15]
  assert not m.insert(keys[0]) and m.census()["live"] == n       # an assign changes nothing
  for k in pm.craft(64, b0=20, b1=40, count=n + 5)[n:]:
    assert m.find(k) is None
  assert m.full_buckets() == n // 15


def test_chain_wraps_past_the_last_bucket():
  keys = pm.craft(64, b0=10, b1=62, count=70)
  m = pm.FirstFit(64)
  for k in keys:
    m.insert(k)
  assert [m.bucket_of(k) for k in keys[::15]] == [10, 62, 63, 0, 1]
  assert m.census()["ovf0"] == 1 and m.census()["ovf1"] == 3 and m.ovf1[62] and m.ovf1[63] and m.ovf1[0] and not m.ovf1[1]
  assert all(m.find(k) == m.bucket_of(k) for k in keys)


def test_substitute_pile_on_the_last_bucket():
  keys = pm.craft(64, b0=63, substituted=True, count=46)
  m = pm.FirstFit(64)
  for k in keys:
    m.insert(k)
  assert [m.bucket_of(k) for k in keys[::15]] == [63, 0, 1, 2]
  assert m.ovf0[63] and m.ovf1[0] and m.ovf1[1] and not m.ovf1[2] and not m.ovf0[0]


def test_three_buckets_every_chain_wraps():
  keys = pm.craft(3, b0=1, b1=2, count=40)
  m = pm.FirstFit(3)
  for k in keys:
    m.insert(k)
  assert [m.bucket_of(k) for k in keys[::15]] == [1, 2, 0]
  assert m.census() == {"live": 40, "empty": 5, "ovf0": 1, "ovf1": 1}


def test_hole_is_refilled_before_the_chain_grows():
  keys = pm.craft(64, b0=20, b1=40, count=100)
  m = pm.FirstFit(64)
  for k in keys[:70]:
    m.insert(k)
  flags = (m.census()["ovf0"], m.census()["ovf1"])
  for k in keys[:15]:                              # chain bucket 0 ...
    assert m.erase(k)
  for k in keys[30:45]:                            # ... and chain bucket 2
    assert m.erase(k)
  assert not m.erase(keys[0])
  assert m.census()["live"] == 40 and (m.census()["ovf0"], m.census()["ovf1"]) == flags      # no tombstones, flags stay
  assert all(m.find(k) == m.bucket_of(k) for k in keys[45:70])                                # keys behind the holes still found
  assert not m.insert(keys[69]) and m.census()["live"] == 40                                  # ... and re-upserted where they are
  for k in keys[70:90]:                            # 20 new keys: 15 into bucket 20, 5 into bucket 41, none at the chain's end
    m.insert(k)
  assert [m.bucket_of(k) for k in keys[70:90]] == [20] * 15 + [41] * 5
  assert (m.census()["ovf0"], m.census()["ovf1"]) == flags and m.census()["live"] == 60
  m.insert(keys[90])
  assert m.bucket_of(keys[90]) == 41


def test_find_needs_both_flags():
  """What the GPU scenarios rest on: without the OVF1 rule (or the OVF0 rule) a resident key of a chain is not found."""
  keys = pm.craft(64, b0=20, b1=40, count=50)
  m = pm.FirstFit(64)
  for k in keys:
    m.insert(k)
  deep = keys[45]
  assert m.depth_of(deep) == 3 and m.find(deep) == 42
  m.ovf1[41] = False
  assert m.find(deep) is None
  m.ovf1[41] = True
  m.ovf0[20] = False
  assert m.find(deep) is None and m.find(keys[20]) is None


def test_pair_scene_key_sets():
  """30 residents fill the pair exactly, call 1 = b0 and call 2 = b1; the bystanders sit in their own b0 in any order of arrival,
  keep clear of b0, b1, b1 + 1, b1 + 2 of every pair and carry the table past 60 %."""
  nb = 89
  pairs = [(5, 12), (25, 32), (45, 52), (65, 86)]          # the last pair's b1 + 2 wraps to bucket 88
  keys, by = pm.pair_scene(nb, pairs)
  assert np.array_equal(by, pm.pair_scene(nb, pairs)[1])
  everything = np.concatenate(keys + [by])
  assert np.unique(everything).size == everything.size
  live = 30 * len(pairs) + by.size
  assert live == int(0.6 * nb * 15) + 60 and live > 0.6 * nb * 15
  shut = {b for b0, b1 in pairs for b in (b0, b1, (b1 + 1) % nb, (b1 + 2) % nb)}
  h0, h1, _ = pm.homes(by, nb)
  assert not (set(h0.tolist()) | set(h1.tolist())) & shut
  for order in (by, by[::-1]):
    m = pm.FirstFit(nb)
    for (b0, b1), k in zip(pairs, keys):
      kb0, kb1, _ = pm.homes(k, nb)
      assert k.size == 75 and (kb0 == b0).all() and (kb1 == b1).all()
      for x in k[:15]:
        m.insert(x)
      assert {m.bucket_of(x) for x in k[:15]} == {b0}
      for x in k[15:30]:
        m.insert(x)
      assert {m.bucket_of(x) for x in k[15:30]} == {b1}
    for x in order:
      m.insert(x)
    assert [m.bucket_of(x) for x in by] == h0.tolist()
    for b0, b1 in pairs:
      assert m.slots[(b1 + 1) % nb] == [None] * 15 and m.slots[(b1 + 2) % nb] == [None] * 15
    assert m.census()["live"] == live
    fresh = keys[0][30]                                     # a table that cannot evict would put it into b1 + 1
    m.insert(fresh)
    assert m.bucket_of(fresh) == pairs[0][1] + 1
  with pytest.raises(ValueError):
    pm.pair_scene(nb, [(5, 12), (13, 40)])                  # bucket 13 is b1 + 1 of the first pair
