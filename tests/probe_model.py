"""A numpy model of where the table places a key (csrc/tfra_device.h), no GPU.

  homes(keys, nb)      the two home buckets of each key, bit for bit what bucket0 / bucket1 compute
  craft(nb, ...)       keys with requested home buckets, filtered from a fixed-seed stream of int64 candidates
  FirstFit(nb)         a sequential table that cannot evict: first-fit placement along b0, b1, b1+1, ... (mod nb) and the two
                       monotone overflow flags, by the rule of locate_or_claim_from; erase empties the slot and keeps the flags
  pair_scene(nb, ...)  the key sets of an eviction scene (tests/test_gpu_eviction.py): bucket pairs with 30 residents + fresh keys
                       each, and bystanders that fill the rest of the table past 60 % without touching the pairs

The GPU tests (tests/test_gpu_probe_chains.py) build overflow chains with craft() and hold the table's slot census against
FirstFit.census().  Within one launch slots only go empty -> key and every inserter takes the first empty slot of its sequence,
so the SET of slots that a batch of distinct keys of ONE probe sequence occupies, and the flags it leaves, do not depend on the
order in which the keys of the batch arrive; which key sits in which of those slots does."""
import numpy as np

SLOTS = 15
STREAM = 4_000_000      # candidates per seed: ~1000 keys per (b0, b1) pair at nb = 64


def fmix64(k):
  k = np.asarray(k).astype(np.uint64)
  with np.errstate(over="ignore"):
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xff51afd7ed558ccd)
    k = k ^ (k >> np.uint64(33))
    k = k * np.uint64(0xc4ceb9fe1a85ec53)
    k = k ^ (k >> np.uint64(33))
  return k


def fmix32(x):
  x = np.asarray(x).astype(np.uint32)
  with np.errstate(over="ignore"):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85ebca6b)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xc2b2ae35)
    x = x ^ (x >> np.uint32(16))
  return x


def _mulhi32(a, nb):
  return ((a.astype(np.uint64) * np.uint64(nb)) >> np.uint64(32)).astype(np.int64)


def homes(keys, nb):
  """(b0, b1, substituted): int64 bucket indices and whether b1 is the b0 + 1 (mod nb) substitute for a b1 equal to b0."""
  nb = int(nb)
  assert 2 <= nb < 2**32
  h = fmix64(np.ascontiguousarray(keys, dtype=np.int64).view(np.uint64))
  b0 = _mulhi32((h >> np.uint64(32)).astype(np.uint32), nb)
  lo = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
  b1 = _mulhi32(fmix32(lo ^ np.uint32(0x9e3779b9)), nb)
  sub = b1 == b0
  b1 = np.where(sub, np.where(b1 + 1 == nb, 0, b1 + 1), b1)
  return b0, b1, sub


_cache = {}
_CACHE_MAX = 4


def _stream(nb, seed):
  key = (int(nb), int(seed))
  if key not in _cache:
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(-2**62, 2**62, size=STREAM, dtype=np.int64))
    rng.shuffle(keys)
    b0, b1, sub = homes(keys, nb)
    while len(_cache) >= _CACHE_MAX:
      _cache.pop(next(iter(_cache)))
    _cache[key] = (keys, b0.astype(np.int32), b1.astype(np.int32), sub)
  return _cache[key]


def craft(nb, b0=None, b1=None, substituted=None, count=1, seed=0):
  """The first `count` keys of the seed's candidate stream whose homes are (b0, b1) — None: any — and whose b1 is (True) / is not
  (False) the substitute.  Raises when the stream holds fewer: a test never runs on a shorter chain than it asked for."""
  keys, kb0, kb1, ksub = _stream(nb, seed)
  m = np.ones(keys.size, bool)
  if b0 is not None:
    m &= kb0 == int(b0)
  if b1 is not None:
    m &= kb1 == int(b1)
  if substituted is not None:
    m &= ksub == bool(substituted)
  got = keys[m]
  if count is None:       # everything the stream holds (a caller that joins several seeds)
    return got.copy()
  if got.size < count:
    raise ValueError("craft: the candidate stream (seed %d) holds %d keys with b0=%r b1=%r substituted=%r at nb=%d, %d wanted"
                     % (seed, got.size, b0, b1, substituted, nb, count))
  return got[:count].copy()


def pair_scene(nb, pairs, n_pair=75, live=None, per_bucket=13, seed=0, by_seed=1):
  """Key sets for a table of nb buckets that holds `live` keys (default: 60 % of the slots + 60) with the bucket pairs
  `pairs` = [(b0, b1), ...] full:
    keys[i]      n_pair keys whose homes are exactly pairs[i]: the first 30 are the residents (15 fill b0, 15 fill b1), the rest fresh
    bystanders   live - 30 * len(pairs) keys with neither home in a pair's {b0, b1, b1 + 1, b1 + 2} (those sets must be disjoint), at
                 most `per_bucket` (< 15) of them sharing a b0: no b0 ever fills, so every bystander sits in its b0 whatever the
                 order of arrival, and the buckets b1 + 1 / b1 + 2 of every pair stay EMPTY (a fresh pair key that walked would land
                 there and be seen)
  -> (keys, bystanders)"""
  nb = int(nb)
  assert 0 < per_bucket < SLOTS and 30 <= n_pair
  shut = []
  for b0, b1 in pairs:
    quad = [int(b0), int(b1), (int(b1) + 1) % nb, (int(b1) + 2) % nb]
    if len(set(quad)) != 4 or set(quad) & set(shut):
      raise ValueError("pair_scene: the buckets b0, b1, b1 + 1, b1 + 2 of the pairs %r overlap at nb=%d" % (pairs, nb))
    shut += quad
  keys = [craft(nb, b0=b0, b1=b1, count=n_pair, seed=seed) for b0, b1 in pairs]
  if live is None:
    live = int(0.6 * nb * SLOTS) + 60
  want = live - 30 * len(pairs)
  cand, h0, h1, _ = _stream(nb, by_seed)
  n_look = min(cand.size, 40 * max(want, 1))
  cand, h0, h1 = cand[:n_look], h0[:n_look], h1[:n_look]
  ok = ~(np.isin(h0, shut) | np.isin(h1, shut))
  occ = np.zeros(nb, np.int64)
  by = []
  for k, a in zip(cand[ok].tolist(), h0[ok].tolist()):
    if len(by) == want:
      break
    if occ[a] < per_bucket:
      occ[a] += 1
      by.append(k)
  if len(by) < want:
    raise ValueError("pair_scene: %d bystanders wanted at nb=%d, %d found (%d buckets x %d)" % (want, nb, len(by), nb - len(shut), per_bucket))
  return keys, np.array(by, np.int64)


class FirstFit:
  """Sequential model of an unbounded table of nb buckets of 15 slots that never grows."""

  def __init__(self, nb):
    self.nb = int(nb)
    self.slots = [[None] * SLOTS for _ in range(self.nb)]
    self.ovf0 = [False] * self.nb
    self.ovf1 = [False] * self.nb
    self.where = {}       # key -> (bucket, slot)
    self.was_full = [False] * self.nb

  def sequence(self, key):
    """the key's probe sequence: b0, b1, b1 + 1, ... — nb + 1 buckets, as many as an insert looks at"""
    b0, b1, _ = homes(np.array([key], np.int64), self.nb)
    seq, b = [int(b0[0])], int(b1[0])
    for _ in range(self.nb):
      seq.append(b)
      b = 0 if b + 1 == self.nb else b + 1
    return seq

  def insert(self, key):
    """locate_or_claim_from: walk while flagged, remember the first empty slot, flag a full unflagged bucket only when no empty
    slot was seen and the key goes on.  Returns True when the key is new."""
    key = int(key)
    fe = None
    for step, b in enumerate(self.sequence(key)):
      row = self.slots[b]
      if key in row:
        return False
      if fe is None and None in row:
        fe = (b, row.index(None))
      flags = self.ovf0 if step == 0 else self.ovf1
      if not flags[b]:
        if fe is not None:
          break
        flags[b] = True
    if fe is None:
      raise RuntimeError("FirstFit: no slot for key %d" % key)
    self.slots[fe[0]][fe[1]] = key
    self.where[key] = fe
    if None not in self.slots[fe[0]]:
      self.was_full[fe[0]] = True
    return True

  def find(self, key):
    """probe_find_from: the bucket the search finds the key in, or None.  Stops at the first unflagged bucket."""
    key = int(key)
    for step, b in enumerate(self.sequence(key)):
      if key in self.slots[b]:
        return b
      if not (self.ovf0 if step == 0 else self.ovf1)[b] or step >= self.nb:
        return None
    return None

  def erase(self, key):
    key = int(key)
    at = self.where.pop(key, None)
    if at is None:
      return False
    self.slots[at[0]][at[1]] = None
    return True

  def bucket_of(self, key):
    at = self.where.get(int(key))
    return None if at is None else at[0]

  def depth_of(self, key):
    """position of the key's bucket in its probe sequence (0 = b0, 1 = b1, 2 = b1 + 1, ...), None when absent"""
    b = self.bucket_of(key)
    return None if b is None else self.sequence(key).index(b)

  def full_buckets(self):
    return sum(1 for row in self.slots if None not in row)

  def ever_full(self):
    """buckets that have been full at some time: only those can carry a flag (the flags outlive an erase)"""
    return sum(self.was_full)

  def census(self):
    live = len(self.where)
    return {"live": live, "empty": self.nb * SLOTS - live, "ovf0": sum(self.ovf0), "ovf1": sum(self.ovf1)}
