"""GPU: every table entry point on crafted home-bucket collisions.

The table's protocol — first-fit placement along b0, b1, b1 + 1, ... (mod nb), two monotone overflow flags that end a search, no
tombstones (csrc/tfra_device.h) — is implemented several times over: probe_find_from / probe_find_word / locate_or_claim_from,
the ownership pass with its own stop rule and 8-step walk (own_batch16), the overlapped step, the fused appliers, the pooled
lookup, both growth paths.  Random keys at load factor <= 0.75 never fill a 15-slot bucket, so here the chains are BUILT: keys
crafted (tests/probe_model.py) to share one (b0, b1) pair on a table of ~89 buckets, 160 of them = a chain 11 buckets deep
(deeper than the ownership pass's walk, whose `why = 2` exit hands the last bucket's keys to the locked protocol), one chain that
wraps over the last bucket, a pile on the last bucket made of keys whose b1 was the b0 + 1 substitute.

Condition on every scenario: the slot census shows `live` and `empty` equal to the sequential model's; for the build in 15-key
batches through the locked insert `ovf0` / `ovf1` equal the model's exactly, for the other build paths model <= flags <= number
of buckets that ever filled; ovf1 == 0 means no chain was built and fails.  References are exact: a dict of last writes, and a roomy twin
(the same calls on a table with a large init_size, census ovf0 == 0) compared bit for bit — placement must not change a result.

nb = 2 cannot hold a chain: OVF1 is only set by a key that found both buckets full, and then the table is full and grows.  The
nb = 3 case (max_load_factor 1) holds one that wraps; the `step >= nb` cut-off needs every bucket flagged, i.e. a full table, and
stays out of reach without growth."""
import numpy as np
import pytest

from tests import probe_model as pm

pytestmark = pytest.mark.gpu

SLOTS = 15
DIM = 8
INIT = 1000            # -> 89 buckets, soft growth threshold 1001 keys
N_CHAIN, N_ABSENT, N_EXTRA, N_PILE, N_BY = 160, 32, 20, 46, 250


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _nb(tbl):
  return (tbl.capacity() - 2) // SLOTS


def _np_dt(name):
  return {"float32": np.float32, "float16": np.float16, "int32": np.int32}[name]


def _vals(keys, ver, dt="float32", dim=DIM):
  """rows that are a closed-form function of (key, version): [n, dim] numpy array of the table's dtype"""
  k = np.asarray(keys, np.int64).astype(np.uint64)
  j = np.arange(dim, dtype=np.uint64)
  with np.errstate(over="ignore"):
    x = (k[:, None] * np.uint64(2654435761) + j[None, :] * np.uint64(40503) + np.uint64(ver * 7919)) % np.uint64(65521)
  if dt == "int32":
    return x.astype(np.int32) - 30000
  return (x.astype(np.float32) / np.float32(65521.0) - np.float32(0.5)).astype(_np_dt(dt))


def _kt(torch, keys):
  return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).cuda()


def _vt(torch, vals):
  return torch.from_numpy(np.ascontiguousarray(vals)).cuda()


def _table(env, name, dt="float32", init=INIT, aux=0, mlf=0.0, aux_init=(0.0,) * 4):
  torch, _ = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  tdt = getattr(torch, dt)
  default = torch.full((DIM,), 7, dtype=tdt) if dt == "int32" else torch.full((DIM,), 0.125, dtype=tdt)
  return _DeviceTable(torch.int64, tdt, default, name, "cuda:0", dim=DIM, aux_fields=aux, init_capacity=init, max_load_factor=mlf,
                      aux_init=aux_init)


class Scn:
  """The key sets of one scenario, crafted for the table's actual bucket count."""

  def __init__(self, nb, kind):
    self.nb, self.kind = nb, kind
    if kind == "mid":
      b0, b1 = nb // 4, nb // 2
      pile = pm.craft(nb, b0=nb // 8, count=N_PILE + 60)                         # one b0, assorted b1 ...
      pile = pile[~np.isin(pm.homes(pile, nb)[1], [(b1 + j) % nb for j in range(16)])][:N_PILE]   # ... none of them on the chain
      assert pile.size == N_PILE
    else:            # "wrap": the chain runs b0, nb-2, nb-1, 0, 1, ...; the pile's b1 is the substitute that wraps to 0
      b0, b1 = nb // 4, nb - 2
      pile = pm.craft(nb, b0=nb - 1, substituted=True, count=N_PILE)
    pair = pm.craft(nb, b0=b0, b1=b1, count=N_CHAIN + N_ABSENT + N_EXTRA)
    self.b0, self.b1 = b0, b1
    self.chain, self.absent, self.extra = pair[:N_CHAIN], pair[N_CHAIN:N_CHAIN + N_ABSENT], pair[N_CHAIN + N_ABSENT:]
    self.pile = pile
    # bystanders: random keys, minus those whose placement a race inside their batch could decide (then the flags they leave would
    # depend on it): keys that touch a bucket the chain or the pile filled partly, and keys whose two home buckets are both full
    # (they walk).  What stays still meets the chain: a bystander whose b0 is a full chain bucket moves to its b1 and flags b0.
    m = pm.FirstFit(nb)
    for k in np.concatenate([self.chain, pile]):
      m.insert(k)
    occ = np.array([SLOTS - row.count(None) for row in m.slots])
    by = pm.craft(nb, count=N_BY + 600)
    by = by[~np.isin(by, np.concatenate([pair, pile]))]
    h0, h1, _ = pm.homes(by, nb)
    partly = (occ > 0) & (occ < SLOTS)
    self.by = by[~(partly[h0] | partly[h1] | ((occ[h0] == SLOTS) & (occ[h1] == SLOTS)))][:N_BY]
    assert self.by.size == N_BY
    self.chain_buckets = [b0] + [(b1 + j) % nb for j in range(10)]

  def batches(self):
    """the build, call by call: the chain in 15-key batches (batch j fills chain bucket j of the still empty table), the pile as
    one racing batch, the bystanders as one racing batch"""
    return [self.chain[a:a + SLOTS] for a in range(0, N_CHAIN, SLOTS)] + [self.pile, self.by]

  def resident(self):
    return np.concatenate([self.chain, self.pile, self.by])


def _census(tbl, model, exact, tag=""):
  """the condition on every scenario (module docstring)"""
  c, m = tbl.slot_census(), model.census()
  assert c["locked"] == 0, (tag, c)
  assert (c["live"], c["empty"]) == (m["live"], m["empty"]), (tag, c, m)
  assert c["ovf1"] > 0, (tag, "no chain was built", c)
  if exact:
    assert (c["ovf0"], c["ovf1"]) == (m["ovf0"], m["ovf1"]), (tag, c, m)
  else:
    full = model.ever_full()          # a flag on a bucket that never filled would lengthen misses for nothing
    assert m["ovf0"] <= c["ovf0"] <= full and m["ovf1"] <= c["ovf1"] <= full, (tag, c, m, full)
  return c


def _expect(ref, keys, default):
  rows = np.stack([ref.get(int(k), default) for k in keys])
  ex = np.array([int(k) in ref for k in keys])
  return rows, ex


def _check(env, tbl, ref, keys, field=0, tag=""):
  torch, _ = env
  default = tbl._default_value.cpu().numpy()
  got, ex = tbl.find(_kt(torch, keys), return_exists=True, field=field)
  want, wex = _expect(ref, keys, default)
  np.testing.assert_array_equal(ex.cpu().numpy(), wex, err_msg="%s exists" % tag)
  np.testing.assert_array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8), err_msg="%s rows" % tag)
  assert tbl.size_host() == len(ref), tag
  tbl.check_errors()
  c = tbl.slot_census()
  assert c["live"] == len(ref) and c["locked"] == 0, (tag, c)


def _own_takes(tbl, n):
  """own_upsert_unique (csrc/tfra_own.hip) takes a unique-key call while 2 n^2 / buckets < 2048"""
  return 2.0 * n * n / _nb(tbl) < 2048.0


def _sorted_export(torch, tbl, with_scores=False):
  k, v, s = tbl.export_all(with_scores=with_scores)
  o = torch.argsort(k)
  return (k[o], v[o], s[o]) if with_scores else (k[o], v[o])


# ---- the assign paths: each writes rows `vals` for `keys` (distinct) and updates the dict ------------------------------------------
def _dups(rng, keys, vals):
  """the call with a quarter of its keys repeated, shuffled -> ids, rows; the LAST occurrence of a key carries `vals`"""
  n = keys.size
  extra = rng.integers(0, n, size=max(1, n // 4))
  ids = np.concatenate([keys[extra], keys])
  rows = np.concatenate([_vals(keys[extra], 99, str(vals.dtype)), vals])
  o = np.concatenate([rng.permutation(extra.size), extra.size + rng.permutation(n)])     # every repeat in front of the real one
  return ids[o], rows[o]


def _a_locked(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  tbl.upsert(_kt(torch, keys), _vt(torch, vals))
  ref.update({int(k): v for k, v in zip(keys, vals)})


def _a_own(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  assert _own_takes(tbl, keys.size)
  tbl.upsert(_kt(torch, keys), _vt(torch, vals), unique_keys=True)
  ref.update({int(k): v for k, v in zip(keys, vals)})


def _a_notags(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  tbl.set_owner_tags(False)
  tbl.upsert(_kt(torch, keys), _vt(torch, vals), unique_keys=True)
  tbl.set_owner_tags(True)
  ref.update({int(k): v for k, v in zip(keys, vals)})


def _a_upsert_n(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  pad = np.arange(1, 8, dtype=np.int64) * 1000003 + int(rng.integers(1, 1 << 40))      # beyond the count: must stay absent
  buf = np.concatenate([keys, pad])
  rows = np.concatenate([vals, _vals(pad, 98, str(vals.dtype))])
  assert _own_takes(tbl, buf.size)
  tbl.upsert_n(_kt(torch, buf), torch.tensor([keys.size], dtype=torch.int64, device="cuda"), _vt(torch, rows))
  ref.update({int(k): v for k, v in zip(keys, vals)})
  _, ex = tbl.find(_kt(torch, pad), return_exists=True)
  assert not bool(ex.any())


def _a_sparse(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  ids, rows = _dups(rng, keys, vals)
  tbl.upsert_sparse(_kt(torch, ids), _vt(torch, rows))
  ref.update({int(k): v for k, v in zip(keys, vals)})


def _a_planned(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  ids, rows = _dups(rng, keys, vals)
  plan = SparsePlan("cuda:0", 0).build(_kt(torch, ids))
  tbl.upsert_planned(plan, _vt(torch, rows))
  torch.cuda.synchronize()
  ref.update({int(k): v for k, v in zip(keys, vals)})


def _a_field(env, tbl, keys, vals, ref, rng):
  torch, _ = env
  tbl.upsert(_kt(torch, keys), _vt(torch, vals), field=1)         # creates absent keys: field 0 zeros
  ref.update({int(k): v for k, v in zip(keys, vals)})


def _accum(unique):
  def run(env, tbl, keys, vals, ref, rng):
    """absent keys are inserted (exists False), resident ones accumulate (exists True): int32 rows, the sums are exact"""
    torch, _ = env
    ex = np.array([int(k) in ref for k in keys])
    if unique:
      assert _own_takes(tbl, keys.size)
    tbl.accum_or_assign(_kt(torch, keys), _vt(torch, vals), torch.from_numpy(ex).cuda(), unique_keys=unique)
    for k, v, e in zip(keys, vals, ex):
      ref[int(k)] = (ref[int(k)] + v) if e else v
  return run


#        name: (assign, dtype, aux fields, field the rows are read from)
PATHS = {"locked": (_a_locked, "float32", 0, 0), "own": (_a_own, "float32", 0, 0), "notags": (_a_notags, "float32", 0, 0),
         "upsert_n": (_a_upsert_n, "float32", 0, 0), "sparse": (_a_sparse, "float32", 0, 0), "planned": (_a_planned, "float32", 0, 0),
         "field": (_a_field, "float32", 1, 1), "accum_own": (_accum(True), "int32", 0, 0), "accum_locked": (_accum(False), "int32", 0, 0)}


def _build(env, tbl, scn, assign, dt, ref, model, rng, exact):
  """the scenario through one assign path; the census condition after the chain and after everything"""
  for i, b in enumerate(scn.batches()):
    assign(env, tbl, b, _vals(b, 1, dt), ref, rng)
    for k in b:
      model.insert(k)
    if i == (N_CHAIN - 1) // SLOTS:        # the chain stands, alone in the table: batch j sits in chain bucket j
      _census(tbl, model, exact, "chain")
      assert [model.bucket_of(k) for k in scn.chain[::SLOTS]] == scn.chain_buckets
      assert model.depth_of(scn.chain[-1]) == 10
  c = _census(tbl, model, False, "built")
  assert tbl.growth_stats()["growths"] == 0
  return c


# ---- 1. the hole sequence on every assign path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mid", "wrap"])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_hole_sequence(env, path, kind):
  torch, _ = env
  assign, dt, aux, field = PATHS[path]
  rng = np.random.default_rng(len(path) * 7 + len(kind))
  tbl = _table(env, "holes_%s_%s" % (path, kind), dt=dt, aux=aux)
  scn = Scn(_nb(tbl), kind)
  ref, model = {}, pm.FirstFit(scn.nb)
  # 1. build: the chain in 15-key batches, the pile, the bystanders
  _build(env, tbl, scn, assign, dt, ref, model, rng, exact=(path == "locked"))
  everything = np.concatenate([scn.resident(), scn.absent, scn.extra])
  _check(env, tbl, ref, everything, field, "built")
  if field:      # a field insert of an absent key creates it with field 0 zeros
    z = tbl.find(_kt(torch, scn.chain))
    assert not bool(z.any())
  # 2. holes in chain buckets 0 and 2
  holes = np.concatenate([scn.chain[0:15], scn.chain[30:45]])
  assert {model.bucket_of(k) for k in holes} == {scn.chain_buckets[0], scn.chain_buckets[2]}
  tbl.erase(_kt(torch, holes))
  for k in holes:
    model.erase(k)
    del ref[int(k)]
  size = len(ref)
  # 3. the keys of chain buckets 5 and 10 still hit
  deep = np.concatenate([scn.chain[75:90], scn.chain[150:160]])
  assert sorted({model.depth_of(k) for k in deep}) == [5, 10]
  _check(env, tbl, ref, np.concatenate([deep, holes]), field, "behind the holes")
  # 4. ... and are re-upserted where they are, not into the holes
  flags = tbl.slot_census()
  assign(env, tbl, deep, _vals(deep, 2, dt), ref, rng)
  for k in deep:
    assert not model.insert(k)
  if path.startswith("accum"):    # the two combinations that change nothing: present & !exists, absent & exists
    k = np.concatenate([deep[:8], scn.absent[:8]])
    ex = np.array([False] * 8 + [True] * 8)
    tbl.accum_or_assign(_kt(torch, k), _vt(torch, _vals(k, 3, dt)), torch.from_numpy(ex).cuda(), unique_keys=(path == "accum_own"))
  # 5. nothing twice
  assert tbl.size_host() == size == len(ref)
  ek = tbl.export_all()[0].cpu().numpy()
  assert ek.size == np.unique(ek).size == size
  _check(env, tbl, ref, everything, field, "re-upserted")
  _census(tbl, model, False, "re-upserted")
  # 6. 20 new keys of the pair refill the holes before anything else
  assign(env, tbl, scn.extra, _vals(scn.extra, 1, dt), ref, rng)
  for k in scn.extra:
    model.insert(k)
  assert {model.bucket_of(k) for k in scn.extra} == {scn.chain_buckets[0], scn.chain_buckets[2]}
  c = _census(tbl, model, False, "refilled")
  assert (c["ovf0"], c["ovf1"]) == (flags["ovf0"], flags["ovf1"])
  _check(env, tbl, ref, everything, field, "refilled")
  # 7. the chain goes; the flags stay and nothing of it is found
  gone = np.concatenate([scn.chain, scn.extra, scn.absent])
  tbl.erase(_kt(torch, gone))
  for k in gone:
    ref.pop(int(k), None)
  _, ex = tbl.find(_kt(torch, gone), return_exists=True, field=field)
  assert not bool(ex.any())
  assert tbl.size_host() == N_PILE + N_BY
  _check(env, tbl, ref, everything, field, "chain erased")
  assert tbl.growth_stats()["growths"] == 0


def test_one_racing_batch_builds_the_chain(env):
  """160 keys of one pair in ONE call: through the locked kernels, and through the ownership pass (every key loses its claim
  or finds its home buckets full and is handed on)."""
  torch, _ = env
  for unique in (False, True):
    tbl = _table(env, "racing_%d" % unique)
    scn = Scn(_nb(tbl), "mid")
    ref, model = {}, pm.FirstFit(scn.nb)
    rng = np.random.default_rng(3)
    for b in (scn.by, scn.chain, scn.pile):       # the chain runs through occupied buckets
      if unique:
        assert _own_takes(tbl, b.size)
      tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)), unique_keys=unique)
      ref.update({int(k): v for k, v in zip(b, _vals(b, 1))})
      for k in b:
        model.insert(k)
    _census(tbl, model, False, "racing")
    assert max(model.depth_of(k) for k in scn.chain) >= 10
    _check(env, tbl, ref, np.concatenate([scn.resident(), scn.absent]), 0, "racing")
    assert tbl.growth_stats()["growths"] == 0


def test_three_buckets_every_chain_wraps(env):
  torch, _ = env
  tbl = _table(env, "nb3", init=30, mlf=1.0)
  nb = _nb(tbl)
  assert nb == 3
  pair = pm.craft(3, b0=1, b1=2, count=50)
  keys, absent = pair[:33], pair[33:]       # (45 slots, growth past 45 keys counted by calls: 33 + 3 + 8 stay below)
  ref, model = {}, pm.FirstFit(3)
  for a in range(0, 33, SLOTS):
    b = keys[a:a + SLOTS]
    _a_locked(env, tbl, b, _vals(b, 1), ref, None)
    for k in b:
      model.insert(k)
  assert [model.bucket_of(k) for k in keys[::SLOTS]] == [1, 2, 0]
  _census(tbl, model, True, "nb3")
  _check(env, tbl, ref, pair, 0, "nb3")
  _a_own(env, tbl, keys[30:], _vals(keys[30:], 2), ref, None)        # the keys that wrapped into bucket 0, by the ownership pass
  _check(env, tbl, ref, pair, 0, "nb3 own")
  tbl.erase(_kt(torch, keys[:15]))
  for k in keys[:15]:
    model.erase(k)
    del ref[int(k)]
  _a_locked(env, tbl, absent[:8], _vals(absent[:8], 1), ref, None)   # 12 free slots at the chain's end, 15 in the hole: the hole
  for k in absent[:8]:
    model.insert(k)
  assert {model.bucket_of(k) for k in absent[:8]} == {1}
  _census(tbl, model, True, "nb3 refilled")
  _check(env, tbl, ref, pair, 0, "nb3 refilled")
  assert tbl.growth_stats()["growths"] == 0


# ---- 2. the readers ----------------------------------------------------------------------------------------------------------------
_READ = {}


def _read_fixture(env, kind, dt):
  """one chained table per (scenario, dtype), built once by the locked insert, aux field 1 scribbled: readers change nothing"""
  if (kind, dt) not in _READ:
    torch, _ = env
    tbl = _table(env, "read_%s_%s" % (kind, dt), dt=dt, aux=1)
    scn = Scn(_nb(tbl), kind)
    ref, model = {}, pm.FirstFit(scn.nb)
    _build(env, tbl, scn, _a_locked, dt, ref, model, None, exact=True)
    ref1 = {}
    res = scn.resident()
    tbl.upsert(_kt(torch, res), _vt(torch, _vals(res, 5, dt)), field=1)
    ref1.update({int(k): v for k, v in zip(res, _vals(res, 5, dt))})
    rng = np.random.default_rng(11)
    look = np.concatenate([scn.chain, scn.absent, scn.pile, scn.by[:40], scn.chain[100:160], scn.absent[:8]])   # duplicates in one call
    rng.shuffle(look)
    _census(tbl, model, False, "read fixture")
    _READ[(kind, dt)] = (tbl, scn, ref, ref1, look, model)
  return _READ[(kind, dt)]


READERS = ["find", "find_n", "find_unique", "find_field", "find_combine", "find_combine_many", "export_windows"]


@pytest.mark.parametrize("kind", ["mid", "wrap"])
@pytest.mark.parametrize("reader", READERS)
def test_readers_on_chains(env, reader, kind):
  torch, de = env
  tbl, scn, ref, ref1, look, model = _read_fixture(env, kind, "float32")
  default = tbl._default_value.cpu().numpy()
  kt = _kt(torch, look)
  want, wex = _expect(ref, look, default)
  assert wex.sum() > 250 and (~wex).sum() == N_ABSENT + 8
  if reader == "find":
    _check(env, tbl, ref, look, 0, "find")
    got = tbl.find(kt)                                            # without exists
    np.testing.assert_array_equal(got.cpu().numpy(), want)
  elif reader == "find_n":
    cnt = look.size - 13
    out = torch.full((look.size, DIM), -9.0, device="cuda")
    got, ex = tbl.find_n(kt, torch.tensor([cnt], dtype=torch.int64, device="cuda"), out=out, return_exists=True)
    np.testing.assert_array_equal(got[:cnt].cpu().numpy(), want[:cnt])
    np.testing.assert_array_equal(ex[:cnt].cpu().numpy(), wex[:cnt])
    assert bool((got[cnt:] == -9.0).all())
  elif reader == "find_unique":
    rows, uniq, idx, cnt, ex = tbl.find_unique(kt, return_exists=True)
    np.testing.assert_array_equal(rows.cpu().numpy(), want)
    np.testing.assert_array_equal(ex.cpu().numpy(), wex)
    u = int(cnt.item())
    assert u == np.unique(look).size and torch.equal(uniq[:u][idx.long()], kt)
  elif reader == "find_field":
    _check(env, tbl, ref1, look, 1, "find_field")
  elif reader in ("find_combine", "find_combine_many"):
    from tfra_amd.dynamic_embedding.table_ops import find_combine_many
    rng = np.random.default_rng(13)
    n_rows = 40
    seg = torch.from_numpy(np.sort(rng.integers(0, n_rows, size=look.size)).astype(np.int64)).cuda()
    w = torch.from_numpy((rng.integers(1, 8, size=look.size) * 0.25).astype(np.float32)).cuda()
    idx = torch.arange(look.size, dtype=torch.int32, device="cuda")
    tbl16, _, ref16, _, look16, _ = _read_fixture(env, kind, "float16")
    assert np.array_equal(look16, look)
    want16, _ = _expect(ref16, look, tbl16._default_value.cpu().numpy())
    rows16 = tbl16.find(kt)
    np.testing.assert_array_equal(rows16.cpu().numpy().view(np.uint16), want16.view(np.uint16))
    rows32 = _vt(torch, want)
    for comb, cname in enumerate(("sum", "mean", "sqrtn")):
      for wt in (None, w):
        exp32 = de.device_ops.sparse_segment_combine(rows32, idx, seg, wt, cname, n_rows)
        exp16 = de.device_ops.sparse_segment_combine(rows16.to(torch.float32), idx, seg, wt, cname, n_rows)
        if reader == "find_combine":
          got32 = tbl.find_combine(kt, seg, wt, comb, n_rows)
          got16 = tbl16.find_combine(kt, seg, wt, comb, n_rows)
        else:
          got32, got16 = find_combine_many([(tbl, kt, seg, wt, comb, n_rows), (tbl16, kt, seg, wt, comb, n_rows)])
        assert torch.equal(got32.view(torch.int32), exp32.view(torch.int32)), (cname, wt is not None)
        assert torch.equal(got16.view(torch.int32), exp16.view(torch.int32)), (cname, wt is not None)
  else:          # export in windows of 7 slots: every 15-slot chain bucket is cut in two (and three)
    ek, ev, _ = tbl.export_all(split_size=7)
    ek, ev = ek.cpu().numpy(), ev.cpu().numpy()
    assert ek.size == np.unique(ek).size == len(ref)
    assert {int(k): ev[i].tobytes() for i, k in enumerate(ek)} == {k: v.tobytes() for k, v in ref.items()}
  _census(tbl, model, False, "after " + reader)
  assert tbl.growth_stats()["growths"] == 0


# ---- 3. the fused write-back against a roomy twin ----------------------------------------------------------------------------------
def _opt(de, name):
  return {"sgd": lambda: de.optimizers.SGD(0.05), "adagrad": lambda: de.optimizers.Adagrad(0.05), "adam": lambda: de.optimizers.Adam(0.01)}[name]()


def _var(env, opt, dt, init, name):
  torch, de = env
  return de.Variable(value_dtype=getattr(torch, dt), dim=DIM, name=name, initializer=0.125, init_size=init, devices=["cuda:0"],
                     **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))


def _seed_var(env, var, scn, dt):
  """the scenario into a Variable's table by the locked insert (slots start at the optimizer's aux_init) -> model"""
  torch, _ = env
  tbl = var.tables[0]._table
  tdt = getattr(torch, dt)
  model = pm.FirstFit(_nb(tbl))
  for b in scn.batches():
    tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)).to(tdt))
    for k in b:
      model.insert(k)
  return tbl, model


def _same_tables(torch, a, b, look, n_fields, tag):
  """placement changes no result: exports sorted by key, lookups, the optimizer slots, the size — bit for bit"""
  ka, va = _sorted_export(torch, a)
  kb, vb = _sorted_export(torch, b)
  assert torch.equal(ka, kb), tag
  assert torch.equal(va.view(torch.uint8), vb.view(torch.uint8)), tag
  kt = _kt(torch, look)
  for f in range(n_fields):
    ra, ea = a.find(kt, return_exists=True, field=f)
    rb, eb = b.find(kt, return_exists=True, field=f)
    assert torch.equal(ea, eb) and torch.equal(ra.view(torch.uint8), rb.view(torch.uint8)), (tag, f)
  assert a.size_host() == b.size_host() == ka.numel(), tag
  a.check_errors()
  b.check_errors()


WRITEBACKS = ["apply_optimizer", "apply_sparse", "apply_planned", "combined", "combined_many", "step_prefetch"]
WB_CASES = [(o, "float32", h) for o in ("sgd", "adagrad", "adam") for h in WRITEBACKS] + [("adam", "float16", "apply_sparse"),
                                                                                             ("adagrad", "bfloat16", "apply_planned")]


@pytest.mark.parametrize("opt_name,dt,how", WB_CASES, ids=["%s-%s-%s" % c for c in WB_CASES])
def test_writeback_matches_roomy_twin(env, opt_name, dt, how):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan, apply_planned_combined_many
  kinds = ["mid", "wrap"] if how == "combined_many" else ["mid"]
  rng = np.random.default_rng(17)
  sides = []                         # [small tables, roomy twins]: per table (var, tbl, scn, deo)
  for init, label in ((INIT, "small"), (200_000, "roomy")):
    group = []
    for kind in kinds:
      opt = _opt(de, opt_name)
      var = _var(env, opt, dt, init, "wb_%s_%s_%s_%s_%s" % (opt_name, dt, how, kind, label))
      scn = sides[0][len(group)][2] if sides else Scn(_nb(var.tables[0]._table), kind)    # crafted for the SMALL table's bucket count
      tbl, model = _seed_var(env, var, scn, dt)
      if label == "small":
        _census(tbl, model, False, "seeded")
      else:
        c = tbl.slot_census()
        assert c["ovf0"] == 0 and c["ovf1"] == 0 and c["live"] == scn.resident().size, c
      group.append((var, tbl, scn, de.DynamicEmbeddingOptimizer(opt)))
    sides.append(group)
  n_fields = 1 + len(sides[0][0][3].opt.slots)
  dflt = torch.full((DIM,), 0.125, device="cuda")
  # ids: half chain residents at depth >= 3, a quarter repeats of them, a quarter never-seen keys of the pair (inserted by the write-back)
  steps = []
  for s in range(3):
    per_table = []
    for _, _, scn, _ in sides[0]:
      deep = scn.chain[45:][rng.permutation(N_CHAIN - 45)[:64]]
      if how == "apply_optimizer":      # takes unique keys and summed gradients
        ids = np.concatenate([deep, scn.chain[:32], scn.absent])
      else:
        ids = np.concatenate([deep, deep[rng.integers(0, 64, size=32)], scn.absent])
      rng.shuffle(ids)
      g = (rng.standard_normal((ids.size, DIM)) * 0.05).astype(np.float32)
      n_rows = 24
      seg = np.sort(rng.integers(0, n_rows, size=ids.size)).astype(np.int64)
      w = (rng.integers(1, 8, size=ids.size) * 0.25).astype(np.float32)
      go = (rng.standard_normal((n_rows, DIM)) * 0.05).astype(np.float32)
      per_table.append(dict(ids=_kt(torch, ids), g=_vt(torch, g), seg=_vt(torch, seg), w=_vt(torch, w), go=_vt(torch, go)))
    steps.append(per_table)
  outs = [[], []]
  for side, group in enumerate(sides):
    if how == "step_prefetch":
      var, tbl, scn, deo = group[0]
      ps = de.PrefetchStep(var, deo)
      ps.prime(steps[0][0]["ids"])
      for s in range(3):
        outs[side].append(ps.step(steps[s][0]["g"], steps[s + 1][0]["ids"] if s < 2 else None))
      torch.cuda.synchronize()
      continue
    for s in range(3):
      ps_ = [deo.begin_step() for _, _, _, deo in group]
      if how == "combined_many":
        reqs, plans = [], []
        for (var, tbl, scn, deo), d in zip(group, steps[s]):
          plans.append(SparsePlan("cuda:0", DIM).build(d["ids"]))
          reqs.append((tbl, plans[-1], d["go"], d["seg"], d["w"], 1, dflt))
        apply_planned_combined_many(reqs, ps_)
        torch.cuda.synchronize()
        continue
      (var, tbl, scn, deo), d, p = group[0], steps[s][0], ps_[0]
      if how == "apply_optimizer":
        tbl.apply_optimizer(p, d["ids"], d["g"], dflt)
      elif how == "apply_sparse":
        tbl.apply_sparse(p, d["ids"], d["g"], dflt)
      elif how == "apply_planned":
        plan = SparsePlan("cuda:0", DIM).build(d["ids"])
        tbl.apply_planned(p, plan, d["g"], dflt)
      else:
        plan = SparsePlan("cuda:0", DIM).build(d["ids"])
        tbl.apply_planned_combined(p, plan, d["go"], d["seg"], d["w"], 2, dflt)
      torch.cuda.synchronize()
  for i in range(len(kinds)):
    (_, a, scn, _), (_, b, _, _) = sides[0][i], sides[1][i]
    look = np.concatenate([scn.resident(), scn.absent, scn.extra])
    _same_tables(torch, a, b, look, n_fields, "%s %s" % (how, kinds[i]))
    assert a.size_host() == scn.resident().size + N_ABSENT            # the never-seen keys were inserted once each
    ca, cb = a.slot_census(), b.slot_census()
    assert ca["ovf1"] > 0 and ca["live"] == a.size_host() and cb["ovf0"] == 0, (ca, cb)
    got = a.find(_kt(torch, scn.chain[45:]))
    assert not torch.equal(got, _vt(torch, _vals(scn.chain[45:], 1)).to(got.dtype))      # the updates did land on the deep keys
    assert a.growth_stats()["growths"] == 0
  for x, y in zip(outs[0], outs[1]):
    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---- 4. the step drivers of a lookup + insert_or_assign stream, on a growing table --------------------------------------------------
@pytest.mark.parametrize("driver", ["look_ahead", "overlapped_step"])
def test_assign_step_drivers_with_the_chain_in_every_batch(env, driver):
  torch, de = env
  assign_step_driver_for, assign_step_for = de.assign_step_driver_for, de.assign_step_for
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.full((DIM,), 0.125), device="cuda:0", dim=DIM, init_size=INIT,
                         name="steps_" + driver)
  tbl = t._table
  scn = Scn(_nb(tbl), "wrap")
  ref, model = {}, pm.FirstFit(scn.nb)
  rng = np.random.default_rng(23)
  _build(env, tbl, scn, _a_locked, "float32", ref, model, rng, exact=True)
  ratio = 0.5 if driver == "look_ahead" else 0.0
  assert assign_step_driver_for(ratio) == driver
  drv = assign_step_for(t, ratio)
  fresh = pm.craft(scn.nb, count=3000, seed=1)
  fresh = fresh[~np.isin(fresh, np.concatenate([scn.resident(), scn.absent, scn.extra]))]
  batches, vals = [], []
  for s in range(6):
    b = np.concatenate([scn.chain, fresh[s * 130:(s + 1) * 130], scn.absent[:4 * s], scn.chain[rng.integers(0, N_CHAIN, size=20)]])
    rng.shuffle(b)
    batches.append(b)
    vals.append(_vals(b, 10 + s) + np.arange(b.size, dtype=np.float32)[:, None])      # repeats carry different rows: the last wins
  bt, vt = [_kt(torch, b) for b in batches], [_vt(torch, v) for v in vals]
  default = tbl._default_value.cpu().numpy()
  drv.prime(bt[0])
  for s in range(6):
    out, ex = drv.step(vt[s], bt[s + 1] if s < 5 else None, bt[s + 2] if s < 4 else None, return_exists=True)
    want, wex = _expect(ref, batches[s], default)
    np.testing.assert_array_equal(ex.cpu().numpy(), wex, err_msg="step %d" % s)
    np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg="step %d" % s)
    ref.update({int(k): v for k, v in zip(batches[s], vals[s])})
  drv.flush()
  assert tbl.growth_stats()["growths"] >= 1                       # 780 new keys on top of 456: past the threshold
  _check(env, tbl, ref, np.concatenate([scn.resident(), scn.absent, fresh[:900]]), 0, "after the steps")
  ek = tbl.export_all()[0].cpu().numpy()
  assert ek.size == np.unique(ek).size == len(ref)


# ---- 5. growth with chains in place ------------------------------------------------------------------------------------------------
def _fresh_chain(nb, b0, b1, count):
  got = np.concatenate([pm.craft(nb, b0=b0, b1=b1, count=None, seed=s) for s in range(4)])
  got = np.unique(got)
  if got.size < count:
    raise ValueError("fresh chain: %d keys of (%d, %d) at nb=%d, %d wanted" % (got.size, b0, b1, nb, count))
  return got[:count]


@pytest.mark.parametrize("how", ["reserve2", "reserve4", "insert"])
def test_growth_with_chains_in_place(env, monkeypatch, how):
  """The copying growth (rehash_kernel) and the split in place, each on a Hkv CUSTOMIZED table below max_capacity (scores) with two
  state fields.  In place every key that sat in a chain bucket other than its b0 / b1 — 130 of the chain's 160 and most of the
  pile — goes through the spill list; both paths must end with the same table."""
  torch, de = env
  exports = {}
  for mode in ("-1", "0"):
    monkeypatch.setenv("TFRA_VMM_THRESHOLD_MB", mode)
    t = de.HkvHashTable(torch.int64, torch.float32, torch.full((DIM,), 0.125), init_capacity=600, max_capacity=SLOTS * 89 * 16,
                        device="cuda:0", dim=DIM, evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, aux_fields=2, aux_init=(0.5, -1.0, 0, 0),
                        name="grow_%s_%s" % (how, mode))
    tbl = t._table
    nb0 = _nb(tbl)
    assert tbl.growth_stats()["mapped_range"] == (mode == "0")
    scn = Scn(nb0, "wrap")
    ref, score, model = {}, {}, pm.FirstFit(nb0)
    for b in scn.batches():
      sc = (np.abs(b) % 100_003 + 1).astype(np.int64)
      assert _own_takes(tbl, b.size)
      tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)), scores=_kt(torch, sc), unique_keys=True)
      ref.update({int(k): v for k, v in zip(b, _vals(b, 1))})
      score.update({int(k): int(s) for k, s in zip(b, sc)})
      for k in b:
        model.insert(k)
    _census(tbl, model, False, "before growth")
    assert tbl.growth_stats()["growths"] == 0
    assert sum(1 for k in scn.chain if model.depth_of(k) >= 2) == 130        # the spill list's share, in place
    res = scn.resident()
    slots = [{}, {}]
    for f in (1, 2):
      for a in range(0, res.size, 150):      # (a call counts its keys as new ones: small calls stay under the growth threshold)
        tbl.upsert(_kt(torch, res[a:a + 150]), _vt(torch, _vals(res[a:a + 150], 20 + f)), field=f)
      slots[f - 1].update({int(k): v for k, v in zip(res, _vals(res, 20 + f))})
    for a in range(0, res.size, 150):        # (a field insert carries no score and leaves the default 1 behind: the scores once more)
      b = res[a:a + 150]
      tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)), scores=_kt(torch, np.array([score[int(k)] for k in b], np.int64)), unique_keys=True)
    size = len(ref)
    assert tbl.size_host() == size and tbl.growth_stats()["growths"] == 0      # (the host's bound of the size is exact from here)
    ek, _, es = _sorted_export(torch, tbl, with_scores=True)
    assert ek.cpu().numpy().tolist() == sorted(ref) and es.cpu().numpy().tolist() == [score[k] for k in sorted(ref)]
    # ---- grow
    if how == "insert":
      more = pm.craft(nb0, count=1400, seed=2)       # 456 + 800 keys: past 92 % of the 1335 slots, the table has to grow first
      more = more[~np.isin(more, np.concatenate([res, scn.absent, scn.extra]))][:800]
      sc = (np.abs(more) % 100_003 + 1).astype(np.int64)
      tbl.upsert(_kt(torch, more), _vt(torch, _vals(more, 1)), scores=_kt(torch, sc), unique_keys=True)
      ref.update({int(k): v for k, v in zip(more, _vals(more, 1))})
      score.update({int(k): int(s) for k, s in zip(more, sc)})
      aux = np.broadcast_to(np.array([0.5, -1.0], np.float32)[:, None], (2, DIM))
      for f in (1, 2):
        slots[f - 1].update({int(k): aux[f - 1].copy() for k in more})
      size = len(ref)
    else:
      tbl.reserve((tbl.capacity() - 2) * (2 if how == "reserve2" else 4))
    st = tbl.growth_stats()
    nb1 = _nb(tbl)
    assert st["growths"] == 1 and st["in_place"] == (mode == "0") and nb1 == nb0 * (4 if how == "reserve4" else 2), (st, nb0, nb1)
    # ---- everything is still there: rows, scores, slots; the absent keys absent; size and live unchanged
    look = np.concatenate([np.array(sorted(ref), np.int64), scn.absent, scn.extra])
    _check(env, tbl, ref, look, 0, "grown rows")
    for f in (1, 2):
      got = tbl.find(_kt(torch, np.array(sorted(ref), np.int64)), field=f).cpu().numpy()
      np.testing.assert_array_equal(got, np.stack([slots[f - 1][k] for k in sorted(ref)]), err_msg="grown field %d" % f)
    ek, ev, es = _sorted_export(torch, tbl, with_scores=True)
    assert ek.cpu().numpy().tolist() == sorted(ref)
    assert es.cpu().numpy().tolist() == [score[k] for k in sorted(ref)]
    assert tbl.size_host() == size and tbl.slot_census()["live"] == size
    exports[mode] = (ek, ev, es, [tbl.find(ek, field=f) for f in (1, 2)])
    # ---- the hole sequence once more, on a chain crafted for the NEW bucket count (the old one has scattered)
    fc = _fresh_chain(nb1, nb1 // 4 + 7, nb1 // 2 + 5, 46 + 10)      # (buckets that are no child of the old chain's)
    fresh, fabsent = fc[:46], fc[46:]
    before = tbl.slot_census()
    for a in range(0, 46, SLOTS):
      b = fresh[a:a + SLOTS]
      tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)), scores=_kt(torch, np.full(b.size, 77, np.int64)), unique_keys=True)
      ref.update({int(k): v for k, v in zip(b, _vals(b, 1))})
    after = tbl.slot_census()
    assert after["ovf1"] >= before["ovf1"] + 2 and after["ovf0"] >= 1, (before, after)     # 46 keys of one pair: at least four buckets
    _check(env, tbl, ref, np.concatenate([fresh, fabsent, scn.chain]), 0, "fresh chain")
    tbl.erase(_kt(torch, fresh[:15]))
    for k in fresh[:15]:
      del ref[int(k)]
    _check(env, tbl, ref, np.concatenate([fresh, fabsent]), 0, "fresh chain, hole")
    b = fresh[15:]
    tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 2)), scores=_kt(torch, np.full(b.size, 78, np.int64)), unique_keys=True)
    ref.update({int(k): v for k, v in zip(b, _vals(b, 2))})
    _check(env, tbl, ref, np.concatenate([fresh, fabsent, scn.chain]), 0, "fresh chain, re-upserted")
    ek2 = tbl.export_all()[0].cpu().numpy()
    assert ek2.size == np.unique(ek2).size == len(ref)
    b = fabsent
    tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)), scores=_kt(torch, np.full(b.size, 79, np.int64)), unique_keys=True)
    ref.update({int(k): v for k, v in zip(b, _vals(b, 1))})
    assert tbl.slot_census()["ovf1"] == after["ovf1"]                      # 10 keys into the 15-slot hole: the chain does not grow
    _check(env, tbl, ref, np.concatenate([fresh, fabsent, scn.chain]), 0, "fresh chain, refilled")
  a, b = exports["-1"], exports["0"]
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
  assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])


# ---- 6. checkpoint ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_of_a_chained_table(env, tmp_path):
  torch, _ = env
  tbl = _table(env, "ckpt_src")
  scn = Scn(_nb(tbl), "wrap")
  ref, model = {}, pm.FirstFit(scn.nb)
  _build(env, tbl, scn, _a_locked, "float32", ref, model, None, exact=True)
  prefix = str(tmp_path / "chained")
  assert tbl.save(prefix) == len(ref)
  look = np.concatenate([scn.resident(), scn.absent])
  ka, va = _sorted_export(torch, tbl)
  for init in (20_000, INIT):              # another bucket count, then the same one (the chain stands again)
    t2 = _table(env, "ckpt_dst_%d" % init, init=init)
    assert (_nb(t2) == scn.nb) == (init == INIT)
    assert t2.load(prefix) == len(ref)
    _check(env, t2, ref, look, 0, "loaded %d" % init)
    kb, vb = _sorted_export(torch, t2)
    assert torch.equal(ka, kb) and torch.equal(va, vb)
    if init == INIT:      # (one racing batch in file order: another placement than the build's, a chain all the same)
      c = t2.slot_census()
      assert c["ovf1"] >= 9 and c["ovf0"] >= 1 and c["live"] == len(ref), c
      assert t2.growth_stats()["growths"] == 0


# ---- 7. a bounded table: the four buckets a new key may use, then the minimum score of the two home buckets goes ----------------------
def test_bounded_chain_evicts_the_minimum_of_the_home_buckets(env):
  torch, de = env
  cap = SLOTS * 89
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(DIM), init_capacity=cap, max_capacity=cap, device="cuda:0", dim=DIM,
                      evict_strategy=de.HkvEvictStrategy.CUSTOMIZED, name="bounded_chain")
  tbl = t._table
  nb = _nb(tbl)
  assert nb * SLOTS <= cap < 2 * nb * SLOTS          # at max_capacity: it cannot double
  pair = pm.craft(nb, b0=nb // 4, b1=nb // 2, count=61)
  keys, last = pair[:60], pair[60:]
  base = [1000, 2000, 10, 20]                       # the table-wide minimum sits in batch 2: beyond the home buckets, not a candidate
  score = {}
  model = pm.FirstFit(nb)
  for j in range(4):
    b = keys[j * SLOTS:(j + 1) * SLOTS]
    sc = base[j] + np.arange(SLOTS, dtype=np.int64)
    tbl.upsert(_kt(torch, b), _vt(torch, _vals(b, 1)), scores=_kt(torch, sc), unique_keys=True)
    score.update({int(k): int(s) for k, s in zip(b, sc)})
    for k in b:
      model.insert(k)
  assert tbl.size_host() == 60
  c = tbl.slot_census()
  assert (c["live"], c["ovf0"], c["ovf1"]) == (60, 1, 2), c      # b0, b1, b1 + 1, b1 + 2 full; far below 60 % load
  _, ex = tbl.find(_kt(torch, keys), return_exists=True)
  assert bool(ex.all())
  tbl.upsert(_kt(torch, last), _vt(torch, _vals(last, 1)), scores=_kt(torch, np.array([5000], np.int64)), unique_keys=True)
  tbl.check_errors()
  assert tbl.size_host() == 60
  got, ex = tbl.find(_kt(torch, last), return_exists=True)
  assert bool(ex.all()) and np.array_equal(got.cpu().numpy(), _vals(last, 1))
  _, ex = tbl.find(_kt(torch, keys), return_exists=True)
  gone = keys[~ex.cpu().numpy()]
  assert gone.size == 1
  homes = [k for k in keys if model.depth_of(k) <= 1]
  assert len(homes) == 30
  assert int(gone[0]) == min(homes, key=lambda k: score[int(k)])            # select_victim: minimum score of b0 and b1
  assert score[int(gone[0])] == 1000
  assert tbl.slot_census()["locked"] == 0
