"""GPU: WHICH key leaves a bounded (Hkv) table at max_capacity, whether a new key is admitted, and what score it starts with — on
every write path.

The rule (csrc/tfra_device.h, select_victim / evict_and_lock): a key that finds neither itself nor an empty slot in its two home
buckets b0 / b1 replaces the minimum-score entry among their 30 slots (ties: b0 before b1); an empty slot beats any victim; under
LFU / EPOCHLFU / CUSTOMIZED the key enters only if its compare score (EPOCHLFU: epoch << 32 | n) is >= that minimum, else it is
dropped without an error; the slot starts a new life (score from zero, aux fields at aux_init).  Six consumers act on that result
(insert_evict_kernel, the ownership pass, apply_evict_kernel, apply_csr_body<PHASE2> single and grouped, the two step drivers).

The scene (class Scene, one builder for every test): a table of 15 * 89 slots with init_capacity == max_capacity, four disjoint
bucket pairs (b0, b1) each FULL of 30 crafted residents (tests/probe_model.py: pair_scene), every resident written in a call of its
own group so that the test knows each key's score or age, and bystanders elsewhere that carry the table past 60 % of its slots —
the dense regime, where a new key is confined to b0 / b1.  The buckets b1 + 1 and b1 + 2 of every pair are EMPTY: a fresh pair key
that walked (the regime below 60 %) would land there, the size would grow and no resident would go; Scene.check names that.

No expectation comes from asking the table what is resident: the present set is computed from the scores and ages the test wrote.
Every outcome holds for any order in which the keys of a call arrive (fresh scores above every resident score unless the case
says otherwise; ages by call, never within a call).  Everything is compared bit for bit; rows written by an optimizer path against
a roomy twin that received the same calls and cannot evict.

Conditions after every call under test (Scene.check): check_errors() clean; no LOCKED slot; size_host() == census live == number
of exported keys, all distinct; every bystander untouched (row, score and aux bytes); the exported pair keys are exactly the
expected set, each with its own row and score.

What the tests found out (pinned here, stated in include/tfra_mi355x.h where it was not):
  * upsert / accum_or_assign WITHOUT unique keys answer TFRA_ERR_UNSUPPORTED at max_capacity and change nothing; so does upsert_n
    with the owner tags off.  A field insert (field != 0) never evicts.
  * an optimizer write-back counts as one upsert with in_score 1: on a CUSTOMIZED table a hit key's score BECOMES 1; a fresh key that
    is not admitted loses its gradient silently."""
import numpy as np
import pytest

from tests import probe_model as pm
from tests.test_gpu_probe_chains import PATHS, _kt, _sorted_export, _vals, _vt

pytestmark = pytest.mark.gpu

SLOTS = 15
DIM = 8
CAP = SLOTS * 89
N_PAIRS = 4


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _pairs(nb):
  """four bucket pairs whose b0, b1, b1 + 1, b1 + 2 are disjoint (pair_scene checks it)"""
  return [(nb // 16 + j * (nb // 4), nb // 16 + 7 + j * (nb // 4)) for j in range(N_PAIRS)]


_KEYS = {}


def _set_epoch(tbl, epoch):
  from tfra_amd import _capi
  _capi.call("tfra_table_set_global_epoch", tbl._h, int(epoch))


class _Scored:
  """The table as the assign functions of PATHS see it: every write carries the caller score of its keys (`score`: {key: int},
  1 for a key it does not hold; None: no scores).  Everything else is the table's."""

  def __init__(self, torch, tbl, score):
    self._torch, self._t, self._s = torch, tbl, score

  def __getattr__(self, name):
    return getattr(self._t, name)

  def _sc(self, keys):
    if self._s is None:
      return None
    k = keys.cpu().numpy().reshape(-1)
    return self._torch.from_numpy(np.array([self._s.get(int(x), 1) for x in k], np.int64)).cuda()

  def upsert(self, keys, values, scores=None, unique_keys=False, field=0):
    return self._t.upsert(keys, values, scores=self._sc(keys), unique_keys=unique_keys, field=field)

  def upsert_n(self, keys, count, values, scores=None):
    return self._t.upsert_n(keys, count, values, scores=self._sc(keys))

  def upsert_sparse(self, ids, values, scores=None):
    return self._t.upsert_sparse(ids, values, scores=self._sc(ids))

  def upsert_planned(self, plan, values, scores=None, sync=True):
    return self._t.upsert_planned(plan, values, scores=self._sc(plan.ids), sync=sync)

  def accum_or_assign(self, keys, values_or_deltas, exists, scores=None, unique_keys=False):
    return self._t.accum_or_assign(keys, values_or_deltas, exists, scores=self._sc(keys), unique_keys=unique_keys)


class Scene:
  """The scene of the module docstring.
    groups   sizes of the calls that write a pair's 30 residents (the same calls serve all four pairs): (15, 15), six fives, ...
    score    (pair, index of the resident 0..29) -> caller score, or None (LRU-type strategies)
    epochs   the global epoch set in front of each of those calls (EPOCH* strategies), then `epoch_after` for everything later
  self.present: {pair key: [row, score]} — what the table must hold of the pairs; score None = not compared (a device clock),
  ("hi", e) = the score's upper word is e."""

  def __init__(self, env, name, strategy, dt="float32", dim=DIM, aux=0, aux_init=(0.0,) * 4, groups=(15, 15), score=None, epochs=None,
               epoch_after=None, by_score=1):
    torch, de = env
    self.env, self.dt, self.dim, self.strategy, self.aux = env, dt, dim, strategy, aux
    tdt = getattr(torch, dt)
    default = torch.full((dim,), 7, dtype=tdt) if dt == "int32" else torch.full((dim,), 0.125, dtype=tdt)
    self.t = de.HkvHashTable(torch.int64, tdt, default, init_capacity=CAP, max_capacity=CAP, device="cuda:0", dim=dim,
                             evict_strategy=de.HkvEvictStrategy[strategy], step_per_epoch=0, aux_fields=aux, aux_init=aux_init, name=name)
    tbl = self.tbl = self.t._table
    nb = self.nb = (tbl.capacity() - 2) // SLOTS
    assert nb * SLOTS <= CAP < 2 * nb * SLOTS          # at max_capacity: it cannot double
    self.pairs = _pairs(nb)
    if nb not in _KEYS:         # (one bucket count: the key sets are crafted once)
      _KEYS[nb] = pm.pair_scene(nb, self.pairs)
    self.keys, self.by = _KEYS[nb]
    self.res = [k[:30] for k in self.keys]
    self.fresh = [k[30:] for k in self.keys]
    self.n_live = 30 * N_PAIRS + self.by.size
    assert sum(groups) == 30 and self.n_live > 0.6 * nb * SLOTS
    self.lru_like = strategy in ("LRU", "EPOCHLRU")
    model = pm.FirstFit(nb)
    self.present, self.group_of, lo = {}, {}, 0
    for g, size in enumerate(groups):
      if epochs is not None:
        _set_epoch(tbl, epochs[g])
      idx = np.arange(lo, lo + size)
      ks = np.concatenate([r[idx] for r in self.res])
      sc = None if score is None else np.array([score(i, int(r)) for i in range(N_PAIRS) for r in idx], np.int64)
      tbl.upsert(_kt(torch, ks), _vt(torch, self.rows(ks, 1)), scores=None if sc is None else _kt(torch, sc), unique_keys=True)
      torch.cuda.synchronize()
      for j, k in enumerate(ks.tolist()):
        model.insert(k)
        want = None
        if strategy in ("CUSTOMIZED", "LFU"):
          want = int(sc[j])
        elif strategy == "EPOCHLFU":
          want = (int(epochs[g]) << 32) | int(sc[j])
        elif strategy == "EPOCHLRU":
          want = ("hi", int(epochs[g]))
        self.present[k] = [self.rows([k], 1)[0], want]
        self.group_of[k] = g
      lo += size
      # the calls that cover a pair's first 15 residents fill b0, the rest b1 (a group never straddles the two)
      assert lo <= 15 or lo - size >= 15
      for (b0, b1), r in zip(self.pairs, self.res):
        assert {model.bucket_of(k) for k in r[idx]} == {b0 if lo <= 15 else b1}
    if epoch_after is not None:
      _set_epoch(tbl, epoch_after)
    # bystanders: one call (it carries the table past the mark: the device's density flag is up from its start), every key into its b0
    bsc = None if self.lru_like else _kt(torch, np.full(self.by.size, by_score, np.int64))
    tbl.upsert(_kt(torch, self.by), _vt(torch, self.rows(self.by, 1)), scores=bsc, unique_keys=True)
    torch.cuda.synchronize()
    for k in self.by:
      model.insert(k)
    h0 = pm.homes(self.by, nb)[0]
    assert [model.bucket_of(k) for k in self.by] == h0.tolist()
    for _, b1 in self.pairs:
      assert model.slots[(b1 + 1) % nb] == [None] * SLOTS and model.slots[(b1 + 2) % nb] == [None] * SLOTS
    for _ in range(3):     # the host learns the density from asynchronous size reads: give it calls to complete in
      s = self.by[:16]
      tbl.upsert(_kt(torch, s), _vt(torch, self.rows(s, 1)), scores=None if bsc is None else bsc[:16], unique_keys=True)
      torch.cuda.synchronize()
    # the start state, once: bystanders as they are from here on (their scores: device clocks under LRU), the pairs as written
    k, v, s = _sorted_export(torch, tbl, with_scores=True)
    isby = torch.from_numpy(np.isin(k.cpu().numpy(), self.by)).cuda()
    self.by_snap = (k[isby].clone(), v[isby].clone(), s[isby].clone())
    assert np.array_equal(self.by_snap[0].cpu().numpy(), np.sort(self.by))
    np.testing.assert_array_equal(self.by_snap[1].cpu().numpy().view(np.uint8), self.rows(np.sort(self.by), 1).view(np.uint8))
    if strategy == "CUSTOMIZED":
      assert bool((self.by_snap[2] == by_score).all())
    self.by_aux = [tbl.find(self.by_snap[0], field=f).clone() for f in range(1, aux + 1)]
    self.check("built")

  # ---- helpers
  def rows(self, keys, ver):
    return _vals(np.asarray(keys, np.int64), ver, self.dt, self.dim)

  def scored(self, score):
    return _Scored(self.env[0], self.tbl, score)

  def pair_of(self, key):
    for i, k in enumerate(self.keys):
      if key in k:
        return "pair %d key %d" % (i, int(np.nonzero(k == key)[0][0]))
    return "no pair key"

  def snap(self):
    """the whole table, sorted by key: keys, rows, scores, aux fields"""
    torch = self.env[0]
    k, v, s = _sorted_export(torch, self.tbl, with_scores=True)
    return [k, v, s] + [self.tbl.find(k, field=f) for f in range(1, self.aux + 1)]

  def same(self, a, b, tag):
    torch = self.env[0]
    for x, y in zip(a, b):
      assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), tag

  def check(self, tag, scores=True):
    """the conditions after every call under test (module docstring), against self.present"""
    torch, tbl = self.env[0], self.tbl
    tbl.check_errors()
    c = tbl.slot_census()
    assert c["locked"] == 0, (tag, c)
    k, v, s = _sorted_export(torch, tbl, with_scores=True)
    kn = k.cpu().numpy()
    assert kn.size == np.unique(kn).size == tbl.size_host() == c["live"], (tag, kn.size, c)
    isby = np.isin(kn, self.by)
    pk = kn[~isby]
    want = np.array(sorted(self.present), np.int64)
    if pk.size > want.size and want.size == 30 * N_PAIRS and set(want.tolist()) <= set(pk.tolist()):
      raise AssertionError("%s: the dense regime was not on — %d pair keys more than the pairs' 120 slots hold: fresh keys walked to "
                           "b1 + 1 instead of evicting" % (tag, pk.size - want.size))
    if not np.array_equal(pk, want):
      missing = [self.pair_of(x) for x in sorted(set(want.tolist()) - set(pk.tolist()))]
      extra = [self.pair_of(x) for x in sorted(set(pk.tolist()) - set(want.tolist()))]
      raise AssertionError("%s: pair keys expected and not resident: %s; resident and not expected: %s" % (tag, missing, extra))
    assert kn.size == self.n_live, (tag, "size", kn.size, self.n_live)
    # bystanders: untouched
    m = torch.from_numpy(isby).cuda()
    bk, bv, bs = k[m], v[m], s[m]
    assert torch.equal(bk, self.by_snap[0]), tag
    assert torch.equal(bv.view(torch.uint8), self.by_snap[1].view(torch.uint8)), (tag, "bystander rows")
    assert torch.equal(bs, self.by_snap[2]), (tag, "bystander scores")
    for f, a in enumerate(self.by_aux):
      assert torch.equal(tbl.find(bk, field=f + 1).view(torch.uint8), a.view(torch.uint8)), (tag, "bystander aux", f + 1)
    # the pairs: each present key carries exactly its own row and score
    pv, ps = v.cpu().numpy()[~isby], s.cpu().numpy()[~isby]
    for i, x in enumerate(pk.tolist()):
      row, sc = self.present[x]
      assert pv[i].tobytes() == row.tobytes(), (tag, "row of", self.pair_of(x), pv[i], row)
      if not scores or sc is None:
        continue
      if isinstance(sc, tuple):
        assert int(ps[i]) >> 32 == sc[1], (tag, "epoch word of", self.pair_of(x), hex(int(ps[i])), sc)
      else:
        assert int(ps[i]) == sc, (tag, "score of", self.pair_of(x), int(ps[i]), sc)

  def order(self, pair, cmp_of=None):
    """the pair's present keys, the next victim first: by expected score (ties: written in b0 first is NOT modelled — a test
    that needs a tie states its victim itself).  Raises when the order of two keys is not determined."""
    ks = [k for k in self.keys[pair].tolist() if k in self.present]
    return sorted(ks, key=lambda k: self.present[k][1])

  def evict(self, pair, fresh, in_scores, new_scores, ver):
    """model of one call's fresh keys of a pair, all admitted: the len(fresh) lowest-scoring present keys go (their order must be
    determined: distinct scores up to the cut), the fresh keys enter with `new_scores` and rows of version `ver`"""
    order = self.order(pair)
    f = len(fresh)
    assert len(order) == 30 and f <= 30
    sc = [self.present[k][1] for k in order]
    if f < 30:
      assert sc[f - 1] < sc[f], "the victim set of this call is not determined by the scores"
      assert min(in_scores) >= sc[f - 1], "a fresh key of this call might not be admitted"
    for k in order[:f]:
      del self.present[k]
    for k, ns in zip(fresh, new_scores):
      self.present[int(k)] = [self.rows([k], ver)[0], ns]
    return order[:f]


def _distinct_scores(seed, base=1000, step=3):
  """(pair, resident) -> base + step * a per-pair permutation of 0..29: distinct, and the low ones sit in both buckets"""
  perm = [np.random.default_rng(seed + i).permutation(30) for i in range(N_PAIRS)]
  return lambda i, r: base + step * int(perm[i][r])


def _assign(scn, path, keys, ver, score=None, tags=True, seed=0):
  """rows of version `ver` for `keys` through one entry of PATHS, with caller scores `score` ({key: int} or None)"""
  torch = scn.env[0]
  fn = PATHS[path][0]
  keys = np.asarray(keys, np.int64)
  if not tags:
    scn.tbl.set_owner_tags(False)
  try:
    fn(scn.env, scn.scored(score), keys, scn.rows(keys, ver), {}, np.random.default_rng(seed))     # ({}: accum sends exists = False)
  finally:
    scn.tbl.set_owner_tags(True)
  torch.cuda.synchronize()


def _unsupported(scn, path, keys, score, tags=True):
  """the path answers TFRA_ERR_UNSUPPORTED and leaves the table byte-identical"""
  from tfra_amd import _capi
  before = scn.snap()
  with pytest.raises(_capi.TfraError) as e:
    _assign(scn, path, keys, 2, score, tags)
  assert e.value.code == _capi.ERR_UNSUPPORTED, e.value
  scn.same(before, scn.snap(), path + " refused")
  scn.check(path + " refused")


# the assign paths a bounded table at max_capacity takes (name in PATHS, owner tags); int32 rows for accum
EVICTING = [("own", True), ("notags", True), ("upsert_n", True), ("sparse", True), ("sparse", False), ("planned", True), ("planned", False),
            ("accum_own", True), ("accum_own", False)]
REFUSING = [("locked", True), ("accum_locked", True), ("upsert_n", False)]
FEW = [("own", True), ("notags", True), ("planned", True), ("planned", False), ("accum_own", True), ("accum_own", False)]


def _pid(p):
  return "%s-%s" % (p[0], "tags" if p[1] else "notags")


# ---- 1. the victim set -------------------------------------------------------------------------------------------------------------------
F_CALL1, F_CALL2 = (1, 4, 15, 30), (30, 1, 4, 15)


@pytest.mark.parametrize("path", EVICTING + REFUSING + [("field", True)], ids=_pid)
def test_victim_set_customized(env, path):
  """One call carries F = 1, 4, 15 and 30 fresh keys for the four pairs, scores above every resident: exactly the F lowest-scoring
  residents of each pair go, everything else keeps row and score, the size does not change.  A second call (F rotated, scores above
  the first call's) takes the next lowest — residents and, where they are used up, the first call's keys."""
  name, tags = path
  dt, aux = PATHS[name][1], PATHS[name][2]
  scn = Scene(env, "ev_set_%s_%d" % (name, tags), "CUSTOMIZED", dt=dt, aux=aux, score=_distinct_scores(1))
  used = [0] * N_PAIRS
  for call, fs in enumerate((F_CALL1, F_CALL2)):
    fresh = [scn.fresh[i][used[i]:used[i] + f] for i, f in enumerate(fs)]
    keys = np.concatenate(fresh)
    score = {int(k): 5000 * (call + 1) + j for j, k in enumerate(keys)}
    if path in REFUSING:
      _unsupported(scn, name, keys, score, tags)
      return
    if name == "field":      # a field insert never evicts (include/tfra_mi355x.h): no resident changes, whatever becomes of the new keys
      before = scn.snap()
      _assign(scn, name, keys, 2, score, tags)
      after = scn.snap()
      old = np.isin(after[0].cpu().numpy(), before[0].cpu().numpy())
      assert int(old.sum()) == before[0].numel()
      scn.same(before, [x[scn.env[0].from_numpy(old).cuda()] for x in after], "field insert")
      return
    for i, f in enumerate(fresh):
      scn.evict(i, f, [score[int(k)] for k in f], [score[int(k)] for k in f], 2 + call)
      used[i] += f.size
    _assign(scn, name, keys, 2 + call, score, tags, seed=call)
    scn.check("%s call %d" % (_pid(path), call))


# ---- 2. admission -----------------------------------------------------------------------------------------------------------------------
def _word(strategy, epoch, n):
  return (epoch << 32) | n if strategy == "EPOCHLFU" else n


@pytest.mark.parametrize("path", FEW, ids=_pid)
@pytest.mark.parametrize("strategy", ["CUSTOMIZED", "LFU", "EPOCHLFU"])
def test_admission(env, strategy, path):
  """Below the pair's minimum: dropped, the whole export byte-identical, no error.  Equal to it: admitted, the minimum goes.  One call
  with both kinds: the union.  LFU: the caller's scores are the increments, a new key's count is its own (a new life).  EPOCHLFU:
  the compare word is epoch << 32 | count — in the residents' epoch a count below every resident's is dropped, one epoch later a
  count of 1 beats them all."""
  name, tags = path
  epoch = 5
  scn = Scene(env, "ev_adm_%s_%s_%d" % (strategy, name, tags), strategy, dt=PATHS[name][1], score=_distinct_scores(2),
              epochs=[epoch, epoch] if strategy == "EPOCHLFU" else None)
  mins = [scn.order(i)[0] for i in range(N_PAIRS)]
  lo = [scn.present[m][1] & 0xffffffff for m in mins]
  assert lo == [1000] * N_PAIRS
  # (a) one fresh key per pair scoring minimum - 1
  before = scn.snap()
  keys = np.array([scn.fresh[i][0] for i in range(N_PAIRS)], np.int64)
  _assign(scn, name, keys, 2, {int(k): lo[i] - 1 for i, k in enumerate(keys)}, tags)
  scn.same(before, scn.snap(), "below the minimum")
  scn.check("below the minimum")
  # (b) the same keys scoring exactly the minimum
  for i, k in enumerate(keys):
    gone = scn.evict(i, [k], [_word(strategy, epoch, lo[i])], [_word(strategy, epoch, lo[i])], 3)
    assert gone == [mins[i]]
  _assign(scn, name, keys, 3, {int(k): lo[i] for i, k in enumerate(keys)}, tags)
  scn.check("equal to the minimum")
  # (c) per pair two keys below everything and three above everything, in one call
  low = [scn.fresh[i][1:3] for i in range(N_PAIRS)]
  high = [scn.fresh[i][3:6] for i in range(N_PAIRS)]
  score = {}
  for i in range(N_PAIRS):
    score.update({int(k): 10 + j for j, k in enumerate(low[i])})
    score.update({int(k): 7000 + 10 * i + j for j, k in enumerate(high[i])})
    w = [_word(strategy, epoch, score[int(k)]) for k in high[i]]
    scn.evict(i, high[i], w, w, 4)
  _assign(scn, name, np.concatenate(low + high), 4, score, tags, seed=1)
  scn.check("below and above in one call")
  if strategy != "EPOCHLFU":
    return
  # (d) a later epoch: count 1 beats every count of the earlier one; the victim is the minimum of the whole word
  _set_epoch(scn.tbl, epoch + 1)
  keys = np.array([scn.fresh[i][6] for i in range(N_PAIRS)], np.int64)
  for i, k in enumerate(keys):
    scn.evict(i, [k], [((epoch + 1) << 32) | 1], [((epoch + 1) << 32) | 1], 5)
  _assign(scn, name, keys, 5, {int(k): 1 for k in keys}, tags)
  scn.check("count 1, one epoch later")


# ---- 3. the tie rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FEW, ids=_pid)
def test_tie_goes_to_b0(env, path):
  """The minimum is held by one key of b0 (written in call 1) and one of b1 (call 2): the b0 key goes first, then the b1 key."""
  name, tags = path
  base = _distinct_scores(3)
  scn = Scene(env, "ev_tie_%s_%d" % (name, tags), "CUSTOMIZED", dt=PATHS[name][1], score=lambda i, r: 500 if r in (3 + i, 20 + i) else base(i, r))
  for rnd, r in enumerate((3, 20)):
    keys = np.array([scn.fresh[i][rnd] for i in range(N_PAIRS)], np.int64)
    score = {int(k): 8000 + 10 * rnd + i for i, k in enumerate(keys)}
    for i, k in enumerate(keys):
      victim = int(scn.res[i][r + i])
      assert scn.present[victim][1] == 500 == min(v[1] for x, v in scn.present.items() if x in scn.keys[i])
      del scn.present[victim]
      scn.present[int(k)] = [scn.rows([k], 2)[0], score[int(k)]]
    _assign(scn, name, keys, 2, score, tags)
    scn.check("tie, round %d" % rnd)


# ---- 4. a new life ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [("own", True), ("notags", True), ("sparse", True), ("planned", False)], ids=_pid)
@pytest.mark.parametrize("strategy", ["LFU", "EPOCHLFU"])
def test_new_life_score_and_aux(env, strategy, path):
  """The victim's count and aux bytes do not live on: the new key's count is its in_score (EPOCHLFU: epoch << 32 | in_score), its
  aux field is at aux_init.  (A field insert of a resident key counts as one upsert: count + 1.)"""
  torch = env[0]
  name, tags = path
  epoch = 9
  scn = Scene(env, "ev_life_%s_%s_%d" % (strategy, name, tags), strategy, aux=1, aux_init=(0.5, 0, 0, 0), score=_distinct_scores(4),
              epochs=[epoch, epoch] if strategy == "EPOCHLFU" else None)
  res = np.concatenate(scn.res)
  scn.tbl.upsert(_kt(torch, res), _vt(torch, scn.rows(res, 30)), field=1)      # the victims' aux bytes: not the default
  for k in res.tolist():
    scn.present[k][1] += 1
  scn.check("aux written")
  got = scn.tbl.find(_kt(torch, res), field=1)
  np.testing.assert_array_equal(got.cpu().numpy(), scn.rows(res, 30))
  fresh = [scn.fresh[i][:3] for i in range(N_PAIRS)]
  keys = np.concatenate(fresh)
  score = {int(k): 2000 + j for j, k in enumerate(keys)}       # above every resident count (<= 1000 + 87 + 1)
  for i, f in enumerate(fresh):
    w = [_word(strategy, epoch, score[int(k)]) for k in f]
    scn.evict(i, f, w, w, 2)
  _assign(scn, name, keys, 2, score, tags)
  scn.check("new life")
  aux = scn.tbl.find(_kt(torch, keys), field=1)
  assert bool((aux == 0.5).all()), aux
  stay = np.array([k for k in res.tolist() if k in scn.present], np.int64)
  np.testing.assert_array_equal(scn.tbl.find(_kt(torch, stay), field=1).cpu().numpy(), scn.rows(stay, 30))


@pytest.mark.parametrize("how", ["sparse", "planned", "planned-notags"])
def test_lfu_sparse_counts_occurrences(env, how):
  """upsert_sparse on LFU without scores: a key occurring 3 times in the call has in_score 3 — admitted against a minimum of 3
  (pairs 0, 1), dropped against a minimum of 4 (pairs 2, 3); an admitted key's count is 3."""
  torch = env[0]
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  base = _distinct_scores(5)
  scn = Scene(env, "ev_occ_" + how, "LFU", score=lambda i, r: (3 if i < 2 else 4) if r == 11 + 4 * i else base(i, r))
  keys = np.array([scn.fresh[i][0] for i in range(N_PAIRS)], np.int64)
  ids = np.concatenate([keys, keys[::-1], keys])
  for i in (0, 1):
    assert scn.evict(i, [keys[i]], [3], [3], 2) == [int(scn.res[i][11 + 4 * i])]
  rows = _vt(torch, scn.rows(ids, 2))
  if how == "sparse":
    scn.tbl.upsert_sparse(_kt(torch, ids), rows)
  else:
    scn.tbl.set_owner_tags(how == "planned")
    plan = SparsePlan("cuda:0", 0).build(_kt(torch, ids))
    scn.tbl.upsert_planned(plan, rows)
    scn.tbl.set_owner_tags(True)
  torch.cuda.synchronize()
  scn.check("three occurrences")


# ---- 5. an empty slot beats a victim ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FEW, ids=_pid)
def test_empty_slot_beats_victim(env, path):
  """Three residents that are not among the lowest are erased, five fresh keys arrive in one call: all five are present, exactly the
  two lowest residents are gone, the pair holds 30 keys again."""
  torch = env[0]
  name, tags = path
  scn = Scene(env, "ev_empty_%s_%d" % (name, tags), "CUSTOMIZED", dt=PATHS[name][1], score=_distinct_scores(6))
  erased = []
  for i in range(N_PAIRS):
    order = scn.order(i)
    erased += [order[7], order[16], order[29]]
  scn.tbl.erase(_kt(torch, np.array(erased, np.int64)))
  for k in erased:
    del scn.present[k]
  scn.n_live -= len(erased)
  scn.check("erased")
  fresh = [scn.fresh[i][:5] for i in range(N_PAIRS)]
  keys = np.concatenate(fresh)
  score = {int(k): 6000 + j for j, k in enumerate(keys)}
  for i, f in enumerate(fresh):
    order = scn.order(i)
    assert len(order) == 27
    for k in order[:2]:
      del scn.present[k]
    for k in f:
      scn.present[int(k)] = [scn.rows([k], 2)[0], score[int(k)]]
  scn.n_live += len(erased)
  _assign(scn, name, keys, 2, score, tags)
  scn.check("three empty slots, five keys")


# ---- 6. LRU / EPOCHLRU: the oldest call goes ----------------------------------------------------------------------------------------------
class Ages:
  """who is oldest, by call: {key: age}; a call's keys share one age, so a victim set is determined only where it ends on a
  boundary between two ages — asserted at every use"""

  def __init__(self, scn):
    self.scn, self.age, self.now = scn, dict(scn.group_of), max(scn.group_of.values()) + 1

  def call(self, hits, fresh, ver, score=None):
    """one write call: the hits are written first (phase 1), then each fresh key of a pair replaces that pair's oldest key"""
    scn = self.scn
    for k in hits:
      assert int(k) in scn.present
      self.age[int(k)] = self.now
      scn.present[int(k)] = [scn.rows([k], ver)[0], score]
    gone = []
    for i in range(N_PAIRS):
      f = [int(k) for k in fresh if int(k) in scn.keys[i]]
      if not f:
        continue
      order = sorted((k for k in scn.keys[i].tolist() if k in scn.present), key=lambda k: self.age[k])
      assert len(order) == 30
      assert len(f) == 30 or self.age[order[len(f) - 1]] < self.age[order[len(f)]], "the victim set of this call is not determined by the ages"
      for k in order[:len(f)]:
        del scn.present[k]
        del self.age[k]
      gone += order[:len(f)]
      for k in f:
        self.age[k] = self.now
        scn.present[k] = [scn.rows([k], ver)[0], score]
    self.now += 1
    return gone


@pytest.mark.parametrize("path", FEW, ids=_pid)
@pytest.mark.parametrize("strategy", ["LRU", "EPOCHLRU"])
def test_lru_order(env, strategy, path):
  """Residents in six calls of five.  F = 5 (pairs 0, 1) and F = 10 (pairs 2, 3) remove exactly the oldest groups; a re-upsert makes
  a group the youngest; a find protects nobody.  EPOCHLRU: every call has an epoch of its own, NOT in the order of the calls (the
  engine takes any epoch it is given): the epoch word decides, a group written later under a lower epoch goes first."""
  torch = env[0]
  name, tags = path
  epochs = [12, 10, 14, 11, 15, 13] if strategy == "EPOCHLRU" else None
  scn = Scene(env, "ev_lru_%s_%s_%d" % (strategy, name, tags), strategy, dt=PATHS[name][1], groups=(5,) * 6, epochs=epochs, epoch_after=20)
  ages = Ages(scn)
  if epochs:
    ages.age = {k: epochs[g] for k, g in scn.group_of.items()}
    ages.now = 20
  by_age = sorted(range(6), key=lambda g: epochs[g] if epochs else g)       # the groups, the oldest first
  group = lambda i, j: scn.res[i][5 * by_age[j]:5 * by_age[j] + 5]
  mark = ("hi", 20) if epochs else None
  # 1. five / ten fresh keys
  fresh = np.concatenate([scn.fresh[i][:5 if i < 2 else 10] for i in range(N_PAIRS)])
  gone = ages.call([], fresh, 2, mark)
  want = np.concatenate([group(0, 0), group(1, 0), group(2, 0), group(2, 1), group(3, 0), group(3, 1)])
  assert sorted(gone) == sorted(want.tolist())
  _assign(scn, name, fresh, 2, None, tags)
  scn.check("the oldest groups")
  # 2. the oldest group that is left is written again; the next one is looked up
  if epochs:
    _set_epoch(scn.tbl, 21)
    ages.now, mark = 21, ("hi", 21)
  again = np.concatenate([group(i, 1 if i < 2 else 2) for i in range(N_PAIRS)])
  if name.startswith("accum"):     # (accum of a resident key with exists = False changes nothing: the plain unique upsert renews it)
    scn.tbl.upsert(_kt(torch, again), _vt(torch, scn.rows(again, 3)), unique_keys=True)
    torch.cuda.synchronize()
  else:
    _assign(scn, name, again, 3, None, tags)
  ages.call(again, [], 3, mark)
  scn.check("re-upserted")
  found = np.concatenate([group(i, 2 if i < 2 else 3) for i in range(N_PAIRS)])
  rows, ex = scn.tbl.find(_kt(torch, found), return_exists=True)
  assert bool(ex.all())
  np.testing.assert_array_equal(rows.cpu().numpy(), scn.rows(found, 1))
  # 3. five more fresh keys per pair: the looked-up group goes
  if epochs:
    _set_epoch(scn.tbl, 22)
    ages.now, mark = 22, ("hi", 22)
  fresh = np.concatenate([scn.fresh[i][10:15] for i in range(N_PAIRS)])
  gone = ages.call([], fresh, 4, mark)
  assert sorted(gone) == sorted(found.tolist())
  _assign(scn, name, fresh, 4, None, tags, seed=1)
  scn.check("the found group")


# ---- 7. the optimizer write paths -------------------------------------------------------------------------------------------------------
def _opt(de, name):
  return de.optimizers.SGD(0.05) if name == "sgd" else de.optimizers.Adam(0.01)


HOWS = ["apply_optimizer", "apply_sparse", "apply_planned", "combined", "combined_many"]
OPT_CASES = ([(s, h, "adam", "float32") for s in ("LRU", "LFU", "CUSTOMIZED", "EPOCHLFU") for h in HOWS] +
             [(s, h, "sgd", "float32") for s in ("LRU", "LFU", "CUSTOMIZED", "EPOCHLFU") for h in ("apply_optimizer", "apply_planned")] +
             [(s, h, "adam", "float16") for s in ("LRU", "LFU") for h in ("apply_sparse", "combined_many")])


class _Writer:
  """one side (the scene's table or its roomy twin) of an optimizer write path: the same ids, gradients and step parameters"""

  def __init__(self, env, tbl, how, opt_name, dim, other):
    torch, de = env
    self.env, self.tbl, self.how, self.dim, self.other = env, tbl, how, dim, other
    self.deo = [de.DynamicEmbeddingOptimizer(_opt(de, opt_name)) for _ in range(2)]
    self.dflt = torch.full((dim,), 0.125, device="cuda")

  def apply(self, d):
    torch, _ = self.env
    from tfra_amd.dynamic_embedding.table_ops import SparsePlan, apply_planned_combined_many
    p = self.deo[0].begin_step()
    tbl, how = self.tbl, self.how
    if how == "apply_optimizer":
      tbl.apply_optimizer(p, d["uids"], d["ug"], self.dflt)
    elif how == "apply_sparse":
      tbl.apply_sparse(p, d["ids"], d["g"], self.dflt)
    elif how == "apply_planned":
      tbl.apply_planned(p, SparsePlan("cuda:0", self.dim).build(d["ids"]), d["g"], self.dflt)
    elif how == "combined":
      tbl.apply_planned_combined(p, SparsePlan("cuda:0", self.dim).build(d["ids"]), d["go"], d["seg"], d["w"], 2, self.dflt)
    else:
      plans = [SparsePlan("cuda:0", self.dim).build(d["ids"]), SparsePlan("cuda:0", self.dim).build(d["oids"])]
      reqs = [(tbl, plans[0], d["go"], d["seg"], d["w"], 1, self.dflt), (self.other, plans[1], d["go"], d["oseg"], None, 0, self.dflt)]
      apply_planned_combined_many(reqs, [p, self.deo[1].begin_step()])
    torch.cuda.synchronize()


def _batch(env, rng, how, hits, fresh, dim):
  """the operands of one write-back: unique keys and gradients for apply_optimizer, else ids with every hit three times"""
  torch = env[0]
  uids = np.concatenate([hits, fresh]).astype(np.int64)
  ids = np.concatenate([hits, hits, fresh, hits]).astype(np.int64)
  rng.shuffle(ids)
  n_rows = 12
  other = np.arange(1, 41, dtype=np.int64) * 7919
  return dict(uids=_kt(torch, uids), ug=_vt(torch, (rng.standard_normal((uids.size, dim)) * 0.05).astype(np.float32)),
              ids=_kt(torch, ids), g=_vt(torch, (rng.standard_normal((ids.size, dim)) * 0.05).astype(np.float32)),
              go=_vt(torch, (rng.standard_normal((n_rows, dim)) * 0.05).astype(np.float32)),
              seg=_vt(torch, np.sort(rng.integers(0, n_rows, size=ids.size)).astype(np.int64)),
              w=_vt(torch, (rng.integers(1, 8, size=ids.size) * 0.25).astype(np.float32)),
              oids=_kt(torch, other), oseg=_vt(torch, np.sort(rng.integers(0, n_rows, size=other.size)).astype(np.int64)))


@pytest.mark.parametrize("strategy,how,opt_name,dt", OPT_CASES, ids=["%s-%s-%s-%s" % c for c in OPT_CASES])
def test_optimizer_write_paths(env, strategy, how, opt_name, dt):
  """The fused write-backs (in_score fixed at 1) against a roomy twin that received the same calls and cannot evict.
  LRU: residents in calls of 1, 1, 13 and 15 keys; one call = hits on the oldest key (three times in the sparse forms) plus one fresh
  key per pair: the hit is written before anything is evicted, so the SECOND-oldest key goes, the hit key continues from its old row
  and slots, the fresh key starts from the default row and aux_init.
  LFU / CUSTOMIZED / EPOCHLFU (compare word 1 resp. epoch << 32 | 1): pairs 0, 1 hold exactly one resident of count / score 1 — the fresh
  key is admitted, that resident goes, the new count is 1; in pairs 2, 3 every resident has >= 2 — the fresh key is dropped without
  an error.  Hits count + 1 per call (none under CUSTOMIZED, where a write-back sets a hit's score to 1)."""
  torch, de = env
  dim = 6 if how == "apply_optimizer" else DIM
  opt = _opt(de, opt_name)
  S = len(opt.slots)
  epoch = 7
  base = _distinct_scores(7, base=40)
  low = lambda i, r: 1 if (i < 2 and r == 9 + 7 * i) else base(i, r)
  scn = Scene(env, "ev_opt_%s_%s_%s_%s" % (strategy, how, opt_name, dt), strategy, dt=dt, dim=dim, aux=S, aux_init=opt.aux_init(),
              groups=(1, 1, 13, 15) if strategy == "LRU" else (15, 15), score=None if strategy == "LRU" else low,
              epochs=[epoch, epoch] if strategy == "EPOCHLFU" else None)
  tdt = getattr(torch, dt)
  mk = lambda name: de.CuckooHashTable(torch.int64, tdt, torch.full((dim,), 0.125, dtype=tdt), device="cuda:0", dim=dim, init_size=200_000,
                                       aux_fields=S, aux_init=opt.aux_init(), name=name)._table
  twin = mk("ev_twin")
  res = np.concatenate(scn.res)
  twin.upsert(_kt(torch, res), _vt(torch, scn.rows(res, 1)))
  sides = [_Writer(env, scn.tbl, how, opt_name, dim, mk("ev_other_a")), _Writer(env, twin, how, opt_name, dim, mk("ev_other_b"))]
  rng = np.random.default_rng(31)
  ages = Ages(scn) if strategy == "LRU" else None

  def run(hits, fresh, tag):
    d = _batch(env, rng, how, hits, fresh, dim)
    for w in sides:
      w.apply(d)
    # what the table holds of the pairs carries the twin's bytes, every field
    keys = np.array(sorted(scn.present), np.int64)
    got = twin.find(_kt(torch, keys)).cpu().numpy()
    for k, row in zip(keys.tolist(), got):
      scn.present[k][0] = row
    scn.check(tag)
    for f in range(1, S + 1):
      a, b = scn.tbl.find(_kt(torch, keys), field=f), twin.find(_kt(torch, keys), field=f)
      assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (tag, "slot", f)

  if strategy == "LRU":
    # warm-up, group by group in the order of the ages: every resident has a state of its own, who is oldest is unchanged
    lo = 0
    for size in (1, 1, 13, 15):
      hits = np.concatenate([r[lo:lo + size] for r in scn.res])
      ages.call(hits, [], 1)
      run(hits, np.zeros(0, np.int64), "warm-up")
      lo += size
    hits = np.array([r[0] for r in scn.res], np.int64)
    fresh = np.array([f[0] for f in scn.fresh], np.int64)
    gone = ages.call(hits, fresh, 1)
    assert sorted(gone) == sorted(int(r[1]) for r in scn.res)          # the second-oldest: the hit was written first
    run(hits, fresh, "hit the oldest, one fresh key")
    assert not np.array_equal(scn.present[int(hits[0])][0], scn.rows(hits[:1], 1)[0])      # the updates did land
    return
  hit_idx = [] if strategy == "CUSTOMIZED" else [2, 17, 23]

  def bump(hits):
    for k in hits.tolist():
      s = scn.present[k][1]
      scn.present[k][1] = s + 1 if strategy == "LFU" else ((epoch << 32) | ((s & 0xffffffff) + 1))

  # warm-up: hits only (the count-1 residents are left alone)
  hits = np.array([r[j] for r in scn.res for j in hit_idx], np.int64)
  if hits.size:
    bump(hits)
    run(hits, np.zeros(0, np.int64), "warm-up")
  fresh = np.array([f[0] for f in scn.fresh], np.int64)
  for i in (0, 1):
    gone = scn.evict(i, [fresh[i]], [_word(strategy, epoch, 1)], [_word(strategy, epoch, 1)], 1)
    assert gone == [int(scn.res[i][9 + 7 * i])]
  bump(hits)
  run(hits, fresh, "one fresh key per pair")
  assert int(fresh[2]) not in scn.present and int(fresh[3]) not in scn.present


# ---- 8. the step drivers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["look_ahead", "overlapped_step"])
def test_step_drivers_evict_the_oldest(env, driver):
  """Six steps of a lookup + insert_or_assign stream on an LRU table (residents in six calls of five).  Every step carries, per pair,
  hits on one group and five never-resident or returning keys; from the second step on the returning keys are the victims of the
  step before — the write-back evicts what the next lookup asks for.  Every lookup equals a dictionary over the set that (write
  the hits, then each new key replaces the oldest) gives; after the flush the table holds exactly that set."""
  torch, de = env
  scn = Scene(env, "ev_steps_" + driver, "LRU", groups=(5,) * 6)
  ratio = 0.5 if driver == "look_ahead" else 0.0
  assert de.assign_step_driver_for(ratio) == driver
  drv = de.assign_step_for(scn.t, ratio)
  ages = Ages(scn)
  G = lambda i, g: scn.res[i][5 * g:5 * g + 5]
  N0 = [scn.fresh[i][:5] for i in range(N_PAIRS)]
  plan = [(0, N0), (3, 1), (5, 2), (0, 4), (3, N0), (2, 1)]        # (group hit, group or keys that come (back) in)
  batches = []
  for hit, new in plan:
    b = np.concatenate([np.concatenate([G(i, hit), new[i] if isinstance(new, list) else G(i, new)]) for i in range(N_PAIRS)])
    np.random.default_rng(len(batches)).shuffle(b)
    batches.append(b)
  bt = [_kt(torch, b) for b in batches]
  vt = [_vt(torch, scn.rows(b, 10 + s)) for s, b in enumerate(batches)]
  default = scn.tbl._default_value.cpu().numpy()
  drv.prime(bt[0])
  expected_victims = [1, 2, 4, None, 1, 5]
  for s, b in enumerate(batches):
    out, ex = drv.step(vt[s], bt[s + 1] if s < 5 else None, bt[s + 2] if s < 4 else None, return_exists=True)
    wex = np.array([int(k) in scn.present for k in b])
    want = np.stack([scn.present[int(k)][0] if int(k) in scn.present else default for k in b])
    np.testing.assert_array_equal(ex.cpu().numpy(), wex, err_msg="step %d" % s)
    np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg="step %d" % s)
    hits = b[wex]
    assert hits.size == 5 * N_PAIRS
    gone = ages.call(hits, b[~wex], 10 + s)
    v = expected_victims[s]
    wantgone = np.concatenate([N0[i] if v is None else G(i, v) for i in range(N_PAIRS)])
    assert sorted(gone) == sorted(wantgone.tolist()), s
  drv.flush()
  torch.cuda.synchronize()
  scn.check("after the steps")
  if driver == "overlapped_step":
    st = drv.stats()
    assert st["overlapped"] >= 5 and st["deferred_evictions"] > 0, ("the overlapped launch or its deferred evictions did not run", st)


# ---- 9. more fresh keys than the pair has slots --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", EVICTING, ids=_pid)
def test_more_fresh_keys_than_slots(env, path):
  """45 fresh keys of one pair in one call on an LRU table (two pairs at once): every resident of the pair is older than every fresh
  key, so the pair ends up holding 30 keys, all of them fresh — which 30 is a race and is not asserted.  Each present key carries its
  own row, no slot stays LOCKED, the size is unchanged, no key is reported unplaced."""
  torch = env[0]
  name, tags = path
  scn = Scene(env, "ev_45_%s_%d" % (name, tags), "LRU", dt=PATHS[name][1])
  crowded = (0, 2)
  keys = np.concatenate([scn.fresh[i] for i in crowded])
  assert keys.size == 90
  _assign(scn, name, keys, 2, None, tags)
  scn.tbl.check_errors()
  k, v, _ = _sorted_export(torch, scn.tbl, with_scores=True)
  kn, vn = k.cpu().numpy(), v.cpu().numpy()
  for i in crowded:
    m = np.isin(kn, scn.keys[i])
    assert int(m.sum()) == 30 and np.isin(kn[m], scn.fresh[i]).all(), (i, int(m.sum()), int(np.isin(kn[m], scn.res[i]).sum()))
    for r in scn.res[i].tolist():
      del scn.present[r]
    for x, row in zip(kn[m].tolist(), vn[m]):
      scn.present[x] = [scn.rows([x], 2)[0], None]
  scn.check("45 keys for 30 slots")
