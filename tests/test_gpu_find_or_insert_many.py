"""GPU: the grouped admitting lookup of plain tables (tfra_multi_find_or_insert; table_ops.find_or_insert_many /
table_admit_many) — per descriptor it IS tfra_table_find_or_insert.

Every member of a list is a table `a` that is served by the grouped call and a TWIN `b`, built by the same calls, that is served by
the single call on buffers of the same alignment.  Compared per member, bit for bit: values_out and found (whole buffers, the
sentinel beyond the count included), the export sorted by key (rows, scores where the table has them and they are no device clock,
every slot field), size_host, and check_errors clean on both.

At max_capacity the tables are the eviction scene of tests/test_gpu_eviction.py (CUSTOMIZED, four full bucket pairs whose residents
carry distinct scores).  The never-seen keys of a batch score above every resident and NO TWO OF THEM SHARE A HOME BUCKET (checked on
the CPU with tests/probe_model.homes; picked by rejection): then every never-seen key has its victim — the minimum of its own two
buckets — to itself, the victim set does not depend on the order of the blocks, and the twin comparison by key is exact."""
import ctypes

import numpy as np
import pytest

from tests import probe_model as pm
from tests.test_gpu_eviction import N_PAIRS, Scene, _distinct_scores
from tests.test_gpu_find_or_insert import _rows
from tests.test_gpu_probe_chains import Scn, _a_locked, _build, _kt, _nb, _table

pytestmark = pytest.mark.gpu

SENT = 0x5A
AUX_INIT = (0.5, 0.25, 0.0, 0.0)
CAP = 15 * 89
CUSTOMIZED, EPOCHLFU = 4, 3


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


_count = [0]


def _mk(torch, dt, dim, aux=0, strategy=-1, max_capacity=0, init_capacity=8192, step_per_epoch=0):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  _count[0] += 1
  tdt = getattr(torch, dt)
  return _DeviceTable(torch.int64, tdt, torch.full((dim,), 3, dtype=tdt), "foim%d" % _count[0], "cuda:0", dim=dim, aux_fields=aux,
                      init_capacity=init_capacity, max_capacity=max_capacity, strategy=strategy, step_per_epoch=step_per_epoch,
                      aux_init=AUX_INIT)


def _row_t(torch, keys, ver, dt, dim):
  """[n, dim] rows on the device in the table's dtype, a closed-form function of (key, version); bfloat16 by rounding float32"""
  if dt == "bfloat16":
    return torch.from_numpy(_rows(keys, ver, "float32", dim)).cuda().to(torch.bfloat16)
  return torch.from_numpy(_rows(keys, ver, dt, dim)).cuda()


def _at(torch, data, off):
  """a uint8 device buffer holding `data`'s bytes that starts `off` bytes behind an aligned address"""
  flat = data.contiguous().reshape(-1).view(torch.uint8)
  base = torch.empty(flat.numel() + 64, dtype=torch.uint8, device="cuda")
  view = base[off:off + flat.numel()]
  view.copy_(flat)
  assert view.data_ptr() % 16 == off % 16
  return view


class Member:
  """A table and its twin with one call's operands: `a` goes into the grouped call, `b` into the single one."""

  def __init__(self, torch, a, b, dt, dim, aux=0, off=0, scored=False):
    self.torch, self.a, self.b, self.dt, self.dim, self.aux, self.off, self.scored = torch, a, b, dt, dim, aux, off, scored
    self.row_bytes = dim * torch.empty(0, dtype=getattr(torch, dt)).element_size()

  def seed(self, keys, slotted=0):
    torch = self.torch
    for t in (self.a, self.b):
      t.upsert(_kt(torch, keys), _row_t(torch, keys, 1, self.dt, self.dim))
      for f in range(1, self.aux + 1):
        t.upsert(_kt(torch, keys[:slotted]), _row_t(torch, keys[:slotted], 10 + f, self.dt, self.dim), field=f)

  def call(self, keys, ver, full=True, count=None, scores=None, want_out=True, want_found=True):
    """sets up the buffers of one call for both sides; n = keys.size"""
    torch = self.torch
    self.keys, self.n = _kt(torch, keys), keys.size
    self.full = full
    init = _row_t(torch, keys if full else np.array([77], np.int64), ver, self.dt, self.dim)
    self.init = _at(torch, init, self.off)
    self.count = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    self.scores = None if scores is None else _kt(torch, np.asarray(scores, np.int64))
    sent = torch.full((self.n * self.row_bytes,), SENT, dtype=torch.uint8, device="cuda")
    self.out = [_at(torch, sent, self.off) if want_out else None for _ in range(2)]
    self.found = [torch.full((self.n,), SENT, dtype=torch.uint8, device="cuda") if want_found else None for _ in range(2)]
    return self

  def desc(self, side=0, table=None, **over):
    from tfra_amd import _capi
    p = lambda x: None if x is None else x.data_ptr()
    d = _capi.FindOrInsertDesc()
    d.struct_size = ctypes.sizeof(_capi.FindOrInsertDesc)
    d.flags, d.table, d.n, d.d_n, d.keys = 0, (table or (self.a, self.b)[side])._h.value, self.n, p(self.count), p(self.keys)
    d.init_values, d.init_is_full, d.reserved, d.scores = p(self.init), int(self.full), 0, p(self.scores)
    d.values_out, d.found = p(self.out[side]), p(self.found[side])
    for k, v in over.items():
      setattr(d, k, v)
    return d

  def single(self):
    """tfra_table_find_or_insert on the twin, buffers of side 1"""
    from tfra_amd import _capi
    from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
    _capi.call("tfra_table_find_or_insert", self.b._h, self.n, _ptr(self.count), _ptr(self.keys), _ptr(self.init), int(self.full),
               _ptr(self.scores), _ptr(self.out[1]), _ptr(self.found[1]), _stream(self.b.device))

  def snap(self, t):
    """the table sorted by key: keys, row bytes, scores (tables with caller scores), every slot field"""
    torch = self.torch
    k, v, s = t.export_all(with_scores=self.scored)
    o = torch.argsort(k)
    k = k[o]
    return [k, v[o].contiguous().view(torch.uint8)] + ([s[o]] if self.scored else []) + [
        t.find(k, field=f).contiguous().view(torch.uint8) for f in range(1, self.aux + 1)]

  def compare(self, tag):
    torch = self.torch
    for name, (x, y) in (("values_out", self.out), ("found", self.found)):
      assert (x is None) == (y is None)
      if x is not None:
        assert torch.equal(x, y), "%s: %s differs from the single call's" % (tag, name)
    for i, (x, y) in enumerate(zip(self.snap(self.a), self.snap(self.b))):
      assert x.shape == y.shape and torch.equal(x, y), "%s: the tables differ (part %d of keys, rows, scores, slot fields)" % (tag, i)
    self.a.check_errors()
    self.b.check_errors()
    assert self.a.size_host() == self.b.size_host(), tag


def _grouped(torch, descs, expect_launches=None):
  """tfra_multi_find_or_insert itself -> launches"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import table_ops as T
  arr = (_capi.FindOrInsertDesc * len(descs))(*descs)
  launches = ctypes.c_uint32(77)
  dev = torch.device("cuda:0")
  try:
    _capi.call("tfra_multi_find_or_insert", T._workspace(dev), len(descs), ctypes.c_void_p(ctypes.addressof(arr)),
               ctypes.c_void_p(ctypes.addressof(launches)), T._stream(dev))
  finally:
    torch.cuda.synchronize()
    if expect_launches is not None:
      assert launches.value == expect_launches, launches.value
  return launches.value


def _pool(seed, n):
  rng = np.random.default_rng(seed)
  keys = np.unique(rng.integers(-2**62, 2**62, size=n + 50, dtype=np.int64))
  rng.shuffle(keys)
  return keys[:n]


# ---- the eviction scene as a member ------------------------------------------------------------------------------------------------
def _scene_member(env, tag):
  torch = env[0]
  sa, sb = (Scene(env, "foim_%s_%s" % (tag, x), "CUSTOMIZED", score=_distinct_scores(1)) for x in "ab")
  m = Member(torch, sa.tbl, sb.tbl, "float32", 8, scored=True)
  m.scene = sa
  return m


def _scene_batch(scn, call, n_open=8):
  """-> keys, scores, never-seen keys.  One fresh key per full pair (it must evict: the pair's minimum goes), the two highest-scoring
  residents of every pair (hits: never a victim) and n_open never-seen keys homed outside the pairs, where every bucket has room.
  The never-seen keys are taken by rejection so that no two share a home bucket; all score above every resident."""
  nb = scn.nb
  sc = _distinct_scores(1)
  hits = np.array([scn.res[i][r] for i in range(N_PAIRS) for r in sorted(range(30), key=lambda r: sc(i, r))[-2:]], np.int64)
  shut = {b for b0, b1 in scn.pairs for b in (b0, b1, (b1 + 1) % nb, (b1 + 2) % nb)}
  fresh, taken = [], set()
  cand = np.concatenate([[scn.fresh[i][call] for i in range(N_PAIRS)], _pool(1000 + call, 4000)])
  h0, h1, _ = pm.homes(cand, nb)
  for j, k in enumerate(cand.tolist()):
    own = {int(h0[j]), int(h1[j])}
    if own & taken or (j >= N_PAIRS and own & shut) or k in scn.by:
      continue
    fresh.append(k)
    taken |= own
    if len(fresh) == N_PAIRS + n_open:
      break
  fresh = np.array(fresh, np.int64)
  assert fresh.size == N_PAIRS + n_open and set(fresh[:N_PAIRS].tolist()) == {int(scn.fresh[i][call]) for i in range(N_PAIRS)}
  f0, f1, _ = pm.homes(fresh, nb)                        # the condition of the module docstring, on the CPU
  assert np.unique(np.concatenate([f0, f1])).size == 2 * fresh.size, "two never-seen keys share a home bucket"
  keys = np.concatenate([fresh, hits])
  scores = np.concatenate([5000 * (call + 1) + np.arange(fresh.size), 5000 * (call + 1) + 1000 + np.arange(hits.size)])
  o = np.random.default_rng(call).permutation(keys.size)
  return keys[o], scores[o], fresh


# ---- 1. a heterogeneous list -------------------------------------------------------------------------------------------------------
def test_a_heterogeneous_list(env):
  """Three grouped calls over 11 members: float32 / float16 / bfloat16 / int8; dims 4, 8, 64, 130 and 3 (granules 16, 8, 2, 1, and 4
  by buffers that start 4 bytes off); growing tables (one seeded with 8000 keys at init_capacity 8192: it grows under the calls, at the third one's hard bound at the latest), bounded tables below capacity (CUSTOMIZED
  with caller scores; EPOCHLFU with step_per_epoch 1, whose new scores carry the epoch: it steps once per table and call) and three
  at max_capacity (full init rows; ONE init row with values_out: phase 2 reads the rows phase 1 left there; ONE init row with
  neither output: the spill rows); d_n NULL, given, and larger than n; values_out and / or found NULL."""
  torch, _ = env
  twins = lambda *a, **kw: (_mk(torch, *a, **kw), _mk(torch, *a, **kw))
  M = [
      Member(torch, *twins("float32", 4), "float32", 4),                                        # 0  granule 16
      Member(torch, *twins("float16", 4), "float16", 4),                                        # 1  granule 8; d_n < n, one init row
      Member(torch, *twins("bfloat16", 64, aux=2), "bfloat16", 64, aux=2),                      # 2  d_n > n; found NULL; slot fields
      Member(torch, *twins("int8", 130), "int8", 130),                                          # 3  granule 2; values_out NULL
      Member(torch, *twins("int8", 3), "int8", 3),                                              # 4  granule 1; one init row
      Member(torch, *twins("float32", 64), "float32", 64, off=4),                               # 5  granule 4 by the buffers' offset
      Member(torch, *twins("float32", 8, strategy=CUSTOMIZED, max_capacity=64 * CAP, init_capacity=CAP), "float32", 8, scored=True),   # 6
      Member(torch, *twins("float32", 8, aux=1, strategy=EPOCHLFU, max_capacity=64 * CAP, init_capacity=CAP, step_per_epoch=1),
             "float32", 8, aux=1, scored=True),                                                 # 7
      _scene_member(env, "full"),                                                               # 8  at max_capacity, full init rows
      _scene_member(env, "out"),                                                                # 9  one init row, values_out given
      _scene_member(env, "spill"),                                                              # 10 one init row, no outputs
  ]
  pools = [_pool(10 + i, 11200 if i == 0 else 9000) for i in range(8)]
  for i, m in enumerate(M[:8]):
    m.seed(pools[i][:8000 if i == 0 else 400], slotted=100)        # (member 0: 8000 keys at init_capacity 8192 — it grows under the calls)
  size0 = [m.a.size_host() for m in M]
  for call in range(3):
    descs = []
    for i, m in enumerate(M):
      if i < 8:
        n = (1000, 257, 64, 130, 33, 100, 200, 150)[i]
        new = pools[i][8000 + call * n:8000 + call * n + n - n // 3]
        keys = np.concatenate([pools[i][:8000 if i == 0 else 400][call * 50:call * 50 + n // 3], new])          # a third of the keys are resident
        np.random.default_rng(100 * call + i).shuffle(keys)
        scores = 100 + np.arange(keys.size) + 1000 * call if i in (6, 7) else None
        m.call(keys, 2 + call, full=i not in (1, 4), count={1: 200, 2: 5000}.get(i), scores=scores, want_out=i != 3, want_found=i != 2)
      else:
        keys, scores, fresh = _scene_batch(m.scene, call)
        m.fresh = fresh
        m.call(keys, 2 + call, full=i == 8, scores=scores, want_out=i != 10, want_found=i == 8)
      descs.append(m.desc())
    # one launch per granule class of the list (16, 8, 4, 2, 1), and one phase 2 for the three full members (all of class 16)
    assert _grouped(torch, descs) == 6
    for i, m in enumerate(M):
      m.single()
    torch.cuda.synchronize()
    for i, m in enumerate(M):
      m.compare("call %d member %d" % (call, i))
    assert bool((M[1].out[0][200 * M[1].row_bytes:] == SENT).all()) and bool((M[1].found[0][200:] == SENT).all()), "written beyond d_n"
    for m in M[8:]:      # every never-seen key got in: four of them by evicting (the size grew by the other eight only)
      assert bool(m.a.contains(_kt(torch, m.fresh)).all())
      assert m.a.size_host() == m.scene.n_live + 8 * (call + 1)
  assert M[0].a.growth_stats()["growths"] >= 1, "no call grew member 0"
  assert all(m.a.size_host() > s for m, s in zip(M, size0))


# ---- 2. block and prefix edges -----------------------------------------------------------------------------------------------------
def test_block_and_prefix_edges(env):
  """n = 1, 15, 16, 17, 63, 64, 65 (16 keys per wave, 64 per block) in one list, with a member of n == 0 (skipped: its EPOCHLFU
  table's epoch does not step — the next key it admits scores as the twin's, which got no call) and one whose *d_n is 0 (served: nothing
  admitted, nothing written)."""
  torch, _ = env
  sizes = [1, 15, 16, 17, 63, 0, 64, 65, 40]
  M = []
  for j, n in enumerate(sizes):
    epoch = dict(strategy=EPOCHLFU, max_capacity=64 * CAP, init_capacity=CAP, step_per_epoch=1) if n == 0 else {}
    m = Member(torch, _mk(torch, "float32", 8, **epoch), _mk(torch, "float32", 8, **epoch), "float32", 8, scored=n == 0)
    pool = _pool(200 + j, 200)
    m.seed(pool[:64])
    keys = np.concatenate([pool[:n // 2], pool[64:64 + n - n // 2]])
    m.call(keys, 2, count=0 if j == 8 else None)
    M.append(m)
  launches = _grouped(torch, [m.desc() for m in M])
  assert launches == 1
  for j, m in enumerate(M):
    if sizes[j]:
      m.single()
    torch.cuda.synchronize()
    m.compare("member %d (n = %d)" % (j, sizes[j]))
  assert M[8].a.size_host() == 64 and bool((M[8].out[0] == SENT).all()) and bool((M[8].found[0] == SENT).all())
  # the skipped member: one key into both tables now; its score carries the epoch
  probe = np.array([123456789], np.int64)
  M[5].call(probe, 3)
  assert _grouped(torch, [M[5].desc()]) == 1
  M[5].single()
  torch.cuda.synchronize()
  M[5].compare("the skipped member's epoch")
  # through the Python call: the requests' order, (rows, exists) or None
  from tfra_amd.dynamic_embedding import table_ops as T
  reqs = [(m.a, m.keys, _row_t(torch, m.keys.cpu().numpy(), 2, "float32", 8)) for m in M[:3]]
  outs = T.find_or_insert_many(reqs[:2] + [reqs[2] + (None, False)])
  assert outs[2] is None and all(bool(o[1].all()) for o in outs[:2])          # (every key is resident by now)
  for (t, k, _), o in zip(reqs[:2], outs[:2]):
    assert torch.equal(o[0], t.find(k))


# ---- 3. the launch count -----------------------------------------------------------------------------------------------------------
def test_a_long_list_takes_the_launches_of_a_short_one(env):
  torch, _ = env
  from tfra_amd.dynamic_embedding import table_ops as T
  tables = [_mk(torch, "float32", 4) for _ in range(26)]
  twins = [_mk(torch, "float32", 4) for _ in range(26)]
  full = [_scene_member(env, "count%d" % j) for j in range(2)]
  got = {}
  for call, n_t in enumerate((26, 2)):
    reqs = []
    for j in range(n_t):
      keys = _pool(300 + 100 * call + j, 40 + j)
      reqs.append((tables[j], _kt(torch, keys), _row_t(torch, keys, 2, "float32", 4)))
    outs, got[n_t] = T.find_or_insert_many(reqs, return_launches=True)
    for (_, k, init), twin, out in zip(reqs, twins, outs):
      rows, ex = twin.find_or_insert(k, init, return_exists=True)
      assert torch.equal(out[0], rows) and torch.equal(out[1], ex)
    # with two full bounded members in the list: their phase 2 is ONE more launch
    more = []
    for m in full:
      keys, scores, _ = _scene_batch(m.scene, call)
      more.append((m.a, _kt(torch, keys), _row_t(torch, keys, 2, "float32", 8), None, True, _kt(torch, scores)))
    _, got[n_t, "full"] = T.find_or_insert_many(reqs + more, return_launches=True)
  assert got == {26: 1, 2: 1, (26, "full"): 2, (2, "full"): 2}, got
  for t in tables:
    t.check_errors()


# ---- 4. overflow chains ------------------------------------------------------------------------------------------------------------
def test_a_member_on_an_overflow_chain(env):
  """The chain of tests/test_gpu_probe_chains.py (11 buckets deep, holes in its buckets 0 and 2) as one member of a list of three:
  the keys at the chain's end and bystanders are hits, 28 new keys of the pair fill the holes.  Against the twin served by the single
  call; the flags do not move."""
  torch, _ = env
  sides = []
  for x in "ab":
    tbl = _table(env, "foim_chain_" + x)
    scn = Scn(_nb(tbl), "mid")
    ref, model = {}, pm.FirstFit(scn.nb)
    _build(env, tbl, scn, _a_locked, "float32", ref, model, None, exact=True)
    tbl.erase(_kt(torch, np.concatenate([scn.chain[0:15], scn.chain[30:45]])))
    sides.append(tbl)
  m = Member(torch, sides[0], sides[1], "float32", 8)
  flags = [t.slot_census() for t in sides]
  deep = np.concatenate([scn.chain[75:90], scn.chain[150:160]])
  new = np.concatenate([scn.extra, scn.absent[:8]])
  keys = np.concatenate([deep, scn.by[:40], new])
  np.random.default_rng(5).shuffle(keys)
  m.call(keys, 2)
  others = []
  for j in range(2):
    o = Member(torch, _mk(torch, "float32", 8), _mk(torch, "float32", 8), "float32", 8)
    others.append(o.call(_pool(400 + j, 70), 2))
  assert _grouped(torch, [others[0].desc(), m.desc(), others[1].desc()]) == 1
  for x in [m] + others:
    x.single()
  torch.cuda.synchronize()
  for x in [m] + others:
    x.compare("chain")
  np.testing.assert_array_equal(m.found[0].cpu().numpy().astype(bool), ~np.isin(keys, new))
  for t, f in zip(sides, flags):
    c = t.slot_census()
    assert c["locked"] == 0 and c["live"] == f["live"] + new.size and (c["ovf0"], c["ovf1"]) == (f["ovf0"], f["ovf1"]) and c["ovf1"] > 0


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _refusal_members(torch):
  """two members; the second is an EPOCHLFU table (step_per_epoch 1) whose epoch a later admission shows"""
  M = [Member(torch, _mk(torch, "float32", 8), _mk(torch, "float32", 8), "float32", 8),
       Member(torch, *(_mk(torch, "float32", 8, strategy=EPOCHLFU, max_capacity=64 * CAP, init_capacity=CAP, step_per_epoch=1) for _ in "ab"),
              "float32", 8, scored=True)]
  for j, m in enumerate(M):
    pool = _pool(500 + j, 400)
    m.seed(pool[:200])
    m.call(np.concatenate([pool[:50], pool[200:300]]), 2)
  return M


def _refused(torch, M, name, descs, text):
  from tfra_amd import _capi
  before = [m.snap(m.a) for m in M]
  with pytest.raises(_capi.TfraError) as e:
    _grouped(torch, descs, expect_launches=0)
  assert e.value.code == -1, name
  assert "multi_find_or_insert: " + text in str(e.value), (name, str(e.value))
  for m, b in zip(M, before):
    for x, y in zip(b, m.snap(m.a)):
      assert torch.equal(x, y), "%s: a refused list changed a table" % name
    assert bool((m.out[0] == SENT).all()) and bool((m.found[0] == SENT).all()), "%s: a refused list wrote an output" % name


def test_refusals_leave_everything_as_it_was(env):
  torch, _ = env
  M = _refusal_members(torch)
  a, e = M
  _refused(torch, M, "the same table twice", [a.desc(), e.desc(), e.desc(table=a.a)], "descriptor 2: the same table as descriptor 0")
  _refused(torch, M, "NULL keys", [a.desc(), e.desc(keys=None)], "descriptor 1: null buffer")
  _refused(torch, M, "NULL init_values", [a.desc(init_values=None), e.desc()], "descriptor 0: null buffer")
  _refused(torch, M, "a wrong struct_size", [a.desc(), e.desc(struct_size=72)], "descriptor 1: descriptor size mismatch")
  _refused(torch, M, "a non-zero reserved", [a.desc(), e.desc(reserved=1)], "descriptor 1: reserved must be 0")
  _refused(torch, M, "non-zero flags", [a.desc(), e.desc(flags=1)], "descriptor 1: unknown flag bits")
  # the single call's wording behind the prefix
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  with pytest.raises(_capi.TfraError) as err:
    _capi.call("tfra_table_find_or_insert", a.a._h, a.n, None, None, _ptr(a.init), 1, None, None, None, _stream(a.a.device))
  assert "tfra_table_find_or_insert: null buffer" in str(err.value) and err.value.code == -1
  # the epochs did not move: the sound list now, the single calls on the twins (which saw no refused call) — the EPOCHLFU scores agree
  assert _grouped(torch, [a.desc(), e.desc()]) == 1
  for m in M:
    m.single()
  torch.cuda.synchronize()
  for j, m in enumerate(M):
    m.compare("served after the refusals, member %d" % j)


def test_a_workspace_of_another_device_is_refused(env):
  torch, _ = env
  if torch.cuda.device_count() < 2:
    pytest.skip("needs two devices")
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import table_ops as T
  M = _refusal_members(torch)
  before = [m.snap(m.a) for m in M]
  arr = (_capi.FindOrInsertDesc * 2)(*[m.desc() for m in M])
  launches = ctypes.c_uint32(77)
  with pytest.raises(_capi.TfraError) as e:
    _capi.call("tfra_multi_find_or_insert", T._workspace(torch.device("cuda:1")), 2, ctypes.c_void_p(ctypes.addressof(arr)),
               ctypes.c_void_p(ctypes.addressof(launches)), T._stream(torch.device("cuda:0")))
  torch.cuda.synchronize()
  assert e.value.code == -1 and "descriptor 0: workspace and table live on different devices" in str(e.value) and launches.value == 0
  for m, b in zip(M, before):
    for x, y in zip(b, m.snap(m.a)):
      assert torch.equal(x, y)
    assert bool((m.out[0] == SENT).all()) and bool((m.found[0] == SENT).all())
