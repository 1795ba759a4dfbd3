"""GPU: tfra_table_find_missed — find that also lists its misses — and the d_n forms of tfra_table_assign / tfra_table_contains.

The reference for rows and exists is tfra_table_find on the same arguments, compared byte for byte; the reference for the miss list is
a Python set of the keys that were inserted: the list, as a multiset of (key, position), is {(keys[i], i): keys[i] not resident}.
Every output buffer is handed in pre-filled and longer than needed, so a write that should not happen shows."""
import numpy as np
import pytest

from tests.test_gpu_eviction import Scene
from tests.test_gpu_probe_chains import _kt, _read_fixture, _sorted_export

pytestmark = pytest.mark.gpu

TILES = (2, 4, 8)               # 64-key tiles per block of find_missed_kernel: the kept TIER_TILES (csrc/tfra_tier.hip) and its neighbours
NS = [1, 15, 16, 17, 63, 64, 65, 257, 1000, 4099] + [64 * t + d for t in TILES for d in (-1, 0, 1) if 64 * t + d != 257]
GRID = [("float32", 1), ("float32", 3), ("float32", 4), ("float32", 64), ("float32", 130), ("float16", 3), ("float16", 128),
        ("bfloat16", 8), ("int8", 5), ("int32", 2), ("int64", 1)]
N_RES, N_ABS = 1500, 1500
GUARD = 16
EMPTY, LOCKED = -2**63, -2**63 + 1


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _universe(seed=5):
  rng = np.random.default_rng(seed)
  u = np.unique(rng.integers(-2**62, 2**62, size=N_RES + N_ABS + 64, dtype=np.int64))
  rng.shuffle(u)
  return u[:N_RES], u[N_RES:N_RES + N_ABS]


RES, ABS = _universe()
RESIDENT = set(RES.tolist())


def _rows(torch, keys, dt, dim, ver=1):
  k = torch.as_tensor(np.asarray(keys, np.int64)).cuda()
  x = (k[:, None] * 31 + torch.arange(dim, device="cuda")[None, :] * 7 + ver * 13) % 97 - 48
  return x.to(getattr(torch, dt)).contiguous()


def make_table(torch, dt, dim, name, resident=RES, **kw):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  tdt = getattr(torch, dt)
  default = torch.full((dim,), 7 if not tdt.is_floating_point else 0.125, dtype=tdt)
  tbl = _DeviceTable(torch.int64, tdt, default, name, "cuda:0", dim=dim, init_capacity=2048, **kw)
  if len(resident):
    tbl.upsert(_kt(torch, resident), _rows(torch, resident, dt, dim), unique_keys=True)
  return tbl


_TABLES = {}


def shared_table(torch, dt="float32", dim=4):
  """one table per (dtype, dim) holding RES, shared by the tests that only read"""
  if (dt, dim) not in _TABLES:
    _TABLES[(dt, dim)] = make_table(torch, dt, dim, "fm_%s_%d" % (dt, dim))
  return _TABLES[(dt, dim)]


def fm(torch, tbl, kt, values=True, exists=True, scores=False, defaults=None, counter=0, cap=None, want_keys=True, want_idx=True,
       count=None, expect_rc=0):
  """one raw tfra_table_find_missed with pre-filled buffers -> dict of numpy arrays (rows and exists as bytes) and the counter"""
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  n = kt.numel()
  cap = n if cap is None else cap
  fb = tbl.dim * tbl._default_value.element_size()
  b = dict(rows=torch.full((n, fb), 0xA5, dtype=torch.uint8, device="cuda") if values else None,
           exists=torch.full((n,), 7, dtype=torch.uint8, device="cuda") if exists else None,
           scores=torch.full((n,), -77, dtype=torch.int64, device="cuda") if scores else None,
           mk=torch.full((max(cap, n) + GUARD,), -555, dtype=torch.int64, device="cuda") if want_keys else None,
           mi=torch.full((max(cap, n) + GUARD,), -333, dtype=torch.int32, device="cuda") if want_idx else None,
           counter=None if counter is None else torch.tensor([counter], dtype=torch.int64, device="cuda"))
  d = tbl._default_value if defaults is None else defaults
  full = int(d.numel() == n * tbl.dim)
  cnt = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
  rc = _capi.lib().tfra_table_find_missed(tbl._h, n, _ptr(cnt), _ptr(kt), _ptr(b["rows"]), _ptr(b["exists"]), _ptr(b["scores"]),
                                          _ptr(d.contiguous()) if values else None, full, _ptr(b["counter"]), cap, _ptr(b["mk"]), _ptr(b["mi"]),
                                          _stream(tbl.device))
  assert rc == expect_rc, (rc, _capi.lib().tfra_last_error())
  torch.cuda.synchronize()
  out = {k: (None if v is None else v.cpu().numpy()) for k, v in b.items()}
  out["n_missed"] = None if counter is None else int(out["counter"][0]) - counter
  return out


def check_pairs(keys, resident, r, served=None, start=0):
  """counter = number of missed positions; the written pairs = the whole multiset (cap permitting), index-aligned; guard intact"""
  served = keys.size if served is None else served
  want = sorted((int(k), i) for i, k in enumerate(keys[:served].tolist()) if k not in resident)
  assert r["n_missed"] == len(want)
  mk, mi = r["mk"], r["mi"]
  end = start + len(want)
  if mk is not None and mi is not None:
    assert sorted(zip(mk[start:end].tolist(), mi[start:end].tolist())) == want
    np.testing.assert_array_equal(mk[start:end], keys[mi[start:end]])
  elif mk is not None:
    assert sorted(mk[start:end].tolist()) == sorted(k for k, _ in want)
  elif mi is not None:
    assert sorted(mi[start:end].tolist()) == sorted(i for _, i in want)
  if mk is not None:
    assert (mk[:start] == -555).all() and (mk[end:] == -555).all()
  if mi is not None:
    assert (mi[:start] == -333).all() and (mi[end:] == -333).all()


def mixed_keys(n, seed):
  """n keys with repeats, about half of them resident"""
  rng = np.random.default_rng(seed)
  pool = np.concatenate([RES[:max(1, min(N_RES, n // 3 + 1))], ABS[:max(1, min(N_ABS, n // 3 + 1))]])
  return pool[rng.integers(0, pool.size, size=n)]


# ---- 1. parity with find -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,dim", GRID, ids=["%s-%d" % g for g in GRID])
def test_parity_with_find(env, dt, dim):
  torch, _ = env
  tbl = shared_table(torch, dt, dim)
  for n in NS:
    keys = mixed_keys(n, n)
    kt = _kt(torch, keys)
    for full in (False, True):
      d = _rows(torch, np.arange(n), dt, dim, ver=9) if full else None
      rows, ex = tbl.find(kt, dynamic_default_values=d, return_exists=True)
      r = fm(torch, tbl, kt, defaults=d)
      np.testing.assert_array_equal(r["rows"], rows.contiguous().view(torch.uint8).reshape(n, -1).cpu().numpy(), err_msg="n=%d full=%d" % (n, full))
      np.testing.assert_array_equal(r["exists"], ex.view(torch.uint8).cpu().numpy())
      np.testing.assert_array_equal(r["exists"] != 0, np.array([k in RESIDENT for k in keys.tolist()]))
      check_pairs(keys, RESIDENT, r)


# ---- 2. miss patterns, one block's worth and many blocks ---------------------------------------------------------------------------
PATTERNS = {
    "none": lambda i, n: np.zeros(n, bool), "all": lambda i, n: np.ones(n, bool), "first": lambda i, n: i == 0, "last": lambda i, n: i == n - 1,
    "one_per_wave": lambda i, n: i % 16 == (i // 16) % 16, "one_per_tile": lambda i, n: i % 64 == (i // 64) % 64, "every_third": lambda i, n: i % 3 == 0,
}


@pytest.mark.parametrize("n", [4099, 70001])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_miss_patterns(env, pattern, n):
  torch, _ = env
  tbl = shared_table(torch)
  i = np.arange(n)
  miss = PATTERNS[pattern](i, n)
  keys = np.where(miss, ABS[i % N_ABS], RES[i % N_RES])
  r = fm(torch, tbl, _kt(torch, keys), scores=True)
  assert r["n_missed"] == int(miss.sum())
  check_pairs(keys, RESIDENT, r)
  np.testing.assert_array_equal(r["exists"] != 0, ~miss)
  if pattern == "none":
    assert r["counter"][0] == 0 and (r["mk"] == -555).all() and (r["mi"] == -333).all()


# ---- 3. cap ------------------------------------------------------------------------------------------------------------------------
def test_cap(env):
  torch, _ = env
  tbl = shared_table(torch)
  n = 1000
  i = np.arange(n)
  keys = np.where(i % 3 == 0, ABS[i], RES[i])
  misses = int((i % 3 == 0).sum())
  true_pairs = {(int(keys[j]), int(j)) for j in i if j % 3 == 0}
  for cap in (0, 1, misses - 1, misses, n):
    r = fm(torch, tbl, _kt(torch, keys), cap=cap)
    assert r["n_missed"] == misses                  # the counter is always the full miss count
    w = min(cap, misses)
    got = list(zip(r["mk"][:w].tolist(), r["mi"][:w].tolist()))
    assert len(set(got)) == w and set(got) <= true_pairs, cap
    assert (r["mk"][w:] == -555).all() and (r["mi"][w:] == -333).all(), cap      # nothing at or beyond cap; the guard is intact


# ---- 4. NULL outputs, counter start ------------------------------------------------------------------------------------------------
def test_null_outputs(env):
  torch, _ = env
  from tfra_amd import _capi
  tbl = shared_table(torch)
  keys = mixed_keys(1000, 3)
  kt = _kt(torch, keys)
  rows, ex = tbl.find(kt, return_exists=True)
  want_rows = rows.view(torch.uint8).reshape(1000, -1).cpu().numpy()
  for wk, wi in ((False, True), (True, False), (False, False)):
    r = fm(torch, tbl, kt, want_keys=wk, want_idx=wi)
    check_pairs(keys, RESIDENT, r)
    np.testing.assert_array_equal(r["rows"], want_rows)
  r = fm(torch, tbl, kt, values=False, exists=False)                       # the miss list alone
  check_pairs(keys, RESIDENT, r)
  r = fm(torch, tbl, kt, counter=None, want_keys=False, want_idx=False, scores=True)   # find plus scores
  np.testing.assert_array_equal(r["rows"], want_rows)
  np.testing.assert_array_equal(r["exists"], ex.view(torch.uint8).cpu().numpy())
  for wk, wi in ((True, False), (False, True)):                           # a list without its counter
    fm(torch, tbl, kt, counter=None, want_keys=wk, want_idx=wi, expect_rc=-1)
    assert "tfra_table_find_missed" in _capi.lib().tfra_last_error().decode()


def test_counter_continues_from_its_value(env):
  torch, _ = env
  keys = mixed_keys(257, 4)
  r = fm(torch, shared_table(torch), _kt(torch, keys), counter=5, cap=300)
  assert r["counter"][0] == 5 + r["n_missed"]
  check_pairs(keys, RESIDENT, r, start=5)


# ---- 5. the count on the device, all three calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 256, 257, 264, -3])
def test_count_on_the_device(env, count):
  torch, _ = env
  n = 257
  tbl = make_table(torch, "float32", 4, "fm_dn_%d" % (count + 3))
  keys = np.concatenate([RES[:130], ABS[:127]])
  np.random.default_rng(8).shuffle(keys)
  kt = _kt(torch, keys)
  served = max(0, min(n, count))
  rows, ex = tbl.find(kt, return_exists=True)
  r = fm(torch, tbl, kt, count=count, scores=True)
  np.testing.assert_array_equal(r["rows"][:served], rows.view(torch.uint8).reshape(n, -1).cpu().numpy()[:served])
  assert (r["rows"][served:] == 0xA5).all() and (r["exists"][served:] == 7).all() and (r["scores"][served:] == -77).all()
  np.testing.assert_array_equal(r["exists"][:served], ex.view(torch.uint8).cpu().numpy()[:served])
  check_pairs(keys, RESIDENT, r, served=served)
  cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
  c = tbl.contains(kt, count=cnt).cpu().numpy()
  np.testing.assert_array_equal(c[:served], ex.cpu().numpy()[:served])
  assert not c[served:].any()                                # (the binding hands in zeros)
  new = _rows(torch, keys, "float32", 4, ver=2)
  f = tbl.assign(kt, new, return_found=True, count=cnt).cpu().numpy()
  np.testing.assert_array_equal(f[:served], ex.cpu().numpy()[:served])
  assert not f[served:].any()
  after = tbl.find(kt)
  hit = ex.clone()
  hit[served:] = False
  assert torch.equal(after[hit], new[hit]) and torch.equal(after[~hit], rows[~hit])
  assert tbl.size_host() == N_RES


# ---- 6. scores_out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["LRU", "LFU", "EPOCHLFU", "CUSTOMIZED", "NONE"])
def test_scores_out(env, strategy):
  torch, de = env
  res = np.concatenate([RES[:600], [EMPTY]])
  if strategy == "NONE":
    tbl = make_table(torch, "float32", 8, "fm_sc_none", resident=res)
  else:
    t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(8), init_capacity=15 * 89, max_capacity=15 * 89, device="cuda:0", dim=8,
                        evict_strategy=de.HkvEvictStrategy[strategy], step_per_epoch=2, name="fm_sc_" + strategy)
    tbl = t._table
    for a in range(0, res.size, 200):                         # several calls: device clocks and epochs differ
      k = res[a:a + 200]
      tbl.upsert(_kt(torch, k), _rows(torch, k, "float32", 8), scores=_kt(torch, 100 + np.arange(a, a + k.size)), unique_keys=True)
  ek, _, es = tbl.export_all(with_scores=True)
  score = dict(zip(ek.cpu().numpy().tolist(), es.cpu().numpy().tolist()))
  assert len(score) == res.size and (strategy == "NONE" or len(set(score.values())) > 3)
  keys = np.concatenate([res, ABS[:300], res[:100], [LOCKED]])
  np.random.default_rng(2).shuffle(keys)
  before = _sorted_export(torch, tbl, with_scores=True)
  r = fm(torch, tbl, _kt(torch, keys), scores=True)
  np.testing.assert_array_equal(r["scores"], np.array([score.get(int(k), 0) for k in keys], np.int64))
  check_pairs(keys, set(res.tolist()), r)
  rows, mk, mi, ex, sc = tbl.find_missed(_kt(torch, keys), return_exists=True, return_scores=True)      # the binding's form
  np.testing.assert_array_equal(sc.cpu().numpy(), r["scores"])
  after = _sorted_export(torch, tbl, with_scores=True)       # not touched: an LRU clock in particular
  for x, y in zip(before, after):
    assert torch.equal(x, y)


# ---- 7. read-only ------------------------------------------------------------------------------------------------------------------
def test_find_missed_and_contains_write_nothing(env):
  torch, _ = env
  scn = Scene(env, "fm_readonly", "LRU")
  tbl = scn.tbl
  keys = np.concatenate([np.concatenate(scn.res), np.concatenate([f[:20] for f in scn.fresh]), scn.by[:100], [EMPTY, LOCKED]])
  before, census = scn.snap(), tbl.slot_census()
  fm(torch, tbl, _kt(torch, keys), scores=True)
  c = tbl.contains(_kt(torch, keys))
  np.testing.assert_array_equal(c.cpu().numpy(), tbl.find(_kt(torch, keys), return_exists=True)[1].cpu().numpy())
  scn.same(before, scn.snap(), "find_missed / contains wrote the table")
  assert tbl.slot_census() == census
  scn.check("after the readers")


# ---- 8. both sentinel keys through all three calls ---------------------------------------------------------------------------------
def test_sentinel_keys(env):
  torch, _ = env
  tbl = make_table(torch, "float32", 4, "fm_sentinels", resident=RES[:40])
  keys = np.array([EMPTY, RES[0], LOCKED, ABS[0]], np.int64)
  kt = _kt(torch, keys)
  r = fm(torch, tbl, kt)
  check_pairs(keys, set(RES[:40].tolist()), r)
  assert tbl.contains(kt).cpu().numpy().tolist() == [False, True, False, False]
  assert tbl.assign(kt, _rows(torch, keys, "float32", 4, 3), return_found=True).cpu().numpy().tolist() == [False, True, False, False]
  assert tbl.size_host() == 40
  tbl.upsert(kt[:3], _rows(torch, keys[:3], "float32", 4, 4), unique_keys=True)
  r = fm(torch, tbl, kt)
  check_pairs(keys, set(RES[:40].tolist()) | {EMPTY, LOCKED}, r)
  np.testing.assert_array_equal(r["rows"], tbl.find(kt).view(torch.uint8).reshape(4, -1).cpu().numpy())
  assert tbl.contains(kt).cpu().numpy().tolist() == [True, True, True, False]
  new = _rows(torch, keys, "float32", 4, 5)
  assert tbl.assign(kt, new, return_found=True).cpu().numpy().tolist() == [True, True, True, False]
  assert torch.equal(tbl.find(kt)[:3], new[:3]) and tbl.size_host() == 42


# ---- 9. probe chains: the growing table and the dense bounded one (both find_kernel variants) --------------------------------------
@pytest.mark.parametrize("kind", ["mid", "wrap"])
def test_probe_chains_growing(env, kind):
  torch, _ = env
  tbl, scn, ref, _, look, _ = _read_fixture(env, kind, "float32")
  kt = _kt(torch, look)
  rows, ex = tbl.find(kt, return_exists=True)
  r = fm(torch, tbl, kt)
  np.testing.assert_array_equal(r["rows"], rows.view(torch.uint8).reshape(look.size, -1).cpu().numpy())
  np.testing.assert_array_equal(r["exists"] != 0, np.array([int(k) in ref for k in look]))
  assert r["exists"][np.isin(look, scn.chain)].all() and not r["exists"][np.isin(look, scn.absent)].any()
  check_pairs(look, set(ref), r)
  np.testing.assert_array_equal(tbl.contains(kt).cpu().numpy(), ex.cpu().numpy())


def test_probe_chains_dense_bounded(env):
  torch, _ = env
  scn = Scene(env, "fm_dense", "CUSTOMIZED", score=lambda i, r: 10 + r)
  tbl = scn.tbl
  res, fresh = np.concatenate(scn.res), np.concatenate(scn.fresh)       # fresh: absent keys with the residents' home buckets
  keys = np.concatenate([res, fresh, scn.by[:150], res[:50], fresh[:30]])
  np.random.default_rng(6).shuffle(keys)
  kt = _kt(torch, keys)
  resident = set(scn.present) | set(scn.by.tolist())
  rows, ex = tbl.find(kt, return_exists=True)
  r = fm(torch, tbl, kt)
  np.testing.assert_array_equal(r["rows"], rows.view(torch.uint8).reshape(keys.size, -1).cpu().numpy())
  np.testing.assert_array_equal(r["exists"] != 0, np.array([int(k) in resident for k in keys]))
  check_pairs(keys, resident, r)
  np.testing.assert_array_equal(tbl.contains(kt).cpu().numpy(), ex.cpu().numpy())
  scn.check("after find_missed")


# ---- 10. int32-key tables ----------------------------------------------------------------------------------------------------------
def test_int32_keys(env):
  torch, de = env
  t = de.CuckooHashTable(torch.int32, torch.float32, torch.zeros(4), name="fm_i32", device="cuda:0", dim=4)
  res = torch.arange(-50, 50, dtype=torch.int32, device="cuda")
  t.insert(res, torch.ones(100, 4, device="cuda"))
  keys = torch.tensor([-60, -50, 0, 49, 50, 2**31 - 1, -2**31], dtype=torch.int32, device="cuda")
  rows, mk, mi = t.lookup_missed(keys)
  assert mk.dtype == torch.int32 and mi.dtype == torch.int32
  assert sorted(zip(mk.tolist(), mi.tolist())) == sorted([(-60, 0), (50, 4), (2**31 - 1, 5), (-2**31, 6)])
  assert torch.equal(rows, t.lookup(keys)) and t.contains(keys).tolist() == [False, True, True, True, False, False, False]
