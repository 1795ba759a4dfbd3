"""GPU: int32 keys through the whole frontend — sharded Variables, checkpoints, the four lookups, training, the step drivers,
find_unique and the routes.  The engine keeps int64 keys and widens int32 ones in front of every call; everything around the table
must keep the ids' own dtype and, for an int32 table, place keys by the reference's int32 rule: default_partition_fn sends int32
keys to ``math_ops.mod(keys, N)``, floor mod (PY/dynamic_embedding_variable.py:191-196), and only int64 keys to
``int32(key & 0x7fffffff) % N`` (:182-190).  Shard counts 3, 5, 6 and 7 tell the two rules apart on negative keys; 2 and 8 are
controls.  Every key set holds INT32_MIN, INT32_MAX, -1, 0, a dense run of negative keys and random keys over the int32 range.

Each check is against a plain reference: oracle.CpuTable, numpy restatements of the reference's partition and file layout
(K/cuckoo_hashtable_op.cc:310-391: `<prefix>-keys` = raw K[]), the numpy forward of tests/test_gpu_sparse_train.py, or an
int64-keyed twin fed the same ids widened — a key's update depends only on its own occurrences (hot_sums_kernel / add_rows in
tfra_apply.hip sum per key), so the twins must agree bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "recommenders-addons_amd")):
  if p not in sys.path:
    sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
_N = [0]


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  assert torch.cuda.is_available()
  return torch, de


def _name(stem):
  _N[0] += 1
  return "i32s_%s_%d" % (stem, _N[0])


def keys32(seed=0, n_random=3000, dense=(-700, 0)):
  """Distinct int32 keys: the extremes, -1, 0, a dense negative run and random keys over the whole range."""
  rng = np.random.default_rng(seed)
  k = np.concatenate([[I32.min, I32.max, -1, 0, I32.min + 1, I32.max - 1, -2, 1], np.arange(*dense),
                      rng.integers(I32.min, I32.max, size=n_random, endpoint=True)]).astype(np.int32)
  k = np.unique(k)
  return k[rng.permutation(k.size)]


def floor_owner(k, n):
  """PY/dynamic_embedding_variable.py:195 for int32 keys: math_ops.mod(keys, shard_num) — floor mod."""
  return np.mod(np.asarray(k, np.int64), n)


def mask_owner(k, n):
  """PY/dynamic_embedding_variable.py:182-190 for int64 keys: int32(key & 0x7fffffff) % shard_num."""
  return (np.asarray(k, np.int64) & 0x7FFFFFFF) % n


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twins(torch, de, stem, shards, dim, opt=None, initializer=0.25, **kw):
  """An int32-key Variable and its int64-key twin, same settings."""
  extra = de.DynamicEmbeddingOptimizer.variable_kwargs(opt) if opt is not None else {}
  extra.update(kw)
  mk = lambda kd, tag: de.Variable(key_dtype=kd, dim=dim, devices=["cuda:0"] * shards, name=_name(stem + tag), initializer=initializer,
                                   **extra)
  return mk(torch.int32, "32"), mk(torch.int64, "64")


def sorted_export(t):
  k, v = t.export()
  k = k.cpu().numpy().astype(np.int64)
  o = np.argsort(k)
  return k[o], v.cpu().numpy()[o]


# ---- shard placement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 5, 6, 7, 2, 8])
def test_shard_placement_and_table_ops(env, n):
  import oracle
  torch, de = env
  dim = 4
  keys = keys32(seed=n)
  vals = np.random.default_rng(n).standard_normal((keys.size, dim)).astype(np.float32)
  v32, v64 = twins(torch, de, "place", n, dim, initializer=-1.0)
  assert v32.tables[0].key_dtype == torch.int32
  v32.upsert(T(torch, keys), T(torch, vals))
  v64.upsert(T(torch, keys.astype(np.int64)), T(torch, vals))
  for i in range(n):
    k, v = sorted_export(v32.tables[i])
    mine = np.sort(keys[floor_owner(keys, n) == i].astype(np.int64))
    np.testing.assert_array_equal(k, mine, err_msg="int32 shard %d of %d" % (i, n))
    k64, _ = sorted_export(v64.tables[i])           # the int64 twin keeps mask-mod placement
    np.testing.assert_array_equal(k64, np.sort(keys[mask_owner(keys, n) == i].astype(np.int64)), err_msg="int64 shard %d" % i)
    assert v32.tables[i].export()[0].dtype == torch.int32
  if n not in (2, 8):
    assert np.any(floor_owner(keys, n) != mask_owner(keys, n))
  ora = oracle.CpuTable(dim)
  ora.insert(keys.astype(np.int64), vals)
  rng = np.random.default_rng(100 + n)
  probe = np.concatenate([keys[:1500], rng.integers(I32.min, I32.max, size=500, endpoint=True).astype(np.int32), [-1, 0, I32.min]])
  got, ex = v32.lookup(T(torch, probe.astype(np.int32)), return_exists=True)
  want, wex = ora.find(probe.astype(np.int64), np.full(dim, -1.0, np.float32), return_exists=True)
  np.testing.assert_array_equal(got.cpu().numpy(), want)
  np.testing.assert_array_equal(ex.cpu().numpy(), wex)
  gone = keys[::3]
  v32.remove(T(torch, gone))
  ora.remove(gone.astype(np.int64))
  assert int(v32.size().item()) == ora.size() == keys.size - gone.size
  for i in range(n):
    assert int(v32.size(i).item()) == int(np.sum(floor_owner(np.setdiff1d(keys, gone), n) == i))
  ek, ev = v32.export()
  assert ek.dtype == torch.int32
  ek = ek.cpu().numpy().astype(np.int64)
  o = np.argsort(ek)
  wk, wv = ora.export_sorted()
  np.testing.assert_array_equal(ek[o], wk)
  np.testing.assert_array_equal(ev.cpu().numpy()[o], wv)
  with pytest.raises(TypeError):
    v32.tables[0].lookup(T(torch, keys[:4].astype(np.int64)))


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_files_by_floor_mod_and_reference_files_load(env, tmp_path):
  torch, de = env
  dim, n = 4, 3
  opt = de.optimizers.Adam(1e-2)
  deo = de.DynamicEmbeddingOptimizer(opt)
  v32, _ = twins(torch, de, "ckpt", n, dim, opt=opt)
  keys = keys32(seed=31, n_random=1500)
  rng = np.random.default_rng(31)
  for _ in range(2):
    emb, tw = de.embedding_lookup(v32, T(torch, keys), return_trainable=True)
    deo.apply_gradients([(T(torch, rng.standard_normal((keys.size, dim)).astype(np.float32)), tw)])
  want = v32.lookup(T(torch, keys)).cpu().numpy()
  slots = v32.get_slot_variables(deo)
  want_slots = [s.lookup(T(torch, keys)).cpu().numpy() for s in slots]
  assert all(np.abs(w).max() > 0 for w in want_slots)
  d = tmp_path / "saved"
  v32.save_to_file_system(str(d), optimizer=deo)
  for base in [v32.name] + [s.name.replace("/", "_") for s in slots]:
    for i in range(n):
      pre = str(d / ("%s_mht_%dof%d" % (base, i + 1, n)))
      fk = np.fromfile(pre + "-keys", dtype=np.int32)            # raw 4-byte keys
      assert os.path.getsize(pre + "-values") == fk.size * dim * 4
      np.testing.assert_array_equal(np.sort(fk), np.sort(keys[floor_owner(keys, n) == i]), err_msg=pre)
  # restore into 3 shards and into 5 (re-partitioned through the int32 rule), slots included
  for shards in (3, 5):
    r = de.Variable(key_dtype=torch.int32, dim=dim, devices=["cuda:0"] * shards, name=v32.name, initializer=0.25,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    r.load_from_file_system(str(d), optimizer=deo)
    assert int(r.size().item()) == keys.size
    np.testing.assert_array_equal(r.lookup(T(torch, keys)).cpu().numpy(), want)
    for s, w in zip(r.get_slot_variables(deo), want_slots):
      np.testing.assert_array_equal(s.lookup(T(torch, keys)).cpu().numpy(), w)
    for i in range(shards):
      np.testing.assert_array_equal(sorted_export(r.tables[i])[0], np.sort(keys[floor_owner(keys, shards) == i].astype(np.int64)))
  # files written the reference's way (numpy, floor-mod split, <name>_mht_{i}of{N}-keys/-values) load into 3 and into 2 shards
  ref = tmp_path / "ref"
  ref.mkdir()
  rk = keys32(seed=32, n_random=800)
  rv = np.random.default_rng(32).standard_normal((rk.size, dim)).astype(np.float32)
  own = floor_owner(rk, n)
  for i in range(n):
    rk[own == i].tofile(str(ref / ("refvar_mht_%dof%d-keys" % (i + 1, n))))
    rv[own == i].tofile(str(ref / ("refvar_mht_%dof%d-values" % (i + 1, n))))
  for shards in (3, 2):
    r = de.Variable(key_dtype=torch.int32, dim=dim, devices=["cuda:0"] * shards, name="refvar", initializer=-9.0)
    r.load_from_file_system(str(ref))
    got, ex = r.lookup(T(torch, rk), return_exists=True)
    assert bool(ex.all())
    np.testing.assert_array_equal(got.cpu().numpy(), rv)


# ---- unique / find_unique ----------------------------------------------------------------------------------------------------------
def test_unique_ops_keep_int32(env):
  torch, de = env
  from tfra_amd.dynamic_embedding import device_ops
  keys = keys32(seed=5, n_random=2000)
  rng = np.random.default_rng(5)
  ids = keys[rng.integers(0, keys.size, size=9000)]
  ids[:6] = [I32.min, I32.max, -1, 0, I32.min, -1]
  t = T(torch, ids)
  for ordered in (True, False):
    u, idx, cnt = device_ops.unique(t, ordered=ordered)
    assert u.dtype == torch.int32 and int(cnt.item()) == u.numel()
    un, ix = u.cpu().numpy(), idx.cpu().numpy()
    np.testing.assert_array_equal(np.sort(un), np.unique(ids))
    np.testing.assert_array_equal(un[ix], ids)
  u, idx, cnt = device_ops.unique_no_sync(t)
  assert u.dtype == torch.int32 and u.numel() == ids.size
  c = int(cnt.item())
  np.testing.assert_array_equal(np.sort(u.cpu().numpy()[:c]), np.unique(ids))
  np.testing.assert_array_equal(u.cpu().numpy()[idx.cpu().numpy()], ids)
  # widened ids give the same de-duplication
  u64, idx64, _ = device_ops.unique(t.to(torch.int64))
  np.testing.assert_array_equal(device_ops.unique(t)[0].cpu().numpy().astype(np.int64), u64.cpu().numpy())
  np.testing.assert_array_equal(device_ops.unique(t)[1].cpu().numpy(), idx64.cpu().numpy())
  g = torch.randn((ids.size, 8), device="cuda")
  kb, sums, cnt = device_ops.reduce_by_key(t, g)
  kb64, sums64, cnt64 = device_ops.reduce_by_key(t.to(torch.int64), g)
  c = int(cnt.item())
  assert kb.dtype == torch.int32 and c == int(cnt64.item()) == np.unique(ids).size
  k32, k64 = kb.cpu().numpy()[:c].astype(np.int64), kb64.cpu().numpy()[:c]   # (the key order is unspecified)
  o32, o64 = np.argsort(k32), np.argsort(k64)
  np.testing.assert_array_equal(k32[o32], np.unique(ids))
  np.testing.assert_array_equal(k64[o64], np.unique(ids))
  np.testing.assert_array_equal(sums[:c].cpu().numpy()[o32], sums64[:c].cpu().numpy()[o64])
  for n in (3, 7):
    km, perm, counts = device_ops.partition(t, n, device_ops.PARTITION_FLOOR_MOD)
    assert km.dtype == torch.int32
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(floor_owner(ids, n), minlength=n))
    np.testing.assert_array_equal(km.cpu().numpy(), ids[perm.cpu().numpy()])
  for bad in (t.to(torch.int16), t.to(torch.float32)):
    with pytest.raises(TypeError):
      device_ops.unique(bad)
    with pytest.raises(TypeError):
      device_ops.unique_no_sync(bad)
  torch.cuda.synchronize()


def test_find_unique_returns_table_dtype(env):
  import oracle
  torch, de = env
  dim = 4
  keys = keys32(seed=8, n_random=1000)
  vals = np.random.default_rng(8).standard_normal((keys.size, dim)).astype(np.float32)
  t = de.CuckooHashTable(torch.int32, torch.float32, torch.full((dim,), -1.0), device="cuda:0", dim=dim, name=_name("fu"))
  t.insert(T(torch, keys), T(torch, vals))
  rng = np.random.default_rng(9)
  ids = np.concatenate([keys[rng.integers(0, keys.size, size=3000)], [I32.min, I32.max, -1, 0, 7, 7]]).astype(np.int32)
  rows, uniq, idx, cnt = t._table.find_unique(T(torch, ids))
  assert uniq.dtype == torch.int32
  c = int(cnt.item())
  un = uniq[:c].cpu().numpy()
  np.testing.assert_array_equal(np.sort(un), np.unique(ids))
  np.testing.assert_array_equal(uniq.cpu().numpy()[idx.cpu().numpy()], ids)
  ora = oracle.CpuTable(dim)
  ora.insert(keys.astype(np.int64), vals)
  np.testing.assert_array_equal(rows.cpu().numpy(), ora.find(ids.astype(np.int64), np.full(dim, -1.0, np.float32)))
  # the uniques go straight back into the table
  t._table.upsert(uniq[:c], torch.full((c, dim), 3.0, device="cuda"))
  ora.insert(un.astype(np.int64), np.full((c, dim), 3.0, np.float32))
  t._table.erase(uniq[: c // 2])
  ora.remove(un[: c // 2].astype(np.int64))
  k, v = sorted_export(t)
  wk, wv = ora.export_sorted()
  np.testing.assert_array_equal(k, wk)
  np.testing.assert_array_equal(v, wv)


# ---- the four lookups ----------------------------------------------------------------------------------------------------------------
def _sparse_case(rng, n_rows, keys, weighted):
  counts = rng.integers(0, 5, size=n_rows)
  counts[0] = 0
  counts[3] = 0
  rows = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = keys[rng.integers(0, keys.size, size=rows.size)].astype(np.int32)
  ids[:4] = [I32.min, I32.max, -1, 0]
  w = rng.uniform(-0.5, 2.0, size=rows.size).astype(np.float32) if weighted else None   # weights <= 0 are pruned
  ind = np.stack([rows, np.zeros_like(rows)], 1)
  return ind, ids, w


@pytest.mark.parametrize("shards", [1, 3])
def test_lookups_int32_ids_match_int64_twin_and_numpy(env, shards):
  import oracle
  from tests.test_gpu_sparse_train import _np_entries, _np_forward
  torch, de = env
  dim = 8
  keys = keys32(seed=20 + shards, n_random=1500)
  vals = np.random.default_rng(20).standard_normal((keys.size, dim)).astype(np.float32)
  v32, v64 = twins(torch, de, "look", shards, dim, initializer=0.5)
  v32.upsert(T(torch, keys), T(torch, vals))
  v64.upsert(T(torch, keys.astype(np.int64)), T(torch, vals))
  tab = oracle.CpuTable(dim)
  tab.insert(keys.astype(np.int64), vals)
  rng = np.random.default_rng(21)
  ids = np.concatenate([keys[rng.integers(0, keys.size, size=4000)], [I32.min, I32.max, -1, 0, -123456789, 55]]).astype(np.int32)
  ids2 = ids.reshape(-1, 2)
  for fn in (de.embedding_lookup, de.embedding_lookup_unique):
    a = fn(v32, T(torch, ids2))
    b = fn(v64, T(torch, ids2.astype(np.int64)))
    assert tuple(a.shape) == ids2.shape + (dim,)
    assert torch.equal(a, b), fn.__name__
    np.testing.assert_array_equal(a.cpu().numpy().reshape(-1, dim), tab.find(ids.astype(np.int64), np.full(dim, 0.5, np.float32)))
  n_rows = 300
  for weighted in (False, True):
    ind, sid, w = _sparse_case(rng, n_rows, keys, weighted)
    sp_w = None if w is None else T(torch, w)
    for comb in ("sum", "mean", "sqrtn"):
      if weighted and comb != "sum":
        a = de.embedding_lookup_sparse(v32, (T(torch, ind), T(torch, sid)), T(torch, np.abs(w) + 0.1), combiner=comb, num_rows=n_rows)
        b = de.embedding_lookup_sparse(v64, (T(torch, ind), T(torch, sid.astype(np.int64))), T(torch, np.abs(w) + 0.1), combiner=comb,
                                       num_rows=n_rows)
        assert torch.equal(a, b)
      else:
        a = de.embedding_lookup_sparse(v32, (T(torch, ind), T(torch, sid)), sp_w, combiner=comb, num_rows=n_rows)
        b = de.embedding_lookup_sparse(v64, (T(torch, ind), T(torch, sid.astype(np.int64))), sp_w, combiner=comb, num_rows=n_rows)
        assert torch.equal(a, b)
      for default_id in (None, -1, I32.min):
        kw = dict(combiner=comb, default_id=default_id)
        a = de.safe_embedding_lookup_sparse(v32, (T(torch, ind), T(torch, sid), [n_rows, 2]), sp_w, **kw)
        b = de.safe_embedding_lookup_sparse(v64, (T(torch, ind), T(torch, sid.astype(np.int64)), [n_rows, 2]), sp_w, **kw)
        assert torch.equal(a, b), (comb, default_id, weighted)
        e = _np_entries(ind, sid.astype(np.int64), w, [n_rows, 2], kw, safe=True)
        want = _np_forward(tab, *e, dim, 0.5)
        np.testing.assert_allclose(a.cpu().numpy(), want, rtol=2e-6, atol=2e-6)
  with pytest.raises(TypeError):
    de.embedding_lookup(v32, T(torch, ids.astype(np.int64)))


# ---- training ------------------------------------------------------------------------------------------------------------------------
OPTS = {
    "sgd": lambda de: de.optimizers.SGD(0.1),
    "adam": lambda de: de.optimizers.Adam(1e-2),
    "adagrad": lambda de: de.optimizers.Adagrad(0.05, 0.1),
    "ftrl": lambda de: de.optimizers.Ftrl(0.05, -0.5, 0.1, 1e-3, 1e-3),
    "momentum": lambda de: de.optimizers.Momentum(0.05, 0.9),
}


def _assert_twins_equal(torch, deo, v32, v64, keys):
  a, b = sorted_export(v32), sorted_export(v64)
  np.testing.assert_array_equal(a[0], b[0])
  np.testing.assert_array_equal(a[1], b[1])
  for s32, s64 in zip(v32.get_slot_variables(deo), v64.get_slot_variables(deo)):
    assert torch.equal(s32.lookup(T(torch, keys)), s64.lookup(T(torch, keys.astype(np.int64))))


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("name", list(OPTS))
def test_training_int32_matches_int64_twin_bitwise(env, name, shards):
  torch, de = env
  dim = 8
  opt = OPTS[name](de)
  deo32, deo64 = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(OPTS[name](de))
  v32, v64 = twins(torch, de, "train_" + name, shards, dim, opt=opt, restrict_policy=de.FrequencyRestrictPolicy)
  keys = keys32(seed=40, n_random=600)
  rng = np.random.default_rng(41)
  n_rows = 256
  for step in range(3):
    ids = keys[rng.integers(0, keys.size, size=2048)]
    ids[:5] = [I32.min, I32.max, -1, 0, -1]
    g = T(torch, rng.standard_normal((ids.size, dim)).astype(np.float32))
    e32, tw32 = de.embedding_lookup(v32, T(torch, ids), return_trainable=True)
    e64, tw64 = de.embedding_lookup(v64, T(torch, ids.astype(np.int64)), return_trainable=True)
    assert torch.equal(e32, e64)
    deo32.apply_gradients([(g, tw32)])
    deo64.apply_gradients([(g, tw64)])
    # the combined route: safe_embedding_lookup_sparse with empty rows, pruned weights and a default id
    ind, sid, w = _sparse_case(rng, n_rows, keys, True)
    sp = lambda kd: (T(torch, ind), T(torch, sid.astype(kd)), [n_rows, 2])
    r32, st32 = de.safe_embedding_lookup_sparse(v32, sp(np.int32), T(torch, w), combiner="mean", default_id=-1, return_trainable=True)
    r64, st64 = de.safe_embedding_lookup_sparse(v64, sp(np.int64), T(torch, w), combiner="mean", default_id=-1, return_trainable=True)
    assert torch.equal(r32, r64)
    assert st32.entry_ids.dtype == torch.int32
    go = T(torch, rng.standard_normal((n_rows, dim)).astype(np.float32))
    deo32.apply_combined_gradients([(go, st32)])
    deo64.apply_combined_gradients([(go, st64)])
  _assert_twins_equal(torch, deo32, v32, v64, keys)
  f32, f64 = sorted_export(v32.restrict_policy.status), sorted_export(v64.restrict_policy.status)
  np.testing.assert_array_equal(f32[0], f64[0])
  np.testing.assert_array_equal(f32[1], f64[1])     # the restrict policy's status: the same keys and counts


@pytest.mark.parametrize("shards", [1, 3])
def test_restrict_policy_keeps_each_shards_frequent_keys(env, shards):
  """FrequencyRestrictPolicy on an int32 Variable: every shard keeps its num_reserved / N most frequent keys
  (PY/restrict_policies.py:332-358).  Ten hot keys per floor-mod residue, the rest seen once: with the wrong placement the hot
  keys spread unevenly and some shards keep cold keys."""
  torch, de = env
  dim = 4
  opt = de.optimizers.SGD(0.1)
  deo = de.DynamicEmbeddingOptimizer(opt)
  v = de.Variable(key_dtype=torch.int32, dim=dim, devices=["cuda:0"] * shards, name=_name("restrict"), initializer=0.0,
                  restrict_policy=de.FrequencyRestrictPolicy)
  keys = keys32(seed=50, n_random=400)
  own = floor_owner(keys, 3)
  hot = np.concatenate([keys[own == r][:10] for r in range(3)])
  assert np.sum(hot < 0) >= 10
  cold = np.setdiff1d(keys, hot)
  rng = np.random.default_rng(51)
  for step in range(4):
    ids = np.concatenate([hot, cold[step::4]]).astype(np.int32)
    ids = ids[rng.permutation(ids.size)]
    _, tw = de.embedding_lookup(v, T(torch, ids), return_trainable=True)
    deo.apply_gradients([(torch.ones((ids.size, dim), device="cuda"), tw)])
  removed = v.restrict(hot.size, trigger=0)
  assert removed == keys.size - hot.size
  np.testing.assert_array_equal(sorted_export(v)[0], np.sort(hot.astype(np.int64)))
  np.testing.assert_array_equal(sorted_export(v.restrict_policy.status)[0], np.sort(hot.astype(np.int64)))


# ---- step drivers ----------------------------------------------------------------------------------------------------------------
def _batches(seed, keys, n=4, size=3000):
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(n):
    b = keys[rng.integers(0, keys.size, size=size)].astype(np.int32)
    b[:4] = [I32.min, I32.max, -1, 0]
    out.append(b)
  return out


def test_step_drivers_int32_match_int64_twin(env):
  torch, de = env
  dim = 16
  keys = keys32(seed=60, n_random=2000)
  batches = _batches(61, keys)
  rng = np.random.default_rng(62)
  # PrefetchStep: fused Adam
  opt = de.optimizers.Adam(1e-2)
  deos = [de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(de.optimizers.Adam(1e-2))]
  v32, v64 = twins(torch, de, "pf", 1, dim, opt=opt)
  grads = [T(torch, rng.standard_normal((b.size, dim)).astype(np.float32)) for b in batches]
  outs = []
  for v, deo, kd in ((v32, deos[0], np.int32), (v64, deos[1], np.int64)):
    ps = de.PrefetchStep(v, deo).prime(T(torch, batches[0].astype(kd)))
    o = []
    for i in range(len(batches)):
      nxt = T(torch, batches[i + 1].astype(kd)) if i + 1 < len(batches) else None
      o.append(ps.step(grads[i], nxt).cpu().numpy())
    outs.append(o)
  for a, b in zip(*outs):
    np.testing.assert_array_equal(a, b)
  _assert_twins_equal(torch, deos[0], v32, v64, keys)
  ps = de.PrefetchStep(v32, deos[0])
  with pytest.raises(TypeError):
    ps.prime(T(torch, batches[0].astype(np.int64)))
  ps.prime(T(torch, batches[0]))
  it = deos[0].iterations
  with pytest.raises(TypeError):
    ps.step(grads[0], T(torch, batches[1].astype(np.int64)))
  assert deos[0].iterations == it
  # PrefetchAssignStep and OverlapAssignStep: lookup + insert_or_assign, the last occurrence wins
  values = [T(torch, rng.standard_normal((b.size, dim)).astype(np.float32)) for b in batches]
  for drv in ("prefetch_assign", "overlap"):
    tabs = [de.CuckooHashTable(kd, torch.float32, torch.full((dim,), -1.0), device="cuda:0", dim=dim, name=_name(drv))
            for kd in (torch.int32, torch.int64)]
    outs = []
    for t, kd in zip(tabs, (np.int32, np.int64)):
      s = (de.PrefetchAssignStep(t) if drv == "prefetch_assign" else de.OverlapAssignStep(t)).prime(T(torch, batches[0].astype(kd)))
      o = []
      for i in range(len(batches)):
        nxt = T(torch, batches[i + 1].astype(kd)) if i + 1 < len(batches) else None
        o.append(s.step(values[i], nxt).cpu().numpy())
      if drv == "overlap":
        s.flush()
      outs.append(o)
    for a, b in zip(*outs):
      np.testing.assert_array_equal(a, b)
    a, b = sorted_export(tabs[0]), sorted_export(tabs[1])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    size = int(tabs[0].size().item())
    s = de.PrefetchAssignStep(tabs[0]) if drv == "prefetch_assign" else de.OverlapAssignStep(tabs[0])
    with pytest.raises(TypeError):
      s.prime(T(torch, np.array([2**31 + 5, 1], np.int64)))    # would not fit the table's keys
    s.prime(T(torch, batches[0]))
    with pytest.raises(TypeError):
      s.step(values[0], T(torch, np.array([2**31 + 5, 1], np.int64)))
    assert int(tabs[0].size().item()) == size
  torch.cuda.synchronize()


# ---- the drivers order their second stream after the widen of int32 ids --------------------------------------------------------
SLEEP_CYCLES = 20_000_000


def test_look_ahead_drivers_wait_for_the_widen(env):
  """For an int32 table the drivers widen the next batch's ids on the current stream, and the plan of that batch is built on a
  second stream.  A long kernel (torch.cuda._sleep) in front of every step holds the current stream back: unless the second
  stream waits for the widen, the plan is built from the widened buffer before it is written.  The ids themselves are complete
  in memory (next_ids_ready=True).  Results must equal the int64 twin run without the delay."""
  torch, de = env
  dim = 16
  keys = keys32(seed=90, n_random=2000)
  batches = _batches(91, keys, n=5)
  rng = np.random.default_rng(92)
  grads = [T(torch, rng.standard_normal((b.size, dim)).astype(np.float32)) for b in batches]

  def run(make, kd, delay):
    s = make().prime(T(torch, batches[0].astype(kd)))
    outs = []
    for i in range(len(batches)):
      nxt = T(torch, batches[i + 1].astype(kd)) if i + 1 < len(batches) else None
      torch.cuda.synchronize()                      # the ids are complete before the call
      if delay:
        torch.cuda._sleep(SLEEP_CYCLES)
      outs.append(s.step(grads[i], nxt))
    return [o.cpu().numpy() for o in outs]

  opt = de.optimizers.Adagrad(0.05, 0.1)
  deos = [de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(de.optimizers.Adagrad(0.05, 0.1))]
  v32, v64 = twins(torch, de, "order_pf", 1, dim, opt=opt)
  a = run(lambda: de.PrefetchStep(v32, deos[0]), np.int32, True)
  b = run(lambda: de.PrefetchStep(v64, deos[1]), np.int64, False)
  for x, y in zip(a, b):
    np.testing.assert_array_equal(x, y)
  _assert_twins_equal(torch, deos[0], v32, v64, keys)
  tabs = [de.CuckooHashTable(kd, torch.float32, torch.full((dim,), -1.0), device="cuda:0", dim=dim, name=_name("order_pa"))
          for kd in (torch.int32, torch.int64)]
  a = run(lambda: de.PrefetchAssignStep(tabs[0]), np.int32, True)
  b = run(lambda: de.PrefetchAssignStep(tabs[1]), np.int64, False)
  for x, y in zip(a, b):
    np.testing.assert_array_equal(x, y)
  x, y = sorted_export(tabs[0]), sorted_export(tabs[1])
  np.testing.assert_array_equal(x[0], y[0])
  np.testing.assert_array_equal(x[1], y[1])


# ---- routes: world 3 on one GPU, collectives staged through gloo -------------------------------------------------------------------
RA_STEPS, RA_DIM, RA_LR = 4, 8, 0.5


def _free_port():
  import socket
  with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
    so.bind(("127.0.0.1", 0))
    return so.getsockname()[1]


def _ra_batch(rank, step):
  rng = np.random.default_rng(700 + 40 * step + rank)
  keys = keys32(seed=70, n_random=300)
  ids = keys[rng.integers(0, keys.size, size=500 + 37 * rank)].astype(np.int32)
  ids[:4] = [I32.min, I32.max, -1, 0]
  vals = rng.standard_normal((ids.size, RA_DIM)).astype(np.float32)
  return ids, vals


def _ra_worker(rank, world, port, out_dir, kind):
  """kind 'assign': RoutedAssignStep on an int32 CuckooHashTable; 'prefetch' / 'native': RoutedPrefetchStep / NativeRoutedStep on an
  int32 Variable with SGD and a frequency restrict policy.  partition_mode is left at its default everywhere.  The ids are complete
  when they are fed (ids_ready=True) and a long kernel holds the current stream back in front of every feed, so the driver's own
  stream must wait for the widen of the ids."""
  import torch
  import torch.distributed as dist
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding.distributed import NativeRoutedStep, RoutedAssignStep, RoutedPrefetchStep
  os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
  torch.cuda.set_device(0)
  dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
  try:
    batches = [_ra_batch(rank, s) for s in range(RA_STEPS)]
    ids = [torch.from_numpy(b[0]).cuda() for b in batches]
    vals = [torch.from_numpy(b[1]).cuda() for b in batches]
    torch.cuda.synchronize()

    def feed(rs, x):
      torch.cuda._sleep(SLEEP_CYCLES)
      rs.feed(x, ids_ready=True)

    out = {}
    if kind == "assign":
      t = de.CuckooHashTable(torch.int32, torch.float32, torch.zeros(RA_DIM), device="cuda:0", dim=RA_DIM, name="i32_route_r%d" % rank)
      rs = RoutedAssignStep(t, transport="staged", max_batch=4096)
      assert rs.world == world
      try:
        rs.feed(ids[0].to(torch.int64))
        raised = False
      except TypeError:
        raised = True
      for s in range(RA_STEPS):
        feed(rs, ids[s])
      looked = [rs.step().cpu().numpy()]
      for s in range(1, RA_STEPS):
        looked.append(rs.step(vals[s - 1]).cpu().numpy())
      rs.flush(vals[-1])
      torch.cuda.synchronize()
      rs.close()
    else:
      opt = de.optimizers.SGD(RA_LR)
      deo = de.DynamicEmbeddingOptimizer(opt)
      t = de.Variable(key_dtype=torch.int32, dim=RA_DIM, name="i32_%s_r%d" % (kind, rank), initializer=0.5, devices=["cuda:0"],
                      restrict_policy=de.FrequencyRestrictPolicy, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
      if kind == "native":
        rs = NativeRoutedStep(t, deo, transport="staged", max_batch=4096)
      else:
        rs = RoutedPrefetchStep(t, deo)
        assert rs.collectives
      assert rs.world == world
      try:
        rs.feed(ids[0].to(torch.int64))
        raised = False
      except TypeError:
        raised = True
      for s in range(2):
        feed(rs, ids[s])
      looked = []
      for s in range(RA_STEPS):
        looked.append(rs.lookup().cpu().numpy())
        rs.apply(vals[s])                               # the batch's gradients
        if s + 2 < RA_STEPS:
          feed(rs, ids[s + 2])
      torch.cuda.synchronize()
      if kind == "native":
        rs.close()
      sk, _ = t.restrict_policy.status.export()
      out["status_keys"] = sk.cpu().numpy()
    k, v = t.export()
    np.savez(os.path.join(out_dir, "i32_%s_rank%d.npz" % (kind, rank)), keys=k.cpu().numpy(), vals=v.cpu().numpy(),
             raised=np.array(raised), **out, **{"look%d" % s: looked[s] for s in range(RA_STEPS)})
  finally:
    dist.destroy_process_group()


def _spawn_world3(kind, tmp_path):
  import torch.multiprocessing as mp
  world = 3
  mp.spawn(_ra_worker, args=(world, _free_port(), str(tmp_path), kind), nprocs=world, join=True)
  return world, [np.load(tmp_path / ("i32_%s_rank%d.npz" % (kind, r))) for r in range(world)]


def _check_shards(res, world, ek, ev, rtol=0.0):
  gk = np.concatenate([x["keys"].astype(np.int64) for x in res])
  gv = np.concatenate([x["vals"] for x in res])
  o = np.argsort(gk)
  np.testing.assert_array_equal(gk[o], ek)           # every key on exactly one shard
  np.testing.assert_allclose(gv[o], ev, rtol=rtol, atol=rtol)
  for r in range(world):
    assert res[r]["keys"].dtype == np.int32
    assert np.all(floor_owner(res[r]["keys"], world) == r), "rank %d holds keys of another owner" % r
    assert bool(res[r]["raised"])                   # int64 ids were refused before any launch


def test_routed_assign_step_world3_int32_floor_mod(env, tmp_path):
  """RoutedAssignStep over int32 tables at world 3: each rank's shard holds exactly the keys with np.mod(k, 3) == rank, and every
  lookup equals ONE table that sees all ranks' batches (oracle/frontends.py routed_assign_model)."""
  import oracle
  from oracle import frontends as ofe
  world, res = _spawn_world3("assign", tmp_path)
  tab = oracle.CpuTable(RA_DIM)
  dflt = np.zeros(RA_DIM, np.float32)
  for s in range(RA_STEPS):
    b = [_ra_batch(r, s) for r in range(world)]
    rows = ofe.routed_assign_model(tab, [x[0] for x in b], [x[1] for x in b], dflt)
    for r in range(world):
      np.testing.assert_array_equal(res[r]["look%d" % s], rows[r], err_msg="rank %d step %d" % (r, s))
  ek, ev = tab.export_sorted()
  _check_shards(res, world, ek, ev)


@pytest.mark.parametrize("kind", ["prefetch", "native"])
def test_routed_training_world3_int32_floor_mod(env, tmp_path, kind):
  """RoutedPrefetchStep (the ids stay int32 along the route) and NativeRoutedStep (widened for the C driver; the restrict policy
  gets the served ids narrowed back) over int32 Variables at world 3, SGD: every lookup equals ONE table that sees all ranks'
  batches, the trained rows equal that table after the sum of all ranks' gradients (PY/shadow_embedding_ops.py:397-447), each
  shard holds its floor-mod keys, and the restrict policy's status has exactly the keys of its shard."""
  import oracle
  from oracle import optimizers as oopt
  world, res = _spawn_world3(kind, tmp_path)
  tab = oracle.CpuTable(RA_DIM)
  dflt = np.full(RA_DIM, 0.5, np.float32)
  for s in range(RA_STEPS):
    b = [_ra_batch(r, s) for r in range(world)]
    for r in range(world):
      np.testing.assert_allclose(res[r]["look%d" % s], tab.find(b[r][0].astype(np.int64), dflt), rtol=1e-6, atol=1e-6,
                                 err_msg="rank %d step %d" % (r, s))
    uniq, gsum, _ = oopt.segment_sum_by_key(np.concatenate([x[0] for x in b]), np.concatenate([x[1] for x in b]))
    tab.insert(uniq, oopt.sgd(tab.find(uniq, dflt), gsum, RA_LR))
  ek, ev = tab.export_sorted()
  _check_shards(res, world, ek, ev, rtol=1e-6)
  for r in range(world):
    np.testing.assert_array_equal(np.sort(res[r]["status_keys"].astype(np.int64)), np.sort(res[r]["keys"].astype(np.int64)))
