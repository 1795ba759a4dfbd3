"""GPU: the grouped training lookups de-duplicate their members' entry ids with ONE device_ops.unique_many (tfra_multi_unique) per
device and step, ahead of both grouped admissions, and change no result.

5 plain init_on_lookup="pooled" variables with a seeded callable initializer and 3 tiered ones, 256 rows x 4 ids each, dims 16 and
64.  Two steps of the tuple, safe and ragged `*_many` lookups with return_trainable, each followed by apply_combined_gradients_many:
outputs and exported contents (embedding and slots) equal, bit for bit, the same run with `device_ops.unique_many` replaced by the
loop of `unique_no_sync` — the parent's code.  The C calls are counted by wrapping `_capi.call`."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls, T, bits

pytestmark = pytest.mark.gpu

N_ROWS, PER_ROW, STEPS, UNIVERSE, DEFAULT_ID = 256, 4, 2, 1500, 424242
DIMS_PLAIN, DIMS_TIER = (16, 64, 16, 64, 16), (16, 64, 16)


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _initializer(torch, seed):
  """a seeded callable: draw c of a variable is randn of the generator seeded with (seed, c)"""
  count = [0]

  def draw(shape):
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + count[0])
    count[0] += 1
    return torch.randn(tuple(int(x) for x in shape), generator=g, device="cuda") * 0.05
  return draw


def _vars(env, tag, n_plain=len(DIMS_PLAIN), n_tier=len(DIMS_TIER)):
  torch, de = env
  opt = de.optimizers.Adam(0.01)
  tier = lambda: de.TieredHashTableCreator(de.TieredHashTableConfig(
      upper=de.HkvHashTableConfig(init_capacity=15 * 512, max_capacity=15 * 512, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=2048))
  vs = []
  for k, dim in enumerate(DIMS_PLAIN[:n_plain] + DIMS_TIER[:n_tier]):
    vs.append(de.Variable(key_dtype=torch.int64, value_dtype=torch.float32, dim=dim, devices=["cuda:0"], name="umv_%s_%d" % (tag, k),
                          initializer=_initializer(torch, k), init_on_lookup="pooled", kv_creator=tier() if k >= n_plain else None,
                          **de.DynamicEmbeddingOptimizer.variable_kwargs(opt)))
  return opt, vs


_BATCHES = {}


def _batch(torch, k, step):
  """(ids, seg, w, splits, grad) of variable k: ids over a universe of its own, half of step 1's seen in step 0; ids[0] is the safe
  form's default_id; a twelfth of the weights <= 0"""
  if (k, step) not in _BATCHES:
    rng = np.random.default_rng(100 * k + step)
    universe = np.random.default_rng(k).permutation(np.arange(1, UNIVERSE + 1, dtype=np.int64) * 7919 - 5_000_000)
    nnz = N_ROWS * PER_ROW
    ids = universe[(rng.zipf(1.2, size=nnz) + 300 * step) % UNIVERSE]
    ids[0] = DEFAULT_ID
    seg = np.repeat(np.arange(N_ROWS, dtype=np.int64), PER_ROW)
    w = rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)
    w[rng.choice(np.arange(1, nnz), size=nnz // 12, replace=False)] = np.float32(-0.5)
    w[8:12] = np.float32(-1.0)                                                  # an empty row for the safe form
    splits = np.arange(0, nnz + 1, PER_ROW, dtype=np.int64)
    _BATCHES[(k, step)] = tuple(T(torch, x) for x in (ids, seg, w, splits))
  return _BATCHES[(k, step)]


def _grad(torch, k, step, dim):
  g = torch.Generator(device="cuda").manual_seed(7000 + 10 * k + step)
  return torch.randn((N_ROWS, dim), generator=g, device="cuda") * 0.01


def _lookup_many(env, form, vs, bs):
  torch, de = env
  if form == "tuple":
    return de.embedding_lookup_sparse_many(vs, [(b[1], b[0]) for b in bs], [b[2].abs() for b in bs], combiner="sqrtn", return_trainable=True,
                                           num_rows=N_ROWS)
  if form == "safe":
    return de.safe_embedding_lookup_sparse_many(vs, [(b[1], b[0]) for b in bs], [b[2] for b in bs], combiner="mean", default_id=DEFAULT_ID,
                                                return_trainable=True, num_rows=N_ROWS)
  return de.ragged_embedding_ops.embedding_lookup_sparse_many(vs, [(b[3], b[0]) for b in bs], [b[2].abs() for b in bs], combiner="sum",
                                                              return_trainable=True)


def _contents(torch, var):
  """(sorted keys, bits of [n, (1 + aux) * dim]): embedding and slots; a tiered variable through flush() and its lower table"""
  keys, _ = var.export()
  keys = torch.sort(keys)[0]
  t = var._tables[0]
  if hasattr(t, "flush"):
    t.flush()
    table = t._lower
  else:
    table = t._table
  assert bool(table.contains(keys).all())
  return keys, bits(torch, torch.cat([table.find(keys, field=f) for f in range(var.aux_fields + 1)], dim=1))


def _train(env, form, tag, calls=None, n_plain=len(DIMS_PLAIN), n_tier=len(DIMS_TIER)):
  """-> (every step's outputs, every variable's contents, per step the C calls made inside the lookup)"""
  torch, de = env
  opt, vs = _vars(env, tag, n_plain, n_tier)
  deo = de.DynamicEmbeddingOptimizer(opt)
  outs, in_lookup = [], []
  for step in range(STEPS):
    bs = [_batch(torch, k, step) for k in range(len(vs))]
    c0 = dict(calls.n) if calls is not None else {}
    res = _lookup_many(env, form, vs, bs)
    if calls is not None:
      in_lookup.append({n: c - c0.get(n, 0) for n, c in calls.n.items() if c - c0.get(n, 0)})
    outs.append([bits(torch, out).clone() for out, _ in res])
    deo.apply_combined_gradients_many([(_grad(torch, k, step, v.dim), tw) for k, (v, (_, tw)) in enumerate(zip(vs, res))])
  for v in vs[:n_plain]:
    v._tables[0]._table.check_errors()
  return outs, [_contents(torch, v) for v in vs], in_lookup


@pytest.mark.parametrize("form", ["tuple", "safe", "ragged"])
def test_grouped_lookups_use_one_grouped_unique_and_change_nothing(env, monkeypatch, form):
  torch, de = env
  calls = Calls(monkeypatch)
  outs, contents, in_lookup = _train(env, form, form + "_new", calls)
  for d in in_lookup:
    # one grouped de-duplication per device and step in front of the two grouped admissions; no tfra_unique where there was one per member
    assert d.get("tfra_multi_unique") == 1 and d.get("tfra_unique", 0) == 0, d
    assert d.get("tfra_multi_find_or_insert") == 1 and d.get("tfra_multi_tier_find_or_insert") == 1, d

  def loop(ids_list, want_idx=True, return_launches=False):
    return [de.device_ops.unique_no_sync(ids) for ids in ids_list]
  monkeypatch.setattr(de.device_ops, "unique_many", loop)
  n0 = calls["tfra_unique"]
  outs_l, contents_l, in_lookup_l = _train(env, form, form + "_loop", calls)
  assert calls["tfra_unique"] - n0 >= STEPS * (len(DIMS_PLAIN) + len(DIMS_TIER)) and all("tfra_multi_unique" not in d for d in in_lookup_l)
  for step, (a, b) in enumerate(zip(outs, outs_l)):
    assert len(a) == len(b) == len(DIMS_PLAIN) + len(DIMS_TIER)
    for k, (x, y) in enumerate(zip(a, b)):
      assert x.shape == y.shape and torch.equal(x, y), "step %d member %d: the result differs from the loop's" % (step, k)
  for k, ((ka, ra), (kb, rb)) in enumerate(zip(contents, contents_l)):
    assert ka.numel() > 200 and torch.equal(ka, kb), "member %d: the keys differ from the loop's" % k
    assert ra.shape == rb.shape and torch.equal(ra, rb), "member %d: embedding or slots differ from the loop's" % k


def test_short_lists_keep_admit_entries(env, monkeypatch):
  """below both thresholds (ADMIT_MANY_MIN_TABLES plain, ADMIT_MANY_MIN_TIERS tiered): one admit_entries per member, no grouped call"""
  torch, de = env
  n_plain, n_tier = de.variable.ADMIT_MANY_MIN_TABLES - 1, de.variable.ADMIT_MANY_MIN_TIERS - 1
  calls = Calls(monkeypatch)
  _, _, in_lookup = _train(env, "tuple", "short", calls, n_plain, n_tier)
  for d in in_lookup:
    assert "tfra_multi_unique" not in d and d.get("tfra_unique") == n_plain + n_tier, d
    assert "tfra_multi_find_or_insert" not in d and "tfra_multi_tier_find_or_insert" not in d, d
