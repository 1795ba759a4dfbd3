"""GPU: the layers of `de.layers`.

FieldWiseEmbedding: the reference docstring's case (PY/keras/layers/embedding.py:385-406) at dim 4 on the pooled route and at dim 2
through the chain, before and after the upsert of ones; the forward is, bit for bit, `ragged_embedding_ops.embedding_lookup_sparse`
on the lists the torch route builds (sum / mean / sqrtn, float32 / float16 / bfloat16); three Adam steps through
`apply_combined_gradients` with gradients of shape [batch, nslots, dim] leave embedding, m and v bit-identical to a twin variable
trained through `embedding_lookup_sparse(return_trainable=True)` on the torch-built lists — with a static initializer, with
init_on_lookup="pooled" and over a tiered variable whose cache evicts.  SquashedEmbedding: sum / mean on rank-2 ids are the ragged
pooled lookup's bits, every other combiner or rank the torch reduction of Embedding's result.  Embedding: with_unique on and off
return the same rows in ids.shape + (dim,)."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls, T, bits

pytestmark = pytest.mark.gpu

BATCH, PER, NSLOTS, DIM = 7, 65, 5, 8
CAP = 15 * 89


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def slot_of(nslots):
  return lambda ids: (ids % nslots + nslots) % nslots   # (a field for negative ids too)


def _initializer(torch, seed):
  count = [0]

  def draw(shape):
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + count[0])
    count[0] += 1
    return torch.randn(tuple(int(x) for x in shape), generator=g, device="cuda") * 0.05
  return draw


def _ids(torch, seed, batch=BATCH, per=PER, universe=3000):
  rng = np.random.default_rng(seed)
  return T(torch, ((rng.zipf(1.2, size=(batch, per)) + 17 * seed) % universe).astype(np.int64) * 7 - 5000)


# ---- the reference docstring's case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 2], ids=["pooled", "chain"])
def test_docstring_case(env, dim):
  torch, de = env
  layer = de.layers.FieldWiseEmbedding(dim, 3, slot_map_fn=lambda x: x % 3, initializer=0.0, name="fwl_kat%d" % dim)
  assert layer.params.can_lookup_combined() == (dim == 4)
  ids = torch.tensor([[23, 12, 0], [9, 13, 10]], dtype=torch.int64, device="cuda")
  out = layer(ids)
  assert out.shape == (2, 3, dim) and out.dtype == torch.float32 and not bool(out.any())
  layer.params.upsert(torch.arange(100, device="cuda"), torch.ones((100, dim), device="cuda"))
  out = layer(ids)
  want = torch.tensor([[2.0, 0.0, 1.0], [1.0, 2.0, 0.0]], device="cuda").reshape(2, 3, 1).expand(2, 3, dim)
  assert torch.equal(out, want)
  mean = de.layers.FieldWiseEmbedding(dim, 3, slot_map_fn=lambda x: x % 3, initializer=0.0, combiner="mean", name="fwl_katm%d" % dim)
  mean.params.upsert(torch.arange(100, device="cuda"), torch.ones((100, dim), device="cuda"))
  assert torch.equal(mean(ids), (want > 0).to(torch.float32))
  assert layer.bad_slots() == 0
  with pytest.raises(NotImplementedError):
    layer(ids.reshape(2, 3, 1))
  with pytest.raises(ValueError, match="per_sample"):
    layer(ids.reshape(-1))


def test_bad_slots_are_counted_and_clamped(env):
  torch, de = env
  layer = de.layers.FieldWiseEmbedding(4, 3, slot_map_fn=lambda x: x - 11, initializer=0.0, name="fwl_bad")
  layer.params.upsert(torch.arange(100, device="cuda"), torch.ones((100, 4), device="cuda"))
  ids = torch.tensor([[10, 11, 12], [13, 14, 15]], dtype=torch.int64, device="cuda")   # slots -1, 0, 1 and 2, 3, 4
  out = layer(ids)
  want = torch.tensor([[2.0, 1.0, 0.0], [0.0, 0.0, 3.0]], device="cuda").reshape(2, 3, 1).expand(2, 3, 4)
  assert torch.equal(out, want) and layer.bad_slots() == 3
  layer(ids)
  assert layer.bad_slots() == 6


# ---- the forward is the ragged lookup on the torch-built lists --------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", ["float32", "float16", "bfloat16"])
def test_forward_equals_the_lookup_on_the_torch_built_lists(env, monkeypatch, vdtype):
  torch, de = env
  dops, reo = de.device_ops, de.ragged_embedding_ops
  ids = _ids(torch, 3)
  dt = getattr(torch, vdtype)
  calls = Calls(monkeypatch)
  for combiner in ("sum", "mean", "sqrtn", "sqrt_n"):
    layer = de.layers.FieldWiseEmbedding(DIM, NSLOTS, slot_map_fn=slot_of(NSLOTS), value_dtype=dt, combiner=combiner, initializer=0.25,
                                         name="fwl_fwd_%s_%s" % (vdtype, combiner))
    keys = torch.unique(ids)[::2].contiguous()   # every second id is resident
    g = torch.Generator(device="cuda").manual_seed(11)
    layer.params.upsert(keys, torch.randn((keys.numel(), DIM), generator=g, device="cuda").to(dt))
    before = calls["tfra_field_entries"]
    out = layer(ids)
    assert calls["tfra_field_entries"] == before + 1
    assert out.shape == (BATCH, NSLOTS, DIM) and out.dtype == torch.float32
    e, rs, _, _ = dops._field_entries_torch(ids, slot_of(NSLOTS)(ids), NSLOTS)
    want = reo.embedding_lookup_sparse(layer.params, (rs, e), None, combiner=combiner.replace("_", ""))
    assert torch.equal(bits(torch, out), bits(torch, want.reshape(BATCH, NSLOTS, DIM))), combiner
    assert bool(out.any())


# ---- training: three Adam steps against a twin on the torch-built lists -----------------------------------------------------------
def _contents(torch, var):
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


def _tier(de):
  return de.TieredHashTableCreator(de.TieredHashTableConfig(
      upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=2048))


@pytest.mark.parametrize("kind", ["static", "pooled", "tiered"])
@pytest.mark.parametrize("combiner", ["mean", "sqrtn"])
def test_three_adam_steps_equal_the_twin(env, monkeypatch, kind, combiner):
  torch, de = env
  dops, reo = de.device_ops, de.ragged_embedding_ops
  opt = de.optimizers.Adam(0.01)
  slots_kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  batch = 30 if kind == "tiered" else BATCH   # 30 x 65 ids a step: three steps bring more keys than the cache holds

  def kw():
    return {"static": dict(initializer=0.25), "pooled": dict(initializer=_initializer(torch, 5), init_on_lookup="pooled"),
            "tiered": dict(initializer=0.25, kv_creator=_tier(de))}[kind]
  tag = "%s_%s" % (kind, combiner)
  layer = de.layers.FieldWiseEmbedding(DIM, NSLOTS, slot_map_fn=slot_of(NSLOTS), combiner=combiner, name="fwl_train_" + tag,
                                       **kw(), **slots_kw)
  twin = de.Variable(dim=DIM, name="fwl_twin_" + tag, **kw(), **slots_kw)
  assert isinstance(layer.params, de.Variable) and layer.params.aux_fields == len(opt.slots)
  deo_a, deo_b = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(de.optimizers.Adam(0.01))
  calls = Calls(monkeypatch)
  for step in range(3):
    ids = _ids(torch, 50 + step, batch=batch, universe=6000)
    g = torch.Generator(device="cuda").manual_seed(900 + step)
    grad = torch.randn((batch, NSLOTS, DIM), generator=g, device="cuda") * 0.01
    out, tw = layer(ids, return_trainable=True, plan_writeback=(step == 1))
    assert isinstance(tw, de.SparseTrainableWrapper) and out.shape == (batch, NSLOTS, DIM)
    e, rs, _, seg = dops._field_entries_torch(ids, slot_of(NSLOTS)(ids), NSLOTS)
    assert torch.equal(tw.entry_ids, e) and torch.equal(tw.seg, seg)   # the builder's segments are the wrapper's, not re-derived
    out_t, tw_t = reo.embedding_lookup_sparse(twin, (rs, e), None, combiner=combiner, return_trainable=True)
    assert torch.equal(bits(torch, out), bits(torch, out_t.reshape(batch, NSLOTS, DIM))), step
    with pytest.raises(ValueError, match="shape"):
      tw.check_grad_out(grad.reshape(batch * NSLOTS, DIM))
    deo_a.apply_combined_gradients([(grad, tw)])
    deo_b.apply_combined_gradients([(grad.reshape(batch * NSLOTS, DIM), tw_t)])
  assert calls["tfra_field_entries"] == 3
  if kind == "tiered":
    t = layer.params._tables[0]
    keys = layer.params.export()[0]
    assert int((~t._table.contains(keys) & t._lower.contains(keys)).sum()) > 0   # the cache has evicted
  (ka, ra), (kb, rb) = _contents(torch, layer.params), _contents(torch, twin)
  assert ka.numel() > 500 and torch.equal(ka, kb)
  assert ra.shape == rb.shape == (ka.numel(), 3 * DIM) and torch.equal(ra, rb)   # embedding, m and v


# ---- SquashedEmbedding and Embedding ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filled(env):
  """a Squashed layer per combiner over the same rows, and the rows' plain Embedding"""
  torch, de = env
  ids = _ids(torch, 9, batch=6, per=10, universe=400)
  keys = torch.unique(ids)[::3].contiguous()
  g = torch.Generator(device="cuda").manual_seed(13)
  rows = torch.randn((keys.numel(), DIM), generator=g, device="cuda")
  layers = {}
  for c in ("sum", "mean", "max", "min", "prod"):
    layers[c] = de.layers.SquashedEmbedding(DIM, combiner=c, initializer=0.5, name="sql_" + c)
    layers[c].params.upsert(keys, rows)
  plain = de.layers.Embedding(DIM, initializer=0.5, name="sql_plain")
  plain.params.upsert(keys, rows)
  return ids, layers, plain


@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_squashed_rank2_is_the_ragged_pooled_lookup(env, filled, combiner):
  torch, de = env
  ids, layers, plain = filled
  layer = layers[combiner]
  b, s = ids.shape
  splits = torch.arange(b + 1, device="cuda") * s
  want = de.ragged_embedding_ops.embedding_lookup_sparse(layer.params, (splits, ids.reshape(-1)), None, combiner=combiner)
  out = layer(ids)
  assert out.shape == (b, DIM) and torch.equal(bits(torch, out), bits(torch, want))
  out, tw = layer(ids, return_trainable=True)
  assert isinstance(tw, de.SparseTrainableWrapper) and tw.out_shape == (b, DIM) and torch.equal(bits(torch, out), bits(torch, want))


@pytest.mark.parametrize("combiner", ["sum", "mean", "max", "min", "prod"])
def test_squashed_elsewhere_is_the_torch_reduction(env, filled, combiner):
  torch, de = env
  ids, layers, plain = filled
  layer = layers[combiner]
  red = {"sum": torch.sum, "mean": torch.mean, "max": torch.amax, "min": torch.amin, "prod": torch.prod}[combiner]
  rows = plain(ids)                                   # [6, 10, DIM]
  if combiner not in ("sum", "mean"):
    assert torch.equal(layer(ids), red(rows, 1))
  ids3 = ids.reshape(3, 2, 10)
  assert torch.equal(layer(ids3), red(red(plain(ids3), 1), 1)) and layer(ids3).shape == (3, DIM)
  one = ids[0]
  assert torch.equal(layer(one), red(plain(one), 0)) and layer(one).shape == (DIM,)
  with pytest.raises(ValueError, match="pooled route"):
    layer(ids3, return_trainable=True)
  if combiner not in ("sum", "mean"):
    with pytest.raises(ValueError, match="combiner"):
      layer(ids, return_trainable=True)


def test_embedding_with_and_without_unique(env, filled):
  torch, de = env
  ids, layers, plain = filled
  other = de.layers.Embedding(DIM, initializer=0.5, name="sql_plain_nu", with_unique=False)
  keys = torch.unique(ids)[::3].contiguous()
  other.params.upsert(keys, plain.params.lookup(keys))
  assert plain.with_unique and not other.with_unique
  for shape in ((6, 10), (60,), (3, 4, 5)):
    x = ids.reshape(shape)
    a, b = plain(x), other(x)
    assert a.shape == tuple(shape) + (DIM,) and torch.equal(a, b)
    assert torch.equal(a.reshape(-1, DIM), plain.params.lookup(x.reshape(-1)))
  out, tw = other(ids, return_trainable=True, plan_writeback=True)
  assert isinstance(tw, de.TrainableWrapper) and out.shape == (6, 10, DIM)
  with pytest.raises(ValueError, match="with_unique=False"):
    plain(ids, plan_writeback=True)
