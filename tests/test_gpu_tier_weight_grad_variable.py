"""GPU: the gradient of sp_weights through a Variable over TieredHashTableCreator.  The tiered variable (dim 8, a static default
row, a cache of 15 * 89 slots under 3000 keys, so most keys are demoted) stands beside a twin over CuckooHashTableCreator that holds
everything: `lookup_combined_weight_grad` and `lookup_combined_ragged_weight_grad` read both tiers and return the twin's bits, and
`SparseTrainableWrapper.weights_grad` takes the table route — `_DeviceTier.find_combine_weight_grad`, no `params.lookup` — for a
tiered variable as it does for any other the pooled forward serves."""
import numpy as np
import pytest

from tests.test_gpu_tier_sparse_variable import CAP, DIM, UNIVERSE, _cfg, _demoted, _sparse_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def bits(torch, x):
  return x.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def served(env):
  """(tiered, twin, keys, absent): both variables hold the same 3000 rows; most of the tiered one's are only below"""
  torch, de = env
  rng = np.random.default_rng(83)
  pool = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 300, dtype=np.int64))
  rng.shuffle(pool)
  keys, absent = pool[:UNIVERSE], pool[UNIVERSE:UNIVERSE + 100]
  rows = rng.standard_normal((UNIVERSE, DIM)).astype(np.float32)
  tiered = de.Variable(dim=DIM, name="twv_tiered", initializer=0.25, kv_creator=de.TieredHashTableCreator(_cfg(de)))
  twin = de.Variable(dim=DIM, name="twv_twin", initializer=0.25, kv_creator=de.CuckooHashTableCreator())
  for var in (tiered, twin):
    var.upsert(torch.from_numpy(keys).cuda(), torch.from_numpy(rows).cuda())
  assert tiered.can_lookup_combined() and twin.can_lookup_combined()
  t = tiered._tables[0]
  assert int(t._table.contains(torch.from_numpy(keys).cuda()).sum()) <= CAP < UNIVERSE // 2
  return tiered, twin, keys, absent


class Counter:
  """counts the calls of owner.name while it is installed; the call goes through"""

  def __init__(self, monkeypatch, owner, name):
    self.n = 0
    inner = getattr(owner, name)

    def counted(*a, **kw):
      self.n += 1
      return inner(*a, **kw)
    monkeypatch.setattr(owner, name, counted)


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_the_variables_reads_see_both_tiers(env, served, combiner):
  torch, de = env
  tiered, twin, keys, absent = served
  seg, ids, w, splits, n = _sparse_batch(torch, np.random.default_rng(89), keys, absent)
  assert _demoted(torch, tiered, ids) > 100                        # the batch is full of keys that are only below
  t = tiered._tables[0]
  stats = t._tier.stats()
  G = torch.randn((n, DIM), generator=torch.Generator(device="cuda").manual_seed(7), device="cuda")
  for wt in (None, w):
    a = tiered.lookup_combined_weight_grad(ids, seg, wt, combiner, G)          # (raised ValueError before the tier had the call)
    b = twin.lookup_combined_weight_grad(ids, seg, wt, combiner, G)
    assert a.dtype == torch.float32 and tuple(a.shape) == (ids.numel(),)
    assert torch.equal(bits(torch, a), bits(torch, b)), wt is None
    cache = t._table.find_combine_weight_grad(ids, seg, wt, de.device_ops.COMBINERS[combiner], G, t._default_value)
    assert int((bits(torch, a) != bits(torch, cache)).sum()) > 100            # the cache alone does not give it
    r = tiered.lookup_combined_ragged_weight_grad(splits, ids, wt, combiner, G)
    assert torch.equal(bits(torch, r), bits(torch, a))
    for kw in (dict(prune=True), dict(prune=True, fill_id=int(keys[0])), dict(fill_id=int(absent[0]))):
      a = tiered.lookup_combined_ragged_weight_grad(splits, ids, wt, combiner, G, **kw)
      b = twin.lookup_combined_ragged_weight_grad(splits, ids, wt, combiner, G, **kw)
      assert torch.equal(bits(torch, a), bits(torch, b)), kw
      if wt is not None and kw.get("prune"):
        assert not bool(bits(torch, a[wt <= 0]).any()) and bool(a[wt > 0].any())
  assert t._tier.stats() == stats                                  # reads: nothing moved, nothing was counted
  assert _demoted(torch, tiered, ids) > 100
  t._table.check_errors()
  t._lower.check_errors()


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_weights_grad_of_a_tiered_variable_takes_the_table_route(env, served, monkeypatch, combiner):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
  tiered, twin, keys, absent = served
  seg, ids, w, splits, n = _sparse_batch(torch, np.random.default_rng(97), keys, absent)
  w = w.abs() + 0.1                                                # the plain form prunes nothing: keep the weight sums away from 0
  G = torch.randn((n, DIM), generator=torch.Generator(device="cuda").manual_seed(11), device="cuda")
  tier_calls = Counter(monkeypatch, _DeviceTier, "find_combine_weight_grad")
  table_calls = Counter(monkeypatch, _DeviceTable, "find_combine_weight_grad")
  got = {}
  for name, var in (("tiered", tiered), ("twin", twin)):
    out, tw = de.embedding_lookup_sparse(var, (seg, ids), w, combiner=combiner, return_trainable=True, num_rows=n)
    lookups = Counter(monkeypatch, var, "lookup")
    before = tier_calls.n, table_calls.n
    got[name] = out, tw.weights_grad(G)
    assert lookups.n == 0, name                                    # no [U, dim] rows were fetched
    # the tiered variable goes through the tier's entry point, every other one through its table's, as before
    assert (tier_calls.n - before[0], table_calls.n - before[1]) == ((1, 0) if name == "tiered" else (0, 1)), name
  assert torch.equal(bits(torch, got["tiered"][0]), bits(torch, got["twin"][0]))
  dw = got["tiered"][1]
  assert dw.dtype == torch.float32 and tuple(dw.shape) == (ids.numel(),) and bool(dw.any())
  assert torch.equal(bits(torch, dw), bits(torch, got["twin"][1]))


def test_the_safe_form_keeps_the_callers_length_and_order(env, served, monkeypatch):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTier
  tiered, twin, keys, absent = served
  seg, ids, w, splits, n = _sparse_batch(torch, np.random.default_rng(101), keys, absent)
  pruned = w <= 0
  assert int(pruned.sum()) > 50 and int((~pruned).sum()) > 50
  G = torch.randn((n, DIM), generator=torch.Generator(device="cuda").manual_seed(13), device="cuda")
  tier_calls = Counter(monkeypatch, _DeviceTier, "find_combine_weight_grad")
  for form, sp in ((de.safe_embedding_lookup_sparse, dict(sp_ids=(seg, ids), num_rows=n)),
                   (de.ragged_embedding_ops.safe_embedding_lookup_sparse, dict(sp_ids=(splits, ids)))):
    got = []
    for var in (tiered, twin):
      kw = dict(sp)
      out, tw = form(var, kw.pop("sp_ids"), w, combiner="mean", default_id=int(keys[1]), return_trainable=True, **kw)
      got.append((out, tw.weights_grad(G)))
    (out_a, dw_a), (out_b, dw_b) = got
    assert torch.equal(bits(torch, out_a), bits(torch, out_b))
    assert tuple(dw_a.shape) == (w.numel(),) and not bool(bits(torch, dw_a[pruned]).any()) and bool(dw_a[~pruned].any())
    assert torch.equal(bits(torch, dw_a), bits(torch, dw_b))
  assert tier_calls.n == 2
