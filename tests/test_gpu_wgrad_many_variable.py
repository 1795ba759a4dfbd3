"""GPU: de.sparse_weights_grad_many — the gradients of the sp_weights of a LIST of sparse lookups, the pooled members in ONE grouped
call (tfra_multi_find_combine_backprop_weights).

Three variables as tests/test_gpu_tier_pooled_many.py's `_side` builds them — tiered, tiered and plain (dims 8, 16, 8) —, each
filled with 3000 keys, so that a tiered one's cache is full and most of its keys are only below.  The wrappers come from
embedding_lookup_sparse_many(..., return_trainable=True) and from safe_embedding_lookup_sparse_many with weights of which a
third prune.  Every result is compared bit for bit with the wrapper's own weights_grad, the single route."""
import numpy as np
import pytest

from tests.test_gpu_tier_pooled import bits
from tests.test_gpu_tier_pooled_many import UNIVERSE, _side, _sparse_batch

pytestmark = pytest.mark.gpu

GROUPED = "tfra_multi_find_combine_backprop_weights"


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture(scope="module")
def side(env):
  """(variables [tiered, tiered, plain], keys, absent, a two-shard variable of dim 8); every variable holds the keys"""
  torch, de = env
  vs, _ = _side(de, "wgm", True)
  assert [hasattr(v._tables[0], "_tier") for v in vs] == [True, True, False]
  rng = np.random.default_rng(211)
  pool = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 300, dtype=np.int64))
  rng.shuffle(pool)
  keys, absent = pool[:UNIVERSE], pool[UNIVERSE:UNIVERSE + 100]
  kt = torch.from_numpy(keys).cuda()
  two = de.Variable(dim=8, name="wgm_two_shards", initializer=0.25, devices=["cuda:0", "cuda:0"])
  for v in vs + [two]:
    v.upsert(kt, torch.from_numpy(rng.standard_normal((UNIVERSE, v.dim)).astype(np.float32)).cuda())
  for v in vs[:2]:
    t = v._tables[0]
    assert int((~t._table.contains(kt) & t._lower.contains(kt)).sum()) > UNIVERSE // 2    # a full cache, most keys only below
  assert all(v.can_lookup_combined() for v in vs) and not two.can_lookup_combined()
  return vs, keys, absent, two


@pytest.fixture
def c_names(monkeypatch):
  from tfra_amd import _capi
  names, real = [], _capi.call

  def call(name, *args):
    names.append(name)
    return real(name, *args)

  monkeypatch.setattr(_capi, "call", call)
  return names


def _grads(torch, rng, wrappers):
  return [torch.from_numpy(rng.standard_normal(tw.out_shape).astype(np.float32)).cuda() for tw in wrappers]


def _same(torch, got, want):
  assert len(got) == len(want)
  for k, (a, b) in enumerate(zip(got, want)):
    assert a.dtype == torch.float32 and a.shape == b.shape, k
    assert torch.equal(bits(torch, a), bits(torch, b)), "member %d" % k


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_one_grouped_call_gives_what_every_weights_grad_gives(env, side, c_names, combiner):
  torch, de = env
  vs, keys, absent, _ = side
  rng = np.random.default_rng(223)
  batches = [_sparse_batch(torch, rng, keys, absent) for _ in vs]      # (seg, ids, weights, splits, n_rows); a third of the weights <= 0
  n = batches[0][4]
  tup, ws = [(b[0], b[1]) for b in batches], [b[2] for b in batches]
  plain = de.embedding_lookup_sparse_many(vs, tup, [w.abs() + 0.1 for w in ws], combiner=combiner, return_trainable=True, num_rows=n)
  safe = de.safe_embedding_lookup_sparse_many(vs, tup, ws, combiner=combiner, return_trainable=True, num_rows=n)
  wrappers = [tw for _, tw in plain] + [tw for _, tw in safe]
  if combiner != "sum":
    assert all(tw._caller_weights is not None for _, tw in safe)       # entries were pruned: the caller's length differs from the lookup's
    assert all(tw._weights.numel() < w.numel() for (_, tw), w in zip(safe, ws))
  grads = _grads(torch, rng, wrappers)
  pairs = list(zip(grads, wrappers))
  del c_names[:]
  got = de.sparse_weights_grad_many(pairs)
  seen = [x for x in c_names if "backprop_weights" in x]
  assert seen == [GROUPED], seen                                        # ONE grouped call, and no single call beside it
  del c_names[:]
  want = [tw.weights_grad(g) for g, tw in pairs]
  assert len([x for x in c_names if "backprop_weights" in x]) == len(pairs) and GROUPED not in c_names
  _same(torch, got, want)
  for dw, w in zip(got, ws + ws):
    assert tuple(dw.shape) == (w.numel(),)                              # the caller's length and order
  if combiner != "sum":
    for dw, w in zip(got[len(vs):], ws):
      assert not bool(bits(torch, dw[~(w > 0)]).any()) and bool(dw.any())   # what the safe form pruned: exactly 0
  for v in vs:
    v._tables[0]._table.check_errors()


def test_a_member_of_another_route_is_served_by_its_own_weights_grad(env, side, c_names):
  torch, de = env
  vs, keys, absent, two = side
  rng = np.random.default_rng(227)
  members = [vs[0], two, vs[2], vs[1]]
  batches = [_sparse_batch(torch, rng, keys, absent) for _ in members]
  n = batches[0][4]
  res = de.safe_embedding_lookup_sparse_many(members, [(b[0], b[1]) for b in batches], [b[2] for b in batches], combiner="mean",
                                             return_trainable=True, num_rows=n)
  wrappers = [tw for _, tw in res]
  assert wrappers[1]._pooled_ids is None                                # two shards: not behind the pooled forward
  pairs = list(zip(_grads(torch, rng, wrappers), wrappers))
  del c_names[:]
  got = de.sparse_weights_grad_many(pairs)
  seen = [x for x in c_names if "backprop_weights" in x]
  assert sorted(seen) == sorted([GROUPED, "tfra_sparse_segment_combine_backprop_weights"]), seen   # three grouped, one on its own route
  _same(torch, got, [tw.weights_grad(g) for g, tw in pairs])
  assert bool(got[1].any())


def test_a_wrapper_without_weights_or_with_max_norm_refuses_the_list(env, side, c_names):
  torch, de = env
  vs, keys, absent, _ = side
  rng = np.random.default_rng(229)
  batches = [_sparse_batch(torch, rng, keys, absent) for _ in vs]
  n = batches[0][4]
  tup, ws = [(b[0], b[1]) for b in batches], [b[2].abs() + 0.1 for b in batches]
  good = [tw for _, tw in de.embedding_lookup_sparse_many(vs, tup, ws, combiner="mean", return_trainable=True, num_rows=n)]
  _, unweighted = de.embedding_lookup_sparse(vs[2], tup[2], None, combiner="mean", return_trainable=True, num_rows=n)
  _, clipped = de.embedding_lookup_sparse(vs[2], tup[2], ws[2], combiner="mean", max_norm=1.0, return_trainable=True, num_rows=n)
  grads = _grads(torch, rng, good)
  for bad, match in ((unweighted, "sp_weights"), (clipped, "max_norm")):
    with pytest.raises(ValueError, match=match):
      bad.weights_grad(grads[2])                                        # weights_grad's own refusal
    del c_names[:]
    with pytest.raises(ValueError, match=match):
      de.sparse_weights_grad_many([(grads[0], good[0]), (grads[1], good[1]), (grads[2], bad)])
    assert c_names == []                                                # nothing was enqueued for the members in front of it
  del c_names[:]
  with pytest.raises(ValueError, match="shape of its result"):
    de.sparse_weights_grad_many([(grads[0], good[0]), (grads[1][:-1], good[1])])
  assert c_names == []
