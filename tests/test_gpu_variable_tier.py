"""GPU: Variable.lookup_missed / assign / contains over 1, 2 and 3 shards (all on one device) give what one shard gives: the same
rows, the same set of (key, batch position) pairs, the same flags; the positions index the caller's batch whatever the partition."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N = 8, 1000


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _rows(torch, keys, ver):
  return ((keys[:, None] % 251).to(torch.float32) + torch.arange(DIM, device=keys.device)[None, :] * 0.25 + ver).contiguous()


def _draw(shape):          # a callable initializer whose rows all look alike: the defaults are drawn per shard
  import torch
  return torch.full(tuple(shape), 0.75)


def _parity_partitioner(keys, shard_num):
  import torch
  return ((keys // 7) % shard_num).to(torch.int32)


def _run(env, shards, partitioner=None, initializer=0.5):
  torch, de = env
  kw = {} if partitioner is None else {"partitioner": partitioner}
  var = de.Variable(dim=DIM, devices=["cuda:0"] * shards, initializer=initializer, name="vt_%d_%s_%s" % (shards, partitioner is not None, callable(initializer)),
                    init_size=4096, **kw)
  rng = np.random.default_rng(9)
  pool = np.unique(rng.integers(-2**40, 2**40, size=2 * N + 20, dtype=np.int64))
  rng.shuffle(pool)
  res, absent = torch.from_numpy(pool[:N]).cuda(), torch.from_numpy(pool[N:2 * N]).cuda()
  var.upsert(res, _rows(torch, res, 1))
  size = [int(var.size(i)) for i in range(shards)]
  # a batch with repeats: half resident
  look = torch.cat([res[:400], absent[:300], res[:100], absent[:50]])[torch.from_numpy(rng.permutation(850)).cuda()]
  rows, mk, mp, ex = var.lookup_missed(look, return_exists=True)
  # unique keys for assign
  uniq = torch.cat([res[300:700], absent[100:400]])[torch.from_numpy(rng.permutation(700)).cuda()]
  found = var.assign(uniq, _rows(torch, uniq, 2), return_found=True)
  assert var.assign(uniq, _rows(torch, uniq, 2)) is None
  assert [int(var.size(i)) for i in range(shards)] == size and sum(size) == N     # assign never changes size()
  after, ex_after = var.lookup(torch.cat([res, absent]), return_exists=True)
  return dict(look=look, rows=rows, pairs=sorted(zip(mk.tolist(), mp.tolist())), mk=mk, mp=mp, ex=ex, contains=var.contains(look),
              found=found, uniq=uniq, after=after, ex_after=ex_after, res=res)


_ONE = {}


def _one(env, initializer):
  key = callable(initializer)
  if key not in _ONE:
    _ONE[key] = _run(env, 1, initializer=initializer)
  return _ONE[key]


def _same(torch, a, b):
  assert torch.equal(a["look"], b["look"])
  for f in ("rows", "ex", "contains", "found", "after", "ex_after"):
    assert torch.equal(a[f], b[f]), f
  assert a["pairs"] == b["pairs"]


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_shards_give_the_one_shard_results(env, shards):
  torch, _ = env
  one, r = _one(env, 0.5), _run(env, shards)
  _same(torch, one, r)
  # the positions index the caller's batch; the list is exactly the positions lookup reports as absent
  assert torch.equal(r["mk"], r["look"][r["mp"]])
  assert sorted(r["mp"].tolist()) == torch.nonzero(~r["ex"]).reshape(-1).tolist()
  assert torch.equal(r["contains"], r["ex"]) and int(r["ex"].sum()) == 500
  hit = torch.from_numpy(np.isin(r["uniq"].cpu().numpy(), r["res"].cpu().numpy())).cuda()
  assert torch.equal(r["found"], hit) and int(hit.sum()) == 400
  assert torch.equal(r["rows"][~r["ex"]], torch.full((350, DIM), 0.5, device="cuda"))
  assert int(r["ex_after"].sum()) == N             # nothing was admitted


def test_custom_partitioner(env):
  torch, _ = env
  _same(torch, _one(env, 0.5), _run(env, 3, partitioner=_parity_partitioner))


def test_callable_initializer_draws_per_shard(env):
  torch, _ = env
  one, r = _one(env, _draw), _run(env, 2, initializer=_draw)
  _same(torch, one, r)
  assert torch.equal(r["rows"][~r["ex"]], torch.full((350, DIM), 0.75, device="cuda"))
