"""GPU: a tiered shard trained through its planned admitting lookup trains like a roomy one.

tests/test_gpu_tier_variable.py::test_trains_like_a_roomy_twin, with the lookup of every step going through the batch's write-back
plan on BOTH sides: `TieredHashTable.find_or_insert_planned` (tfra_tier_find_or_insert_planned) on the tiered variable's shard,
`CuckooHashTable.find_or_insert_planned` on the twin's, and the write-back of both with that same plan
(`DynamicEmbeddingOptimizer.apply_sparse(plan=...)`).  Row p of the one initializer draw belongs to batch position p on both sides,
so a never-seen id enters both with the same row; at the end the embedding AND the optimizer slots of every key ever seen are bit
for bit the twin's.

The loop drives the TABLE layer, not `embedding_lookup`: the variable layer keeps tiered shards on the init_on_lookup=True route.
DESIGN 4.26's decision rule routes them to the planned call only if a training step under "plan" is below one under True by more
than the sum of both spreads at the 10 % mix, and the measurement (profiles/tier_planned_mb.jsonl) did not say so.  The steps below
are what `TrainableWrapper._lookup_admitting` and `apply_gradients` do for a plain table under init_on_lookup="plan".  The second
case pins the variable's side of that decision: a tiered variable with "plan" does what it does with True."""
import numpy as np
import pytest

from tests import probe_model as pm
from tests.sparse_helpers import Calls
from tests.test_gpu_tier_variable import CAP, DIM, _batches, _Init, _whole_rows

pytestmark = pytest.mark.gpu

NAME = "tfra_tier_find_or_insert_planned"


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _var(env, name, opt, creator, init_on_lookup):
  torch, de = env
  return de.Variable(dim=DIM, name=name, initializer=_Init(torch), kv_creator=creator, init_on_lookup=init_on_lookup,
                     **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))


def _tiered_creator(de, max_batch=1024):
  return de.TieredHashTableCreator(de.TieredHashTableConfig(
      upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=max_batch))


def _delta(calls, before):
  return {k: v - before.get(k, 0) for k, v in calls.n.items() if v != before.get(k, 0)}


@pytest.mark.parametrize("opt_name", ["adam", "adagrad"])
def test_planned_steps_train_like_a_roomy_twin(env, monkeypatch, opt_name):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  mk_opt = {"adam": lambda: de.optimizers.Adam(1e-2), "adagrad": lambda: de.optimizers.Adagrad(1e-1)}[opt_name]
  pair = []
  for kind, creator in (("tiered", _tiered_creator(de)), ("twin", de.CuckooHashTableCreator())):
    opt = mk_opt()
    var = _var(env, "tpv_%s_%s" % (opt_name, kind), opt, creator, "plan")
    pair.append((var, de.DynamicEmbeddingOptimizer(opt), SparsePlan(var._tables[0]._device, DIM)))
  tiered, twin = pair[0][0], pair[1][0]
  ids, grads = _batches(23)
  calls = Calls(monkeypatch)
  seen = set()
  for step, (i_np, g_np) in enumerate(zip(ids, grads)):
    b0, b1, _ = pm.homes(np.unique(i_np), 89)
    load = np.bincount(np.concatenate([b0, b1]), minlength=89)
    assert not bool(((load[b0] >= 15) & (load[b1] >= 15)).any())     # no batch saturates its own home buckets (a CPU precondition)
    kt, gt = torch.from_numpy(i_np).cuda(), torch.from_numpy(g_np).cuda()
    embs = []
    for k, (var, deo, plan) in enumerate(pair):
      t = var._tables[0]
      c0 = dict(calls.n)
      plan.build(kt)
      emb = t.find_or_insert_planned(plan, dynamic_default_values=var._create_default_values_by_initializer(kt.numel(), t._device))
      embs.append(emb)
      lookup = _delta(calls, c0)
      c0 = dict(calls.n)
      deo.apply_sparse(var, kt, gt, plan=plan)
      wb = _delta(calls, c0)
      if k == 0:      # the tiered shard: one planned admission, one de-duplication
        assert lookup == {"tfra_sparse_plan_build": 1, NAME: 1}, lookup
        assert wb.get("tfra_table_apply_planned") == 1 and "tfra_sparse_plan_build" not in wb and "tfra_table_apply_sparse" not in wb, wb
        assert not [c for c in list(lookup) + list(wb) if c.startswith("tfra_unique")], (lookup, wb)
    assert torch.equal(embs[0], embs[1]), "step %d: the tiered lookup returned other rows than the twin's" % step
    seen.update(i_np.tolist())
  seen = torch.from_numpy(np.fromiter(seen, np.int64, len(seen))).cuda()
  t = tiered._tables[0]
  t._table.check_errors()
  t._lower.check_errors()
  assert seen.numel() > CAP and t._table.size_host() <= t._table.capacity()
  s = t._tier.stats()
  assert s["calls"] == len(ids) and s["demoted"] > 0 and s["lower_hits"] > 100          # keys went down and came up again
  a, b = _whole_rows(torch, tiered, seen), _whole_rows(torch, twin, seen)
  assert a.shape == b.shape == (seen.numel(), DIM * (1 + tiered.aux_fields))
  bad = (a.view(torch.int32) != b.view(torch.int32)).any(1)
  assert not bool(bad.any()), "%d of %d keys differ from the twin (embedding or slots)" % (int(bad.sum()), seen.numel())
  assert int(tiered.size()) == int(twin.size()) == seen.numel()
  assert torch.equal(tiered.lookup(seen), twin.lookup(seen))
  k, v = tiered.export()
  o = torch.argsort(k)
  assert torch.equal(k[o], torch.sort(seen)[0]) and torch.equal(v[o], a[torch.argsort(seen), :DIM])


@pytest.mark.parametrize("max_batch", [1024, 256], ids=["within-max_batch", "beyond-max_batch"])
def test_a_tiered_variable_keeps_the_true_route_under_plan(env, monkeypatch, max_batch):
  """embedding_lookup(return_trainable=True) of a tiered variable with init_on_lookup="plan" does for a batch — within the tier's
  max_batch or beyond it — whatever init_on_lookup=True does for it: the same calls, and the same rows or the same refusal."""
  torch, de = env
  ids, _ = _batches(31)
  kt = torch.from_numpy(ids[0]).cuda()
  assert (kt.numel() <= max_batch) == (max_batch == 1024)
  calls = Calls(monkeypatch)
  outcomes = []
  for setting in (True, "plan"):
    var = _var(env, "tpv_route_%d_%s" % (max_batch, setting), de.optimizers.Adam(1e-2), _tiered_creator(de, max_batch=max_batch), setting)
    c0 = dict(calls.n)
    try:
      emb, _ = de.embedding_lookup(var, kt, return_trainable=True)
      got = ("rows", emb.clone())
    except Exception as e:      # (whatever the True route answers such a batch with)
      got = (type(e), str(e))
    d = _delta(calls, c0)      # the calls of a lookup's route (a workspace is created once per process, whoever comes first)
    route = {k: v for k, v in d.items() if k.startswith(("tfra_unique", "tfra_tier_", "tfra_gather_rows", "tfra_sparse_plan", "tfra_table_find"))}
    outcomes.append(got + (int(var.size()), route))
  (ka, xa, sa, da), (kb, xb, sb, db) = outcomes
  assert ka == kb and sa == sb and da == db and NAME not in da and da.get("tfra_tier_find_or_insert") == 1, (da, db)      # (a refused call counts too)
  assert torch.equal(xa, xb) if ka == "rows" else xa == xb
  assert (ka == "rows") == (max_batch == 1024)
