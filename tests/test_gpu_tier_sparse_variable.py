"""GPU: the sparse lookups of a Variable over TieredHashTableCreator — embedding_lookup_sparse, safe_embedding_lookup_sparse, the
ragged forms and the grouped forms — read BOTH tiers, and a training step through them admits its entry ids first, so that
apply_combined_gradients only hits.

The tiered variable (dim 8, a static default row, a cache of 15 * 89 slots) stands beside a twin over CuckooHashTableCreator that
holds everything.  Serving: every form returns the twin's bits for batches full of demoted keys.  Training: both see the same
batches and gradients; every step's forward is the twin's, and at the end the embedding AND the optimizer slots of every key ever
seen are bit for bit the twin's."""
import numpy as np
import pytest

from tests import probe_model as pm

pytestmark = pytest.mark.gpu

DIM, CAP, UNIVERSE, BATCH, STEPS, MAX_BATCH = 8, 15 * 89, 3000, 300, 12, 1024
DEFAULT = 0.25


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _cfg(de):
  return de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU),
                                  max_batch=MAX_BATCH)


# ---- serving ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served(env):
  """(tiered, twin, keys, absent): both variables hold the same 3000 rows; most of the tiered one's are only below"""
  torch, de = env
  rng = np.random.default_rng(41)
  pool = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 300, dtype=np.int64))
  rng.shuffle(pool)
  keys, absent = pool[:UNIVERSE], pool[UNIVERSE:UNIVERSE + 100]
  rows = rng.standard_normal((UNIVERSE, DIM)).astype(np.float32)
  tiered = de.Variable(dim=DIM, name="tsv_serve_tiered", initializer=DEFAULT, kv_creator=de.TieredHashTableCreator(_cfg(de)))
  twin = de.Variable(dim=DIM, name="tsv_serve_twin", initializer=DEFAULT, kv_creator=de.CuckooHashTableCreator())
  for var in (tiered, twin):
    var.upsert(torch.from_numpy(keys).cuda(), torch.from_numpy(rows).cuda())
  assert tiered.can_lookup_combined() and twin.can_lookup_combined()
  return tiered, twin, keys, absent


def _sparse_batch(torch, rng, keys, absent, n_rows=120):
  counts = rng.integers(0, 9, size=n_rows)
  counts[[0, 7, n_rows - 1]] = 0
  counts[3] = 20
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = np.where(rng.random(seg.size) < 0.9, rng.choice(keys, seg.size), rng.choice(absent, seg.size))
  w = rng.standard_normal(seg.size).astype(np.float32)      # a third of the weights prune under the safe form
  w[seg == 5] = -1.0
  splits = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  return tuple(torch.from_numpy(x).cuda() for x in (seg, ids, w, splits)) + (n_rows,)


def _demoted(torch, tiered, ids):
  t = tiered._tables[0]
  return int((~t._table.contains(ids) & t._lower.contains(ids)).sum())


def test_serving_forms_read_both_tiers(env, served):
  torch, de = env
  rag = de.ragged_embedding_ops
  tiered, twin, keys, absent = served
  rng = np.random.default_rng(43)
  seg, ids, w, splits, n = _sparse_batch(torch, rng, keys, absent)
  assert _demoted(torch, tiered, ids) > 100                        # the batch is full of keys that are only below
  t = tiered._tables[0]
  below_only = keys[(~t._table.contains(torch.from_numpy(keys).cuda())).cpu().numpy()]
  stats = t._tier.stats()
  both = lambda f: (f(tiered), f(twin))
  for combiner in ("sum", "mean", "sqrtn"):
    for wt in (None, w):
      a, b = both(lambda v: de.embedding_lookup_sparse(v, (seg, ids), wt, combiner=combiner, num_rows=n))
      assert torch.equal(a, b), (combiner, wt is None)
      a, b = both(lambda v: rag.embedding_lookup_sparse(v, (splits, ids), wt, combiner=combiner))
      assert torch.equal(a, b), (combiner, wt is None)
      a, b = both(lambda v: de.safe_embedding_lookup_sparse(v, (seg, ids), wt, combiner=combiner, num_rows=n))
      assert torch.equal(a, b), (combiner, wt is None)
      a, b = both(lambda v: rag.safe_embedding_lookup_sparse(v, (splits, ids), wt, combiner=combiner))
      assert torch.equal(a, b), (combiner, wt is None)
  assert t._tier.stats() == stats                                  # reads: nothing moved, nothing was counted
  assert _demoted(torch, tiered, ids) > 100
  # the safe forms with a default_id that is only below (the ragged form reads it inside its launch)
  for combiner in ("mean", "sum"):
    d = int(below_only[7])
    a, b = both(lambda v: rag.safe_embedding_lookup_sparse(v, (splits, ids), w, combiner=combiner, default_id=d))
    assert torch.equal(a, b) and bool(a[0].any()) and not torch.equal(a[0], torch.full((DIM,), DEFAULT, device="cuda"))
    a, b = both(lambda v: de.safe_embedding_lookup_sparse(v, (seg, ids), w, combiner=combiner, default_id=d, num_rows=n))
    assert torch.equal(a, b) and bool(a[0].any())
  t._table.check_errors()
  t._lower.check_errors()


def test_a_tiered_variable_in_the_grouped_forms(env, served):
  torch, de = env
  rag = de.ragged_embedding_ops
  tiered, _, keys, absent = served
  rng = np.random.default_rng(47)
  plain = []
  for i in range(2):
    var = de.Variable(dim=DIM * (i + 1), name="tsv_many_plain%d" % i, initializer=0.5)
    var.upsert(torch.from_numpy(keys[:500]).cuda(), torch.from_numpy(rng.standard_normal((500, DIM * (i + 1))).astype(np.float32)).cuda())
    plain.append(var)
  variables = [plain[0], tiered, plain[1]]
  batches = [_sparse_batch(torch, rng, keys, absent) for _ in variables]
  assert _demoted(torch, tiered, batches[1][1]) > 100
  n = batches[0][4]
  singles = [de.embedding_lookup_sparse(v, (b[0], b[1]), b[2], combiner="mean", num_rows=n) for v, b in zip(variables, batches)]
  many = de.embedding_lookup_sparse_many(variables, [(b[0], b[1]) for b in batches], [b[2] for b in batches], combiner="mean", num_rows=n)
  assert all(torch.equal(a, b) for a, b in zip(singles, many))
  singles = [de.safe_embedding_lookup_sparse(v, (b[0], b[1]), b[2], combiner="mean", num_rows=n) for v, b in zip(variables, batches)]
  many = de.safe_embedding_lookup_sparse_many(variables, [(b[0], b[1]) for b in batches], [b[2] for b in batches], combiner="mean", num_rows=n)
  assert all(torch.equal(a, b) for a, b in zip(singles, many))
  singles = [rag.embedding_lookup_sparse(v, (b[3], b[1]), b[2], combiner="sqrtn") for v, b in zip(variables, batches)]
  many = rag.embedding_lookup_sparse_many(variables, [(b[3], b[1]) for b in batches], [b[2] for b in batches], combiner="sqrtn")
  assert all(torch.equal(a, b) for a, b in zip(singles, many))
  singles = [rag.safe_embedding_lookup_sparse(v, (b[3], b[1]), b[2], combiner="mean") for v, b in zip(variables, batches)]
  many = rag.safe_embedding_lookup_sparse_many(variables, [(b[3], b[1]) for b in batches], [b[2] for b in batches], combiner="mean")
  assert all(torch.equal(a, b) for a, b in zip(singles, many))


# ---- training --------------------------------------------------------------------------------------------------------------------
def _batches(seed):
  """per step: entry ids (300, repeating), their rows (1 to 8 entries each, ascending), weights, the gradient of the result"""
  rng = np.random.default_rng(seed)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 50, dtype=np.int64))[:UNIVERSE]
  out = []
  for _ in range(STEPS):
    counts = []
    while sum(counts) < BATCH:
      counts.append(min(int(rng.integers(1, 9)), BATCH - sum(counts)))
    seg = np.repeat(np.arange(len(counts)), counts).astype(np.int64)
    ids = rng.choice(universe, size=BATCH, replace=True)
    w = rng.uniform(0.1, 2.0, size=BATCH).astype(np.float32)
    g = rng.standard_normal((len(counts), DIM)).astype(np.float32) * np.float32(0.1)
    out.append((ids, seg, w, g))
  return universe, out


def _pair(env, opt_name, tag):
  torch, de = env
  mk_opt = {"adam": lambda: de.optimizers.Adam(1e-2), "adagrad": lambda: de.optimizers.Adagrad(1e-1)}[opt_name]
  out = []
  for kind, creator in (("tiered", de.TieredHashTableCreator(_cfg(de))), ("twin", de.CuckooHashTableCreator())):
    opt = mk_opt()
    var = de.Variable(dim=DIM, name="tsv_%s_%s_%s" % (tag, opt_name, kind), initializer=DEFAULT, kv_creator=creator,
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    out.append((var, de.DynamicEmbeddingOptimizer(opt)))
  return out


def _whole_rows(torch, var, keys):
  """[n, (1 + aux) * DIM]: embedding and slots of `keys`; a tiered variable is read through flush() plus its lower table"""
  t = var._tables[0]
  if hasattr(t, "flush"):
    t.flush()
    table = t._lower
  else:
    table = t._table
  assert bool(table.contains(keys).all())
  return torch.cat([table.find(keys, field=f) for f in range(var.aux_fields + 1)], dim=1)


def _no_saturation(entry_ids):
  b0, b1, _ = pm.homes(np.unique(entry_ids), 89)
  load = np.bincount(np.concatenate([b0, b1]), minlength=89)
  assert not bool(((load[b0] >= 15) & (load[b1] >= 15)).any())     # no batch saturates its own home buckets (a CPU precondition)


@pytest.mark.parametrize("opt_name", ["adam", "adagrad"])
def test_sparse_training_matches_a_roomy_twin(env, opt_name):
  torch, de = env
  universe, steps = _batches(54)
  pair = _pair(env, opt_name, "train")
  (tiered, _), (twin, _) = pair
  t = tiered._tables[0]
  seen = set()
  for step, (ids, seg, w, g) in enumerate(steps):
    _no_saturation(ids)
    it, st, wt, gt = (torch.from_numpy(x).cuda() for x in (ids, seg, w, g))
    combiner = ("mean", "sum", "sqrtn")[step % 3]
    outs, dws = [], []
    for var, deo in pair:
      out, tw = de.embedding_lookup_sparse(var, (st, it), wt, combiner=combiner, return_trainable=True, num_rows=g.shape[0])
      outs.append(out)
      if step % 4 == 1:
        dws.append(tw.weights_grad(gt))
      deo.apply_combined_gradients([(gt, tw)])
    assert torch.equal(outs[0], outs[1]), "step %d: the tiered forward is not the twin's" % step
    if dws:
      assert torch.equal(dws[0], dws[1]), "step %d: weights_grad" % step
    seen.update(ids.tolist())
  s = t._tier.stats()
  assert s["demoted"] > 0 and s["lower_hits"] > 100                # keys went down and came up again
  # one step through the safe form: rows without entries, and a default_id that is only below
  seen_t = torch.from_numpy(np.fromiter(seen, np.int64, len(seen))).cuda()
  only_below = seen_t[~t._table.contains(seen_t)]
  assert only_below.numel() > 100
  default_id = int(only_below[3])
  rng = np.random.default_rng(59)
  n_rows = 60
  counts = rng.integers(0, 7, size=n_rows)
  counts[[0, 9, n_rows - 1]] = 0
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = rng.choice(universe, size=seg.size, replace=True)
  w = rng.standard_normal(seg.size).astype(np.float32)            # weights <= 0 prune
  g = rng.standard_normal((n_rows, DIM)).astype(np.float32) * np.float32(0.1)
  _no_saturation(np.concatenate([ids, [default_id]]))
  it, st, wt, gt = (torch.from_numpy(x).cuda() for x in (ids, seg, w, g))
  outs, dws = [], []
  for var, deo in pair:
    out, tw = de.safe_embedding_lookup_sparse(var, (st, it), wt, combiner="mean", default_id=default_id, return_trainable=True,
                                              num_rows=n_rows)
    outs.append(out)
    dws.append(tw.weights_grad(gt))
    deo.apply_combined_gradients([(gt, tw)])
  assert torch.equal(outs[0], outs[1]) and torch.equal(dws[0], dws[1])
  assert not torch.equal(outs[0][0], torch.full((DIM,), DEFAULT, device="cuda"))      # the trained row of default_id, from below
  seen.update(ids[w > 0].tolist() + [default_id])
  # the end state: whole rows, size, no dropped key
  seen_t = torch.from_numpy(np.fromiter(seen, np.int64, len(seen))).cuda()
  t._table.check_errors()
  t._lower.check_errors()
  assert seen_t.numel() > CAP and t._table.size_host() <= t._table.capacity()
  a, b = _whole_rows(torch, tiered, seen_t), _whole_rows(torch, twin, seen_t)
  assert a.shape == b.shape == (seen_t.numel(), DIM * (1 + tiered.aux_fields))
  bad = (a.view(torch.int32) != b.view(torch.int32)).any(1)
  assert not bool(bad.any()), "%d of %d keys differ from the twin (embedding or slots)" % (int(bad.sum()), seen_t.numel())
  assert int(tiered.size()) == int(twin.size()) == seen_t.numel()


def test_the_ragged_training_forms_admit_too(env):
  torch, de = env
  rag = de.ragged_embedding_ops
  universe, steps = _batches(61)
  pair = _pair(env, "adam", "ragged")
  (tiered, _), (twin, _) = pair
  t = tiered._tables[0]
  fill = torch.from_numpy(universe).cuda()
  for var, _ in pair:                                                  # start from a full cache: most keys are only below
    var.upsert(fill, torch.from_numpy(np.random.default_rng(67).standard_normal((UNIVERSE, DIM)).astype(np.float32)).cuda())
  seen = set()
  for step, (ids, seg, w, g) in enumerate(steps[:4]):
    _no_saturation(ids)
    splits = np.concatenate([[0], np.cumsum(np.bincount(seg))]).astype(np.int64)
    it, rt, wt, gt = (torch.from_numpy(x).cuda() for x in (ids, splits, w, g))
    assert int((~t._table.contains(it)).sum()) > 100
    outs = []
    for var, deo in pair:
      form = rag.safe_embedding_lookup_sparse if step % 2 else rag.embedding_lookup_sparse
      out, tw = form(var, (rt, it), wt, combiner="mean", return_trainable=True)
      outs.append(out)
      deo.apply_combined_gradients([(gt, tw)])
    assert torch.equal(outs[0], outs[1]), "step %d" % step
    assert bool(t._table.contains(it).all())
    seen.update(ids.tolist())
  seen_t = torch.from_numpy(np.fromiter(seen, np.int64, len(seen))).cuda()
  a, b = _whole_rows(torch, tiered, seen_t), _whole_rows(torch, twin, seen_t)
  assert torch.equal(a.view(torch.int32), b.view(torch.int32))
  t._table.check_errors()
  t._lower.check_errors()


def test_more_entry_ids_than_max_batch_are_refused(env):
  torch, de = env
  (tiered, _), _ = _pair(env, "adam", "big")
  n = MAX_BATCH + 1
  ids = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
  seg = torch.arange(n, dtype=torch.int64, device="cuda") // 4
  with pytest.raises(ValueError, match="max_batch"):
    de.embedding_lookup_sparse(tiered, (seg, ids), None, combiner="sum", return_trainable=True, num_rows=int(seg[-1]) + 1)
  out = de.embedding_lookup_sparse(tiered, (seg, ids), None, combiner="sum", num_rows=int(seg[-1]) + 1)   # serving is not limited
  assert tuple(out.shape) == (int(seg[-1]) + 1, DIM) and int(tiered.size()) == 0
