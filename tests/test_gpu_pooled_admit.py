"""GPU: Variable(init_on_lookup="pooled") — the training forms of the sparse lookups of a variable with a callable initializer admit
their entry ids first (unique on the device, ONE draw initializer([n_entry_ids, dim]), `admit`: find_or_insert with no rows handed
back) and then read once through the pooled kernels, where init_on_lookup=True runs the chain (unique with a host read of the count,
find_or_insert returning [U, dim] rows, the segment combine).

The initializer is deterministic and counts its calls: row j of call c is ((j % 61) * 8 + column) / 64 + c — exact in float16, a
function of j and c only — so a "pooled" variable (row j of [n_entry_ids, dim] for unique id j) and its True twin (row j of [U, dim])
admit the same row for the same id as long as both make the same number of draws, which every step here keeps.  Every batch has 200
to 300 entry ids over rows of 1 to 8 entries, never-seen ids and repeats in every step; its first entry is the id the safe form uses
as default_id, so the order of first occurrences is the same among the looked-up ids (what the chain admits) and the entry ids (what
the pooled route admits).  Everything is compared bit for bit: every step's result, and embedding, m and v at the end."""
import numpy as np
import pytest

from tests import probe_model as pm
from tests.sparse_helpers import Calls, _export_state, bits
from tests.test_gpu_init_on_lookup import _HostReads

pytestmark = pytest.mark.gpu

DIM, STEPS, UNIVERSE, DEFAULT_ID = 8, 4, 600, 424242
CAP, NB = 15 * 89, 89


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _initializer(torch, shapes):
  def draw(shape):
    c = len(shapes)
    shapes.append(tuple(int(x) for x in shape))
    n, dim = shapes[-1]
    j = torch.arange(n, device="cuda", dtype=torch.float32) % 61
    return (j[:, None] * 8 + torch.arange(dim, device="cuda", dtype=torch.float32)[None, :]) / 64 + float(c)
  return draw


def _opt(de, kind):
  return de.optimizers.SGD(0.05) if kind == "sgd" else de.optimizers.Adam(0.01)


def _var(env, name, opt, init_on_lookup, dt="float32", creator=None, static=False, **kw):
  torch, de = env
  shapes = []
  devices = kw.pop("devices", ["cuda:0"])
  var = de.Variable(key_dtype=torch.int64, value_dtype=getattr(torch, dt), dim=DIM, devices=devices, name=name,
                    initializer=0.25 if static else _initializer(torch, shapes), init_on_lookup=init_on_lookup, kv_creator=creator,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt), **kw)
  var._shapes = shapes
  return var


def _universe(seed):
  """the ids a seed's batches draw from (the first thing its generator makes)"""
  return np.unique(np.random.default_rng(seed).integers(1, 2**40, size=UNIVERSE + 20, dtype=np.int64))[:UNIVERSE]


def _batches(seed, steps=STEPS):
  """per step: (ids, seg, weights, row_splits, n_rows, grad): 200 to 300 entries, rows of 1 to 8 and a few empty rows (never row 0),
  some weights <= 0; ids[0] is DEFAULT_ID with a positive weight; a sixth of the positions are ids never seen before the step"""
  rng = np.random.default_rng(seed)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 20, dtype=np.int64))[:UNIVERSE]
  out, fresh_at = [], 0
  for s in range(steps):
    total = int(rng.integers(200, 301))
    counts = []
    while sum(counts) < total:
      if counts and rng.random() < 0.05:
        counts.append(0)                                        # an empty row
      counts.append(min(int(rng.integers(1, 9)), total - sum(counts)))
    counts = np.array(counts)
    n_rows = counts.size
    seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
    n_new = total // 6
    new = universe[300 + fresh_at:300 + fresh_at + n_new // 2]   # never seen before this step, each at least once, some twice
    fresh_at += new.size
    ids = np.concatenate([rng.choice(universe[:300 + fresh_at - new.size], size=total - n_new), new, rng.choice(new, size=n_new - new.size)])
    rng.shuffle(ids)
    ids[0] = DEFAULT_ID
    w = rng.uniform(0.1, 2.0, size=total).astype(np.float32)
    w[rng.choice(np.arange(1, total), size=total // 12, replace=False)] = np.float32(-0.5)
    splits = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    g = (rng.integers(-64, 65, size=(n_rows, DIM)) / 64.0).astype(np.float32)
    uniq = np.unique(ids)
    b0, b1, _ = pm.homes(uniq, NB)                               # (a tier's cache: no batch saturates its own home buckets)
    load = np.bincount(np.concatenate([b0, b1]), minlength=NB)
    assert not bool(((load[b0] >= 15) & (load[b1] >= 15)).any())
    out.append((ids, seg, w, splits, n_rows, g))
  return out


def _dev(torch, b):
  ids, seg, w, splits, n_rows, g = b
  t = lambda x: torch.from_numpy(x).cuda()
  return t(ids), t(seg), t(w), t(splits), n_rows, t(g)


def _lookup(env, form, var, b):
  """the training lookup of one form -> (result, wrapper)"""
  torch, de = env
  ids, seg, w, splits, n_rows, _ = b
  if form == "tuple":
    return de.embedding_lookup_sparse(var, (seg, ids), w.abs(), combiner="sqrtn", return_trainable=True, num_rows=n_rows)
  if form == "safe":
    return de.safe_embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", default_id=DEFAULT_ID, return_trainable=True, num_rows=n_rows)
  return de.ragged_embedding_ops.embedding_lookup_sparse(var, (splits, ids), w.abs(), combiner="sum", return_trainable=True)


def _lookup_many(env, form, vs, bs):
  torch, de = env
  if form == "tuple":
    return de.embedding_lookup_sparse_many(vs, [(b[1], b[0]) for b in bs], [b[2].abs() for b in bs], combiner="sqrtn", return_trainable=True,
                                           num_rows=[b[4] for b in bs])
  if form == "safe":
    return de.safe_embedding_lookup_sparse_many(vs, [(b[1], b[0]) for b in bs], [b[2] for b in bs], combiner="mean", default_id=DEFAULT_ID,
                                                return_trainable=True, num_rows=[b[4] for b in bs])
  return de.ragged_embedding_ops.embedding_lookup_sparse_many(vs, [(b[3], b[0]) for b in bs], [b[2].abs() for b in bs], combiner="sum",
                                                              return_trainable=True)


def _same_state(torch, de, deo_a, deo_b, opt, a, b, tag):
  sa, sb = _export_state(torch, de, deo_a, opt, a), _export_state(torch, de, deo_b, opt, b)
  assert len(sa) == len(sb) == 2 + len(opt.slots)
  for i, (x, y) in enumerate(zip(sa, sb)):
    assert x.shape == y.shape and torch.equal(x, y), "%s: part %d of (keys, embedding, slots) differs from the twin" % (tag, i)


def _entry_ids(form, b):
  """the ids the step's write-back touches: the looked-up ids; the safe form prunes by weight and adds default_id per empty row"""
  ids, seg, w, splits, n_rows, _ = b
  if form != "safe":
    return ids.size
  kept = w > 0
  return int(kept.sum()) + (n_rows - np.unique(seg[kept]).size)


# ---- 1. one variable, against the chain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,dt", [("tuple", "adam", "float32"), ("tuple", "sgd", "float16"), ("safe", "adam", "float32"),
                                          ("safe", "sgd", "float32"), ("ragged", "adam", "float16"), ("ragged", "sgd", "float32")])
def test_a_pooled_variable_trains_as_its_true_twin(env, monkeypatch, form, kind, dt):
  torch, de = env
  opt = _opt(de, kind)
  tag = "%s_%s_%s" % (form, kind, dt)
  P, T = _var(env, "pa_p_" + tag, opt, "pooled", dt), _var(env, "pa_t_" + tag, opt, True, dt)
  assert P.init_on_lookup == "pooled" and P.can_admit_pooled() and not P.can_lookup_combined() and P.admits_on_lookup() and P.misses_are_static()
  deo_p, deo_t = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  calls, reads = Calls(monkeypatch), _HostReads(torch, monkeypatch)
  table = P._tables[0]._table
  read_name = "tfra_table_find_combine_ragged" if form == "ragged" else "tfra_table_find_combine"
  route = {read_name: 0, "tfra_table_find_or_insert": 0, "tfra_unique": 0}
  batches = _batches(7)
  for step, nb in enumerate(batches):
    b = _dev(torch, nb)
    draws0, reads0, calls0 = len(P._shapes), reads.n, dict(calls.n)
    out_p, tw_p = _lookup(env, form, P, b)
    reads_in_lookup = reads.n - reads0
    for name in route:
      route[name] += calls[name] - calls0.get(name, 0)
    assert calls["tfra_sparse_segment_combine"] == calls0.get("tfra_sparse_segment_combine", 0), "the pooled route ran the chain's combine"
    # ONE draw of [n_entry_ids, dim] in the lookup (the safe form then reads default_id's row: its own draw of one row)
    assert P._shapes[draws0] == (_entry_ids(form, nb), DIM), (P._shapes[draws0:], _entry_ids(form, nb))
    assert len(P._shapes) - draws0 == (2 if form == "safe" else 1)
    if form in ("tuple", "ragged"):
      assert reads_in_lookup == 0, "the pooled training lookup read a tensor on the host"
    # residency, before the write-back: every entry id is in the table, with the row the forward combined
    uniq, idx, _ = de.device_ops.unique(tw_p.entry_ids)
    assert bool(table.contains(uniq).all())
    if form != "safe":
      ref = de.device_ops.sparse_segment_combine(table.find(uniq), idx, b[1], b[2].abs(), tw_p.combiner, b[4])
      assert torch.equal(bits(torch, ref), bits(torch, out_p)), "step %d: the forward did not combine the resident rows" % step
    out_t, tw_t = _lookup(env, form, T, b)
    assert len(T._shapes) == len(P._shapes), "the twins' draw counts part: the comparison below would not be about the route"
    assert torch.equal(bits(torch, out_p), bits(torch, out_t)), "step %d: the result differs from the chain's" % step
    if step == STEPS - 1:      # (the twin's weights_grad looks its rows up: a draw of its own, so behind the last lookup)
      dw_p, dw_t = tw_p.weights_grad(b[5]), tw_t.weights_grad(b[5])
      assert dw_p.shape == dw_t.shape == b[2].shape and torch.equal(bits(torch, dw_p), bits(torch, dw_t))
    deo_p.apply_combined_gradients([(b[5], tw_p)])
    deo_t.apply_combined_gradients([(b[5], tw_t)])
  assert route == {read_name: STEPS, "tfra_table_find_or_insert": STEPS, "tfra_unique": STEPS}, route
  table.check_errors()
  _same_state(torch, de, deo_p, deo_t, opt, P, T, tag)
  assert int(P.size()) > 300


# ---- 2. many variables -------------------------------------------------------------------------------------------------------------
def _tier_creator(de):
  return de.TieredHashTableCreator(de.TieredHashTableConfig(
      upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=1024))


def _whole_rows(torch, var, keys):
  """[n, (1 + aux) * dim]: embedding and slots of `keys`; a tiered variable is read through flush() plus its lower table"""
  t = var._tables[0]
  if hasattr(t, "flush"):
    t.flush()
    table = t._lower
  else:
    table = t._table
  assert bool(table.contains(keys).all())
  return torch.cat([table.find(keys, field=f) for f in range(var.aux_fields + 1)], dim=1)


@pytest.mark.parametrize("form,more", [("tuple", 0), ("tuple", 1), ("safe", 0), ("ragged", 0)])
def test_a_mixed_list_trains_as_its_twins(env, monkeypatch, form, more):
  """ADMIT_MANY_MIN_TABLES (+ more) plain "pooled" members (at and above the threshold: ONE grouped admission), a static-default member, a True member
  (its own chain) and a tiered "pooled" member whose small cache (15 * 89 slots for 1 500 keys) evicts under the steps — each against a
  roomy plain twin (the "pooled" ones: init_on_lookup=True) trained by the single calls."""
  torch, de = env
  n_pooled = de.variable.ADMIT_MANY_MIN_TABLES + more
  opt = _opt(de, "adam")
  tag = "%s_%d" % (form, n_pooled)
  kinds = ["pooled"] * n_pooled + ["static", True, "tiered"]
  vs, twins = [], []
  for k, kind in enumerate(kinds):
    static = kind == "static"
    mode = "pooled" if kind == "tiered" else (False if static else kind)
    vs.append(_var(env, "pam_%s_%d" % (tag, k), opt, mode, static=static, creator=_tier_creator(de) if kind == "tiered" else None))
    twins.append(_var(env, "pam_twin_%s_%d" % (tag, k), opt, False if static else True, static=static))
  deo, deo_twin = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  # the tiered member starts from a full cache, the ids its batches repeat only below it (written first, pushed out by 1 500 more)
  rng = np.random.default_rng(5)
  for pre in (_universe(20 + len(kinds) - 1)[:300], np.unique(rng.integers(2**41, 2**42, size=1500, dtype=np.int64))):
    rows = torch.from_numpy(rng.standard_normal((pre.size, DIM)).astype(np.float32)).cuda()
    vs[-1].upsert(torch.from_numpy(pre).cuda(), rows)
    twins[-1].upsert(torch.from_numpy(pre).cuda(), rows)
  calls = Calls(monkeypatch)
  per_var = [_batches(20 + k) for k in range(len(kinds))]
  seen = [set() for _ in kinds]
  for step in range(STEPS):
    bs = [_dev(torch, per_var[k][step]) for k in range(len(kinds))]
    for k in range(len(kinds)):
      ids, w = per_var[k][step][0], per_var[k][step][2]
      seen[k].update((ids[w > 0] if form == "safe" else ids).tolist())      # (the safe form prunes by weight: those ids are not looked up)
    c0 = dict(calls.n)
    res = _lookup_many(env, form, vs, bs)
    d = {n: calls[n] - c0.get(n, 0) for n in ("tfra_multi_find_or_insert", "tfra_table_find_or_insert", "tfra_tier_find_or_insert",
                                               "tfra_multi_tier_find_or_insert")}
    # the plain "pooled" members in ONE grouped admission; the True member's chain is the one single find_or_insert; the tier alone
    # (safe: the True member's default_id row goes through embedding_lookup, which admits for it; a "pooled" member's is a read)
    assert d == {"tfra_multi_find_or_insert": 1, "tfra_table_find_or_insert": 2 if form == "safe" else 1, "tfra_tier_find_or_insert": 1,
                 "tfra_multi_tier_find_or_insert": 0}, d
    deo.apply_combined_gradients_many([(b[5], tw) for b, (_, tw) in zip(bs, res)])
    pairs = []
    for k, (twin, b) in enumerate(zip(twins, bs)):
      out, tw = _lookup(env, form, twin, b)
      assert torch.equal(bits(torch, res[k][0]), bits(torch, out)), "step %d member %d (%s): the grouped result is not the twin's" % (step, k, kinds[k])
      pairs.append((b[5], tw))
    deo_twin.apply_combined_gradients(pairs)
  st = vs[-1]._tables[0]._tier.stats()
  assert st["calls"] >= STEPS and st["demoted"] > 0 and st["lower_hits"] > 0        # keys went down and came up again
  for k, (var, twin) in enumerate(zip(vs, twins)):
    keys = torch.from_numpy(np.fromiter(seen[k], np.int64, len(seen[k]))).cuda()
    a, b = _whole_rows(torch, var, keys), _whole_rows(torch, twin, keys)
    assert a.shape == b.shape == (keys.numel(), DIM * 3)                              # embedding, m, v
    bad = (bits(torch, a) != bits(torch, b)).any(1)
    assert not bool(bad.any()), "member %d (%s): %d of %d keys differ from the twin (embedding, m or v)" % (k, kinds[k], int(bad.sum()), keys.numel())
    var._tables[0]._table.check_errors()


def test_the_grouped_admission_starts_at_its_threshold(env, monkeypatch):
  """Below ADMIT_MANY_MIN_TABLES distinct tables the loop of single admissions stays; from there on the list is ONE
  tfra_multi_find_or_insert and no single one; a table that stands again is admitted by the single call behind the grouped one."""
  torch, de = env
  least = de.variable.ADMIT_MANY_MIN_TABLES
  opt = _opt(de, "sgd")
  vs = [_var(env, "pa_thr_%d" % k, opt, "pooled") for k in range(least + 1)]
  bs = [_dev(torch, _batches(40 + k, steps=1)[0]) for k in range(least + 2)]
  calls = Calls(monkeypatch)
  names = ("tfra_multi_find_or_insert", "tfra_table_find_or_insert")
  lists = [(list(range(n)), (0, n) if n < least else (1, 0)) for n in range(1, least + 2)]
  lists.append((list(range(least)) + [0], (1, 1)))                                   # the first variable stands twice
  for members, want in lists:
    c0 = dict(calls.n)
    res = de.embedding_lookup_sparse_many([vs[k] for k in members], [(bs[j][1], bs[j][0]) for j in range(len(members))],
                                          [bs[j][2].abs() for j in range(len(members))], combiner="sum", return_trainable=True,
                                          num_rows=[bs[j][4] for j in range(len(members))])
    assert tuple(calls[n] - c0.get(n, 0) for n in names) == want, (members, calls.n)
    for j, k in enumerate(members):                                                   # every entry id got in
      assert bool(vs[k]._tables[0]._table.contains(torch.unique(bs[j][0])).all())
    assert len(res) == len(members)


# ---- 3. what stays on the chain, and the errors ------------------------------------------------------------------------------------
def test_what_stays_on_the_chain(env, monkeypatch):
  torch, de = env
  opt = _opt(de, "sgd")
  P = _var(env, "pa_stay", opt, "pooled")
  b = _dev(torch, _batches(60, steps=1)[0])
  calls = Calls(monkeypatch)
  # a non-training lookup inserts nothing and does not read through the pooled kernel
  size0 = int(P.size())
  out = de.embedding_lookup_sparse(P, (b[1], b[0]), b[2].abs(), combiner="sum", num_rows=b[4])
  assert tuple(out.shape) == (b[4], DIM) and int(P.size()) == size0 == 0
  assert calls["tfra_table_find_combine"] == 0 and calls["tfra_table_find_or_insert"] == 0
  out = de.ragged_embedding_ops.embedding_lookup_sparse(P, (b[3], b[0]), b[2].abs(), combiner="sum")
  assert int(P.size()) == 0 and calls["tfra_table_find_combine_ragged"] == 0
  # max_norm keeps the chain for the training lookup too
  de.embedding_lookup_sparse(P, (b[1], b[0]), b[2].abs(), combiner="sum", max_norm=1.0, return_trainable=True, num_rows=b[4])
  assert calls["tfra_table_find_combine"] == 0 and calls["tfra_table_find_or_insert"] == 1
  # the dense lookup behaves as with True: it admits
  _, tw = de.embedding_lookup(P, b[0], return_trainable=True)
  assert calls["tfra_table_find_or_insert"] == 2 and bool(P._tables[0]._table.contains(torch.unique(b[0])).all())
  # several shards take the True route
  S = _var(env, "pa_shards", opt, "pooled", devices=["cuda:0", "cuda:0"])
  assert not S.can_admit_pooled() and S.admits_on_lookup()
  c0 = dict(calls.n)
  out, tw = de.embedding_lookup_sparse(S, (b[1], b[0]), b[2].abs(), combiner="sum", return_trainable=True, num_rows=b[4])
  assert calls["tfra_table_find_combine"] == c0.get("tfra_table_find_combine", 0)
  assert calls["tfra_table_find_or_insert"] - c0.get("tfra_table_find_or_insert", 0) == 2      # one per shard
  assert int(S.size()) == int(torch.unique(b[0]).numel())
  # a static default row with "pooled": the pooled forward as it always was, nothing to admit
  V = _var(env, "pa_static", opt, "pooled", static=True)
  assert V.can_lookup_combined() and not V.can_admit_pooled()
  c0 = dict(calls.n)
  de.embedding_lookup_sparse(V, (b[1], b[0]), b[2].abs(), combiner="sum", return_trainable=True, num_rows=b[4])
  assert calls["tfra_table_find_combine"] - c0.get("tfra_table_find_combine", 0) == 1
  assert calls["tfra_table_find_or_insert"] == c0.get("tfra_table_find_or_insert", 0) and int(V.size()) == 0


def test_errors(env):
  torch, de = env
  for bad in ("nope", "Pooled", 2, None):
    with pytest.raises(ValueError, match="init_on_lookup must be"):
      de.Variable(dim=DIM, name="pa_bad", initializer=0.0, init_on_lookup=bad)
  # more entry ids than a tier's max_batch: the existing ValueError
  opt = _opt(de, "sgd")
  creator = de.TieredHashTableCreator(de.TieredHashTableConfig(
      upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=64))
  P = _var(env, "pa_small_batch", opt, "pooled", creator=creator)
  b = _dev(torch, _batches(61, steps=1)[0])
  with pytest.raises(ValueError, match="max_batch"):
    de.embedding_lookup_sparse(P, (b[1], b[0]), b[2].abs(), combiner="sum", return_trainable=True, num_rows=b[4])
  assert int(P.size()) == 0
