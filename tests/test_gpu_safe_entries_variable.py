"""GPU: the training forms of the safe sparse lookups take their kept lists and entry lists from the device builder
(`device_ops.safe_entries_many`) and change no bit.

Three variables of dims 16 / 64 / 128 — a plain one with a constant initializer, one with init_on_lookup="pooled" and a seeded
callable initializer, a tiered one (with int32 keys: a plain one in the tier's place) —, 192 rows x 4 ids, a twelfth of the weights
<= 0, one row pruned empty, some rows without entries.  Two steps, each the tuple form and the ragged form of
safe_embedding_lookup_sparse with return_trainable followed by apply_combined_gradients with Adam — once through the single calls,
once through the `*_many` forms.  Results, `weights_grad` and the exported keys, rows and slots equal, bit for bit, the same run
with `_safe_sparse_args` / `_safe_sparse_args_many` replaced by `_safe_sparse_args_torch`, the torch preprocessing they replace.
The builder runs under torch's sync debug mode "error": only its one read of the counts is let through."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls, T, bits

pytestmark = pytest.mark.gpu

N_ROWS, PER_ROW, STEPS, UNIVERSE, DEFAULT_ID = 192, 4, 2, 900, 4242
DIMS = (16, 64, 128)


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _initializer(torch, seed):
  count = [0]

  def draw(shape):
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + count[0])
    count[0] += 1
    return torch.randn(tuple(int(x) for x in shape), generator=g, device="cuda") * 0.05
  return draw


def _vars(env, tag, key_dtype):
  torch, de = env
  opt = de.optimizers.Adam(0.01)
  tier = de.TieredHashTableCreator(de.TieredHashTableConfig(
      upper=de.HkvHashTableConfig(init_capacity=15 * 512, max_capacity=15 * 512, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=2048))
  kw = [dict(initializer=0.25), dict(initializer=_initializer(torch, 1), init_on_lookup="pooled"),
        dict(initializer=_initializer(torch, 2), init_on_lookup="pooled", kv_creator=tier) if key_dtype == torch.int64 else
        dict(initializer=-0.5)]
  return opt, [de.Variable(key_dtype=key_dtype, value_dtype=torch.float32, dim=dim, devices=["cuda:0"], name="sev_%s_%d" % (tag, k),
                           **kw[k], **de.DynamicEmbeddingOptimizer.variable_kwargs(opt)) for k, dim in enumerate(DIMS)]


def _batch(torch, k, step, key_dtype):
  """(ids, rows, w, splits): rows 5 .. 8 and the last three have no entries, row 2's are all pruned"""
  rng = np.random.default_rng(100 * k + step)
  per = np.full(N_ROWS, PER_ROW)
  per[5:9] = 0
  per[-3:] = 0
  rows = np.repeat(np.arange(N_ROWS, dtype=np.int64), per)
  nnz = rows.size
  ids = ((rng.zipf(1.2, size=nnz) + 200 * step) % UNIVERSE + 1) * 7 - 3000
  ids[0] = DEFAULT_ID
  w = rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)
  w[rng.choice(np.arange(1, nnz), size=nnz // 12, replace=False)] = np.float32(-0.5)
  w[rows == 2] = np.float32(0.0)
  splits = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
  return T(torch, ids.astype(np.int32 if key_dtype == torch.int32 else np.int64)), T(torch, rows), T(torch, w), T(torch, splits)


def _grad(torch, k, step, dim, form):
  g = torch.Generator(device="cuda").manual_seed(7000 + 10 * k + step + (100 if form == "ragged" else 0))
  return torch.randn((N_ROWS, dim), generator=g, device="cuda") * 0.01


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


def _train(env, tag, key_dtype, many, default_id):
  """-> every lookup's result and weight gradient, every variable's contents"""
  torch, de = env
  reo = de.ragged_embedding_ops
  opt, vs = _vars(env, tag, key_dtype)
  deo = de.DynamicEmbeddingOptimizer(opt)
  seen = []
  for step in range(STEPS):
    bs = [_batch(torch, k, step, key_dtype) for k in range(len(vs))]
    for form in ("tuple", "ragged"):
      kw = dict(combiner="mean", default_id=default_id, return_trainable=True)
      sp = [(b[1], b[0]) if form == "tuple" else (b[3], b[0]) for b in bs]
      if form == "tuple":
        kw["num_rows"] = N_ROWS
      if many:
        fn = de.safe_embedding_lookup_sparse_many if form == "tuple" else reo.safe_embedding_lookup_sparse_many
        res = fn(vs, sp, [b[2] for b in bs], **kw)
      else:
        fn = de.safe_embedding_lookup_sparse if form == "tuple" else reo.safe_embedding_lookup_sparse
        res = [fn(v, s, b[2], **kw) for v, s, b in zip(vs, sp, bs)]
      grads = [_grad(torch, k, step, v.dim, form) for k, v in enumerate(vs)]
      for (out, tw), g in zip(res, grads):
        seen.append(bits(torch, out).clone())
        seen.append(bits(torch, tw.weights_grad(g)).clone())
      pairs = [(g, tw) for g, (_, tw) in zip(grads, res)]
      (deo.apply_combined_gradients_many if many else deo.apply_combined_gradients)(pairs)
  return seen, [_contents(torch, v) for v in vs]


def _relaxed(torch, fn, *a):
  """fn(*a) with synchronising calls allowed, whatever the mode around it"""
  mode = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode("default")
  try:
    return fn(*a)
  finally:
    torch.cuda.set_sync_debug_mode(mode)


def test_a_lookup_that_does_not_train_asks_for_its_kept_list_only(env, monkeypatch):
  """weights and a pruning combiner: one builder call without the entry list; a sum combiner or no weights: no call at all; the
  results are the torch preprocessing's"""
  torch, de = env
  var, dops = de.variable, de.device_ops
  opt, vs = _vars(env, "fwd", torch.int64)
  v = vs[0]
  ids, rows, w, _ = _batch(torch, 0, 0, torch.int64)
  v.upsert(torch.unique(ids), torch.randn((int(torch.unique(ids).numel()), v.dim), device="cuda"))
  asked = []
  real = dops.safe_entries_many
  monkeypatch.setattr(dops, "safe_entries_many", lambda reqs, **k: (asked.append((len(reqs), k)), real(reqs, **k))[1])
  cases = [("mean", w, DEFAULT_ID), ("sqrtn", w, None), ("sum", w, DEFAULT_ID), ("mean", None, DEFAULT_ID)]
  got = [de.safe_embedding_lookup_sparse(v, (rows, ids), ww, combiner=c, default_id=d, num_rows=N_ROWS) for c, ww, d in cases]
  assert asked == [(1, dict(want_kept=[True], want_entries=False))] * 2, asked
  monkeypatch.setattr(var, "_safe_sparse_args", var._safe_sparse_args_torch)
  for (c, ww, d), g in zip(cases, got):
    e = de.safe_embedding_lookup_sparse(v, (rows, ids), ww, combiner=c, default_id=d, num_rows=N_ROWS)
    assert torch.equal(bits(torch, g), bits(torch, e)), (c, d)
  assert len(asked) == 2


@pytest.mark.parametrize("default_id", [DEFAULT_ID, None])
@pytest.mark.parametrize("many", [False, True], ids=["single", "many"])
@pytest.mark.parametrize("keys", ["int64", "int32"])
def test_a_training_step_changes_no_bit(env, monkeypatch, keys, many, default_id):
  torch, de = env
  var, reo, dops = de.variable, de.ragged_embedding_ops, de.device_ops
  key_dtype = getattr(torch, keys)
  tag = "%s_%d_%s" % (keys, many, default_id)
  calls = Calls(monkeypatch)
  reads = []
  real_builder, real_read = dops.safe_entries_many, dops._read_counts

  def strict_builder(*a, **k):   # the builder never synchronises but for its one read of the counts
    torch.cuda.set_sync_debug_mode("error")
    try:
      return real_builder(*a, **k)
    finally:
      torch.cuda.set_sync_debug_mode("default")

  with monkeypatch.context() as m:
    m.setattr(dops, "safe_entries_many", strict_builder)
    m.setattr(dops, "_read_counts", lambda c: (reads.append(tuple(c.shape)), _relaxed(torch, real_read, c))[1])
    seen, contents = _train(env, tag + "_new", key_dtype, many, default_id)
  n_calls = calls["tfra_multi_safe_entries"]
  # one builder call and one read per lookup call: the many forms serve their three members at once
  assert n_calls == len(reads) == STEPS * 2 * (1 if many else len(DIMS)), (n_calls, reads)
  assert all(r == ((len(DIMS) if many else 1), 2) for r in reads), reads

  def many_torch(params_list, sp_ids_list, weights, combiners, default_ids, return_trainable, num, ragged=False):
    sp = [(reo.row_ids_of(s[0], s[1].numel()), s[1]) if ragged else s for s in sp_ids_list]
    return [var._safe_sparse_args_torch(p, sp[i], weights[i], combiners[i], default_ids[i], return_trainable, num[i])
            for i, p in enumerate(params_list)]
  monkeypatch.setattr(var, "_safe_sparse_args", var._safe_sparse_args_torch)
  monkeypatch.setattr(var, "_safe_sparse_args_many", many_torch)
  monkeypatch.setattr(reo, "_safe_sparse_args_many", many_torch)
  seen_t, contents_t = _train(env, tag + "_torch", key_dtype, many, default_id)
  assert calls["tfra_multi_safe_entries"] == n_calls
  assert len(seen) == len(seen_t) == STEPS * 2 * len(DIMS) * 2
  for k, (a, b) in enumerate(zip(seen, seen_t)):
    assert a.shape == b.shape and torch.equal(a, b), "output %d differs from the torch preprocessing's" % k
  for k, ((ka, ra), (kb, rb)) in enumerate(zip(contents, contents_t)):
    assert ka.numel() > 100 and torch.equal(ka, kb), "variable %d: the keys differ" % k
    assert ra.shape == rb.shape and torch.equal(ra, rb), "variable %d: embedding or slots differ" % k
