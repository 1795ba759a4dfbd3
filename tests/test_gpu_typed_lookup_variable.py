"""GPU: out_dtype at the public interface (Variable.lookup / lookup_combined / lookup_combined_ragged, embedding_lookup,
embedding_lookup_unique, embedding_lookup_sparse, safe_embedding_lookup_sparse, their *_many forms and the four functions of
ragged_embedding_ops).

On finite random rows `f(..., out_dtype=d)` has dtype d and equals `f(...).to(d)` bit for bit (torch's conversion of finite
float32 values is round to nearest even, the typed lookups' rounding; the edge values are tests/test_gpu_typed_lookup.py's
business).  Where today's path makes an untyped C call on a plain table, the typed call is made in its place — once, the twin
not at all (the call counter of tests/test_gpu_pooled_lookup.py); every other route runs as it does and converts its result."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls, T, filled_var, sparse_case

pytestmark = pytest.mark.gpu

FIND, FIND_T = "tfra_table_find", "tfra_table_find_typed"
FC, FC_T = "tfra_table_find_combine", "tfra_table_find_combine_typed"
FCR, FCR_T = "tfra_table_find_combine_ragged", "tfra_table_find_combine_ragged_typed"
MANY, MANY_T = "tfra_multi_find_combine", "tfra_multi_find_combine_typed"
MANYR, MANYR_T = "tfra_multi_find_combine_ragged", "tfra_multi_find_combine_ragged_typed"
N_ROWS = 200


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


@pytest.fixture(scope="module")
def var(env):
  torch, de = env
  return filled_var(torch, de, "tlv_plain", dim=64, initializer=0.5)


@pytest.fixture(scope="module")
def case(env):
  torch, _ = env
  seg, ids, w = sparse_case(np.random.default_rng(5), n_rows=N_ROWS)
  counts = np.bincount(seg, minlength=N_ROWS)
  rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  return T(torch, seg), T(torch, ids), T(torch, w), T(torch, rs)


def same(torch, got, ref, d):
  assert got.dtype == d and got.shape == ref.shape, (got.dtype, tuple(got.shape), tuple(ref.shape))
  want = ref.to(d)
  assert bool(torch.isfinite(ref.float()).all())
  assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))


def counted(monkeypatch, fn):
  calls = Calls(monkeypatch)
  out = fn()
  monkeypatch.undo()
  return out, calls


# ---- every entry point on a plain variable: the typed call once, its twin not at all --------------------------------------------------
def entry_points(de, var, case):
  """name -> (f(**kw), the twin's C name, the typed C name)."""
  seg, ids, w, rs = case
  reo = de.ragged_embedding_ops
  return {
      "Variable.lookup": (lambda **kw: var.lookup(ids, **kw), FIND, FIND_T),
      "Variable.lookup_combined": (lambda **kw: var.lookup_combined(ids, seg, w, "mean", N_ROWS, **kw), FC, FC_T),
      "Variable.lookup_combined_ragged": (lambda **kw: var.lookup_combined_ragged(rs, ids, w, "sqrtn", prune=True, fill_id=4, **kw), FCR, FCR_T),
      "embedding_lookup": (lambda **kw: de.embedding_lookup(var, ids[:200].reshape(100, 2), **kw), FIND, FIND_T),
      "embedding_lookup_unique": (lambda **kw: de.embedding_lookup_unique(var, ids, **kw), FIND, FIND_T),
      "embedding_lookup_sparse": (lambda **kw: de.embedding_lookup_sparse(var, (seg, ids), w, combiner="sum", num_rows=N_ROWS, **kw), FC, FC_T),
      "safe_embedding_lookup_sparse": (lambda **kw: de.safe_embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", num_rows=N_ROWS, **kw),
                                       FC, FC_T),
      "embedding_lookup_sparse_many": (lambda **kw: de.embedding_lookup_sparse_many([var, var], [(seg, ids)] * 2, [w, None], combiner="mean",
                                                                                   num_rows=N_ROWS, **kw), MANY, MANY_T),
      "safe_embedding_lookup_sparse_many": (lambda **kw: de.safe_embedding_lookup_sparse_many([var, var], [(seg, ids)] * 2, [w, None],
                                                                                             combiner="mean", num_rows=N_ROWS, **kw), MANY, MANY_T),
      "ragged.embedding_lookup_sparse": (lambda **kw: reo.embedding_lookup_sparse(var, (rs, ids), w, combiner="mean", **kw), FCR, FCR_T),
      "ragged.safe_embedding_lookup_sparse": (lambda **kw: reo.safe_embedding_lookup_sparse(var, (rs, ids), w, combiner="mean", default_id=6, **kw),
                                              FCR, FCR_T),
      "ragged.embedding_lookup_sparse_many": (lambda **kw: reo.embedding_lookup_sparse_many([var, var], [(rs, ids)] * 2, [w, None], **kw),
                                              MANYR, MANYR_T),
      "ragged.safe_embedding_lookup_sparse_many": (lambda **kw: reo.safe_embedding_lookup_sparse_many([var, var], [(rs, ids)] * 2, [w, None],
                                                                                                    default_id=[6, None], **kw), MANYR, MANYR_T),
  }


NAMES = ["Variable.lookup", "Variable.lookup_combined", "Variable.lookup_combined_ragged", "embedding_lookup", "embedding_lookup_unique",
         "embedding_lookup_sparse", "safe_embedding_lookup_sparse", "embedding_lookup_sparse_many", "safe_embedding_lookup_sparse_many",
         "ragged.embedding_lookup_sparse", "ragged.safe_embedding_lookup_sparse", "ragged.embedding_lookup_sparse_many",
         "ragged.safe_embedding_lookup_sparse_many"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_equals_its_result_converted(env, monkeypatch, var, case, name):
  torch, de = env
  f, twin, typed = entry_points(de, var, case)[name]
  ref, calls0 = counted(monkeypatch, f)                      # out_dtype=None: today's counts
  assert calls0[twin] == 1 and calls0[typed] == 0, calls0.n
  for d in (torch.bfloat16, torch.float16):
    got, calls = counted(monkeypatch, lambda: f(out_dtype=d))
    assert calls[typed] == 1 and calls[twin] == 0, (name, calls.n)
    others0 = {k: v for k, v in calls0.n.items() if k != twin}
    others = {k: v for k, v in calls.n.items() if k != typed}
    assert others == others0, (name, calls0.n, calls.n)       # nothing else is called more or less often
    for g, r in zip(got, ref) if isinstance(ref, list) else [(got, ref)]:
      same(torch, g, r, d)
  with pytest.raises(TypeError):
    f(out_dtype=torch.int32)


def test_safe_tuple_form_with_a_default_id(env, var, case):
  torch, de = env
  seg, ids, w, rs = case
  for default_id in (4, 5):   # resident, and a miss that takes the default row
    ref = de.safe_embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", default_id=default_id, num_rows=N_ROWS)
    got = de.safe_embedding_lookup_sparse(var, (seg, ids), w, combiner="mean", default_id=default_id, num_rows=N_ROWS, out_dtype=torch.bfloat16)
    same(torch, got, ref, torch.bfloat16)


def test_half_table_feeding_a_float32_model(env, monkeypatch, case):
  torch, de = env
  seg, ids, w, rs = case
  v16 = filled_var(torch, de, "tlv_f16", dim=64, initializer=0.5, value_dtype=torch.float16)
  ref = v16.lookup(ids)
  got, calls = counted(monkeypatch, lambda: v16.lookup(ids, out_dtype=torch.float32))
  assert calls[FIND_T] == 1 and calls[FIND] == 0
  same(torch, got, ref, torch.float32)
  same(torch, v16.lookup(ids, out_dtype=torch.bfloat16), ref.float(), torch.bfloat16)   # through float32


# ---- the routes without a typed call: they run as they do, and the result is converted -------------------------------------------------
def test_max_norm_is_converted_behind_the_clip(env, monkeypatch, var, case):
  torch, de = env
  seg, ids, w, rs = case
  ref = de.embedding_lookup(var, ids, max_norm=1.5)
  got, calls = counted(monkeypatch, lambda: de.embedding_lookup(var, ids, max_norm=1.5, out_dtype=torch.bfloat16))
  assert calls[FIND] == 1 and calls[FIND_T] == 0, calls.n
  same(torch, got, ref, torch.bfloat16)
  ref = de.embedding_lookup_sparse(var, (seg, ids), w, max_norm=1.5, num_rows=N_ROWS)
  got, calls = counted(monkeypatch, lambda: de.embedding_lookup_sparse(var, (seg, ids), w, max_norm=1.5, num_rows=N_ROWS,
                                                                       out_dtype=torch.float16))
  assert calls[FC_T] == 0 and calls[FIND_T] == 0, calls.n
  same(torch, got, ref, torch.float16)


def test_two_shards_take_a_typed_find_each_and_the_op_chain_converts(env, monkeypatch, case):
  torch, de = env
  seg, ids, w, rs = case
  dev = "cuda:%d" % torch.cuda.current_device()
  v2 = filled_var(torch, de, "tlv_two", dim=64, initializer=0.5, devices=[dev, dev])
  ref = v2.lookup(ids)
  got, calls = counted(monkeypatch, lambda: v2.lookup(ids, out_dtype=torch.bfloat16))
  assert calls[FIND_T] == 2 and calls[FIND] == 0, calls.n     # the conversion commutes with the stitching
  same(torch, got, ref, torch.bfloat16)
  assert not v2.can_lookup_combined()
  ref = de.embedding_lookup_sparse(v2, (seg, ids), w, num_rows=N_ROWS)
  got, calls = counted(monkeypatch, lambda: de.embedding_lookup_sparse(v2, (seg, ids), w, num_rows=N_ROWS, out_dtype=torch.bfloat16))
  assert calls[FC_T] == 0 and calls[FC] == 0 and calls[FIND_T] == 0, calls.n   # the op chain: float32 rows, combined, converted
  same(torch, got, ref, torch.bfloat16)
  ref = de.ragged_embedding_ops.embedding_lookup_sparse(v2, (rs, ids), w)
  same(torch, de.ragged_embedding_ops.embedding_lookup_sparse(v2, (rs, ids), w, out_dtype=torch.float16), ref, torch.float16)


def test_a_tiered_variable_runs_untyped_and_converts(env, monkeypatch, case):
  torch, de = env
  seg, ids, w, rs = case
  cfg = de.TieredHashTableConfig(upper=de.HkvHashTableConfig(init_capacity=1024, max_capacity=1024, evict_strategy=de.HkvEvictStrategy.LRU),
                                 max_batch=4096)
  tv = de.Variable(dim=64, name="tlv_tiered", initializer=0.5, kv_creator=de.TieredHashTableCreator(cfg))
  keys = torch.arange(0, 3000, 2, device="cuda")
  tv.upsert(keys, torch.randn((keys.numel(), 64), generator=torch.Generator(device="cuda").manual_seed(7), device="cuda"))
  plain = filled_var(torch, de, "tlv_beside_tier", dim=64, initializer=0.5)
  for f in (lambda **kw: tv.lookup(ids, **kw),
            lambda **kw: de.embedding_lookup_sparse(tv, (seg, ids), w, num_rows=N_ROWS, **kw),
            lambda **kw: de.ragged_embedding_ops.safe_embedding_lookup_sparse(tv, (rs, ids), w, default_id=4, **kw)):
    ref = f()
    got, calls = counted(monkeypatch, lambda: f(out_dtype=torch.bfloat16))
    assert not any(k.endswith("_typed") for k in calls.n), calls.n
    same(torch, got, ref, torch.bfloat16)
  # a grouped list with a tiered member runs untyped as a whole, and every result is converted
  many = lambda **kw: de.embedding_lookup_sparse_many([plain, tv], [(seg, ids)] * 2, [w, w], num_rows=N_ROWS, **kw)
  ref = many()
  got, calls = counted(monkeypatch, lambda: many(out_dtype=torch.float16))
  assert calls["tfra_multi_tier_find_combine"] == 1 and calls[MANY_T] == 0, calls.n
  for g, r in zip(got, ref):
    same(torch, g, r, torch.float16)


def test_bp_v2_keeps_table_dtype_values_for_accum(env, monkeypatch, case):
  torch, de = env
  seg, ids, w, rs = case
  vb = filled_var(torch, de, "tlv_bpv2", dim=64, initializer=0.5, bp_v2=True)
  uniq = torch.unique(ids)
  ref, _ = de.embedding_lookup(vb, uniq, return_trainable=True)
  (got, tw), calls = counted(monkeypatch, lambda: de.embedding_lookup(vb, uniq, return_trainable=True, out_dtype=torch.bfloat16))
  assert calls[FIND_T] == 0, calls.n
  same(torch, got, ref, torch.bfloat16)
  assert tw.read_value().dtype == torch.float32 and tw.exists is not None     # what update_op hands accum as the old values
  tw.update_op(tw.read_value() + 1.0)
  assert torch.allclose(vb.lookup(uniq), ref + 1.0, atol=1e-5)


def test_init_on_lookup_admits_and_converts(env, monkeypatch):
  torch, de = env
  g = torch.Generator(device="cuda").manual_seed(3)
  init = lambda shape: torch.randn(shape, generator=g, device="cuda")
  va = de.Variable(dim=64, name="tlv_admit", initializer=init, init_on_lookup=True)
  ids = torch.arange(100, 400, 3, device="cuda")
  (got, tw), calls = counted(monkeypatch, lambda: de.embedding_lookup(va, ids, return_trainable=True, out_dtype=torch.bfloat16))
  assert calls[FIND_T] == 0 and sum(v for k, v in calls.n.items() if "find_or_insert" in k) == 1, calls.n
  assert got.dtype == torch.bfloat16 and int(va.size()) == ids.numel()
  same(torch, got, va.lookup(ids), torch.bfloat16)            # what it returned is what the table now holds, converted


# ---- training: bfloat16 activations out, bfloat16 gradients back -----------------------------------------------------------------------
def _state(torch, de, deo, opt, var):
  k, v = var.export()
  o = torch.argsort(k)
  return [k[o], v[o].view(torch.int32)] + [deo.get_slot(var, s).lookup(k[o]).view(torch.int32) for s in opt.slots]


@pytest.mark.parametrize("form", ["embedding_lookup", "embedding_lookup_sparse"])
def test_training_round_trip_equals_the_float32_lookups(env, case, form):
  torch, de = env
  seg, ids, w, rs = case
  opt = de.optimizers.Adam(1e-2)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  va, vb = (filled_var(torch, de, "tlv_train_%s_%s" % (form, t), dim=64, initializer=0.5, **kw) for t in "ab")
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  for step in range(3):
    gen = torch.Generator(device="cuda").manual_seed(50 + step)
    if form == "embedding_lookup":
      ea, twa = de.embedding_lookup(va, ids, return_trainable=True, out_dtype=torch.bfloat16)
      eb, twb = de.embedding_lookup(vb, ids, return_trainable=True)
      grad = (torch.randn(eb.shape, generator=gen, device="cuda") * 0.01).to(torch.bfloat16)
      da.apply_gradients([(grad, twa)])
      db.apply_gradients([(grad, twb)])
    else:
      ea, twa = de.embedding_lookup_sparse(va, (seg, ids), w, return_trainable=True, num_rows=N_ROWS, out_dtype=torch.bfloat16)
      eb, twb = de.embedding_lookup_sparse(vb, (seg, ids), w, return_trainable=True, num_rows=N_ROWS)
      grad = (torch.randn(eb.shape, generator=gen, device="cuda") * 0.01).to(torch.bfloat16)
      da.apply_combined_gradients([(grad, twa)])
      db.apply_combined_gradients([(grad, twb)])
    same(torch, ea, eb, torch.bfloat16)                        # the activations of every step, not only the first
  for x, y in zip(_state(torch, de, da, opt, va), _state(torch, de, db, opt, vb)):
    assert torch.equal(x, y)
