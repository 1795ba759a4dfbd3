"""GPU: the pooled lookup (tfra_table_find_combine; Variable.lookup_combined; the forward of embedding_lookup_sparse and
safe_embedding_lookup_sparse).

"Composition" = what the forward was before: tfra_table_find (or unique -> lookup) followed by
tfra_sparse_segment_combine.  The pooled kernel walks a row's entries in the same order and compiles the same accumulate /
scale expressions (csrc/tfra_combine_device.h) under -ffp-contract=off, so the two must agree BIT FOR BIT: those comparisons
are torch.equal on int32 views, no tolerance."""
import ctypes

import numpy as np
import pytest

import oracle
from tests.sparse_helpers import COMB, Calls, T, _export_state, _raw_find_combine, batch, bits, filled_var, sparse_case, table

pytestmark = pytest.mark.gpu

UNSUPPORTED = -6


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def composition(torch, de, t, ids_t, seg_t, w_t, combiner, n_rows):
  """tfra_table_find (default_is_full = 0) + tfra_sparse_segment_combine over idx = 0..nnz-1."""
  rows = t._table.find(ids_t)
  idx = torch.arange(ids_t.numel(), dtype=torch.int32, device="cuda")
  return de.device_ops.sparse_segment_combine(rows, idx, seg_t, w_t, combiner, n_rows)


# ---- 1. the C entry against the two-call composition, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("dim", [4, 64, 128, 256])
@pytest.mark.parametrize("vdtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("kind", ["cuckoo", "hkv"])
def test_find_combine_equals_find_plus_combine_bitwise(env, kind, vdtype, dim, combiner, weighted):
  torch, de = env
  nnz, n_rows = 20000, 1400
  ids, seg, w, ids_t, seg_t, w_t = batch(torch, nnz, n_rows)
  t = table(torch, de, kind, vdtype, dim)
  wt = w_t if weighted else None
  got = t._table.find_combine(ids_t, seg_t, wt, COMB[combiner], n_rows)
  exp = composition(torch, de, t, ids_t, seg_t, wt, combiner, n_rows)
  assert got.dtype == torch.float32 and tuple(got.shape) == (n_rows, dim)
  assert torch.equal(bits(torch, got), bits(torch, exp))
  # the layout did what it was built for
  g = got.cpu().numpy()
  for r in (0, 1, n_rows // 2, n_rows - 1):
    assert not g[r].any()                                   # rows without entries
  if weighted:
    assert not g[5].any() or combiner == "sum"              # weight sum 0 (sum: every term is 0 * row)
    if combiner == "mean":
      assert not g[4].any()
  assert np.isfinite(g).all() and g[3].any()
  t._table.check_errors()


def test_find_combine_bench_sized_batch_bitwise(env):
  torch, de = env
  nnz, n_rows = 131072, 8192
  ids, seg, w, ids_t, seg_t, w_t = batch(torch, nnz, n_rows)
  t = table(torch, de, "cuckoo", "float32", 64)
  for combiner in ("sum", "mean", "sqrtn"):
    got = t._table.find_combine(ids_t, seg_t, w_t, COMB[combiner], n_rows)
    assert torch.equal(bits(torch, got), bits(torch, composition(torch, de, t, ids_t, seg_t, w_t, combiner, n_rows)))
  t._table.check_errors()


# ---- 2. against the oracle (the shapes and the tolerance of test_gpu_sparse_train.py's kernel check) -------------------------
def _small_batch(rng, n_rows, per_row_max, id_hi, weighted):
  counts = rng.integers(0, per_row_max + 1, size=n_rows)
  counts[0] = 0
  counts[1] = per_row_max
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = rng.integers(0, id_hi, size=seg.size).astype(np.int64)
  ids[1] = ids[0]
  ids[-1] = ids[0]
  w = None
  if weighted:
    w = rng.uniform(0.1, 2.0, size=seg.size).astype(np.float32)
    w[seg == 2] = 0.0
  return seg, ids, w


def np_forward(E, seg, w, combiner, n_rows):
  """float64: out[r] = sum w_e E_e, / sum w (mean), / sqrt(sum w^2) (sqrtn); 0 where that sum is 0."""
  E = E.astype(np.float64)
  w = np.ones(seg.size) if w is None else w.astype(np.float64)
  out = np.zeros((n_rows, E.shape[1]))
  np.add.at(out, seg, E * w[:, None])
  if combiner != "sum":
    den = np.zeros(n_rows)
    np.add.at(den, seg, w if combiner == "mean" else w * w)
    den = den if combiner == "mean" else np.sqrt(den)
    out = np.where(den[:, None] != 0, out / np.where(den != 0, den, 1)[:, None], 0)
  return out


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dim", [4, 64, 256])
def test_find_combine_matches_oracle(env, combiner, weighted, dim):
  torch, de = env
  rng = np.random.default_rng(dim * 7 + COMB[combiner] * 2 + weighted)
  n_rows = 300
  seg, ids, w = _small_batch(rng, n_rows, 6, 40, weighted)
  resident = np.arange(0, 40, 2, dtype=np.int64)           # odd ids miss
  rows = rng.uniform(0.0, 1.0, size=(resident.size, dim)).astype(np.float32)
  var = de.Variable(dim=dim, name="plo_%s_%d_%d" % (combiner, weighted, dim), initializer=0.5)
  var.upsert(T(torch, resident), T(torch, rows))
  tab = oracle.CpuTable(dim)
  tab.insert(resident, rows)
  E = tab.find(ids, np.full(dim, 0.5, np.float32))
  exp = np_forward(E, seg, w, combiner, n_rows).astype(np.float32)
  wt = None if w is None else T(torch, w)
  got = var.lookup_combined(T(torch, ids), T(torch, seg), wt, combiner, n_rows)
  np.testing.assert_allclose(got.cpu().numpy(), exp, rtol=1e-6, atol=1e-6)
  out = de.embedding_lookup_sparse(var, (T(torch, seg), T(torch, ids)), wt, combiner=combiner, num_rows=n_rows)
  assert torch.equal(bits(torch, out), bits(torch, got))


# ---- 3. the public path ----------------------------------------------------------------------------------------------------
def explicit_els(torch, de, var, seg_t, ids_t, w_t, combiner, n_rows):
  """The forward as the op chain: device_ops.unique -> Variable.lookup -> device_ops.sparse_segment_combine."""
  uniq, idx, _ = de.device_ops.unique(ids_t)
  return de.device_ops.sparse_segment_combine(var.lookup(uniq), idx, seg_t, w_t, combiner, n_rows)


@pytest.mark.parametrize("vdtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("key32", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_embedding_lookup_sparse_takes_the_pooled_route(env, monkeypatch, combiner, key32, vdtype):
  torch, de = env
  rng = np.random.default_rng(COMB[combiner])
  n_rows = 200
  seg, ids, w = sparse_case(rng, n_rows)
  var = filled_var(torch, de, "plp_%s_%d_%s" % (combiner, key32, vdtype), key_dtype=torch.int32 if key32 else torch.int64,
                   value_dtype=getattr(torch, vdtype), initializer=0.5)
  ids_t = T(torch, ids.astype(np.int32) if key32 else ids)
  seg_t, w_t = T(torch, seg), T(torch, w)
  exp = explicit_els(torch, de, var, seg_t, ids_t, w_t, combiner, n_rows)
  calls = Calls(monkeypatch)
  ind2 = torch.stack([seg_t, torch.zeros_like(seg_t)], 1)
  got = de.embedding_lookup_sparse(var, (ind2, ids_t), w_t, combiner=combiner, num_rows=n_rows)
  assert calls["tfra_table_find_combine"] == 1 and calls["tfra_unique"] == 0 and calls["tfra_sparse_segment_combine"] == 0
  assert torch.equal(bits(torch, got), bits(torch, exp))
  got2 = de.embedding_lookup_sparse(var, (seg_t, ids_t), None, combiner=combiner)   # no weights, n_rows from seg.max()
  assert torch.equal(bits(torch, got2), bits(torch, explicit_els(torch, de, var, seg_t, ids_t, None, combiner, int(seg.max()) + 1)))


def explicit_safe(torch, de, var, rows, ids_t, w_t, combiner, n, default_id):
  """safe_embedding_lookup_sparse restated over the explicit chain: prune (weights <= 0 unless sum), combine, fill empty rows."""
  if w_t is not None and combiner != "sum":
    keep = w_t > 0
    rows, ids_t, w_t = rows[keep], ids_t[keep], w_t[keep]
  res = explicit_els(torch, de, var, rows, ids_t, w_t, combiner, n)
  if default_id is not None:
    empty = torch.ones(n, dtype=torch.bool, device="cuda")
    empty[rows] = False
    d = var.lookup(torch.tensor([default_id], dtype=var.key_dtype, device="cuda")).to(torch.float32)
    res = torch.where(empty[:, None], d, res)
  return res


@pytest.mark.parametrize("default_id", [None, 4, 5])     # 4 resident, 5 a miss
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_safe_embedding_lookup_sparse_rank2_and_rank3(env, monkeypatch, combiner, default_id):
  torch, de = env
  rng = np.random.default_rng(10 + COMB[combiner])
  var = filled_var(torch, de, "pls_%s_%s" % (combiner, default_id), initializer=0.25)
  n_rows = 200
  seg, ids, w = sparse_case(rng, n_rows)
  seg_t, ids_t, w_t = T(torch, seg), T(torch, ids), T(torch, w)
  exp2 = explicit_safe(torch, de, var, seg_t, ids_t, w_t, combiner, n_rows, default_id)
  # rank 3: [10, 20, 9] — row = i * 20 + j, column = the entry's rank in its row
  col = np.concatenate([np.arange(c) for c in np.bincount(seg, minlength=n_rows)]).astype(np.int64)
  ind3 = T(torch, np.stack([seg // 20, seg % 20, col], 1))
  calls = Calls(monkeypatch)
  got2 = de.safe_embedding_lookup_sparse(var, (seg_t, ids_t, [n_rows, 9]), w_t, combiner=combiner, default_id=default_id)
  got3 = de.safe_embedding_lookup_sparse(var, (ind3, ids_t, [10, 20, 9]), w_t, combiner=combiner, default_id=default_id)
  assert calls["tfra_table_find_combine"] == 2 and calls["tfra_unique"] == 0
  assert torch.equal(bits(torch, got2), bits(torch, exp2))
  assert tuple(got3.shape) == (10, 20, 64)
  assert torch.equal(bits(torch, got3.reshape(n_rows, 64)), bits(torch, exp2))


@pytest.mark.parametrize("why", ["max_norm", "dim6", "shards2", "callable_init", "bp_v2"])
def test_ineligible_variables_keep_the_op_chain(env, monkeypatch, why):
  torch, de = env
  rng = np.random.default_rng(3)
  n_rows = 200
  seg, ids, w = sparse_case(rng, n_rows)
  dim = 6 if why == "dim6" else 8
  kw = dict(initializer=0.5)
  if why == "shards2":
    kw["devices"] = ["cuda:0", "cuda:0"]
  if why == "callable_init":
    kw["initializer"] = lambda shape: torch.full(tuple(shape), 0.5)
  if why == "bp_v2":
    kw["bp_v2"] = True
  var = filled_var(torch, de, "pli_" + why, dim=dim, **kw)
  max_norm = 0.7 if why == "max_norm" else None
  seg_t, ids_t, w_t = T(torch, seg), T(torch, ids), T(torch, w)
  calls = Calls(monkeypatch)
  got = de.embedding_lookup_sparse(var, (seg_t, ids_t), w_t, combiner="mean", num_rows=n_rows, max_norm=max_norm)
  assert calls["tfra_table_find_combine"] == 0 and calls["tfra_unique"] == 1 and calls["tfra_sparse_segment_combine"] == 1
  # correct: float64 numpy over the rows a plain lookup returns (clipped to max_norm where set)
  E = var.lookup(ids_t).to(torch.float32).cpu().numpy().astype(np.float64)
  if max_norm is not None:
    nrm = np.linalg.norm(E, axis=1, keepdims=True)
    E = E * (max_norm / np.maximum(nrm, max_norm))
  den = np.zeros(n_rows)
  np.add.at(den, seg, w.astype(np.float64))
  # (a row of ~4 N(0,1) weights can sum close to 0: the error of its mean scales with sum |w| / |sum w|)
  amp = np.zeros(n_rows)
  np.add.at(amp, seg, np.abs(w.astype(np.float64)))
  exp = np_forward(E, seg, w, "mean", n_rows)
  g = got.cpu().numpy().astype(np.float64)
  tol = 1e-6 * (1 + (amp / np.where(den != 0, np.abs(den), 1))[:, None] * np.abs(E).max())
  assert np.all(np.abs(g - exp) <= tol)


# ---- 4. training through the pooled forward ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_training_step_never_runs_unique_and_matches_the_chain(env, monkeypatch, name):
  torch, de = env
  rng = np.random.default_rng(21)
  dim, n_rows = 64, 2048
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), 8)
  ids = (rng.zipf(1.2, size=seg.size) % 100000).astype(np.int64)
  w = rng.uniform(0.0, 2.0, size=seg.size).astype(np.float32)
  w[seg == 3] = 0.0
  seg_t, ids_t, w_t = T(torch, seg), T(torch, ids), T(torch, w)
  G = T(torch, (rng.standard_normal((n_rows, dim)) * 0.01).astype(np.float32))
  mk = {"sgd": lambda: de.optimizers.SGD(0.1), "adam": lambda: de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)}[name]
  opt = mk()
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  va = de.Variable(dim=dim, name="plt_a_" + name, initializer=0.5, **kw)
  vb = de.Variable(dim=dim, name="plt_b_" + name, initializer=0.5, **kw)
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  for step in range(2):
    # twin B: the forward as the op chain, its wrapper built as the chain's route builds it (eager unique + lookup)
    uniq, idx, cnt = de.device_ops.unique(ids_t)
    twb = de.SparseTrainableWrapper(vb, uniq.reshape(-1), idx, cnt, seg_t, w_t, "mean", n_rows, (n_rows, dim), ids_t, seg_t, w_t)
    out_b = de.device_ops.sparse_segment_combine(twb.read_value(), idx, seg_t, w_t, "mean", n_rows)
    db.apply_combined_gradients([(G, twb)])
    calls = Calls(monkeypatch)
    out_a, tw = de.embedding_lookup_sparse(va, (seg_t, ids_t), w_t, combiner="mean", return_trainable=True, num_rows=n_rows,
                                           plan_writeback=(step == 0))
    da.apply_combined_gradients([(G, tw)])
    assert calls["tfra_table_find_combine"] == 1 and calls["tfra_unique"] == 0 and calls["tfra_table_find"] == 0
    assert torch.equal(bits(torch, out_a), bits(torch, out_b))
    monkeypatch.undo()
    sa, sb = _export_state(torch, de, da, opt, va), _export_state(torch, de, db, opt, vb)
    assert len(sa) == len(sb) == 2 + len(opt.slots)
    for x, y in zip(sa, sb):
      assert torch.equal(x, y)
    # the wrapper's lazy half, after the step: today's values (tf.unique order; the rows the table holds now)
    assert torch.equal(tw.ids, uniq.reshape(-1))
    assert torch.equal(tw._idx, idx) and int(tw._n_unique) == int(cnt) and tw.exists is None
    assert torch.equal(bits(torch, tw.read_value()), bits(torch, va.lookup(uniq)))
    eg = de.device_ops.sparse_segment_combine_backprop(G, seg_t, w_t, "mean")
    exp_g = de.device_ops.segment_sum(eg, idx, cnt, ids_t.numel())
    u = int(cnt)
    assert torch.equal(bits(torch, tw.grad_of(G)[:u]), bits(torch, exp_g[:u]))


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,vdtype", [(6, "float32"), (260, "float32"), (8, "int8")])
def test_unsupported_tables_are_refused_and_write_nothing(env, dim, vdtype):
  torch, de = env
  from tfra_amd import _capi
  dt = getattr(torch, vdtype)
  t = de.CuckooHashTable(torch.int64, dt, torch.zeros(dim, dtype=dt), name="ple_%d_%s" % (dim, vdtype), dim=dim)
  t.insert(torch.arange(8, device="cuda"), torch.ones((8, dim), device="cuda").to(dt))
  ids_t = torch.arange(8, device="cuda")
  seg_t = torch.arange(8, device="cuda") // 2
  out = torch.full((4, dim), 7.0, device="cuda")
  for nnz in (8, 0):
    assert _raw_find_combine(torch, de, t, nnz, ids_t, seg_t, 4, out) == UNSUPPORTED
    assert _capi.lib().tfra_last_error()
  torch.cuda.synchronize()
  assert bool((out == 7.0).all())
  with pytest.raises(_capi.TfraError) as e:
    t._table.find_combine(ids_t, seg_t, None, 0, 4)
  assert e.value.code == UNSUPPORTED
  t._table.check_errors()


def test_argument_errors_and_empty_calls(env):
  torch, de = env
  t = table(torch, de, "cuckoo", "float32", 64)
  none = torch.empty(0, dtype=torch.int64, device="cuda")
  out = t._table.find_combine(none, none, None, 1, 5)
  assert tuple(out.shape) == (5, 64) and not bool(out.any())         # nnz == 0: zeros
  out = t._table.find_combine(none, none, None, 2, 0)
  assert tuple(out.shape) == (0, 64)                                 # n_rows == 0 with nnz == 0
  ids_t = torch.arange(4, device="cuda")
  seg_t = torch.tensor([7, 8, 9, 9], device="cuda")
  out = t._table.find_combine(ids_t, seg_t, None, 0, 3)
  assert not bool(out.any())                                         # every entry out of range
  buf = torch.full((3, 64), 7.0, device="cuda")
  assert _raw_find_combine(torch, de, t, 4, ids_t, seg_t, 3, buf, combiner=3) == -1   # TFRA_ERR_INVALID
  assert _raw_find_combine(torch, de, t, 4, None, seg_t, 3, buf) == -1
  torch.cuda.synchronize()
  assert bool((buf == 7.0).all())
  with pytest.raises(ValueError):
    t._table.find_combine(ids_t, seg_t[:3], None, 0, 3)
  with pytest.raises(ValueError):
    t._table.find_combine(ids_t, seg_t, torch.ones(3, device="cuda"), 0, 3)
  with pytest.raises(TypeError):
    t._table.find_combine(ids_t.to(torch.int32), seg_t, None, 0, 3)
  t._table.check_errors()
