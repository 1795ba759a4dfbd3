"""GPU: training through embedding_lookup_sparse / safe_embedding_lookup_sparse — the combiner's backward
(tfra_sparse_segment_combine_backprop) against a float64 numpy restatement of TF's SparseSegment*Grad, the reference's
common_minimize_trainable cases against a numpy branch + oracle.optimizers, and the fused write-back
(tfra_table_apply_planned_combined) against backprop + apply_sparse, bit for bit."""
import numpy as np
import pytest

import oracle
from oracle import optimizers as oopt

pytestmark = pytest.mark.gpu

COMB = {"sum": 0, "mean": 1, "sqrtn": 2}


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- numpy restatement of the backward (TF: gather, *= weights, segment_sum, / weight_sum or / sqrt(sum w^2)) ----------
def np_backprop(G, seg, w, combiner):
  """float64: g_e = G[seg[e]] / den_r * w_e; den = 1 | sum w | sqrt(sum w^2); a row with weight sum 0 gives 0."""
  G = G.astype(np.float64)
  nnz = seg.size
  w = np.ones(nnz) if w is None else w.astype(np.float64)
  n_rows = G.shape[0]
  if combiner == "sum":
    den = np.ones(n_rows)
  else:
    den = np.zeros(n_rows)
    np.add.at(den, seg, w if combiner == "mean" else w * w)
    if combiner == "sqrtn":
      den = np.sqrt(den)
  d = den[seg]
  safe = np.where(d != 0, d, 1.0)
  out = G[seg] / safe[:, None] * w[:, None]
  out[d == 0] = 0.0
  return out


def np_backprop_f32(G, seg, w, combiner):
  """The same in float32 and in the operation order the library states ((G / den) * w, den summed in entry order): the
  entry gradients the numpy training branch feeds oracle.optimizers."""
  G = G.astype(np.float32)
  w = np.ones(seg.size, np.float32) if w is None else w.astype(np.float32)
  den = np.ones(G.shape[0], np.float32)
  if combiner != "sum":
    den = np.zeros(G.shape[0], np.float32)
    for e in range(seg.size):
      den[seg[e]] = np.float32(den[seg[e]] + (w[e] if combiner == "mean" else w[e] * w[e]))
    if combiner == "sqrtn":
      den = np.sqrt(den).astype(np.float32)
  d = den[seg]
  out = ((G[seg] / np.where(d != 0, d, np.float32(1))[:, None]).astype(np.float32) * w[:, None]).astype(np.float32)
  out[d == 0] = 0.0
  return out


def np_unsorted_segment_sum(x, idx, n):
  out = np.zeros((n, x.shape[1]), np.float64)
  np.add.at(out, idx, x)
  return out


def make_batch(rng, n_rows, per_row_max, id_hi, weighted):
  counts = rng.integers(0, per_row_max + 1, size=n_rows)
  counts[0] = 0                               # an empty row
  counts[min(1, n_rows - 1)] = per_row_max    # a full one
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = rng.integers(0, id_hi, size=seg.size).astype(np.int64)
  if seg.size > 3:
    ids[1] = ids[0]                           # repeats within and across rows
    ids[-1] = ids[0]
  w = None
  if weighted:
    w = rng.uniform(0.1, 2.0, size=seg.size).astype(np.float32)
    zr = 2 if n_rows > 2 else n_rows - 1
    w[seg == zr] = 0.0                        # a row whose weight sum is 0
  return seg, ids, w


@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dim", [1, 4, 10, 64, 130, 256])
def test_backprop_kernel_matches_numpy(env, combiner, weighted, dim):
  torch, de = env
  rng = np.random.default_rng(dim * 7 + COMB[combiner] * 2 + weighted)
  n_rows = 300
  seg, ids, w = make_batch(rng, n_rows, 6, 40, weighted)
  G = rng.standard_normal((n_rows, dim)).astype(np.float32)
  wt = None if w is None else T(torch, w)
  got = de.device_ops.sparse_segment_combine_backprop(T(torch, G), T(torch, seg), wt, combiner)
  again = de.device_ops.sparse_segment_combine_backprop(T(torch, G), T(torch, seg), wt, combiner)
  exp = np_backprop(G, seg, w, combiner)
  np.testing.assert_allclose(got.cpu().numpy(), exp, rtol=1e-6, atol=1e-6)
  np.testing.assert_array_equal(got.cpu().numpy(), again.cpu().numpy())
  # composed with unsorted_segment_sum over the lookup's idx: the gradient of the trainable's rows (grad_of)
  var = de.Variable(dim=dim, name="bp_%s_%d_%d" % (combiner, weighted, dim), initializer=0.5)
  out, tw = de.embedding_lookup_sparse(var, (T(torch, seg), T(torch, ids)), wt, combiner=combiner, return_trainable=True,
                                       num_rows=n_rows)
  assert isinstance(tw, de.SparseTrainableWrapper)
  uniq = tw.ids.cpu().numpy()
  pos = {k: i for i, k in enumerate(uniq)}
  idx = np.array([pos[k] for k in ids], np.int64)
  gu = tw.grad_of(T(torch, G))
  # (fp32 sums of ~25 entries of magnitude ~3 per id against float64: the bound of the summation, not of the kernel)
  np.testing.assert_allclose(gu.cpu().numpy(), np_unsorted_segment_sum(exp, idx, uniq.size), rtol=1e-6, atol=1e-5)


# ---- the reference's common_minimize_trainable, restated ---------------------------------------------------------------
OPTS = {
    "sgd": (lambda de: de.optimizers.SGD(0.1), dict(lr=0.1)),
    "adam": (lambda de: de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8), dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)),
    "adagrad": (lambda de: de.optimizers.Adagrad(0.05, 0.1), dict(lr=0.05, init_acc=0.1)),
    "ftrl": (lambda de: de.optimizers.Ftrl(0.05, -0.5, 0.1, 1e-3, 1e-3), dict(lr=0.05, l1=1e-3, l2=1e-3, init_acc=0.1)),
    "ftrl_pow": (lambda de: de.optimizers.Ftrl(0.05, -0.3, 0.1, 0.0, 1e-3), dict(lr=0.05, l1=0.0, l2=1e-3, init_acc=0.1, lr_power=-0.3)),
    "momentum": (lambda de: de.optimizers.Momentum(0.05, 0.9), dict(lr=0.05, momentum=0.9)),
}
INIT_IDS = np.arange(10, dtype=np.int64)
INIT_VALS = np.array([0.0, 0.1, 0.3, 0.8, 0.16, 0.25, 0.36, 0.49, 0.64, 0.81], np.float32)


def _case(kind):
  """(indices, ids, weights, dense_shape, lookup kwargs) of one restated case."""
  ind2 = np.array([[0, 0], [0, 1], [1, 0], [2, 1]], np.int64)
  ids = np.array([1, 3, 3, 9], np.int64)
  if kind == "els":
    return ind2, ids, None, [3, 2], dict(combiner="sum")
  if kind == "els_w":
    return ind2, ids, np.array([0.5, 1.5, 2.0, 0.25], np.float32), [3, 2], dict(combiner="mean")
  if kind == "safe_r2_default":   # row 1 pruned (weight <= 0) -> empty -> default_id
    return ind2, ids, np.array([1.0, 2.0, -1.0, 0.5], np.float32), [3, 2], dict(combiner="mean", default_id=4)
  if kind == "safe_r2_none":      # rows 1 and 3 empty, default_id=None: key 0 reaches the write-back with a zero gradient
    ind = np.array([[0, 0], [0, 1], [2, 1]], np.int64)
    return ind, np.array([1, 3, 9], np.int64), None, [4, 2], dict(combiner="sqrtn", default_id=None)
  if kind == "safe_r3":           # rank 3, pruned entries, default id
    ind = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 1, 1]], np.int64)
    return ind, ids, np.array([1.0, 0.0, 2.0, 3.0], np.float32), [2, 2, 2], dict(combiner="sqrtn", default_id=7)
  raise ValueError(kind)


def _np_entries(ind, ids, w, shape, kw, safe):
  """The entry list of the numpy branch: rows (row-major over the leading dims), ids, weights, n_rows, combiner, and
  per entry whether it is a default entry whose gradient the reference's `where` zeroes."""
  lead = shape[:-1]
  rows = np.zeros(ind.shape[0], np.int64)
  for d in range(len(lead)):
    rows = rows * lead[d] + ind[:, d]
  n = int(np.prod(lead))
  comb = kw["combiner"]
  ww = np.ones(ids.size, np.float32) if w is None else w.copy()
  if safe and w is not None and comb != "sum":
    keep = ww > 0
    rows, ids, ww = rows[keep], ids[keep], ww[keep]
  zero = np.zeros(ids.size, bool)
  if safe:
    empty = np.setdiff1d(np.arange(n), rows)
    did = kw.get("default_id")
    rows = np.concatenate([rows, empty])
    ids = np.concatenate([ids, np.full(empty.size, 0 if did is None else did, np.int64)])
    ww = np.concatenate([ww, np.ones(empty.size, np.float32)])
    zero = np.concatenate([zero, np.full(empty.size, did is None)])
    o = np.argsort(rows, kind="stable")
    rows, ids, ww, zero = rows[o], ids[o], ww[o], zero[o]
  return rows, ids, ww, n, comb, zero


def _np_forward(tab, rows, ids, ww, n, comb, zero, dim, init):
  E = tab.find(ids, np.full(dim, init, np.float32)).astype(np.float64)
  out = np.zeros((n, dim))
  np.add.at(out, rows, E * ww[:, None])
  if comb != "sum":
    den = np.zeros(n)
    np.add.at(den, rows, ww if comb == "mean" else ww.astype(np.float64) ** 2)
    den = den if comb == "mean" else np.sqrt(den)
    out = np.where(den[:, None] != 0, out / np.where(den != 0, den, 1)[:, None], 0)
  zr = np.unique(rows[zero])
  out[zr] = 0.0
  return out


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("dim", [1, 10, 64])
@pytest.mark.parametrize("kind", ["els", "els_w", "safe_r2_default", "safe_r2_none", "safe_r3"])
def test_common_minimize_trainable(env, name, shards, dim, kind):
  torch, de = env
  mk, hyper = OPTS[name]
  opt = mk(de)
  init = 0.0
  var = de.Variable(dim=dim, name="cmt_%s_%d_%d_%s" % (name, shards, dim, kind), initializer=init, devices=["cuda:0"] * shards,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
  deo = de.DynamicEmbeddingOptimizer(opt)
  init_rows = np.repeat(INIT_VALS[:, None], dim, 1)
  var.upsert(T(torch, INIT_IDS), T(torch, init_rows))
  ind, ids, w, shape, kw = _case(kind)
  safe = kind.startswith("safe")
  tabs = [oracle.CpuTable(dim) for _ in range(1 + len(opt.slots))]
  tabs[0].insert(INIT_IDS, init_rows)
  okind = "ftrl" if name.startswith("ftrl") else name
  ora = oopt.SparseOptimizerOracle(okind, tabs[0], tabs[1:], hyper, init)
  rows, eids, ww, n, comb, zero = _np_entries(ind, ids, w, shape, kw, safe)
  out_shape = tuple(shape[:-1]) + (dim,)
  xv = np.concatenate([np.full(dim, v, np.float32) for v in np.resize(np.array([0.4, 0.5, 0.6], np.float32), n)])
  for _ in range(10):
    if safe:
      sp = (T(torch, ind), T(torch, ids), shape)
      out, tw = de.safe_embedding_lookup_sparse(var, sp, None if w is None else T(torch, w), return_trainable=True, **kw)
    else:
      out, tw = de.embedding_lookup_sparse(var, (T(torch, ind), T(torch, ids)), None if w is None else T(torch, w),
                                           return_trainable=True, **kw)
    assert tuple(out.shape) == out_shape
    # numpy branch: forward, loss = pred^2 with pred = out.flatten() @ x, so d loss / d out = 2 pred x.  Both branches take
    # this one grad_out (a gradient derived from each side's own forward would feed rounding back into the next step).
    o_np = _np_forward(tabs[0], rows, eids, ww, n, comb, zero, dim, init)
    np.testing.assert_allclose(out.reshape(n, dim).cpu().numpy(), o_np, rtol=1e-5, atol=1e-6)
    p_np = float(o_np.reshape(-1) @ xv.astype(np.float64))
    G = (2 * p_np * xv).astype(np.float32).reshape(n, dim)
    deo.apply_combined_gradients([(T(torch, G.reshape(out_shape)), tw)])
    eg = np_backprop_f32(G, rows, np.where(zero, np.float32(0), ww), comb)   # (a zeroed default entry: weight 0, as the library)
    eg[zero] = 0.0
    ora.apply(eids, eg)
  tol = 5e-6 if name == "ftrl_pow" else 1e-6
  k, v = var.export()
  k = k.cpu().numpy()
  o = np.argsort(k)
  ek, ev = tabs[0].export_sorted()
  np.testing.assert_array_equal(k[o], ek)
  if kind == "safe_r2_none":
    assert 0 in set(ek.tolist())      # key 0 inserted by the write-back, as in the reference
  np.testing.assert_allclose(v.cpu().numpy()[o], ev, rtol=tol, atol=tol)
  for si, sname in enumerate(opt.slots):
    got = deo.get_slot(var, sname).lookup(T(torch, ek)).cpu().numpy()
    # (keys no step touched hold the slot's initial value, as a row upserted before training does)
    np.testing.assert_allclose(got, tabs[1 + si].find(ek, np.full(dim, opt.aux_init()[si], np.float32)), rtol=tol, atol=tol)


# ---- fused write-back vs backprop + apply_sparse, bit for bit ----------------------------------------------------------
def _zipf_batch(rng, n_rows=16384, per_row=8, hi=2000000):
  ids = (rng.zipf(1.2, size=n_rows * per_row) % hi).astype(np.int64)
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), per_row)
  w = rng.uniform(0.0, 2.0, size=ids.size).astype(np.float32)
  w[seg == 3] = 0.0
  return seg, ids, w


def _twins(torch, de, name, opt, dim, bounded):
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  vs = []
  for i in range(2):
    if bounded:
      cap = 65536
      v = de.get_variable("fz_%s_%d_b%d" % (name, dim, i), key_dtype=torch.int64, value_dtype=torch.float32, initializer=0.5, dim=dim,
                          init_size=cap, kv_creator=de.HkvHashTableCreator(config=de.HkvHashTableConfig(
                              init_capacity=cap, max_capacity=cap, max_hbm_for_values=1 << 28,
                              evict_strategy=de.HkvEvictStrategy.LRU)), **kw)
    else:
      v = de.Variable(dim=dim, name="fz_%s_%d_g%d" % (name, dim, i), initializer=0.5, **kw)
    vs.append(v)
  return vs


def _state(torch, de, deo, opt, var, keys):
  k, v = var.export()
  k = k.cpu().numpy()
  o = np.argsort(k)
  slots = [deo.get_slot(var, s).lookup(T(torch, keys)).cpu().numpy() for s in opt.slots]
  return k[o], v.cpu().numpy()[o], slots


@pytest.mark.parametrize("name", ["sgd", "adam", "adagrad", "ftrl"])
@pytest.mark.parametrize("bounded", [False, True])
def test_fused_matches_backprop_apply_sparse_bitwise(env, name, bounded):
  torch, de = env
  dim = 64
  rng = np.random.default_rng(11 + bounded)
  opt = OPTS[name][0](de)
  va, vb = _twins(torch, de, name, opt, dim, bounded)
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  if bounded:   # at capacity before the batch: every new key of the batch takes the eviction path (PHASE2)
    old = -np.arange(1, 80001, dtype=np.int64)
    for v in (va, vb):
      v.upsert(T(torch, old), torch.full((old.size, dim), 0.25, device="cuda"))
      assert int(v.size()) > 0.9 * 65536
  for step in range(1 if bounded else 3):
    seg, ids, w = _zipf_batch(rng)
    _, c = np.unique(ids, return_counts=True)
    assert c.max() > 512 and (c > 8).sum() > 10      # hot bins and hot keys
    G = T(torch, (rng.standard_normal((16384, dim)) * 0.01).astype(np.float32))
    st, it, wt = T(torch, seg), T(torch, ids), T(torch, w)
    # A: fused (plan at lookup on even steps, at apply time on odd ones)
    _, tw = de.embedding_lookup_sparse(va, (st, it), wt, combiner="mean", return_trainable=True, num_rows=16384,
                                       plan_writeback=(step % 2 == 0))
    if step % 2 == 0:
      assert tw.entry_plan is not None
    da.apply_combined_gradients([(G, tw)])
    # B: backprop + apply_sparse over the entry ids
    eg = de.device_ops.sparse_segment_combine_backprop(G, st, wt, "mean")
    db.apply_sparse(vb, it, eg)
    keys = np.unique(ids)
    if bounded:
      # WHICH old key a new one evicts depends on the order the key groups run in (as for apply_sparse itself): the twins
      # are compared on the batch's keys both hold
      assert int(va.size()) <= 65536 and int(vb.size()) <= 65536
      ka0, kb0 = va.export()[0].cpu().numpy(), vb.export()[0].cpu().numpy()
      keys = np.intersect1d(np.intersect1d(ka0, kb0), keys)
      assert keys.size > 0.9 * np.unique(ids).size
      ra = va.lookup(T(torch, keys)).cpu().numpy()
      rb = vb.lookup(T(torch, keys)).cpu().numpy()
      sa = [da.get_slot(va, s).lookup(T(torch, keys)).cpu().numpy() for s in opt.slots]
      sb = [db.get_slot(vb, s).lookup(T(torch, keys)).cpu().numpy() for s in opt.slots]
    else:
      ka, ra, sa = _state(torch, de, da, opt, va, keys)
      kb, rb, sb = _state(torch, de, db, opt, vb, keys)
      np.testing.assert_array_equal(ka, kb)
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32))
    for x, y in zip(sa, sb):
      np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_lookup_plan_same_bits_as_apply_plan(env):
  torch, de = env
  dim = 64
  rng = np.random.default_rng(5)
  opt = de.optimizers.Adam(1e-3)
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs(opt)
  va = de.Variable(dim=dim, name="lp_a", initializer=0.5, **kw)
  vb = de.Variable(dim=dim, name="lp_b", initializer=0.5, **kw)
  da, db = de.DynamicEmbeddingOptimizer(opt), de.DynamicEmbeddingOptimizer(opt)
  seg, ids, w = _zipf_batch(rng)
  G = T(torch, (rng.standard_normal((16384, dim)) * 0.01).astype(np.float32))
  st, it, wt = T(torch, seg), T(torch, ids), T(torch, w)
  for var, deo, pw in ((va, da, True), (vb, db, False)):
    _, tw = de.embedding_lookup_sparse(var, (st, it), wt, combiner="sqrtn", return_trainable=True, num_rows=16384, plan_writeback=pw)
    assert (tw.entry_plan is not None) == pw
    deo.apply_combined_gradients([(G, tw)])
  keys = np.unique(ids)
  a, b = _state(torch, de, da, opt, va, keys), _state(torch, de, db, opt, vb, keys)
  np.testing.assert_array_equal(a[0], b[0])
  np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
  for x, y in zip(a[2], b[2]):
    np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- error paths, and a batch too large for one plan ---------------------------------------------------------------------
def test_error_paths(env):
  torch, de = env
  opt = de.optimizers.SGD(0.1)
  var = de.Variable(dim=4, name="err_v", initializer=0.0)
  deo = de.DynamicEmbeddingOptimizer(opt)
  ids = T(torch, np.array([1, 2, 2], np.int64))
  _, tw_plain = de.embedding_lookup(var, ids, return_trainable=True)
  with pytest.raises(TypeError):
    deo.apply_combined_gradients([(torch.zeros(3, 4, device="cuda"), tw_plain)])
  seg = T(torch, np.array([0, 0, 1], np.int64))
  _, tw = de.embedding_lookup_sparse(var, (seg, ids), None, combiner="mean", return_trainable=True)
  with pytest.raises(ValueError, match="shape"):
    deo.apply_combined_gradients([(torch.zeros(3, 4, device="cuda"), tw)])
  _, twn = de.embedding_lookup_sparse(var, (seg, ids), None, combiner="mean", return_trainable=True, max_norm=1.0)
  with pytest.raises(ValueError, match="max_norm"):
    deo.apply_combined_gradients([(torch.zeros(2, 4, device="cuda"), twn)])
  assert deo.iterations == 0     # nothing was applied


def test_more_than_2_18_entries_fallback_vs_oracle(env):
  torch, de = env
  dim = 8
  rng = np.random.default_rng(3)
  n_rows, per = 40000, 7                # 280 000 entries > 2^18: backprop + apply_sparse
  seg = np.repeat(np.arange(n_rows, dtype=np.int64), per)
  ids = (rng.zipf(1.2, size=seg.size) % 50000).astype(np.int64)
  w = rng.uniform(0.1, 1.0, size=seg.size).astype(np.float32)
  opt = de.optimizers.Adagrad(0.05, 0.1)
  var = de.Variable(dim=dim, name="big_fb", initializer=0.25, **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
  deo = de.DynamicEmbeddingOptimizer(opt)
  _, tw = de.embedding_lookup_sparse(var, (T(torch, seg), T(torch, ids)), T(torch, w), combiner="sum", return_trainable=True,
                                     num_rows=n_rows)
  G = (rng.standard_normal((n_rows, dim)) * 0.01).astype(np.float32)
  deo.apply_combined_gradients([(T(torch, G), tw)])
  tabs = [oracle.CpuTable(dim) for _ in range(2)]
  ora = oopt.SparseOptimizerOracle("adagrad", tabs[0], tabs[1:], dict(lr=0.05, init_acc=0.1), 0.25)
  ora.apply(ids, np_backprop(G, seg, w, "sum").astype(np.float32))
  k, v = var.export()
  k = k.cpu().numpy()
  o = np.argsort(k)
  ek, ev = tabs[0].export_sorted()
  np.testing.assert_array_equal(k[o], ek)
  np.testing.assert_allclose(v.cpu().numpy()[o], ev, rtol=1e-6, atol=1e-6)
