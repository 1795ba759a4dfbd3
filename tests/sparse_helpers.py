"""Helpers that more than one GPU test module of the sparse lookups and write-backs uses (a plain module: no fixtures, no tests).

The pooled-lookup part (tests/test_gpu_pooled_lookup.py and the grouped lookups): one Zipf batch per size and one filled table per
(kind, value dtype, dim), shared by every case.  The write-back part (tests/test_gpu_combined_many.py, the grouped plan builds and
the error-parity cases): `Case`, a table of a grouped call with its twin driven through the single call."""
import ctypes

import numpy as np

IMIN = np.iinfo(np.int64).min
COMB = {"sum": 0, "mean": 1, "sqrtn": 2}


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(torch, x):
  return x.contiguous().view(torch.int32)


class Calls:
  """Counts _capi.call by C function name."""

  def __init__(self, monkeypatch):
    from tfra_amd import _capi
    self.n = {}
    real = _capi.call

    def counting(name, *args):
      self.n[name] = self.n.get(name, 0) + 1
      return real(name, *args)

    monkeypatch.setattr(_capi, "call", counting)

  def __getitem__(self, name):
    return self.n.get(name, 0)


def _export_state(torch, de, deo, opt, var):
  k, v = var.export()
  o = torch.argsort(k)
  k = k[o]
  return [k, bits(torch, v[o])] + [bits(torch, deo.get_slot(var, s).lookup(k)) for s in opt.slots]


# ---- one batch per size, shared by every case ----------------------------------------------------------------------------
POOL_UNIVERSE = 6000          # distinct keys the ids are drawn from; every fifth one is never inserted


def _universe():
  rng = np.random.default_rng(1234)
  keys = rng.permutation(np.arange(1, POOL_UNIVERSE + 1, dtype=np.int64) * 7919 - 3_000_000)   # negative keys too
  inserted = keys[np.arange(POOL_UNIVERSE) % 5 != 0]          # rank r of the Zipf law -> keys[r]: misses at every frequency
  return keys, np.concatenate([inserted, [IMIN]])         # INT64_MIN is resident (its side row), INT64_MIN + 1 is not


def _batch(nnz, n_rows, long_row):
  """(ids, seg, w): Zipf ids with ~20 % never-inserted keys and both reserved key values; seg ascending with empty rows at the
  start, in the middle and at the end, a row of 1 entry, a row of `long_row` entries and 4 out-of-range values at the tail;
  weights with zeros and negatives, a row whose weights are all 0 and a row whose weights cancel."""
  rng = np.random.default_rng(nnz)
  keys, _ = _universe()
  counts = rng.integers(0, 24, size=n_rows)
  special = {0: 0, 1: 0, 2: 1, 3: long_row, 4: 2, 5: 3, n_rows // 2: 0, n_rows // 2 + 1: 0, n_rows - 2: 0, n_rows - 1: 0}
  for r, c in special.items():
    counts[r] = c
  free = np.setdiff1d(np.arange(n_rows), list(special))
  deficit = nnz - 4 - int(counts.sum())
  assert deficit >= 0
  counts[free] += rng.multinomial(deficit, np.full(free.size, 1.0 / free.size))
  seg = np.concatenate([np.repeat(np.arange(n_rows), counts), [n_rows, n_rows, n_rows + 5, 1 << 40]]).astype(np.int64)
  assert seg.size == nnz and np.all(np.diff(seg) >= 0)
  ids = keys[(rng.zipf(1.2, size=nnz) - 1) % POOL_UNIVERSE]
  ids[5], ids[nnz // 2], ids[7], ids[nnz // 3] = IMIN, IMIN, IMIN + 1, IMIN + 1
  w = rng.standard_normal(nnz).astype(np.float32)
  w[rng.random(nnz) < 0.05] = 0.0
  w[seg == 4] = [1.0, -1.0]       # mean: weight sum 0 -> zeros; sqrtn: sqrt(2)
  w[seg == 5] = 0.0               # every combiner's weight sum is 0
  return ids, seg, w


_BATCHES = {}


def batch(torch, nnz, n_rows, long_row=2000):
  if (nnz, n_rows) not in _BATCHES:
    ids, seg, w = _batch(nnz, n_rows, long_row)
    _BATCHES[(nnz, n_rows)] = (ids, seg, w, T(torch, ids), T(torch, seg), T(torch, w))
  return _BATCHES[(nnz, n_rows)]


_TABLES = {}


def table(torch, de, kind, vdtype, dim):
  """A table of `kind` ("cuckoo": growing; "hkv": bounded, LRU) holding the inserted part of the universe, random rows."""
  key = (kind, vdtype, dim)
  if key not in _TABLES:
    dt = getattr(torch, vdtype)
    default = torch.full((dim,), 0.375, dtype=dt)
    if kind == "cuckoo":
      t = de.CuckooHashTable(torch.int64, dt, default, name="pl_c_%s_%d" % (vdtype, dim), dim=dim)
    else:
      t = de.HkvHashTable(torch.int64, dt, default, name="pl_h_%s_%d" % (vdtype, dim), init_capacity=8192, max_capacity=8192,
                          max_hbm_for_values=1 << 28, evict_strategy=de.HkvEvictStrategy.LRU, dim=dim)
    _, inserted = _universe()
    g = torch.Generator(device="cuda").manual_seed(dim)
    rows = torch.randn((inserted.size, dim), generator=g, device="cuda").to(dt)
    t.insert(T(torch, inserted), rows)
    _TABLES[key] = t
  return _TABLES[key]


def filled_var(torch, de, name, dim=64, key_dtype=None, scale=1, **kw):
  """A variable holding the even keys below 3000, rows N(0, scale^2) of a fixed seed."""
  var = de.Variable(dim=dim, name=name, key_dtype=key_dtype or torch.int64, **kw)
  keys = torch.arange(0, 3000, 2, device="cuda").to(var.key_dtype)
  g = torch.Generator(device="cuda").manual_seed(7)
  rows = torch.randn((keys.numel(), dim), generator=g, device="cuda")
  var.upsert(keys, (rows if scale == 1 else rows * scale).to(var.value_dtype))
  return var


def sparse_case(rng, n_rows=200, weighted=True):
  counts = rng.integers(0, 9, size=n_rows)
  counts[[0, 7, n_rows - 1]] = 0
  seg = np.repeat(np.arange(n_rows), counts).astype(np.int64)
  ids = (rng.zipf(1.3, size=seg.size) % 3000).astype(np.int64)
  w = rng.standard_normal(seg.size).astype(np.float32) if weighted else None
  return seg, ids, w


def _raw_find_combine(torch, de, t, nnz, ids_t, seg_t, n_rows, out, combiner=0):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  dev = t._table.device
  return _capi.lib().tfra_table_find_combine(t._table._h, _workspace(dev), nnz, _ptr(ids_t), _ptr(seg_t), None, combiner, n_rows,
                                             _ptr(t._default_value), _ptr(out), _stream(dev))


# ---- the grouped pooled lookup's raw call ----------------------------------------------------------------------------------------
def _raw(torch, descs, n=None, launches=None):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _stream
  dev = torch.device("cuda", torch.cuda.current_device())
  rc = _capi.lib().tfra_multi_find_combine(_workspace(dev), len(descs) if n is None else n,
                                           ctypes.c_void_p(ctypes.addressof(descs)) if descs is not None else None,
                                           ctypes.c_void_p(ctypes.addressof(launches)) if launches is not None else None, _stream(dev))
  return rc, _capi.lib().tfra_last_error().decode()


def _desc(e, t, ids, seg, n_rows, out, combiner=0):
  from tfra_amd import _capi
  e.struct_size = ctypes.sizeof(_capi.FindCombineDesc)
  e.combiner = combiner
  e.table = t._table._h.value if t is not None else None
  e.nnz, e.ids, e.seg, e.weights = ids.numel(), ids.data_ptr(), seg.data_ptr(), None
  e.n_rows, e.default_row, e.out = n_rows, (t._default_value.data_ptr() if t is not None else None), out.data_ptr()


# ---- the combined write-back: tables with twins ------------------------------------------------------------------------------
N_ROWS, PER_ROW, UNIVERSE, PLANTED = 256, 8, 500, 7


def opt_of(de, name):
  return {"sgd": lambda: de.optimizers.SGD(0.1), "adam": lambda: de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8),
          "adagrad": lambda: de.optimizers.Adagrad(0.05, 0.1), "ftrl": lambda: de.optimizers.Ftrl(0.05)}[name]()


def key_of(rank):
  return rank.astype(np.int64) * 7919 - 1_000_000


def make_var(torch, de, opt, name, dim, vdtype="float32", fill=True, **kw):
  """A one-shard variable with the rule's slots; holds the keys of rank % 5 != 0 (the others enter from the default row)."""
  var = de.Variable(dim=dim, name=name, initializer=0.5, value_dtype=getattr(torch, vdtype),
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt), **kw)
  if fill:
    r = np.arange(UNIVERSE)
    keys = T(torch, key_of(r[r % 5 != 0]))
    g = torch.Generator(device="cuda").manual_seed(dim)
    var.upsert(keys, torch.randn((keys.numel(), dim), generator=g, device="cuda").to(var.value_dtype))
  return var


_BATCH = {}


def writeback_batch(torch, seed, n_rows=N_ROWS, per_row=PER_ROW, planted=600):
  """(ids, seg, w): Zipf(1.2) % 500 ids, so that many keys occur more than 8 times (the partial-sum route), one id planted 600
  times (more than one 512-entry bin), ~20 % of the ids not resident, one row whose weights are all zero, three seg values
  >= n_rows at the tail."""
  if (seed, n_rows, per_row) not in _BATCH:
    rng = np.random.default_rng(seed)
    nnz = n_rows * per_row
    rank = (rng.zipf(1.2, size=nnz) - 1) % UNIVERSE
    if planted:
      rank[rng.choice(nnz, size=min(planted, nnz // 3), replace=False)] = PLANTED
    seg = np.repeat(np.arange(n_rows, dtype=np.int64), per_row)
    seg[-3:] = [n_rows, n_rows, n_rows + 44]
    w = rng.uniform(0.1, 2.0, size=nnz).astype(np.float32)
    w[seg == 5] = 0.0
    _BATCH[(seed, n_rows, per_row)] = (T(torch, key_of(rank)), T(torch, seg), T(torch, w))
  return _BATCH[(seed, n_rows, per_row)]


def grad(torch, seed, n_rows, dim, step=0):
  g = torch.Generator(device="cuda").manual_seed(1000 * seed + step)
  return torch.randn((n_rows, dim), generator=g, device="cuda") * 0.01


class Case:
  """One descriptor: the table of the grouped call, its twin, and the inputs both get."""

  def __init__(self, torch, de, opt, name, dim, vdtype="float32", comb="mean", weighted=True, seed=1, inputs=None, n_rows=None, **kw):
    from tfra_amd.dynamic_embedding.table_ops import SparsePlan
    self.var, self.twin = make_var(torch, de, opt, name + "_m", dim, vdtype, **kw), make_var(torch, de, opt, name + "_t", dim, vdtype, **kw)
    self.ids, self.seg, w = inputs if inputs is not None else writeback_batch(torch, seed)
    self.w = w if weighted else None
    self.comb, self.dim, self.seed = COMB[comb], dim, seed
    self.n_rows = n_rows if n_rows is not None else N_ROWS
    self.plan, self.plan_t = SparsePlan(self.var._primary, dim), SparsePlan(self.var._primary, dim)

  def table(self, twin=False):
    return (self.twin if twin else self.var)._tables[0]

  def G(self, torch, step):
    return grad(torch, self.seed, self.n_rows, self.dim, step)

  def request(self, torch, step, build=True):
    if build:
      self.plan.build(self.ids)
    t = self.table()
    return (t._table, self.plan, self.G(torch, step), self.seg, self.w, self.comb, t._default_value.to(torch.float32))

  def single(self, torch, p, step, build=True):
    if self.ids.numel() == 0:
      return   # (nothing to write; the single call takes no plan that was never built with ids)
    if build:
      self.plan_t.build(self.ids)
    t = self.table(True)
    t._table.apply_planned_combined(p, self.plan_t, self.G(torch, step), self.seg, self.w, self.comb, t._default_value.to(torch.float32))


def many(reqs, p):
  from tfra_amd.dynamic_embedding import table_ops
  return table_ops.apply_planned_combined_many(reqs, p)


def assert_twins(torch, de, opt, cases):
  deo = de.DynamicEmbeddingOptimizer(opt)
  for i, c in enumerate(cases):
    a, b = _export_state(torch, de, deo, opt, c.var), _export_state(torch, de, deo, opt, c.twin)
    assert len(a) == len(b) == 2 + len(opt.slots)
    for j, (x, y) in enumerate(zip(a, b)):
      assert torch.equal(x, y), "descriptor %d: field %d differs from the twin driven by the single call" % (i, j)
    c.table()._table.check_errors()
    c.table(True)._table.check_errors()


def desc_of(torch, req, p):
  from tfra_amd import _capi
  table, plan, G, seg, w, comb, d = req
  e = _capi.ApplyCombinedDesc()
  e.struct_size, e.combiner = ctypes.sizeof(_capi.ApplyCombinedDesc), int(comb)
  e.table, e.opt, e.plan = table._h.value, ctypes.addressof(p), plan._h.value
  e.grad_out, e.seg, e.weights = G.data_ptr(), seg.data_ptr(), (w.data_ptr() if w is not None else None)
  e.n_rows, e.param_default_row = G.shape[0], d.data_ptr()
  return e


def raw_many(torch, descs):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _stream
  arr = (_capi.ApplyCombinedDesc * max(1, len(descs)))(*descs)
  launches = ctypes.c_uint32(77)
  dev = torch.device("cuda", torch.cuda.current_device())
  rc = _capi.lib().tfra_multi_apply_planned_combined(_workspace(dev), len(descs), ctypes.c_void_p(ctypes.addressof(arr)),
                                                     ctypes.c_void_p(ctypes.addressof(launches)), _stream(dev))
  return rc, int(launches.value), _capi.lib().tfra_last_error().decode()
