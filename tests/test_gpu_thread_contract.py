"""GPU: host threads — the other half of the threading contract (include/tfra_mi355x.h; tests/test_gpu_concurrency.py drives
insert / lookup / remove / accum): any host thread may call any entry point on the same table, the library serialises host
state itself.  A tfra_workspace is NOT part of that: it serves one call at a time, so the Python layer keeps one per (host
thread, device, stream) — `device_ops._workspace`.  ctypes releases the GIL for the length of a C call; before the thread was
part of that key, two threads on the default stream were inside tfra_unique / tfra_reduce_by_key / the pooled lookups with ONE
workspace, whose scratch a growing call frees and whose set parity a call flips on the host.

  1. eight threads on the DEFAULT stream, each with a variable of its own, run the training and serving forms that take a
     workspace, with id lists that make the scratch grow; every output and the final tables equal the same steps on one thread,
     bit for bit;
  2. eight threads share one growing table through find_or_insert / assign / find_missed / find_combine / apply_sparse on
     disjoint key ranges; rows, export and the slot field equal a sequential NumPy model;
  3. two threads issue grouped calls over overlapping table lists in opposite orders: the lists are locked in address order, so
     this ends (a join timeout turns a deadlock into a failure)."""
import threading

import numpy as np
import pytest

import oracle
from oracle import optimizers as oopt
from tests import probe_model as pm

pytestmark = pytest.mark.gpu

JOIN_SECONDS = 120


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _run_threads(workers):
  """start, join with a timeout (a thread still alive then is a deadlock or a hang: the test fails instead of waiting), and
  hand back what the workers raised"""
  errors = []

  def guarded(w, fn):
    try:
      fn()
    except BaseException as e:  # noqa: BLE001
      errors.append("thread %d: %r" % (w, e))

  threads = [threading.Thread(target=guarded, args=(w, fn), daemon=True) for w, fn in enumerate(workers)]
  for th in threads:
    th.start()
  for th in threads:
    th.join(JOIN_SECONDS)
  stuck = [w for w, th in enumerate(threads) if th.is_alive()]
  assert not stuck, "threads %s did not finish within %d s" % (stuck, JOIN_SECONDS)
  assert not errors, errors[:3]


def _bytes(torch, x):
  return x.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


# ---- 0. the rule itself -------------------------------------------------------------------------------------------------------------
def test_a_workspace_belongs_to_one_thread_and_one_stream(env):
  """`device_ops._workspace`: the same handle for the same thread and stream, another one on another stream, and another one
  for another thread on the SAME (default) stream — two threads are never inside the library with one workspace."""
  torch, de = env
  dev = torch.device("cuda:0")
  ws = de.device_ops._workspace
  mine = ws(dev).value
  assert mine and ws(dev).value == mine
  with torch.cuda.stream(torch.cuda.Stream()):
    assert ws(dev).value != mine
  theirs = []
  both = threading.Barrier(2, timeout=JOIN_SECONDS)      # (a thread's workspaces go with it: compare while both threads live)

  def run():
    torch.cuda.set_device(0)
    assert torch.cuda.current_stream().cuda_stream == torch.cuda.default_stream().cuda_stream
    theirs.append((ws(dev).value, ws(dev).value))
    both.wait()
  _run_threads([run, run])
  (a, a2), (b, b2) = theirs
  assert a == a2 and b == b2 and len({mine, a, b}) == 3


# ---- 1. threads on the default stream -----------------------------------------------------------------------------------------
UNIVERSE, CAP, MAX_BATCH, STEPS = 3000, 15 * 89, 1024, 6
LENS = (257, 1000, 40000, 3001, 120000, 513)        # ids per step: the workspace's scratch has to grow, and is reused when they shrink
# (dim, value dtype, tiered)
CONFIGS = [(4, "float32", False), (8, "float32", False), (64, "float32", False), (4, "bfloat16", False), (8, "bfloat16", False),
           (64, "bfloat16", False), (8, "float32", True), (64, "float32", False)]


def _variable(env, w, tag):
  torch, de = env
  dim, dt, tiered = CONFIGS[w]
  opt = de.optimizers.Adam(0.05)
  creator = None
  if tiered:
    creator = de.TieredHashTableCreator(de.TieredHashTableConfig(
        upper=de.HkvHashTableConfig(init_capacity=CAP, max_capacity=CAP, evict_strategy=de.HkvEvictStrategy.LRU), max_batch=MAX_BATCH))
  var = de.Variable(dim=dim, value_dtype=getattr(torch, dt), name="tc_%s_%d" % (tag, w), initializer=0.25, kv_creator=creator,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
  return var, de.DynamicEmbeddingOptimizer(opt)


def _batches(w):
  """per step: (lookup ids, their gradients, entry ids, seg, weights, n_rows, the result's gradient, ids for unique) — numpy, a
  function of the thread's number alone"""
  dim, _, tiered = CONFIGS[w]
  rng = np.random.default_rng(9000 + w)
  universe = np.unique(rng.integers(1, 2**40, size=UNIVERSE + 50, dtype=np.int64))[:UNIVERSE]
  out = []
  for step in range(STEPS):
    n = 150 + 29 * step if tiered else LENS[(step + w) % STEPS]        # (a tiered lookup admits: at most max_batch distinct ids)
    ids = rng.choice(universe, size=n, replace=True)
    g = (rng.standard_normal((n, dim)) * 0.1).astype(np.float32)
    nnz, n_rows = 200 + 37 * step, 40 + step
    seg = np.sort(rng.integers(0, n_rows, size=nnz)).astype(np.int64)
    eids = rng.choice(universe, size=nnz, replace=True)
    wts = rng.standard_normal(nnz).astype(np.float32)                 # (the safe form prunes the ones that are not > 0)
    gout = (rng.standard_normal((n_rows, dim)) * 0.1).astype(np.float32)
    uq = rng.integers(0, 5000, size=LENS[(step + w) % STEPS]).astype(np.int64)
    if tiered:     # no batch saturates its own home buckets in the cache (tests/test_gpu_tier_sparse_variable.py)
      for batch in (ids, eids):
        b0, b1, _ = pm.homes(np.unique(batch), 89)
        load = np.bincount(np.concatenate([b0, b1]), minlength=89)
        assert not bool(((load[b0] >= 15) & (load[b1] >= 15)).any())
    out.append((ids, g, eids, seg, wts, n_rows, gout, uq))
  return universe, out


def _steps(env, var, deo, w, batches):
  """The six steps of thread `w` on the CURRENT stream -> every output as bytes, then the final whole rows and the size."""
  torch, de = env
  torch.cuda.set_device(0)
  universe, steps = batches
  T = lambda a: torch.from_numpy(a).cuda()
  outs = []
  for step, (ids, g, eids, seg, wts, n_rows, gout, uq) in enumerate(steps):
    combiner = ("mean", "sum", "sqrtn")[step % 3]
    # (each write-back directly behind its lookup: over a tier the lookup admits, and the write-back acts on the cache)
    emb, tw = de.embedding_lookup(var, T(ids), return_trainable=True)               # repeated ids: de-duplicated in a workspace
    outs.append(_bytes(torch, emb))
    deo.apply_gradients([(T(g), tw)])                                                # apply_sparse with Adam
    pooled, stw = de.embedding_lookup_sparse(var, (T(seg), T(eids)), T(wts), combiner=combiner, return_trainable=True, num_rows=n_rows)
    outs.append(_bytes(torch, pooled))
    deo.apply_combined_gradients([(T(gout), stw)])
    outs.append(_bytes(torch, de.safe_embedding_lookup_sparse(var, (T(seg), T(eids)), T(wts), combiner="mean", num_rows=n_rows)))
    u, idx, cnt = de.device_ops.unique(T(uq))
    outs += [_bytes(torch, u), _bytes(torch, idx), int(cnt.item())]
  seen = T(np.unique(np.concatenate([np.concatenate([s[0], s[2]]) for s in steps])))
  t = var.tables[0]
  if hasattr(t, "flush"):
    t.flush()
    table = t._lower
  else:
    table = t._table
  table.check_errors()
  assert bool(table.contains(seen).all())
  outs += [_bytes(torch, table.find(seen, field=f)) for f in range(var.aux_fields + 1)]
  outs.append(int(var.size()))
  torch.cuda.synchronize()
  return outs


def test_threads_on_the_default_stream_equal_one_thread(env):
  torch, _ = env
  nthreads = len(CONFIGS)
  batches = [_batches(w) for w in range(nthreads)]
  pairs = [_variable(env, w, "thr") for w in range(nthreads)]
  results = [None] * nthreads
  torch.cuda.synchronize()

  def worker(w):
    def run():
      assert torch.cuda.current_stream().cuda_stream == torch.cuda.default_stream().cuda_stream
      results[w] = _steps(env, pairs[w][0], pairs[w][1], w, batches[w])
    return run

  _run_threads([worker(w) for w in range(nthreads)])
  for w in range(nthreads):
    var, deo = _variable(env, w, "one")
    want = _steps(env, var, deo, w, batches[w])
    assert len(results[w]) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(results[w], want)) if a != b]
    assert not bad, "thread %d %s: outputs %s of %d differ from the one-thread run (6 per step: lookup, pooled, safe, unique x3)" % (
        w, CONFIGS[w], bad[:8], len(want))


# ---- 2. threads on one shared, growing table ----------------------------------------------------------------------------------------
DIM, PER, ROUNDS, NTHREADS, LR = 8, 2000, 6, 8, 0.5


def test_host_threads_share_one_table_through_the_newer_calls(env):
  """Every value is a small dyadic rational (rows k/8, gradients k/16, weights k/4, lr 1/2), so sums and updates are exact in
  float32 in any order: the NumPy model — oracle.CpuTable for the rows, oracle.optimizers.segment_sum_by_key and .sgd for the
  rule — is compared bit for bit."""
  torch, de = env
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.full((DIM,), -1.0), name="tc_shared", device="cuda:0", dim=DIM, init_size=64,
                         aux_fields=1, aux_init=(0.5, 0.0, 0.0, 0.0))
  dt = t._table
  p = de.optimizers.SGD(LR).params(1)
  default = torch.full((DIM,), -1.0, device="cuda")
  final = [[] for _ in range(NTHREADS)]
  T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

  def worker(w):
    def run():
      torch.cuda.set_device(0)
      s = torch.cuda.Stream()
      rng = np.random.default_rng(100 + w)
      with torch.cuda.stream(s):
        for r in range(ROUNDS):
          tag = "round %d" % r
          k = (np.arange(PER, dtype=np.int64) + (w * ROUNDS + r) * PER) * 104729 - 10**9
          absent = -(np.arange(300, dtype=np.int64) + (w * ROUNDS + r) * 300) * 7919 - 2 * 10**15
          v = rng.integers(-100, 100, size=(PER, DIM)).astype(np.float32) / np.float32(8)
          v2 = rng.integers(-100, 100, size=(PER, DIM)).astype(np.float32) / np.float32(8)
          kt = T(k)
          rows, ex = dt.find_or_insert(kt, init_values=T(v), return_exists=True)
          found = dt.assign(kt[:PER // 2], T(v2[:PER // 2]), return_found=True)
          cur = v.copy()
          cur[:PER // 2] = v2[:PER // 2]
          probe = np.concatenate([k[::3], absent])
          got, mk, mi = dt.find_missed(T(probe))
          nnz, n_rows = 1500, 200
          pos = rng.integers(0, PER, size=nnz)
          seg = np.sort(rng.integers(0, n_rows, size=nnz)).astype(np.int64)
          wts = rng.integers(1, 9, size=nnz).astype(np.float32) / np.float32(4)
          pooled = dt.find_combine(T(k[pos]), T(seg), T(wts), 0, n_rows)
          g = rng.integers(-32, 32, size=(nnz, DIM)).astype(np.float32) / np.float32(16)
          dt.apply_sparse(p, T(k[pos]), T(g), default)
          after = dt.find(kt)
          s.synchronize()
          assert not bool(ex.any()) and rows.cpu().numpy().tobytes() == v.tobytes(), tag + ": find_or_insert"
          assert bool(found.all()), tag + ": assign"
          want = np.concatenate([cur[::3], np.full((absent.size, DIM), -1.0, np.float32)])
          assert got.cpu().numpy().tobytes() == want.tobytes(), tag + ": find_missed rows"
          o = np.argsort(mi.cpu().numpy())
          assert np.array_equal(mk.cpu().numpy()[o], absent) and np.array_equal(mi.cpu().numpy()[o], np.arange(absent.size) + k[::3].size), \
              tag + ": find_missed lists"
          model = np.zeros((n_rows, DIM), np.float32)
          np.add.at(model, seg, wts[:, None] * cur[pos])
          assert pooled.cpu().numpy().tobytes() == model.tobytes(), tag + ": find_combine"
          uniq, gsum, _ = oopt.segment_sum_by_key(k[pos], g)
          at = np.searchsorted(k, uniq)
          cur[at] = oopt.sgd(cur[at], gsum, LR)
          assert after.cpu().numpy().tobytes() == cur.tobytes(), tag + ": apply_sparse"
          final[w].append((k, cur))
    return run

  _run_threads([worker(w) for w in range(NTHREADS)])
  ora = oracle.CpuTable(DIM)
  for rs in final:
    assert len(rs) == ROUNDS
    for k, v in rs:
      ora.insert(k, v)
  dt.check_errors()
  assert int(t.size()) == NTHREADS * ROUNDS * PER
  k, v = t.export()
  o = torch.argsort(k)
  ek, ev = ora.export_sorted()
  np.testing.assert_array_equal(k[o].cpu().numpy(), ek)
  np.testing.assert_array_equal(v[o].cpu().numpy(), ev)
  assert bool((dt.find(k[o], field=1) == 0.5).all())          # SGD owns no slot: every key's is at aux_init


# ---- 3. grouped calls over overlapping lists, in opposite orders --------------------------------------------------------------------
def test_grouped_calls_with_overlapping_lists_do_not_deadlock(env):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import find_combine_many
  rng = np.random.default_rng(77)
  keys = np.unique(rng.integers(1, 2**40, size=600, dtype=np.int64))[:512]
  T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
  tabs = []
  for i in range(4):
    t = de.CuckooHashTable(torch.int64, torch.float32, torch.full((DIM,), -1.0), name="tc_many_%d" % i, device="cuda:0", dim=DIM)
    t.insert(T(keys), T(rng.standard_normal((keys.size, DIM)).astype(np.float32)))
    tabs.append(t)
  ids, seg = T(keys[rng.integers(0, keys.size, size=700)]), T(np.sort(rng.integers(0, 50, size=700)).astype(np.int64))
  lists = [[tabs[0], tabs[1], tabs[2]], [tabs[3], tabs[2], tabs[1]]]          # tables 1 and 2 in both, in opposite orders
  reqs = [[(t, ids, seg, None, 1, 50) for t in lst] for lst in lists]
  want = [[_bytes(torch, o) for o in find_combine_many(r)] for r in reqs]
  torch.cuda.synchronize()

  def worker(w):
    def run():
      torch.cuda.set_device(0)
      for i in range(200):
        outs = find_combine_many(reqs[w])
        if i % 50 == 49:
          assert [_bytes(torch, o) for o in outs] == want[w], "thread %d, call %d" % (w, i)
    return run

  _run_threads([worker(0), worker(1)])
  torch.cuda.synchronize()
