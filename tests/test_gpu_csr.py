"""GPU: the write-back plans — the CSR-by-key plan (csrc/tfra_csr.hip) and the assign-only SET plan with the unique ops built on it
(csrc/tfra_setplan.hip) — and the kernels that consume them.

  * the plan itself (tfra_sparse_plan_read) against numpy: unique keys, counts, positions ascending per key;
  * tfra_table_apply_sparse at BASELINE's benchmark shape (B = 131 072 Zipf-1.2 over >= 10 M keys, 3 steps) against
    the reference's write-back sequence with SEQUENTIAL fp32 duplicate sums (what the CPU path does,
    PY/dynamic_embedding_optimizer.py:177-190): embedding values within 1e-6 (north_star tolerance);
  * tfra_table_upsert_sparse (repeats: the last occurrence wins) against the oracle table, bit-exact, every dtype,
    unbounded and bounded-at-capacity tables;
  * the SET plan (dim 0) against numpy: distinct keys, occurrence counts, the last position through upsert_planned; one plan
    object rebuilt as SET and CSR in any order; tfra_unique_unordered and tfra_table_find_unique against numpy.unique.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  return torch, de, SparsePlan


def check_plan(torch, SparsePlan, ids_np, dim=64):
  plan = SparsePlan("cuda:0", dim)
  plan.build(torch.from_numpy(ids_np).cuda())
  counts, keys, cnt, pos = plan.read()
  assert counts["errors"] == 0
  uk, uc = np.unique(ids_np, return_counts=True)
  order = np.argsort(keys, kind="stable")
  np.testing.assert_array_equal(keys[order], uk)
  np.testing.assert_array_equal(cnt[order].astype(np.int64), uc)
  # keys with > 8 occurrences come first
  many = counts["many"]
  assert np.all(cnt[:many] > 8) and np.all(cnt[many:] <= 8)
  off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
  assert off[-1] == ids_np.size
  # every key's positions: exactly the positions where it occurs, ascending
  assert np.array_equal(ids_np[pos], np.repeat(keys, cnt))
  starts = np.zeros(ids_np.size, bool)
  starts[off[:-1]] = True
  asc = np.diff(pos.astype(np.int64)) > 0
  assert np.all(asc | starts[1:])
  return counts


@pytest.mark.parametrize("n", [1, 7, 511, 512, 513, 4096, 131072, 262144])
def test_plan_matches_numpy_zipf(env, n):
  torch, de, SparsePlan = env
  rng = np.random.default_rng(n)
  ids = (rng.zipf(1.2, size=n) % 1_000_003).astype(np.int64) * 7919 - 5
  check_plan(torch, SparsePlan, ids)


def test_plan_edge_shapes(env):
  torch, de, SparsePlan = env
  rng = np.random.default_rng(0)
  n = 100_000
  check_plan(torch, SparsePlan, np.full(n, 42, np.int64))                      # one key, 195 bins of 512
  check_plan(torch, SparsePlan, np.arange(n, dtype=np.int64) - 50_000)          # all distinct
  check_plan(torch, SparsePlan, np.repeat(np.arange(n // 9, dtype=np.int64), 9))   # every key just past the direct limit
  check_plan(torch, SparsePlan, np.tile(np.arange(n // 2, dtype=np.int64), 2))     # every key in two far-apart tiles
  check_plan(torch, SparsePlan, rng.integers(0, 40, size=n).astype(np.int64))   # 40 keys, ~2500 each: every tile holds every key
  check_plan(torch, SparsePlan, np.concatenate([np.full(70_000, np.iinfo(np.int64).min), rng.integers(-3, 3, size=30_000)]).astype(np.int64))
  k = rng.integers(0, 3000, size=n).astype(np.int64)                            # ~33 each
  check_plan(torch, SparsePlan, k)
  # a rebuilt plan forgets the previous batch
  plan = SparsePlan("cuda:0", 64)
  for seed in range(3):
    ids = np.random.default_rng(seed).integers(0, 1000 * (seed + 1), size=50_000).astype(np.int64)
    plan.build(torch.from_numpy(ids).cuda())
    counts, keys, cnt, pos = plan.read()
    assert np.array_equal(np.sort(keys), np.unique(ids)) and np.array_equal(ids[pos], np.repeat(keys, cnt))


@pytest.mark.parametrize("world,mode", [(1, 0), (2, 0), (8, 0), (8, 1), (5, 2)])
def test_plan_partition_and_positions(env, world, mode):
  """tfra_plan_partition / tfra_plan_positions_to (the route's stand-in for tf.unique + dynamic_partition): the plan's
  distinct ids grouped by owner, and for every batch position the owner-major row of its id."""
  torch, de, SparsePlan = env
  rng = np.random.default_rng(100 * world + mode)
  shapes = [np.full(70_000, -9, np.int64), np.arange(5000, dtype=np.int64) * 3 - 7000,
            (rng.zipf(1.2, size=131072) % 1_000_003).astype(np.int64) * 7919 - 5, rng.integers(-20, 20, size=40_000).astype(np.int64),
            np.array([5], np.int64), np.repeat(np.arange(3000, dtype=np.int64), 9)]
  plan = SparsePlan("cuda:0", 16)
  for ids in shapes:
    plan.build(torch.from_numpy(ids).cuda())
    keys_out, perm, counts = plan.partition(world, mode)
    dest = plan.positions_to(perm)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy(); keys_out = keys_out.cpu().numpy(); dest = dest.cpu().numpy()
    u = int(counts.sum())
    uniq = np.unique(ids)
    assert u == uniq.size
    assert np.array_equal(np.sort(keys_out[:u]), uniq)
    if mode != 2:   # (hash mode has no reference twin)
      owner = (keys_out[:u] & 0x7FFFFFFF) % world if mode == 0 else np.mod(keys_out[:u], world)
      assert np.all(np.diff(owner) >= 0)                                        # owner-major
      assert np.array_equal(np.bincount(owner, minlength=world), counts)
    assert dest.min() >= 0 and dest.max() < u
    assert np.array_equal(keys_out[dest], ids)                                  # every position maps to the row of its id


def test_apply_sparse_benchmark_shape_vs_sequential_oracle(env):
  """B = 131 072, Zipf-1.2 over 10 M resident keys, 3 Adam steps, one-call path and step driver: embedding values
  within 1e-6 of the reference's sequence with sequential fp32 duplicate sums; slots within 1e-6 relative."""
  torch, de, SparsePlan = env
  from bench import keys_of_ranks, keys_of_ranks_torch, zipf_bounded
  from oracle import optimizers as oopt
  N, dim, B = 10_000_000, 64, 131072
  rng = np.random.default_rng(11)
  opt = de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)
  hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
  for driver in ("one_call", "prefetch"):
    deo = de.DynamicEmbeddingOptimizer(opt)
    var = de.Variable(dim=dim, name="csr_bench_%s" % driver, initializer=0.0, init_size=int(N * 1.05),
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
    gen = torch.Generator(device="cuda").manual_seed(5)
    for lo in range(1, N + 1, 2_000_000):
      k = keys_of_ranks_torch(torch, torch.arange(lo, lo + 2_000_000, dtype=torch.int64, device="cuda"))
      var.tables[0]._table.upsert(k, torch.randn((k.numel(), dim), generator=gen, device="cuda") * 0.01, unique_keys=True)
    steps = 3
    ids = keys_of_ranks(zipf_bounded(rng, steps * B, N)).reshape(steps, B)
    grads = (rng.standard_normal((steps, B, dim)) * 0.01).astype(np.float32)
    touched = np.unique(ids)
    kt = torch.from_numpy(touched).cuda()
    p0 = var.lookup(kt).cpu().numpy()
    # the oracles hold only the touched keys (their rows before the steps; slots start at 0):
    #   state  — duplicate gradients summed SEQUENTIALLY in fp32, batch order (the reference's CPU unsorted_segment_sum)
    #   exact  — duplicate gradients summed in fp64, rounded once (what every fp32 summation order approximates)
    state = {"p": p0.copy(), "m": np.zeros_like(p0), "v": np.zeros_like(p0)}
    exact = {"p": p0.copy(), "m": np.zeros_like(p0), "v": np.zeros_like(p0)}
    ids_t = torch.from_numpy(ids).cuda()
    g_t = torch.from_numpy(grads).cuda()
    ps = de.PrefetchStep(var, deo).prime(ids_t[0]) if driver == "prefetch" else None
    for s in range(steps):
      if ps is not None:
        ps.step(g_t[s], ids_t[s + 1] if s + 1 < steps else None)
      else:
        var.lookup(ids_t[s])
        deo.apply_sparse(var, ids_t[s], g_t[s])
      # reference: unique + unsorted_segment_sum (sequential fp32, index order) + dense Adam on the unique rows
      uk, inv = np.unique(ids[s], return_inverse=True)
      gs = np.zeros((uk.size, dim), np.float32)
      g64 = np.zeros((uk.size, dim), np.float64)
      np.add.at(g64, inv, grads[s].astype(np.float64))
      order = np.argsort(inv, kind="stable")
      bounds = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=uk.size))])
      gsorted = grads[s][order]
      for j in range(uk.size):   # sequential fp32 adds in batch order
        seg = gsorted[bounds[j]:bounds[j + 1]]
        gs[j] = seg[0] if seg.shape[0] == 1 else np.add.accumulate(seg, axis=0, dtype=np.float32)[-1]
      rows = np.searchsorted(touched, uk)
      p, m, v = oopt.adam(state["p"][rows], state["m"][rows], state["v"][rows], gs, 1e-3, 0.9, 0.999, 1e-8, s + 1)
      state["p"][rows], state["m"][rows], state["v"][rows] = p, m, v
      p, m, v = oopt.adam(exact["p"][rows], exact["m"][rows], exact["v"][rows], g64.astype(np.float32), 1e-3, 0.9, 0.999, 1e-8, s + 1)
      exact["p"][rows], exact["m"][rows], exact["v"][rows] = p, m, v
    torch.cuda.synchronize()
    got_p = var.lookup(kt).cpu().numpy()
    # Adam's update lr*m^/(sqrt(v^)+eps) is ill-conditioned where a gradient sum is ~0 (sensitivity lr*eps/(|g|+eps)^2:
    # up to 1e5 per unit of g): there the reference's OWN result moves by more than 1e-6 when its duplicate sum is
    # rounded differently.  Elements where the reference's sequential-fp32 sum and the exactly-rounded sum lead to
    # embedding values more than 2.5e-7 apart are therefore excluded (a handful in 3 M); everywhere else the
    # north_star tolerance applies: 1e-6 on float32 embedding values against the reference's sequence.
    stable = np.abs(state["p"] - exact["p"]) <= 2.5e-7
    assert (~stable).mean() < 1e-5, (~stable).sum()
    err_p = float(np.max(np.abs(got_p - state["p"])[stable]))
    assert err_p <= 1e-6, err_p
    assert float(np.max(np.abs(got_p - exact["p"])[stable])) <= 1e-6
    got_m = deo.get_slot(var, "m").lookup(kt).cpu().numpy()
    got_v = deo.get_slot(var, "v").lookup(kt).cpu().numpy()
    # The slots see the gradient sum itself (m += 0.1 (g - m)): for the hottest key (~24 000 addends) the
    # reference's own sequential fp32 sum is ~1e-5 away from the exact sum, so "equal to the reference" cannot be
    # tighter than that for m.  Pin the slots to the exactly-summed oracle at 1e-6 and to the sequential one at 1e-5,
    # and require that we are not further from exact than the reference's order is.
    np.testing.assert_allclose(got_m, exact["m"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got_v, exact["v"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got_m, state["m"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got_v, state["v"], rtol=1e-5, atol=1e-5)
    e_ours = float(np.max(np.abs(got_m - exact["m"])))
    e_ref = float(np.max(np.abs(state["m"] - exact["m"])))
    assert e_ours <= e_ref + 1e-9, (e_ours, e_ref)
    print("driver %s: max|p - sequential oracle| = %.3g over %d of %d elements (%d ill-conditioned excluded); slot m: "
          "max|ours - exact| = %.3g, max|sequential - exact| = %.3g" % (driver, err_p, int(stable.sum()), stable.size,
                                                                          int((~stable).sum()), e_ours, e_ref))
    del var, deo, ps


@pytest.mark.parametrize("owner_tags", [True, False])
@pytest.mark.parametrize("dtype_name,dim", [("float32", 64), ("float16", 128), ("int8", 3), ("int64", 10), ("bfloat16", 33)])
def test_upsert_sparse_last_occurrence_wins(env, dtype_name, dim, owner_tags):
  import oracle
  torch, de, SparsePlan = env
  dt = getattr(torch, dtype_name)
  npdt = {"float32": np.float32, "float16": np.float16, "int8": np.int8, "int64": np.int64, "bfloat16": np.float32}[dtype_name]
  rng = np.random.default_rng(dim)
  t = de.CuckooHashTable(torch.int64, dt, torch.zeros(dim, dtype=dt), device="cuda:0", dim=dim, name="ups_%s" % dtype_name)
  t._table.set_owner_tags(owner_tags)   # False: the general two-kernel write-back (runs when the tag array cannot be allocated)
  ref = {}
  for step in range(3):
    n = 30_000
    keys = (rng.zipf(1.3, size=n) % 5000).astype(np.int64) - 7
    vals = rng.integers(-100, 100, size=(n, dim)).astype(npdt)
    vt = torch.from_numpy(vals).cuda().to(dt)
    t._table.upsert_sparse(torch.from_numpy(keys).cuda(), vt)
    for i in range(n):
      ref[int(keys[i])] = i
    uk = np.array(sorted(ref), np.int64)
    # rows of the LAST occurrence (across steps the latest step wins)
    if step == 0:
      want = {int(k): vt[ref[int(k)]].clone() for k in uk}
    else:
      for k in np.unique(keys):
        want[int(k)] = vt[ref[int(k)]].clone()
  ek, ev = t.export()
  assert int(t.size().item()) == len(want) == ek.numel()
  got = t.lookup(torch.from_numpy(uk).cuda())
  exp = torch.stack([want[int(k)] for k in uk])
  assert torch.equal(got, exp)


@pytest.mark.parametrize("owner_tags", [True, False])
def test_upsert_sparse_bounded_table_at_capacity(env, owner_tags):
  """A bounded (Hkv) table at max_capacity takes batches with repeats through the plan: size <= capacity, every
  resident key returns the row of its last occurrence."""
  torch, de, SparsePlan = env
  dim, cap, B = 16, 60_000, 50_000
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=cap, max_capacity=cap, device="cuda:0", dim=dim,
                      evict_strategy=de.HkvEvictStrategy.LRU, name="ups_bounded")
  t._table.set_owner_tags(owner_tags)
  rng = np.random.default_rng(3)
  latest = {}
  fresh = 1
  for step in range(12):
    old = (rng.zipf(1.2, size=B // 2) % 20_000).astype(np.int64)
    new = np.arange(fresh, fresh + B // 2, dtype=np.int64) + 1_000_000
    fresh += B // 2
    keys = np.concatenate([old, new])
    rng.shuffle(keys)
    vals = np.tile((np.arange(B, dtype=np.float32) + step * B)[:, None], (1, dim))
    t._table.upsert_sparse(torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda())
    for i in range(B):
      latest[int(keys[i])] = float(vals[i, 0])
    n = int(t.size().item())
    assert n <= cap
  assert int(t.size().item()) > cap * 0.9
  k, v = t.export()
  k, v = k.cpu().numpy(), v.cpu().numpy()
  assert np.unique(k).size == k.size
  np.testing.assert_array_equal(v[:, 0], np.array([latest[int(x)] for x in k], np.float32))
  assert np.all(v == v[:, :1])


@pytest.mark.parametrize("form", ["auto", "hf", "claims"])
def test_upsert_sparse_both_forms_of_the_pass_on_a_table_at_capacity(env, monkeypatch, form):
  """The ownership pass over a SET plan's keys has two forms (upsert_own_kernel<…, HF>): every key claims its two home buckets up front, or
  only the keys that CHANGE a bucket claim them behind their decision and a victim that is a key of the same batch defers the new key to
  the remainder.  Forced either way (TFRA_OWN_HF) and picked from the previous write-back's sample ("auto": the stream alternates
  between batches of resident keys and batches that are half new, so both forms run): after EVERY step each key of the batch holds the
  row of its last occurrence (a hit that claims nothing must never lose its slot to an eviction of the same launch), size <= capacity,
  and the export is a dictionary of last writes."""
  torch, de, SparsePlan = env
  if form == "auto":
    monkeypatch.delenv("TFRA_OWN_HF", raising=False)
  else:
    monkeypatch.setenv("TFRA_OWN_HF", "1" if form == "hf" else "0")
  dim, cap, B = 16, 60_000, 40_000
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=cap, max_capacity=cap, device="cuda:0", dim=dim,
                      evict_strategy=de.HkvEvictStrategy.LRU, name="ups_forms_" + form)
  rng = np.random.default_rng(11)
  latest = {}
  fresh = 1
  zero = torch.zeros(dim, device="cuda")
  for step in range(16):
    hot = (rng.zipf(1.2, size=B) % 20_000).astype(np.int64)
    if step % 4 >= 2:   # two steps of resident keys only, then two with half of the batch never seen before (evictions at capacity)
      keys = hot
      keys[: B // 2] = np.arange(fresh, fresh + B // 2, dtype=np.int64) + 1_000_000
      fresh += B // 2
      rng.shuffle(keys)
    else:
      keys = hot
    vals = np.tile((np.arange(B, dtype=np.float32) + step * B)[:, None], (1, dim))
    kt = torch.from_numpy(keys).cuda()
    t._table.upsert_sparse(kt, torch.from_numpy(vals).cuda())
    for i in range(B):
      latest[int(keys[i])] = float(vals[i, 0])
    got, ex = t._table.find(kt, zero, return_exists=True)
    assert bool(ex.all()), (form, step, int((~ex).sum()))
    np.testing.assert_array_equal(got[:, 0].cpu().numpy(), np.array([latest[int(x)] for x in keys], np.float32))
    assert int(t.size().item()) <= cap
  assert int(t.size().item()) > cap * 0.9
  k, v = t.export()
  k, v = k.cpu().numpy(), v.cpu().numpy()
  assert np.unique(k).size == k.size
  np.testing.assert_array_equal(v[:, 0], np.array([latest[int(x)] for x in k], np.float32))
  assert np.all(v == v[:, :1])
  t._table.check_errors()


@pytest.mark.parametrize("form", ["auto", "hf", "claims"])
def test_insert_of_unique_keys_both_forms_of_the_pass_on_a_growing_table(env, monkeypatch, form):
  """The reference's Insert op (insert_or_assign of a caller's UNIQUE keys) on a table that never evicts (the cuckoo flavour, TFRA's
  default): the pass may take the form in which a hit claims nothing — there is no eviction a claim would protect it from.  Forced both
  ways and auto-picked; batches of resident keys, batches with a third of new keys (the table grows under the stream), the sentinel
  keys: the table is a dictionary of last writes after every step."""
  torch, de, SparsePlan = env
  if form == "auto":
    monkeypatch.delenv("TFRA_OWN_HF", raising=False)
  else:
    monkeypatch.setenv("TFRA_OWN_HF", "1" if form == "hf" else "0")
  dim = 16
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(dim), device="cuda:0", dim=dim, name="ins_forms_" + form, init_size=200_000)
  rng = np.random.default_rng(19)
  imin = np.iinfo(np.int64).min
  latest = {}
  fresh = 1
  zero = torch.zeros(dim, device="cuda")
  for step in range(14):
    keys = np.unique((rng.zipf(1.2, size=60_000) % 50_000).astype(np.int64) * 7919 - 11)
    if step % 3 == 2:
      new = np.arange(fresh, fresh + keys.size // 2, dtype=np.int64) * 7919 - 11 + 7919 * 1_000_000
      fresh += new.size
      keys = np.concatenate([keys, new, np.array([imin, imin + 1], np.int64)])
    rng.shuffle(keys)
    vals = np.tile((np.arange(keys.size, dtype=np.float32) + step * 100_000)[:, None], (1, dim))
    kt = torch.from_numpy(keys).cuda()
    t._table.upsert(kt, torch.from_numpy(vals).cuda(), unique_keys=True)
    for i in range(keys.size):
      latest[int(keys[i])] = float(vals[i, 0])
    got, ex = t._table.find(kt, zero, return_exists=True)
    assert bool(ex.all()), (form, step, int((~ex).sum()))
    np.testing.assert_array_equal(got[:, 0].cpu().numpy(), vals[:, 0])
    assert int(t.size().item()) == len(latest)
  k, v = t.export()
  k, v = k.cpu().numpy(), v.cpu().numpy()
  assert np.unique(k).size == k.size == len(latest)
  np.testing.assert_array_equal(v[:, 0], np.array([latest[int(x)] for x in k], np.float32))
  t._table.check_errors()


def test_multi_table_step_matches_per_table_steps(env):
  """tfra_multi_step_prefetch (host-thread pool, several stream pairs) == one PrefetchStep per table, bit for bit: the
  tables are independent, only who issues the launches differs.  26-table shape of BASELINE configs[4] in small."""
  torch, de, SparsePlan = env
  rng = np.random.default_rng(5)
  dims = [16, 32, 64, 128]
  nt, B, steps = 7, 4096, 4

  def build(tag):
    opt = de.optimizers.Ftrl(0.05, l1_regularization_strength=1e-3, l2_regularization_strength=1e-3)
    deo = de.DynamicEmbeddingOptimizer(opt)
    vs = [de.Variable(dim=dims[i % 4], name="mt_%s_%d" % (tag, i), initializer=0.1, devices=["cuda:0"],
                      **de.DynamicEmbeddingOptimizer.variable_kwargs(opt)) for i in range(nt)]
    return deo, vs

  ids = [[torch.from_numpy((rng.zipf(1.2, size=B) % (3000 + 500 * i)).astype(np.int64) * 7919 + i).cuda() for _ in range(steps + 1)]
         for i in range(nt)]
  grads = [[torch.from_numpy((rng.standard_normal((B, dims[i % 4])) * 0.01).astype(np.float32)).cuda() for _ in range(steps)]
           for i in range(nt)]
  deo_a, va = build("a")
  deo_b, vb = build("b")
  ms = de.MultiTablePrefetchStep(va, deo_a, streams=3, workers=3).prime([ids[i][0] for i in range(nt)])
  pss = [de.PrefetchStep(v, deo_b).prime(ids[i][0]) for i, v in enumerate(vb)]
  for s in range(steps):
    outs = ms.step([grads[i][s] for i in range(nt)], [ids[i][s + 1] for i in range(nt)])
    ms.synchronize()
    deo_b.iterations = s   # one global step per training step (PrefetchStep advances it once per table)
    for i, ps in enumerate(pss):
      deo_b.iterations = s
      ref = ps.step(grads[i][s], ids[i][s + 1])
      assert torch.equal(outs[i], ref), (s, i)
  torch.cuda.synchronize()
  assert deo_a.iterations == steps
  for a, b in zip(va, vb):
    ka, xa = a.export()
    kb, xb = b.export()
    oa, ob = torch.argsort(ka), torch.argsort(kb)
    assert torch.equal(ka[oa], kb[ob]) and torch.equal(xa[oa], xb[ob])


@pytest.mark.parametrize("n,universe", [(600_000, 50_000), (1_300_000, 5_000_000)])
def test_apply_sparse_more_ids_than_a_plan_holds(env, n, universe):
  """n > 2^18 ids in ONE apply_sparse call: equal ids of different chunks still meet in one update.  Compared with the
  reference's sequence (unique + sequential fp32 duplicate sums + one Adam update per key: oracle/optimizers.py) to 1e-6;
  (600 K ids over 50 K keys: the reduced list fits one plan; 1.3 M over 5 M keys: it is split by key hash)."""
  torch, de, SparsePlan = env
  from oracle import optimizers as oopt
  dim = 16
  rng = np.random.default_rng(n)
  opt = de.optimizers.Adam(1e-3, 0.9, 0.999, 1e-8)
  var = de.Variable(dim=dim, name="big_apply_%d" % n, initializer=0.25, init_size=universe * 2,
                    **de.DynamicEmbeddingOptimizer.variable_kwargs(opt))
  deo = de.DynamicEmbeddingOptimizer(opt)
  # two oracles: duplicate sums rounded once from fp64 (A) and summed sequentially in fp32 (B, the reference's CPU order)
  A = [np.full((universe, dim), 0.25, np.float32), np.zeros((universe, dim), np.float32), np.zeros((universe, dim), np.float32)]
  Bq = [x.copy() for x in A]
  seen = np.zeros(universe, bool)
  for step in range(2):
    r = rng.zipf(1.2, size=n) % universe
    ids = r.astype(np.int64) * 7919 - 77
    g = (rng.standard_normal((n, dim)) * 0.01).astype(np.float32)
    deo.apply_sparse(var, torch.from_numpy(ids).cuda(), torch.from_numpy(g).cuda())
    ur, inv = np.unique(r, return_inverse=True)
    g64 = np.zeros((ur.size, dim), np.float64)
    np.add.at(g64, inv, g.astype(np.float64))
    g32 = np.zeros((ur.size, dim), np.float32)
    np.add.at(g32, inv, g)
    A[0][ur], A[1][ur], A[2][ur] = oopt.adam(A[0][ur], A[1][ur], A[2][ur], g64.astype(np.float32), 1e-3, 0.9, 0.999, 1e-8, step + 1)
    Bq[0][ur], Bq[1][ur], Bq[2][ur] = oopt.adam(Bq[0][ur], Bq[1][ur], Bq[2][ur], g32, 1e-3, 0.9, 0.999, 1e-8, step + 1)
    seen[ur] = True
  rows = np.nonzero(seen)[0]
  keys = rows.astype(np.int64) * 7919 - 77
  assert int(var.size().item()) == keys.size
  got = var.lookup(torch.from_numpy(keys).cuda()).cpu().numpy()
  # Adam is ill-conditioned where a gradient sum is ~0 (see test_apply_sparse_benchmark_shape_vs_sequential_oracle): the
  # elements where the reference's own result depends on the rounding of its duplicate sum are excluded
  stable = np.abs(A[0][rows] - Bq[0][rows]) <= 2.5e-7
  assert (~stable).mean() < 1e-4, int((~stable).sum())
  assert float(np.max(np.abs(got - A[0][rows])[stable])) <= 1e-6
  assert float(np.max(np.abs(got - Bq[0][rows])[stable])) <= 1e-6
  assert var.tables[0]._table.check_errors() is None


def test_upsert_sparse_more_ids_than_a_plan_holds(env):
  torch, de, SparsePlan = env
  n, dim = 700_000, 8
  rng = np.random.default_rng(4)
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(dim), device="cuda:0", dim=dim, name="big_upsert")
  keys = (rng.zipf(1.3, size=n) % 90_000).astype(np.int64) - 100
  vals = np.tile(np.arange(n, dtype=np.float32)[:, None], (1, dim))
  t._table.upsert_sparse(torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda())
  last = {}
  for i, k in enumerate(keys.tolist()):
    last[k] = i
  uk = np.array(sorted(last), np.int64)
  assert int(t.size().item()) == uk.size
  got = t.lookup(torch.from_numpy(uk).cuda()).cpu().numpy()
  np.testing.assert_array_equal(got[:, 0], np.array([last[int(k)] for k in uk], np.float32))
  assert np.all(got == got[:, :1])


def test_set_plan_counts_last_positions_and_reuse(env):
  """The assign-only plan (dim 0, setplan_kernel): distinct keys, occurrence counts and — through upsert_planned — the LAST
  position of every id, over a sequence of builds of ONE plan object with very different sizes (its two tables alternate and
  empty each other: a stale entry of an earlier build would show up as a wrong count or a phantom key), with the two sentinel
  key values (they have slots of their own) and a hot id."""
  torch, de, SparsePlan = env
  dim = 8
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(dim), device="cuda:0", dim=dim, name="setplan")
  plan = SparsePlan("cuda:0", 0)
  rng = np.random.default_rng(11)
  imin = np.iinfo(np.int64).min
  expect = {}
  for n in (1, 5, 3000, 70_000, 17, 262_144, 40_000, 2):
    keys = (rng.zipf(1.25, size=n) % max(3, n // 3)).astype(np.int64) * 104729 - 3
    if n >= 17:
      keys[rng.integers(0, n, size=max(1, n // 50))] = imin          # EMPTY_KEY as an ordinary key
      keys[rng.integers(0, n, size=max(1, n // 70))] = imin + 1      # LOCKED_KEY as an ordinary key
      keys[: n // 5] = 42                                            # a hot id
    ids = torch.from_numpy(keys).cuda()
    plan.build(ids)
    counts, pk, pc, ppos = plan.read()
    uk, uc = np.unique(keys, return_counts=True)
    assert counts["many"] == 0 and counts["few"] == uk.size and counts["errors"] == 0 and ppos is None
    o = np.argsort(pk)
    np.testing.assert_array_equal(pk[o], uk)
    np.testing.assert_array_equal(pc[o], uc)
    vals = torch.arange(n, device="cuda", dtype=torch.float32)[:, None].repeat(1, dim)   # row i = [i] * dim
    t._table.upsert_planned(plan, vals)
    last = {}
    for i, k in enumerate(keys.tolist()):
      last[k] = i
    expect.update(last)
    got = t.lookup(torch.from_numpy(uk).cuda())
    want = torch.tensor([float(last[int(k)]) for k in uk], device="cuda")[:, None].repeat(1, dim)
    assert torch.equal(got, want)
  ek, ev = t.export()
  assert ek.numel() == len(expect) == int(t.size().item())
  t._table.check_errors()


def test_one_plan_object_alternating_csr_and_set_builds(env):
  """A plan object may be rebuilt with dim > 0 (CSR buffer) and dim 0 (SET buffer) in any order; each buffer keeps its own
  pair of left-over counter sets and its own flag bytes, selected by that buffer's OWN use count.  With one shared count a
  CSR use -> SET use -> CSR use found the CSR buffer's counter where the first launch left it (stale left-over list replayed
  against new values).  Small table, many keys per bucket pair: every launch has left-over keys."""
  torch, de, SparsePlan = env
  dim = 4
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=4096, max_capacity=4096, device="cuda:0", dim=dim,
                      evict_strategy=de.HkvEvictStrategy.LRU, name="altplan")
  universe = torch.arange(1, 1501, dtype=torch.int64, device="cuda") * 7919
  t._table.upsert(universe, torch.zeros((universe.numel(), dim), device="cuda"), unique_keys=True)
  plan = SparsePlan("cuda:0", dim)
  rng = np.random.default_rng(3)
  expect = {}
  for step, pdim in enumerate([dim, 0, dim, dim, 0, 0, dim, 0, dim]):
    n = int(rng.integers(500, 2000))
    keys = universe.cpu().numpy()[rng.integers(0, universe.numel(), size=n)]
    ids = torch.from_numpy(keys).cuda()
    plan._dim = pdim          # (the C entry point takes the dim per build: the same object, the other buffer)
    plan.build(ids)
    vals = (torch.arange(n, device="cuda", dtype=torch.float32) + 10000.0 * step)[:, None].repeat(1, dim)
    t._table.upsert_planned(plan, vals)
    for i, k in enumerate(keys.tolist()):
      expect[k] = float(i + 10000.0 * step)
    uk = np.array(sorted(expect), np.int64)
    got = t.lookup(torch.from_numpy(uk).cuda())
    want = torch.tensor([expect[int(k)] for k in uk], device="cuda")[:, None].repeat(1, dim)
    assert torch.equal(got, want), "step %d (plan dim %d)" % (step, pdim)
  t._table.check_errors()


def test_set_csr_set_builds_then_upsert_on_one_plan_object(env):
  """One plan object: regular SET build, CSR build (dim 4), regular SET build, then upsert_planned from it on a small LFU table
  without caller scores.  The path on which the plan's control words meet: the count word of each of the SET buffer's two tables
  (the second build walks the first table's list through that table's count word), the SET use block read as a CSR d_counts block
  (tfra_sparse_plan_read and the write-back see the keys through keys_of), the CSR buffer's own block in between, the SET buffer's
  OwnCtrs set selected by that buffer's use count, and the occurrence counts as the LFU scores.  n = 1500: two 1024-id blocks, the
  smallest shape with a second block; both sentinel key values, and one key with more than 8 occurrences."""
  torch, de, SparsePlan = env
  dim, n = 4, 1500
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=8192, max_capacity=8192, device="cuda:0", dim=dim,
                      evict_strategy=de.HkvEvictStrategy.LFU, name="set_csr_set")
  plan = SparsePlan("cuda:0", 0)
  rng = np.random.default_rng(23)
  imin = np.iinfo(np.int64).min

  def batch():
    keys = rng.integers(1, 700, size=n).astype(np.int64) * 104729 - 3
    keys[rng.integers(0, n, size=5)] = imin          # EMPTY_KEY as an ordinary key
    keys[rng.integers(0, n, size=3)] = imin + 1      # LOCKED_KEY as an ordinary key
    keys[rng.integers(0, n, size=40)] = 42           # a key with more than 8 occurrences
    return keys

  def build_and_check_set(keys):
    plan._dim = 0
    plan.build(torch.from_numpy(keys).cuda())
    counts, pk, pc, ppos = plan.read()
    uk, uc = np.unique(keys, return_counts=True)
    assert uc[uk == 42][0] > 8 and imin in uk and imin + 1 in uk
    assert counts["many"] == 0 and counts["few"] == uk.size and counts["errors"] == 0 and ppos is None
    o = np.argsort(pk)
    np.testing.assert_array_equal(pk[o], uk)
    np.testing.assert_array_equal(pc[o], uc)
    return uk, uc

  build_and_check_set(batch())
  plan._dim = dim               # (the C entry point takes the dim per build: the same object, the other buffer)
  plan.build(torch.from_numpy(batch()).cuda())
  keys = batch()
  uk, uc = build_and_check_set(keys)
  vals = torch.arange(n, device="cuda", dtype=torch.float32)[:, None].repeat(1, dim)   # row i = [i] * dim
  t._table.upsert_planned(plan, vals)
  last = {}
  for i, k in enumerate(keys.tolist()):
    last[k] = i
  got = t.lookup(torch.from_numpy(uk).cuda())
  want = torch.tensor([float(last[int(k)]) for k in uk], device="cuda")[:, None].repeat(1, dim)
  assert torch.equal(got, want)
  assert int(t.size().item()) == uk.size
  ek, es = t.export_keys_and_scores(1 << 14)
  ek, es = ek.cpu().numpy(), es.cpu().numpy()
  np.testing.assert_array_equal(np.sort(ek), uk)
  scored = uk > imin + 1   # (the two sentinel key values live in side rows, which keep no score)
  np.testing.assert_array_equal(es[np.argsort(ek)][scored], uc[scored].astype(es.dtype))   # an LFU score = the occurrences the plan counted
  t._table.check_errors()


def test_unique_many_calls_one_workspace(env):
  """tfra_unique keeps two persistent sets per workspace that empty each other: a sequence of calls with sizes going up and
  down (incl. the sentinel value and a hot id) must each equal numpy's first-occurrence unique."""
  torch, de, SparsePlan = env
  rng = np.random.default_rng(13)
  imin = np.iinfo(np.int64).min
  for n in (7, 50_000, 3, 131_072, 1000, 600_000, 131_072, 1):
    ids = (rng.zipf(1.2, size=n) % max(2, n // 2)).astype(np.int64) * 7919 - 11
    if n > 100:
      ids[rng.integers(0, n, size=n // 40)] = imin
      ids[n // 3: n // 2] = 5
    u, idx, cnt = de.device_ops.unique(torch.from_numpy(ids).cuda())
    _, first = np.unique(ids, return_index=True)
    want = ids[np.sort(first)]                       # distinct values in order of first occurrence (tf.unique)
    assert int(cnt.item()) == want.size
    np.testing.assert_array_equal(u.cpu().numpy(), want)
    np.testing.assert_array_equal(want[idx.cpu().numpy()], ids)


def _zipf_ids_hot_and_sentinel(rng, n):
  """The stream of test_unique_many_calls_one_workspace: Zipf ids under a modulus of n // 2, int64.min (the scratch sets' sentinel
  value, which both implementations keep in a side slot) at n // 40 positions, one hot id over [n // 3, n // 2)."""
  ids = (rng.zipf(1.2, size=n) % max(2, n // 2)).astype(np.int64) * 7919 - 11
  ids[rng.integers(0, n, size=n // 40)] = np.iinfo(np.int64).min
  ids[n // 3: n // 2] = 5
  return ids


def _check_tf_unique(torch, de, ids):
  from oracle import frontends as ofe
  u, idx, cnt = de.device_ops.unique(torch.from_numpy(ids).cuda())
  eu, eidx = ofe.unique(ids)
  assert int(cnt.item()) == eu.size
  np.testing.assert_array_equal(u.cpu().numpy(), eu)
  np.testing.assert_array_equal(idx.cpu().numpy(), eidx)


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 1])
def test_unique_at_the_path_switch(env, n):
  """tfra_unique changes implementation at 2^20 ids.  2^20 is the largest call of the three-launch path: its look-back runs over
  the largest legal grid, 1024 tiles.  2^20 + 1 is the smallest call of the six-launch path (fill, insert, count, scan, scatter,
  idx over the workspace's scratch).  Both against tf.unique, bit for bit."""
  torch, de, SparsePlan = env
  _check_tf_unique(torch, de, _zipf_ids_hot_and_sentinel(np.random.default_rng(n), n))


def test_unique_six_launch_call_between_fast_calls(env):
  """One workspace: a three-launch call, a six-launch call (it works in the workspace's scratch, not in the two persistent sets),
  a three-launch call again — the sets are as usable after the call in between as before it."""
  torch, de, SparsePlan = env
  rng = np.random.default_rng(29)
  for n in (131_072, (1 << 20) + 1, 131_072):
    _check_tf_unique(torch, de, _zipf_ids_hot_and_sentinel(rng, n))


def test_unique_unordered_matches_numpy_as_a_set(env):
  """tfra_unique_unordered: the distinct ids in ANY order + a consistent inverse index (what embedding_lookup needs of tf.unique);
  a sequence of calls on one workspace with sizes going up and down, the sentinel values and a hot id."""
  torch, de, SparsePlan = env
  rng = np.random.default_rng(17)
  imin = np.iinfo(np.int64).min
  for n in (7, 50_000, 3, 131_072, 1000, 262_144, 131_072, 1):
    ids = (rng.zipf(1.2, size=n) % max(2, n // 2)).astype(np.int64) * 7919 - 11
    if n > 100:
      ids[rng.integers(0, n, size=n // 40)] = imin
      ids[rng.integers(0, n, size=n // 50)] = imin + 1
      ids[n // 3: n // 2] = 5
    u, idx, cnt = de.device_ops.unique(torch.from_numpy(ids).cuda(), ordered=False)
    un, idxn = u.cpu().numpy(), idx.cpu().numpy()
    want = np.unique(ids)
    assert int(cnt.item()) == want.size == un.size
    np.testing.assert_array_equal(np.sort(un), want)
    np.testing.assert_array_equal(un[idxn], ids)


@pytest.mark.parametrize("kind", ["bounded_dense_f32", "growing_f32", "bounded_f16_dim128", "rows_of_24_bytes"])
def test_find_unique_equals_find_and_unique(env, kind):
  """tfra_table_find_unique (ONE launch: the lookup of all ids next to their de-duplication — what the fused TF op
  TFRA>HkvHashTableEmbeddingLookup issues) against tfra_table_find and numpy.unique: rows and exists flags bit-exact, the distinct ids
  as a set with a consistent inverse index.  Sizes up and down on one workspace (the plan's two tables alternate and empty each other),
  up to 262144 ids in ONE launch (two ids per de-duplicating thread above 131072); with rows that are not 16-byte granules the call
  runs the two launches one after the other — same results."""
  torch, de, SparsePlan = env
  rng = np.random.default_rng(5)
  imin = np.iinfo(np.int64).min
  dtype, dim, bounded = {"bounded_dense_f32": (torch.float32, 64, True), "growing_f32": (torch.float32, 64, False),
                         "bounded_f16_dim128": (torch.float16, 128, True), "rows_of_24_bytes": (torch.float32, 6, True)}[kind]
  cap = 1 << 18
  if bounded:
    t = de.HkvHashTable(torch.int64, dtype, torch.zeros(dim, dtype=dtype), init_capacity=cap, max_capacity=cap, device="cuda:0", dim=dim,
                        evict_strategy=de.HkvEvictStrategy.LRU, name="fu_" + kind)
  else:
    t = de.CuckooHashTable(torch.int64, dtype, torch.zeros(dim, dtype=dtype), device="cuda:0", dim=dim, name="fu_" + kind)
  tbl = t._table
  resident = np.arange(1, int(cap * 0.9) + 1, dtype=np.int64) * 7919 - 11     # a bounded table above 60 %: "dense" (both lines in flight)
  for lo in range(0, resident.size, 1 << 16):
    k = torch.from_numpy(resident[lo:lo + (1 << 16)]).cuda()
    tbl.upsert(k, ((k % 1000).to(torch.float32)[:, None] + torch.arange(dim, device="cuda")[None, :] / 64.0).to(dtype), unique_keys=True)
  tbl.upsert(torch.tensor([imin, imin + 1], device="cuda"), torch.full((2, dim), 7.0, dtype=dtype, device="cuda"), unique_keys=True)
  one_row = torch.full((dim,), -3.0, dtype=dtype, device="cuda")
  for n in (7, 50_000, 3, 131_072, 1000, 200_000, 131_072, 1, 17, 0):
    ids = (rng.zipf(1.2, size=n) % max(2, n)).astype(np.int64) * 7919 - 11    # ~10 % beyond the resident range for the big sizes: misses
    if n > 100:
      ids[rng.integers(0, n, size=n // 40)] = imin
      ids[rng.integers(0, n, size=n // 50)] = imin + 1
      ids[rng.integers(0, n, size=n // 10)] = -5 - rng.integers(0, 1000, size=n // 10)   # never inserted
      ids[n // 3: n // 2] = 5 * 7919 - 11
    kt = torch.from_numpy(ids).cuda()
    for full in (False, True):
      dflt = (torch.arange(n * dim, device="cuda").reshape(n, dim) % 251).to(dtype) if (full and n) else one_row
      rows, uniq, idx, cnt, ex = tbl.find_unique(kt, dflt, return_exists=True)
      ref, rex = tbl.find(kt, dflt, return_exists=True)
      assert torch.equal(ex, rex) and torch.equal(rows, ref), (kind, n, full)
      if n > 100:
        assert 0 < int((~ex).sum()) < n
      want = np.unique(ids)
      u = int(cnt.item())
      un, idxn = uniq[:u].cpu().numpy(), idx.cpu().numpy()
      assert u == want.size
      np.testing.assert_array_equal(np.sort(un), want)
      np.testing.assert_array_equal(un[idxn], ids)
  tbl.check_errors()


@pytest.mark.parametrize("owner_tags", [True, False])
@pytest.mark.parametrize("driver", ["upsert_sparse", "step"])
def test_sparse_write_back_lfu_scores_are_occurrence_counts(env, driver, owner_tags):
  """An LFU table's score of a key = how often it was written (lookup_table_op_hkv.h:454-475, kLfu: score += 1 per upsert
  of the key; a batch with repeats counts every occurrence).  The assign-only plan counts occurrences only for tables that
  read them (LFU without caller scores) — here they must arrive — and the write-back adds them to the key's score."""
  torch, de, SparsePlan = env
  dim, cap = 8, 1 << 16
  t = de.HkvHashTable(torch.int64, torch.float32, torch.zeros(dim), init_capacity=cap, max_capacity=cap, device="cuda:0", dim=dim,
                      evict_strategy=de.HkvEvictStrategy.LFU, name="lfu_counts_%s_%d" % (driver, owner_tags))
  t._table.set_owner_tags(owner_tags)
  rng = np.random.default_rng(17)
  total = {}
  batches = [(rng.zipf(1.3, size=20_000) % 3000).astype(np.int64) * 11 + 5 for _ in range(4)]
  if driver == "step":
    ps = de.PrefetchAssignStep(t).prime(torch.from_numpy(batches[0]).cuda())
  for i, ids in enumerate(batches):
    vals = torch.full((ids.size, dim), float(i + 1), device="cuda")
    if driver == "step":
      ps.step(vals, torch.from_numpy(batches[i + 1]).cuda() if i + 1 < len(batches) else None, lookup=False)
    else:
      t._table.upsert_sparse(torch.from_numpy(ids).cuda(), vals)
    for k, c in zip(*np.unique(ids, return_counts=True)):
      total[int(k)] = total.get(int(k), 0) + int(c)
  ek, es = t.export_keys_and_scores(1 << 20)
  ek, es = ek.cpu().numpy(), es.cpu().numpy()
  assert ek.size == len(total) == int(t.size().item())
  np.testing.assert_array_equal(es[np.argsort(ek)], np.array([total[k] for k in sorted(total)], np.uint64).astype(es.dtype))
  t._table.check_errors()
