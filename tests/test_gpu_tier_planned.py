"""GPU: tfra_tier_find_or_insert_planned — the tier's admitting lookup over the distinct keys of a write-back plan.

The tier is that of tests/test_gpu_tier_driver.py: an upper LRU table of 15 * 89 slots at max_capacity in front of a growing lower
table.  Which resident an LRU table evicts depends on device clocks, so nothing here asserts a victim and nothing is compared with
a second tier.  The truth is a dictionary of whole rows: after every call every key ever written through the tier has its newest
whole row in the upper table if that contains the key, otherwise in the lower one, and the driver's statistics count what the
dictionary says — per DISTINCT key of the plan, not per position.  Every comparison is bit for bit."""
import numpy as np
import pytest

from tests.sparse_helpers import Calls
from tests.test_gpu_find_or_insert import _rows
from tests.test_gpu_find_or_insert_planned import _last_positions, _plan, _pos_rows
from tests.test_gpu_tier_driver import AUX, AUX_INIT, CAP, DIM, MAX_BATCH, Truth, _fresh_whole, _never_seen, _saturated, _tier

pytestmark = pytest.mark.gpu

NAME = "tfra_tier_find_or_insert_planned"
NB = 89
DIRECT = 8     # occurrences a plan keeps in a key's record; one more and the positions sit in the bins


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _t(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
  """[n, row bytes] uint8 on the host, of any value dtype"""
  import torch
  return t.contiguous().view(torch.uint8).cpu().numpy().reshape(t.shape[0], -1)


# ---- 1. every plan structure, in every shape -------------------------------------------------------------------------------------------
SHAPES = [("float32", 4, 0), ("float32", 64, 2), ("float16", 128, 0), ("bfloat16", 256, 0), ("float16", 12, 0)]   # (the last: 24-B rows, 8-B granules)
GROUPS = ((150, 1), (40, 2), (20, DIRECT), (20, DIRECT + 1), (1, 600), (1, 1100))
STRUCT_SEED = 41


def _structured():
  """-> (2270 ids, the 232 distinct keys group by group, the two heavy keys, 2100 further keys to fill the tier with)"""
  rng = np.random.default_rng(STRUCT_SEED)
  pool = np.unique(rng.integers(1, 2**40, size=2600, dtype=np.int64))
  rng.shuffle(pool)
  n_keys = sum(k for k, _ in GROUPS)
  distinct, fillers = pool[:n_keys], pool[n_keys:n_keys + 2100]
  parts, at = [], 0
  for nkeys, cnt in GROUPS:
    parts.append(np.repeat(distinct[at:at + nkeys], cnt))
    at += nkeys
  ids = np.concatenate(parts)
  rng.shuffle(ids)
  assert ids.size == 2270 and ids.size % 16 != 0 and n_keys == 232 and fillers.size == 2100
  return ids, distinct, (int(distinct[230]), int(distinct[231])), fillers


class ShapedTruth(Truth):
  """tests/test_gpu_tier_driver.py's Truth for any value dtype and row shape: the rows of the dictionary are the BYTES of whole rows"""

  def __init__(self, torch, upper, lower, tier, dim, aux):
    super().__init__(torch, upper, lower, tier)
    self.dim, self.aux = dim, aux

  def after_call(self, batch, tag):
    torch, upper, lower = self.torch, self.upper, self.lower
    seen = self.seen()
    st = _t(torch, seen)
    up = upper.contains(st)
    now = set(seen[up.cpu().numpy()].tolist())
    self.demoted += len((self.in_upper | set(batch.tolist())) - now)
    self.in_upper = now
    self.calls += 1
    want = np.stack([self.rows[k] for k in seen.tolist()])
    got = np.concatenate([_bits(torch.where(up[:, None], upper.find(st, field=f), lower.find(st, field=f))) for f in range(self.aux + 1)], axis=1)
    bad = (got != want).any(1)
    assert not bad.any(), "%s: %d keys do not hold their newest whole row (%d of them in the upper table)" % (
        tag, int(bad.sum()), int((bad & up.cpu().numpy()).sum()))
    assert bool(lower.contains(st[~up]).all()), tag
    upper.check_errors()
    lower.check_errors()
    assert upper.size_host() <= upper.capacity()
    s = self.tier.stats()
    assert (s["calls"], s["missed"], s["lower_hits"], s["demoted"]) == (self.calls, self.missed, self.lower_hits, self.demoted), (tag, s)


def _shaped_tier(torch, tag, tdt, dim, aux, max_batch):
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier
  upper = _DeviceTable(torch.int64, tdt, torch.zeros(dim, dtype=tdt), "tierplan_up_" + tag, "cuda:0", dim=dim, aux_fields=aux, init_capacity=CAP,
                       max_capacity=CAP, strategy=0, aux_init=AUX_INIT)
  lower = _DeviceTable(torch.int64, tdt, torch.zeros(dim, dtype=tdt), "tierplan_lo_" + tag, "cuda:0", dim=dim, aux_fields=aux, aux_init=AUX_INIT)
  return upper, lower, _DeviceTier(upper, lower, max_batch)


@pytest.mark.parametrize("full", [True, False], ids=["init-full", "init-row"])
@pytest.mark.parametrize("dt,dim,aux", SHAPES, ids=["f32-4", "f32-64-aux2", "f16-128", "bf16-256", "f16-12"])
def test_every_plan_structure(env, dt, dim, aux, full):
  torch, _ = env
  tdt = getattr(torch, dt)
  upper, lower, tier = _shaped_tier(torch, "%s_%d_%d" % (dt, dim, full), tdt, dim, aux, 4096)
  assert (upper.capacity() - 2) // 15 == NB
  ids, distinct, (heavy_a, heavy_b), fillers = _structured()
  assert _saturated(distinct, NB) == 0        # the batch does not saturate its own home buckets (a CPU precondition; the seed is chosen for it)
  # a third of the batch's keys goes in first (the filling that follows pushes them down), a third last (they stay up), a third never
  third = np.arange(distinct.size) % 3
  third[230], third[231] = 2, 1               # one heavy key is never seen, the other one resident
  early, late = distinct[third == 0], distinct[third == 1]
  truth = ShapedTruth(torch, upper, lower, tier, dim, aux)
  aux_bits = [_bits(torch.full((1, dim), AUX_INIT[f], dtype=tdt))[0] for f in range(aux)]
  emb = lambda keys, ver: _t(torch, _rows(keys, ver, "float32", dim)).to(tdt)
  calls = [np.concatenate([early, fillers[:300 - early.size]])]
  calls += [fillers[300 * i:300 * (i + 1)] for i in range(1, 6)]
  calls += [np.concatenate([late, fillers[1800:1800 + 300 - late.size]])]
  for i, keys in enumerate(calls):
    assert keys.size == 300 and _saturated(keys, NB) == 0
    rows = emb(keys, 1)
    tier.insert(_t(torch, keys), rows)
    truth.rows.update(zip(keys.tolist(), np.concatenate([_bits(rows)] + [np.tile(b, (keys.size, 1)) for b in aux_bits], axis=1)))
    truth.after_call(keys, "prefill %d" % i)
  assert upper.size_host() > 0.9 * CAP and len(truth.rows) > CAP
  # slot vectors of their own for every key, written where the key lives, so that a promoted key is seen to bring them along
  known_keys = truth.seen()
  kt = _t(torch, known_keys)
  in_up = upper.contains(kt)
  whole = [_bits(emb(known_keys, 1))]
  for f in range(1, aux + 1):
    slot = emb(known_keys, 10 + f)
    upper.upsert(kt[in_up], slot[in_up].contiguous(), field=f)
    lower.upsert(kt[~in_up], slot[~in_up].contiguous(), field=f)
    whole.append(_bits(slot))
  truth.rows.update(zip(known_keys.tolist(), np.concatenate(whole, axis=1)))
  # the three classes of the batch's keys, as the tables say before the call
  dk = _t(torch, distinct)
  up_before = upper.contains(dk).cpu().numpy()
  known = np.array([k in truth.rows for k in distinct.tolist()])
  cls = np.where(up_before, 1, np.where(known, 2, 0)).astype(np.uint8)
  assert (cls == 1).any() and (cls == 2).any() and (cls == 0).any()
  cls_of = dict(zip(distinct.tolist(), cls.tolist()))
  assert cls_of[heavy_a] != cls_of[heavy_b]
  n = ids.size
  plan = _plan(torch, ids, dim)
  counts = plan.read()[0]
  assert counts["many"] >= 22 and counts["bins"] >= 2 and counts["errors"] == 0, counts
  init = _pos_rows(torch, n, 2, tdt, dim) if full else _pos_rows(torch, 1, 3, tdt, dim)[0].contiguous()
  init_bits = _bits(init if full else init[None, :].expand(n, dim))
  u, last, inv = _last_positions(ids)
  s0 = tier.stats()
  rows, where = tier.find_or_insert_planned(plan, init, return_where=True, verify=True)
  eb = dim * tdt.itemsize
  want_u = np.stack([truth.rows[k][:eb] if k in truth.rows else init_bits[l] for k, l in zip(u.tolist(), last.tolist())])
  bad = (_bits(rows) != want_u[inv]).any(1)
  assert not bad.any(), "%d positions hold another row than their key's (classes %s)" % (
      int(bad.sum()), np.bincount(np.array([cls_of[k] for k in ids[bad].tolist()]), minlength=3))
  want_where = np.array([cls_of[k] for k in ids.tolist()], np.uint8)
  np.testing.assert_array_equal(where.cpu().numpy(), want_where)
  truth.missed += int((cls != 1).sum())
  truth.lower_hits += int((cls == 2).sum())
  for k, l in zip(u.tolist(), last.tolist()):
    if k not in truth.rows:                   # [init[L(k)] | slot vectors at aux_init]
      truth.rows[k] = np.concatenate([init_bits[l]] + aux_bits)
  truth.after_call(distinct, "the planned call")
  s = tier.stats()
  assert s["not_resident"] == s0["not_resident"] == 0 and bool(upper.contains(dk).all())
  assert s["missed"] - s0["missed"] == int((cls != 1).sum()) < n      # per distinct key, not per position


# ---- 2. a loop: keys go down and come up again with their slots -------------------------------------------------------------------------
LOOP_SEED, LOOP_UNIVERSE, LOOP_BATCH, LOOP_STEPS = 19, 3000, 300, 12


def _loop_batches(seed=LOOP_SEED, steps=LOOP_STEPS):
  rng = np.random.default_rng(seed)
  universe = np.unique(rng.integers(1, 2**40, size=LOOP_UNIVERSE + 50, dtype=np.int64))[:LOOP_UNIVERSE]
  prefill = [rng.choice(universe, size=LOOP_BATCH, replace=False) for _ in range(6)]
  batches = [rng.choice(universe, size=LOOP_BATCH, replace=True) for _ in range(steps)]
  return prefill, batches


def _pos_init(n, step):
  """numpy [n, DIM]: the init row of batch POSITION p at `step`"""
  return (np.arange(n, dtype=np.float32)[:, None] * np.float32(0.25) + np.arange(DIM, dtype=np.float32)[None, :] + np.float32(100 * (step + 1)))


def _prefilled(torch, tag, prefill):
  upper, lower, tier = _tier(torch, tag)
  truth = Truth(torch, upper, lower, tier)
  for i, ids in enumerate(prefill):
    rows = _never_seen(ids) + np.float32(0.25)
    tier.insert(_t(torch, ids), _t(torch, rows))
    truth.rows.update(zip(ids.tolist(), np.concatenate([rows, _fresh_whole(ids)[:, DIM:]], axis=1)))
    truth.after_call(ids, "prefill %d" % i)
  assert upper.size_host() > 0.9 * CAP and len(truth.rows) > CAP
  return upper, lower, tier, truth


def _expect(truth, upper, torch, ids, init):
  """what the planned call over `ids` must return and count -> (u, last, rows [n, DIM], where [n], up_before [u], known [u])"""
  u, last, inv = _last_positions(ids)
  up_before = upper.contains(_t(torch, u)).cpu().numpy()
  known = np.array([k in truth.rows for k in u.tolist()])
  rows_u = np.stack([truth.rows[k][:DIM] if k in truth.rows else init[l] for k, l in zip(u.tolist(), last.tolist())])
  where_u = np.where(up_before, 1, np.where(known, 2, 0)).astype(np.uint8)
  return u, last, rows_u[inv], where_u[inv], up_before, known


def _account(truth, u, last, init, up_before, known):
  truth.missed += int((~up_before).sum())
  truth.lower_hits += int((known & ~up_before).sum())
  for k, l in zip(u[~known].tolist(), last[~known].tolist()):
    truth.rows[k] = np.concatenate([init[l]] + [np.full(DIM, AUX_INIT[f], np.float32) for f in range(AUX)])


def test_lookup_loop_with_repeats_keeps_whole_rows(env):
  torch, _ = env
  prefill, batches = _loop_batches()
  upper, lower, tier, truth = _prefilled(torch, "plan_loop", prefill)
  for step, ids in enumerate(batches):
    init = _pos_init(ids.size, step)
    u, last, want_rows, want_where, up_before, known = _expect(truth, upper, torch, ids, init)
    assert u.size < ids.size and _saturated(u, NB) == 0
    plan = _plan(torch, ids, DIM)
    rows, where = tier.find_or_insert_planned(plan, _t(torch, init), return_where=True, verify=True)
    assert rows.cpu().numpy().tobytes() == want_rows.tobytes(), "step %d: a position holds another row than its key's" % step
    assert np.array_equal(where.cpu().numpy(), want_where), "step %d: where" % step
    _account(truth, u, last, init, up_before, known)
    truth.after_call(u, "step %d, lookup" % step)
    ut = _t(torch, u)
    assert tier.stats()["not_resident"] == 0 and bool(upper.contains(ut).all())
    # "training": new embedding AND new slot vectors for the distinct keys, written into the upper table
    old = np.stack([truth.rows[k] for k in u.tolist()])
    new = old * np.float32(0.5) + np.float32(step + 1)
    for f in range(AUX + 1):
      upper.upsert(ut, _t(torch, new[:, f * DIM:(f + 1) * DIM]), unique_keys=f == 0, field=f)
    truth.rows.update(zip(u.tolist(), new))
  s = tier.stats()
  assert s["demoted"] > 0 and s["lower_hits"] > 100        # keys went down and came up again, slot vectors and all


# ---- 3. admit-only ----------------------------------------------------------------------------------------------------------------------
def test_admit_planned_hands_nothing_back(env, monkeypatch):
  torch, _ = env
  prefill, batches = _loop_batches(seed=23, steps=2)
  upper, lower, tier, truth = _prefilled(torch, "plan_admit", prefill)
  calls = Calls(monkeypatch)
  deltas = []
  for form, ids in zip(("admit", "full"), batches):
    init = _pos_init(ids.size, 0)
    u, last, want_rows, want_where, up_before, known = _expect(truth, upper, torch, ids, init)
    assert _saturated(u, NB) == 0 and (~known).any() and (known & ~up_before).any() and up_before.any()
    plan = _plan(torch, ids, DIM)
    sent_rows = torch.full((ids.size, DIM), -9.0, device="cuda")        # never passed: what a stray write would hit
    sent_where = torch.full((ids.size,), 7, dtype=torch.uint8, device="cuda")
    s0, c0 = tier.stats(), calls[NAME]
    if form == "admit":
      assert tier.admit_planned(plan, _t(torch, init), verify=True) is None
    else:
      rows, where = tier.find_or_insert_planned(plan, _t(torch, init), return_where=True, verify=True)
      assert rows.cpu().numpy().tobytes() == want_rows.tobytes() and np.array_equal(where.cpu().numpy(), want_where)
    assert calls[NAME] == c0 + 1 and calls["tfra_tier_find_or_insert"] == 0
    assert bool((sent_rows == -9.0).all()) and bool((sent_where == 7).all())
    _account(truth, u, last, init, up_before, known)
    truth.after_call(u, form)                     # the invariant, and calls / missed / lower_hits / demoted as the dictionary counts them
    s = tier.stats()
    assert s["not_resident"] == 0 and bool(upper.contains(_t(torch, u)).all())
    deltas.append((s["calls"] - s0["calls"], s["missed"] - s0["missed"] == int((~up_before).sum()),
                   s["lower_hits"] - s0["lower_hits"] == int((known & ~up_before).sum())))
  assert deltas[0] == deltas[1] == (1, True, True)


# ---- 4. the plan still serves the write-back -------------------------------------------------------------------------------------------
def test_the_plan_still_serves_the_write_back(env):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable
  prefill, batches = _loop_batches(seed=29, steps=1)
  upper, lower, tier, truth = _prefilled(torch, "plan_wb", prefill)
  ids = batches[0]
  init = _pos_init(ids.size, 0)
  u, last, want_rows, _, up_before, known = _expect(truth, upper, torch, ids, init)
  assert _saturated(u, NB) == 0 and (~known).any() and (known & ~up_before).any() and up_before.any()
  # a roomy twin that holds the whole rows of the batch's known keys
  twin = _DeviceTable(torch.int64, torch.float32, torch.zeros(DIM), "tierplan_wb_twin", "cuda:0", dim=DIM, aux_fields=AUX, init_capacity=1 << 12,
                      aux_init=AUX_INIT)
  kk = u[known]
  whole = np.stack([truth.rows[k] for k in kk.tolist()])
  for f in range(AUX + 1):
    twin.upsert(_t(torch, kk), _t(torch, whole[:, f * DIM:(f + 1) * DIM]), unique_keys=f == 0, field=f)
  plan, plan_twin = _plan(torch, ids, DIM), _plan(torch, ids, DIM)
  before = plan.read()
  rows = tier.find_or_insert_planned(plan, _t(torch, init), verify=True)
  rows_twin = twin.find_or_insert_planned(plan_twin, _t(torch, init))
  assert rows.cpu().numpy().tobytes() == want_rows.tobytes() and torch.equal(rows, rows_twin)
  after = plan.read()
  assert before[0] == after[0]
  for x, y in zip(before[1:], after[1:]):
    np.testing.assert_array_equal(x, y)           # the call left the plan as it was
  ut = _t(torch, u)
  assert tier.stats()["not_resident"] == 0 and bool(upper.contains(ut).all())
  # gradients that are multiples of 1/64: the sum over an id's positions is exact in any order
  grads = _t(torch, (np.random.default_rng(3).integers(-64, 65, size=(ids.size, DIM)) / 64.0).astype(np.float32))
  p = de.optimizers.Adam(0.01).params(1)
  default = torch.zeros(DIM, device="cuda")
  upper.apply_planned(p, plan, grads, default)
  twin.apply_planned(p, plan_twin, grads, default)
  for f in range(AUX + 1):
    a, b = upper.find(ut, field=f), twin.find(ut, field=f)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "field %d differs from the twin's after the write-back" % f
  assert not torch.equal(upper.find(_t(torch, ids)), rows), "the write-back moved nothing"
  upper.check_errors()
  lower.check_errors()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def _raw(tier, plan, init, full, out, where, flags=0):
  """the C call itself on buffers of the test (any of them None = NULL)"""
  import torch
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _ptr, _stream
  try:
    _capi.call(NAME, tier._h, None if plan is None else plan._h, _ptr(init), int(full), _ptr(out), _ptr(where), flags, _stream(tier._upper.device))
  finally:
    torch.cuda.synchronize()


def test_refusals_name_the_function_and_change_nothing(env):
  torch, _ = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  prefill, _ = _loop_batches(seed=31, steps=0)
  upper, lower, tier, _ = _prefilled(torch, "plan_refuse", prefill)
  ids = np.repeat(np.arange(1, 9, dtype=np.int64) * 15485863, 3)
  n = ids.size
  init = _t(torch, _pos_init(n, 0))
  flat = torch.full((n * DIM + 4,), -9.0, device="cuda")
  out, odd = flat[:n * DIM].view(n, DIM), flat[1:n * DIM + 1].view(n, DIM)
  assert out.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 4
  where = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
  dev = torch.device("cuda:0")
  good = _plan(torch, ids, DIM)
  many = np.arange(1, MAX_BATCH + 2, dtype=np.int64)
  big_init = torch.zeros((many.size, DIM), device="cuda")
  big_out = torch.full((many.size, DIM), -9.0, device="cuda")
  state = lambda: (upper.size_host(), lower.size_host(), tier.stats())
  before = state()
  cases = [("a plan of another dim", _plan(torch, ids, 2 * DIM), init, out, 0, -1),
           ("a plan never built", SparsePlan(dev, DIM), init, out, 0, -1),
           ("a SET plan", _plan(torch, ids, 0), init, out, 0, _capi.ERR_UNSUPPORTED),
           ("more ids than max_batch", _plan(torch, many, DIM), big_init, big_out, 0, -1),
           ("unknown flag bits", good, init, out, 2, -1),
           ("NULL init_values", good, None, out, 0, -1),
           ("a NULL plan", None, init, out, 0, -1),
           ("a misaligned rows_out", good, init, odd, 0, _capi.ERR_UNSUPPORTED)]
  for tag, plan, i, o, flags, code in cases:
    with pytest.raises(_capi.TfraError) as e:
      _raw(tier, plan, i, 1, o, where, flags)
    assert e.value.code == code and NAME in str(e.value), (tag, e.value)
    assert state() == before, tag
  assert bool((flat == -9.0).all()) and bool((big_out == -9.0).all()) and bool((where == 7).all())
  with pytest.raises(ValueError):          # the Python methods check the plan's dim and its id count themselves
    tier.find_or_insert_planned(_plan(torch, ids, 2 * DIM), init)
  for call in (tier.find_or_insert_planned, tier.admit_planned):
    with pytest.raises(ValueError, match="max_batch"):
      call(_plan(torch, many, DIM), big_init)
  assert state() == before
  upper.check_errors()
  lower.check_errors()
  # the plan the refusals were tried with is unharmed
  rows, w = tier.find_or_insert_planned(good, init, return_where=True, verify=True)
  u, last, inv = _last_positions(ids)
  assert torch.equal(rows, init[_t(torch, last)][_t(torch, inv)]) and not bool(w.any())
  s = tier.stats()
  assert s["calls"] == before[2]["calls"] + 1 and s["missed"] == before[2]["missed"] + 8 and s["not_resident"] == 0
