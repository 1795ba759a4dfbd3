"""GPU: a grouped call refuses what its single-table call refuses, with the same code and the same words.

Each case makes ONE faulty argument set and gives it to the single C entry point (tfra_table_apply_planned_combined /
tfra_table_find_combine) and, as a lone descriptor, to the grouped one (tfra_multi_apply_planned_combined /
tfra_multi_find_combine).  Both run one function per operation for their checks (check_apply_combined + check_apply_planned,
csrc/tfra_apply.h; check_find_combine, csrc/tfra_pool.hip), so: the codes are equal, the grouped text behind "descriptor 0: " is
a prefix of the single text behind its "name: " (the single call may add a hint), and neither call writes anything — every input
here is refused on the host, before any launch."""
import ctypes

import pytest

from tests import sparse_helpers as H

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def last_error():
  from tfra_amd import _capi
  return _capi.lib().tfra_last_error().decode()


def assert_parity(single, grouped):
  """single / grouped: (code, tfra_last_error text) of the two calls."""
  (rc1, msg1), (rc2, msg2) = single, grouped
  assert rc1 == rc2 and rc1 != 0, (single, grouped)
  assert "descriptor 0: " in msg2 and ": " in msg1, (msg1, msg2)
  tail1, tail2 = msg1.split(": ", 1)[1], msg2.split("descriptor 0: ", 1)[1]
  assert tail2 and tail1.startswith(tail2), (msg1, msg2)


def table_state(torch, t):
  """Keys, value bits and score-free export of a CuckooHashTable, key-sorted."""
  k, v = t.export()
  o = torch.argsort(k)
  return [k[o], v[o].contiguous().view(torch.uint8)]


# ---- the combined write-back ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def writeback(env):
  """Three tables of dim 64 with Adam's slots, N_ROWS rows each (the shapes of test_gpu_combined_many's bad-descriptor test), an
  int8 table and a table without slot fields."""
  torch, de = env
  opt = H.opt_of(de, "adam")
  cases = [H.Case(torch, de, opt, "ep_w%d" % i, 64, seed=60 + i) for i in range(3)]
  t8 = de.CuckooHashTable(torch.int64, torch.int8, torch.zeros(64, dtype=torch.int8), name="ep_i8", dim=64, aux_fields=2)
  t8.insert(torch.arange(8, device="cuda"), torch.ones((8, 64), device="cuda").to(torch.int8))
  bare = H.make_var(torch, de, H.opt_of(de, "sgd"), "ep_bare", 64)
  return opt, cases, t8, bare


def single_apply(torch, e):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.table_ops import _stream
  dev = torch.device("cuda", torch.cuda.current_device())
  P = ctypes.c_void_p
  rc = _capi.lib().tfra_table_apply_planned_combined(P(e.table), ctypes.cast(P(e.opt), ctypes.POINTER(_capi.OptParams)), P(e.plan),
                                                     P(e.grad_out), P(e.seg), P(e.weights), e.combiner, e.n_rows,
                                                     P(e.param_default_row), _stream(dev))
  return rc, last_error()


WRITEBACK_FAULTS = ["int8_table", "misaligned_grad_out", "combiner_3", "plan_of_another_dim", "adam_without_slots", "null_grad_out",
                    "n_rows_0"]


@pytest.mark.parametrize("what", WRITEBACK_FAULTS)
def test_write_back_single_and_grouped_refuse_alike(env, writeback, what):
  torch, de = env
  from tfra_amd.dynamic_embedding.table_ops import SparsePlan
  opt, cases, t8, bare = writeback
  p = opt.params(1)
  case = cases[WRITEBACK_FAULTS.index(what) % 3]
  req = case.request(torch, 1)
  e = H.desc_of(torch, req, p)
  keep, want = [req], INVALID
  sgd = H.opt_of(de, "sgd")
  watched = [lambda: table_state(torch, t8), lambda: H._export_state(torch, de, de.DynamicEmbeddingOptimizer(sgd), sgd, bare)]
  deo = de.DynamicEmbeddingOptimizer(opt)
  watched += [lambda c=c: H._export_state(torch, de, deo, opt, c.var) for c in cases]
  if what == "int8_table":
    e.table, want = t8._table._h.value, UNSUPPORTED
  elif what == "misaligned_grad_out":
    G = torch.zeros(H.N_ROWS * 64 + 4, device="cuda")[1:1 + H.N_ROWS * 64].view(H.N_ROWS, 64)
    keep.append(G)
    e.grad_out, want = G.data_ptr(), UNSUPPORTED
    assert G.data_ptr() % 16 == 4
  elif what == "combiner_3":
    e.combiner = 3
  elif what == "plan_of_another_dim":
    pl = SparsePlan(case.var._primary, 32).build(case.ids)
    keep.append(pl)
    e.plan = pl._h.value
  elif what == "adam_without_slots":
    e.table = bare._tables[0]._table._h.value
  elif what == "null_grad_out":
    e.grad_out = None                                                      # (the plan holds ids)
    assert case.plan.n > 0
  elif what == "n_rows_0":
    e.n_rows = 0
  before = [w() for w in watched]
  torch.cuda.synchronize()
  single = single_apply(torch, e)
  rc, launches, msg = H.raw_many(torch, [e])
  print(what, "single:", single, "grouped:", (rc, msg))
  assert single[0] == want
  assert launches == 0
  assert_parity(single, (rc, msg))
  torch.cuda.synchronize()
  for b, w in zip(before, watched):
    for x, y in zip(b, w()):
      assert torch.equal(x, y)


# ---- the pooled lookup ------------------------------------------------------------------------------------------------------------
def single_find(torch, t, e):
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _stream
  dev = t._table.device
  P = ctypes.c_void_p
  rc = _capi.lib().tfra_table_find_combine(P(e.table), _workspace(dev), e.nnz, P(e.ids), P(e.seg), P(e.weights), e.combiner, e.n_rows,
                                           P(e.default_row), P(e.out), _stream(dev))
  return rc, last_error()


LOOKUP_FAULTS = ["int8", "combiner3", "misaligned_out", "null_out", "null_ids", "dim6"]


@pytest.mark.parametrize("bad", LOOKUP_FAULTS)
def test_lookup_single_and_grouped_refuse_alike(env, bad):
  """4 rows of 2 entries each: the shape of test_gpu_pooled_many's bad-descriptor test."""
  torch, de = env
  from tfra_amd import _capi
  t = H.table(torch, de, "cuckoo", "float32", 64)
  if bad in ("dim6", "int8"):
    dim, dt = (6, torch.float32) if bad == "dim6" else (8, torch.int8)
    t = de.CuckooHashTable(torch.int64, dt, torch.zeros(dim, dtype=dt), name="ep_bad_" + bad, dim=dim)
    t.insert(torch.arange(8, device="cuda"), torch.ones((8, dim), device="cuda").to(dt))
  ids_t = torch.arange(8, device="cuda")
  seg_t = torch.arange(8, device="cuda") // 2
  out = torch.full((4, t._table.dim + 4), 7.0, device="cuda")
  descs = (_capi.FindCombineDesc * 1)()
  e = descs[0]
  H._desc(e, t, ids_t, seg_t, 4, out)
  want = UNSUPPORTED
  if bad == "combiner3":
    e.combiner, want = 3, INVALID
  elif bad == "misaligned_out":
    e.out = out.data_ptr() + 4
  elif bad == "null_out":
    e.out, want = None, INVALID
  elif bad == "null_ids":
    e.ids, want = None, INVALID
    assert e.nnz > 0
  before = table_state(torch, t)
  torch.cuda.synchronize()
  single = single_find(torch, t, e)
  launches = ctypes.c_uint32(99)
  grouped = H._raw(torch, descs, launches=launches)
  print(bad, "single:", single, "grouped:", grouped)
  assert single[0] == want
  assert launches.value == 0
  assert_parity(single, grouped)
  torch.cuda.synchronize()
  assert bool((out == 7.0).all())
  for x, y in zip(before, table_state(torch, t)):
    assert torch.equal(x, y)
