"""CPU: the references of tests/test_gpu_fused_rules.py checked without a GPU — tests/fused_rules_edges.py's one-step results
against SparseOptimizerOracle's write-back sequence over CpuTables on the same batch, and the condition on the inputs that keeps a
kernel which confuses Momentum with Nesterov from passing."""
import numpy as np
import pytest

import oracle
from oracle import optimizers as oopt
from tests import fused_rules_edges as fe
from tests import numeric_edges as ne

f32 = np.float32


@pytest.fixture(scope="module")
def torch():
  import torch
  return torch


def test_grids_have_the_sizes_the_cases_are_budgeted_for():
  assert fe.rule_grid("momentum")[0].size == fe.rule_grid("nesterov")[0].size == 27 ** 3
  assert fe.rule_grid("rmsprop")[0].size == 27 * 27 * 13 * 27 == 255879   # numeric_edges' Adam grid has the same size
  assert fe.rule_grid("rmsprop")[2].min() >= 0                           # ms: the accumulator class
  assert fe.rule_grid("momentum")[3] is None


def same_bits(a, b, what):
  a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
  nan = np.isnan(b)
  bad = np.where(nan, ~np.isnan(a), a.view(np.uint32) != b.view(np.uint32))
  assert not bad.any(), "%s: %d of %d elements differ" % (what, int(bad.sum()), bad.size)


@pytest.mark.parametrize("rule", fe.RULES)
@pytest.mark.parametrize("vdtype,dim", [("float32", 68), ("bfloat16", 4)])
def test_references_equal_the_sparse_optimizer_oracle(torch, rule, vdtype, dim):
  """One SparseOptimizerOracle.apply over CpuTables seeded with the case's resident rows, on the case's batch (ids repeating 1, 2
  and 8 times): the parameter and every slot of every key are the case's want_* — bits, or a NaN where a NaN is expected."""
  c = fe.FusedCase(torch, rule, vdtype, dim, True)
  S = fe.n_slots(rule)
  a1, a2 = fe.new_row_slots(rule)
  assert np.array_equal(np.unique(np.bincount(c.idx)), [1, 2, 8])
  assert c.in_p[c.n_res:].view(np.uint32).tolist() == [[int(f32(ne.DEFAULT).view(np.uint32))] * dim] * (c.keys.size - c.n_res)
  tabs = [oracle.CpuTable(dim) for _ in range(1 + S)]
  kres = c.keys[:c.n_res]
  for t, rows in zip(tabs, (c.p0, c.s10, c.s20)):
    t.insert(kres, rows)
  ora = oopt.SparseOptimizerOracle(fe.ORACLE_KIND[rule], tabs[0], tabs[1:], fe.HYPER[rule], ne.DEFAULT)
  with np.errstate(all="ignore"):
    ora.apply(c.ids, c.grads)
  for name, t, want, init in zip(("p", "s1", "s2"), tabs, (c.want_p, c.want_s1, c.want_s2), (ne.DEFAULT, a1, a2)):
    got, ex = t.find(c.keys, np.full(dim, init, f32), return_exists=True)
    assert np.asarray(ex).all()
    same_bits(got, want, "%s %s dim %d: %s" % (rule, vdtype, dim, name))


def test_momentum_and_nesterov_differ_on_the_grid(torch):
  """A condition on the INPUTS: where both rules give a finite parameter, they give different ones for at least 20 % of the
  elements — a kernel that runs one rule for the other kind cannot pass the GPU cases.  The accumulators are equal everywhere."""
  for vdtype, dim in (("float32", 4), ("float16", 68), ("bfloat16", 68)):
    m = fe.FusedCase(torch, "momentum", vdtype, dim, False)
    n = fe.FusedCase(torch, "nesterov", vdtype, dim, False)
    same_bits(m.want_s1, n.want_s1, "accum")
    finite = np.isfinite(m.want_p) & np.isfinite(n.want_p)
    differ = float(np.mean(m.want_p[finite] != n.want_p[finite]))
    print("%s dim %d: %d finite elements, %.1f %% differ" % (vdtype, dim, int(finite.sum()), 100 * differ))
    assert finite.sum() > 5000 and differ >= 0.20, (vdtype, dim, differ)


def test_rmsprop_grid_meets_its_edges():
  """Where the GPU cases rely on the oracle for a NaN, an infinity and a zero denominator: ms = 0 with g = 0 divides 0 by
  sqrt(eps) (no NaN: eps is added inside the root), g = 2^64 overflows g * g, and a NaN gradient reaches all three results."""
  g, p, ms, mom = fe.rule_grid("rmsprop")
  wp, wms, wmom = fe.oracle_step("rmsprop", g, p, ms, mom)
  z = (g == 0) & (ms == 0) & (np.abs(p) <= 3) & (np.abs(mom) <= 3)   # (p - momentum * mom cannot overflow)
  assert z.any() and np.isfinite(wp[z]).all() and (wms[z] == 0).all()
  big = (np.abs(g) == f32(2.0 ** 64)) & np.isfinite(ms)
  assert big.any() and np.isinf(wms[big]).all()
  nan = np.isnan(g)
  assert np.isnan(wp[nan]).all() and np.isnan(wms[nan]).all() and np.isnan(wmom[nan]).all()
