"""TEST INFRASTRUCTURE ONLY — the edge grids, the batches and the references of the fused Momentum / Nesterov / RMSProp rules
(TFRA_OPT_MOMENTUM, TFRA_OPT_NESTEROV, TFRA_OPT_RMSPROP), shared by tests/test_gpu_fused_rules.py (the HIP kernels on a GPU) and
tests/test_fused_rules_model.py (the same references checked against SparseOptimizerOracle without one).

Built from the blocks of tests/numeric_edges.py — EDGE, NONNEG, pack_rows, row_keys, repeat_counts, OCC_SCALE, through_storage —
the way its RuleCase is built for the four earlier rules; FusedCase carries the same attributes, so that the drivers of
tests/test_gpu_numeric_edges.py (seed_rows, check_rows, write_back) serve it unchanged."""
import numpy as np

from oracle import optimizers as oopt
from tests.numeric_edges import DEFAULT, EDGE, NONNEG, OCC_SCALE, pack_rows, repeat_counts, row_keys, through_storage

f32 = np.float32

INITIAL_RMS = 0.1   # RMSProp's initial ms: not a bfloat16 (or float16) value, as numeric_edges.INIT_ACC
# the hyper-parameters of test_k13_fused_optimizer_matches_reference_sequence (tests/test_gpu_frontend.py: OPTS)
HYPER = {
    "momentum": dict(lr=0.05, momentum=0.9),
    "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True),
    "rmsprop": dict(lr=0.01, rho=0.9, momentum=0.5, eps=1e-10, initial_rms=INITIAL_RMS),
}
RULES = ["momentum", "nesterov", "rmsprop"]
ORACLE_KIND = {"momentum": "momentum", "nesterov": "momentum", "rmsprop": "rmsprop"}   # SparseOptimizerOracle's names


def n_slots(rule):
  return 2 if rule == "rmsprop" else 1


def new_row_slots(rule):
  """(s1, s2) a never-seen key starts from: the optimizer's aux_init."""
  return (INITIAL_RMS, 0.0) if rule == "rmsprop" else (0.0, 0.0)


def rule_grid(rule):
  """The Cartesian product of the rule's value classes, flat float32 arrays (g, p, s1, s2), s2 None for the momentum rules:
  momentum / nesterov g, p, accum in EDGE^3 (19 683 elements); rmsprop g, p in EDGE, ms in NONNEG, mom in EDGE (255 879)."""
  axes = [EDGE, EDGE, NONNEG, EDGE] if rule == "rmsprop" else [EDGE, EDGE, EDGE]
  cols = [m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")]
  return tuple(cols + [None] * (4 - len(cols)))


def oracle_step(rule, g, p, s1, s2):
  """ONE call of oracle.optimizers.momentum / rmsprop -> (p, s1, s2) float32, s2 None for the momentum rules."""
  h = HYPER[rule]
  with np.errstate(all="ignore"):
    if rule == "rmsprop":
      return oopt.rmsprop(p, s1, s2, g, h["lr"], h["rho"], h["momentum"], h["eps"])
    p, a = oopt.momentum(p, s1, g, h["lr"], h["momentum"], h.get("nesterov", False))
    return p, a, None


def make_opt(de, rule, fused=True):
  h = HYPER[rule]
  if rule == "rmsprop":
    return de.optimizers.RMSProp(h["lr"], h["rho"], h["momentum"], h["eps"], h["initial_rms"], fused=fused)
  return de.optimizers.Momentum(h["lr"], h["momentum"], use_nesterov=h.get("nesterov", False), fused=fused)


def batch_over(n_keys, repeats, seed):
  """Key index per batch position, shuffled, and each position's occurrence number of its key (input order)."""
  rng = np.random.default_rng(seed)
  idx = np.repeat(np.arange(n_keys), repeat_counts(n_keys, repeats))
  rng.shuffle(idx)
  order = np.argsort(idx, kind="stable")
  occ = np.empty(idx.size, dtype=np.int64)
  occ[order] = np.arange(idx.size) - np.searchsorted(idx[order], idx[order], side="left")
  return idx, occ


class FusedCase:
  """numeric_edges.RuleCase for `rule` in RULES: one batch over the rule's edge grid for rows of `dim` elements of `vdtype`.

  Resident keys `keys[:n_res]` hold p0 / s10 / s20 (the grid rounded to the storage type first); the keys behind them were never
  seen and start from `default` and the rule's aux_init as FLOATS.  ids [n] (with `repeats` a key occurs 1, 2 or 8 times — 8 is
  the longest list the kernels sum strictly in input order), grads [n, dim].  want_p / want_s1 / want_s2 [n_keys, dim] float32: the
  rule applied ONCE to segment_sum_by_key's sums (without `repeats`: to the gradients themselves), before the one conversion."""

  def __init__(self, torch, rule, vdtype, dim, repeats, default=DEFAULT):
    self.rule, self.step, self.vdtype, self.dim = rule, 1, vdtype, dim
    g, p, s1, s2 = rule_grid(rule)
    S = n_slots(rule)
    a1, a2 = new_row_slots(rule)
    G = pack_rows(g, dim, 0.0)
    self.n_res = n_res = G.shape[0]
    self.p0 = through_storage(torch, pack_rows(p, dim, 0.0), vdtype)
    self.s10 = through_storage(torch, pack_rows(s1, dim, 1.0 if rule == "rmsprop" else 0.0), vdtype)
    self.s20 = through_storage(torch, pack_rows(s2, dim, 0.0), vdtype) if S >= 2 else None
    n_abs = max(2, -(-EDGE.size // dim))
    G = np.concatenate([G, np.resize(EDGE, n_abs * dim).reshape(n_abs, dim)])
    n_keys = n_res + n_abs
    self.keys = np.concatenate([row_keys(n_res), -np.arange(1, n_abs + 1, dtype=np.int64) * 104729])
    idx, occ = batch_over(n_keys, repeats, dim * 1000 + n_keys % 997)
    with np.errstate(all="ignore"):
      self.grads = (G[idx] * OCC_SCALE[occ][:, None]).astype(f32)
      uniq, gsum, _ = oopt.segment_sum_by_key(idx, self.grads)
    self.idx = idx
    self.ids = self.keys[idx]
    self.gsum = gsum[np.argsort(uniq)] if repeats else G.astype(f32)
    self.in_p = np.concatenate([self.p0, np.full((n_abs, dim), default, f32)])
    self.in_s1 = np.concatenate([self.s10, np.full((n_abs, dim), a1, f32)])
    self.in_s2 = np.concatenate([self.s20, np.full((n_abs, dim), a2, f32)]) if S >= 2 else None
    self.want_p, self.want_s1, self.want_s2 = oracle_step(rule, self.gsum, self.in_p, self.in_s1, self.in_s2)

  def context(self, i):
    """The operands of flat element i, as floats and as bits."""
    def one(a):
      if a is None:
        return "-"
      v = a.reshape(-1)[i:i + 1]
      return "%r/%08x" % (float(v[0]), int(v.view(np.uint32)[0]))
    return "(%s, g %s, p %s, s1 %s, s2 %s)%s" % (self.rule, one(self.gsum), one(self.in_p), one(self.in_s1), one(self.in_s2),
                                                 "" if i < self.n_res * self.dim else " new row")


_case_cache = {}


def fused_case(torch, rule, vdtype, dim, repeats, default=DEFAULT):
  """FusedCase, the last few kept: the routes of one (rule, vdtype, dim) share one reference and leave it unchanged."""
  key = (rule, vdtype, dim, bool(repeats), float(default))
  if key not in _case_cache:
    while len(_case_cache) >= 3:
      _case_cache.pop(next(iter(_case_cache)))
    _case_cache[key] = FusedCase(torch, rule, vdtype, dim, repeats, default)
  return _case_cache[key]
