"""TEST INFRASTRUCTURE ONLY — the value sets, the batches and the bit comparison shared by tests/test_gpu_numeric_edges.py (the
HIP kernels on a GPU) and tests/test_numeric_edges_model.py (the same references checked against each other without one).

Three things live here so that both files work on THE SAME inputs:
  * the storage set: float32 values at which a conversion to bfloat16 / float16 can go wrong (every bfloat16 tie and near-tie,
    every float16 tie and its two float32 neighbours), and the SGD carrier that brings a value x through a write-back unchanged;
  * the edge grid of the fused rules: the Cartesian product of the value classes at which an update rule meets a subnormal, a zero
    accumulator, an overflowing g*g, an infinity, a NaN or FTRL's |z| == l1 boundary, packed into the rows of one batch;
  * the comparison rule: expected not NaN -> the stored bits are equal; expected NaN -> the result is a NaN (payload free)."""
import functools

import numpy as np

from oracle import optimizers as oopt

f32 = np.float32

# ---- 1. the storage set -----------------------------------------------------------------------------------------------------
LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)


def bf16_edge_patterns():
  """uint32 [65536 * 6]: every high half with the low halves at which round-to-nearest-even decides — 0x8000 the tie, 0x7fff /
  0x8001 its neighbours, 0x0000 / 0x0001 / 0xffff the ends.  Holds the carry into the exponent (0x..7fffff8000), the round-up to
  infinity (0x7f7f8000), the float32 subnormals, both infinities and NaNs of every kind."""
  hi = np.arange(65536, dtype=np.uint32) << 16
  return (hi[:, None] | np.array(LOW_HALVES, np.uint32)[None, :]).reshape(-1)


def f16_tie_values():
  """float32 [31744 * 3 * 2]: for every pair of adjacent float16 magnitudes — the 31744 finite ones, the last pair being 65504 and
  2^16, where infinity starts, so that its midpoint is 65520, the tie to infinity — the float32 midpoint and its two float32
  neighbours, with both signs.  The pairs inside the float16 subnormal range (spacing 2^-24) are among them."""
  lo = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
  hi = np.append(lo[1:], 65536.0)
  mid64 = (lo + hi) / 2
  mid = mid64.astype(f32)
  assert np.array_equal(mid.astype(np.float64), mid64)   # 12 significant bits: exact in float32
  trio = np.stack([np.nextafter(mid, f32(0)), mid, np.nextafter(mid, f32(np.inf))], 1).reshape(-1)
  return np.concatenate([trio, -trio])


@functools.lru_cache(maxsize=None)
def storage_values():
  """float32 [393216 + 190464], read-only: the bfloat16 patterns, then the float16 ties."""
  x = np.concatenate([bf16_edge_patterns().view(f32), f16_tie_values()])
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def sgd_carrier_result():
  """What the oracle leaves in a row that held 0 after one SGD step, lr = 1, with the gradient -x, each key once:
  0 - 1 * (0 + (-x)), float32 [len(storage_values())], read-only.  It is x itself (zeros of either sign -> +0, NaN -> NaN;
  test_numeric_edges_model.py checks that), but it is COMPUTED, by segment_sum_by_key + sgd, so that the expectation of the GPU tests is
  the oracle's result and not an argument about it."""
  x = storage_values()
  with np.errstate(all="ignore"):
    uniq, gsum, _ = oopt.segment_sum_by_key(np.arange(x.size, dtype=np.int64), (-x).reshape(-1, 1))
    assert np.array_equal(uniq, np.arange(x.size))
    out = oopt.sgd(np.zeros((x.size, 1), f32), gsum, 1.0).reshape(-1)
  out.setflags(write=False)
  return out


def pack_rows(flat, dim, pad=0.0):
  """flat [n] -> [ceil(n / dim), dim], the tail of the last row filled with `pad`."""
  flat = np.asarray(flat)
  rows = -(-flat.size // dim)
  out = np.full(rows * dim, pad, dtype=flat.dtype)
  out[:flat.size] = flat
  return out.reshape(rows, dim)


def row_keys(n, stride=7919, base=13):
  """n distinct int64 keys."""
  return np.arange(n, dtype=np.int64) * stride + base


def bf16_bits_like_the_kernel(x):
  """to_stored<TFRA_BF16> (csrc/tfra_optim_device.h) restated: u + 0x7fff + ((u >> 16) & 1), high half; a NaN keeps its high half
  and gets bit 0x40 set.  float32 [n] -> uint16 [n]."""
  u = np.ascontiguousarray(x, f32).view(np.uint32)
  nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
  r = ((u.astype(np.uint64) + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
  return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def upcast_bits(bits16, vdtype):
  """The float32 value of every 16-bit storage pattern, by NumPy alone: float16 through np.float16, bfloat16 as the high half."""
  b = np.ascontiguousarray(bits16).view(np.uint16)
  if vdtype == "float16":
    return b.view(np.float16).astype(f32)
  return (b.astype(np.uint32) << 16).view(f32)


# ---- the comparison rule ------------------------------------------------------------------------------------------------------
def _hex(torch, t):
  it = {2: torch.int16, 4: torch.int32}[t.element_size()]
  return [("%0" + str(2 * t.element_size()) + "x") % (int(b) & ((1 << (8 * t.element_size())) - 1)) for b in t.view(it).tolist()]


def mismatches(torch, got, want):
  """bool tensor: the elements that break the rule.  got / want: CPU tensors of one dtype (float32 / float16 / bfloat16)."""
  assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
  it = {2: torch.int16, 4: torch.int32}[want.element_size()]
  nan = torch.isnan(want)
  return torch.where(nan, ~torch.isnan(got), got.contiguous().view(it) != want.contiguous().view(it))


def assert_bits(torch, got, want, what, context=None):
  """The rule, with a message that names the first failing elements: their flat index, the bits on both sides and, with
  `context(flat_index) -> str`, what went into them."""
  got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
  bad = mismatches(torch, got, want).reshape(-1)
  n_bad = int(bad.sum())
  if n_bad:
    idx = torch.nonzero(bad).reshape(-1)[:8]
    g, w = got.reshape(-1)[idx], want.reshape(-1)[idx]
    lines = ["%s: %d of %d elements differ" % (what, n_bad, bad.numel())]
    for i, gh, wh, gv, wv in zip(idx.tolist(), _hex(torch, g), _hex(torch, w), g.to(torch.float64).tolist(), w.to(torch.float64).tolist()):
      lines.append("  [%d] got %s (%r) want %s (%r)%s" % (i, gh, gv, wh, wv, "" if context is None else "  <- " + context(i)))
    raise AssertionError("\n".join(lines))


# ---- 3. the edge grid of the rules ----------------------------------------------------------------------------------------------
_MAGS = np.array([0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -64, 1e-3, 0.25, 1.0, 3.0, 2.0 ** 40, 2.0 ** 64,
                  float(np.finfo(f32).max), np.inf], dtype=f32)
EDGE = np.concatenate([_MAGS, -_MAGS, np.array([np.nan], f32)])   # g, p, Adam's m (2^64: g*g overflows)
NONNEG = _MAGS.copy()                                               # accumulators (0: Adagrad without epsilon meets 0/0)
assert EDGE.size == 27 and NONNEG.size == 13

DEFAULT = 0.3     # the param default of a never-seen key, and ...
INIT_ACC = 0.1    # ... Adagrad's / FTRL's initial accumulator: neither is a bfloat16 (or float16) value
L1 = f32(1e-3)
HYPER = {
    "sgd": dict(lr=0.1),
    "adam": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8),
    "adagrad": dict(lr=0.05, eps=None),
    "adagrad_v2": dict(lr=0.05, eps=1e-7),
    "ftrl": dict(lr=0.05, l1=1e-3, l2=1e-3, lr_power=-0.5),
}
RULES = [("sgd", 1), ("adam", 1), ("adam", 1000), ("adagrad", 1), ("adagrad_v2", 1), ("ftrl", 1)]   # (rule, step)


def ftrl_linear_values():
  """EDGE plus +-l1 and their float32 neighbours on both sides: |z| == l1 gives 0, the outer neighbour does not."""
  l1 = L1
  extra = [l1, -l1, np.nextafter(l1, f32(np.inf)), np.nextafter(-l1, f32(-np.inf)), np.nextafter(l1, f32(0)), np.nextafter(-l1, f32(0))]
  return np.concatenate([EDGE, np.array(extra, f32)])


def n_slots(rule):
  return {"sgd": 0, "adam": 2, "adagrad": 1, "adagrad_v2": 1, "ftrl": 2}[rule]


def new_row_slots(rule):
  """(s1, s2) a never-seen key starts from: the optimizer's aux_init."""
  return (INIT_ACC, 0.0) if rule in ("adagrad", "adagrad_v2", "ftrl") else (0.0, 0.0)


def rule_grid(rule):
  """The Cartesian product of the rule's value classes, flat float32 arrays (g, p, s1, s2), s1 / s2 None where the rule has none."""
  axes = [EDGE, EDGE]
  if rule == "adam":
    axes += [EDGE, NONNEG]
  elif rule in ("adagrad", "adagrad_v2"):
    axes += [NONNEG]
  elif rule == "ftrl":
    axes += [NONNEG, ftrl_linear_values()]
  cols = [m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")]
  return tuple(cols + [None] * (4 - len(cols)))


def oracle_step(rule, step, g, p, s1, s2):
  """ONE call of oracle.optimizers' rule -> (p, s1, s2) float32, None where the rule has no such slot."""
  h = HYPER[rule]
  with np.errstate(all="ignore"):
    if rule == "sgd":
      return oopt.sgd(p, g, h["lr"]), None, None
    if rule == "adam":
      return oopt.adam(p, s1, s2, g, h["lr"], h["beta1"], h["beta2"], h["eps"], step)
    if rule in ("adagrad", "adagrad_v2"):
      p, a = oopt.adagrad(p, s1, g, h["lr"], h["eps"])
      return p, a, None
    return oopt.ftrl(p, s1, s2, g, h["lr"], h["l1"], h["l2"], h["lr_power"])


def to_storage(torch, x, vdtype):
  """float32 ndarray -> CPU tensor of the storage type: torch's conversion, round to nearest even, ONE rounding."""
  return torch.from_numpy(np.ascontiguousarray(x, f32)).to(getattr(torch, vdtype))


def through_storage(torch, x, vdtype):
  """float32 -> storage type -> float32 (what a resident value of a half table is)."""
  if vdtype == "float32":
    return np.ascontiguousarray(x, f32)
  return to_storage(torch, x, vdtype).to(torch.float32).numpy()


OCC_SCALE = np.array([1.0, 3.0, -0.5, 1e-3, 7.0, -2.0, 0.3, 5.0], dtype=f32)   # occurrence j of a repeated id carries g * OCC_SCALE[j]


def repeat_counts(n_keys, repeats):
  """How often each key occurs in the batch: 1, 2 or 8 times (8: the longest list that is summed strictly in input order)."""
  r = np.ones(n_keys, dtype=np.int64)
  if repeats:
    i = np.arange(n_keys)
    r[i % 8 == 1] = 2
    r[i % 8 == 2] = 8
  return r


class RuleCase:
  """One batch over the edge grid of `rule` for rows of `dim` elements of `vdtype`, and what the oracle makes of it.

  resident keys: `keys[:n_res]`, holding p0 / s10 / s20 [n_res, dim] (float32 images of what is stored: the grid values rounded to
  the storage type first); absent keys: `keys[n_res:]`, never seen, which start from `default` and the rule's aux_init as FLOATS.
  The batch: ids [n] (shuffled; with `repeats` a key occurs 1, 2 or 8 times), grads [n, dim] float32.  want_p / want_s1 / want_s2
  [n_keys, dim] float32: the rule applied ONCE to the per-key sums of segment_sum_by_key (input order; without `repeats`: to the
  gradients themselves, each key occurring once), before the one conversion to the storage type.  gsum, in_p, in_s1, in_s2: the operands, for the failure message."""

  def __init__(self, torch, rule, step, vdtype, dim, repeats, default=DEFAULT):
    self.rule, self.step, self.vdtype, self.dim = rule, step, vdtype, dim
    g, p, s1, s2 = rule_grid(rule)
    S = n_slots(rule)
    a1, a2 = new_row_slots(rule)
    G = pack_rows(g, dim, 0.0)
    self.n_res = n_res = G.shape[0]
    self.p0 = through_storage(torch, pack_rows(p, dim, 0.0), vdtype)
    self.s10 = through_storage(torch, pack_rows(s1, dim, 1.0), vdtype) if S >= 1 else None
    self.s20 = through_storage(torch, pack_rows(s2, dim, 0.0), vdtype) if S >= 2 else None
    n_abs = max(2, -(-EDGE.size // dim))
    G_abs = np.resize(EDGE, n_abs * dim).reshape(n_abs, dim)
    G = np.concatenate([G, G_abs])
    n_keys = n_res + n_abs
    self.keys = np.concatenate([row_keys(n_res), -np.arange(1, n_abs + 1, dtype=np.int64) * 104729])
    # the batch: key index per position, shuffled; the j-th position of a key (in input order) is its occurrence j
    rng = np.random.default_rng(dim * 1000 + n_keys % 997)
    idx = np.repeat(np.arange(n_keys), repeat_counts(n_keys, repeats))
    rng.shuffle(idx)
    order = np.argsort(idx, kind="stable")
    first = np.searchsorted(idx[order], idx[order], side="left")
    occ = np.empty(idx.size, dtype=np.int64)
    occ[order] = np.arange(idx.size) - first
    with np.errstate(all="ignore"):
      self.grads = (G[idx] * OCC_SCALE[occ][:, None]).astype(f32)
      uniq, gsum, _ = oopt.segment_sum_by_key(idx, self.grads)
    self.ids = self.keys[idx]
    # without repeats the batch is what tfra_table_apply_optimizer takes — unique keys with their gradients AS THEY ARE (a -0 stays
    # -0; the sum's 0 + x belongs to the routes that sum)
    self.gsum = gsum[np.argsort(uniq)] if repeats else G.astype(f32)
    self.in_p = np.concatenate([self.p0, np.full((n_abs, dim), default, f32)])
    self.in_s1 = np.concatenate([self.s10, np.full((n_abs, dim), a1, f32)]) if S >= 1 else None
    self.in_s2 = np.concatenate([self.s20, np.full((n_abs, dim), a2, f32)]) if S >= 2 else None
    self.want_p, self.want_s1, self.want_s2 = oracle_step(rule, step, self.gsum, self.in_p, self.in_s1, self.in_s2)

  def context(self, i):
    """The operands of flat element i, as floats and as bits."""
    def one(a):
      if a is None:
        return "-"
      v = a.reshape(-1)[i:i + 1]
      return "%r/%08x" % (float(v[0]), int(v.view(np.uint32)[0]))
    return "(%s step %d, g %s, p %s, s1 %s, s2 %s)%s" % (self.rule, self.step, one(self.gsum), one(self.in_p), one(self.in_s1),
                                                        one(self.in_s2), "" if i < self.n_res * self.dim else " new row")


_case_cache = {}


def rule_case(torch, rule, step, vdtype, dim, repeats, default=DEFAULT):
  """RuleCase, the last few kept: the routes of one (rule, step, vdtype, dim) share one reference and leave it unchanged."""
  key = (rule, step, vdtype, dim, bool(repeats), float(default))
  if key not in _case_cache:
    while len(_case_cache) >= 3:
      _case_cache.pop(next(iter(_case_cache)))
    _case_cache[key] = RuleCase(torch, rule, step, vdtype, dim, repeats, default)
  return _case_cache[key]
