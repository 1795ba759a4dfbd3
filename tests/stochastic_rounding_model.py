"""TEST INFRASTRUCTURE ONLY — a NumPy model of TFRA_OPTION_STOCHASTIC_ROUNDING (include/tfra_mi355x.h): the hash that
gives every stored element its 16 random bits, the rounding rule for both storage types, and "oracle rule, then stochastic
rounding" for the fused optimizers.  tests/test_stochastic_rounding_model.py checks it against the contract's known answers
without a GPU; tests/test_gpu_stochastic_rounding.py compares what the HIP kernels store with it, bit for bit.

The rule is stated here the way the contract states it — lo, hi and F as VALUES, in float64, where every quantity is exact — and
not as the kernels' bit tricks, so that the two are two derivations of one result."""
import functools

import numpy as np

from oracle import optimizers as oopt
from tests import numeric_edges as ne

f32 = np.float32
u64 = np.uint64
GAMMA = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


# ---- the random bits ----------------------------------------------------------------------------------------------------------
def mix64(z):
  """The splitmix64 finalizer, element-wise on uint64 (arithmetic mod 2^64)."""
  z = np.asarray(z, dtype=u64)
  with np.errstate(over="ignore"):
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    return z ^ (z >> u64(31))


def call_word(seed, call):
  """a = mix64(seed + call * GAMMA): one per write-back."""
  return mix64(u64((int(seed) + int(call) * GAMMA) & _M64))


def key_words(seed, call, keys):
  """b = mix64(a ^ key): uint64 [n_keys]."""
  return mix64(call_word(seed, call) ^ np.ascontiguousarray(keys, np.int64).view(u64))


def element_words(seed, call, keys, e):
  """w = mix64(b + ((e >> 2) + 1) * GAMMA) for every key and every element index e: uint64 [n_keys, len(e)]."""
  e = np.asarray(e, dtype=u64).reshape(-1)
  with np.errstate(over="ignore"):
    return mix64(key_words(seed, call, keys).reshape(-1, 1) + ((e >> u64(2)) + u64(1))[None, :] * u64(GAMMA))


def random_bits(seed, call, keys, dim, field):
  """r of the elements of field `field` (0 parameter, 1 and 2 the slots) of the rows of `keys`: uint32 [n_keys, dim]."""
  e = np.arange(dim, dtype=np.int64) + field * dim
  w = element_words(seed, call, keys, e)
  return ((w >> (u64(16) * (e.astype(u64) & u64(3)))[None, :]) & u64(0xffff)).astype(np.uint32)


# ---- the rounding rule ---------------------------------------------------------------------------------------------------------
def _grid_f16(ax):
  """|x| float64, finite and below 2^16 -> (lo16, lo value, hi value): lo = |x| toward zero on the float16 grid, hi the next value
  (0x7bff + 1 = 0x7c00 stands for the continued step 2^16)."""
  with np.errstate(over="ignore"):
    h = ax.astype(np.float16)           # to nearest: at most one step above
  lo16 = h.view(np.uint16).astype(np.int64)
  lo16 = lo16 - (np.where(np.isinf(h), np.inf, h.astype(np.float64)) > ax)
  val = lambda b: np.where(b >= 0x7c00, 65536.0, np.minimum(b, 0x7bff).astype(np.uint16).view(np.float16).astype(np.float64))
  return lo16, val(lo16), val(lo16 + 1)


def _grid_bf16(ax):
  """The same for bfloat16, |x| finite: the grid is the float32 values whose low half is 0; 0x7f7f + 1 = 0x7f80 stands for 2^128."""
  lo16 = (ax.astype(f32).view(np.uint32) >> 16).astype(np.int64)
  val = lambda b: np.where(b >= 0x7f80, 2.0 ** 128, (np.minimum(b, 0x7f7f).astype(np.uint32) << 16).view(f32).astype(np.float64))
  return lo16, val(lo16), val(lo16 + 1)


def fraction(x, vdtype):
  """(F, lo16) of finite values below the continued step: F = 65536 (|x| - |lo|) / (|hi| - |lo|), exact in float64."""
  ax = np.abs(np.asarray(x, f32).astype(np.float64))
  lo16, lo, hi = (_grid_f16 if vdtype == "float16" else _grid_bf16)(ax)
  return 65536.0 * (ax - lo) / (hi - lo), lo16


def nearest_bits(x, vdtype):
  """The nearest-even storage bits (uint16), by NumPy alone; a NaN is some NaN."""
  x = np.ascontiguousarray(x, f32)
  if vdtype == "float16":
    with np.errstate(over="ignore"):
      return x.astype(np.float16).view(np.uint16)
  return ne.bf16_bits_like_the_kernel(x)


def stochastic_bits(x, r, vdtype):
  """The storage bits (uint16, the shape of x) of float32 x rounded with the random bits r: hi iff 65536 - r <= F; the sign is
  kept; infinities, NaNs and |x| at or beyond the continued step as nearest-even stores them."""
  x = np.ascontiguousarray(x, f32)
  r = np.broadcast_to(np.asarray(r, dtype=np.int64), x.shape)
  top = 65536.0 if vdtype == "float16" else np.inf
  with np.errstate(invalid="ignore"):
    plain = ~(np.abs(x.astype(np.float64)) < top)     # NaN included
  safe = np.where(plain, f32(0), x)
  F, lo16 = fraction(safe, vdtype)
  mag = lo16 + ((65536 - r) <= F)
  sign = (x.view(np.uint32) >> 16) & 0x8000
  return np.where(plain, nearest_bits(x, vdtype), (sign | mag).astype(np.uint16)).astype(np.uint16)


def stochastic_field(x, vdtype, seed, call, keys, field):
  """Rows x [n_keys, dim] of field `field` as the write-back `call` of a table seeded `seed` stores them: uint16 [n_keys, dim]."""
  x = np.ascontiguousarray(x, f32)
  return stochastic_bits(x, random_bits(seed, call, keys, x.shape[1], field), vdtype)


def as_tensor(torch, bits16, vdtype):
  """uint16 bits -> CPU tensor of the storage type."""
  return torch.from_numpy(np.ascontiguousarray(bits16).view(np.int16).copy()).view(getattr(torch, vdtype))


# ---- the storage set of the GPU tests -------------------------------------------------------------------------------------------
N_MIDDLE = 196608


@functools.lru_cache(maxsize=None)
def storage_values():
  """float32 [780288 = 3048 * 256], read-only: numeric_edges.storage_values() — every bfloat16 tie pattern and every float16 tie —
  and behind it N_MIDDLE values with random low bits in the normal float16 range, whose fraction between two float16 neighbours
  lies in [1/4, 3/4).  Why the second part: every comparison of the GPU tests asks that at least 20 % of its elements differ from
  the nearest-even bits, so that a kernel that ignores the option cannot pass.  On the first part alone the model differs in 25.0 %
  for bfloat16 but in 17.1 % for float16 (most bfloat16 patterns are float16 values, or lie outside its range); the second part
  differs in 3/8 of its elements for float16 and in 1/4 for bfloat16 (its low halves are random), which lifts float16 to 22 %."""
  rng = np.random.default_rng(20261020)
  mag = rng.integers(0x0400, 0x7c00, size=N_MIDDLE).astype(np.uint16).view(np.float16).astype(f32).view(np.uint32)
  low = (rng.integers(1, 3, size=N_MIDDLE) << 11) | rng.integers(0, 1 << 11, size=N_MIDDLE)     # 13 bits, the top two 01 or 10
  sign = rng.integers(0, 2, size=N_MIDDLE).astype(np.uint32) << 31
  x = np.concatenate([ne.storage_values(), (mag | low.astype(np.uint32) | sign).view(f32)])
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def sgd_carrier_result():
  """numeric_edges.sgd_carrier_result() over storage_values() above: what the oracle leaves in a row of 0 after one SGD step with
  lr = 1 and the gradient -x, each key once, computed by segment_sum_by_key + sgd.  float32, read-only."""
  x = storage_values()
  with np.errstate(all="ignore"):
    uniq, gsum, _ = oopt.segment_sum_by_key(np.arange(x.size, dtype=np.int64), (-x).reshape(-1, 1))
    assert np.array_equal(uniq, np.arange(x.size))
    out = oopt.sgd(np.zeros((x.size, 1), f32), gsum, 1.0).reshape(-1)
  out.setflags(write=False)
  return out


# ---- oracle rule, then stochastic rounding ------------------------------------------------------------------------------------------
def oracle_step(rule, step, g, p, s1, s2, hyper=None):
  """numeric_edges.oracle_step — ONE call of oracle.optimizers' rule -> (p, s1, s2) — with the hyper-parameters `hyper` instead of
  numeric_edges.HYPER[rule] where given."""
  if hyper is None:
    return ne.oracle_step(rule, step, g, p, s1, s2)
  h = hyper
  with np.errstate(all="ignore"):
    if rule == "sgd":
      return oopt.sgd(p, g, h["lr"]), None, None
    if rule == "adam":
      return oopt.adam(p, s1, s2, g, h["lr"], h["beta1"], h["beta2"], h["eps"], step)
    if rule in ("adagrad", "adagrad_v2"):
      p, a = oopt.adagrad(p, s1, g, h["lr"], h["eps"])
      return p, a, None
    return oopt.ftrl(p, s1, s2, g, h["lr"], h["l1"], h["l2"], h["lr_power"])


def stochastic_step(rule, step, g, p, s1, s2, vdtype, seed, call, keys, hyper=None):
  """oracle.optimizers' rule on float32 rows [n_keys, dim] (oracle_step), then the rounding of the parameter and of every slot
  the rule owns: (bits_p, bits_s1, bits_s2) uint16, None where the rule has no such slot, and the float32 results."""
  outs = oracle_step(rule, step, g, p, s1, s2, hyper)
  bits = tuple(None if o is None else stochastic_field(o, vdtype, seed, call, keys, f) for f, o in enumerate(outs))
  return bits, outs


def differing_fraction(bits, x, vdtype):
  """The share of elements whose stochastic bits are not the nearest-even ones (NaNs count as equal)."""
  x = np.ascontiguousarray(x, f32)
  return float(np.mean((np.asarray(bits) != nearest_bits(x, vdtype)) & ~np.isnan(x)))
