"""CPU: the NumPy model of the stochastic rounding (tests/stochastic_rounding_model.py) against the contract of
TFRA_OPTION_STOCHASTIC_ROUNDING — the hash's known answers, the rule by enumeration of all 65536 values of the random bits, the
uniformity of the bits, and the two cases that motivate the mode: a bfloat16 parameter and Adam's v that stop moving under
nearest-even rounding and follow the float32 result in the mean under stochastic rounding."""
import numpy as np
import pytest

from tests import numeric_edges as ne
from tests import stochastic_rounding_model as srm

f32 = np.float32
ALL_R = np.arange(65536, dtype=np.int64)


def bits_f32(u):
  return np.array([u], np.uint32).view(f32)[0]


# ---- the hash ------------------------------------------------------------------------------------------------------------------
def test_mix64_is_the_published_splitmix64_finalizer():
  got = [int(srm.mix64(np.uint64((n * srm.GAMMA) & ((1 << 64) - 1)))) for n in (1, 2, 3)]
  assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_element_words_known_answers():
  assert int(srm.element_words(1, 0, np.array([0], np.int64), [0])[0, 0]) == 0x4181B152FB77616F
  w = srm.element_words(1, 1, np.array([-1], np.int64), [20, 21, 22, 23])[0]
  assert [int(x) for x in w] == [0xE63101E98C52059D] * 4
  # the four elements of a granule take the four 16-bit fields of that word, element 0 the lowest; dim 8, field 2 = elements 16..23
  r = srm.random_bits(1, 1, np.array([-1], np.int64), 8, 2)[0]
  assert [int(x) for x in r[4:]] == [0x059D, 0x8C52, 0x01E9, 0xE631]


def test_random_bits_are_uniform():
  """The mean of r / 65536 over N elements lies within 5 standard errors (0.2887 / sqrt(N)) of 0.5."""
  keys = ne.row_keys(4080)
  r = np.concatenate([srm.random_bits(0x5eed, 3, keys, 32, f).reshape(-1) for f in range(3)])
  assert r.size == 391680 and int(r.max()) < 65536
  assert abs(float(np.mean(r / 65536.0)) - 0.5) <= 5 * 0.2887 / np.sqrt(r.size)


# ---- the rule, by enumeration -------------------------------------------------------------------------------------------------
ENUM = [
    # (storage type, float32 bits, times rounded up out of 65536)
    ("bfloat16", 0x3f808000, 32768),
    ("bfloat16", 0x3f800001, 1),
    ("bfloat16", 0xbf80ffff, 65535),          # negative: away from zero
    ("bfloat16", 0x7f7f8000, 32768),          # the top interval: hi is the continued step, stored as infinity
    ("bfloat16", 0x00000001, 1),              # the smallest float32 subnormal
    ("bfloat16", 0x3f800000, 0),              # representable
    ("bfloat16", 0x80000000, 0),              # -0
    ("float16", int(np.array([1 + 2.0 ** -13], f32).view(np.uint32)[0]), 8192),
    ("float16", int(np.array([2.0 ** -20 + 2.0 ** -30], f32).view(np.uint32)[0]), 1024),   # the subnormal range
    ("float16", int(np.array([-(2.0 ** -24) * 0.75], f32).view(np.uint32)[0]), 49152),    # below the smallest subnormal, negative
    ("float16", int(np.array([2.0 ** -24 * (1 + 2.0 ** -20)], f32).view(np.uint32)[0]), 0),  # F = 2^-4: a dyadic fraction, floor 0
    ("float16", int(np.array([65520.0], f32).view(np.uint32)[0]), 32768),                  # the top interval 65504 .. 2^16
    ("float16", int(np.array([0.333251953125], f32).view(np.uint32)[0]), 0),               # representable (0x3555)
    ("float16", 0x00000001, 0),               # a float32 subnormal: F = 2^-109
]


@pytest.mark.parametrize("vdtype,u,ups", ENUM, ids=["%s-%08x" % (v, u) for v, u, _ in ENUM])
def test_rule_by_enumeration_of_the_random_bits(vdtype, u, ups):
  """Over all 65536 values of r: every result is lo or hi, and hi comes floor(F) times — the exact fraction where F is an integer."""
  x = np.full(65536, bits_f32(u), f32)
  F, lo16 = srm.fraction(x[:1], vdtype)
  assert int(np.floor(F[0])) == ups
  got = srm.stochastic_bits(x, ALL_R, vdtype).astype(np.int64)
  sign = (u >> 16) & 0x8000
  lo, hi = sign | int(lo16[0]), sign | (int(lo16[0]) + 1)
  assert set(np.unique(got).tolist()) <= {lo, hi}
  assert int((got == hi).sum()) == ups
  # lo is x toward zero: its value does not exceed |x|, and hi's does (the continued step counts as its value)
  top = 65536.0 if vdtype == "float16" else 2.0 ** 128
  val = lambda b: min(top, abs(float(ne.upcast_bits(np.array([b], np.uint16), vdtype).astype(np.float64)[0])))
  assert val(lo) <= abs(float(x[0])) < val(hi) or (ups == 0 and val(lo) == abs(float(x[0])))


def test_the_top_interval_stores_infinity_and_beyond_it_nearest_even():
  x = np.array([65520.0, -65520.0, 65536.0, 1e30, np.inf, -np.inf], f32)
  got = srm.stochastic_bits(x, np.full(x.size, 65535), "float16")
  assert got.tolist() == [0x7c00, 0xfc00, 0x7c00, 0x7c00, 0x7c00, 0xfc00]
  y = np.array([bits_f32(0x7f7f0001), bits_f32(0xff7f0001), np.inf, -np.inf], f32)
  assert srm.stochastic_bits(y, np.full(y.size, 65535), "bfloat16").tolist() == [0x7f80, 0xff80, 0x7f80, 0xff80]
  assert srm.stochastic_bits(y[:2], np.zeros(2, np.int64), "bfloat16").tolist() == [0x7f7f, 0xff7f]
  for vdtype in ("float16", "bfloat16"):
    nan = srm.stochastic_bits(np.array([np.nan], f32), [12345], vdtype)
    assert np.isnan(ne.upcast_bits(nan, vdtype)[0])


@pytest.mark.parametrize("vdtype", ["float16", "bfloat16"])
def test_the_bit_forms_of_the_contract(vdtype):
  """bfloat16: (bits + r) >> 16.  Normal float16: add r >> 3 to the bits, clear the low 13, convert."""
  rng = np.random.default_rng(7)
  if vdtype == "bfloat16":
    u = rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7fffffff) < 0x7f800000]
    r = rng.integers(0, 65536, size=u.size)
    want = ((u.astype(np.uint64) + r.astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)
  else:
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-13, 15, size=200000))).astype(f32)
    x = x[(np.abs(x) >= 2.0 ** -14) & (np.abs(x) < 65504)]
    u, r = x.view(np.uint32), rng.integers(0, 65536, size=x.size)
    v = ((u + (r >> 3).astype(np.uint32)) & np.uint32(0xffffe000)).view(f32)
    with np.errstate(over="ignore"):
      want = v.astype(np.float16).view(np.uint16)
  got = srm.stochastic_bits(u.view(f32), r, vdtype)
  assert np.array_equal(got, want)
  assert 0.20 <= float(np.mean(got != srm.nearest_bits(u.view(f32), vdtype))) <= 0.30   # random low bits: a quarter differs


def test_a_quarter_of_the_finite_bfloat16_edge_patterns_differs_from_nearest_even():
  u = ne.bf16_edge_patterns()
  x = u[(u & 0x7fffffff) < 0x7f800000].view(f32)
  r = srm.random_bits(11, 0, np.arange(x.size // 6, dtype=np.int64), 6, 0).reshape(-1)
  frac = srm.differing_fraction(srm.stochastic_bits(x, r, "bfloat16"), x, "bfloat16")
  assert abs(frac - 0.25) < 0.005, frac


# ---- why the mode exists -----------------------------------------------------------------------------------------------------
N_EL, N_STEPS = 4096, 1000


def _train(update, start, vdtype, stochastic):
  """N_STEPS write-backs of one row of N_EL independent elements held in `vdtype`; update: float32 row -> float32 row."""
  keys = np.array([77], np.int64)
  x = ne.upcast_bits(srm.nearest_bits(np.full((1, N_EL), start, f32), vdtype), vdtype)
  for call in range(N_STEPS):
    y = update(x)
    bits = srm.stochastic_field(y, vdtype, 0xabcdef, call, keys, 0) if stochastic else srm.nearest_bits(y, vdtype)
    x = ne.upcast_bits(bits, vdtype).reshape(1, N_EL)
  return x.reshape(-1).astype(np.float64)


def _within_five_standard_errors(sample, target):
  se = float(np.std(sample, ddof=1)) / np.sqrt(sample.size)
  assert se > 0 and abs(float(np.mean(sample)) - target) <= 5 * se, (float(np.mean(sample)), target, se)


def test_sgd_on_a_bfloat16_parameter_moves_only_with_stochastic_rounding():
  """A parameter at 1.0 takes 1000 steps of lr * g = 1e-3 (the bfloat16 ulp at 1.0 is 2^-7): float32 ends at 0, nearest-even at
  exactly 1.0, the stochastic mean within 5 standard errors of the float32 result."""
  step = lambda x: (x - f32(1e-3) * f32(1.0)).astype(f32)
  ref = f32(1.0)
  for _ in range(N_STEPS):
    ref = f32(ref - f32(1e-3) * f32(1.0))
  assert abs(float(ref)) < 1e-4
  assert np.all(_train(step, 1.0, "bfloat16", False) == 1.0)
  _within_five_standard_errors(_train(step, 1.0, "bfloat16", True), float(ref))


def test_adams_v_on_bfloat16_moves_only_with_stochastic_rounding():
  """v += (g*g - v)(1 - beta2), beta2 = 0.999, from 0.01 with g*g = 0.04: float32 ends at 0.02897, nearest-even at 0.0100098 (one
  move, then the relative step of 0.1 % is below half an ulp), the stochastic mean within 5 standard errors of float32."""
  gg, omb = f32(0.04), f32(1) - f32(0.999)
  step = lambda v: (v + (gg - v) * omb).astype(f32)
  ref = f32(0.01)
  for _ in range(N_STEPS):
    ref = f32(ref + f32(gg - ref) * omb)
  assert abs(float(ref) - 0.02897) < 1e-5
  rne = _train(step, 0.01, "bfloat16", False)
  assert np.all(rne == rne[0]) and abs(rne[0] - 0.0100098) < 1e-7
  _within_five_standard_errors(_train(step, 0.01, "bfloat16", True), float(ref))
