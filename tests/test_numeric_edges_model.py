"""CPU: the references of tests/test_gpu_numeric_edges.py checked against each other, so that the GPU file compares the kernels
with something that is itself pinned.  torch's float32 -> bfloat16 / float16 conversions (the expectation there) against the
kernel's bfloat16 formula restated in NumPy and against NumPy's float16; the SGD carrier; and the places of the edge grid where the
oracle must produce a NaN, an infinity or FTRL's exact zero for the GPU cases to mean what they say."""
import numpy as np
import pytest

from oracle import optimizers as oopt
from tests import numeric_edges as ne

f32 = np.float32


@pytest.fixture(scope="module")
def torch():
  import torch
  return torch


def test_value_sets_hold_what_they_claim():
  u = ne.bf16_edge_patterns()
  assert u.size == 393216 and np.unique(u).size == u.size
  for pattern in (0x3f7f8000,    # tie whose round-up carries into the exponent (-> 0x3f80)
                  0x7f7f8000,    # tie that rounds up to infinity
                  0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7f800001, 0x7fc00000, 0xffffffff, 0x3f808000, 0x3f818000):
    assert pattern in u
  t = ne.f16_tie_values()
  assert t.size == 31744 * 6
  mids = t[1:31744 * 3:3]
  assert mids[0] == f32(2.0 ** -25) and mids[-1] == f32(65520.0)            # the first subnormal tie, the tie to infinity
  assert f32(1.5 * 2.0 ** -24) in mids and f32(1023.5 * 2.0 ** -24) in mids   # ties inside the float16 subnormal range
  assert np.array_equal(t[31744 * 3:], -t[:31744 * 3])
  assert ne.storage_values().size == 393216 + 190464


def test_bf16_formula_of_the_kernel_equals_torch(torch):
  """to_stored<TFRA_BF16>, restated: equal to torch's conversion on every pattern of the storage set — bits where the value is not
  a NaN, NaN-ness where it is."""
  x = ne.storage_values()
  mine = ne.bf16_bits_like_the_kernel(x)
  ref = torch.from_numpy(np.array(x)).to(torch.bfloat16)
  got = torch.from_numpy(mine.view(np.int16).copy()).view(torch.bfloat16)
  ne.assert_bits(torch, got, ref, "bfloat16 formula vs torch")
  assert np.array_equal(np.isnan(x), torch.isnan(got).numpy())   # a NaN stays one, nothing else becomes one


def test_bf16_ties_go_to_the_even_neighbour(torch):
  """Independent of any conversion routine: a pattern with low half 0x8000 lies midway, so the result's last bit is 0; 0x7fff goes
  down, 0x8001 up."""
  u = ne.bf16_edge_patterns()
  finite = (u & 0x7f800000) != 0x7f800000
  got = torch.from_numpy(u.view(f32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
  hi, lo = u >> 16, u & 0xffff
  want = np.select([lo == 0x8000, lo > 0x8000], [hi + (hi & 1), hi + 1], hi)
  assert np.array_equal(got[finite], want[finite])


def test_f16_conversions_of_torch_and_numpy_agree(torch):
  x = ne.storage_values()
  with np.errstate(all="ignore"):
    ref = torch.from_numpy(np.array(x).astype(np.float16).view(np.int16)).view(torch.float16)
  got = torch.from_numpy(np.array(x)).to(torch.float16)
  ne.assert_bits(torch, got, ref, "float16: torch vs numpy")
  assert np.array_equal(np.isnan(x), torch.isnan(got).numpy())


def test_f16_ties_go_to_the_even_neighbour(torch):
  """The midpoint of the float16 magnitudes with bits b and b + 1 becomes the even one of the two; its lower float32 neighbour b,
  its upper one b + 1 (b + 1 = 0x7c00 is infinity: 65520 rounds to it)."""
  t = ne.f16_tie_values()[:31744 * 3]
  got = torch.from_numpy(t.copy()).to(torch.float16).view(torch.int16).numpy().astype(np.int64).reshape(-1, 3)
  b = np.arange(31744)
  assert np.array_equal(got[:, 0], b) and np.array_equal(got[:, 2], b + 1)
  assert np.array_equal(got[:, 1], b + (b & 1))


def test_sgd_carrier_is_exact():
  """0 - 1 * (0 + (-x)) is x for every x of the storage set: the bits, except that a zero of either sign comes back as +0 and a NaN
  as some NaN."""
  x, y = ne.storage_values(), ne.sgd_carrier_result()
  nan, zero = np.isnan(x), x == 0
  assert np.array_equal(np.isnan(y), nan)
  assert np.array_equal(y[zero].view(np.uint32), np.zeros(int(zero.sum()), np.uint32))
  rest = ~nan & ~zero
  assert np.array_equal(y[rest].view(np.uint32), x[rest].view(np.uint32))


def test_upcast_by_numpy_equals_torch(torch):
  bits = np.arange(65536, dtype=np.uint16)
  for vdtype in ("float16", "bfloat16"):
    ref = torch.from_numpy(bits.view(np.int16).copy()).view(getattr(torch, vdtype)).to(torch.float32)
    ne.assert_bits(torch, torch.from_numpy(ne.upcast_bits(bits, vdtype)), ref, "up-cast " + vdtype)


def _pick(cols, **where):
  names = ("g", "p", "s1", "s2")
  m = np.ones(cols[0].size, bool)
  for k, v in where.items():
    c = cols[names.index(k)]
    m &= np.isnan(c) if isinstance(v, float) and np.isnan(v) else (c.view(np.uint32) == f32(v).view(np.uint32))
  return m


def test_oracle_places_nan_inf_and_zero_where_the_gpu_cases_rely_on_them():
  # Adagrad: a = 0, g = 0 is 0/0 without epsilon, and no update with it
  cols = ne.rule_grid("adagrad")
  m = _pick(cols, g=0.0, s1=0.0) & np.isfinite(cols[1])
  assert m.sum() >= 12
  p, a, _ = ne.oracle_step("adagrad", 1, *cols)
  assert np.isnan(p[m]).all() and (a[m] == 0).all()
  p2, a2, _ = ne.oracle_step("adagrad_v2", 1, *ne.rule_grid("adagrad_v2"))
  assert np.array_equal(p2[m].view(np.uint32), cols[1][m].view(np.uint32)) and (a2[m] == 0).all()
  # g = 2^64: g*g overflows, the accumulator is +inf and the step 0
  m = _pick(cols, g=2.0 ** 64, s1=0.25) & np.isfinite(cols[1])
  assert np.isposinf(a[m]).all() and np.array_equal(p[m], cols[1][m])
  # a subnormal gradient on a zero accumulator: g*g underflows to 0 -> g / sqrt(0) = +-inf
  m = _pick(cols, g=2.0 ** -127, p=1.0, s1=0.0)
  assert m.sum() == 1 and np.isneginf(p[m]).all()
  # ... and the smallest one does not survive lr * g either: 0/0
  m = _pick(cols, g=2.0 ** -149, p=1.0, s1=0.0)
  assert m.sum() == 1 and np.isnan(p[m]).all()
  # FTRL: |z| == l1 -> exactly 0; one ulp outside -> not 0.  (g = 0, p = 0: z is the stored linear value.)
  cols = ne.rule_grid("ftrl")
  p, a, z = ne.oracle_step("ftrl", 1, *cols)
  base = _pick(cols, g=0.0, p=0.0, s1=1.0)
  for sign in (1.0, -1.0):
    l1 = f32(sign) * ne.L1
    on = base & _pick(cols, s2=l1)
    out = base & _pick(cols, s2=np.nextafter(l1, f32(sign * np.inf)))
    inside = base & _pick(cols, s2=np.nextafter(l1, f32(0)))
    assert on.sum() >= 1 and out.sum() == 1 and inside.sum() == 1   # (1e-3 is a member of EDGE too)
    assert (z[on] == l1).all() and not p[on].view(np.uint32).any()
    assert not p[inside].view(np.uint32).any()
    assert p[out][0] != 0 and np.sign(p[out][0]) == -sign
  # Adam: a NaN in g reaches p, m and v
  cols = ne.rule_grid("adam")
  for step in (1, 1000):
    p, m_, v = ne.oracle_step("adam", step, *cols)
    nan_g = np.isnan(cols[0])
    assert np.isnan(p[nan_g]).all() and np.isnan(m_[nan_g]).all() and np.isnan(v[nan_g]).all()


def test_adam_params_equal_the_oracles_lr_t():
  """The lr_t the kernels are handed (Adam.params(t).lr, a C float) is the oracle's, bit for bit; steps 1 and 1000 are the ones the
  GPU cases use."""
  import tfra_amd.dynamic_embedding as de
  h = ne.HYPER["adam"]
  opt = de.optimizers.Adam(h["lr"], h["beta1"], h["beta2"], h["eps"])
  for t in (1, 2, 999, 1000, 1023, 1024, 1025, 4999):
    want = oopt.adam_lr_t(h["lr"], h["beta1"], h["beta2"], t)
    assert f32(opt.params(t).lr).view(np.uint32) == want.view(np.uint32), t


def test_rule_case_is_consistent(torch):
  """The batch builder: per-key sums in input order, the three repeat counts present, new rows from the float default."""
  c = ne.RuleCase(torch, "adagrad", 1, "bfloat16", 4, True)
  n_keys = c.keys.size
  assert np.unique(c.keys).size == n_keys and c.n_res == -(-27 * 27 * 13 // 4)
  cnt = np.bincount(np.searchsorted(np.sort(c.keys), c.ids))
  assert set(cnt.tolist()) == {1, 2, 8}
  # key 2 (of the resident ones) occurs 8 times: its sum is the sequential one
  pos = np.nonzero(c.ids == c.keys[2])[0]
  acc = np.zeros(4, f32)
  with np.errstate(all="ignore"):
    for q in pos:
      acc = acc + c.grads[q]
  assert pos.size == 8 and np.array_equal(acc.view(np.uint32), c.gsum[2].view(np.uint32))
  assert np.array_equal(c.in_p[c.n_res:], np.full((n_keys - c.n_res, 4), 0.3, f32))
  assert np.array_equal(c.in_s1[c.n_res:], np.full((n_keys - c.n_res, 4), 0.1, f32))
  # resident values are storage values
  assert np.array_equal(ne.through_storage(torch, c.p0, "bfloat16").view(np.uint32), c.p0.view(np.uint32))
  # 0.3 / 0.1 are not: a row that started from the rounded default would differ
  assert ne.through_storage(torch, np.array([0.3, 0.1], f32), "bfloat16").tolist() != [float(f32(0.3)), float(f32(0.1))]
