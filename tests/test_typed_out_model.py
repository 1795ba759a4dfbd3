"""The NumPy model of the typed lookups' conversion (tests/typed_out_model.py) against independent restatements, without a GPU:
over the whole storage set of tests/numeric_edges.py — every bfloat16 tie and near-tie, every float16 tie and its float32
neighbours, 583 680 values — bfloat16 against numeric_edges.bf16_bits_like_the_kernel, float16 against an integer restatement of
round to nearest even.  The comparison is numeric_edges.assert_bits' rule: expected not NaN -> equal bits, expected NaN -> a NaN."""
import numpy as np

from tests import numeric_edges as ne
from tests import typed_out_model as tom


def _assert_rule(got, want, dtype, what):
  bad = tom.bits_mismatch(got, want, dtype)
  if bad.any():
    i = np.flatnonzero(bad)[:8]
    raise AssertionError("%s: %d of %d differ, first at %s: got %s want %s" % (
        what, int(bad.sum()), bad.size, i.tolist(), [hex(int(v)) for v in got.reshape(-1)[i]], [hex(int(v)) for v in want.reshape(-1)[i]]))


def test_storage_set_size():
  assert ne.storage_values().size == 583680


def test_bf16_model_equals_the_kernel_restatement():
  x = ne.storage_values()
  _assert_rule(tom.narrow_bits(x, "bfloat16"), ne.bf16_bits_like_the_kernel(x), "bfloat16", "bfloat16 over the storage set")


def test_f16_model_equals_integer_round_to_nearest_even():
  x = ne.storage_values()
  _assert_rule(tom.narrow_bits(x, "float16"), tom.f16_bits_by_integers(x), "float16", "float16 over the storage set")


def test_f16_integer_restatement_on_known_points():
  x = np.array([0.0, -0.0, 1.0, 65504.0, 65519.996, 65520.0, 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                2.0 ** -14, np.inf, -np.inf, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], np.float32)
  want = np.array([0x0000, 0x8000, 0x3c00, 0x7bff, 0x7bff, 0x7c00, 0x0001, 0x0000, 0x0001, 0x0400, 0x7c00, 0xfc00, 0x3c00, 0x3c02], np.uint16)
  assert tom.f16_bits_by_integers(x).tolist() == want.tolist()
  assert tom.narrow_bits(x, "float16").tolist() == want.tolist()


def test_nan_stays_nan_and_f32_is_identity():
  x = np.array([0x7fc00000, 0x7f800001, 0xffffffff, 0x7fbfffff], np.uint32).view(np.float32)
  for dt in tom.BITS16:
    assert tom.is_nan_bits(tom.narrow_bits(x, dt), dt).all()
  assert tom.narrow_bits(x, "bfloat16").tolist() == [0x7fc0, 0x7fc0, 0xffff, 0x7fff]
  y = ne.storage_values()
  assert np.array_equal(tom.narrow_bits(y, "float32"), y.view(np.uint32))


def test_widen_is_exact_and_narrow_inverts_it():
  b = np.arange(65536, dtype=np.uint16)
  for dt in tom.BITS16:
    x = tom.widen_bits(b, dt)
    assert np.array_equal(x.view(np.uint32), ne.upcast_bits(b, dt).view(np.uint32))
    back = tom.narrow_bits(x, dt)
    _assert_rule(back, b, dt, "narrow(widen(b)) for " + dt)   # every half value is a float32 value: rounding it changes nothing


def test_subnormal_results_are_kept():
  # float16's smallest subnormals and bfloat16's (= float32's upper halves): not flushed
  assert tom.narrow_bits(np.array([2.0 ** -24, 3 * 2.0 ** -24], np.float32), "float16").tolist() == [1, 3]
  x = np.array([0x00010000, 0x00018000, 0x00028000], np.uint32).view(np.float32)
  assert tom.narrow_bits(x, "bfloat16").tolist() == [1, 2, 2]
