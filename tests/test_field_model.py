"""CPU self-test of tests/field_model.py: the image of aux_init in every value dtype against byte strings worked out by hand,
and the model's rules on a small dictionary."""
import numpy as np
import pytest

from tests import field_model as fm

AUX = (0.1, -2.75, 3.0, 0.0)

# little-endian bytes of one element, by hand:
#   float32   0.1 = 0x3DCCCCCD (1.6 * 2^-4, mantissa 0x4CCCCD rounded up), -2.75 = -1.375 * 2^1 = 0xC0300000, 3.0 = 0x40400000
#   float16   0.1: exponent -4 + 15 = 11 -> 0x2C00, mantissa 0.6 * 1024 = 614.4 -> 614 = 0x266: 0x2E66;
#             -2.75: sign | (1 + 15) << 10 | 0.375 * 1024 = 0x8000 | 0x4000 | 0x180 = 0xC180; 3.0 = 0x4000 | 0x200 = 0x4200
#   bfloat16  the top half of the float32 pattern, round to nearest even on the lower half: 0x3DCC|CCCD -> lower half above
#             0x8000, up: 0x3DCD; 0xC030|0000 -> 0xC030; 0x4040|0000 -> 0x4040
#   int32 / int8   truncation toward zero: 0, -2, 3, 0 in two's complement
#   int64 / float64   aux_init is ignored: 0
EXPECT = {
    "float32": ["cdcccc3d", "000030c0", "00004040", "00000000"],
    "float16": ["662e", "80c1", "0042", "0000"],
    "bfloat16": ["cd3d", "30c0", "4040", "0000"],
    "int32": ["00000000", "feffffff", "03000000", "00000000"],
    "int8": ["00", "fe", "03", "00"],
    "int64": ["00" * 8] * 4,
    "float64": ["00" * 8] * 4,
}


@pytest.mark.parametrize("dtype_name", sorted(EXPECT))
def test_aux_init_image_bytes(dtype_name):
  for f, x in enumerate(AUX):
    img = np.array([fm.aux_image(dtype_name, x)], dtype=fm.STORAGE[dtype_name])
    assert img.tobytes().hex() == EXPECT[dtype_name][f], (dtype_name, f)


@pytest.mark.parametrize("dtype_name", ["float32", "float16", "bfloat16", "int32", "int8"])
def test_aux_init_image_matches_torch_cast(dtype_name):
  """The hand-made bytes once more from torch.tensor(x).to(dtype) (the 8-byte types are an exception of the engine, not a cast)."""
  import torch
  for f, x in enumerate(AUX):
    t = torch.tensor([x], dtype=torch.float32).to(getattr(torch, dtype_name))
    assert t.view(torch.uint8).numpy().tobytes().hex() == EXPECT[dtype_name][f], (dtype_name, f)


def test_bf16_rounding_ties_to_even_and_nan():
  f = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x7FC00001, 0xFF800001], np.uint32).view(np.float32)
  assert fm.f32_to_bf16_bits(f).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x7FC0, 0xFFC0]
  b = np.array([0x3F80, 0xC030], np.uint16)
  assert fm.bf16_bits_to_f32(b).tolist() == [1.0, -2.75]


@pytest.mark.parametrize("dtype_name", sorted(EXPECT))
def test_model_rules(dtype_name):
  dim, S = 3, 4
  m = fm.FieldModel(dtype_name, dim, S, AUX)
  v = lambda *x: fm.from_float(dtype_name, np.array(x, np.float32).reshape(-1, dim))
  zero = np.zeros(dim, m.st)
  aux_rows = [np.full(dim, m.aux[f], m.st) for f in range(4)]
  # new key through insert_or_assign; the last occurrence of a repeated key wins
  m.insert_or_assign([7, 9, 7], v(1, 2, 3, 4, 5, 6, 7, 8, 9))
  assert m.size() == 2
  assert np.array_equal(m.rows[7][0], v(7, 8, 9)[0]) and np.array_equal(m.rows[9][0], v(4, 5, 6)[0])
  for f in range(1, 5):
    assert np.array_equal(m.rows[7][f], aux_rows[f - 1])
  # existing key: only the named field changes
  m.insert_field(2, [7], v(10, 11, 12))
  assert np.array_equal(m.rows[7][0], v(7, 8, 9)[0]) and np.array_equal(m.rows[7][2], v(10, 11, 12)[0])
  assert np.array_equal(m.rows[7][1], aux_rows[0]) and np.array_equal(m.rows[7][3], aux_rows[2])
  m.insert_or_assign([7], v(1, 1, 1))
  assert np.array_equal(m.rows[7][2], v(10, 11, 12)[0])
  # new key through insert_field: field 0 zeros, the other aux fields aux_init
  m.insert_field(3, [5], v(2, 2, 2))
  assert np.array_equal(m.rows[5][0], zero) and np.array_equal(m.rows[5][3], v(2, 2, 2)[0])
  assert np.array_equal(m.rows[5][1], aux_rows[0]) and np.array_equal(m.rows[5][2], aux_rows[1]) and np.array_equal(m.rows[5][4], aux_rows[3])
  # the four accumulate cases
  m.accum_or_assign([7, 9, 100, 101], v(1, 2, 3, 9, 9, 9, 4, 4, 4, 5, 5, 5), [True, False, False, True])
  assert np.array_equal(m.rows[7][0], fm.add_rows(dtype_name, v(1, 1, 1)[0], v(1, 2, 3)[0]))
  assert np.array_equal(m.rows[9][0], v(4, 5, 6)[0])            # present & !exists
  assert np.array_equal(m.rows[100][0], v(4, 4, 4)[0]) and np.array_equal(m.rows[100][2], aux_rows[1])
  assert 101 not in m.rows                                        # absent & exists
  assert np.array_equal(m.rows[7][2], v(10, 11, 12)[0])           # accumulate touches field 0 only
  # find: broadcast and per-position defaults
  d1 = v(8, 8, 8)[0]
  rows, ex = m.find_field(2, [7, 1234, 9], d1)
  assert ex.tolist() == [True, False, True]
  assert np.array_equal(rows, np.stack([v(10, 11, 12)[0], d1, aux_rows[1]]))
  dn = v(1, 1, 1, 2, 2, 2, 3, 3, 3)
  rows, ex = m.find_field(0, [1234, 7, 4321], dn)
  assert np.array_equal(rows[0], dn[0]) and np.array_equal(rows[2], dn[2]) and ex.tolist() == [False, True, False]
  with pytest.raises(ValueError):
    m.find_field(5, [7], d1)
  with pytest.raises(ValueError):
    m.insert_field(-1, [7], v(1, 1, 1))
  # erase / clear: a key that comes back starts from aux_init again
  m.erase([7, 555])
  assert 7 not in m.rows and m.size() == 3
  m.insert_or_assign([7], v(3, 3, 3))
  assert np.array_equal(m.rows[7][2], aux_rows[1])
  m.clear()
  assert m.size() == 0


def test_add_rows_rounds_once_and_wraps():
  a = np.array([1.0], np.float16)
  assert fm.add_rows("float16", a, np.array([2.0 ** -11], np.float16)).tolist() == [1.0]        # tie -> even
  assert fm.add_rows("int8", np.array([127], np.int8), np.array([1], np.int8)).tolist() == [-128]
  one = fm.from_float("bfloat16", np.array([1.0]))
  assert fm.add_rows("bfloat16", one, fm.from_float("bfloat16", np.array([2.0 ** -8]))).tolist() == [0x3F80]   # tie -> even
  assert fm.as_bytes(np.zeros((2, 3), np.float16)).shape == (2, 6)
