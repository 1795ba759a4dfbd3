"""TEST INFRASTRUCTURE ONLY — the conversion of the typed lookups (include/tfra_mi355x.h, tfra_rows_out) restated in NumPy, shared
by tests/test_typed_out_model.py (checked against independent restatements, no GPU) and the GPU tests of the typed lookups.

The contract: a typed call equals its untyped twin followed by the elementwise conversion of the twin's output.  The conversion:
  float32 -> bfloat16   f32_to_bf16 (csrc/tfra_device.h): u + 0x7fff + ((u >> 16) & 1), high half; a NaN keeps its high half and gets
                        bit 0x40 set
  float32 -> float16    the hardware's round to nearest even (the _Float16 cast) = NumPy's astype(float16)
  half -> float32       the exact up-cast
  half -> other half    through float32: up-cast, then the rounding above
Bits are compared by numeric_edges.assert_bits' rule: expected not NaN -> equal bits, expected NaN -> a NaN."""
import numpy as np

f32 = np.float32
BITS16 = ("float16", "bfloat16")


def narrow_bits(x32, dtype):
  """float32 [..] -> the bits of the typed lookups' output in `dtype`: uint32 for "float32" (the value itself), uint16 otherwise."""
  x = np.ascontiguousarray(x32, f32)
  if dtype == "float32":
    return x.view(np.uint32).copy()
  if dtype == "float16":
    with np.errstate(all="ignore"):
      return x.astype(np.float16).view(np.uint16)
  assert dtype == "bfloat16", dtype
  u = x.view(np.uint32)
  nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
  r = ((u.astype(np.uint64) + np.uint64(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)
  return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def widen_bits(bits16, dtype):
  """uint16 [..] patterns of a half type -> their exact float32 values."""
  b = np.ascontiguousarray(bits16).view(np.uint16)
  if dtype == "float16":
    return b.view(np.float16).astype(f32)
  assert dtype == "bfloat16", dtype
  return (b.astype(np.uint32) << np.uint32(16)).view(f32)


def is_nan_bits(bits, dtype):
  b = np.asarray(bits)
  if dtype == "float32":
    return (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
  if dtype == "float16":
    return (b & np.uint16(0x7fff)) > np.uint16(0x7c00)
  return (b & np.uint16(0x7fff)) > np.uint16(0x7f80)


def bits_mismatch(got, want, dtype):
  """bool [..]: where `got` breaks the rule against `want` (both bit patterns of `dtype`)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
  return np.where(is_nan_bits(want, dtype), ~is_nan_bits(got, dtype), got != want)


def f16_bits_by_integers(x32):
  """float32 -> float16 bits, round to nearest even, in integer arithmetic alone (an independent restatement for the model's own
  test): the 24-bit significand is shifted to float16's position — 13 bits for a normal result, more inside the subnormal range —
  and rounded by the shifted-out bits; a carry out of the significand runs into the exponent, and past the largest finite value
  into infinity, by plain addition.  A NaN gives a quiet NaN."""
  u = np.ascontiguousarray(x32, f32).view(np.uint32).astype(np.uint64)
  sign = ((u >> np.uint64(16)) & np.uint64(0x8000))
  e = ((u >> np.uint64(23)) & np.uint64(0xff)).astype(np.int64)
  m = (u & np.uint64(0x7fffff))
  out = np.zeros(u.shape, np.uint64)
  nan = (e == 255) & (m != 0)
  inf = (e == 255) & (m == 0)
  # finite: value = sig * 2^(e' - 150) with sig = m | 2^23 (normal, e' = e) or m (float32 subnormal, e' = 1)
  sig = np.where(e == 0, m, m | np.uint64(0x800000))
  e1 = np.where(e == 0, 1, e)
  he = e1 - 127 + 15                       # float16's biased exponent of the leading bit 2^23
  shift = np.where(he >= 1, 13, 14 - he)   # bits to drop: 13 for a normal result, more for a subnormal one
  shift = np.minimum(shift, 40).astype(np.uint64)
  kept = sig >> shift
  rem = sig & ((np.uint64(1) << shift) - np.uint64(1))
  half = np.uint64(1) << (shift - np.uint64(1))
  up = (rem > half) | ((rem == half) & ((kept & np.uint64(1)) == 1))
  kept = kept + up.astype(np.uint64)
  # normal: kept has the hidden bit at 2^10: bits = ((he - 1) << 10) + kept, the carry running into the exponent; subnormal: bits = kept
  base = np.where(he >= 1, (np.maximum(he, 1) - 1).astype(np.uint64) << np.uint64(10), np.uint64(0))
  fin = base + kept
  fin = np.where(fin >= np.uint64(0x7c00), np.uint64(0x7c00), fin)   # past 65504 (and 65520, the tie): infinity
  out = np.where(nan, np.uint64(0x7e00), np.where(inf, np.uint64(0x7c00), fin))
  return (out | sign).astype(np.uint16)


def convert_tensor(torch, t, out_dtype):
  """The model applied to a float32 / float16 / bfloat16 CPU tensor -> a CPU tensor of torch dtype `out_dtype` (its bits)."""
  name = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
  src, dst = name[t.dtype], name[out_dtype]
  t = t.detach().cpu().contiguous()
  if src == "float32":
    x = t.numpy()
  else:
    x = widen_bits(t.view(torch.int16).numpy().view(np.uint16), src)
  bits = narrow_bits(x, dst)
  if dst == "float32":
    return torch.from_numpy(bits.view(f32).copy()).reshape(t.shape)
  return torch.from_numpy(bits.view(np.int16).copy()).view(out_dtype).reshape(t.shape)
