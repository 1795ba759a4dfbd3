"""TEST INFRASTRUCTURE ONLY — the NumPy model of what the *_typed write-backs read (include/tfra_mi355x.h: tfra_grads):

    G32[e] = f32(grads[e]) * s

from the 16 stored bits of a gradient element, its format and a float32 scale.  f32() is the exact up-cast — float16: sign, five
exponent bits, ten fraction bits, subnormals kept; bfloat16: the high half of a float32 — and the product is ONE float32
multiplication, rounded to nearest even on its own, float32 subnormals kept.  s = None is the call without a scale and equals
s = 1.  tests/test_half_grads_model.py checks it against torch on the CPU over all 65 536 patterns of both formats;
tests/test_gpu_half_grads.py takes its expectations from it."""
import numpy as np

f32 = np.float32
FORMATS = ("float16", "bfloat16")
SUBNORMAL_SCALE = f32(f32(1e-3) * f32(2.0 ** -10))   # small bfloat16 values (float32's exponent range) times this: float32 subnormals, rounded
SCALES = (f32(1.0), f32(2.0 ** -16), f32(1.0 / 1024), f32(1e-3), SUBNORMAL_SCALE)


def all_patterns():
  """uint16 [65536]: every stored pattern of a 16-bit format."""
  return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def upcast(bits16, fmt):
  """uint16 [...] -> float32 [...], exact, from the bits."""
  b = np.ascontiguousarray(bits16, np.uint16).astype(np.uint32)
  if fmt == "bfloat16":
    return (b << 16).view(f32)
  assert fmt == "float16", fmt
  sign, e, m = (b >> 15) << 31, (b >> 10) & 0x1f, b & 0x3ff
  # normal: rebias 15 -> 127; infinity / NaN: exponent 255, the fraction kept; subnormal and zero: m * 2^-24, exact in float32
  normal = sign | ((e + 112) << 23) | (m << 13)
  special = sign | np.uint32(0x7f800000) | (m << 13)
  small = (m.astype(f32) * f32(2.0 ** -24)).view(np.uint32) | sign
  return np.where(e == 0, small, np.where(e == 31, special, normal)).astype(np.uint32).view(f32)


def g32(bits16, fmt, scale=None):
  """uint16 [...] -> float32 [...]: the matrix the untyped twin of a typed call is given."""
  x = upcast(bits16, fmt)
  with np.errstate(all="ignore"):
    return (x * f32(1.0 if scale is None else scale)).astype(f32)


def bits_of(torch, t):
  """A float16 / bfloat16 tensor's stored bits, uint16 ndarray of its shape."""
  return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(torch, bits16, fmt):
  """uint16 ndarray -> CPU tensor of the format with exactly these bits."""
  return torch.from_numpy(np.ascontiguousarray(bits16, np.uint16).view(np.int16)).view(getattr(torch, fmt))
