"""CPU-only: tests/half_grads_model.py — G32[e] = f32(grads[e]) * s, the definition of the *_typed write-backs — against torch on the
CPU (`.to(torch.float32) * s`) over all 65 536 patterns of float16 and of bfloat16: NaN-ness agrees, everything else bit for bit."""
import numpy as np
import pytest

from tests import half_grads_model as hm


@pytest.mark.parametrize("scale", [None] + list(hm.SCALES), ids=lambda s: "none" if s is None else "%g" % s)
@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_model_equals_torch_on_every_pattern(fmt, scale):
  import torch
  bits = hm.all_patterns()
  t = hm.from_bits(torch, bits, fmt)
  assert np.array_equal(hm.bits_of(torch, t), bits)
  want = t.to(torch.float32)
  if scale is not None:
    want = want * torch.tensor(float(scale), dtype=torch.float32)
  want = want.numpy()
  got = hm.g32(bits, fmt, scale)
  assert got.dtype == np.float32 and got.shape == bits.shape
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan)
  bad = np.nonzero(~nan & (got.view(np.uint32) != want.view(np.uint32)))[0]
  assert bad.size == 0, "%s scale %r: %d patterns differ, first %04x: model %08x torch %08x" % (
      fmt, scale, bad.size, bits[bad[0]], got.view(np.uint32)[bad[0]], want.view(np.uint32)[bad[0]])


@pytest.mark.parametrize("fmt", hm.FORMATS)
def test_no_scale_is_the_exact_upcast_and_equals_scale_one(fmt):
  import torch
  bits = hm.all_patterns()
  up = hm.upcast(bits, fmt)
  want = hm.from_bits(torch, bits, fmt).to(torch.float32).numpy()
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(up), nan) and np.array_equal(up.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
  a, b = hm.g32(bits, fmt, None), hm.g32(bits, fmt, 1.0)
  assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]) and np.array_equal(a.view(np.uint32)[~nan], up.view(np.uint32)[~nan])
  sub = (np.abs(up) > 0) & (np.abs(up) < np.float32(2.0 ** -126 if fmt == "bfloat16" else 2.0 ** -14))
  assert sub.sum() == (254 if fmt == "bfloat16" else 2046)   # every subnormal of the format is kept, none flushed


def test_the_subnormal_scale_reaches_rounded_float32_subnormals():
  g = hm.g32(hm.all_patterns(), "bfloat16", hm.SUBNORMAL_SCALE)
  sub = np.isfinite(g) & (np.abs(g) > 0) & (np.abs(g) < np.float32(2.0 ** -126))
  assert sub.sum() > 1000
  with np.errstate(all="ignore"):
    exact = hm.upcast(hm.all_patterns(), "bfloat16").astype(np.float64) * float(hm.SUBNORMAL_SCALE)
  assert (g[sub].astype(np.float64) != exact[sub]).any()   # some of those products were rounded: the one rounding is exercised
