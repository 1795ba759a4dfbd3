"""CPU-only: what the single pooled calls refuse before any device is needed, by code and by the COMPLETE text of tfra_last_error().
The 14 single entry points of the pooled family (forward and weight gradient; tuple and ragged; plain, typed, long, tiered) and the
four typed weight gradients beside them refuse a NULL table or tier in words of their own — the prefixes are not uniform, and that
is part of the behaviour.  The six *_typed calls refuse a bad record (tfra_rows_out, tfra_grads) before the owner is looked at, so
every call here runs with a NULL owner and NULL operands: no handle is made up."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -6
F32, F16, BF16 = 0, 1, 2

# the complete message of a NULL owner; the typed calls are given a float16 record (a float32 one forwards: below)
NULL_OWNER = {
    "tfra_table_find_combine": "find_combine: null table",
    "tfra_table_find_combine_ragged": "find_combine_ragged: null table",
    "tfra_table_find_combine_typed": "find_combine_typed: null table",
    "tfra_table_find_combine_ragged_typed": "find_combine_ragged_typed: null table",
    "tfra_table_find_combine_long": "find_combine_long: null table",
    "tfra_table_find_combine_ragged_long": "find_combine_ragged_long: null table",
    "tfra_tier_find_combine": "tfra_tier_find_combine: null tier",
    "tfra_tier_find_combine_ragged": "tfra_tier_find_combine_ragged: null tier",
    "tfra_table_find_combine_backprop_weights": "find_combine_backprop_weights (out = grad_out): null table",
    "tfra_table_find_combine_ragged_backprop_weights": "find_combine_ragged_backprop_weights (out = grad_out): null table",
    "tfra_table_find_combine_backprop_weights_long": "find_combine_backprop_weights_long (out = grad_out): null table",
    "tfra_table_find_combine_ragged_backprop_weights_long": "find_combine_ragged_backprop_weights_long (out = grad_out): null table",
    "tfra_tier_find_combine_backprop_weights": "tfra_tier_find_combine_backprop_weights: null tier",
    "tfra_tier_find_combine_ragged_backprop_weights": "tfra_tier_find_combine_ragged_backprop_weights: null tier",
    "tfra_table_find_combine_backprop_weights_typed": "find_combine_backprop_weights_typed (out = grad_out): null table",
    "tfra_table_find_combine_ragged_backprop_weights_typed": "find_combine_ragged_backprop_weights_typed (out = grad_out): null table",
    "tfra_tier_find_combine_backprop_weights_typed": "tfra_tier_find_combine_backprop_weights_typed: null tier",
    "tfra_tier_find_combine_ragged_backprop_weights_typed": "tfra_tier_find_combine_ragged_backprop_weights_typed: null tier",
}
# a typed call with a float32 record (and no scale) is the untyped call: its code, its words
FORWARDED = {
    "tfra_table_find_combine_typed": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_typed": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_backprop_weights_typed": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_ragged_backprop_weights_typed": "tfra_table_find_combine_ragged_backprop_weights",
    "tfra_tier_find_combine_backprop_weights_typed": "tfra_tier_find_combine_backprop_weights",
    "tfra_tier_find_combine_ragged_backprop_weights_typed": "tfra_tier_find_combine_ragged_backprop_weights",
}
# the prefix of a record's refusal
RECORD_PREFIX = {
    "tfra_table_find_combine_typed": "find_combine_typed: ",
    "tfra_table_find_combine_ragged_typed": "find_combine_ragged_typed: ",
    "tfra_table_find_combine_backprop_weights_typed": "find_combine_backprop_weights_typed: ",
    "tfra_table_find_combine_ragged_backprop_weights_typed": "find_combine_ragged_backprop_weights_typed: ",
    "tfra_tier_find_combine_backprop_weights_typed": "tfra_tier_find_combine_backprop_weights_typed: ",
    "tfra_tier_find_combine_ragged_backprop_weights_typed": "tfra_tier_find_combine_ragged_backprop_weights_typed: ",
}
OUT_TYPED = sorted(n for n in RECORD_PREFIX if "backprop" not in n)
GRADS_TYPED = sorted(n for n in RECORD_PREFIX if "backprop" in n)
ADDR = 0x10000   # an address for a record's matrix: 16-byte aligned, never read on the host


@pytest.fixture(scope="module")
def capi():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _call(capi, name, record=None):
  """The call with a NULL owner and NULL / 0 operands; `record` stands where the typed call takes its tfra_rows_out / tfra_grads."""
  args = []
  for t in capi._SIGS[name]:
    if t in (ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64):
      args.append(0)
    elif t in (ctypes.POINTER(capi.RowsOut), ctypes.POINTER(capi.Grads)):
      args.append(None if record is None else ctypes.byref(record))
    else:
      args.append(None)
  rc = getattr(capi.lib(), name)(*args)
  return rc, capi.lib().tfra_last_error().decode()


def _half_record(capi, name):
  if name in OUT_TYPED:
    return capi.RowsOut(ADDR, F16, 0)
  return capi.Grads(ADDR, F16, 0, None) if name in GRADS_TYPED else None


def test_the_tables_cover_the_family(capi):
  single = [n for n in capi._SIGS if "find_combine" in n and "multi" not in n]
  assert sorted(single) == sorted(NULL_OWNER) and len(NULL_OWNER) == 18
  assert sorted(n for n in single if n.endswith("_typed")) == sorted(RECORD_PREFIX) == sorted(FORWARDED)
  assert capi.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", sorted(NULL_OWNER))
def test_a_null_owner_is_refused_in_the_calls_own_words(capi, name):
  assert _call(capi, name, _half_record(capi, name)) == (INVALID, NULL_OWNER[name])


@pytest.mark.parametrize("name", sorted(FORWARDED))
def test_a_float32_record_forwards_to_the_untyped_call(capi, name):
  rec = capi.RowsOut(ADDR, F32, 0) if name in OUT_TYPED else capi.Grads(ADDR, F32, 0, None)
  assert _call(capi, name, rec) == (INVALID, NULL_OWNER[FORWARDED[name]])


@pytest.mark.parametrize("name", OUT_TYPED)
def test_the_output_record_is_refused_before_the_owner(capi, name):
  R, pre = capi.RowsOut, RECORD_PREFIX[name]
  assert _call(capi, name, None) == (INVALID, pre + "null out record")
  assert _call(capi, name, R(ADDR, F16, 1)) == (INVALID, pre + "out.reserved must be 0")
  for dtype in (-1, 3, 6):
    assert _call(capi, name, R(ADDR, dtype, 0)) == (INVALID, pre + "out.dtype must be TFRA_F32, TFRA_F16 or TFRA_BF16")
  misaligned = pre + "misaligned out.rows (float32: 16 bytes, halves: 8 bytes)"
  assert _call(capi, name, R(ADDR + 8, F32, 0)) == (UNSUPPORTED, misaligned)
  assert _call(capi, name, R(ADDR + 4, F16, 0)) == (UNSUPPORTED, misaligned)
  assert _call(capi, name, R(ADDR + 4, BF16, 0)) == (UNSUPPORTED, misaligned)
  # 8 bytes are enough for a half matrix, and NULL rows are the twin's to refuse: the owner is looked at next
  assert _call(capi, name, R(ADDR + 8, BF16, 0)) == (INVALID, NULL_OWNER[name])
  assert _call(capi, name, R(None, F16, 0)) == (INVALID, NULL_OWNER[name])


@pytest.mark.parametrize("name", GRADS_TYPED)
def test_the_gradient_record_is_refused_before_the_owner(capi, name):
  G, pre = capi.Grads, RECORD_PREFIX[name]
  assert _call(capi, name, None) == (INVALID, pre + "null gradients")
  assert _call(capi, name, G(None, F16, 0, None)) == (INVALID, pre + "null gradients")
  assert _call(capi, name, G(ADDR, F16, 1, None)) == (INVALID, pre + "tfra_grads.reserved must be 0")
  for dtype in (-1, 3, 6):
    assert _call(capi, name, G(ADDR, dtype, 0, None)) == (INVALID, pre + "tfra_grads.dtype must be float32, float16 or bfloat16")
  assert _call(capi, name, G(ADDR, F32, 0, ADDR)) == (UNSUPPORTED, pre + "float32 gradients take no scale (loss scaling belongs to float16)")
  for dtype in (F16, BF16):
    assert _call(capi, name, G(ADDR + 4, dtype, 0, None)) == (UNSUPPORTED, pre + "half gradients must be 8-B aligned")
  # a half matrix with a scale at an address = 8 mod 16 passes: the owner is looked at next
  assert _call(capi, name, G(ADDR + 8, F16, 0, ADDR)) == (INVALID, NULL_OWNER[name])
