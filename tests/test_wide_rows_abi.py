"""CPU-only: the four wide-row calls (tfra_table_find_combine_wide, its ragged form and their *_backprop_weights_wide forms) are
exported by the library that build() makes and bound in the ctypes layer with their twins' arity and types; the ABI version is
unchanged (additive); without a device a call refuses what its twin refuses, in the twin's words behind its own name; the Python
surface is there, down to the public functions' keyword."""
import ctypes
import inspect

import pytest

TWINS = {
    "tfra_table_find_combine_wide": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_wide": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_backprop_weights_wide": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_ragged_backprop_weights_wide": "tfra_table_find_combine_ragged_backprop_weights",
}
NAMES = sorted(TWINS)


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_binding_is_the_twins(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1
  # (the wide calls' table stands beside _SIGS, whose single find_combine names tests/test_pooled_refusals_abi.py holds to 18)
  assert built._SIGS_WIDE.get(name) == built._SIGS[TWINS[name]] and getattr(built.lib(), name).argtypes == built._SIGS[TWINS[name]]
  assert getattr(built.lib(), name).restype is ctypes.c_int


def _null_table(capi, name):
  args = [0 if t in (ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64) else None for t in {**capi._SIGS, **capi._SIGS_WIDE}[name]]
  args[1] = 1
  rc = getattr(capi.lib(), name)(*args)
  return rc, capi.lib().tfra_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_a_null_table_is_refused_in_the_twins_words(built, name):
  rc, msg = _null_table(built, name)
  rc_t, msg_t = _null_table(built, TWINS[name])
  assert rc == rc_t == -1
  stem = TWINS[name][len("tfra_table_"):]
  assert msg_t.startswith(stem) and msg == msg_t.replace(stem, stem + "_wide", 1)


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import ragged_embedding_ops, table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  pairs = [("find_combine_wide", "find_combine"), ("find_combine_weight_grad_wide", "find_combine_weight_grad"),
           ("find_combine_ragged_weight_grad_wide", "find_combine_ragged_weight_grad")]
  for cls in (table_ops._DeviceTable, table_ops.HkvHashTable, table_ops.CuckooHashTable):
    for wide, twin in pairs:
      assert par(getattr(cls, wide)) == par(getattr(table_ops._DeviceTable, twin))
    assert par(cls.find_combine_ragged_wide) == par(table_ops._DeviceTable.find_combine_ragged)[:-1]   # (no out_dtype)
  var = variable.Variable
  for f in (variable.embedding_lookup_sparse, variable.safe_embedding_lookup_sparse,
            ragged_embedding_ops.embedding_lookup_sparse, ragged_embedding_ops.safe_embedding_lookup_sparse):
    assert inspect.signature(f).parameters["wide_rows"].default is False
  # methods of their own beside the existing ones, which keep their parameter lists (no wide_rows keyword on them)
  assert par(var.lookup_combined_wide) == par(var.lookup_combined)[:6]
  assert par(var.lookup_combined_ragged_wide) == par(var.lookup_combined_ragged)[:7]
  assert par(var.lookup_combined_weight_grad_wide) == par(var.lookup_combined_weight_grad)
  assert par(var.lookup_combined_ragged_weight_grad_wide) == par(var.lookup_combined_ragged_weight_grad)
  assert "wide_rows" not in par(var.lookup_combined) and callable(var.can_lookup_combined_wide)
