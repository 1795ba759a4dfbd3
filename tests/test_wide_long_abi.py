"""CPU-only: the four block-per-row wide calls (tfra_table_find_combine_wide_long, its ragged form and their
*_backprop_weights_wide_long forms) are exported by the library that build() makes and bound in the ctypes layer with their twins'
arity and types; the ABI version is unchanged (additive); without a device a call refuses what its twin refuses, in the twin's
words behind its own name; the Python surface is there with the wide methods' parameter lists, and `wide_rows` still defaults to
False."""
import ctypes
import inspect

import pytest

TWINS = {
    "tfra_table_find_combine_wide_long": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_wide_long": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_backprop_weights_wide_long": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_ragged_backprop_weights_wide_long": "tfra_table_find_combine_ragged_backprop_weights",
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
  assert msg_t.startswith(stem) and msg == msg_t.replace(stem, stem + "_wide_long", 1)


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import ragged_embedding_ops, table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  stems = ["find_combine", "find_combine_ragged", "find_combine_weight_grad", "find_combine_ragged_weight_grad"]
  for cls in (table_ops._DeviceTable, table_ops.HkvHashTable, table_ops.CuckooHashTable):
    for stem in stems:
      assert par(getattr(cls, stem + "_wide_long")) == par(getattr(table_ops._DeviceTable, stem + "_wide"))
  var = variable.Variable
  for stem in ("lookup_combined", "lookup_combined_ragged", "lookup_combined_weight_grad", "lookup_combined_ragged_weight_grad"):
    assert par(getattr(var, stem + "_wide_long")) == par(getattr(var, stem + "_wide"))
  for f in (variable.embedding_lookup_sparse, variable.safe_embedding_lookup_sparse,
            ragged_embedding_ops.embedding_lookup_sparse, ragged_embedding_ops.safe_embedding_lookup_sparse):
    assert inspect.signature(f).parameters["wide_rows"].default is False
