"""CPU-only: the four long-row calls (tfra_table_find_combine_long, its ragged form and their *_backprop_weights_long forms) are
declared in the header with their twins' argument lists, exported by the library that build() makes and bound in the ctypes layer
with the twins' arity and types; the ABI version is unchanged (additive); without a device a call refuses what its twin refuses,
in the twin's words behind its own name; the Python surface is there, down to the public functions' keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {
    "tfra_table_find_combine_long": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_long": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_backprop_weights_long": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_ragged_backprop_weights_long": "tfra_table_find_combine_ragged_backprop_weights",
}
NAMES = sorted(TWINS)


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _declared(name):
  hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % name
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_call_with_its_twins_arguments(name):
  assert _declared(name) == _declared(TWINS[name])


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_binding_is_the_twins(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1
  assert built._SIGS.get(name) == built._SIGS[TWINS[name]]
  assert len(built._SIGS[name]) == len(_declared(name))
  assert getattr(built.lib(), name).restype is ctypes.c_int


def _null_table(capi, name):
  args = [0 if t in (ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64) else None for t in capi._SIGS[name]]
  args[1] = 1
  rc = getattr(capi.lib(), name)(*args)
  return rc, capi.lib().tfra_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_a_null_table_is_refused_in_the_twins_words(built, name):
  rc, msg = _null_table(built, name)
  rc_t, msg_t = _null_table(built, TWINS[name])
  assert rc == rc_t == -1
  stem = TWINS[name][len("tfra_table_"):]
  assert msg_t.startswith(stem) and msg == msg_t.replace(stem, stem + "_long", 1)


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import ragged_embedding_ops, table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  pairs = [("find_combine_long", "find_combine"), ("find_combine_weight_grad_long", "find_combine_weight_grad"),
           ("find_combine_ragged_weight_grad_long", "find_combine_ragged_weight_grad")]
  for cls in (table_ops._DeviceTable, table_ops.HkvHashTable, table_ops.CuckooHashTable):
    for long, twin in pairs:
      assert par(getattr(cls, long)) == par(getattr(table_ops._DeviceTable, twin))
    assert par(cls.find_combine_ragged_long) == par(table_ops._DeviceTable.find_combine_ragged)[:-1]   # (no out_dtype)
  var = variable.Variable
  for f in (var.lookup_combined, var.lookup_combined_ragged, variable.embedding_lookup_sparse, variable.safe_embedding_lookup_sparse,
            ragged_embedding_ops.embedding_lookup_sparse, ragged_embedding_ops.safe_embedding_lookup_sparse):
    assert inspect.signature(f).parameters["long_rows"].default is False
  # the two weight-gradient methods keep their parameter lists; their long forms stand beside them with the same lists
  assert par(var.lookup_combined_weight_grad_long) == par(var.lookup_combined_weight_grad)
  assert par(var.lookup_combined_ragged_weight_grad_long) == par(var.lookup_combined_ragged_weight_grad)
