"""CPU-only: the four mixed-row calls (tfra_table_find_combine_mixed, its ragged form and their *_backprop_weights_mixed forms) are
declared in the header with their twins' argument lists plus `uint32_t long_from` directly before the stream, exported by the
library that build() makes and bound in the ctypes layer (`_capi._SIGS_MIXED`) with that arity; the ABI version is unchanged
(additive); without a device a call refuses what its twin refuses, in the twin's words behind its own name; the Python surface is
there, down to the public functions' keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {
    "tfra_table_find_combine_mixed": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_mixed": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_backprop_weights_mixed": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_ragged_backprop_weights_mixed": "tfra_table_find_combine_ragged_backprop_weights",
}
NAMES = sorted(TWINS)


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def _declared(name):
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, _header())
  assert m, "include/tfra_mi355x.h does not declare %s" % name
  return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_call_with_its_twins_arguments_and_long_from(name):
  twin = _declared(TWINS[name])
  assert _declared(name) == twin[:-1] + ["uint32_t long_from"] + twin[-1:]
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", _header())
  assert re.search(r"#define\s+TFRA_MIXED_LONG_FROM_DEFAULT\s+\d+\b", _header())


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_binding_has_the_declared_arity(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1
  twin = built._SIGS[TWINS[name]]
  assert built._SIGS_MIXED.get(name) == twin[:-1] + [ctypes.c_uint32] + twin[-1:]
  assert len(built._SIGS_MIXED[name]) == len(_declared(name))
  assert getattr(built.lib(), name).restype is ctypes.c_int


def _null_table(capi, name):
  args = [0 if t in (ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64) else None for t in {**capi._SIGS, **capi._SIGS_MIXED}[name]]
  args[1] = 1
  rc = getattr(capi.lib(), name)(*args)
  return rc, capi.lib().tfra_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_a_null_table_is_refused_in_the_twins_words(built, name):
  rc, msg = _null_table(built, name)
  rc_t, msg_t = _null_table(built, TWINS[name])
  assert rc == rc_t == -1
  stem = TWINS[name][len("tfra_table_"):]
  assert msg_t.startswith(stem) and msg == msg_t.replace(stem, stem + "_mixed", 1)


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import ragged_embedding_ops, table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  pairs = [("find_combine_mixed", "find_combine"), ("find_combine_weight_grad_mixed", "find_combine_weight_grad"),
           ("find_combine_ragged_weight_grad_mixed", "find_combine_ragged_weight_grad"),
           ("find_combine_ragged_mixed", "find_combine_ragged_long")]   # (the ragged twin without its out_dtype)
  for cls in (table_ops._DeviceTable, table_ops.HkvHashTable, table_ops.CuckooHashTable):
    for mixed, twin in pairs:
      assert par(getattr(cls, mixed)) == par(getattr(table_ops._DeviceTable, twin)) + ["long_from"]
      assert inspect.signature(getattr(cls, mixed)).parameters["long_from"].default == 0
  var = variable.Variable
  for f in (var.lookup_combined, var.lookup_combined_ragged, variable.embedding_lookup_sparse, variable.safe_embedding_lookup_sparse,
            ragged_embedding_ops.embedding_lookup_sparse, ragged_embedding_ops.safe_embedding_lookup_sparse):
    assert inspect.signature(f).parameters["mixed_rows"].default is False
    assert par(f)[-1] == "mixed_rows"   # (behind every parameter the function had)
  assert par(var.lookup_combined_weight_grad_mixed) == par(var.lookup_combined_weight_grad)
  assert par(var.lookup_combined_ragged_weight_grad_mixed) == par(var.lookup_combined_ragged_weight_grad)
