"""CPU-only: the four grouped pooled calls with long members (tfra_multi_find_combine_long, its ragged form and their
*_backprop_weights_long forms) are declared in the header with their twins' argument lists plus `const uint8_t* long_rows` in front
of the stream, exported by the library that build() makes and bound in a table of their own beside _SIGS; the ABI version is
unchanged (additive); the Python surface carries the keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {
    "tfra_multi_find_combine_long": "tfra_multi_find_combine",
    "tfra_multi_find_combine_ragged_long": "tfra_multi_find_combine_ragged",
    "tfra_multi_find_combine_backprop_weights_long": "tfra_multi_find_combine_backprop_weights",
    "tfra_multi_find_combine_ragged_backprop_weights_long": "tfra_multi_find_combine_ragged_backprop_weights",
}


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


@pytest.mark.parametrize("name", sorted(TWINS))
def test_header_library_and_binding(built, name):
  twin = _declared(TWINS[name])
  assert _declared(name) == twin[:-1] + ["const uint8_t* long_rows", twin[-1]]
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name) and built.lib().tfra_abi_version() == 1
  assert name not in built._SIGS and built._SIGS_LONG_MANY[name] == built._SIGS[TWINS[name]][:-1] + [ctypes.c_void_p] * 2
  assert getattr(built.lib(), name).argtypes == built._SIGS_LONG_MANY[name] and getattr(built.lib(), name).restype is ctypes.c_int
  # n_tables == 0 is TFRA_OK without a device, as in the twin; a list without descriptors is the twin's "null argument"
  assert getattr(built.lib(), name)(None, 0, None, None, None, None) == 0
  assert getattr(built.lib(), name)(None, 1, None, None, None, None) == getattr(built.lib(), TWINS[name])(None, 1, None, None, None) == -1


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import ragged_embedding_ops, table_ops, variable
  # (the two *_weight_grad_many keep their pinned parameter lists: the gradient's keyword stands on their *_long siblings)
  for f in (table_ops.find_combine_many, table_ops.find_combine_ragged_many, table_ops.find_combine_weight_grad_many_long,
            table_ops.find_combine_ragged_weight_grad_many_long):
    assert inspect.signature(f).parameters["long_rows"].default is None
  for f in (variable.embedding_lookup_sparse_many, variable.safe_embedding_lookup_sparse_many,
            ragged_embedding_ops.embedding_lookup_sparse_many, ragged_embedding_ops.safe_embedding_lookup_sparse_many):
    assert inspect.signature(f).parameters["long_rows"].default is False
