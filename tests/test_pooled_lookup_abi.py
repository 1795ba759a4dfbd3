"""CPU-only: the pooled lookup's C entry (tfra_table_find_combine) is declared in the header, exported by the library that
build() makes and bound in the ctypes layer with the header's argument list; the ABI version is unchanged (additive)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_table_find_combine"


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def test_header_declares_find_combine():
  hdr = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % NAME
  args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
  names = [re.split(r"[\s\*]+", a)[-1] for a in args]
  assert names == ["t", "ws", "nnz", "ids", "seg", "weights", "combiner", "n_rows", "default_row", "out", "stream"]


def test_library_exports_find_combine(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  assert hasattr(lib, NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_signature(built):
  P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
  assert built._SIGS.get(NAME) == [P, P, SZ, P, P, P, I, SZ, P, P, P]
  assert getattr(built.lib(), NAME).restype is ctypes.c_int


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  assert callable(getattr(table_ops._DeviceTable, "find_combine", None))
  assert callable(getattr(variable.Variable, "lookup_combined", None))
