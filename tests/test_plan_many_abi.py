"""CPU-only: the grouped plan build's C entry (tfra_multi_sparse_plan_build) and its descriptor are declared in the header, exported
by the library that build() makes and bound in the ctypes layer with the header's argument list and field order; the ABI version is
unchanged (additive); the Python surface is there."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_multi_sparse_plan_build"
FIELDS = ["struct_size", "plan", "n", "ids", "dim"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def _names(decls, sep):
  return [re.split(r"[\s\*]+", a.strip())[-1] for a in decls.replace("\n", " ").split(sep) if a.strip()]


def test_header_declares_the_call_and_its_descriptor():
  hdr = _header()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % NAME
  assert _names(m.group(1), ",") == ["ws", "n_plans", "descs", "launches_out", "stream"]
  s = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_plan_build_desc\s*;", hdr)
  assert s, "include/tfra_mi355x.h does not declare tfra_plan_build_desc"
  assert _names(s.group(1), ";") == FIELDS
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


def test_library_exports_it_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  assert hasattr(lib, NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_signature_and_layout(built):
  P, SZ = ctypes.c_void_p, ctypes.c_size_t
  assert built._SIGS.get(NAME) == [P, SZ, P, P, P]
  assert getattr(built.lib(), NAME).restype is ctypes.c_int
  d = built.PlanBuildDesc
  assert [f[0] for f in d._fields_] == FIELDS
  assert [f[1] for f in d._fields_] == [ctypes.c_uint32, P, SZ, P, ctypes.c_int]
  # the C struct's layout on LP64: a 4-byte field padded to 8, three 8-byte ones, an int padded to the struct's alignment
  assert ctypes.sizeof(d) == 40 and d.plan.offset == 8 and d.n.offset == 16 and d.ids.offset == 24 and d.dim.offset == 32


def test_python_surface_is_present():
  import inspect
  from tfra_amd.dynamic_embedding import table_ops, variable
  assert callable(getattr(table_ops, "build_plans_many", None))
  assert "return_launches" in inspect.signature(table_ops.build_plans_many).parameters
  assert "entry_plan" in inspect.signature(variable.SparseTrainableWrapper.__init__).parameters
