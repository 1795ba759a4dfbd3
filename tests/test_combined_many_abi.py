"""CPU-only: the grouped combined write-back's C entry (tfra_multi_apply_planned_combined) and its descriptor are declared in the
header, exported by the library that build() makes and bound in the ctypes layer with the header's argument list and field order;
the ABI version is unchanged (additive); the Python surface is there."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_multi_apply_planned_combined"
FIELDS = ["struct_size", "combiner", "table", "opt", "plan", "grad_out", "seg", "weights", "n_rows", "param_default_row"]


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
  assert _names(m.group(1), ",") == ["ws", "n_tables", "descs", "launches_out", "stream"]
  s = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_apply_combined_desc\s*;", hdr)
  assert s, "include/tfra_mi355x.h does not declare tfra_apply_combined_desc"
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
  d = built.ApplyCombinedDesc
  assert [f[0] for f in d._fields_] == FIELDS
  assert [f[1] for f in d._fields_] == [ctypes.c_uint32, ctypes.c_int32, P, P, P, P, P, P, SZ, P]
  # the C struct's layout on LP64: two 4-byte fields, then eight 8-byte ones
  assert ctypes.sizeof(d) == 72 and d.table.offset == 8 and d.n_rows.offset == 56 and d.param_default_row.offset == 64


def test_python_surface_is_present():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops
  assert callable(getattr(table_ops, "apply_planned_combined_many", None))
  assert callable(getattr(de.DynamicEmbeddingOptimizer, "apply_combined_gradients_many", None))
