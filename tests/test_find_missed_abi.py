"""CPU-only: tfra_table_find_missed, tfra_table_assign and tfra_table_contains are declared in the header with their argument
lists, exported by the library that build() makes and bound in the ctypes layer with the header's arity and types; the ABI version
is unchanged (additive); a NULL table is refused by name without a device; the Python surface is there, down to Variable."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
CALLS = {
    "tfra_table_find_missed": (
        ["tfra_table_t* t", "size_t n", "const int64_t* d_n", "const int64_t* keys", "void* values", "uint8_t* exists",
         "uint64_t* scores_out", "const void* defaults", "int default_is_full", "size_t* d_missed_counter", "size_t cap",
         "int64_t* missed_keys", "int32_t* missed_indices", "tfra_stream_t stream"],
        [P, SZ, P, P, P, P, P, P, I, P, SZ, P, P, P]),
    "tfra_table_assign": (
        ["tfra_table_t* t", "size_t n", "const int64_t* d_n", "const int64_t* keys", "const void* values", "const uint64_t* scores",
         "uint8_t* found", "tfra_stream_t stream"],
        [P, SZ, P, P, P, P, P, P]),
    "tfra_table_contains": (
        ["tfra_table_t* t", "size_t n", "const int64_t* d_n", "const int64_t* keys", "uint8_t* exists", "tfra_stream_t stream"],
        [P, SZ, P, P, P, P]),
}
NAMES = sorted(CALLS)


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_call(name):
  hdr = _header()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % name
  args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == CALLS[name][0]
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_abi_version_stays(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", NAMES)
def test_binding_has_the_headers_arity_and_types(built, name):
  assert built._SIGS.get(name) == CALLS[name][1]
  assert len(built._SIGS[name]) == len(CALLS[name][0])
  assert getattr(built.lib(), name).restype is ctypes.c_int


@pytest.mark.parametrize("name", NAMES)
def test_a_null_table_is_refused_by_name(built, name):
  lib = built.lib()
  args = [0 if t in (SZ, I) else None for t in CALLS[name][1]]
  args[1] = 1
  assert getattr(lib, name)(*args) == -1
  assert name in lib.tfra_last_error().decode()


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  dt = table_ops._DeviceTable
  assert par(dt.find_missed) == ["keys", "dynamic_default_values", "return_exists", "return_scores", "count", "cap", "sync"]
  assert inspect.signature(dt.find_missed).parameters["sync"].default is True
  assert par(dt.assign) == ["keys", "values", "scores", "return_found", "count"]
  assert par(dt.contains) == ["keys", "count"]
  for cls in (table_ops.HkvHashTable, table_ops.CuckooHashTable):
    assert par(cls.lookup_missed) == ["keys", "dynamic_default_values", "name"]
    assert par(cls.contains) == ["keys", "name"]
  assert par(table_ops.CuckooHashTable.assign) == ["keys", "values", "name"]
  assert par(table_ops.HkvHashTable.assign) == ["keys", "values", "scores", "name"]
  assert par(variable.Variable.lookup_missed)[:2] == ["keys", "return_exists"]
  assert par(variable.Variable.assign)[:3] == ["keys", "values", "return_found"]
  assert par(variable.Variable.contains)[:1] == ["keys"]
