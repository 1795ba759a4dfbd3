"""CPU-only: tfra_table_insert_and_evict and TFRA_EVICT_WHOLE_ROWS are declared in the header, exported by the library that build()
makes and bound in the ctypes layer with the header's argument list; the ABI version is unchanged (additive); the argument checks
that come before anything is enqueued need no device; the Python surface is there, and CuckooHashTable does not get the method."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_table_insert_and_evict"
ARGS = ["t", "n", "keys", "values", "scores", "flags", "d_evicted_counter", "cap", "evicted_keys", "evicted_values", "evicted_scores",
        "stream"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def test_header_declares_the_call_and_the_flag():
  hdr = _header()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % NAME
  names = [re.split(r"[\s\*]+", a.strip())[-1] for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
  assert names == ARGS
  assert re.search(r"#define\s+TFRA_EVICT_WHOLE_ROWS\s+1u\b", hdr)
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_and_types(built):
  P, SZ = ctypes.c_void_p, ctypes.c_size_t
  assert built._SIGS.get(NAME) == [P, SZ, P, P, P, ctypes.c_uint32, P, SZ, P, P, P, P]
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int
  assert built.EVICT_WHOLE_ROWS == 1


def test_a_null_table_is_refused_by_name(built):
  lib = built.lib()
  assert lib.tfra_table_insert_and_evict(None, 1, None, None, None, 0, None, 0, None, None, None, None) == -1
  assert NAME in lib.tfra_last_error().decode()


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  assert callable(getattr(table_ops._DeviceTable, "upsert_and_evict", None))
  assert callable(getattr(table_ops.HkvHashTable, "insert_and_evict", None))
  assert callable(getattr(variable.Variable, "upsert_and_evict", None))
  assert not hasattr(table_ops.CuckooHashTable, "insert_and_evict")
