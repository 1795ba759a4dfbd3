"""CPU-only: tfra_tier_find_or_insert_planned is declared in the header, exported by the library that build() makes and bound in
the ctypes layer with the header's argument list; the ABI version is unchanged (additive); the refusal of a NULL tier needs no
device; the Python surface is there: the tier's planned admitting lookup and its admit-only form, on _DeviceTier and on
TieredHashTable."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_tier_find_or_insert_planned"
ARGS = ["tfra_tier_t* tier", "const tfra_sparse_plan_t* plan", "const void* init_values", "int init_is_full", "void* rows_out",
        "uint8_t* where", "uint32_t flags", "tfra_stream_t stream"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def test_header_declares_the_call():
  hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % NAME
  args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == ARGS
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_and_types(built):
  P = ctypes.c_void_p
  assert built._SIGS.get(NAME) == [P, P, P, ctypes.c_int, P, P, ctypes.c_uint32, P]
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int


def test_a_null_tier_is_refused_by_name(built):
  lib = built.lib()
  assert getattr(lib, NAME)(None, None, None, 0, None, None, 0, None) == -1
  assert NAME in lib.tfra_last_error().decode()


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops
  params = lambda f: list(inspect.signature(f).parameters)[1:]
  assert params(table_ops._DeviceTier.find_or_insert_planned) == ["plan", "init_values", "return_where", "out", "verify"]
  assert params(table_ops._DeviceTier.admit_planned) == ["plan", "init_values", "verify"]
  assert params(table_ops.TieredHashTable.admit_planned) == ["plan", "init_values", "verify"]
  for f in (table_ops._DeviceTier.find_or_insert_planned, table_ops._DeviceTier.admit_planned, table_ops.TieredHashTable.admit_planned):
    sig = inspect.signature(f).parameters
    assert sig["init_values"].default is None and sig["verify"].default is False
  want = params(table_ops.HkvHashTable.find_or_insert_planned)
  assert want == params(table_ops.CuckooHashTable.find_or_insert_planned) == ["plan", "dynamic_default_values", "return_exists", "name"]
  assert params(table_ops.TieredHashTable.find_or_insert_planned) == want
  src = inspect.getsource(table_ops.TieredHashTable.find_or_insert_planned)
  assert "NotImplementedError" not in src
