"""CPU-only: tfra_table_insert_and_evict_n and the six tfra_tier_* calls are declared in the header with their argument lists,
exported by the library that build() makes and bound in the ctypes layer with the header's arity and types; the ABI version is
unchanged (additive); a NULL table or tier is refused by name without a device; the Python surface is there, down to
TieredHashTableCreator."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, I, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
CALLS = {
    "tfra_table_insert_and_evict_n": (
        ["tfra_table_t* t", "size_t n", "const int64_t* d_n", "const int64_t* keys", "const void* values", "const uint64_t* scores",
         "uint32_t flags", "size_t* d_evicted_counter", "size_t cap", "int64_t* evicted_keys", "void* evicted_values",
         "uint64_t* evicted_scores", "tfra_stream_t stream"],
        [P, SZ, P, P, P, P, U32, P, SZ, P, P, P, P]),
    "tfra_tier_create": (
        ["tfra_table_t* upper", "tfra_table_t* lower", "size_t max_batch", "tfra_tier_t** out"],
        [P, P, SZ, ctypes.POINTER(P)]),
    "tfra_tier_destroy": (["tfra_tier_t* tier"], [P]),
    "tfra_tier_find": (
        ["tfra_tier_t* tier", "size_t n", "const int64_t* d_n", "const int64_t* keys", "void* values", "uint8_t* where",
         "const void* defaults", "int default_is_full", "tfra_stream_t stream"],
        [P, SZ, P, P, P, P, P, I, P]),
    "tfra_tier_find_or_insert": (
        ["tfra_tier_t* tier", "size_t n", "const int64_t* d_n", "const int64_t* keys", "const void* init_values", "int init_is_full",
         "void* values_out", "uint8_t* where", "uint32_t flags", "tfra_stream_t stream"],
        [P, SZ, P, P, P, I, P, P, U32, P]),
    "tfra_tier_insert": (
        ["tfra_tier_t* tier", "size_t n", "const int64_t* d_n", "const int64_t* keys", "const void* values", "tfra_stream_t stream"],
        [P, SZ, P, P, P, P]),
    "tfra_tier_stats": (["tfra_tier_t* tier", "uint64_t* out8", "tfra_stream_t stream"], [P, ctypes.POINTER(ctypes.c_uint64), P]),
}
NAMES = sorted(CALLS)
REFUSING = [n for n in NAMES if n != "tfra_tier_destroy"]     # (destroying nothing is not an error)


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


def test_header_defines_the_flags():
  hdr = _header()
  assert re.search(r"#define\s+TFRA_INSERT_WHOLE_ROWS\s+2u\b", hdr) and re.search(r"#define\s+TFRA_EVICT_WHOLE_ROWS\s+1u\b", hdr)
  assert re.search(r"#define\s+TFRA_TIER_VERIFY\s+1u\b", hdr)
  assert re.search(r"typedef\s+struct\s+tfra_tier\s+tfra_tier_t\s*;", hdr)


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_abi_version_stays(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", NAMES)
def test_binding_has_the_headers_arity_and_types(built, name):
  assert built._SIGS.get(name) == CALLS[name][1]
  assert len(built._SIGS[name]) == len(CALLS[name][0])
  assert getattr(built.lib(), name).restype is ctypes.c_int
  assert (built.INSERT_WHOLE_ROWS, built.EVICT_WHOLE_ROWS, built.TIER_VERIFY) == (2, 1, 1)


@pytest.mark.parametrize("name", REFUSING)
def test_a_null_handle_is_refused_by_name(built, name):
  lib = built.lib()
  args = [0 if t in (SZ, I, U32) else None for t in CALLS[name][1]]
  if SZ in CALLS[name][1]:
    args[CALLS[name][1].index(SZ)] = 1
  assert getattr(lib, name)(*args) == -1
  assert name in lib.tfra_last_error().decode()


def test_destroying_no_tier_is_ok(built):
  assert built.lib().tfra_tier_destroy(None) == 0


def test_python_surface_is_present():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  dt = table_ops._DeviceTable
  assert par(dt.upsert_and_evict) == ["keys", "values", "scores", "whole_rows", "cap", "sync", "count", "whole_rows_in"]
  sig = inspect.signature(dt.upsert_and_evict).parameters
  assert sig["count"].default is None and sig["whole_rows_in"].default is False and sig["sync"].default is True
  tier = table_ops._DeviceTier
  assert par(tier.__init__) == ["upper", "lower", "max_batch"]
  assert par(tier.find)[:1] == ["keys"] and "count" in par(tier.find)
  assert par(tier.find_or_insert) == ["keys", "init_values", "return_where", "count", "out", "verify"]
  assert par(tier.insert)[:2] == ["keys", "values"] and par(tier.stats) == []
  tab = table_ops.TieredHashTable
  assert issubclass(tab, table_ops._LookupInterfaceMirror)
  assert par(tab.find_or_insert) == ["keys", "dynamic_default_values", "return_exists", "name", "count"]
  assert par(tab.lookup) == ["keys", "dynamic_default_values", "return_exists", "name"]
  for m in ("insert", "remove", "clear", "contains", "export", "size", "flush", "_checkpoint_table"):
    assert callable(getattr(tab, m)), m
  assert callable(table_ops._LookupInterfaceMirror._checkpoint_table)
  assert par(variable.TieredHashTableConfig.__init__) == ["upper", "lower", "max_batch"]
  assert issubclass(variable.TieredHashTableCreator, variable.KVCreator)
  for n in ("TieredHashTable", "TieredHashTableConfig", "TieredHashTableCreator"):
    assert hasattr(de, n), n
  cfg = de.TieredHashTableConfig(max_batch=77)
  assert isinstance(cfg.upper, de.HkvHashTableConfig) and isinstance(cfg.lower, de.CuckooHashTableConfig) and cfg.max_batch == 77
