"""CPU-only: tfra_multi_find_or_insert and its descriptor are declared in the header — the struct's fields in order, the call's
argument list —, exported by the library that build() makes and bound in the ctypes layer with the header's arity, types and
struct layout; the ABI version is unchanged (additive); descs == NULL with n_tables = 1 is refused by name without a device and
n_tables == 0 is TFRA_OK; the Python surface is there: table_ops.find_or_insert_many / table_admit_many, `admit` on _DeviceTable
and the table classes, and _DeviceTable.find_or_insert keeps its parameter list."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, U32, I32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int32
NAME = "tfra_multi_find_or_insert"
ARGS = ["tfra_workspace_t* ws", "size_t n_tables", "const tfra_find_or_insert_desc* descs", "uint32_t* launches_out",
        "tfra_stream_t stream"]
FIELDS = [("uint32_t", "struct_size", U32), ("uint32_t", "flags", U32), ("tfra_table_t*", "table", P), ("size_t", "n", SZ),
          ("const int64_t*", "d_n", P), ("const int64_t*", "keys", P), ("const void*", "init_values", P), ("int32_t", "init_is_full", I32),
          ("uint32_t", "reserved", U32), ("const uint64_t*", "scores", P), ("void*", "values_out", P), ("uint8_t*", "found", P)]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def test_header_declares_the_struct_and_the_call():
  hdr = _header()
  m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_find_or_insert_desc\s*;", hdr)
  assert m, "include/tfra_mi355x.h does not declare tfra_find_or_insert_desc"
  fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).replace("\n", " ").split(";") if f.strip()]
  assert fields == ["%s %s" % (t, n) for t, n, _ in FIELDS]
  c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert c, "include/tfra_mi355x.h does not declare %s" % NAME
  assert c.start() > m.end()
  args = [re.sub(r"\s+", " ", a.strip()) for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == ARGS
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  assert 0 <= hdr.find("tfra_table_t;") < m.start() and 0 <= hdr.find("tfra_workspace_t;") < m.start()


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_types_and_layout(built):
  assert built._SIGS.get(NAME) == [P, SZ, P, P, P]
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int
  assert built._SIGS[NAME] == built._SIGS["tfra_multi_tier_find_or_insert"]   # (the grouped calls' one shape)
  d = built.FindOrInsertDesc
  assert [(n, t) for n, t in d._fields_] == [(n, t) for _, n, t in FIELDS]
  assert ctypes.sizeof(d) == 80 and d.table.offset == 8 and d.init_is_full.offset == 48 and d.reserved.offset == 52
  assert d.scores.offset == 56 and d.values_out.offset == 64 and d.found.offset == 72


def test_null_descs_are_refused_by_name_without_a_device(built):
  lib = built.lib()
  launches = ctypes.c_uint32(7)
  assert getattr(lib, NAME)(None, 1, None, ctypes.byref(launches), None) == -1          # TFRA_ERR_INVALID
  msg = lib.tfra_last_error().decode()
  assert "multi_find_or_insert" in msg and "null argument" in msg
  assert launches.value == 0
  launches = ctypes.c_uint32(7)
  assert getattr(lib, NAME)(None, 0, None, ctypes.byref(launches), None) == 0            # n_tables == 0: TFRA_OK, nothing looked at
  assert launches.value == 0
  assert getattr(lib, NAME)(None, 0, None, None, None) == 0


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)
  assert par(table_ops.find_or_insert_many) == ["requests", "return_launches"]
  assert inspect.signature(table_ops.find_or_insert_many).parameters["return_launches"].default is False
  assert par(table_ops.table_admit_many) == ["requests"]
  table = table_ops._DeviceTable
  assert par(table.find_or_insert)[1:] == ["keys", "init_values", "scores", "return_exists", "count", "out"]   # (untouched)
  assert par(table.admit)[1:] == ["keys", "init_values", "scores", "count"]
  for cls in (table_ops.HkvHashTable, table_ops.CuckooHashTable):
    assert par(cls.admit)[1:] == ["keys", "dynamic_default_values", "count"]
  assert par(table_ops.TieredHashTable.admit)[1:] == ["keys", "init_values", "count", "verify"]                # (untouched)
  assert par(variable._admit_entries_many) == ["params_list", "entry_ids"]
  assert variable.ADMIT_MANY_MIN_TABLES >= 1 and variable.ADMIT_MANY_MIN_TIERS == 3
  assert table_ops.find_or_insert_many([]) == [] and table_ops.find_or_insert_many([], return_launches=True) == ([], 0)
  assert table_ops.table_admit_many([]) is None
