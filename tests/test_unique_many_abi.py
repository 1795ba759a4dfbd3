"""CPU-only: tfra_multi_unique and its descriptor are declared in the header — the struct's fields in order, the call's argument
list, behind tfra_unique_unordered —, exported by the library that build() makes and bound in the ctypes layer with the header's
arity, types and struct layout; the ABI version is unchanged (additive); descs == NULL with n_lists = 1 is refused by name without
a device and n_lists == 0 is TFRA_OK; the Python surface is there: device_ops.unique_many, and `unique` / `unique_no_sync` keep
their parameter lists."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
NAME = "tfra_multi_unique"
ARGS = ["tfra_workspace_t* ws", "size_t n_lists", "const tfra_unique_desc* descs", "uint32_t* launches_out", "tfra_stream_t stream"]
FIELDS = [("uint32_t", "struct_size", U32), ("uint32_t", "flags", U32), ("size_t", "n", SZ), ("const int64_t*", "ids", P),
          ("int64_t*", "unique_out", P), ("int32_t*", "idx_out", P), ("int64_t*", "d_num_unique", P)]


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
  m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_unique_desc\s*;", hdr)
  assert m, "include/tfra_mi355x.h does not declare tfra_unique_desc"
  fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).replace("\n", " ").split(";") if f.strip()]
  assert fields == ["%s %s" % (t, n) for t, n, _ in FIELDS]
  c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert c, "include/tfra_mi355x.h does not declare %s" % NAME
  assert c.start() > m.end()
  args = [re.sub(r"\s+", " ", a.strip()) for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == ARGS
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  behind = re.search(r"\bint\s+tfra_unique_unordered\s*\(", hdr)
  assert behind and behind.start() < m.start() and 0 <= hdr.find("tfra_workspace_t;") < m.start()


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_types_and_layout(built):
  assert built._SIGS.get(NAME) == [P, SZ, P, P, P]
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int
  assert built._SIGS[NAME] == built._SIGS["tfra_multi_find_or_insert"]   # (the grouped calls' one shape)
  d = built.UniqueDesc
  assert [(n, t) for n, t in d._fields_] == [(n, t) for _, n, t in FIELDS]
  assert ctypes.sizeof(d) == 48 and d.flags.offset == 4 and d.n.offset == 8 and d.ids.offset == 16
  assert d.unique_out.offset == 24 and d.idx_out.offset == 32 and d.d_num_unique.offset == 40


def test_null_descs_are_refused_by_name_without_a_device(built):
  lib = built.lib()
  launches = ctypes.c_uint32(7)
  assert getattr(lib, NAME)(None, 1, None, ctypes.byref(launches), None) == -1          # TFRA_ERR_INVALID
  msg = lib.tfra_last_error().decode()
  assert "multi_unique: null argument" in msg
  assert launches.value == 0
  launches = ctypes.c_uint32(7)
  assert getattr(lib, NAME)(None, 0, None, ctypes.byref(launches), None) == 0            # n_lists == 0: TFRA_OK, nothing looked at
  assert launches.value == 0
  assert getattr(lib, NAME)(None, 0, None, None, None) == 0


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import device_ops
  sig = inspect.signature(device_ops.unique_many)
  assert list(sig.parameters) == ["ids_list", "want_idx", "return_launches"]
  assert sig.parameters["want_idx"].default is True and sig.parameters["return_launches"].default is False
  assert device_ops.unique_many([]) == [] and device_ops.unique_many([], return_launches=True) == ([], 0)
  assert device_ops.unique_many([], want_idx=False) == []
  assert list(inspect.signature(device_ops.unique).parameters) == ["ids", "ordered"]                         # (untouched)
  assert list(inspect.signature(device_ops.unique_no_sync).parameters) == ["ids"]
  assert device_ops.UNIQUE_MANY_MAX_LIST == 1 << 20 and device_ops.UNIQUE_MANY_MAX_TOTAL == 1 << 22
