"""CPU-only: tfra_multi_safe_entries, its descriptor and its flags are declared in the header — the struct's fields in order, the
call's argument list, behind tfra_multi_unique —, exported by the library that build() makes and bound in the ctypes layer with
the header's arity, types and struct layout; the ABI version is unchanged (additive); descs == NULL with n_lists = 1 is refused by
name without a device and n_lists == 0 is TFRA_OK; the Python surface is there: device_ops.safe_entries_many, and
`_safe_sparse_args` keeps its parameter list beside `_safe_sparse_args_torch` and `_safe_sparse_args_many`."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, U32, I64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int64
NAME = "tfra_multi_safe_entries"
ARGS = ["tfra_workspace_t* ws", "size_t n_lists", "const tfra_safe_entries_desc* descs", "uint32_t* launches_out", "tfra_stream_t stream"]
FIELDS = [("uint32_t", "struct_size", U32), ("uint32_t", "flags", U32), ("size_t", "n_rows", SZ), ("size_t", "nnz", SZ),
          ("const int64_t*", "rows", P), ("const int64_t*", "ids", P), ("const float*", "weights", P), ("int64_t", "fill_id", I64),
          ("int64_t*", "kept_ids", P), ("int64_t*", "kept_rows", P), ("float*", "kept_weights", P), ("int64_t*", "entry_ids", P),
          ("int64_t*", "entry_rows", P), ("float*", "entry_weights", P), ("int64_t*", "d_counts", P)]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def test_header_declares_the_struct_the_flags_and_the_call():
  hdr = _header()
  m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_safe_entries_desc\s*;", hdr)
  assert m, "include/tfra_mi355x.h does not declare tfra_safe_entries_desc"
  fields = [re.sub(r"\s+", " ", f.strip()) for f in m.group(1).replace("\n", " ").split(";") if f.strip()]
  assert fields == ["%s %s" % (t, n) for t, n, _ in FIELDS]
  c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert c, "include/tfra_mi355x.h does not declare %s" % NAME
  assert c.start() > m.end()
  args = [re.sub(r"\s+", " ", a.strip()) for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == ARGS
  for flag, bit in (("PRUNE", 1), ("FILL", 2), ("RAGGED", 4)):
    assert re.search(r"#define\s+TFRA_SAFE_%s\s+%du\b" % (flag, bit), hdr), flag
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  behind = re.search(r"\bint\s+tfra_multi_unique\s*\(", hdr)
  assert behind and behind.start() < m.start()


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_types_and_layout(built):
  assert built._SIGS.get(NAME) == [P, SZ, P, P, P]
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int
  assert built._SIGS[NAME] == built._SIGS["tfra_multi_unique"]   # (the grouped calls' one shape)
  d = built.SafeEntriesDesc
  assert [(n, t) for n, t in d._fields_] == [(n, t) for _, n, t in FIELDS]
  assert ctypes.sizeof(d) == 112
  offsets = [getattr(d, n).offset for _, n, _ in FIELDS]
  assert offsets == [0, 4] + list(range(8, 112, 8))
  assert (built.SAFE_PRUNE, built.SAFE_FILL, built.SAFE_RAGGED) == (1, 2, 4)


def test_null_descs_are_refused_by_name_without_a_device(built):
  lib = built.lib()
  launches = ctypes.c_uint32(7)
  assert getattr(lib, NAME)(None, 1, None, ctypes.byref(launches), None) == -1          # TFRA_ERR_INVALID
  msg = lib.tfra_last_error().decode()
  assert "multi_safe_entries: null argument" in msg
  assert launches.value == 0
  launches = ctypes.c_uint32(7)
  assert getattr(lib, NAME)(None, 0, None, ctypes.byref(launches), None) == 0            # n_lists == 0: TFRA_OK, nothing looked at
  assert launches.value == 0
  assert getattr(lib, NAME)(None, 0, None, None, None) == 0


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import device_ops, ragged_embedding_ops, variable
  sig = inspect.signature(device_ops.safe_entries_many)
  assert list(sig.parameters) == ["requests", "want_kept", "want_entries", "return_launches"]
  assert sig.parameters["want_kept"].default is True and sig.parameters["want_entries"].default is True
  assert sig.parameters["return_launches"].default is False
  assert device_ops.safe_entries_many([]) == [] and device_ops.safe_entries_many([], return_launches=True) == ([], 0)
  assert device_ops.SAFE_ENTRIES_MAX_LIST == 1 << 31 and device_ops.SAFE_ENTRIES_MAX_TOTAL == 1 << 24
  assert device_ops.safe_entries_fit([(1 << 23, 1 << 23)]) and not device_ops.safe_entries_fit([(1 << 23, 1 << 23), (1, 0)])
  assert not device_ops.safe_entries_fit([(1 << 31, 0)])
  names = ["params", "sp_ids", "sparse_weights", "combiner", "default_id", "return_trainable", "num_rows"]
  assert list(inspect.signature(variable._safe_sparse_args).parameters) == names                               # (kept)
  assert list(inspect.signature(variable._safe_sparse_args_torch).parameters) == names
  assert list(inspect.signature(variable._safe_sparse_args_many).parameters) == [
      "params_list", "sp_ids_list", "weights", "combiners", "default_ids", "return_trainable", "num", "ragged"]
  assert ragged_embedding_ops._safe_sparse_args is variable._safe_sparse_args
