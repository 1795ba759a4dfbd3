"""CPU-only: the typed lookups' C entries (tfra_table_find_typed, tfra_table_find_combine_typed, tfra_table_find_combine_ragged_typed,
tfra_multi_find_combine_typed, tfra_multi_find_combine_ragged_typed), the output record tfra_rows_out and the two typed descriptors
are declared in the header, exported by the library that build() makes and bound in the ctypes layer with the header's argument
lists, field order and sizes; the ABI version is unchanged (additive); the Python surface takes out_dtype."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "tfra_table_find_typed": ["t", "n", "d_n", "keys", "out", "exists", "defaults", "default_is_full", "stream"],
    "tfra_table_find_combine_typed": ["t", "ws", "nnz", "ids", "seg", "weights", "combiner", "n_rows", "default_row", "out", "stream"],
    "tfra_table_find_combine_ragged_typed": ["t", "n_rows", "row_splits", "nnz", "ids", "weights", "combiner", "flags", "fill_id",
                                             "default_row", "out", "stream"],
    "tfra_multi_find_combine_typed": ["ws", "n_tables", "descs", "launches_out", "stream"],
    "tfra_multi_find_combine_ragged_typed": ["ws", "n_tables", "descs", "launches_out", "stream"],
}
ROWS_OUT = ["rows", "dtype", "reserved"]
TUPLE_FIELDS = ["struct_size", "combiner", "table", "nnz", "ids", "seg", "weights", "n_rows", "default_row", "out"]
RAGGED_FIELDS = ["struct_size", "combiner", "table", "n_rows", "row_splits", "nnz", "ids", "weights", "flags", "reserved", "fill_id",
                 "default_row", "out"]


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


def _struct(hdr, name):
  s = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, hdr)
  assert s, "include/tfra_mi355x.h does not declare %s" % name
  return _names(s.group(1), ";")


def test_header_declares_the_calls_the_record_and_the_descriptors():
  hdr = _header()
  for name, args in CALLS.items():
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, "include/tfra_mi355x.h does not declare %s" % name
    assert _names(m.group(1), ",") == args, name
  assert _struct(hdr, "tfra_rows_out") == ROWS_OUT
  assert _struct(hdr, "tfra_find_combine_typed_desc") == TUPLE_FIELDS
  assert _struct(hdr, "tfra_find_combine_ragged_typed_desc") == RAGGED_FIELDS
  # the typed descriptors are their twins' with the record in the place of the pointer
  assert _struct(hdr, "tfra_find_combine_desc") == TUPLE_FIELDS
  assert _struct(hdr, "tfra_find_combine_ragged_desc") == RAGGED_FIELDS


def test_library_exports_them_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  for name in CALLS:
    assert hasattr(lib, name), name
  assert built.lib().tfra_abi_version() == 1


def test_bindings_have_the_headers_signatures_and_layout(built):
  P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
  RO = ctypes.POINTER(built.RowsOut)
  assert built._SIGS.get("tfra_table_find_typed") == [P, SZ, P, P, RO, P, P, I, P]
  assert built._SIGS.get("tfra_table_find_combine_typed") == [P, P, SZ, P, P, P, I, SZ, P, RO, P]
  assert built._SIGS.get("tfra_table_find_combine_ragged_typed") == [P, SZ, P, SZ, P, P, I, ctypes.c_uint32, ctypes.c_int64, P, RO, P]
  assert built._SIGS.get("tfra_multi_find_combine_typed") == [P, SZ, P, P, P]
  assert built._SIGS.get("tfra_multi_find_combine_ragged_typed") == [P, SZ, P, P, P]
  for name in CALLS:   # the signatures load
    assert getattr(built.lib(), name).restype is ctypes.c_int
  r = built.RowsOut
  assert [f[0] for f in r._fields_] == ROWS_OUT
  assert ctypes.sizeof(r) == 16 and [getattr(r, f).offset for f in ROWS_OUT] == [0, 8, 12]
  d = built.FindCombineTypedDesc
  assert [f[0] for f in d._fields_] == TUPLE_FIELDS
  assert ctypes.sizeof(d) == 80 and d.out.offset == 64 and d.out.size == 16
  assert [f[:2] for f in d._fields_[:-1]] == [f[:2] for f in built.FindCombineDesc._fields_[:-1]]
  d = built.FindCombineRaggedTypedDesc
  assert [f[0] for f in d._fields_] == RAGGED_FIELDS
  assert ctypes.sizeof(d) == 96 and d.out.offset == 80 and d.out.size == 16
  assert [f[:2] for f in d._fields_[:-1]] == [f[:2] for f in built.FindCombineRaggedDesc._fields_[:-1]]


def test_sizes_equal_the_headers(built, tmp_path):
  """sizeof of the record and the two descriptors as a C++ compiler lays the header out, against the ctypes structures."""
  src = tmp_path / "sizes.cpp"
  src.write_text('#include <cstdio>\n#include "%s"\nint main() { std::printf("%%zu %%zu %%zu\\n", sizeof(tfra_rows_out), '
                 'sizeof(tfra_find_combine_typed_desc), sizeof(tfra_find_combine_ragged_typed_desc)); return 0; }\n'
                 % os.path.join(ROOT, "include", "tfra_mi355x.h"))
  exe = tmp_path / "sizes"
  subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", str(src), "-o", str(exe)])
  sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
  assert sizes == [ctypes.sizeof(built.RowsOut), ctypes.sizeof(built.FindCombineTypedDesc), ctypes.sizeof(built.FindCombineRaggedTypedDesc)]
  assert sizes == [16, 80, 96]


def test_python_surface_takes_out_dtype():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import ragged_embedding_ops, table_ops

  def takes(f):
    return "out_dtype" in inspect.signature(f).parameters

  for f in (table_ops._DeviceTable.find, table_ops._DeviceTable.find_combine_typed, table_ops._DeviceTable.find_combine_ragged,
            table_ops._DeviceTier.find, table_ops._DeviceTier.find_combine_typed, table_ops._DeviceTier.find_combine_ragged,
            table_ops.find_combine_many, table_ops.find_combine_ragged_many, table_ops.HkvHashTable.lookup,
            table_ops.CuckooHashTable.lookup, table_ops.TieredHashTable.find_combine_typed,
            table_ops.TieredHashTable.find_combine_ragged, de.Variable.lookup, de.Variable.lookup_combined,
            de.Variable.lookup_combined_ragged):
    assert takes(f), f.__qualname__
  for name in ("embedding_lookup", "embedding_lookup_unique", "embedding_lookup_sparse", "safe_embedding_lookup_sparse",
               "embedding_lookup_sparse_many",
               "safe_embedding_lookup_sparse_many"):
    assert takes(getattr(de, name)), name
  for name in ("embedding_lookup_sparse", "safe_embedding_lookup_sparse", "embedding_lookup_sparse_many",
               "safe_embedding_lookup_sparse_many"):
    assert takes(getattr(ragged_embedding_ops, name)), "ragged_embedding_ops." + name


def test_out_dtype_is_checked_before_any_call():
  import torch
  from tfra_amd.dynamic_embedding import _args
  assert _args._out_dtype(None) is None
  for d in (torch.float32, torch.float16, torch.bfloat16):
    assert _args._out_dtype(d) is d
  for d in (torch.int32, torch.float64, "bfloat16"):
    with pytest.raises(TypeError):
      _args._out_dtype(d)
