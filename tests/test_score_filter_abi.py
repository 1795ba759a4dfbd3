"""CPU-only: the score-filtered calls (tfra_table_export_batch_if, tfra_table_erase_if, tfra_table_save_if) and the predicate enum
are declared in the header, exported by the library that build() makes and bound in the ctypes layer with the header's argument
lists; the ABI version is unchanged (additive); the Python surface is there, and its argument checks need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "tfra_table_export_batch_if": ["t", "pred", "threshold", "n", "offset", "d_counter", "cap", "keys", "values", "scores", "stream"],
    "tfra_table_erase_if": ["t", "pred", "threshold", "d_erased", "stream"],
    "tfra_table_save_if": ["t", "field", "pred", "threshold", "prefix", "buffer_keys", "append", "stream", "n_saved"],
}


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def _names(decls):
  return [re.split(r"[\s\*]+", a.strip())[-1] for a in decls.replace("\n", " ").split(",") if a.strip()]


def test_header_declares_the_calls_and_the_enum():
  hdr = _header()
  for name, args in ARGS.items():
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, "include/tfra_mi355x.h does not declare %s" % name
    assert _names(m.group(1)) == args, name
  e = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*tfra_score_pred\s*;", hdr)
  assert e, "include/tfra_mi355x.h does not declare tfra_score_pred"
  assert [x.strip().replace(" ", "") for x in e.group(1).split(",")] == ["TFRA_SCORE_GE=0", "TFRA_SCORE_LT=1"]
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


def test_library_exports_them_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  for name in ARGS:
    assert hasattr(lib, name), name
  assert built.lib().tfra_abi_version() == 1


def test_bindings_have_the_headers_arity_and_types(built):
  P, SZ, I, U64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
  assert built._SIGS.get("tfra_table_export_batch_if") == [P, I, U64, SZ, SZ, P, SZ, P, P, P, P]
  assert built._SIGS.get("tfra_table_erase_if") == [P, I, U64, P, P]
  assert built._SIGS.get("tfra_table_save_if") == [P, I, I, U64, ctypes.c_char_p, SZ, I, P, ctypes.POINTER(SZ)]
  for name, args in ARGS.items():
    assert len(built._SIGS[name]) == len(args), name
    assert getattr(built.lib(), name).restype is ctypes.c_int
  assert (built.SCORE_GE, built.SCORE_LT) == (0, 1)


def test_a_null_table_and_an_unknown_predicate_are_refused_by_name(built):
  """argument checks that come before anything is enqueued need no device"""
  lib = built.lib()
  for name, call in (("tfra_table_export_batch_if", lambda: lib.tfra_table_export_batch_if(None, 0, 0, 0, 0, None, 0, None, None, None, None)),
                     ("tfra_table_erase_if", lambda: lib.tfra_table_erase_if(None, 0, 0, None, None)),
                     ("tfra_table_save_if", lambda: lib.tfra_table_save_if(None, 0, 0, 0, b"x", 0, 0, None, None))):
    assert call() == -1
    assert name in lib.tfra_last_error().decode()


def test_python_surface_is_present_and_checks_its_arguments():
  from tfra_amd.dynamic_embedding import table_ops, variable
  for cls, names in ((table_ops._DeviceTable, ("count_if", "export_if", "erase_if", "save_if")),
                     (table_ops.HkvHashTable, ("export_if", "remove_if", "size_if", "save_delta_to_file_system")),
                     (variable.Variable, ("export_if", "remove_if", "size_if", "save_delta"))):
    for n in names:
      assert callable(getattr(cls, n, None)), (cls.__name__, n)
  for n in ("export_if", "remove_if", "size_if", "save_delta_to_file_system"):
    assert not hasattr(table_ops.CuckooHashTable, n), n
  assert table_ops._score_filter(0, "ge") == (0, 0)
  assert table_ops._score_filter(2**64 - 1, "lt") == (1, 2**64 - 1)
  for bad in ("GE", "gt", 0, None):
    with pytest.raises(ValueError):
      table_ops._score_filter(1, bad)
  for bad in (-1, 2**64, "x", None):
    with pytest.raises(ValueError):
      table_ops._score_filter(bad, "ge")
