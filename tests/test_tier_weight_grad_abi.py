"""CPU-only: tfra_tier_find_combine_backprop_weights and tfra_tier_find_combine_ragged_backprop_weights are declared in the header
with their argument lists, behind the tfra_tier_t typedef, exported by the library that build() makes and bound in the ctypes layer
with the lists of their tfra_table_ twins; the ABI version is unchanged (additive); a NULL tier is refused by name without a
device; the Python surface is there: _DeviceTier, TieredHashTable and Variable carry the weight-gradient methods, and
Variable._combined_operands no longer knows a one-table caller."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, I, U32, I64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64
CALLS = {
    "tfra_tier_find_combine_backprop_weights": (
        ["tfra_tier_t* tier", "tfra_workspace_t* ws", "size_t nnz", "const int64_t* ids", "const int64_t* seg", "const float* weights",
         "int combiner", "size_t n_rows", "const void* default_row", "const float* grad_out", "float* dw_out", "tfra_stream_t stream"],
        [P, P, SZ, P, P, P, I, SZ, P, P, P, P]),
    "tfra_tier_find_combine_ragged_backprop_weights": (
        ["tfra_tier_t* tier", "size_t n_rows", "const int64_t* row_splits", "size_t nnz", "const int64_t* ids", "const float* weights",
         "int combiner", "uint32_t flags", "int64_t fill_id", "const void* default_row", "const float* grad_out", "float* dw_out",
         "tfra_stream_t stream"],
        [P, SZ, P, SZ, P, P, I, U32, I64, P, P, P, P]),
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


def _declared(hdr, name):
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % name
  return m, [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_call(name):
  hdr = _header()
  m, args = _declared(hdr, name)
  assert args == CALLS[name][0]
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  # the types of the argument lists are declared above the calls
  at = m.start()
  assert 0 <= hdr.find("tfra_tier_t;") < at and 0 <= hdr.find("tfra_workspace_t;") < at
  # the one-table call's argument list, the tier in the table's place
  _, twin = _declared(hdr, name.replace("tfra_tier_", "tfra_table_"))
  assert twin[0] == "tfra_table_t* t" and twin[1:] == args[1:]


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_abi_version_stays(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", NAMES)
def test_binding_has_the_headers_arity_and_types(built, name):
  assert built._SIGS.get(name) == CALLS[name][1]
  assert len(built._SIGS[name]) == len(CALLS[name][0])
  assert getattr(built.lib(), name).restype is ctypes.c_int
  assert built._SIGS[name] == built._SIGS[name.replace("tfra_tier_", "tfra_table_")]


@pytest.mark.parametrize("name", NAMES)
def test_a_null_tier_is_refused_by_name(built, name):
  lib = built.lib()
  args = [0 if t in (SZ, I, U32, I64) else None for t in CALLS[name][1]]
  args[CALLS[name][1].index(SZ)] = 1
  assert getattr(lib, name)(*args) == -1          # TFRA_ERR_INVALID
  msg = lib.tfra_last_error().decode()
  assert msg.startswith(name + ":") and "null tier" in msg


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  tier, tab, dt = table_ops._DeviceTier, table_ops.TieredHashTable, table_ops._DeviceTable
  for owner in (tier, tab):
    assert par(owner.find_combine_weight_grad) == par(dt.find_combine_weight_grad) == ["ids", "seg", "weights", "combiner", "grad_out",
                                                                                        "default_row"]
    assert par(owner.find_combine_ragged_weight_grad) == par(dt.find_combine_ragged_weight_grad) == [
        "row_splits", "ids", "weights", "combiner", "grad_out", "prune", "fill_id", "default_row"]
    sig = inspect.signature(owner.find_combine_ragged_weight_grad).parameters
    assert sig["prune"].default is False and sig["fill_id"].default is None and sig["default_row"].default is None
  var = variable.Variable
  assert par(var.lookup_combined_weight_grad) == ["ids", "seg", "weights", "combiner", "grad_out", "name"]
  assert par(var.lookup_combined_ragged_weight_grad) == ["row_splits", "ids", "weights", "combiner", "grad_out", "prune", "fill_id", "name"]
  assert par(var._combined_operands) == ["ids", "ragged"]      # no caller reads one table only any more
