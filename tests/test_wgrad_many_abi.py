"""CPU-only: tfra_multi_find_combine_backprop_weights and tfra_multi_find_combine_ragged_backprop_weights are declared in the header
with their argument lists and their descriptors' fields in order, exported by the library that build() makes and bound in the
ctypes layer — the mirrors have the header's field names, order and size —; the ABI version is unchanged (additive); an empty
list is TFRA_OK and a NULL list is refused by name, both without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, I32, U32, I64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64
ARGS = ["tfra_workspace_t* ws", "size_t n_tables", "const %s* descs", "uint32_t* launches_out", "tfra_stream_t stream"]
CTYPE = {"uint32_t": U32, "int32_t": I32, "int64_t": I64, "size_t": SZ}
# call -> (descriptor, its ctypes mirror, the forward's mirror, [(C type, field)] in order)
CALLS = {
    "tfra_multi_find_combine_backprop_weights": ("tfra_find_combine_wgrad_desc", "FindCombineWgradDesc", "TierFindCombineDesc", [
        ("uint32_t", "struct_size"), ("int32_t", "combiner"), ("tfra_table_t*", "table"), ("tfra_tier_t*", "tier"), ("size_t", "nnz"),
        ("const int64_t*", "ids"), ("const int64_t*", "seg"), ("const float*", "weights"), ("size_t", "n_rows"),
        ("const void*", "default_row"), ("const float*", "grad_out"), ("float*", "dw_out")]),
    "tfra_multi_find_combine_ragged_backprop_weights": (
        "tfra_find_combine_ragged_wgrad_desc", "FindCombineRaggedWgradDesc", "TierFindCombineRaggedDesc", [
            ("uint32_t", "struct_size"), ("int32_t", "combiner"), ("tfra_table_t*", "table"), ("tfra_tier_t*", "tier"),
            ("size_t", "n_rows"), ("const int64_t*", "row_splits"), ("size_t", "nnz"), ("const int64_t*", "ids"),
            ("const float*", "weights"), ("uint32_t", "flags"), ("uint32_t", "reserved"), ("int64_t", "fill_id"),
            ("const void*", "default_row"), ("const float*", "grad_out"), ("float*", "dw_out")]),
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
  assert args == [a % CALLS[name][0] if "%s" in a else a for a in ARGS]
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  # the types of the argument list and of the descriptor are declared above the call
  at = m.start()
  for t in ("tfra_tier_t;", "tfra_workspace_t;", "} %s;" % CALLS[name][0]):
    assert 0 <= hdr.find(t) < at, t


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_descriptor_fields_in_order(name):
  desc, _, _, fields = CALLS[name]
  m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % desc, _header())
  assert m, "include/tfra_mi355x.h does not declare %s" % desc
  got = []
  for decl in m.group(1).split(";"):
    decl = re.sub(r"\s+", " ", decl.strip())
    if decl:
      t, f = decl.rsplit(" ", 1)
      got.append((t.replace(" *", "*"), f))
  assert got == fields


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_abi_version_stays(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", NAMES)
def test_binding_and_mirror_match_the_header(built, name):
  _, mirror, forward, fields = CALLS[name]
  assert built._SIGS.get(name) == [P, SZ, P, P, P]
  assert getattr(built.lib(), name).restype is ctypes.c_int
  cls = getattr(built, mirror)
  assert [f for f, _ in cls._fields_] == [f for _, f in fields]
  assert [t for _, t in cls._fields_] == [P if c.endswith("*") else CTYPE[c] for c, _ in fields]
  # sizeof against the header's layout: every field at its natural alignment on LP64, the struct rounded to 8
  off = 0
  for c, f in fields:
    size = 8 if c.endswith("*") else ctypes.sizeof(CTYPE[c])
    off = (off + size - 1) // size * size
    assert getattr(cls, f).offset == off, f
    off += size
  assert ctypes.sizeof(cls) == (off + 7) // 8 * 8
  # the forward's tier descriptor with grad_out and dw_out in the place of out
  fwd = getattr(built, forward)
  assert list(cls._fields_[:-2]) == list(fwd._fields_[:-1]) and fwd._fields_[-1][0] == "out"
  assert ctypes.sizeof(cls) == ctypes.sizeof(fwd) + 8


@pytest.mark.parametrize("name", NAMES)
def test_an_empty_list_is_ok_and_a_null_list_is_refused_by_name(built, name):
  lib = built.lib()
  launches = ctypes.c_uint32(7)
  assert getattr(lib, name)(None, 0, None, ctypes.byref(launches), None) == 0          # TFRA_OK, no workspace, no device
  assert launches.value == 0
  assert getattr(lib, name)(None, 0, None, None, None) == 0
  assert getattr(lib, name)(None, 2, None, ctypes.byref(launches), None) == -1         # TFRA_ERR_INVALID
  msg = lib.tfra_last_error().decode()
  assert msg.startswith(name[len("tfra_"):] + ":") and "null argument" in msg


def test_the_python_layer_exports_the_grouped_forms(built):
  import tfra_amd.dynamic_embedding as de
  assert callable(de.sparse_weights_grad_many)
  assert de.table_ops.find_combine_weight_grad_many([]) == [] and de.table_ops.find_combine_ragged_weight_grad_many([]) == []
  assert de.table_ops.find_combine_weight_grad_many([], return_launches=True) == ([], 0)
  assert de.sparse_weights_grad_many([]) == []
