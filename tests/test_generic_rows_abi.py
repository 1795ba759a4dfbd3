"""CPU-only: tfra_table_fetch_planned and tfra_table_store_rows are declared in the header with their argument lists,
exported by the library that build() makes and bound in the ctypes layer with the header's arity and types; the ABI version is
unchanged (additive); tfra_row_fields has the header's layout in `_capi.RowFields`; the refusals that need no device name their
function and return the stated code; the Python surface is there, down to the optimizers' keyword."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ = ctypes.c_void_p, ctypes.c_size_t
INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _calls(capi):
  return {
      "tfra_table_fetch_planned": (
          ["tfra_table_t* t", "const tfra_sparse_plan_t* plan", "const tfra_grads* g", "const void* default_row", "int64_t* keys_out",
           "const tfra_row_fields* rows_out", "float* gsum_out", "int64_t* d_count", "tfra_stream_t stream"],
          [P, P, ctypes.POINTER(capi.Grads), P, P, ctypes.POINTER(capi.RowFields), P, P, P]),
      "tfra_table_store_rows": (
          ["tfra_table_t* t", "size_t n", "const int64_t* d_n", "const int64_t* keys", "const tfra_row_fields* rows",
           "tfra_stream_t stream"],
          [P, SZ, P, P, ctypes.POINTER(capi.RowFields), P]),
  }


NAMES = ["tfra_table_fetch_planned", "tfra_table_store_rows"]


def _header(comments=False):
  text = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  return text if comments else re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_call(built, name):
  hdr = _header()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % name
  args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == _calls(built)[name][0]
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_it_and_the_abi_version_stays(built, name):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
  assert built.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", NAMES)
def test_binding_has_the_headers_arity_and_types(built, name):
  assert built._SIGS.get(name) == _calls(built)[name][1]
  assert getattr(built.lib(), name).restype is ctypes.c_int


def test_row_fields_layout(built):
  rf = built.RowFields
  assert ctypes.sizeof(rf) == 48
  assert (rf.struct_size.offset, rf.n_fields.offset, rf.field.offset) == (0, 4, 8)
  assert rf.field.size == 5 * 8 and ctypes.sizeof(ctypes.c_void_p) == 8   # five pointers in 8-byte steps
  m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_row_fields\s*;", _header())
  assert m, "include/tfra_mi355x.h does not define tfra_row_fields"
  members = [re.sub(r"\[.*", "", d.split()[-1].lstrip("*")) for d in m.group(1).split(";") if d.strip()]
  assert members == [f[0] for f in rf._fields_] == ["struct_size", "n_fields", "field"]
  assert re.search(r"float\s*\*\s*field\s*\[\s*5\s*\]", m.group(1))
  assert "sizeof(tfra_row_fields) = 48" in _header(comments=True)


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import optimizer, table_ops
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  dt = table_ops._DeviceTable
  assert par(dt.fetch_planned)[:4] == ["plan", "grads", "grad_scale", "fields"]
  assert par(dt.store_rows) == ["keys", "fields", "count"]
  for cls in (table_ops.HkvHashTable, table_ops.CuckooHashTable):
    assert par(cls.fetch_planned) == ["plan", "grads", "grad_scale", "fields"]
    assert par(cls.store_rows) == ["keys", "fields", "count"]
  for cls in (optimizer.Generic, optimizer.Momentum, optimizer.RMSProp):
    assert inspect.signature(cls.__init__).parameters["whole_rows"].default is False
  assert hasattr(optimizer.DynamicEmbeddingOptimizer, "_apply_generic_rows")


def test_the_keyword_reaches_the_optimizer_and_excludes_fused():
  from tfra_amd.dynamic_embedding import optimizer
  assert optimizer.Generic(slots=("a",), slot_init=(0.5,)).whole_rows is False
  assert optimizer.Generic(slots=("a",), slot_init=(0.5,), whole_rows=True).whole_rows is True
  for make in (optimizer.Momentum, optimizer.RMSProp):
    assert make().whole_rows is False and make(whole_rows=True).whole_rows is True
    assert make(whole_rows=True).kind is None          # still the Generic route: no fused kind
    assert make(fused=True).whole_rows is False
    with pytest.raises(ValueError, match="whole_rows"):
      make(fused=True, whole_rows=True)
  with pytest.raises(ValueError, match="whole_rows"):
    optimizer.Momentum(use_nesterov=True, fused=True, whole_rows=True)


# ---- refusals that are decided before the table or the plan is looked at: the handles below are never dereferenced ----
class _Bufs:
  def __init__(self, capi):
    self.raw = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(self.raw) + 63) & ~63
    self.aligned = ctypes.c_void_p(base)             # 64-byte aligned
    self.odd = ctypes.c_void_p(base + 4)             # 4-byte aligned only
    self.capi = capi

  def fields(self, n_fields=1, struct_size=48, ptrs=None):
    rf = self.capi.RowFields()
    rf.struct_size, rf.n_fields = struct_size, n_fields
    for f, p in enumerate(ptrs if ptrs is not None else [self.aligned.value] * max(0, min(n_fields, 5))):
      rf.field[f] = p
    return rf


def _refused(lib, name, rc, code):
  assert rc == code, (rc, lib.tfra_last_error().decode())
  assert name in lib.tfra_last_error().decode()


def test_fetch_refuses_null_arguments_by_name(built):
  lib, b = built.lib(), _Bufs(built)
  a = b.aligned
  good = [a, a, None, a, a, ctypes.byref(b.fields()), None, a, None]
  for i in (0, 1, 3, 4, 5, 7):   # t, plan, default_row, keys_out, rows_out, d_count
    args = list(good)
    args[i] = None
    _refused(lib, "tfra_table_fetch_planned", lib.tfra_table_fetch_planned(*args), INVALID)


def test_fetch_refuses_a_bad_record_by_name(built):
  lib, b = built.lib(), _Bufs(built)
  a = b.aligned
  call = lambda rf, g=None, gsum=None: lib.tfra_table_fetch_planned(a, a, g, a, a, ctypes.byref(rf), gsum, a, None)
  name = "tfra_table_fetch_planned"
  _refused(lib, name, call(b.fields(struct_size=40)), INVALID)
  _refused(lib, name, call(b.fields(n_fields=0)), INVALID)
  _refused(lib, name, call(b.fields(n_fields=6)), INVALID)
  _refused(lib, name, call(b.fields(n_fields=2, ptrs=[a.value, a.value, a.value])), INVALID)   # an entry beyond n_fields
  _refused(lib, name, call(b.fields(n_fields=1, ptrs=[b.odd.value])), UNSUPPORTED)              # a misaligned field
  # gradients and gsum_out go together; the record of the typed calls is checked with their codes
  g32 = built.Grads(a.value, built.TFRA_F32, 0, None)
  _refused(lib, name, call(b.fields(), ctypes.byref(g32), None), INVALID)
  _refused(lib, name, call(b.fields(), None, a), INVALID)
  _refused(lib, name, call(b.fields(), ctypes.byref(built.Grads(None, built.TFRA_F32, 0, None)), a), INVALID)
  _refused(lib, name, call(b.fields(), ctypes.byref(built.Grads(a.value, built.TFRA_F32, 1, None)), a), INVALID)
  _refused(lib, name, call(b.fields(), ctypes.byref(built.Grads(a.value, built.TFRA_I8, 0, None)), a), INVALID)
  _refused(lib, name, call(b.fields(), ctypes.byref(built.Grads(a.value, built.TFRA_F32, 0, a.value)), a), UNSUPPORTED)
  _refused(lib, name, call(b.fields(), ctypes.byref(built.Grads(b.odd.value, built.TFRA_BF16, 0, None)), a), UNSUPPORTED)
  _refused(lib, name, call(b.fields(), ctypes.byref(g32), b.odd), UNSUPPORTED)


def test_store_refuses_by_name_and_an_empty_call_is_ok(built):
  lib, b = built.lib(), _Bufs(built)
  a = b.aligned
  name = "tfra_table_store_rows"
  _refused(lib, name, lib.tfra_table_store_rows(None, 1, None, a, ctypes.byref(b.fields()), None), INVALID)
  assert lib.tfra_table_store_rows(a, 0, None, None, None, None) == 0       # n == 0: nothing is looked at
  _refused(lib, name, lib.tfra_table_store_rows(a, 1, None, None, ctypes.byref(b.fields()), None), INVALID)
  _refused(lib, name, lib.tfra_table_store_rows(a, 1, None, a, None, None), INVALID)
  call = lambda rf: lib.tfra_table_store_rows(a, 1, None, a, ctypes.byref(rf), None)
  _refused(lib, name, call(b.fields(struct_size=56)), INVALID)
  _refused(lib, name, call(b.fields(n_fields=0)), INVALID)
  _refused(lib, name, call(b.fields(n_fields=6)), INVALID)
  _refused(lib, name, call(b.fields(n_fields=1, ptrs=[a.value, a.value])), INVALID)
  _refused(lib, name, call(b.fields(n_fields=2, ptrs=[None, a.value])), INVALID)                # field[0] is required
  _refused(lib, name, call(b.fields(n_fields=2, ptrs=[a.value, b.odd.value])), UNSUPPORTED)
