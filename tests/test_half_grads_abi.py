"""CPU-only: the half-gradient write-backs' ABI — tfra_grads and the three *_typed calls are declared in the header, exported by the
library that build() makes and bound in the ctypes layer with the header's layout; the ABI version is unchanged (additive); the
refusals that need no device name their function; the Python keywords are there."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tfra_table_apply_sparse_typed", "tfra_table_apply_planned_typed", "tfra_reduce_by_key_typed")


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def test_library_exports_the_three_calls_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  for name in NAMES:
    assert hasattr(lib, name), name
  assert built.lib().tfra_abi_version() == 1
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", _header())


def test_grads_struct_layout(built):
  G = built.Grads
  assert ctypes.sizeof(G) == 24
  assert [getattr(G, n).offset for n, _ in G._fields_] == [0, 8, 12, 16]


def test_header_member_order_equals_the_bindings(built):
  hdr = _header()
  m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_grads\s*;", hdr)
  assert m, "include/tfra_mi355x.h does not define tfra_grads"
  members = [re.sub(r"\s+", " ", d.strip()) for d in m.group(1).split(";") if d.strip()]
  assert members == ["const void* grads", "int32_t dtype", "int32_t reserved", "const float* d_scale"]
  assert [d.split()[-1] for d in members] == [n for n, _ in built.Grads._fields_]
  for name in NAMES:
    c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert c, "include/tfra_mi355x.h does not declare %s" % name
    args = [a.strip() for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
    assert len(args) == len(built._SIGS[name]) and "const tfra_grads* g" in args
    assert built._SIGS[name][args.index("const tfra_grads* g")] == ctypes.POINTER(built.Grads)
    twin = name[:-len("_typed")]
    assert len(built._SIGS[twin]) == len(built._SIGS[name])   # the twin's arguments, the matrix replaced by the record


def test_refusals_of_the_record_need_no_device_and_name_their_function(built):
  lib = built.lib()
  buf = (ctypes.c_uint16 * 64)()
  at = ctypes.addressof(buf)
  at += (-at) % 16
  cases = [(None, -1, "null gradients"),
           (built.Grads(None, built.TFRA_BF16, 0, None), -1, "null gradients"),
           (built.Grads(at, built.TFRA_BF16, 1, None), -1, "reserved"),
           (built.Grads(at, 99, 0, None), -1, "dtype"),
           (built.Grads(at + 2, built.TFRA_F16, 0, None), built.ERR_UNSUPPORTED, "8-B aligned"),
           (built.Grads(at, built.TFRA_F32, 0, at), built.ERR_UNSUPPORTED, "float32 gradients take no scale")]
  one = ctypes.c_void_p(8)   # a non-NULL table / workspace that must never be looked at
  for g, code, text in cases:
    ref = None if g is None else ctypes.byref(g)
    for name, call in (("apply_sparse_typed", lambda: lib.tfra_table_apply_sparse_typed(one, None, 4, None, ref, None, None)),
                       ("apply_planned_typed", lambda: lib.tfra_table_apply_planned_typed(one, None, None, ref, None, None)),
                       ("reduce_by_key_typed", lambda: lib.tfra_reduce_by_key_typed(one, 4, None, 4, ref, None, None, None, None))):
      assert call() == code, (name, text)
      msg = lib.tfra_last_error().decode()
      assert msg.startswith(name + ": ") and text in msg, msg


def test_python_keywords_exist():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops, table_ops
  for fn in (table_ops._DeviceTable.apply_sparse, table_ops._DeviceTable.apply_planned, device_ops.reduce_by_key,
             de.DynamicEmbeddingOptimizer.apply_sparse, de.DynamicEmbeddingOptimizer.apply_gradients):
    p = inspect.signature(fn).parameters
    assert "grad_scale" in p and p["grad_scale"].default is None, fn
  assert list(inspect.signature(de.DynamicEmbeddingOptimizer.apply_sparse).parameters) == ["self", "var", "ids", "grad", "p", "plan", "grad_scale"]
