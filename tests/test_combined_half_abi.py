"""CPU-only: the ABI of the typed combined write-backs — tfra_table_apply_planned_combined_typed and
tfra_multi_apply_planned_combined_typed are declared in the header, exported by the library that build() makes and bound in the
ctypes layer; tfra_apply_combined_typed_desc has the header's layout in its mirror; the ABI version and the untyped descriptor are
unchanged (additive); the record's refusals need no device and name their function; the Python keywords are there."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tfra_mi355x.h")
NAMES = ("tfra_table_apply_planned_combined_typed", "tfra_multi_apply_planned_combined_typed")
FIELDS = ["struct_size", "combiner", "table", "opt", "plan", "grad_out", "seg", "weights", "n_rows", "param_default_row"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_library_exports_both_calls_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  for name in NAMES:
    assert hasattr(lib, name), name
  assert built.lib().tfra_abi_version() == 1
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", _header())


def test_header_declares_both_calls_with_the_twins_arguments(built):
  hdr = _header()
  for name in NAMES:
    c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert c, "include/tfra_mi355x.h does not declare %s" % name
    args = [a.strip() for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
    twin = name[:-len("_typed")]
    assert len(args) == len(built._SIGS[name]) == len(built._SIGS[twin])   # the twin's arguments, grad_out replaced by the record
  single = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAMES[0], hdr).group(1)
  assert "const tfra_grads* grad_out" in single
  assert built._SIGS[NAMES[0]][3] == ctypes.POINTER(built.Grads)
  assert "const tfra_apply_combined_typed_desc* descs" in re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAMES[1], hdr).group(1)


def test_header_member_order_equals_the_mirror(built):
  hdr = _header()
  for c_name, mirror, grad in (("tfra_apply_combined_typed_desc", built.ApplyCombinedTypedDesc, "tfra_grads grad_out"),
                               ("tfra_apply_combined_desc", built.ApplyCombinedDesc, "const float* grad_out")):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % c_name, hdr)
    assert m, "include/tfra_mi355x.h does not define %s" % c_name
    members = [re.sub(r"\s+", " ", d.strip()) for d in m.group(1).split(";") if d.strip()]
    assert grad in members
    assert [d.split()[-1] for d in members] == FIELDS == [n for n, _ in mirror._fields_]


def test_sizes_and_offsets_equal_what_the_compiler_gives(built):
  """sizeof and every offsetof of both descriptors, printed by a C program compiled against the header."""
  cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if
             subprocess.call("command -v %s" % c, shell=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
  assert cc, "no C compiler"
  lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tfra_mi355x.h"', 'int main(void) {']
  for c_name in ("tfra_apply_combined_typed_desc", "tfra_apply_combined_desc"):
    lines.append('printf("%%zu", sizeof(%s));' % c_name)
    lines += ['printf(" %%zu", offsetof(%s, %s));' % (c_name, f) for f in FIELDS]
    lines.append('printf("\\n");')
  lines.append("return 0; }")
  with tempfile.TemporaryDirectory() as tmp:
    src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.dirname(HEADER), src, "-o", exe])
    out = subprocess.check_output([exe]).decode().split("\n")
  for line, mirror in zip(out, (built.ApplyCombinedTypedDesc, built.ApplyCombinedDesc)):
    got = [int(x) for x in line.split()]
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in FIELDS], (mirror.__name__, got)
  assert ctypes.sizeof(built.ApplyCombinedTypedDesc) == 88
  assert ctypes.sizeof(built.ApplyCombinedDesc) == 72   # the untyped descriptor is what it was
  assert ctypes.sizeof(built.ApplyCombinedTypedDesc) - ctypes.sizeof(built.ApplyCombinedDesc) == ctypes.sizeof(built.Grads) - 8


def test_refusals_of_the_record_need_no_device_and_name_the_function(built):
  lib = built.lib()
  buf = (ctypes.c_uint16 * 64)()
  at = ctypes.addressof(buf)
  at += (-at) % 16
  cases = [(None, -1, "null gradients"),
           (built.Grads(None, built.TFRA_BF16, 0, None), -1, "null gradients"),
           (built.Grads(at, built.TFRA_BF16, 1, None), -1, "reserved"),
           (built.Grads(at, 3, 0, None), -1, "dtype"),
           (built.Grads(at + 2, built.TFRA_F16, 0, None), built.ERR_UNSUPPORTED, "8-B aligned"),
           (built.Grads(at, built.TFRA_F32, 0, at), built.ERR_UNSUPPORTED, "float32 gradients take no scale")]
  one = ctypes.c_void_p(8)   # a non-NULL table that must never be looked at
  for g, code, text in cases:
    ref = None if g is None else ctypes.byref(g)
    assert lib.tfra_table_apply_planned_combined_typed(one, None, None, ref, None, None, 0, 4, None, None) == code, text
    msg = lib.tfra_last_error().decode()
    assert msg.startswith("apply_planned_combined_typed: ") and text in msg, msg
  # the grouped call: an empty list is fine, a NULL list with members is not; neither needs a device
  launches = ctypes.c_uint32(77)
  assert lib.tfra_multi_apply_planned_combined_typed(None, 0, None, ctypes.c_void_p(ctypes.addressof(launches)), None) == 0
  assert launches.value == 0
  assert lib.tfra_multi_apply_planned_combined_typed(None, 2, None, None, None) == -1
  assert lib.tfra_last_error().decode().startswith("multi_apply_planned_combined_typed: ")


def test_python_keywords_exist():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops
  from tfra_amd.dynamic_embedding.variable import SparseTrainableWrapper
  for fn in (table_ops._DeviceTable.apply_planned_combined, table_ops.apply_planned_combined_many,
             de.DynamicEmbeddingOptimizer.apply_combined_gradients, de.DynamicEmbeddingOptimizer.apply_combined_gradients_many):
    p = inspect.signature(fn).parameters
    assert "grad_scale" in p and p["grad_scale"].default is None, fn
  p = inspect.signature(SparseTrainableWrapper.check_grad_out).parameters
  assert list(p) == ["self", "grad_out", "keep_half"] and p["keep_half"].default is False
  assert list(inspect.signature(table_ops.apply_planned_combined_many).parameters) == ["requests", "p_list", "sync", "grad_scale"]
