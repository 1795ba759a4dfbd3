"""CPU-only: the ABI of the typed weight-gradient calls — the seven *_backprop_weights_typed calls are declared in
the header, exported by the library that build() makes and bound in the ctypes layer; the two typed descriptors have the header's
layout in their mirrors; the ABI version and the untyped descriptors are unchanged (additive); the record's refusals need no device,
name their function and never look at the table or tier handle; the Python keywords are there."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tfra_mi355x.h")
SINGLE = ("tfra_table_find_combine_backprop_weights_typed", "tfra_table_find_combine_ragged_backprop_weights_typed",
          "tfra_tier_find_combine_backprop_weights_typed", "tfra_tier_find_combine_ragged_backprop_weights_typed",
          "tfra_sparse_segment_combine_backprop_weights_typed")
GROUPED = ("tfra_multi_find_combine_backprop_weights_typed", "tfra_multi_find_combine_ragged_backprop_weights_typed")
NAMES = SINGLE + GROUPED
TUPLE_FIELDS = ["struct_size", "combiner", "table", "tier", "nnz", "ids", "seg", "weights", "n_rows", "default_row", "grad_out", "dw_out"]
RAGGED_FIELDS = ["struct_size", "combiner", "table", "tier", "n_rows", "row_splits", "nnz", "ids", "weights", "flags", "reserved",
                 "fill_id", "default_row", "grad_out", "dw_out"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def _descs(built):
  """(C name, mirror, grad_out's declaration, member names): the two typed descriptors, then their untyped twins."""
  return (("tfra_find_combine_wgrad_typed_desc", built.FindCombineWgradTypedDesc, "tfra_grads grad_out", TUPLE_FIELDS),
          ("tfra_find_combine_ragged_wgrad_typed_desc", built.FindCombineRaggedWgradTypedDesc, "tfra_grads grad_out", RAGGED_FIELDS),
          ("tfra_find_combine_wgrad_desc", built.FindCombineWgradDesc, "const float* grad_out", TUPLE_FIELDS),
          ("tfra_find_combine_ragged_wgrad_desc", built.FindCombineRaggedWgradDesc, "const float* grad_out", RAGGED_FIELDS))


def test_library_exports_the_seven_calls_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  for name in NAMES:
    assert hasattr(lib, name), name
  assert built.lib().tfra_abi_version() == 1
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", _header())


def test_header_declares_the_calls_with_the_twins_arguments(built):
  hdr = _header()
  for name in NAMES:
    c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert c, "include/tfra_mi355x.h does not declare %s" % name
    args = [a.strip() for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
    twin = name[:-len("_typed")]
    t = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % twin, hdr)
    twin_args = [a.strip() for a in t.group(1).replace("\n", " ").split(",") if a.strip()]
    assert len(args) == len(twin_args) == len(built._SIGS[name]) == len(built._SIGS[twin]), name
    if name in SINGLE:
      at = args.index("const tfra_grads* grad_out")
      assert twin_args[at] == "const float* grad_out", name           # the record stands where the float pointer stood
      assert [a for i, a in enumerate(args) if i != at] == [a for i, a in enumerate(twin_args) if i != at], name
      assert built._SIGS[name][at] == ctypes.POINTER(built.Grads)
  assert "const tfra_find_combine_wgrad_typed_desc* descs" in re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % GROUPED[0], hdr).group(1)
  assert "const tfra_find_combine_ragged_wgrad_typed_desc* descs" in re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % GROUPED[1], hdr).group(1)


def test_header_member_order_equals_the_mirrors(built):
  hdr = _header()
  for c_name, mirror, grad, fields in _descs(built):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % c_name, hdr)
    assert m, "include/tfra_mi355x.h does not define %s" % c_name
    members = [re.sub(r"\s+", " ", d.strip()) for d in m.group(1).split(";") if d.strip()]
    assert grad in members, c_name
    assert [d.split()[-1] for d in members] == fields == [n for n, _ in mirror._fields_], c_name


def test_sizes_and_offsets_equal_what_the_compiler_gives(built):
  """sizeof and every offsetof of the four descriptors, printed by a C program compiled against the header."""
  cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if
             subprocess.call("command -v %s" % c, shell=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0), None)
  assert cc, "no C compiler"
  lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tfra_mi355x.h"', 'int main(void) {']
  for c_name, _, _, fields in _descs(built):
    lines.append('printf("%%zu", sizeof(%s));' % c_name)
    lines += ['printf(" %%zu", offsetof(%s, %s));' % (c_name, f) for f in fields]
    lines.append('printf("\\n");')
  lines.append("return 0; }")
  with tempfile.TemporaryDirectory() as tmp:
    src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.dirname(HEADER), src, "-o", exe])
    out = subprocess.check_output([exe]).decode().split("\n")
  for line, (c_name, mirror, _, fields) in zip(out, _descs(built)):
    got = [int(x) for x in line.split()]
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields], (c_name, got)
  # each typed descriptor is its twin with 24 bytes of record in the 8-byte pointer's place; the twins keep their sizes
  assert ctypes.sizeof(built.FindCombineWgradDesc) == 88 and ctypes.sizeof(built.FindCombineRaggedWgradDesc) == 104
  assert ctypes.sizeof(built.FindCombineWgradTypedDesc) - ctypes.sizeof(built.FindCombineWgradDesc) == 16
  assert ctypes.sizeof(built.FindCombineRaggedWgradTypedDesc) - ctypes.sizeof(built.FindCombineRaggedWgradDesc) == 16
  assert ctypes.sizeof(built.Grads) - 8 == 16


def _single_calls(lib, one):
  """name -> (message prefix, f(record reference) -> code): each single call with a bogus non-NULL owner and nothing else."""
  return {
      "find_combine_backprop_weights_typed: ":
          lambda g: lib.tfra_table_find_combine_backprop_weights_typed(one, None, 4, None, None, None, 0, 4, None, g, None, None),
      "find_combine_ragged_backprop_weights_typed: ":
          lambda g: lib.tfra_table_find_combine_ragged_backprop_weights_typed(one, 4, None, 4, None, None, 0, 0, 0, None, g, None, None),
      "tfra_tier_find_combine_backprop_weights_typed: ":
          lambda g: lib.tfra_tier_find_combine_backprop_weights_typed(one, None, 4, None, None, None, 0, 4, None, g, None, None),
      "tfra_tier_find_combine_ragged_backprop_weights_typed: ":
          lambda g: lib.tfra_tier_find_combine_ragged_backprop_weights_typed(one, 4, None, 4, None, None, 0, 0, 0, None, g, None, None),
      "segment_combine_backprop_weights_typed: ":
          lambda g: lib.tfra_sparse_segment_combine_backprop_weights_typed(one, 4, 4, None, None, g, None, None, 0, 4, None, None),
  }


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
  one = ctypes.c_void_p(8)   # a non-NULL table / tier / workspace that must never be looked at
  for prefix, call in _single_calls(lib, one).items():
    for g, code, text in cases:
      assert call(None if g is None else ctypes.byref(g)) == code, (prefix, text)
      msg = lib.tfra_last_error().decode()
      assert msg.startswith(prefix) and text in msg, msg


def test_grouped_refusals_check_the_record_before_the_owner(built):
  lib = built.lib()
  buf = (ctypes.c_uint16 * 64)()
  at = ctypes.addressof(buf)
  at += (-at) % 16
  one = ctypes.c_void_p(8)   # a non-NULL workspace: a list's records are checked before it is used
  for name, mirror in zip(GROUPED, (built.FindCombineWgradTypedDesc, built.FindCombineRaggedWgradTypedDesc)):
    f = getattr(lib, name)
    launches = ctypes.c_uint32(77)
    assert f(None, 0, None, ctypes.c_void_p(ctypes.addressof(launches)), None) == 0     # an empty list is fine
    assert launches.value == 0
    assert f(None, 2, None, None, None) == -1                                             # a NULL list with members is not
    assert lib.tfra_last_error().decode().startswith(name[len("tfra_"):] + ": ")
    descs = (mirror * 2)()
    for d in descs:
      d.struct_size = ctypes.sizeof(mirror)
      d.table, d.tier = 8, 8            # bogus handles, both set: looked at only behind the record
      d.grad_out = built.Grads(at, built.TFRA_BF16, 0, None)
    descs[1].grad_out = built.Grads(at + 2, built.TFRA_F16, 0, None)
    assert f(one, 2, ctypes.c_void_p(ctypes.addressof(descs)), None, None) == built.ERR_UNSUPPORTED
    msg = lib.tfra_last_error().decode()
    assert msg.startswith(name[len("tfra_"):] + ": descriptor 1: ") and "8-B aligned" in msg, msg
    descs[1].grad_out = built.Grads(at, built.TFRA_F16, 1, None)
    assert f(one, 2, ctypes.c_void_p(ctypes.addressof(descs)), None, None) == -1
    assert "descriptor 1: " in lib.tfra_last_error().decode() and "reserved" in lib.tfra_last_error().decode()
    descs[1].grad_out = built.Grads(at, built.TFRA_F16, 0, None)
    assert f(one, 2, ctypes.c_void_p(ctypes.addressof(descs)), None, None) == -1        # the records pass: now the owner is looked at
    assert "descriptor 0: exactly one of table / tier" in lib.tfra_last_error().decode()


def test_python_keywords_exist():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops, table_ops, variable
  par = lambda f: list(inspect.signature(f).parameters)[1:]
  dt = table_ops._DeviceTable
  for owner in (dt, table_ops._DeviceTier, table_ops.TieredHashTable):
    assert par(owner.find_combine_weight_grad_typed) == ["ids", "seg", "weights", "combiner", "grad_out", "default_row", "grad_scale"]
    assert par(owner.find_combine_ragged_weight_grad_typed) == ["row_splits", "ids", "weights", "combiner", "grad_out", "prune",
                                                                "fill_id", "default_row", "grad_scale"]
    for f in (owner.find_combine_weight_grad_typed, owner.find_combine_ragged_weight_grad_typed):
      p = inspect.signature(f).parameters
      assert p["grad_scale"].default is None and p["default_row"].default is None
  var = variable.Variable
  assert par(var.lookup_combined_weight_grad_typed) == ["ids", "seg", "weights", "combiner", "grad_out", "grad_scale", "name"]
  assert par(var.lookup_combined_ragged_weight_grad_typed) == ["row_splits", "ids", "weights", "combiner", "grad_out", "prune", "fill_id",
                                                               "grad_scale", "name"]
  for fn in (var.lookup_combined_weight_grad_typed, var.lookup_combined_ragged_weight_grad_typed,
             variable.SparseTrainableWrapper.weights_grad, variable.sparse_weights_grad_many, de.sparse_weights_grad_many,
             table_ops.find_combine_weight_grad_many, table_ops.find_combine_ragged_weight_grad_many,
             device_ops.sparse_segment_combine_weight_grad):
    p = inspect.signature(fn).parameters
    assert "grad_scale" in p and p["grad_scale"].default is None, fn
  assert list(inspect.signature(table_ops.find_combine_weight_grad_many).parameters) == ["requests", "return_launches", "grad_scale"]
  assert list(inspect.signature(table_ops.find_combine_ragged_weight_grad_many).parameters) == ["requests", "return_launches", "grad_scale"]
  assert list(inspect.signature(variable.SparseTrainableWrapper.weights_grad).parameters) == ["self", "grad_out", "grad_scale"]
  p = inspect.signature(variable.SparseTrainableWrapper.check_grad_out).parameters
  assert list(p) == ["self", "grad_out", "keep_half"] and p["keep_half"].default is False      # pinned as it is
  p = inspect.signature(dt._weight_grad_out).parameters
  assert list(p) == ["self", "grad_out", "n_rows", "keep_half", "grad_scale"] and p["keep_half"].default is False


def test_the_model_tells_a_scale_before_the_dot_product_from_one_after_it():
  """No code of the library runs here: the GPU comparisons at scale 1e-3 (tests/test_gpu_wgrad_half.py) take GO32 with the scale
  per element from tests/half_grads_model.py, and this shows that such an expectation sees a kernel that scales d_p instead —
  (sum of f32(g) * x) * s differs from sum of (f32(g) * s) * x in the last bits for most rows of 64 random columns."""
  import numpy as np
  from tests import half_grads_model as M
  from tests.test_gpu_wgrad_half import random_half_bits
  f32 = np.float32
  b16 = random_half_bits(64, 64, "bfloat16", 5)
  x = np.random.default_rng(6).standard_normal(64).astype(f32)
  before, after = np.zeros(64, f32), np.zeros(64, f32)
  for c in range(64):
    before = before + M.g32(b16[:, c], "bfloat16", 1e-3) * x[c]
    after = after + M.g32(b16[:, c], "bfloat16", None) * x[c]
  after = after * f32(1e-3)
  assert (before.view(np.uint32) != after.view(np.uint32)).sum() > 16
