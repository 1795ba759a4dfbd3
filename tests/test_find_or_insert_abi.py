"""CPU-only: tfra_table_find_or_insert is declared in the header, exported by the library that build() makes and bound in the ctypes
layer with the header's argument list; the ABI version is unchanged (additive); the argument checks that come before anything is
enqueued need no device; the Python surface is there, down to Variable.lookup_or_insert and the init_on_lookup keyword."""
import ctypes
import inspect
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_table_find_or_insert"
ARGS = ["t", "n", "d_n", "keys", "init_values", "init_is_full", "scores", "values_out", "found", "stream"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def test_header_declares_the_call():
  hdr = _header()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % NAME
  args = [a.strip() for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
  assert [re.split(r"[\s\*]+", a)[-1] for a in args] == ARGS
  assert re.sub(r"\s+", " ", args[2]) == "const int64_t* d_n" and re.sub(r"\s+", " ", args[5]) == "int init_is_full"
  assert re.sub(r"\s+", " ", args[7]) == "void* values_out" and re.sub(r"\s+", " ", args[8]) == "uint8_t* found"
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_and_types(built):
  P, SZ = ctypes.c_void_p, ctypes.c_size_t
  assert built._SIGS.get(NAME) == [P, SZ, P, P, P, ctypes.c_int, P, P, P, P]
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int


def test_a_null_table_is_refused_by_name(built):
  lib = built.lib()
  assert lib.tfra_table_find_or_insert(None, 1, None, None, None, 0, None, None, None, None) == -1
  assert NAME in lib.tfra_last_error().decode()


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  sig = inspect.signature(table_ops._DeviceTable.find_or_insert)
  assert list(sig.parameters)[1:] == ["keys", "init_values", "scores", "return_exists", "count", "out"]
  for cls in (table_ops.HkvHashTable, table_ops.CuckooHashTable):
    names = list(inspect.signature(cls.find_or_insert).parameters)
    assert names[1:4] == ["keys", "dynamic_default_values", "return_exists"]
  assert list(inspect.signature(variable.Variable.lookup_or_insert).parameters)[1:3] == ["keys", "return_exists"]
  for fn in (variable.Variable.__init__, variable.get_variable):
    assert inspect.signature(fn).parameters["init_on_lookup"].default is False


def test_one_predicate_decides_the_fused_write_backs():
  """not callable, or init_on_lookup: what can_plan asks of the variable's initializer (on stubs, as tests/test_half_writeback_can_plan.py)"""
  import torch
  from tfra_amd.dynamic_embedding import variable
  from tfra_amd.dynamic_embedding.optimizer import DynamicEmbeddingOptimizer
  draw = lambda shape: None

  def stub(shard_num=1, **kw):
    return types.SimpleNamespace(value_dtype=torch.float32, dim=8, shard_num=shard_num, **kw)

  assert variable.misses_are_static(stub(initializer=0.5)) and variable.misses_are_static(stub(initializer=None))
  assert not variable.misses_are_static(stub(initializer=draw))
  assert not variable.misses_are_static(stub(initializer=draw, init_on_lookup=False))
  assert variable.misses_are_static(stub(initializer=draw, init_on_lookup=True))
  assert DynamicEmbeddingOptimizer.can_plan(stub(initializer=draw, init_on_lookup=True), 200) is True
  assert DynamicEmbeddingOptimizer.can_plan(stub(initializer=draw, init_on_lookup=False), 200) is False
  assert DynamicEmbeddingOptimizer.can_plan(stub(initializer=draw, init_on_lookup=True, shard_num=2), 200) is False
