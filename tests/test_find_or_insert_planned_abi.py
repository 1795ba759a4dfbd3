"""CPU-only: tfra_table_find_or_insert_planned is declared in the header, exported by the library that build() makes and bound in
the ctypes layer with the header's argument list; the ABI version is unchanged (additive); the argument checks that come before
anything is enqueued need no device; the Python surface is there, down to init_on_lookup="plan"."""
import ctypes
import inspect
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfra_table_find_or_insert_planned"
ARGS = ["const tfra_sparse_plan_t* plan", "const void* init_values", "int init_is_full", "const uint64_t* scores", "void* rows_out",
        "uint8_t* found", "tfra_stream_t stream"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def test_header_declares_the_call():
  hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % NAME
  args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == ["tfra_table_t* t"] + ARGS
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity_and_types(built):
  P = ctypes.c_void_p
  assert built._SIGS.get(NAME) == [P, P, P, ctypes.c_int, P, P, P, P]
  assert len(built._SIGS[NAME]) == len(ARGS) + 1
  assert getattr(built.lib(), NAME).restype is ctypes.c_int


def test_a_null_table_is_refused_by_name(built):
  lib = built.lib()
  assert getattr(lib, NAME)(None, None, None, 0, None, None, None, None) == -1
  assert NAME in lib.tfra_last_error().decode()


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import table_ops, variable
  sig = inspect.signature(table_ops._DeviceTable.find_or_insert_planned)
  assert list(sig.parameters)[1:] == ["plan", "init_values", "scores", "return_exists", "out"]
  for cls in (table_ops.HkvHashTable, table_ops.CuckooHashTable):
    assert list(inspect.signature(cls.find_or_insert_planned).parameters)[1:] == ["plan", "dynamic_default_values", "return_exists", "name"]
  assert callable(variable.TrainableWrapper._plan_for_lookup)


def test_init_on_lookup_takes_plan_and_refuses_anything_else():
  """Variable.__init__ checks the keyword before it touches a device; get_variable hands it through"""
  from tfra_amd.dynamic_embedding import variable

  class Stop(Exception):
    pass

  def creator_that_stops(*a, **kw):
    raise Stop()

  for bad in ("bogus", "True", 2, None):
    with pytest.raises(ValueError, match="init_on_lookup"):
      variable.Variable(dim=8, devices=["cuda:0"], init_on_lookup=bad)
    with pytest.raises(ValueError, match="init_on_lookup"):
      variable.get_variable("foip_abi_bad_%r" % (bad,), dim=8, devices=["cuda:0"], init_on_lookup=bad)
  for good in (False, True, "plan"):
    v = variable.Variable.__new__(variable.Variable)
    try:
      v.__init__(dim=8, devices=["cuda:0"], init_on_lookup=good, kv_creator=types.SimpleNamespace(create=creator_that_stops))
    except ValueError as e:   # (the keyword itself was accepted)
      assert "init_on_lookup" not in str(e), e
    except Exception:
      pass
    assert v.init_on_lookup == good and type(v.init_on_lookup) is type(good)


def test_plan_is_true_for_every_predicate():
  """misses_are_static, admits_on_lookup and can_plan treat "plan" as True (on stubs, as tests/test_find_or_insert_abi.py)"""
  import torch
  from tfra_amd.dynamic_embedding import variable
  from tfra_amd.dynamic_embedding.optimizer import DynamicEmbeddingOptimizer, _refuse_init_on_lookup
  draw = lambda shape: None

  def stub(shard_num=1, **kw):
    return types.SimpleNamespace(value_dtype=torch.float32, dim=8, shard_num=shard_num, **kw)

  assert variable.misses_are_static(stub(initializer=draw, init_on_lookup="plan"))
  assert not variable.misses_are_static(stub(initializer=draw, init_on_lookup=False))
  assert DynamicEmbeddingOptimizer.can_plan(stub(initializer=draw, init_on_lookup="plan"), 200) is True
  assert DynamicEmbeddingOptimizer.can_plan(stub(initializer=draw, init_on_lookup="plan", shard_num=2), 200) is False
  s = stub(initializer=draw, init_on_lookup="plan")
  assert variable.Variable.admits_on_lookup(s) is True
  assert variable.Variable.admits_on_lookup(stub(initializer=0.5, init_on_lookup="plan")) is False
  s.admits_on_lookup = lambda: variable.Variable.admits_on_lookup(s)
  with pytest.raises(ValueError, match="init_on_lookup"):   # the step drivers' refusal
    _refuse_init_on_lookup(s, "PrefetchStep")
