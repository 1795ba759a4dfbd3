"""CPU-only: tfra_field_entries is declared in the header behind tfra_multi_safe_entries with its cap, exported by the library that
build() makes and bound in the ctypes layer with the header's arity; the ABI version is unchanged (additive); n_rows == 0 is
TFRA_OK and a NULL row_splits, nslots == 0 and nslots above the cap are refused by name without a device.  The Python surface is
there: device_ops.field_entries and _field_entries_torch, de.layers and de.keras.layers, the layers' constructor errors, and the
torch route reproduces the reference docstring's case by hand."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ = ctypes.c_void_p, ctypes.c_size_t
NAME = "tfra_field_entries"
ARGS = ["size_t n_rows", "size_t per_row", "size_t nslots", "const int64_t* ids", "const int64_t* slots", "int64_t* entry_ids",
        "int64_t* row_splits", "int32_t* entry_pos", "int64_t* entry_seg", "int64_t* d_bad", "tfra_stream_t stream"]


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def test_header_declares_the_call_and_its_cap():
  hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)
  c = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, hdr)
  assert c, "include/tfra_mi355x.h does not declare %s" % NAME
  args = [re.sub(r"\s+", " ", a.strip()) for a in c.group(1).replace("\n", " ").split(",") if a.strip()]
  assert args == ARGS
  cap = re.search(r"#define\s+TFRA_FIELD_ENTRIES_MAX_SLOTS\s+(\d+)u\b", hdr)
  assert cap and int(cap.group(1)) >= 1024
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  behind = re.search(r"\bint\s+tfra_multi_safe_entries\s*\(", hdr)
  assert behind and behind.start() < c.start()


def test_library_exports_it_and_the_abi_version_stays(built):
  assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
  assert built.lib().tfra_abi_version() == 1


def test_binding_has_the_headers_arity(built):
  assert built._SIGS.get(NAME) == [SZ, SZ, SZ] + [P] * 8
  assert len(built._SIGS[NAME]) == len(ARGS)
  assert getattr(built.lib(), NAME).restype is ctypes.c_int


def test_refusals_that_need_no_device(built):
  from tfra_amd.dynamic_embedding import device_ops
  lib = built.lib()
  fn = getattr(lib, NAME)
  assert fn(0, 4, 3, None, None, None, None, None, None, None, None) == 0            # n_rows == 0: TFRA_OK, nothing looked at
  buf = (ctypes.c_int64 * 16)()
  at = ctypes.addressof(buf)
  assert fn(2, 0, 0, None, None, None, at, None, None, None, None) == -1              # TFRA_ERR_INVALID
  assert "field_entries: nslots == 0" in lib.tfra_last_error().decode()
  assert fn(2, 0, 3, None, None, None, None, None, None, None, None) == -1
  assert "field_entries: null row_splits" in lib.tfra_last_error().decode()
  assert fn(2, 2, 3, None, None, None, at, None, None, None, None) == -1
  assert "field_entries: null ids, slots or entry_ids" in lib.tfra_last_error().decode()
  cap = device_ops.FIELD_ENTRIES_MAX_SLOTS
  rc = fn(2, 0, cap + 1, None, None, None, at, None, None, None, None)
  assert rc != 0 and rc != -1 and ("exceeds %d" % cap) in lib.tfra_last_error().decode()   # TFRA_ERR_UNSUPPORTED
  rc = fn(1 << 16, 1 << 15, 3, at, at, at, at, None, None, None, None)
  assert rc != 0 and rc != -1 and ">= 2^31" in lib.tfra_last_error().decode()
  assert fn(2, 2, 3, at + 64, at + 64, at, at + 4, None, None, None, None) == -1
  assert "not 8-byte aligned" in lib.tfra_last_error().decode()
  assert fn(1, 2, 3, at + 64, at + 64, at, at + 8, None, None, None, None) == -1      # entry_ids [2] meets row_splits [4]
  assert "overlaps" in lib.tfra_last_error().decode()
  assert all(v == 0 for v in buf)


def test_python_surface_is_present():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import device_ops, ragged_embedding_ops
  names = ["ids2d", "slots2d", "nslots", "want_pos", "want_seg", "bad"]
  for fn in (device_ops.field_entries, device_ops._field_entries_torch):
    sig = inspect.signature(fn)
    assert list(sig.parameters) == names
    assert (sig.parameters["want_pos"].default, sig.parameters["want_seg"].default, sig.parameters["bad"].default) == (False, True, None)
  assert device_ops.FIELD_ENTRIES_MAX_SLOTS >= 1024
  assert device_ops.field_entries_fit(4096, 64, 26) and not device_ops.field_entries_fit(2, 3, device_ops.FIELD_ENTRIES_MAX_SLOTS + 1)
  assert not device_ops.field_entries_fit(1 << 16, 1 << 15, 3)
  assert de.layers is de.keras.layers
  import tfra_amd.dynamic_embedding.keras.layers  # noqa: F401  (the reference's import path)
  for cls in ("Embedding", "BasicEmbedding", "SquashedEmbedding", "FieldWiseEmbedding"):
    assert inspect.isclass(getattr(de.layers, cls))
  assert issubclass(de.layers.FieldWiseEmbedding, de.layers.Embedding) and issubclass(de.layers.SquashedEmbedding, de.layers.Embedding)
  call = inspect.signature(de.layers.FieldWiseEmbedding.__call__)
  assert list(call.parameters) == ["self", "ids", "return_trainable", "plan_writeback"]
  # the ragged training form takes the builder's segments, and its defaults keep today's path
  sig = inspect.signature(ragged_embedding_ops.embedding_lookup_sparse)
  assert sig.parameters["entry_seg"].default is None and sig.parameters["out_shape"].default is None


def test_constructor_errors_come_before_any_table():
  import torch
  from tfra_amd.dynamic_embedding import layers
  with pytest.raises(ValueError, match="slot_map_fn is not callable"):
    layers.FieldWiseEmbedding(4, 3, slot_map_fn=None)
  with pytest.raises(ValueError, match="slot_map_fn is not callable"):
    layers.FieldWiseEmbedding(4, 3, slot_map_fn=7)
  with pytest.raises(TypeError, match="nslots should be convertible to int"):
    layers.FieldWiseEmbedding(4, "three", slot_map_fn=lambda x: x % 3)
  with pytest.raises(TypeError, match="nslots should be convertible to int"):
    layers.FieldWiseEmbedding(4, None, slot_map_fn=lambda x: x % 3)
  with pytest.raises(ValueError, match="combiner"):
    layers.FieldWiseEmbedding(4, 3, slot_map_fn=lambda x: x % 3, combiner="max")
  with pytest.raises(ValueError, match="combiner"):
    layers.SquashedEmbedding(4, combiner="std")
  with pytest.raises(TypeError, match="embedding size"):
    layers.Embedding("wide")
  with pytest.raises(ValueError, match="max_norm"):
    layers.Embedding(4, max_norm=1.0)
  with pytest.raises(TypeError, match="unexpected keyword"):
    layers.Embedding(4, vocabulary=10)
  # ids of rank above 2 are refused before the layer's table is touched (PY/keras/layers/embedding.py:483-485)
  bare = layers.FieldWiseEmbedding.__new__(layers.FieldWiseEmbedding)
  with pytest.raises(NotImplementedError, match="higher than 2"):
    bare(torch.zeros((2, 3, 4), dtype=torch.int64))


def test_torch_route_reproduces_the_docstring_case_on_the_cpu():
  """PY/keras/layers/embedding.py:385-391: ids [[23, 12, 0], [9, 13, 10]], nslots 3, slot = id % 3.  Sample 0: slots 2, 0, 0 ->
  field 0 holds 12, 0 (input order), field 2 holds 23; sample 1: slots 0, 1, 1 -> field 0 holds 9, field 1 holds 13, 10."""
  import torch
  from tfra_amd.dynamic_embedding.device_ops import _field_entries_torch
  ids = torch.tensor([[23, 12, 0], [9, 13, 10]], dtype=torch.int64)
  bad = torch.zeros(1, dtype=torch.int64)
  e, rs, pos, seg = _field_entries_torch(ids, ids % 3, 3, want_pos=True, bad=bad)
  assert e.tolist() == [12, 0, 23, 9, 13, 10]
  # row_splits[b * 3 + f] = 3 b + sample b's entries with slot < f, then n: 0 2 2 | 3 4 6 | 6.  (Not "0 2 2 3 3 4 6", the two
  # samples' starts with sample 0's end between them: as this array, segment 3 = (sample 1, field 0) would be empty, and the
  # docstring's result has id 9 there.)
  assert rs.tolist() == [0, 2, 2, 3, 4, 6, 6] and rs.dtype == torch.int64
  assert pos.tolist() == [1, 2, 0, 3, 4, 5] and pos.dtype == torch.int32
  assert seg.tolist() == [0, 0, 2, 3, 4, 4]
  assert int(bad) == 0
  e, rs, pos, seg = _field_entries_torch(ids.to(torch.int32), ids % 3 - 1, 3, want_seg=False, bad=bad)   # slots 1, -1, -1 and -1, 0, 0: -1 is clamped to 0
  assert e.dtype == torch.int32 and pos is None and seg is None
  assert int(bad) == 3 and rs.tolist() == [0, 2, 3, 3, 6, 6, 6]
  assert e.tolist() == [12, 0, 23, 9, 13, 10]
  e, rs, _, _ = _field_entries_torch(torch.zeros((0, 4), dtype=torch.int64), torch.zeros((0, 4), dtype=torch.int64), 3)
  assert e.numel() == 0 and rs.tolist() == [0]
  e, rs, _, _ = _field_entries_torch(torch.zeros((3, 0), dtype=torch.int64), torch.zeros((3, 0), dtype=torch.int64), 3)
  assert e.numel() == 0 and rs.tolist() == [0] * 10
