"""CPU-only: the C entries of the gradient of the pooled lookup's weights (tfra_table_find_combine_backprop_weights, its ragged
form and the chain twin tfra_sparse_segment_combine_backprop_weights) are declared in the header with their argument names,
exported by the library that build() makes and bound in the ctypes layer with the header's argument lists; the ABI version is
unchanged (additive); the Python surface is present."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SZ, I, U32, I64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64
ENTRIES = {
    "tfra_table_find_combine_backprop_weights":
        (["t", "ws", "nnz", "ids", "seg", "weights", "combiner", "n_rows", "default_row", "grad_out", "dw_out", "stream"],
         [P, P, SZ, P, P, P, I, SZ, P, P, P, P]),
    "tfra_table_find_combine_ragged_backprop_weights":
        (["t", "n_rows", "row_splits", "nnz", "ids", "weights", "combiner", "flags", "fill_id", "default_row", "grad_out", "dw_out",
          "stream"],
         [P, SZ, P, SZ, P, P, I, U32, I64, P, P, P, P]),
    "tfra_sparse_segment_combine_backprop_weights":
        (["ws", "nnz", "dim", "rows", "idx", "grad_out", "seg", "weights", "combiner", "n_rows", "dw_out", "stream"],
         [P, SZ, I, P, P, P, P, P, I, SZ, P, P]),
}


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares_the_entry(name):
  hdr = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % name
  args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
  assert [re.split(r"[\s\*]+", a)[-1] for a in args] == ENTRIES[name][0]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_the_entry(built, name):
  lib = ctypes.CDLL(built.LIB_PATH)
  assert hasattr(lib, name)
  assert built.lib().tfra_abi_version() == 1


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_binding_has_the_headers_signature(built, name):
  assert built._SIGS.get(name) == ENTRIES[name][1]
  assert len(ENTRIES[name][0]) == len(ENTRIES[name][1])
  assert getattr(built.lib(), name).restype is ctypes.c_int


def test_python_surface_is_present():
  from tfra_amd.dynamic_embedding import device_ops, table_ops, variable
  assert callable(getattr(device_ops, "sparse_segment_combine_weight_grad", None))
  assert callable(getattr(table_ops._DeviceTable, "find_combine_weight_grad", None))
  assert callable(getattr(table_ops._DeviceTable, "find_combine_ragged_weight_grad", None))
  assert callable(getattr(variable.Variable, "lookup_combined_weight_grad", None))
  assert callable(getattr(variable.Variable, "lookup_combined_ragged_weight_grad", None))
  assert callable(getattr(variable.SparseTrainableWrapper, "weights_grad", None))


# ---- the float64 closed form the GPU tests compare against (tests/wgrad_model.py) is the autograd of the reference's chain ------
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_the_closed_form_is_the_autograd_of_the_reference_chain(combiner):
  import numpy as np
  from tests.wgrad_model import bounds_of, chain_autograd, wgrad_model
  rng = np.random.default_rng(17)
  n_rows, dim = 40, 12
  counts = rng.integers(0, 9, size=n_rows)
  seg = np.repeat(np.arange(n_rows), counts)
  E = rng.standard_normal((seg.size, dim))
  G = rng.standard_normal((n_rows, dim))
  w = rng.uniform(0.1, 2.0, size=seg.size)
  dw, T, cnt = wgrad_model(E, G, bounds_of(seg, n_rows), w, combiner)
  np.testing.assert_allclose(dw, chain_autograd(E, G, seg, w, combiner, n_rows), rtol=0, atol=1e-12)
  assert np.all(T >= np.abs(dw) - 1e-12) and np.array_equal(cnt, np.repeat(counts, counts))
