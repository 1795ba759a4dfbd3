"""CPU-only: the ragged pooled lookup's C entries (tfra_table_find_combine_ragged, tfra_multi_find_combine_ragged), their flag
macros and descriptor are declared in the header, exported by the library that build() makes and bound in the ctypes layer with
the header's argument lists and field order; the ABI version is unchanged (additive); the Python surface is there.

Also here: `ragged_model`, a float64 NumPy model of the ragged safe semantics (row_splits clamp, prune, fill, sum / mean /
sqrtn), pinned to hand-computed cases.  tests/test_gpu_ragged_lookup.py imports it."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = "tfra_table_find_combine_ragged"
MANY = "tfra_multi_find_combine_ragged"
FIELDS = ["struct_size", "combiner", "table", "n_rows", "row_splits", "nnz", "ids", "weights", "flags", "reserved", "fill_id",
          "default_row", "out"]


# ---- the model -------------------------------------------------------------------------------------------------------------------
def ragged_bounds(row_splits, nnz):
  """[(b, e)] per row: b = clamp(row_splits[r], 0, nnz), e = clamp(row_splits[r + 1], b, nnz)."""
  rs = [int(x) for x in row_splits]
  out = []
  for r in range(len(rs) - 1):
    b = min(max(rs[r], 0), nnz)
    e = min(max(rs[r + 1], b), nnz)
    out.append((b, e))
  return out


def ragged_model(row_splits, nnz, E, w, combiner, prune=False, fill_row=None):
  """float64.  E [>= nnz, dim]: the embedding of each entry; w [>= nnz] or None (all 1); combiner "sum" / "mean" / "sqrtn".
  prune (ignored when w is None): entry p is a member only if w[p] > 0 (a NaN weight is no member).  fill_row [dim] or None: what
  a row without members yields (None: zeros).  Returns (out [n_rows, dim], den [n_rows], amp [n_rows]): den = the combiner's
  denominator over the members (1 for sum), amp = sum |w| over them."""
  E = np.asarray(E, np.float64)
  dim = E.shape[1]
  bounds = ragged_bounds(row_splits, nnz)
  out = np.zeros((len(bounds), dim))
  den = np.ones(len(bounds))
  amp = np.zeros(len(bounds))
  for r, (b, e) in enumerate(bounds):
    members = [p for p in range(b, e) if w is None or not prune or w[p] > 0]
    if not members:
      if fill_row is not None:
        out[r] = np.asarray(fill_row, np.float64)
      continue
    ww = np.ones(len(members)) if w is None else np.asarray([w[p] for p in members], np.float64)
    acc = (E[members] * ww[:, None]).sum(0)
    amp[r] = np.abs(ww).sum()
    if combiner == "sum":
      out[r] = acc
      continue
    d = ww.sum() if combiner == "mean" else np.sqrt((ww * ww).sum())
    den[r] = d
    if np.isnan(d):
      out[r] = np.nan
    elif d != 0:
      out[r] = acc / d
  return out, den, amp


# ---- the model against hand-computed cases ---------------------------------------------------------------------------------------
def _params():
  return np.array([[float(i), 10.0 * i] for i in range(10)])   # params[i] = (i, 10 i); a miss: (-7, -70)


MISS = np.array([-7.0, -70.0])


def _E(ids):
  P = _params()
  return np.array([P[i] if 0 <= i < 10 else MISS for i in ids])


@pytest.mark.parametrize("default_id", [0, None])
def test_model_on_the_reference_docstring_example(default_id):
  # PY/ragged_embedding_ops.py:385-402: [0,0] id 1 w 2.0; [0,1] id 3 w 0.5; [1,0] id -1 w 1.0; [2,3] id 1 w 3.0, combiner mean.
  # ids are never pruned here (any int64 is a key): id -1 is looked up and misses
  ids, w, rs = [1, 3, -1, 1], np.array([2.0, 0.5, 1.0, 3.0]), [0, 2, 3, 4]
  P = _params()
  fill = None if default_id is None else P[default_id]
  out, den, amp = ragged_model(rs, 4, _E(ids), w, "mean", prune=True, fill_row=fill)
  np.testing.assert_allclose(out[0], (P[1] * 2.0 + P[3] * 0.5) / 2.5, rtol=1e-15)
  np.testing.assert_allclose(out[0], [1.4, 14.0], rtol=1e-15)
  np.testing.assert_array_equal(out[1], MISS)
  np.testing.assert_array_equal(out[2], P[1])
  np.testing.assert_array_equal(den, [2.5, 1.0, 3.0])
  # the docstring's own reading — entry [1,0] gone (there: an invalid id; here: a weight that is not > 0) — fills row 1
  w2 = np.array([2.0, 0.5, 0.0, 3.0])
  out, _, _ = ragged_model(rs, 4, _E(ids), w2, "mean", prune=True, fill_row=fill)
  np.testing.assert_array_equal(out[1], P[0] if default_id is not None else [0.0, 0.0])
  np.testing.assert_array_equal(out[2], P[1])


def test_model_on_the_reference_fill_empty_rows_case():
  # T/ragged_embedding_ops_test.py:9-22: [[1, 2, 3], [], [4], [], [5, 6]], default_id 0 -> [[1, 2, 3], [0], [4], [0], [5, 6]],
  # is_row_empty [F, T, F, T, F]
  ids, rs = [1, 2, 3, 4, 5, 6], [0, 3, 3, 4, 4, 6]
  P = _params()
  out, _, _ = ragged_model(rs, 6, _E(ids), None, "sum", fill_row=P[0] + 0.5)
  np.testing.assert_array_equal(out, [P[1] + P[2] + P[3], P[0] + 0.5, P[4], P[0] + 0.5, P[5] + P[6]])
  empty = [b == e for b, e in ragged_bounds(rs, 6)]
  assert empty == [False, True, False, True, False]
  out, _, _ = ragged_model(rs, 6, _E(ids), None, "mean")
  np.testing.assert_array_equal(out[1], [0.0, 0.0])
  np.testing.assert_array_equal(out[4], (P[5] + P[6]) / 2)


def test_model_prunes_non_positive_and_nan_weights():
  ids = [1, 2, 3, 4, 5, 6, 7]
  w = np.array([0.0, -1.0, -0.0, 2.0, np.nan, 4.0, 3.0])
  rs = [0, 3, 6, 7]             # row 0: every weight <= 0; row 1: 2.0, NaN, 4.0; row 2: 3.0
  P = _params()
  out, den, _ = ragged_model(rs, 7, _E(ids), w, "sqrtn", prune=True, fill_row=P[9])
  np.testing.assert_array_equal(out[0], P[9])                                    # no member: the fill row
  np.testing.assert_allclose(out[1], (2.0 * P[4] + 4.0 * P[6]) / np.sqrt(20.0), rtol=1e-15)   # the NaN weight is no member
  np.testing.assert_array_equal(out[2], P[7])
  out, _, _ = ragged_model(rs, 7, _E(ids), w, "sqrtn", prune=True)
  np.testing.assert_array_equal(out[0], [0.0, 0.0])                              # no fill: zeros
  # sum never prunes (the caller does not set the flag): the NaN weight reaches the result, -1 counts
  out, _, _ = ragged_model(rs, 7, _E(ids), w, "sum", prune=False, fill_row=P[9])
  np.testing.assert_array_equal(out[0], -P[2])
  assert np.isnan(out[1]).all()
  # without prune a mean over weights that sum to 0 is zeros, and the row is not empty: no fill
  out, _, _ = ragged_model([0, 2], 2, _E([1, 2]), np.array([1.0, -1.0]), "mean", fill_row=P[9])
  np.testing.assert_array_equal(out[0], [0.0, 0.0])
  # prune is ignored without weights
  out, _, _ = ragged_model([0, 2], 2, _E([1, 2]), None, "mean", prune=True)
  np.testing.assert_array_equal(out[0], (P[1] + P[2]) / 2)


def test_model_clamps_row_splits():
  assert ragged_bounds([-3, 2, 1, 5, 9, 4], 6) == [(0, 2), (2, 2), (1, 5), (5, 6), (6, 6)]
  assert ragged_bounds([7, 8], 6) == [(6, 6)]
  ids = [1, 2, 3, 4, 5, 6, 7, 8]
  P = _params()
  out, _, _ = ragged_model([-3, 2, 1, 5, 9, 4], 6, _E(ids), None, "sum", fill_row=MISS)
  np.testing.assert_array_equal(out, [P[1] + P[2], MISS, P[2] + P[3] + P[4] + P[5], P[6], MISS])   # entries 6, 7 are in no row


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


def _header():
  return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)


def _names(decls, sep):
  return [re.split(r"[\s\*]+", a.strip())[-1] for a in decls.replace("\n", " ").split(sep) if a.strip()]


def test_header_declares_the_calls_the_flags_and_the_descriptor():
  hdr = _header()
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % SINGLE, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % SINGLE
  assert _names(m.group(1), ",") == ["t", "n_rows", "row_splits", "nnz", "ids", "weights", "combiner", "flags", "fill_id",
                                     "default_row", "out", "stream"]
  m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % MANY, hdr)
  assert m, "include/tfra_mi355x.h does not declare %s" % MANY
  assert _names(m.group(1), ",") == ["ws", "n_tables", "descs", "launches_out", "stream"]
  assert re.search(r"#define\s+TFRA_RAGGED_PRUNE\s+1u\b", hdr) and re.search(r"#define\s+TFRA_RAGGED_FILL\s+2u\b", hdr)
  s = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*tfra_find_combine_ragged_desc\s*;", hdr)
  assert s, "include/tfra_mi355x.h does not declare tfra_find_combine_ragged_desc"
  assert _names(s.group(1), ";") == FIELDS


def test_library_exports_them_and_the_abi_version_stays(built):
  lib = ctypes.CDLL(built.LIB_PATH)
  assert hasattr(lib, SINGLE) and hasattr(lib, MANY)
  assert built.lib().tfra_abi_version() == 1


def test_bindings_have_the_headers_signatures_and_layout(built):
  P, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
  assert built._SIGS.get(SINGLE) == [P, SZ, P, SZ, P, P, I, ctypes.c_uint32, ctypes.c_int64, P, P, P]
  assert built._SIGS.get(MANY) == [P, SZ, P, P, P]
  assert getattr(built.lib(), SINGLE).restype is ctypes.c_int and getattr(built.lib(), MANY).restype is ctypes.c_int
  assert (built.RAGGED_PRUNE, built.RAGGED_FILL) == (1, 2)
  d = built.FindCombineRaggedDesc
  assert [f[0] for f in d._fields_] == FIELDS
  assert [f[1] for f in d._fields_] == [ctypes.c_uint32, ctypes.c_int32, P, SZ, P, SZ, P, P, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_int64, P, P]
  # the C struct's layout on LP64
  assert ctypes.sizeof(d) == 88
  assert [getattr(d, f).offset for f in FIELDS] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80]


def test_python_surface_is_present():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops
  assert callable(getattr(table_ops, "find_combine_ragged_many", None))
  assert callable(getattr(table_ops._DeviceTable, "find_combine_ragged", None))
  assert callable(getattr(de.Variable, "lookup_combined_ragged", None))
  for name in ("embedding_lookup_sparse", "safe_embedding_lookup_sparse", "embedding_lookup_sparse_many",
               "safe_embedding_lookup_sparse_many"):
    assert callable(getattr(de.ragged_embedding_ops, name, None)), name
