"""CPU-only: tfra_table_fetch_planned_wide and tfra_table_store_rows_wide are declared in the header with their
twins' argument lists, exported by the library that build() makes and bound in `_capi._SIGS_WIDE` with the twins' types; the ABI
version stays 1; the refusals that need no device return the twins' codes behind the new names; the Python surface is there."""
import ctypes
import inspect
import os
import re

import pytest

from tests.test_generic_rows_abi import _Bufs   # the twins' file: an aligned and a misaligned host address, a tfra_row_fields over them

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -6
FETCH, STORE = "tfra_table_fetch_planned_wide", "tfra_table_store_rows_wide"


@pytest.fixture(scope="module")
def built():
  import __graft_entry__
  __graft_entry__.build()
  from tfra_amd import _capi
  return _capi


@pytest.mark.parametrize("name", [FETCH, STORE])
def test_declared_exported_and_bound_as_the_twin(built, name):
  hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read(), flags=re.S)
  args = lambda n: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % n, hdr).group(1)).strip()
  twin = name[:-len("_wide")]
  assert args(name) == args(twin) and re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", hdr)
  assert hasattr(ctypes.CDLL(built.LIB_PATH), name) and built.lib().tfra_abi_version() == 1
  assert built._SIGS_WIDE[name] == built._SIGS[twin] and name not in built._SIGS
  assert getattr(built.lib(), name).restype is ctypes.c_int
  from tfra_amd.dynamic_embedding import table_ops   # the Python surface: a method of its own on the three table classes
  for cls in (table_ops._DeviceTable, table_ops.HkvHashTable, table_ops.CuckooHashTable):
    par = list(inspect.signature(getattr(cls, name[len("tfra_table_"):])).parameters)[1:4]
    assert par == (["plan", "grads", "fields"] if name == FETCH else ["keys", "fields", "count"])


# ---- refusals that are decided before the table or the plan is looked at: the handles below are never dereferenced.
# (call, row fields or the index of a NULL argument, tfra_grads or None, gsum_out, code, words): test_generic_rows_abi.py's cases,
# and the well-formed half gradient.  "a": a 64-byte aligned address, "o": one that is 4-byte aligned only.
HALF = "half gradients are up-cast by the caller"
RECORDS = [(FETCH,) + r for r in [
    (dict(struct_size=40), None, None, INVALID, ""), (dict(n_fields=0), None, None, INVALID, ""), (dict(n_fields=6), None, None, INVALID, ""),
    (dict(n_fields=2, ptrs="aaa"), None, None, INVALID, ""),                  # an entry beyond n_fields
    (dict(n_fields=1, ptrs="o"), None, None, UNSUPPORTED, ""),                # a misaligned field
    ({}, ("a", "TFRA_F32", 0, None), None, INVALID, ""), ({}, None, "a", INVALID, ""),   # gradients and gsum_out go together
    ({}, (None, "TFRA_F32", 0, None), "a", INVALID, ""),                      # the typed calls' record, with their codes
    ({}, ("a", "TFRA_F32", 1, None), "a", INVALID, ""), ({}, ("a", "TFRA_I8", 0, None), "a", INVALID, ""),
    ({}, ("a", "TFRA_F32", 0, "a"), "a", UNSUPPORTED, ""), ({}, ("o", "TFRA_BF16", 0, None), "a", UNSUPPORTED, ""),
    ({}, ("a", "TFRA_F32", 0, None), "o", UNSUPPORTED, ""),
    ({}, ("a", "TFRA_BF16", 0, None), "a", UNSUPPORTED, HALF), ({}, ("a", "TFRA_F16", 0, "a"), "a", UNSUPPORTED, HALF)]
] + [(FETCH, i, None, None, INVALID, ": null argument") for i in (0, 1, 3, 4, 5, 7)] + [   # t, plan, default_row, keys_out, rows_out, d_count
    (STORE, rf, None, None, code, words) for rf, code, words in [
        (0, INVALID, ": null table"), (3, INVALID, ": null buffer"), (4, INVALID, ": null buffer"), (dict(struct_size=56), INVALID, ""),
        (dict(n_fields=0), INVALID, ""), (dict(n_fields=6), INVALID, ""), (dict(n_fields=1, ptrs="aa"), INVALID, ""),
        (dict(n_fields=2, ptrs=[None, "a"]), INVALID, ""), (dict(n_fields=2, ptrs="ao"), UNSUPPORTED, "")]]


@pytest.mark.parametrize("call,rf,g,gsum,code,words", RECORDS)
def test_refused_by_name_with_the_twins_code(built, call, rf, g, gsum, code, words):
  b = _Bufs(built)
  at, a = {"a": b.aligned.value, "o": b.odd.value, None: None}, b.aligned
  kw = dict(rf, ptrs=[at[p] for p in rf["ptrs"]]) if isinstance(rf, dict) and "ptrs" in rf else rf if isinstance(rf, dict) else {}
  grads = ctypes.byref(built.Grads(at[g[0]], getattr(built, g[1]), g[2], at[g[3]])) if g else None
  args = [a, 1, None, a, ctypes.byref(b.fields(**kw)), None] if call == STORE else [a, a, grads, a, a, ctypes.byref(b.fields(**kw)), at[gsum], a, None]
  if not isinstance(rf, dict):
    args[rf] = None
  rc, msg = getattr(built.lib(), call)(*args), built.lib().tfra_last_error().decode()
  assert rc == code and msg.startswith(call + ": ") and words in msg, (rc, msg)


def test_an_empty_store_is_ok(built):
  assert built.lib().tfra_table_store_rows_wide(ctypes.c_void_p(64), 0, None, None, None, None) == 0   # n == 0: nothing is looked at
