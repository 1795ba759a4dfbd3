"""CPU: every argument check of the Python table layer raises its exception type and exact message BEFORE any C call.

The tables here are bare objects on the CPU (`_DeviceTable.__new__`, no handle): a check that reaches the library instead of
raising fails the row (`_capi.call` is replaced by a function that fails the test).  CASES is a literal table with one row for
every `raise` of `_DeviceTable`, `_DeviceTier`, `_score_filter`, `_driver_ids` and `_wide_keys`, and one row per method for each
shared operand check (`_args.py`), so that a method which stops calling the shared check fails here.  Not covered, because they
cannot be reached without a device: `_DeviceTable.__init__`'s default_value check (behind `_as_device`) and `export_all`'s
"table changed during export" (behind the export itself).  The last two tests pin the absence of an import cycle."""
import os
import subprocess
import sys
import types

import pytest
import torch

from tfra_amd import _capi
from tfra_amd.dynamic_embedding import table_ops
from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier

DIM = 4
CPU = torch.device("cpu")


def _table(key_dtype=torch.int64):
  t = _DeviceTable.__new__(_DeviceTable)
  t._key_dtype, t._value_dtype, t._device, t._dim, t._aux_fields = key_dtype, torch.float32, CPU, DIM, 1
  t._default_value, t._h = torch.zeros(DIM), None
  return t


def _tier():
  tier = _DeviceTier.__new__(_DeviceTier)
  tier._upper, tier._lower, tier._max_batch, tier._h = _table(), _table(), 16, None
  return tier


K = torch.tensor([1, 2, 3], dtype=torch.int64)          # 3 keys
K32 = K.to(torch.int32)
V = torch.zeros(3, DIM)                                  # their rows
F64 = torch.zeros(3, DIM, dtype=torch.float64)           # rows of the wrong dtype
SHORT = torch.tensor([7, 7], dtype=torch.int64)          # scores: one entry too few
PLAN = types.SimpleNamespace(_dim=DIM, _device=CPU, n=3, ids=K)
PLAN8 = types.SimpleNamespace(_dim=8, _device=CPU, n=3, ids=K)
PLAN_ELSEWHERE = types.SimpleNamespace(_dim=0, _device=torch.device("cuda:1"), n=3, ids=K)
SEG = torch.tensor([0, 0, 1])
G = torch.zeros(2, DIM)                                  # the gradient of a pooled lookup of 2 rows

KEYS_I64 = "Signature mismatch. Keys must be dtype torch.int64, got torch.int32."
KEYS_I32 = "Signature mismatch. Keys must be dtype torch.int32, got torch.int64."
VALUES_F32 = "Signature mismatch. values must be dtype torch.float32, got torch.float64."
DEFAULT_DTYPE = "default values must be dtype torch.float32, got torch.float64"
DEFAULT_SHORT = "default value needs at least dim=4 elements, got 2"
INIT_DTYPE = "init values must be dtype torch.float32, got torch.float64"
INIT_SHAPE = "init values must be [n, dim] or one row of dim=4 elements, got shape [2]"
OUT = "out must be a contiguous torch.float32 tensor of 3 x 4 elements on cpu"
SCORES = "scores must have one entry per key"
SCORES_PLAN = "scores must have one entry per batch position"
CAP = "cap must be >= 0, got -1"
PLAN_FIT = "the plan was built for dim 8 on cpu"
PRED = "pred must be 'ge' or 'lt', got 'gt'"

# (target, method, args, kwargs, exception type, exact message).  target: "table" — a bare int64-key table; "table32" — a bare
# int32-key one; "tier" — a bare tier over two int64-key tables; "fn" — the function of that name in table_ops.
CASES = [
    # ---- the marshalling functions
    ("fn", "_wide_keys", (torch.zeros(3),), {}, TypeError, "keys must be torch.int64 or torch.int32, got torch.float32"),
    ("fn", "_driver_ids", (_table(torch.int32), K, CPU), {}, TypeError, KEYS_I32),
    ("fn", "_score_filter", (0, "gt"), {}, ValueError, PRED),
    ("fn", "_score_filter", ("x", "ge"), {}, ValueError, "threshold must be an integer in [0, 2^64), got 'x'"),
    ("fn", "_score_filter", (-1, "ge"), {}, ValueError, "threshold must be in [0, 2^64), got -1"),
    # ---- the constructor, ahead of the device
    ("fn", "_DeviceTable", (torch.float32, torch.float32, 0.0, "t", "cuda:0"), {}, TypeError,
     "key_dtype must be torch.int64 or torch.int32 on GPU tables, got torch.float32"),
    ("fn", "_DeviceTable", (torch.int64, torch.bool, 0.0, "t", "cuda:0"), {}, TypeError, "unsupported value_dtype torch.bool"),
    # ---- keys: the table's dtype only (an int32-key table raises before the widen call)
    ("table", "find", (K32,), {}, TypeError, KEYS_I64),
    ("table32", "find", (K,), {}, TypeError, KEYS_I32),
    ("table", "erase", (K32,), {}, TypeError, KEYS_I64),
    ("table", "contains", (K32,), {}, TypeError, KEYS_I64),
    ("table", "find_n", (K32, None), {}, TypeError, KEYS_I64),
    ("tier", "find", (K32,), {}, TypeError, KEYS_I64),
    ("tier", "find_or_insert", (K32,), {}, TypeError, KEYS_I64),
    ("tier", "insert", (K32, V), {}, TypeError, KEYS_I64),
    # ---- values: dtype and shape
    ("table", "upsert", (K, F64), {}, TypeError, VALUES_F32),
    ("table", "upsert", (K, torch.zeros(3, 5)), {}, ValueError, "Expected shape [3, 4] for values, got [3, 5]"),
    ("table", "upsert_and_evict", (K, F64), {}, TypeError, VALUES_F32),
    ("table", "assign", (K, F64), {}, TypeError, VALUES_F32),
    ("table", "upsert_n", (K, None, F64), {}, TypeError, VALUES_F32),
    ("table", "upsert_sparse", (K, F64), {}, TypeError, VALUES_F32),
    ("table", "accum_or_assign", (K, F64, torch.ones(3, dtype=torch.bool)), {}, TypeError,
     "Signature mismatch. values_or_deltas must be dtype torch.float32, got torch.float64."),
    ("tier", "insert", (K, torch.zeros(3, 5)), {}, ValueError, "Expected shape [3, 4] for values, got [3, 5]"),
    ("table", "upsert_and_evict", (K, [[0.0] * 8] * 3), {"whole_rows_in": True}, TypeError,
     "Signature mismatch. values must be a torch.float32 tensor."),
    ("table", "upsert_and_evict", (K, V), {"whole_rows_in": True}, ValueError,
     "Expected shape [3, 8] for whole-row values, got [3, 4]"),
    ("table", "upsert_planned", (PLAN, F64), {}, ValueError, "Expected torch.float32 values of shape [3, 4]"),
    # ---- the default rows of the find family: full, or at least dim elements
    ("table", "find", (K, F64), {}, TypeError, DEFAULT_DTYPE),
    ("table", "find", (K, torch.zeros(2)), {}, ValueError, DEFAULT_SHORT),
    ("table", "find_unique", (K, F64), {}, TypeError, DEFAULT_DTYPE),
    ("table", "find_unique", (K, torch.zeros(2)), {}, ValueError, DEFAULT_SHORT),
    ("table", "find_missed", (K, F64), {}, TypeError, DEFAULT_DTYPE),
    ("table", "find_missed", (K, torch.zeros(2)), {}, ValueError, DEFAULT_SHORT),
    # ---- the rows of the admitting family: [n, dim] or exactly one row
    ("table", "find_or_insert", (K, F64), {}, TypeError, INIT_DTYPE),
    ("table", "find_or_insert", (K, torch.zeros(2)), {}, ValueError, INIT_SHAPE),
    ("table", "find_or_insert", (K, torch.zeros(2, DIM)), {}, ValueError,
     "init values must be [n, dim] or one row of dim=4 elements, got shape [2, 4]"),
    ("table", "find_or_insert_planned", (PLAN, F64), {}, TypeError, INIT_DTYPE),
    ("table", "find_or_insert_planned", (PLAN, torch.zeros(2)), {}, ValueError, INIT_SHAPE),
    ("tier", "find", (K, F64), {}, TypeError, DEFAULT_DTYPE),
    ("tier", "find", (K, torch.zeros(2)), {}, ValueError, "default values must be [n, dim] or one row of dim=4 elements, got shape [2]"),
    ("tier", "find_or_insert", (K, F64), {}, TypeError, INIT_DTYPE),
    ("tier", "find_or_insert", (K, torch.zeros(2)), {}, ValueError, INIT_SHAPE),
    # ---- out=
    ("table", "find_or_insert", (K,), {"out": torch.zeros(2, DIM)}, ValueError, OUT),
    ("table", "find_or_insert", (K,), {"out": F64}, ValueError, OUT),
    ("table", "find_or_insert", (K,), {"out": torch.zeros(DIM, 3).t()}, ValueError, OUT),
    ("table", "find_or_insert_planned", (PLAN,), {"out": torch.zeros(2, DIM)}, ValueError, OUT),
    ("tier", "find", (K,), {"out": torch.zeros(2, DIM)}, ValueError, OUT),
    ("tier", "find_or_insert", (K,), {"out": torch.zeros(2, DIM)}, ValueError, OUT),
    # ---- scores: one entry per key (a plan: per batch position)
    ("table", "upsert", (K, V), {"scores": SHORT}, ValueError, SCORES),
    ("table", "upsert_and_evict", (K, V), {"scores": SHORT}, ValueError, SCORES),
    ("table", "find_or_insert", (K,), {"scores": SHORT}, ValueError, SCORES),
    ("table", "find_or_insert_planned", (PLAN,), {"scores": SHORT}, ValueError, SCORES_PLAN),
    ("table", "assign", (K, V), {"scores": SHORT}, ValueError, SCORES),
    ("table", "upsert_n", (K, None, V), {"scores": SHORT}, ValueError, SCORES),                                     # new
    ("table", "upsert_sparse", (K, V), {"scores": SHORT}, ValueError, SCORES),                                      # new
    ("table", "upsert_planned", (PLAN, V), {"scores": SHORT}, ValueError, SCORES_PLAN),                             # new
    ("table", "accum_or_assign", (K, V, torch.ones(3, dtype=torch.bool)), {"scores": SHORT}, ValueError, SCORES),   # new
    # ---- cap
    ("table", "upsert_and_evict", (K, V), {"cap": -1}, ValueError, CAP),
    ("table", "find_missed", (K,), {"cap": -1}, ValueError, CAP),
    # ---- plans
    ("table", "find_or_insert_planned", (PLAN8,), {}, ValueError, PLAN_FIT),
    ("table", "apply_planned", (None, PLAN8, V, torch.zeros(DIM)), {}, ValueError, PLAN_FIT),
    ("table", "apply_planned_combined", (None, PLAN8, G, SEG, None, 0, torch.zeros(DIM)), {}, ValueError, PLAN_FIT),
    ("table", "upsert_planned", (PLAN_ELSEWHERE, V), {}, ValueError, "the plan lives on cuda:1"),
    # ---- accum_or_assign's exists
    ("table", "accum_or_assign", (K, V, torch.ones(3)), {}, TypeError, "exists must be a bool tensor"),
    ("table", "accum_or_assign", (K, V, torch.ones(2, dtype=torch.bool)), {}, ValueError,
     "exists must have the same number of elements as keys"),
    # ---- the pooled lookups
    ("table", "find_combine", (K, SEG[:2], None, 0, 2), {}, ValueError,
     "ids and segment_ids must have the same number of elements: 3 vs 2"),
    ("table", "find_combine", (K, SEG, torch.ones(2), 0, 2), {}, ValueError, "weights must have one element per id"),
    ("table", "find_combine", (K, SEG, None, 0, 2, torch.zeros(DIM, dtype=torch.float64)), {}, TypeError, DEFAULT_DTYPE),
    ("table", "find_combine", (K, SEG, None, 0, 2, torch.zeros(2)), {}, ValueError,
     "default_row must be one row of dim=4 elements, got 2"),
    ("table", "find_combine_ragged", (torch.tensor([0.0, 3.0]), K, None, 0), {}, TypeError,
     "row_splits must be int32 or int64, got torch.float32"),
    ("table", "find_combine_ragged", (torch.empty(0, dtype=torch.int64), K, None, 0), {}, ValueError,
     "row_splits needs n_rows + 1 >= 1 elements"),
    ("table", "find_combine_ragged", (torch.tensor([0, 3]), K, torch.ones(2), 0), {}, ValueError,
     "weights must have one element per id"),
    ("table", "find_combine_weight_grad", (K, SEG, None, 0, torch.zeros(2, 5)), {}, ValueError,
     "grad_out must be [n_rows, 4] (the lookup's result), got [2, 5]"),
    ("table", "find_combine_ragged_weight_grad", (torch.tensor([0, 3]), K, None, 0, G), {}, ValueError,
     "grad_out must be [1, 4] (the lookup's result), got [2, 4]"),
    # ---- the write-backs' gradients
    ("table", "apply_optimizer", (None, K, torch.zeros(3, 5), torch.zeros(DIM)), {}, ValueError,
     "Expected shape [3, 4] for grads, got [3, 5]"),
    ("table", "apply_sparse", (None, K, torch.zeros(3, 5), torch.zeros(DIM)), {}, ValueError,
     "Expected shape [3, 4] for grads, got [3, 5]"),
    ("table", "apply_planned", (None, PLAN, G, torch.zeros(DIM)), {}, ValueError, "Expected shape [3, 4] for grads, got [2, 4]"),
    ("table", "apply_planned_combined", (None, PLAN, torch.zeros(2, 5), SEG, None, 0, torch.zeros(DIM)), {}, ValueError,
     "Expected grad_out of shape [n_rows, 4], got [2, 5]"),
    ("table", "apply_planned_combined", (None, PLAN, G, SEG[:2], None, 0, torch.zeros(DIM)), {}, ValueError,
     "seg / weights need one element per plan entry (3)"),
    ("table", "apply_planned_combined", (None, PLAN, G, SEG, torch.ones(2), 0, torch.zeros(DIM)), {}, ValueError,
     "seg / weights need one element per plan entry (3)"),
    # ---- the score-filtered scans
    ("table", "count_if", (0, "gt"), {}, ValueError, PRED),
    ("table", "export_if", (0, "gt"), {}, ValueError, PRED),
    ("table", "erase_if", (0, "gt"), {}, ValueError, PRED),
    ("table", "save_if", ("prefix", 0, "gt"), {}, ValueError, PRED),
]


@pytest.fixture(autouse=True)
def _no_c_call(monkeypatch):
  def call(name, *args):
    pytest.fail("reached the C call %s: the check must raise before it" % name)
  monkeypatch.setattr(_capi, "call", call)


def _target(name):
  return {"table": _table, "table32": lambda: _table(torch.int32), "tier": _tier, "fn": lambda: table_ops}[name]()


@pytest.mark.parametrize("case", CASES, ids=["%02d-%s.%s" % (i, c[0], c[1]) for i, c in enumerate(CASES)])
def test_check_raises_before_the_c_call(case):
  target, method, args, kwargs, exc, message = case
  with pytest.raises(exc) as info:
    getattr(_target(target), method)(*args, **kwargs)
  assert type(info.value) is exc and str(info.value) == message


def test_empty_int32_keys_launch_nothing():
  t = _table(torch.int32)
  none = torch.empty(0, dtype=torch.int32)
  rows, exists = t.find(none, return_exists=True)
  assert tuple(rows.shape) == (0, DIM) and rows.dtype == torch.float32 and tuple(exists.shape) == (0,)
  assert t.upsert(none, torch.zeros(0, DIM)) is None
  assert tuple(t.contains(none).shape) == (0,) and t.erase(none) is None
  assert tuple(t.find_or_insert(none).shape) == (0, DIM)
  assert t.assign(none, torch.zeros(0, DIM), return_found=True).numel() == 0


def test_empty_scores_are_no_scores():
  # (an empty tensor means "no scores" for every writer; with no keys nothing is launched)
  t, none = _table(), torch.empty(0, dtype=torch.int64)
  assert t.upsert_n(none, None, torch.zeros(0, DIM), scores=none) is None
  assert t.assign(none, torch.zeros(0, DIM), scores=none) is None


@pytest.mark.parametrize("first", ["_args", "device_ops", "table_ops", "variable", "optimizer", "distributed"])
def test_package_imports_with_any_module_first(first):
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  code = "import sys; sys.path.insert(0, %r); import tfra_amd.dynamic_embedding.%s; import tfra_amd.dynamic_embedding" % (
      os.path.join(root, "recommenders-addons_amd"), first)
  subprocess.run([sys.executable, "-c", code], check=True)


def test_table_ops_uses_device_ops_workspace_itself():
  from tfra_amd.dynamic_embedding import device_ops
  assert table_ops._workspace is device_ops._workspace     # (no call-time wrapper: device_ops no longer imports table_ops)
