"""KV-table wrappers: `CuckooHashTable` / `HkvHashTable` with the reference's method surface.

Mirrors PY/cuckoo_hashtable_ops.py:45-575 and PY/hkv_hashtable_ops.py:47-560
(PY = /root/reference/tensorflow_recommenders_addons/dynamic_embedding/python/ops): same
constructor arguments, same methods (`size, lookup, insert, accum, remove, clear, export,
save_to_file_system, load_from_file_system`; Hkv adds `export_with_scores,
export_keys_and_scores`), same argument meaning and error behaviour.  Tensors are torch
tensors on the table's MI355X; every method is one call through the C ABI
(include/tfra_mi355x.h) on torch's current HIP stream — no per-op host sync (the reference
syncs 1-3x per op, R/kernels/hkv_hashtable_op_gpu.cu.cc:192-213).

In the reference `CuckooHashTable` on a GPU device silently issues the Hkv ops
(PY/cuckoo_hashtable_ops.py:153-165,309-338); here both classes are the same HIP engine:
`CuckooHashTable` = unbounded, growing, never-evicting flavour (libcuckoo semantics),
`HkvHashTable` = bounded `max_capacity` flavour with scores.
"""
import ctypes
import enum
import os
import sys

import torch

from .. import _capi
from ._args import (_TORCH2DT, _admitted_rows, _as_device, _as_tensor, _cap_for, _check_plan, _default_rows, _driver_ids, _grads_arg,
                    _narrow_keys, _out_dtype, _out_rows, _over_plans, _ptr, _rows_on, _rows_out, _score_filter, _scores_for, _stream,
                    _trim_to_count, _wide_keys)
from .device_ops import _workspace

KHkvHashTableInitCapacity = 1024 * 1024  # PY/hkv_hashtable_ops.py:40-44
KHkvHashTableMaxCapacity = 1024 * 1024
KHkvHashTableMaxHbmForValuesByBytes = 1024 * 1024 * 1024


class HkvEvictStrategy(enum.IntEnum):
  """PY/dynamic_embedding_creator.py:141-146"""
  LRU = 0
  LFU = 1
  EPOCHLRU = 2
  EPOCHLFU = 3
  CUSTOMIZED = 4


class _DeviceTable:
  """Owns one tfra_table_t and exposes the table ops on torch tensors."""

  def __init__(self, key_dtype, value_dtype, default_value, name, device, dim=None, aux_fields=0,
               init_capacity=0, max_capacity=0, max_hbm_for_values=0, strategy=-1, step_per_epoch=0,
               reserved_key_start_bit=0, max_load_factor=0.0, aux_init=(0.0, 0.0, 0.0, 0.0)):
    if key_dtype not in (torch.int64, torch.int32):
      # GPU ops: K = int64 (R/kernels/hkv_hashtable_op_gpu.cu.cc:1133-1138) and, for the cuckoo ops, (int32, float)
      # (R/kernels/cuckoo_hashtable_op_gpu.cu.cc:1058).  The engine's keys are int64: int32 keys are widened on the device in
      # front of every call (tfra_keys_widen_i32), exports narrow them, and the key files hold 4-byte keys like the reference's.
      raise TypeError("key_dtype must be torch.int64 or torch.int32 on GPU tables, got %s" % key_dtype)
    if value_dtype not in _TORCH2DT:
      raise TypeError("unsupported value_dtype %s" % value_dtype)
    self._key_dtype = key_dtype
    self._value_dtype = value_dtype
    self._device = _as_device(device)
    self._name = name
    self.stochastic_rounding = 0   # the seed of set_stochastic_rounding (0: off)
    dv = torch.as_tensor(default_value, dtype=value_dtype).reshape(-1)
    if dim is None:
      dim = dv.numel()
    elif dv.numel() == 1 and dim != 1:
      dv = dv.repeat(dim)
    if dv.numel() != dim:
      raise ValueError("default_value must be a vector of dim %d, got shape %s" % (dim, tuple(dv.shape)))
    self._dim = int(dim)
    self._default_value = dv.to(self._device).contiguous()
    o = _capi.TableOpts()
    o.struct_size = ctypes.sizeof(_capi.TableOpts)
    o.value_dtype = _TORCH2DT[value_dtype]
    o.dim = self._dim
    o.aux_fields = aux_fields
    o.init_capacity = int(init_capacity)
    o.max_capacity = int(max_capacity)
    o.max_hbm_for_vectors = int(max_hbm_for_values)
    o.max_load_factor = float(max_load_factor)
    o.strategy = int(strategy)
    o.step_per_epoch = int(step_per_epoch)
    o.reserved_key_start_bit = int(reserved_key_start_bit)
    o.device = self._device.index
    for i in range(4):
      o.aux_init[i] = float(aux_init[i]) if i < len(aux_init) else 0.0
    self._aux_fields = aux_fields
    h = ctypes.c_void_p()
    _capi.call("tfra_table_create", ctypes.byref(o), None, ctypes.byref(h))
    self._h = h
    if key_dtype == torch.int32:
      _capi.call("tfra_table_set_option", self._h, _capi.OPTION_KEY_BYTES_ON_DISK, 4)

  def __del__(self):
    h = getattr(self, "_h", None)
    if h:
      try:
        _capi.lib().tfra_table_destroy(h)
      except Exception:  # interpreter shutdown
        pass
      self._h = None

  # ---- helpers -----------------------------------------------------------------------------
  @property
  def dim(self):
    return self._dim

  @property
  def device(self):
    return self._device

  @property
  def key_dtype(self):
    return self._key_dtype

  @property
  def value_dtype(self):
    return self._value_dtype

  def _keys(self, keys):
    keys = _as_tensor(keys, self._device)
    if keys.dtype != self._key_dtype:
      raise TypeError("Signature mismatch. Keys must be dtype %s, got %s." % (self._key_dtype, keys.dtype))
    return _wide_keys(keys.to(self._device))   # the engine's keys are int64

  def _values_for(self, keys, values, what="values"):
    values = _as_tensor(values, self._device)
    if values.dtype != self._value_dtype:
      raise TypeError("Signature mismatch. %s must be dtype %s, got %s." % (what, self._value_dtype, values.dtype))
    want = tuple(keys.shape) + (self._dim,)
    if tuple(values.shape) != want:
      # CheckKeyAndValueTensorsForInsert (R/kernels/cuckoo_hashtable_op.cc:640-660), KAT K6
      raise ValueError("Expected shape %s for %s, got %s" % (list(want), what, list(values.shape)))
    return values.to(self._device).contiguous()

  # the rows and out= operands of this table's lookups (None: the table's default row), by `_args`' rules -> (rows, is_full) / out
  def _defaults(self, rows, n):
    return _default_rows(self._value_dtype, self._dim, self._device, self._default_value if rows is None else rows, n * self._dim)

  def _init_rows(self, rows, n, what="init values"):
    return _admitted_rows(self._value_dtype, self._dim, self._device, self._default_value if rows is None else rows, n, what)

  def _out(self, shape, out):
    return _out_rows(self._value_dtype, self._dim, self._device, shape, out)

  # ---- ops ---------------------------------------------------------------------------------
  def find(self, keys, dynamic_default_values=None, return_exists=False, field=0, out_dtype=None):
    """out_dtype (field 0 only): the rows in float32 / float16 / bfloat16 instead of the value dtype, converted in the lookup's
    kernel (tfra_table_find_typed): bit for bit `find(...).to(out_dtype)`.  The default rows stay in the value dtype."""
    keys = self._keys(keys)
    n = keys.numel()
    d, full = self._defaults(dynamic_default_values, n)
    if _out_dtype(out_dtype) is not None and field:
      raise ValueError("out_dtype serves field 0 only")
    out = torch.empty(tuple(keys.shape) + (self._dim,), dtype=out_dtype or self._value_dtype, device=self._device)
    exists = torch.empty(keys.shape, dtype=torch.bool, device=self._device) if return_exists else None
    if n:
      if out_dtype is not None:
        ro = _rows_out(out)
        _capi.call("tfra_table_find_typed", self._h, n, None, _ptr(keys), ctypes.byref(ro), _ptr(exists), _ptr(d), full,
                   _stream(self._device))
      elif field:
        _capi.call("tfra_table_find_field", self._h, field, n, _ptr(keys), _ptr(out), _ptr(exists), _ptr(d), full,
                   _stream(self._device))
      else:
        _capi.call("tfra_table_find", self._h, n, _ptr(keys), _ptr(out), _ptr(exists), _ptr(d), full,
                   _stream(self._device))
    return (out, exists) if return_exists else out

  def find_unique(self, keys, dynamic_default_values=None, return_exists=False):
    """find(keys) and the de-duplication of the same keys in ONE launch (tfra_table_find_unique: the forward half of embedding_lookup
    as the fused TF op issues it): returns (rows [n, dim], unique [n] — the first `count` entries are the distinct keys, in no
    particular order —, idx [n] int32 with unique[idx] == keys, count: device int64 scalar[, exists]).  Nothing is read on the host."""
    keys = self._keys(keys).reshape(-1)
    n = keys.numel()
    d, full = self._defaults(dynamic_default_values, n)
    out = torch.empty((n, self._dim), dtype=self._value_dtype, device=self._device)
    exists = torch.empty(n, dtype=torch.bool, device=self._device) if return_exists else None
    uniq = torch.empty(n, dtype=torch.int64, device=self._device)
    idx = torch.empty(n, dtype=torch.int32, device=self._device)
    cnt = torch.zeros((), dtype=torch.int64, device=self._device)
    _capi.call("tfra_table_find_unique", self._h, _workspace(self._device), n, _ptr(keys), _ptr(out), _ptr(exists), _ptr(d), full,
               _ptr(uniq), _ptr(idx), _ptr(cnt), _stream(self._device))
    uniq = _narrow_keys(uniq, self._key_dtype)   # the table's key dtype, so that `unique` goes back into upsert / erase
    return (out, uniq, idx, cnt, exists) if return_exists else (out, uniq, idx, cnt)

  def _pooled_operands(self, nnz, weights, default_row):
    """The weights (float32 [nnz], or None) and the default row (one row of the value dtype, the table's when None) of a pooled
    lookup, checked and on the table's device: what the tuple and the ragged form share behind their own ids / rows checks."""
    w = None
    if weights is not None:
      w = torch.as_tensor(weights, device=self._device).reshape(-1).to(torch.float32).contiguous()
      if w.numel() != nnz:
        raise ValueError("weights must have one element per id")
    d = self._default_value if default_row is None else torch.as_tensor(default_row, device=self._device)
    if d.dtype != self._value_dtype:
      raise TypeError("default values must be dtype %s, got %s" % (self._value_dtype, d.dtype))
    if d.numel() != self._dim:
      raise ValueError("default_row must be one row of dim=%d elements, got %d" % (self._dim, d.numel()))
    d = d.contiguous()
    return w, d

  def _find_combine_args(self, ids, seg, weights, n_rows, default_row, out_dtype=None):
    """The arguments of one pooled lookup as the C calls read them: (ids, seg, weights or None, default row, out), checked and on
    the table's device (find_combine and find_combine_many share it).  out: float32, or `out_dtype` (the typed calls)."""
    ids = self._keys(ids).reshape(-1)
    nnz = ids.numel()
    seg = torch.as_tensor(seg, device=self._device).reshape(-1).to(torch.int64).contiguous()
    if seg.numel() != nnz:
      raise ValueError("ids and segment_ids must have the same number of elements: %d vs %d" % (nnz, seg.numel()))
    w, d = self._pooled_operands(nnz, weights, default_row)
    out = torch.empty((int(n_rows), self._dim), dtype=_out_dtype(out_dtype) or torch.float32, device=self._device)
    return ids, seg, w, d, out

  def find_combine(self, ids, seg, weights, combiner, n_rows, default_row=None):
    """`find_combine_typed` with the call's own output type, float32 (tfra_table_find_combine)."""
    return self.find_combine_typed(ids, seg, weights, combiner, n_rows, default_row)

  def find_combine_typed(self, ids, seg, weights, combiner, n_rows, default_row=None, out_dtype=None):
    """The pooled lookup (tfra_table_find_combine): out[r] = combine over {p: seg[p] == r}, in input order, of weights[p] * (the row
    of ids[p], or `default_row` — one row of the value dtype, the table's default when None — on a miss), float32 [n_rows, dim].
    seg ascending int64, weights float32 or None (all 1), combiner 0 sum / 1 mean / 2 sqrtn.  float32 / float16 / bfloat16 rows,
    dim % 4 == 0, dim <= 256 (TfraError UNSUPPORTED otherwise).  Bit-identical to find + device_ops.sparse_segment_combine over
    idx = arange(nnz); no unique pass, nothing read on the host.  out_dtype: the result in float32 / float16 / bfloat16, rounded
    in the lookup's kernel (tfra_table_find_combine_typed): bit for bit `find_combine(...).to(out_dtype)`; None: `find_combine`.
    (A method beside `find_combine`, whose parameter list the tiered owners mirror and stays as it is.)"""
    ids, seg, w, d, out = self._find_combine_args(ids, seg, weights, n_rows, default_row, out_dtype)
    if out_dtype is not None:
      ro = _rows_out(out)
      _capi.call("tfra_table_find_combine_typed", self._h, _workspace(self._device), ids.numel(), _ptr(ids), _ptr(seg), _ptr(w),
                 int(combiner), int(n_rows), _ptr(d), ctypes.byref(ro), _stream(self._device))
      return out
    _capi.call("tfra_table_find_combine", self._h, _workspace(self._device), ids.numel(), _ptr(ids), _ptr(seg), _ptr(w), int(combiner),
               int(n_rows), _ptr(d), _ptr(out), _stream(self._device))
    return out

  def _find_combine_ragged_args(self, row_splits, ids, weights, prune, fill_id, default_row, out_dtype=None):
    """The arguments of one ragged pooled lookup as the C calls read them: (row_splits int64 [n_rows + 1], ids, weights or None,
    flags, fill id, default row, out), checked and on the table's device (find_combine_ragged and find_combine_ragged_many share
    it).  Shapes only: the content of row_splits is the kernel's business (it clamps), nothing is read on the host."""
    ids = self._keys(ids).reshape(-1)
    rs = torch.as_tensor(row_splits, device=self._device).reshape(-1)
    if rs.dtype not in (torch.int32, torch.int64):
      raise TypeError("row_splits must be int32 or int64, got %s" % rs.dtype)
    if rs.numel() < 1:
      raise ValueError("row_splits needs n_rows + 1 >= 1 elements")
    rs = rs.to(torch.int64).contiguous()   # int32 splits are widened
    w, d = self._pooled_operands(ids.numel(), weights, default_row)
    flags = (_capi.RAGGED_PRUNE if prune else 0) | (_capi.RAGGED_FILL if fill_id is not None else 0)
    out = torch.empty((rs.numel() - 1, self._dim), dtype=_out_dtype(out_dtype) or torch.float32, device=self._device)
    return rs, ids, w, flags, (0 if fill_id is None else int(fill_id)), d, out

  def find_combine_ragged(self, row_splits, ids, weights, combiner, prune=False, fill_id=None, default_row=None, out_dtype=None):
    """The pooled lookup over a ragged batch (tfra_table_find_combine_ragged): row r combines the entries
    [row_splits[r], row_splits[r + 1]) of ids / weights as `find_combine` combines the entries with seg == r, bit for bit, in ONE
    launch (no bounds pass).  row_splits int64 or int32 [n_rows + 1]; out-of-range or decreasing splits give empty or shortened
    rows, never a read outside ids.  prune: only entries with weight > 0 are members (ignored without weights).  fill_id: a row
    without members is the row of that key (`default_row` on a miss), up-cast as it is; None: zeros.  Nothing is read on the host.
    out_dtype: as `find_combine`'s (tfra_table_find_combine_ragged_typed)."""
    rs, ids, w, flags, fill, d, out = self._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row, out_dtype)
    if out_dtype is not None:
      ro = _rows_out(out)
      _capi.call("tfra_table_find_combine_ragged_typed", self._h, rs.numel() - 1, _ptr(rs), ids.numel(), _ptr(ids), _ptr(w),
                 int(combiner), flags, fill, _ptr(d), ctypes.byref(ro), _stream(self._device))
      return out
    _capi.call("tfra_table_find_combine_ragged", self._h, rs.numel() - 1, _ptr(rs), ids.numel(), _ptr(ids), _ptr(w), int(combiner),
               flags, fill, _ptr(d), _ptr(out), _stream(self._device))
    return out

  def _weight_grad_out(self, grad_out, n_rows, keep_half=False, grad_scale=None):
    """grad_out of a pooled lookup as the C calls read it: float32 [n_rows, dim] on the table's device, contiguous.
    keep_half (the *_typed calls): returns (tfra_grads, tensor) for a contiguous float16 / bfloat16 matrix, which goes down as it
    is with grad_scale beside it, else (None, the float32 up-cast times grad_scale) — `_grads_arg`, as the write-backs take it."""
    g = torch.as_tensor(grad_out, device=self._device)
    if g.dim() != 2 or g.shape[1] != self._dim or (n_rows is not None and g.shape[0] != n_rows):
      raise ValueError("grad_out must be [%s, %d] (the lookup's result), got %s" %
                       ("n_rows" if n_rows is None else n_rows, self._dim, list(g.shape)))
    if keep_half:
      return _grads_arg(g, self._device, self._dim, grad_scale)
    return g.to(torch.float32).contiguous()

  def find_combine_weight_grad(self, ids, seg, weights, combiner, grad_out, default_row=None):
    """The gradient of `find_combine` with respect to its weights (tfra_table_find_combine_backprop_weights): float32 [nnz],
    dw[p] = d loss / d weights[p] for grad_out = d loss / d out, float32 [n_rows, dim] — the rows read straight from the table as
    the forward reads them (the default row on a miss), never inserted, no [nnz, dim] tensor.  weights None = all 1 (the gradient
    with respect to those ones is still returned); an entry whose row lies outside [0, n_rows) gets 0; mean / sqrtn give 0 for a
    row whose weight sum is 0.  The limits are `find_combine`'s.  Bit-identical to find + device_ops.sparse_segment_combine_weight_grad
    over idx = arange(nnz)."""
    g = self._weight_grad_out(grad_out, None)
    ids, seg, w, d, _ = self._find_combine_args(ids, seg, weights, 0, default_row)
    dw = torch.empty(ids.numel(), dtype=torch.float32, device=self._device)
    _capi.call("tfra_table_find_combine_backprop_weights", self._h, _workspace(self._device), ids.numel(), _ptr(ids), _ptr(seg),
               _ptr(w), int(combiner), g.shape[0], _ptr(d), _ptr(g), _ptr(dw), _stream(self._device))
    return dw

  def find_combine_ragged_weight_grad(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                      default_row=None):
    """`find_combine_weight_grad` for `find_combine_ragged` (tfra_table_find_combine_ragged_backprop_weights), bit-identical to it on
    the row ids the splits stand for, in one launch.  An entry outside the clamped cover of row_splits gets 0.  prune: an entry
    whose weight is not > 0 gets exactly 0 and is in no sum, the members' values are those of the compacted list.  fill_id: the
    entries of a row without members get 0 (the fill row does not depend on the weights)."""
    rs, ids, w, flags, fill, d, _ = self._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row)
    g = self._weight_grad_out(grad_out, rs.numel() - 1)
    dw = torch.empty(ids.numel(), dtype=torch.float32, device=self._device)
    _capi.call("tfra_table_find_combine_ragged_backprop_weights", self._h, rs.numel() - 1, _ptr(rs), ids.numel(), _ptr(ids),
               _ptr(w), int(combiner), flags, fill, _ptr(d), _ptr(g), _ptr(dw), _stream(self._device))
    return dw

  def find_combine_weight_grad_typed(self, ids, seg, weights, combiner, grad_out, default_row=None, grad_scale=None):
    """`find_combine_weight_grad` that takes grad_out as the dense part of a half model hands it back: a contiguous float16 /
    bfloat16 [n_rows, dim] matrix goes down as it is (tfra_table_find_combine_backprop_weights_typed: no conversion pass, no
    float32 temporary), grad_scale — a one-element float32 device tensor the gradient is multiplied by, read by the kernel — with
    it.  The result is bit for bit `find_combine_weight_grad(grad_out.float() * grad_scale)`.  Any other grad_out (float32, or a
    half one that is not contiguous) is up-cast, multiplied in torch where a scale is given, and takes the untyped call.
    (A method beside `find_combine_weight_grad`, whose parameter list the tiered owners mirror and stays as it is.)"""
    return _wgrad_typed(self, self, "tfra_table_find_combine_backprop_weights", ids, seg, weights, combiner, grad_out, default_row,
                        grad_scale)

  def find_combine_ragged_weight_grad_typed(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                            default_row=None, grad_scale=None):
    """`find_combine_ragged_weight_grad` with grad_out and grad_scale as `find_combine_weight_grad_typed` takes them
    (tfra_table_find_combine_ragged_backprop_weights_typed)."""
    return _wgrad_ragged_typed(self, self, "tfra_table_find_combine_ragged_backprop_weights", row_splits, ids, weights, combiner,
                               grad_out, prune, fill_id, default_row, grad_scale)

  def upsert(self, keys, values, scores=None, unique_keys=False, field=0):
    keys = self._keys(keys)
    values = self._values_for(keys, values)
    n = keys.numel()
    if n == 0:
      return
    flags = _capi.FLAG_UNIQUE_KEYS if unique_keys else 0
    scores = _scores_for(scores, n, self._device)
    if field:
      _capi.call("tfra_table_insert_field", self._h, field, n, _ptr(keys), _ptr(values), flags, _stream(self._device))
    else:
      _capi.call("tfra_table_insert_or_assign", self._h, n, _ptr(keys), _ptr(values), _ptr(scores), flags,
                 _stream(self._device))

  def upsert_and_evict(self, keys, values, scores=None, whole_rows=False, cap=None, sync=True, count=None, whole_rows_in=False):
    """upsert(keys, values, scores, unique_keys=True) that hands back what it displaces (tfra_table_insert_and_evict): every entry
    that leaves a table at max_capacity because of this call, and every key the table does not admit (with the caller's row and
    its compare score).  -> (evicted_keys, evicted_values, evicted_scores), trimmed to their count: ONE host read of the counter.
    whole_rows: the rows are the whole co-located row, [(1 + aux_fields) * dim].  cap: room in the buffers (default: one entry
    per key, which always suffices); the count goes on beyond it, entries beyond it are not written.
    sync=False: (count, keys, values, scores) with `count` a device int64 tensor of shape [1] and the buffers untrimmed — no
    host read.  A table that is not at max_capacity reports nothing.
    count: a device int64 (or pinned) count of the leading keys that are served, read on the device; whole_rows_in: `values`
    rows are whole co-located rows, [(1 + aux_fields) * dim], and the slot vectors are written from them for new, replacing
    and resident keys alike (either one: tfra_table_insert_and_evict_n)."""
    keys = self._keys(keys)
    if whole_rows_in:
      if not torch.is_tensor(values) or values.dtype != self._value_dtype:
        raise TypeError("Signature mismatch. values must be a %s tensor." % self._value_dtype)
      want = tuple(keys.shape) + (self._dim * (1 + self._aux_fields),)
      if tuple(values.shape) != want:
        raise ValueError("Expected shape %s for whole-row values, got %s" % (list(want), list(values.shape)))
      values = values.to(self._device).contiguous()
    else:
      values = self._values_for(keys, values)
    n = keys.numel()
    scores = _scores_for(scores, n, self._device)
    cap = _cap_for(cap, n)
    width = self._dim * (1 + self._aux_fields if whole_rows else 1)
    counter = torch.zeros(1, dtype=torch.int64, device=self._device)
    ek = torch.empty(cap, dtype=torch.int64, device=self._device)
    ev = torch.empty((cap, width), dtype=self._value_dtype, device=self._device)
    es = torch.empty(cap, dtype=torch.int64, device=self._device)
    flags = _capi.EVICT_WHOLE_ROWS if whole_rows else 0
    if n and (count is not None or whole_rows_in):
      _capi.call("tfra_table_insert_and_evict_n", self._h, n, _ptr(count), _ptr(keys), _ptr(values), _ptr(scores),
                 flags | (_capi.INSERT_WHOLE_ROWS if whole_rows_in else 0), _ptr(counter), cap, _ptr(ek), _ptr(ev), _ptr(es),
                 _stream(self._device))
    elif n:
      _capi.call("tfra_table_insert_and_evict", self._h, n, _ptr(keys), _ptr(values), _ptr(scores),
                 flags, _ptr(counter), cap, _ptr(ek), _ptr(ev), _ptr(es), _stream(self._device))
    if not sync:
      return counter, ek, ev, es   # (the keys stay int64 here: narrowing the unwritten tail would read it)
    return _trim_to_count(counter, cap, ek, self._key_dtype, ev, es)

  def find_or_insert(self, keys, init_values=None, scores=None, return_exists=False, count=None, out=None):
    """The lookup that admits (tfra_table_find_or_insert): the resident row of every key that has one; a key that has none is
    inserted with its init row — `init_values[i]` ([n, dim]), or the one row `init_values` ([dim]; None: the table's default row)
    — as upsert(.., unique_keys=True) would insert it, and that row is returned.  `keys` are UNIQUE.  scores: as for `upsert`.
    count: a device int64 (or pinned) count of the leading keys that are served, read on the device; rows of `out` beyond it are
    left as they are.  out: the [n, dim] buffer to fill (default: a new one).  -> rows, or (rows, exists) — exists[i] False for
    every key that was not resident before the call, admitted or not.  Nothing is read on the host."""
    keys = self._keys(keys)
    n = keys.numel()
    d, full = self._init_rows(init_values, n)
    out = self._out(keys.shape, out)
    scores = _scores_for(scores, n, self._device)
    exists = torch.zeros(keys.shape, dtype=torch.bool, device=self._device) if return_exists else None
    if n:
      _capi.call("tfra_table_find_or_insert", self._h, n, _ptr(count), _ptr(keys), _ptr(d), full, _ptr(scores), _ptr(out),
                 _ptr(exists), _stream(self._device))
    return (out, exists) if return_exists else out

  def admit(self, keys, init_values=None, scores=None, count=None):
    """`find_or_insert` without its result (tfra_table_find_or_insert with values_out and found NULL): UNIQUE keys; afterwards every
    one of them that could be placed is resident, a never-seen key with its init row (`init_values`: [n, dim] or one row; None: the
    table's default row) and the slot vectors at aux_init, a resident key untouched but for its score.  scores, count: as for
    `find_or_insert`.  No [n, dim] buffer is allocated, no row is written back to the caller and nothing is read on the host: what
    a pooled training step of a random-initializer variable calls before `find_combine` (the write-back of the step then only
    hits).  Many tables at once: `table_admit_many`."""
    keys = self._keys(keys)
    n = keys.numel()
    d, full = self._init_rows(init_values, n)
    scores = _scores_for(scores, n, self._device)
    if n:
      _capi.call("tfra_table_find_or_insert", self._h, n, _ptr(count), _ptr(keys), _ptr(d), full, _ptr(scores), None, None,
                 _stream(self._device))

  def find_or_insert_planned(self, plan, init_values=None, scores=None, return_exists=False, out=None):
    """`find_or_insert` of a batch whose ids may repeat, over the write-back plan of that batch (tfra_table_find_or_insert_planned):
    `plan` is a built `SparsePlan` of this table's dim; the keys served are its distinct ids, and every batch position of an id
    gets the id's row.  init_values: [n, dim] — row p belongs to batch POSITION p, an id takes the row of its last position — or
    one row ([dim]; None: the table's default row).  scores: per position, an id takes its last position's.  out: the [n, dim]
    buffer to fill.  -> rows [n, dim], or (rows, exists).  The plan stays usable for `apply_planned` / `upsert_planned`: the
    batch is de-duplicated once.  Nothing is read on the host."""
    _check_plan(plan, self._dim, self._device)
    n = plan.n
    d, full = self._init_rows(init_values, n)
    out = self._out((n,), out)
    scores = _scores_for(scores, n, self._device, per="batch position")
    exists = torch.zeros(n, dtype=torch.bool, device=self._device) if return_exists else None
    if n:
      _over_plans((plan,), self._device, True, _capi.call, "tfra_table_find_or_insert_planned", self._h, plan._h, _ptr(d), full,
                  _ptr(scores), _ptr(out), _ptr(exists), _stream(self._device))
    return (out, exists) if return_exists else out

  # ---- the read side of a tier: find that lists its misses, a write that only hits, membership ----
  def find_missed(self, keys, dynamic_default_values=None, return_exists=False, return_scores=False, count=None, cap=None,
                  sync=True):
    """`find` that also lists its misses (tfra_table_find_missed): rows (and exists) are `find`'s; every batch position whose key is
    not resident is reported as a pair (key, position), in no particular order.  -> (rows, missed_keys, missed_indices[, exists]
    [, scores]) with the two lists trimmed to their count: ONE host read of the counter.  missed_indices is int32; scores [n]
    int64 holds what `export_all(with_scores=True)` reports for a hit and 0 for a miss.  count: a device int64 (or pinned) count
    of the leading keys that are served.  cap: room in the lists (default: one pair per key, which always suffices); the count
    goes on beyond it, pairs beyond it are not written.
    sync=False: (rows, counter, missed_keys, missed_indices, ...) with `counter` a device int64 tensor of shape [1] and the lists
    untrimmed (the keys stay int64) — nothing is read on the host, and `counter` can be the `count` of the next call on another
    table: find_n, upsert_n, find_or_insert."""
    keys = self._keys(keys)
    n = keys.numel()
    d, full = self._defaults(dynamic_default_values, n)
    out = torch.empty(tuple(keys.shape) + (self._dim,), dtype=self._value_dtype, device=self._device)
    cap = _cap_for(cap, n)
    exists = torch.zeros(keys.shape, dtype=torch.bool, device=self._device) if return_exists else None
    scores = torch.zeros(keys.shape, dtype=torch.int64, device=self._device) if return_scores else None
    counter = torch.zeros(1, dtype=torch.int64, device=self._device)
    mk = torch.empty(cap, dtype=torch.int64, device=self._device)
    mi = torch.empty(cap, dtype=torch.int32, device=self._device)
    if n:
      _capi.call("tfra_table_find_missed", self._h, n, _ptr(count), _ptr(keys), _ptr(out), _ptr(exists), _ptr(scores), _ptr(d), full,
                 _ptr(counter), cap, _ptr(mk), _ptr(mi), _stream(self._device))
    extra = ((exists,) if return_exists else ()) + ((scores,) if return_scores else ())
    if not sync:
      return (out, counter, mk, mi) + extra   # (the keys stay int64 here: narrowing the unwritten tail would read it)
    return (out,) + _trim_to_count(counter, cap, mk, self._key_dtype, mi) + extra

  def assign(self, keys, values, scores=None, return_found=False, count=None):
    """The write that only hits (tfra_table_assign): a resident key gets its row of `values` and its score is touched as `upsert`
    touches it; a key that is not resident changes nothing — it is not inserted, nothing is evicted for it.  `keys` are UNIQUE.
    count: a device int64 (or pinned) count of the leading keys that are served.  -> None, or found [n] bool (return_found)."""
    keys = self._keys(keys)
    values = self._values_for(keys, values)
    n = keys.numel()
    scores = _scores_for(scores, n, self._device)
    found = torch.zeros(keys.shape, dtype=torch.bool, device=self._device) if return_found else None
    if n:
      _capi.call("tfra_table_assign", self._h, n, _ptr(count), _ptr(keys), _ptr(values), _ptr(scores), _ptr(found),
                 _stream(self._device))
    return found

  def contains(self, keys, count=None):
    """exists of `find` without reading a row (tfra_table_contains) -> bool tensor shaped like keys."""
    keys = self._keys(keys)
    exists = torch.zeros(keys.shape, dtype=torch.bool, device=self._device)
    if keys.numel():
      _capi.call("tfra_table_contains", self._h, keys.numel(), _ptr(count), _ptr(keys), _ptr(exists), _stream(self._device))
    return exists

  def find_n(self, keys, count, out=None, return_exists=False):
    """find over the first `count[0]` entries of the buffer `keys`, the count read ON THE DEVICE (`count`: an int64 tensor on the
    table's device, or pinned host memory): tfra_table_find_n.  Rows beyond the count are left as they are."""
    keys = self._keys(keys)
    n = keys.numel()
    d = self._default_value.contiguous()
    if out is None:
      out = torch.empty((n, self._dim), dtype=self._value_dtype, device=self._device)
    exists = torch.zeros(n, dtype=torch.bool, device=self._device) if return_exists else None
    if n:
      _capi.call("tfra_table_find_n", self._h, n, _ptr(count), _ptr(keys), _ptr(out), _ptr(exists), _ptr(d), 0, _stream(self._device))
    return (out, exists) if return_exists else out

  def upsert_n(self, keys, count, values, scores=None):
    """insert_or_assign of the first `count[0]` UNIQUE keys of the buffer, the count read on the device
    (tfra_table_insert_or_assign_n; raises when the single-pass write-back cannot take the call)."""
    keys = self._keys(keys)
    values = self._values_for(keys, values)
    scores = _scores_for(scores, keys.numel(), self._device)
    if keys.numel():
      _capi.call("tfra_table_insert_or_assign_n", self._h, keys.numel(), _ptr(count), _ptr(keys), _ptr(values), _ptr(scores),
                 _stream(self._device))

  def accum_or_assign(self, keys, values_or_deltas, exists, scores=None, unique_keys=False):
    keys = self._keys(keys)
    vod = self._values_for(keys, values_or_deltas, "values_or_deltas")
    exists = torch.as_tensor(exists, device=self._device)
    if exists.dtype != torch.bool:
      raise TypeError("exists must be a bool tensor")
    if exists.numel() != keys.numel():
      raise ValueError("exists must have the same number of elements as keys")
    exists = exists.contiguous()
    n = keys.numel()
    if n == 0:
      return
    scores = _scores_for(scores, n, self._device)
    _capi.call("tfra_table_accum_or_assign", self._h, n, _ptr(keys), _ptr(vod), _ptr(exists), _ptr(scores),
               _capi.FLAG_UNIQUE_KEYS if unique_keys else 0, _stream(self._device))

  def erase(self, keys):
    keys = self._keys(keys)
    if keys.numel():
      _capi.call("tfra_table_erase", self._h, keys.numel(), _ptr(keys), _stream(self._device))

  def clear_all(self):
    _capi.call("tfra_table_clear", self._h, _stream(self._device))

  def size_host(self):
    out = ctypes.c_size_t()
    _capi.call("tfra_table_size", self._h, ctypes.byref(out), _stream(self._device))
    return out.value

  def size_device(self):
    out = torch.empty((), dtype=torch.int64, device=self._device)
    _capi.call("tfra_table_size_to_device", self._h, _ptr(out), _stream(self._device))
    return out

  def capacity(self):
    out = ctypes.c_size_t()
    _capi.call("tfra_table_capacity", self._h, ctypes.byref(out))
    return out.value

  def check_errors(self):
    """Raises TfraError if the device dropped keys since the last check (table full, plan overflow); synchronises."""
    _capi.call("tfra_table_check_errors", self._h, _stream(self.device))

  def slot_census(self):
    """{empty, locked, live, ovf0, ovf1}: key-slot and bucket-flag counts (introspection; synchronises)."""
    out = (ctypes.c_uint64 * 5)()
    _capi.call("tfra_table_slot_census", self._h, out, _stream(self.device))
    return dict(zip(("empty", "locked", "live", "ovf0", "ovf1"), [int(x) for x in out]))

  def growth_stats(self):
    """{growths, in_place, mapped_range, mapped_bytes} (tfra_table_growth_stats)."""
    out = (ctypes.c_uint64 * 4)()
    _capi.call("tfra_table_growth_stats", self._h, out)
    return dict(zip(("growths", "in_place", "mapped_range", "mapped_bytes"), [int(x) for x in out]))

  def set_capture_safe(self, on):
    """While True every op on this table can be captured into a HIP graph (no host sync, no growth)."""
    _capi.call("tfra_table_set_option", self._h, _capi.OPTION_CAPTURE_SAFE, int(bool(on)))

  def set_stochastic_rounding(self, seed):
    """seed: None or 0 = off (the default: nearest even); any other 64-bit value: the fused optimizer write-backs of this float16 /
    bfloat16 table round the parameter and the slots the rule owns stochastically, with random bits that are a pure function of
    (seed, write-backs since this call, key, element) — TFRA_OPTION_STOCHASTIC_ROUNDING.  Every call restarts the count at 0.
    Upserts, insert_or_accum, the constant fill of fields the rule does not own and the Generic optimizers
    (Momentum / RMSProp without fused=True among them) keep nearest even."""
    seed = 0 if seed is None else int(seed) & ((1 << 64) - 1)
    _capi.call("tfra_table_set_option", self._h, _capi.OPTION_STOCHASTIC_ROUNDING, seed - (1 << 64) if seed >> 63 else seed)
    self.stochastic_rounding = seed

  def set_owner_tags(self, on):
    """False: planned write-backs take the general two-kernel path (what runs when the tag array cannot be allocated)."""
    _capi.call("tfra_table_set_option", self._h, _capi.OPTION_NO_OWNER_TAGS, int(not on))

  def reserve(self, n_slots):
    _capi.call("tfra_table_reserve", self._h, int(n_slots), _stream(self._device))

  def export_all(self, with_scores=False, values=True, split_size=None):
    """Export = size, then export_batch over the capacity (hkv_hashtable_op_gpu.cu.cc:425-470)."""
    n = self.size_host()
    cap = self.capacity()
    keys = torch.empty(n, dtype=torch.int64, device=self._device)
    vals = torch.empty((n, self._dim), dtype=self._value_dtype, device=self._device) if values else None
    scores = torch.empty(n, dtype=torch.int64, device=self._device) if with_scores else None
    counter = torch.zeros(1, dtype=torch.int64, device=self._device)
    step = cap if not split_size else int(split_size)
    for off in range(0, cap, step):
      _capi.call("tfra_table_export_batch", self._h, min(step, cap - off), off, _ptr(counter), _ptr(keys), _ptr(vals),
                 _ptr(scores), _stream(self._device))
    got = int(counter.item())
    if got != n:
      raise RuntimeError("export: table changed during export (%d vs %d)" % (got, n))
    return _narrow_keys(keys, self._key_dtype), vals, scores

  # ---- score-filtered scans (tables with scores: every Hkv strategy) --------------------------
  def count_if(self, threshold, pred="ge"):
    """Number of entries whose score matches, as a device int64 tensor of shape [1] (tfra_table_export_batch_if, count only:
    one scan of the key and score lines, no host read)."""
    p, thr = _score_filter(threshold, pred)
    counter = torch.zeros(1, dtype=torch.int64, device=self._device)
    _capi.call("tfra_table_export_batch_if", self._h, p, thr, self.capacity(), 0, _ptr(counter), 0, None, None, None,
               _stream(self._device))
    return counter

  def export_if(self, threshold, pred="ge", with_scores=True, values=True):
    """(keys, values, scores) of the entries whose score matches, order unspecified: a count-only pass, ONE host read of the
    count (it sizes the tensors), then the export pass with cap = that count."""
    p, thr = _score_filter(threshold, pred)
    n = int(self.count_if(threshold, pred).item())
    keys = torch.empty(n, dtype=torch.int64, device=self._device)
    vals = torch.empty((n, self._dim), dtype=self._value_dtype, device=self._device) if values else None
    scores = torch.empty(n, dtype=torch.int64, device=self._device) if with_scores else None
    if n:
      counter = torch.zeros(1, dtype=torch.int64, device=self._device)
      _capi.call("tfra_table_export_batch_if", self._h, p, thr, self.capacity(), 0, _ptr(counter), n, _ptr(keys), _ptr(vals),
                 _ptr(scores), _stream(self._device))
    return _narrow_keys(keys, self._key_dtype), vals, scores

  def erase_if(self, threshold, pred="lt"):
    """Erases every entry whose score matches; the number erased as a device int64 tensor of shape [1] (no host sync)."""
    p, thr = _score_filter(threshold, pred)
    erased = torch.zeros(1, dtype=torch.int64, device=self._device)
    _capi.call("tfra_table_erase_if", self._h, p, thr, _ptr(erased), _stream(self._device))
    return erased

  def save_if(self, prefix, threshold, pred="ge", buffer_size=4194304, append_to_file=False, field=0):
    """save() of the entries whose score matches only (a delta checkpoint; load() merges it over a base)."""
    p, thr = _score_filter(threshold, pred)
    out = ctypes.c_size_t()
    _capi.call("tfra_table_save_if", self._h, int(field), p, thr, prefix.encode(), int(buffer_size), int(bool(append_to_file)),
               _stream(self._device), ctypes.byref(out))
    return out.value

  def save(self, prefix, buffer_size=4194304, append_to_file=False, field=0):
    """field > 0: the co-located state vector `field` (an optimizer slot) in the same file format."""
    self.check_errors()   # a sync point anyway: insert / apply failures must not pass silently into a checkpoint
    out = ctypes.c_size_t()
    _capi.call("tfra_table_save_field", self._h, int(field), prefix.encode(), int(buffer_size), int(bool(append_to_file)),
               _stream(self._device), ctypes.byref(out))
    return out.value

  def load(self, prefix, buffer_size=4194304, field=0):
    out = ctypes.c_size_t()
    _capi.call("tfra_table_load_field", self._h, int(field), prefix.encode(), int(buffer_size), _stream(self._device),
               ctypes.byref(out))
    return out.value

  def apply_optimizer(self, params, keys, grads, param_defaults, n_dev=None):
    """n_dev: optional device int64 scalar = number of leading (key, grad) pairs that are valid."""
    keys = self._keys(keys)
    grads = grads.to(self._device, torch.float32).contiguous()
    if tuple(grads.shape) != tuple(keys.shape) + (self._dim,):
      raise ValueError("Expected shape %s for grads, got %s" % (list(keys.shape) + [self._dim], list(grads.shape)))
    d = param_defaults.to(self._device, torch.float32).contiguous()
    full = int(d.numel() == grads.numel())
    _capi.call("tfra_table_apply_optimizer", self._h, ctypes.byref(params), keys.numel(), _ptr(keys), _ptr(grads), _ptr(d),
               full, _ptr(n_dev), _stream(self._device))

  # ---- write-backs of a batch whose ids may repeat; `plan`: a built `SparsePlan`, the id-only half made ahead ----
  def apply_sparse(self, params, ids, grads, default_row, grad_scale=None):
    """ids may repeat: duplicate gradients are summed (fixed order), one fused update per unique key.  A contiguous float16 /
    bfloat16 gradient matrix on the table's device goes down as it is (tfra_table_apply_sparse_typed: the same bits as its
    float32 up-cast gives), grad_scale — a one-element float32 device tensor the gradients are multiplied by — with it."""
    ids = self._keys(ids).reshape(-1)
    typed, grads = _grads_arg(grads, self._device, self._dim, grad_scale)
    if grads.numel() != ids.numel() * self._dim:
      raise ValueError("Expected shape %s for grads, got %s" % ([ids.numel(), self._dim], list(grads.shape)))
    d = default_row.to(self._device, torch.float32).contiguous()
    if typed is not None:
      _capi.call("tfra_table_apply_sparse_typed", self._h, ctypes.byref(params), ids.numel(), _ptr(ids), ctypes.byref(typed), _ptr(d),
                 _stream(self._device))
      return
    _capi.call("tfra_table_apply_sparse", self._h, ctypes.byref(params), ids.numel(), _ptr(ids), _ptr(grads), _ptr(d),
               _stream(self._device))

  def apply_planned(self, params, plan, grads, default_row, sync=True, grad_scale=None):
    """Gradient half of apply_sparse for a batch whose id-only half was built ahead (`SparsePlan`); half gradients and
    grad_scale as in apply_sparse (tfra_table_apply_planned_typed)."""
    _check_plan(plan, self._dim, self._device)
    typed, grads = _grads_arg(grads, self._device, self._dim, grad_scale)
    if grads.numel() != plan.n * self._dim:
      raise ValueError("Expected shape %s for grads, got %s" % ([plan.n, self._dim], list(grads.shape)))
    d = default_row.to(self._device, torch.float32).contiguous()
    if typed is not None:
      _over_plans((plan,), self._device, sync, _capi.call, "tfra_table_apply_planned_typed", self._h, ctypes.byref(params), plan._h,
                  ctypes.byref(typed), _ptr(d), _stream(self._device))
      return
    _over_plans((plan,), self._device, sync, _capi.call, "tfra_table_apply_planned", self._h, ctypes.byref(params), plan._h,
                _ptr(grads), _ptr(d), _stream(self._device))

  def _apply_combined_args(self, plan, grad_out, seg, weights, default_row, grad_scale=None):
    """A combined write-back's grad_out, seg, weights (or None) and default row, checked and as the C calls take them.  grad_out
    comes back as `_grads_arg` gives it: (tfra_grads, tensor) for a contiguous half matrix inside the typed calls' limits (8-byte
    aligned, n_rows * dim < 2^32), else (None, the float32 up-cast times grad_scale)."""
    _check_plan(plan, self._dim, self._device)
    if grad_out.dim() != 2 or grad_out.shape[1] != self._dim:
      raise ValueError("Expected grad_out of shape [n_rows, %d], got %s" % (self._dim, list(grad_out.shape)))
    grad_out = _grads_arg(grad_out, self._device, self._dim, grad_scale, max_elements=1 << 32)
    seg = seg.to(self._device, torch.int64).contiguous()
    if seg.numel() != plan.n or (weights is not None and weights.numel() != plan.n):
      raise ValueError("seg / weights need one element per plan entry (%d)" % plan.n)
    w = None if weights is None else weights.to(self._device, torch.float32).contiguous()
    d = default_row.to(self._device, torch.float32).contiguous()
    return grad_out, seg, w, d

  def apply_planned_combined(self, params, plan, grad_out, seg, weights, combiner, default_row, sync=True, grad_scale=None):
    """apply_planned for an embedding_lookup_sparse (tfra_table_apply_planned_combined): `plan` built over the entry ids,
    grad_out [n_rows, dim] the gradient of the combined result, seg [nnz] its row ids (ascending), weights [nnz] or None,
    combiner 0 sum / 1 mean / 2 sqrtn.  Entry e's gradient is formed from grad_out inside the write-back kernels.  A contiguous
    float16 / bfloat16 grad_out goes down as it is, grad_scale (as in apply_sparse) with it (tfra_table_apply_planned_combined_typed:
    the same bits as the float32 up-cast times the scale gives)."""
    (typed, grad_out), seg, w, d = self._apply_combined_args(plan, grad_out, seg, weights, default_row, grad_scale)
    if typed is not None:
      _over_plans((plan,), self._device, sync, _capi.call, "tfra_table_apply_planned_combined_typed", self._h, ctypes.byref(params),
                  plan._h, ctypes.byref(typed), _ptr(seg), _ptr(w), int(combiner), grad_out.shape[0], _ptr(d), _stream(self._device))
      return
    _over_plans((plan,), self._device, sync, _capi.call, "tfra_table_apply_planned_combined", self._h, ctypes.byref(params), plan._h,
                _ptr(grad_out), _ptr(seg), _ptr(w), int(combiner), grad_out.shape[0], _ptr(d), _stream(self._device))

  def upsert_sparse(self, ids, values, scores=None):
    """insert_or_assign of a batch whose keys may repeat: the LAST occurrence wins (the reference's sequential
    order), de-duplicated on the device — also on a bounded table at max_capacity."""
    ids = self._keys(ids).reshape(-1)
    values = self._values_for(ids, values.reshape(ids.numel(), -1))
    scores = _scores_for(scores, ids.numel(), self._device)
    if ids.numel():
      _capi.call("tfra_table_upsert_sparse", self._h, ids.numel(), _ptr(ids), _ptr(values), _ptr(scores), _stream(self._device))

  def upsert_planned(self, plan, values, scores=None, sync=True):
    """Assign half of upsert_sparse for a batch whose id-only half was built ahead (`SparsePlan`)."""
    if plan._device != self._device:   # (not `_check_plan`: an assign-only plan is built with dim 0 and serves any row width)
      raise ValueError("the plan lives on %s" % (plan._device,))
    values = values.to(self._device).contiguous()
    if values.dtype != self._value_dtype or values.numel() != plan.n * self._dim:
      raise ValueError("Expected %s values of shape %s" % (self._value_dtype, [plan.n, self._dim]))
    scores = _scores_for(scores, plan.n, self._device, per="batch position")
    _over_plans((plan,), self._device, sync, _capi.call, "tfra_table_upsert_planned", self._h, plan._h, _ptr(values), _ptr(scores),
                _stream(self._device))

  # ---- whole rows out and back: the two calls of a dense rule without a fused write-back (optimizers.Generic, whole_rows=True) ----
  def _row_fields(self, tensors):
    """A tfra_row_fields over `tensors` (one per field, None = NULL)."""
    rf = _capi.RowFields()
    rf.struct_size, rf.n_fields = ctypes.sizeof(_capi.RowFields), 1 + self._aux_fields
    for f, x in enumerate(tensors):
      rf.field[f] = None if x is None else x.data_ptr()
    return rf

  def fetch_planned(self, plan, grads=None, grad_scale=None, fields=None, default_row=None):
    """The rows of a batch's distinct keys, whole, and the per-key sums of its gradients (tfra_table_fetch_planned): `plan` is a
    built `SparsePlan` of this table's dim.  -> (keys [n] int64, [field tensors], gsum, count): row j < count of every output
    belongs to keys[j]; field tensor f is [n, dim] float32 — the exact up-cast of the stored field of a resident key, of
    `default_row` (None: the table's; one row in the table's value dtype) for field 0 and of aux_init for the slot vectors of a
    key that is not resident — or None where `fields[f]` is false (fields None: all of them); gsum [n, dim] float32 the sums
    `device_ops.reduce_by_key` gives for the same ids and `grads` (float32, or float16 / bfloat16 as they are; grad_scale as in
    `apply_sparse`), None without `grads`; count a one-element int64 DEVICE tensor (-1: the plan overflowed).  Rows at or beyond
    count are not written.  A read: nothing is inserted, no score is touched, nothing is read on the host."""
    _check_plan(plan, self._dim, self._device)
    n, nf = plan.n, 1 + self._aux_fields
    want = [True] * nf if fields is None else [bool(x) for x in fields]
    if len(want) != nf:
      raise ValueError("fields must have one entry per field of the row (%d), got %d" % (nf, len(want)))
    typed = g = None
    if grads is not None:
      typed, g = _grads_arg(grads, self._device, self._dim, grad_scale)
      if g.numel() != n * self._dim:
        raise ValueError("Expected shape %s for grads, got %s" % ([n, self._dim], list(g.shape)))
      if typed is None:
        typed = _capi.Grads(g.data_ptr(), _capi.TFRA_F32, 0, None)
    d = _rows_on(self._value_dtype, self._device, self._default_value if default_row is None else default_row, "default row")
    if d.numel() < self._dim:
      raise ValueError("default row needs dim=%d elements, got %d" % (self._dim, d.numel()))
    keys = torch.empty(n, dtype=torch.int64, device=self._device)
    outs = [torch.empty((n, self._dim), dtype=torch.float32, device=self._device) if w else None for w in want]
    gsum = torch.empty((n, self._dim), dtype=torch.float32, device=self._device) if g is not None and n else None
    count = torch.zeros(1, dtype=torch.int64, device=self._device)
    if n:
      rf = self._row_fields(outs)
      _over_plans((plan,), self._device, True, _capi.call, "tfra_table_fetch_planned", self._h, plan._h,
                  ctypes.byref(typed) if gsum is not None else None, _ptr(d), _ptr(keys), ctypes.byref(rf), _ptr(gsum), _ptr(count),
                  _stream(self._device))
    return keys, outs, gsum, count

  def store_rows(self, keys, fields, count=None):
    """The write that goes with `fetch_planned` (tfra_table_store_rows): a unique-keys upsert of whole rows given as float32
    field tensors.  keys [n] int64, UNIQUE; fields: one [n, dim] float32 tensor per field of the row, or None for a field that
    is not written (a resident key keeps its bytes there, a new key starts at aux_init); fields[0] is required.  Every element
    is rounded to the table's value dtype once, to nearest even.  count: a device int64 count of the leading keys that are
    written (None: all).  Scores and the epoch move as for ONE upsert(unique_keys=True) without scores."""
    keys = _as_tensor(keys, self._device)
    if keys.dtype != torch.int64:
      raise TypeError("store_rows takes the engine's int64 keys (as fetch_planned returns them), got %s" % keys.dtype)
    keys = keys.to(self._device).contiguous().reshape(-1)
    n, nf = keys.numel(), 1 + self._aux_fields
    fields = list(fields)
    if len(fields) != nf:
      raise ValueError("fields must have one entry per field of the row (%d), got %d" % (nf, len(fields)))
    if fields[0] is None:
      raise ValueError("fields[0], the embedding, is required")
    rows = []
    for f, x in enumerate(fields):
      if x is not None:
        x = x.to(self._device, torch.float32).contiguous()
        if x.numel() != n * self._dim:
          raise ValueError("Expected shape %s for field %d, got %s" % ([n, self._dim], f, list(x.shape)))
      rows.append(x)
    if n == 0:
      return
    rf = self._row_fields(rows)
    _capi.call("tfra_table_store_rows", self._h, n, _ptr(count), _ptr(keys), ctypes.byref(rf), _stream(self._device))


class _DeviceTier:
  """Owns one tfra_tier_t: `upper`, a bounded LRU / EPOCHLRU _DeviceTable, in front of `lower`, a growing _DeviceTable without
  eviction.  Whole co-located rows move between the two on the device; nothing but `stats` reads on the host.  After every call,
  for every key ever written through the tier: upper holds its newest whole row if it contains the key, otherwise lower does."""

  def __init__(self, upper, lower, max_batch):
    self._upper, self._lower = upper, lower   # (kept alive: the driver must go before its tables)
    self._max_batch = int(max_batch)
    h = ctypes.c_void_p()
    _capi.call("tfra_tier_create", upper._h, lower._h, self._max_batch, ctypes.byref(h))
    self._h = h

  def __del__(self):
    h = getattr(self, "_h", None)
    if h:
      try:
        _capi.lib().tfra_tier_destroy(h)
      except Exception:  # interpreter shutdown
        pass
      self._h = None

  @property
  def max_batch(self):
    return self._max_batch

  def find(self, keys, dynamic_default_values=None, return_where=False, count=None, out=None, out_dtype=None):
    """A read (tfra_tier_find): the row upper holds, else the row lower holds, else the default.  Keys may repeat; nothing moves and
    neither table is written.  -> rows, or (rows, where) with where uint8: 1 = upper, 2 = lower, 0 = neither.  The default rows
    follow the admitting rule ([n, dim] or exactly one row), not `_DeviceTable.find`'s.  out_dtype: the tier calls are not typed —
    the rows are converted behind the call."""
    if _out_dtype(out_dtype) is not None:
      r = self.find(keys, dynamic_default_values, return_where, count, out)
      return (r[0].to(out_dtype), r[1]) if return_where else r.to(out_dtype)
    keys = self._upper._keys(keys)
    d, full = self._upper._init_rows(dynamic_default_values, keys.numel(), "default values")
    out = self._upper._out(keys.shape, out)
    where = torch.zeros(keys.shape, dtype=torch.uint8, device=self._upper._device)
    if keys.numel():
      _capi.call("tfra_tier_find", self._h, keys.numel(), _ptr(count), _ptr(keys), _ptr(out), _ptr(where), _ptr(d), full,
                 _stream(self._upper._device))
    return (out, where) if return_where else out

  def _admit_args(self, keys, init_values, want_rows, out=None):
    """The operands of tfra_tier_find_or_insert, ONE copy for `find_or_insert`, `admit` and the grouped forms
    (`tier_find_or_insert_many`, `admit_many`): -> keys, init rows, init_is_full, rows out, where (the last two None unless
    want_rows)."""
    keys = self._upper._keys(keys)
    d, full = self._upper._init_rows(init_values, keys.numel())
    if not want_rows:
      return keys, d, full, None, None
    out = self._upper._out(keys.shape, out)
    return keys, d, full, out, torch.zeros(keys.shape, dtype=torch.uint8, device=self._upper._device)

  def find_or_insert(self, keys, init_values=None, return_where=False, count=None, out=None, verify=False):
    """The lookup of a training step (tfra_tier_find_or_insert): UNIQUE keys; rows as `find` returns them, a never-seen key's being
    its init row.  Afterwards every key of the batch is resident in upper with its whole row (the slot vectors it had below, or
    aux_init), and what that displaced is below.  verify: count the batch keys that are NOT resident at the end into
    stats()["not_resident"] (a batch that fills both home buckets of one of its keys with its own keys)."""
    keys, d, full, out, where = self._admit_args(keys, init_values, True, out)
    if keys.numel():
      _capi.call("tfra_tier_find_or_insert", self._h, keys.numel(), _ptr(count), _ptr(keys), _ptr(d), full, _ptr(out), _ptr(where),
                 _capi.TIER_VERIFY if verify else 0, _stream(self._upper._device))
    return (out, where) if return_where else out

  def admit(self, keys, init_values=None, count=None, verify=False):
    """`find_or_insert` without its result (tfra_tier_find_or_insert with values_out and where NULL): UNIQUE keys, at most
    max_batch; afterwards every one of them is resident in upper with its whole row, a never-seen key with its init row
    (`init_values`: [n, dim] or one row; None: the table's default row).  count: a device int64 (or pinned) count of the leading
    keys that are served.  No row is written back to the caller and nothing is read on the host: what a pooled training step
    calls before `find_combine` (the write-back of the step then only hits).  Many tiers at once: `admit_many`."""
    keys, d, full, _, _ = self._admit_args(keys, init_values, False)
    if keys.numel():
      _capi.call("tfra_tier_find_or_insert", self._h, keys.numel(), _ptr(count), _ptr(keys), _ptr(d), full, None, None,
                 _capi.TIER_VERIFY if verify else 0, _stream(self._upper._device))

  def _planned_args(self, plan, init_values):
    """The plan-side operands of tfra_tier_find_or_insert_planned, ONE copy for `find_or_insert_planned` and `admit_planned`: the
    plan's checks — its dim and device, at most max_batch ids (the tier's staging) — and the init rows, [n, dim] per batch
    POSITION or one row, by the admitting rule."""
    up = self._upper
    _check_plan(plan, up._dim, up._device)
    if plan.n > self._max_batch:
      raise ValueError("the plan holds %d ids, more than the tier's max_batch %d" % (plan.n, self._max_batch))
    return up._init_rows(init_values, plan.n)

  def find_or_insert_planned(self, plan, init_values=None, return_where=False, out=None, verify=False):
    """`find_or_insert` of a batch whose ids may repeat, over the write-back plan of that batch (tfra_tier_find_or_insert_planned):
    `plan` is a built `SparsePlan` of the tables' dim with at most max_batch ids; the keys served are its distinct ids, and every
    batch position of an id gets the id's row and its `where` byte.  init_values: [n, dim] — row p belongs to batch POSITION p, an
    id takes the row of its last position — or one row ([dim]; None: the table's default row).  out: the [n, dim] buffer to fill.
    -> rows [n, dim], or (rows, where).  Afterwards every distinct id is resident in upper with its whole row, and the plan serves
    `apply_planned` / `upsert_planned` on upper: the batch is de-duplicated once.  verify: as `find_or_insert`, per distinct id.
    Nothing is read on the host."""
    d, full = self._planned_args(plan, init_values)
    up, n = self._upper, plan.n
    out = up._out((n,), out)
    where = torch.zeros(n, dtype=torch.uint8, device=up._device) if return_where else None   # (not wanted: not written)
    if n:
      _over_plans((plan,), up._device, True, _capi.call, "tfra_tier_find_or_insert_planned", self._h, plan._h, _ptr(d), full,
                  _ptr(out), _ptr(where), _capi.TIER_VERIFY if verify else 0, _stream(up._device))
    return (out, where) if return_where else out

  def admit_planned(self, plan, init_values=None, verify=False):
    """`find_or_insert_planned` without its result (rows_out and where NULL): afterwards every distinct id of the plan is resident
    in upper with its whole row; no row is written back to the caller, and the launches that spread rows to positions do not run."""
    d, full = self._planned_args(plan, init_values)
    if plan.n:
      _over_plans((plan,), self._upper._device, True, _capi.call, "tfra_tier_find_or_insert_planned", self._h, plan._h, _ptr(d), full,
                  None, None, _capi.TIER_VERIFY if verify else 0, _stream(self._upper._device))

  def find_combine_typed(self, ids, seg, weights, combiner, n_rows, default_row=None, out_dtype=None):
    """`find_combine` with `_DeviceTable.find_combine_typed`'s out_dtype: the tier calls are not typed — the float32 result is
    converted."""
    out = self.find_combine(ids, seg, weights, combiner, n_rows, default_row)
    return out if _out_dtype(out_dtype) is None else out.to(out_dtype)

  def find_combine(self, ids, seg, weights, combiner, n_rows, default_row=None):
    """`_DeviceTable.find_combine` over both tiers (tfra_tier_find_combine): an entry's row is the one upper holds, else the one
    lower holds, else `default_row`.  A read: nothing moves, nothing is written, `stats()` does not change; ids are not limited by
    max_batch.  Bit-identical to `find` + device_ops.sparse_segment_combine over idx = arange(nnz)."""
    up = self._upper
    ids, seg, w, d, out = up._find_combine_args(ids, seg, weights, n_rows, default_row)
    _capi.call("tfra_tier_find_combine", self._h, _workspace(up._device), ids.numel(), _ptr(ids), _ptr(seg), _ptr(w), int(combiner),
               int(n_rows), _ptr(d), _ptr(out), _stream(up._device))
    return out

  def find_combine_ragged(self, row_splits, ids, weights, combiner, prune=False, fill_id=None, default_row=None, out_dtype=None):
    """`_DeviceTable.find_combine_ragged` over both tiers (tfra_tier_find_combine_ragged), in one launch: bit-identical to
    `find_combine` on the row ids the splits stand for; the row of `fill_id` is looked up in upper, then lower, then is
    `default_row`.  A read, as `find_combine`; out_dtype as there."""
    if _out_dtype(out_dtype) is not None:
      return self.find_combine_ragged(row_splits, ids, weights, combiner, prune, fill_id, default_row).to(out_dtype)
    up = self._upper
    rs, ids, w, flags, fill, d, out = up._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row)
    _capi.call("tfra_tier_find_combine_ragged", self._h, rs.numel() - 1, _ptr(rs), ids.numel(), _ptr(ids), _ptr(w), int(combiner),
               flags, fill, _ptr(d), _ptr(out), _stream(up._device))
    return out

  def find_combine_weight_grad(self, ids, seg, weights, combiner, grad_out, default_row=None):
    """`_DeviceTable.find_combine_weight_grad` over both tiers (tfra_tier_find_combine_backprop_weights): float32 [nnz], the rows
    read as `find_combine` reads them — upper's, else lower's, else `default_row`.  A read: nothing moves, nothing is written,
    `stats()` does not change; ids are not limited by max_batch.  Bit-identical to `find` +
    device_ops.sparse_segment_combine_weight_grad over idx = arange(nnz)."""
    up = self._upper
    g = up._weight_grad_out(grad_out, None)
    ids, seg, w, d, _ = up._find_combine_args(ids, seg, weights, 0, default_row)
    dw = torch.empty(ids.numel(), dtype=torch.float32, device=up._device)
    _capi.call("tfra_tier_find_combine_backprop_weights", self._h, _workspace(up._device), ids.numel(), _ptr(ids), _ptr(seg),
               _ptr(w), int(combiner), g.shape[0], _ptr(d), _ptr(g), _ptr(dw), _stream(up._device))
    return dw

  def find_combine_ragged_weight_grad(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                      default_row=None):
    """`_DeviceTable.find_combine_ragged_weight_grad` over both tiers (tfra_tier_find_combine_ragged_backprop_weights), in one
    launch: bit-identical to `find_combine_weight_grad` on the row ids the splits stand for; prune and fill_id as there (a pruned
    entry and the entries of a row without members get 0; the fill id is not looked up).  A read, as `find_combine_weight_grad`."""
    up = self._upper
    rs, ids, w, flags, fill, d, _ = up._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row)
    g = up._weight_grad_out(grad_out, rs.numel() - 1)
    dw = torch.empty(ids.numel(), dtype=torch.float32, device=up._device)
    _capi.call("tfra_tier_find_combine_ragged_backprop_weights", self._h, rs.numel() - 1, _ptr(rs), ids.numel(), _ptr(ids),
               _ptr(w), int(combiner), flags, fill, _ptr(d), _ptr(g), _ptr(dw), _stream(up._device))
    return dw

  def find_combine_weight_grad_typed(self, ids, seg, weights, combiner, grad_out, default_row=None, grad_scale=None):
    """`_DeviceTable.find_combine_weight_grad_typed` over both tiers (tfra_tier_find_combine_backprop_weights_typed): a contiguous
    float16 / bfloat16 grad_out goes down as it is, grad_scale with it.  A read, as `find_combine_weight_grad`."""
    return _wgrad_typed(self, self._upper, "tfra_tier_find_combine_backprop_weights", ids, seg, weights, combiner, grad_out,
                        default_row, grad_scale)

  def find_combine_ragged_weight_grad_typed(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                            default_row=None, grad_scale=None):
    """`_DeviceTable.find_combine_ragged_weight_grad_typed` over both tiers (tfra_tier_find_combine_ragged_backprop_weights_typed)."""
    return _wgrad_ragged_typed(self, self._upper, "tfra_tier_find_combine_ragged_backprop_weights", row_splits, ids, weights,
                               combiner, grad_out, prune, fill_id, default_row, grad_scale)

  def insert(self, keys, values, count=None):
    """upsert of embedding rows (UNIQUE keys) into upper; what it displaces goes down as whole rows (tfra_tier_insert)."""
    keys = self._upper._keys(keys)
    values = self._upper._values_for(keys, values)
    if keys.numel():
      _capi.call("tfra_tier_insert", self._h, keys.numel(), _ptr(count), _ptr(keys), _ptr(values), _stream(self._upper._device))

  def stats(self):
    """-> dict(calls, missed, lower_hits, demoted, not_resident), cumulative.  The one call that reads on the host."""
    w = (ctypes.c_uint64 * 8)()
    _capi.call("tfra_tier_stats", self._h, w, _stream(self._upper._device))
    return dict(zip(("calls", "missed", "lower_hits", "demoted", "not_resident"), (int(x) for x in w[:5])))


class SparsePlan:
  """The id-only half of `apply_sparse` for one batch (tfra_sparse_plan_*): which ids repeat, the order
  their gradients are summed in, the unique keys of the step.  Build it as soon as the ids are known —
  on a side stream next to the lookup of the same ids, or while the previous step is still running —
  and hand it to `_DeviceTable.apply_planned` with the gradients.  Stream ordering is handled here:
  `apply_planned` waits for the build, a rebuild waits for the last `apply_planned` that used the plan."""

  def __init__(self, device, dim):
    self._device = _as_device(device)
    self._dim = int(dim)
    self._h = ctypes.c_void_p()
    _capi.call("tfra_sparse_plan_create", self._device.index, ctypes.byref(self._h))
    self._built = torch.cuda.Event()
    self._used = None
    self.ids = None
    self.n = 0

  def build(self, ids, sync=True):
    """Enqueue the build on the CURRENT stream of the plan's device.  sync=False leaves the ordering
    against `apply_planned` to the caller (a captured HIP graph orders them by its edges)."""
    ids = ids.to(self._device, torch.int64).contiguous().reshape(-1)
    stream = torch.cuda.current_stream(self._device)
    if sync:
      if self._used is not None:
        stream.wait_event(self._used)     # the previous batch's sums/apply still read the plan buffers
      ids.record_stream(stream)
    self.ids, self.n = ids, ids.numel()   # keeps the ids alive until the next build
    _capi.call("tfra_sparse_plan_build", self._h, self.n, _ptr(ids), self._dim, _stream(self._device))
    if sync:
      self._built.record(stream)
    return self

  def _wait_built(self, stream):    # before a reader of the plan is enqueued on `stream`
    stream.wait_event(self._built)

  def _mark_used(self, stream):     # behind a reader of the plan's buffers on `stream`: the next build waits for it
    if self._used is None:
      self._used = torch.cuda.Event()
    self._used.record(stream)

  def partition(self, num_shards, mode=0):
    """The plan's distinct ids grouped by owner (tfra_plan_partition: tfra_partition over the plan's keys, in place of
    tf.unique + dynamic_partition): owner-major ids [n], perm [n] (plan index of each owner-major row), counts
    [num_shards] (device).  Entries past sum(counts) are unspecified.  Runs on the current stream after the build."""
    dev = self._device
    keys_out = torch.empty(self.n, dtype=torch.int64, device=dev)
    perm = torch.empty(self.n, dtype=torch.int32, device=dev)
    counts = torch.zeros(num_shards, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).wait_event(self._built)
    _capi.call("tfra_plan_partition", self._h, _workspace(dev), int(num_shards), int(mode), _ptr(keys_out), _ptr(perm), _ptr(counts),
               _stream(dev))
    return keys_out, perm, counts

  def positions_to(self, perm):
    """dest[p] = j for every batch position p whose id is the key of owner-major row j (tfra_plan_positions_to)."""
    dest = torch.empty(self.n, dtype=torch.int32, device=self._device)
    _capi.call("tfra_plan_positions_to", self._h, _ptr(perm), _ptr(dest), _stream(self._device))
    return dest

  def reduce_to(self, grads, dest, rows_out, sync=True):
    """rows_out[dest[p], :] = sum of the gradient rows of the id at position p (tfra_plan_reduce_to): the per-key sums of
    the plan's batch, scattered by a caller-supplied position -> row map (equal for all positions of an id)."""
    grads = grads.to(self._device, torch.float32).contiguous()
    if grads.numel() != self.n * self._dim:
      raise ValueError("Expected shape %s for grads, got %s" % ([self.n, self._dim], list(grads.shape)))
    if dest.dtype != torch.int32 or dest.numel() != self.n or not dest.is_contiguous():
      raise ValueError("dest must be a contiguous int32 tensor with one entry per id")
    _over_plans((self,), self._device, sync, _capi.call, "tfra_plan_reduce_to", self._h, _ptr(grads), _ptr(dest), _ptr(rows_out),
                _stream(self._device))
    return rows_out

  def read(self):
    """The batch as CSR-by-key, on the host (tests / tools): counts dict, keys [U], cnt [U], positions [n]
    (the positions of key 0, of key 1, ..., each ascending).  Synchronises the current stream."""
    import numpy as np
    counts = (ctypes.c_uint32 * 6)()
    _capi.call("tfra_sparse_plan_read", self._h, counts, None, None, None, 0, _stream(self._device))
    u = counts[0] + counts[1]
    keys = np.empty(u, np.int64)
    cnt = np.empty(u, np.uint32)
    pos = np.empty(self.n, np.uint32) if self._dim else None   # an assign-only plan (dim 0) keeps the last position of a key only
    _capi.call("tfra_sparse_plan_read", self._h, counts, keys.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p),
               pos.ctypes.data_as(ctypes.c_void_p) if pos is not None else None, u, _stream(self._device))
    names = ("many", "few", "partials", "bins", "few_entries", "errors")
    return dict(zip(names, list(counts))), keys, cnt, pos

  def __del__(self):
    try:
      if self._h:
        _capi.call("tfra_sparse_plan_destroy", self._h)
        self._h = None
    except Exception:
      pass


class _LookupInterfaceMirror:
  """Shared method surface of CuckooHashTable / HkvHashTable (tf LookupInterface subclasses)."""

  _table: _DeviceTable

  @property
  def name(self):
    return self._name

  @property
  def key_dtype(self):
    return self._key_dtype

  @property
  def value_dtype(self):
    return self._value_dtype

  @property
  def resource_handle(self):
    return self._table

  def size(self, name=None):
    """Scalar int64 DEVICE tensor (GPU `size_i64`, hkv_hashtable_op_gpu.cu.cc:172-179)."""
    return self._table.size_device()

  def remove(self, keys, name=None):
    """PY/cuckoo_hashtable_ops.py:219-246: absent keys are silently ignored."""
    self._table.erase(keys)

  def clear(self, name=None):
    self._table.clear_all()

  def set_stochastic_rounding(self, seed):
    """Stochastic rounding of the fused optimizer write-backs of a float16 / bfloat16 table (`_DeviceTable.set_stochastic_rounding`):
    seed None or 0 = off.  A tiered table sets its cache table, where the write-backs land; rows that move between the tiers
    are copied, not rounded."""
    self._table.set_stochastic_rounding(seed)

  def lookup(self, keys, dynamic_default_values=None, return_exists=False, name=None, out_dtype=None):
    """PY/cuckoo_hashtable_ops.py:272-340.  out_dtype: `_DeviceTable.find`'s."""
    return self._table.find(keys, dynamic_default_values, return_exists, out_dtype=out_dtype)

  def find_or_insert(self, keys, dynamic_default_values=None, return_exists=False, name=None, count=None):
    """HierarchicalKV's find_or_insert: `lookup` that inserts every key it does not find with the row it returns for it
    (`dynamic_default_values[i]`, else the table's default row), as `insert` would.  Keys must be unique.  Scores follow
    `insert`'s rule.  count: a device int64 count of the leading keys to serve (`_DeviceTable.find_or_insert`)."""
    keys = _as_tensor(keys, self._device)
    return self._table.find_or_insert(keys, dynamic_default_values, scores=self._gen_scores(keys), return_exists=return_exists,
                                      count=count)

  def admit(self, keys, dynamic_default_values=None, count=None):
    """`find_or_insert` without its result (`_DeviceTable.admit`): the unique `keys` become resident, a never-seen key with its
    row of `dynamic_default_values` ([n, dim] or one row; None: the table's default row); no rows are handed back.  Scores as
    `find_or_insert` passes them (`_gen_scores`)."""
    keys = _as_tensor(keys, self._device)
    self._table.admit(keys, dynamic_default_values, scores=self._gen_scores(keys), count=count)

  def find_or_insert_planned(self, plan, dynamic_default_values=None, return_exists=False, name=None):
    """`find_or_insert` of the batch a `SparsePlan` was built over (ids may repeat): every position gets its id's row, an id that
    is not resident enters with the row of its LAST position (`dynamic_default_values[p]`, else the table's default row).  Scores
    follow `insert`'s rule, evaluated per position.  The plan then serves the write-back (`_DeviceTable.find_or_insert_planned`)."""
    return self._table.find_or_insert_planned(plan, dynamic_default_values, scores=self._gen_scores(plan.ids),
                                              return_exists=return_exists)

  def lookup_missed(self, keys, dynamic_default_values=None, name=None):
    """`lookup` that also lists its misses (HierarchicalKV's find with missed_keys / missed_indices): -> (rows, missed_keys,
    missed_indices), the pairs (key, batch position) of the keys that are not resident, in no particular order
    (`_DeviceTable.find_missed`).  Never inserts; an LRU score is not touched."""
    return self._table.find_missed(keys, dynamic_default_values)

  def assign(self, keys, values, name=None):
    """HierarchicalKV's assign: `insert` for the keys that are resident, nothing for the others (they are not inserted and
    nothing is evicted for them).  Keys must be unique.  Scores follow `insert`'s rule."""
    keys = _as_tensor(keys, self._device)
    self._table.assign(keys, values, scores=self._gen_scores(keys))

  def contains(self, keys, name=None):
    """HierarchicalKV's contains: a bool tensor, True where the key is resident.  No row is read."""
    return self._table.contains(keys)

  def _gen_scores(self, keys):   # tables without scores
    return None

  def export(self, name=None):
    k, v, _ = self._table.export_all()
    return k, v

  def _file_prefix(self, dirpath, file_name, dirpath_env):
    # PY/cuckoo_hashtable_ops.py:437-480: env var wins over dirpath; file name defaults to table name
    if dirpath_env:
      dirpath = os.environ.get(dirpath_env, dirpath)
    if not dirpath:
      raise ValueError("dirpath is required")
    os.makedirs(dirpath, exist_ok=True)
    return os.path.join(dirpath, file_name if file_name else self._name)

  def _checkpoint_table(self):
    """The device table whose rows and slot vectors ARE the checkpoint: what is saved from and loaded into, here and by
    `Variable.save_to_file_system` / `load_from_file_system`.  An accessor: it changes nothing.  (A TieredHashTable: its lower table.)"""
    return self._table

  def _checkpoint_flush(self):
    """Called ONCE per shard before `_checkpoint_table()` is read from or has single fields written: afterwards that table alone holds
    everything.  (A TieredHashTable copies its cache down; `save_to_file_system` calls this itself, so the slot files a Variable
    saves behind it need no second flush.)"""

  def _checkpoint_loaded(self):
    """Called once per shard behind the loads into `_checkpoint_table()`.  (A TieredHashTable empties its cache.)"""

  # the per-shard forms of Variable.lookup_missed / Variable.assign: a tiered shard answers for both of its tiers
  def _shard_find_missed(self, keys, defaults, return_exists):
    return self._table.find_missed(keys, defaults, return_exists=return_exists)

  def _shard_assign(self, keys, values, return_found):
    return self._table.assign(keys, values, scores=self._gen_scores(keys), return_found=return_found)

  def save_to_file_system(self, dirpath, file_name=None, dirpath_env="TFRA_SAVED_KV", append_to_file=False,
                          buffer_size=4194304, name=None):
    self._checkpoint_flush()
    return self._checkpoint_table().save(self._file_prefix(dirpath, file_name, dirpath_env), buffer_size, append_to_file)

  def load_from_file_system(self, dirpath, file_name=None, dirpath_env="TFRA_SAVED_KV", load_entire_dir=False,
                            buffer_size=4194304, name=None):
    """load_entire_dir: load every `*-keys` file of the directory (PY/cuckoo_hashtable_ops.py:482-523).
    The GPU op clears the table first (hkv_hashtable_op_gpu.cu.cc:619)."""
    prefix = self._file_prefix(dirpath, file_name, dirpath_env)
    table = self._checkpoint_table()
    table.clear_all()
    if load_entire_dir:
      d = os.path.dirname(prefix)
      total = 0
      for f in sorted(os.listdir(d)):
        if f.endswith("-keys"):
          total += table.load(os.path.join(d, f[:-len("-keys")]), buffer_size)
    else:
      total = table.load(prefix, buffer_size)
    self._checkpoint_loaded()
    return total


class _WholeRows:
  """`fetch_planned` / `store_rows` of a plain table's device table (`_DeviceTable`'s: DESIGN 4.34)."""

  def fetch_planned(self, plan, grads=None, grad_scale=None, fields=None):
    return self._table.fetch_planned(plan, grads=grads, grad_scale=grad_scale, fields=fields)

  def store_rows(self, keys, fields, count=None):
    return self._table.store_rows(keys, fields, count=count)


class CuckooHashTable(_LookupInterfaceMirror, _WholeRows):
  """PY/cuckoo_hashtable_ops.py:45-145.  Growing, never-evicting table (libcuckoo semantics)."""

  def __init__(self, key_dtype, value_dtype, default_value, name="CuckooHashTable", checkpoint=True, init_size=0,
               config=None, device="", shard_saveable_object_fn=None, dim=None, aux_fields=0, aux_init=(0.0,) * 4):
    self._key_dtype = key_dtype
    self._value_dtype = value_dtype
    self._name = name
    self._checkpoint = checkpoint
    self._init_size = init_size
    self._max_capacity = sys.maxsize
    if init_size == 0:
      # K/cuckoo_hashtable_op.cc:199-207: TF_HASHTABLE_INIT_SIZE, default 8192
      init_size = int(os.environ.get("TF_HASHTABLE_INIT_SIZE", 8192))
    self._table = _DeviceTable(key_dtype, value_dtype, default_value, name, device, dim=dim, aux_fields=aux_fields,
                               init_capacity=init_size, max_capacity=0, strategy=-1, aux_init=aux_init)
    self._default_value = self._table._default_value
    self._device = self._table.device

  def insert(self, keys, values, name=None):
    """PY/cuckoo_hashtable_ops.py:342-373.  Duplicate keys: last one wins (sequential CPU order)."""
    self._table.upsert(keys, values)

  def accum(self, keys, values_or_deltas, exists, name=None):
    """PY/cuckoo_hashtable_ops.py:375-412"""
    self._table.accum_or_assign(keys, values_or_deltas, exists)


class HkvHashTable(_LookupInterfaceMirror, _WholeRows):
  """PY/hkv_hashtable_ops.py:47-175.  Bounded table with per-key scores and in-bucket eviction."""

  def __init__(self, key_dtype, value_dtype, default_value, name="HkvHashTable", checkpoint=True,
               init_capacity=KHkvHashTableInitCapacity, max_capacity=KHkvHashTableMaxCapacity,
               max_hbm_for_values=KHkvHashTableMaxHbmForValuesByBytes, config=None, device="",
               shard_saveable_object_fn=None, evict_strategy=HkvEvictStrategy.LRU, step_per_epoch=0, gen_scores_fn=None,
               reserved_key_start_bit=0, dim=None, aux_fields=0, aux_init=(0.0,) * 4):
    if config:
      init_capacity = config.init_capacity
      max_capacity = config.max_capacity
      max_hbm_for_values = config.max_hbm_for_values
      evict_strategy = config.evict_strategy
      step_per_epoch = config.step_per_epoch
      gen_scores_fn = config.gen_scores_fn
      reserved_key_start_bit = config.reserved_key_start_bit
    self._key_dtype = key_dtype
    self._value_dtype = value_dtype
    self._scores_dtype = torch.int64
    self._name = name
    self._checkpoint = checkpoint
    self._init_capacity = init_capacity
    self._max_capacity = max_capacity
    self._max_hbm_for_values = max_hbm_for_values
    self._evict_strategy = HkvEvictStrategy(evict_strategy)
    self._step_per_epoch = step_per_epoch
    self._gen_scores_fn = gen_scores_fn
    self._reserved_key_start_bit = reserved_key_start_bit
    if max_capacity == 0:
      # hkv_hashtable_op_gpu.cu.cc:104-120
      env = os.environ.get("TFRA_GPU_HASHTABLE_UPLIMIT_SIZE")
      if env is None:
        raise ValueError("max_capaicty=0 and TFRA_GPU_HASHTABLE_UPLIMIT_SIZE not set is not valid.")
      max_capacity = int(env)
    self._table = _DeviceTable(key_dtype, value_dtype, default_value, name, device, dim=dim, aux_fields=aux_fields,
                               init_capacity=init_capacity, max_capacity=max_capacity,
                               max_hbm_for_values=max_hbm_for_values, strategy=int(self._evict_strategy),
                               step_per_epoch=step_per_epoch, reserved_key_start_bit=reserved_key_start_bit,
                               aux_init=aux_init)
    self._default_value = self._table._default_value
    self._device = self._table.device

  def _gen_scores(self, keys):
    """PY/hkv_hashtable_ops.py:209-217"""
    if self._evict_strategy == HkvEvictStrategy.CUSTOMIZED:
      assert self._gen_scores_fn is not None, "You must set gen_scores_fn when set evict strategy to CUSTOMIZED"
      return self._gen_scores_fn(keys)
    if self._evict_strategy in (HkvEvictStrategy.LFU, HkvEvictStrategy.EPOCHLFU):
      return torch.ones(keys.shape, dtype=torch.int64, device=keys.device)
    return None

  def insert(self, keys, values, name=None):
    """PY/hkv_hashtable_ops.py:339-367"""
    keys = self._table._keys(keys)
    # HKV requires unique keys per call (PY/dynamic_embedding_variable.py:1377-1378); with that contract
    # a full bounded table can evict by score
    self._table.upsert(keys, values, scores=self._gen_scores(keys), unique_keys=True)

  def insert_and_evict(self, keys, values, scores=None, name=None):
    """insert that returns (evicted_keys, evicted_values, evicted_scores): what left the table because of this call and what it
    did not admit (HierarchicalKV's insert_and_evict).  scores: as the engine takes them; None = gen_scores_fn / the strategy's."""
    keys = _as_tensor(keys, self._device)
    return self._table.upsert_and_evict(keys, values, scores=self._gen_scores(keys) if scores is None else scores)

  def assign(self, keys, values, scores=None, name=None):
    """HierarchicalKV's assign: the resident keys get their rows and their scores are touched as `insert` touches them; the
    others change nothing.  scores: as the engine takes them; None = gen_scores_fn / the strategy's."""
    keys = _as_tensor(keys, self._device)
    self._table.assign(keys, values, scores=self._gen_scores(keys) if scores is None else scores)

  def accum(self, keys, values_or_deltas, exists, name=None):
    """PY/hkv_hashtable_ops.py:369-402"""
    keys = self._table._keys(keys)
    self._table.accum_or_assign(keys, values_or_deltas, exists, scores=self._gen_scores(keys), unique_keys=True)

  def export_keys_and_scores(self, split_size, name=None):
    """PY/hkv_hashtable_ops.py:421-434"""
    k, _, s = self._export_split(split_size, values=False)
    return k, s

  def export_with_scores(self, split_size, name=None):
    """PY/hkv_hashtable_ops.py:436-450"""
    return self._export_split(split_size, values=True)

  def _export_split(self, split_size, values):
    if not (isinstance(split_size, int) and split_size > 0):
      raise ValueError("split_size must be positive integer.")
    return self._table.export_all(with_scores=True, values=values, split_size=split_size)

  # ---- score-filtered forms (HKV export_batch_if / erase_if / size_if) ------------------------
  def export_if(self, threshold, pred="ge", name=None):
    """(keys, values, scores) of the entries with score >= threshold ("ge") or < threshold ("lt")."""
    return self._table.export_if(threshold, pred)

  def remove_if(self, threshold, pred="lt", name=None):
    """Erases the matching entries; returns their number as a device int64 tensor of shape [1]."""
    return self._table.erase_if(threshold, pred)

  def size_if(self, threshold, pred="ge", name=None):
    """Number of matching entries as a device int64 tensor of shape [1]."""
    return self._table.count_if(threshold, pred)

  def save_delta_to_file_system(self, dirpath, threshold, pred="ge", file_name=None, dirpath_env="TFRA_SAVED_KV",
                                append_to_file=False, buffer_size=4194304, name=None):
    """save_to_file_system of the matching entries only (same path and naming rules, same files): a delta checkpoint in the
    format load_from_file_system reads (that call clears first; the device table's `load` merges over what is resident).
    Erased keys are not recorded; scores are not written."""
    return self._table.save_if(self._file_prefix(dirpath, file_name, dirpath_env), threshold, pred, buffer_size, append_to_file)


def _export_or_empty(table, values=True):
  """(keys, rows) of a _DeviceTable's export_all; an empty table exports two empty tensors (export_batch refuses a buffer of no
  bytes)."""
  if table.size_host() == 0:
    return (torch.empty(0, dtype=table._key_dtype, device=table._device),
            torch.empty((0, table._dim), dtype=table._value_dtype, device=table._device) if values else None)
  k, v, _ = table.export_all(values=values)
  return k, v


class TieredHashTable(_LookupInterfaceMirror):
  """Two tiers behind one table interface: `_table`, a bounded LRU / EPOCHLRU _DeviceTable at max_capacity (the cache: the fused
  write-backs, `_device_table` and the slot views act on it), in front of `_lower`, a growing _DeviceTable that holds every key
  the cache does not, driven by `_tier` (a _DeviceTier).  Whole co-located rows move between the two, so a key that is demoted
  and promoted again keeps its optimizer slots.  After every call that goes through this class, for every key ever written: the
  upper table holds its newest whole row if it contains the key, otherwise the lower one does.
  `find_or_insert` — the lookup of a training step — leaves every key of the batch resident in the upper table, so the
  write-back of the step only hits.  One limit, next to "not resident at write-back time": a batch that fills both home buckets
  of one of its own keys with its own keys (30 slots) cannot keep that key up; its row is below and a fused write-back restarts
  it from the default row (`_DeviceTier.find_or_insert(verify=True)` counts such keys).
  config: a TieredHashTableConfig (`upper`: an HkvHashTableConfig, `max_batch`: the most keys one call may carry)."""

  def __init__(self, key_dtype, value_dtype, default_value, name="TieredHashTable", checkpoint=True, config=None, device="",
               shard_saveable_object_fn=None, dim=None, aux_fields=0, aux_init=(0.0,) * 4, init_size=0):
    if config is None:
      raise ValueError("TieredHashTable needs a TieredHashTableConfig")
    up = config.upper
    self._key_dtype, self._value_dtype, self._name, self._checkpoint = key_dtype, value_dtype, name, checkpoint
    self._evict_strategy = HkvEvictStrategy(up.evict_strategy)
    self._table = _DeviceTable(key_dtype, value_dtype, default_value, name, device, dim=dim, aux_fields=aux_fields,
                               init_capacity=up.init_capacity, max_capacity=up.max_capacity, max_hbm_for_values=up.max_hbm_for_values,
                               strategy=int(self._evict_strategy), step_per_epoch=up.step_per_epoch,
                               reserved_key_start_bit=up.reserved_key_start_bit, aux_init=aux_init)
    self._lower = _DeviceTable(key_dtype, value_dtype, default_value, name + "_lower", device, dim=dim, aux_fields=aux_fields,
                               init_capacity=init_size or int(os.environ.get("TF_HASHTABLE_INIT_SIZE", 8192)), max_capacity=0,
                               strategy=-1, aux_init=aux_init)
    self._tier = _DeviceTier(self._table, self._lower, config.max_batch)
    self._aux_fields = aux_fields
    self._default_value = self._table._default_value
    self._device = self._table.device

  def _chunks(self, n):
    mb = self._tier.max_batch
    return [(a, min(a + mb, n)) for a in range(0, n, mb)]

  def size(self, name=None):
    """The number of distinct keys of the two tiers, a scalar int64 device tensor."""
    uk, _ = _export_or_empty(self._table, values=False)
    below = self._lower.size_device()
    return below + (~self._lower.contains(uk)).sum() if uk.numel() else below

  def remove(self, keys, name=None):
    self._table.erase(keys)
    self._lower.erase(keys)

  def clear(self, name=None):
    self._table.clear_all()
    self._lower.clear_all()

  def lookup(self, keys, dynamic_default_values=None, return_exists=False, name=None):
    """A read of both tiers (`_DeviceTier.find`): nothing moves.  (No out_dtype here: the tier calls are not typed, and
    `Variable.lookup` converts a tiered shard's rows behind this call.)"""
    keys = _as_tensor(keys, self._device)
    flat = keys.reshape(-1)
    n, dim = flat.numel(), self._table.dim
    d = dynamic_default_values
    full = d is not None and torch.is_tensor(d) and d.numel() == n * dim and n > 1
    rows = torch.empty((n, dim), dtype=self._value_dtype, device=self._device)
    where = torch.zeros(n, dtype=torch.uint8, device=self._device)
    for a, b in self._chunks(n):
      r, w = self._tier.find(flat[a:b], d.reshape(n, dim)[a:b] if full else d, return_where=True)
      rows[a:b], where[a:b] = r, w
    rows = rows.reshape(tuple(keys.shape) + (dim,))
    return (rows, (where != 0).reshape(keys.shape)) if return_exists else rows

  def find_or_insert(self, keys, dynamic_default_values=None, return_exists=False, name=None, count=None):
    """The admitting lookup through both tiers (`_DeviceTier.find_or_insert`): UNIQUE keys, at most `max_batch` of them.  exists[i]
    is False for a key neither tier held."""
    keys = _as_tensor(keys, self._device)
    rows, where = self._tier.find_or_insert(keys, dynamic_default_values, return_where=True, count=count)
    return (rows, where != 0) if return_exists else rows

  def find_or_insert_planned(self, plan, dynamic_default_values=None, return_exists=False, name=None):
    """`find_or_insert` of the batch a `SparsePlan` was built over (ids may repeat, at most `max_batch` of them), through both
    tiers (`_DeviceTier.find_or_insert_planned`): every position gets its id's row, an id neither tier held enters with the row of
    its LAST position (`dynamic_default_values[p]`, else the table's default row).  exists[p] is False for such an id.  The plan
    then serves the write-back on the cache."""
    if not return_exists:
      return self._tier.find_or_insert_planned(plan, dynamic_default_values)
    rows, where = self._tier.find_or_insert_planned(plan, dynamic_default_values, return_where=True)
    return rows, where != 0

  def admit_planned(self, plan, init_values=None, verify=False):
    """`find_or_insert_planned` that hands no rows back (`_DeviceTier.admit_planned`): afterwards every distinct id of the plan is
    in the cache with its whole row."""
    self._tier.admit_planned(plan, init_values, verify=verify)

  def admit(self, keys, init_values=None, count=None, verify=False):
    """`find_or_insert` that hands no rows back (`_DeviceTier.admit`): UNIQUE keys, at most `max_batch`; afterwards each is in the
    cache with its whole row.  What a pooled training step runs over its entry ids before `find_combine`."""
    self._tier.admit(_as_tensor(keys, self._device), init_values, count=count, verify=verify)

  def find_combine(self, ids, seg, weights, combiner, n_rows, default_row=None):
    """The pooled lookup over both tiers (`_DeviceTier.find_combine`): a read, nothing moves."""
    return self._tier.find_combine(ids, seg, weights, combiner, n_rows, default_row)

  def find_combine_typed(self, ids, seg, weights, combiner, n_rows, default_row=None, out_dtype=None):
    """`find_combine` converted to out_dtype (`_DeviceTier.find_combine_typed`)."""
    return self._tier.find_combine_typed(ids, seg, weights, combiner, n_rows, default_row, out_dtype=out_dtype)

  def find_combine_ragged(self, row_splits, ids, weights, combiner, prune=False, fill_id=None, default_row=None, out_dtype=None):
    """The ragged pooled lookup over both tiers (`_DeviceTier.find_combine_ragged`): a read, nothing moves."""
    return self._tier.find_combine_ragged(row_splits, ids, weights, combiner, prune=prune, fill_id=fill_id, default_row=default_row,
                                          out_dtype=out_dtype)

  def find_combine_weight_grad(self, ids, seg, weights, combiner, grad_out, default_row=None):
    """The gradient of `find_combine` with respect to its weights, over both tiers (`_DeviceTier.find_combine_weight_grad`): a
    read, nothing moves."""
    return self._tier.find_combine_weight_grad(ids, seg, weights, combiner, grad_out, default_row)

  def find_combine_ragged_weight_grad(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                      default_row=None):
    """The same gradient for `find_combine_ragged` (`_DeviceTier.find_combine_ragged_weight_grad`): a read, nothing moves."""
    return self._tier.find_combine_ragged_weight_grad(row_splits, ids, weights, combiner, grad_out, prune=prune, fill_id=fill_id,
                                                      default_row=default_row)

  def find_combine_weight_grad_typed(self, ids, seg, weights, combiner, grad_out, default_row=None, grad_scale=None):
    """`find_combine_weight_grad` with a half grad_out as it is (`_DeviceTier.find_combine_weight_grad_typed`): a read."""
    return self._tier.find_combine_weight_grad_typed(ids, seg, weights, combiner, grad_out, default_row, grad_scale=grad_scale)

  def find_combine_ragged_weight_grad_typed(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                            default_row=None, grad_scale=None):
    """The same for `find_combine_ragged` (`_DeviceTier.find_combine_ragged_weight_grad_typed`): a read."""
    return self._tier.find_combine_ragged_weight_grad_typed(row_splits, ids, weights, combiner, grad_out, prune=prune,
                                                            fill_id=fill_id, default_row=default_row, grad_scale=grad_scale)

  def lookup_missed(self, keys, dynamic_default_values=None, name=None):
    """`lookup` plus the pairs (key, position) that NEITHER tier holds (one host read for their number)."""
    return self._shard_find_missed(keys, dynamic_default_values, False)

  def _shard_find_missed(self, keys, defaults, return_exists):
    keys = _as_tensor(keys, self._device)
    rows, exists = self.lookup(keys, defaults, return_exists=True)
    mi = torch.nonzero(~exists.reshape(-1)).reshape(-1)
    out = (rows, keys.reshape(-1)[mi], mi.to(torch.int32))
    return out + (exists,) if return_exists else out

  def insert(self, keys, values, name=None):
    """upsert of embedding rows (UNIQUE keys) into the cache; what that displaces goes down with its slots (`_DeviceTier.insert`)."""
    keys = _as_tensor(keys, self._device)
    values = _as_tensor(values, self._device)
    flat, n = keys.reshape(-1), keys.numel()
    vals = values.reshape(n, self._table.dim)
    for a, b in self._chunks(n):
      self._tier.insert(flat[a:b], vals[a:b])

  def assign(self, keys, values, name=None):
    """The write that only hits, in both tiers: a key the cache holds gets its row there, and whatever copy the lower tier has is
    overwritten too (a stale copy of a promoted key is never read: the upper table wins)."""
    self._shard_assign(keys, values, False)

  def _shard_assign(self, keys, values, return_found):
    keys = _as_tensor(keys, self._device)
    up = self._table.assign(keys, values, return_found=return_found)
    lo = self._lower.assign(keys, values, return_found=return_found)
    return (up | lo) if return_found else None

  def accum(self, keys, values_or_deltas, exists, name=None):
    raise NotImplementedError("TieredHashTable does not serve accum (bp_v2)")

  def contains(self, keys, name=None):
    return self._table.contains(keys) | self._lower.contains(keys)

  def export(self, name=None):
    """The lower tier's export with the upper tier's rows over it."""
    uk, uv = _export_or_empty(self._table)
    lk, lv = _export_or_empty(self._lower)
    if not uk.numel() or not lk.numel():
      return (lk, lv) if not uk.numel() else (uk, uv)
    keep = ~self._table.contains(lk)
    return torch.cat([uk, lk[keep]]), torch.cat([uv, lv[keep]])

  def flush(self):
    """Every key of the cache gets its whole row copied to the lower tier, field by field (export, find(field=), upsert(field=)):
    afterwards the lower table alone holds everything.  The cache is unchanged."""
    uk, uv = _export_or_empty(self._table)
    if not uk.numel():
      return
    self._lower.upsert(uk, uv, unique_keys=True)
    for f in range(1, self._aux_fields + 1):
      self._lower.upsert(uk, self._table.find(uk, field=f), field=f)

  def _checkpoint_table(self):
    return self._lower

  def _checkpoint_flush(self):
    self.flush()

  def _checkpoint_loaded(self):
    self._table.clear_all()   # everything was loaded below: the cache fills again from there


def _wgrad_typed(owner, table, c_name, ids, seg, weights, combiner, grad_out, default_row, grad_scale):
  """The frame of `find_combine_weight_grad_typed` for a table (owner is table) and a tier (table: its upper table, which prepares
  the operands): `c_name`_typed when grad_out goes down as a half matrix, `c_name` on the float32 up-cast otherwise."""
  typed, g = table._weight_grad_out(grad_out, None, keep_half=True, grad_scale=grad_scale)
  ids, seg, w, d, _ = table._find_combine_args(ids, seg, weights, 0, default_row)
  dw = torch.empty(ids.numel(), dtype=torch.float32, device=table._device)
  _capi.call(c_name + ("_typed" if typed is not None else ""), owner._h, _workspace(table._device), ids.numel(), _ptr(ids), _ptr(seg),
             _ptr(w), int(combiner), g.shape[0], _ptr(d), (ctypes.byref(typed) if typed is not None else _ptr(g)), _ptr(dw),
             _stream(table._device))
  return dw


def _wgrad_ragged_typed(owner, table, c_name, row_splits, ids, weights, combiner, grad_out, prune, fill_id, default_row, grad_scale):
  """`_wgrad_typed` for the ragged calls."""
  rs, ids, w, flags, fill, d, _ = table._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row)
  typed, g = table._weight_grad_out(grad_out, rs.numel() - 1, keep_half=True, grad_scale=grad_scale)
  dw = torch.empty(ids.numel(), dtype=torch.float32, device=table._device)
  _capi.call(c_name + ("_typed" if typed is not None else ""), owner._h, rs.numel() - 1, _ptr(rs), ids.numel(), _ptr(ids), _ptr(w),
             int(combiner), flags, fill, _ptr(d), (ctypes.byref(typed) if typed is not None else _ptr(g)), _ptr(dw),
             _stream(table._device))
  return dw


def _device_table(x):
  """`x` if it is a _DeviceTable, the device table of a CuckooHashTable / HkvHashTable (a TieredHashTable: its cache, which is what
  a write-back acts on; a pooled READ of a tiered owner goes through `_device_tier`)."""
  return getattr(x, "_table", x)


def _device_tier(x):
  """The _DeviceTier behind a tiered owner of a pooled read — a TieredHashTable's driver, or `x` if it is a _DeviceTier —, else
  None: the owner is one table (`_device_table`)."""
  if isinstance(x, _DeviceTier):
    return x
  return x._tier if isinstance(x, TieredHashTable) else None


def _owner_device(x):
  """The device of a grouped call's owner: a tier's is its upper table's (both tables of a tier live on one device)."""
  tier = _device_tier(x)
  return tier._upper._device if tier is not None else _device_table(x)._device


def _pooled_owner(e, owner, tiered):
  """Sets the owner of a pooled descriptor `e` — `tiered`: of the tier ABI (`_capi.TierFindCombineDesc` / `...RaggedDesc`), which
  names exactly one of table / tier — and returns the _DeviceTable that prepares the operands: the owner's device table, or a
  tier's upper table."""
  tier = _device_tier(owner)
  table = tier._upper if tier is not None else _device_table(owner)
  if tiered:
    e.table, e.tier = (None, tier._h.value) if tier is not None else (table._h.value, None)
  else:
    e.table = table._h.value
  return table


def _grouped_call(c_name, desc_type, who, owners, fill):
  """The frame of the grouped calls (`find_combine_many`, `find_combine_ragged_many`, their `*_weight_grad_many` forms,
  `apply_planned_combined_many`, `build_plans_many`): ONE C call `c_name(workspace, n, descs, &launches, stream)` over one descriptor of `desc_type` per entry of
  `owners`, on the current stream of the one device all of them live on.  An owner is a _DeviceTable, a CuckooHashTable /
  HkvHashTable (whose device table is taken: `_device_table`), a TieredHashTable / _DeviceTier (the pooled reads: `_device_tier`)
  or a SparsePlan.  Member by member, the owner's device (`_owner_device`) is compared
  with the first one's (ValueError in the name of `who`), then `fill(descs[i], i)` checks the member's arguments and sets the
  descriptor's fields behind struct_size.  What `fill` returns — the tensors whose data_ptr() it stored — stays referenced here
  until the C call has returned.  Returns the number of kernel launches the call enqueued."""
  descs = (desc_type * len(owners))()
  keep, device = [], _owner_device(owners[0])
  for i, owner in enumerate(owners):
    dev = _owner_device(owner)
    if dev != device:
      raise ValueError("%s: all tables must live on one device (%s and %s)" % (who, device, dev))
    descs[i].struct_size = ctypes.sizeof(desc_type)
    keep.append(fill(descs[i], i))
  launches = ctypes.c_uint32(0)
  _capi.call(c_name, _workspace(device), len(owners), ctypes.c_void_p(ctypes.addressof(descs)),
             ctypes.c_void_p(ctypes.addressof(launches)), _stream(device))
  return int(launches.value)


def _out_dtypes(out_dtype, n):
  """The `out_dtype=` of a grouped lookup as one entry per request: one dtype for the list, or a list of n (None: float32, the
  request's own type).  None when every entry is None: today's call."""
  dts = list(out_dtype) if isinstance(out_dtype, (list, tuple)) else [out_dtype] * n
  if len(dts) != n:
    raise ValueError("out_dtype must be one dtype or one per request: %d for %d requests" % (len(dts), n))
  dts = [_out_dtype(d) for d in dts]
  return None if all(d is None for d in dts) else dts


def _converted(result, dts, return_launches):
  """The results of an untyped grouped lookup, each converted to its request's out_dtype (a list with a tiered member)."""
  outs = result[0] if return_launches else result
  outs = [o if d is None else o.to(d) for o, d in zip(outs, dts)]
  return (outs, result[1]) if return_launches else outs


def find_combine_many(requests, return_launches=False, out_dtype=None):
  """The pooled lookups of a list of tables in ONE C call (tfra_multi_find_combine; the frame: `_grouped_call`).  `requests`: a
  list of (table, ids, seg, weights, combiner, n_rows[, default_row]), the arguments behind `table` those of
  `_DeviceTable.find_combine`, handled the same way (int32 keys widened, the default row falling back to the table's).  Returns
  the [n_rows, dim] float32 results in the requests' order, each bit-identical to `find_combine` of its request (with
  return_launches: also the number of kernel launches the call enqueued — it does not grow with the list).
  `table` may be a TieredHashTable or a _DeviceTier: its request is read in BOTH tiers, bit-identical to the tier's `find_combine`
  (the operands prepared by the upper table).  A list with a tiered owner goes through tfra_multi_tier_find_combine as a whole,
  plain tables included — still one call; a list without one takes the call, the descriptor and the launch counts it always took.
  out_dtype: one of float32 / float16 / bfloat16 for the list, or one per request (None: float32): each result in that type,
  rounded in the lookup's kernel (tfra_multi_find_combine_typed), bit for bit `result.to(out_dtype)`; the output type is one more
  launch-class axis, so a list with one output type keeps its launch count.  The tier calls are not typed: a list with a tiered
  member runs untyped as a whole and each result is converted."""
  if not requests:
    return ([], 0) if return_launches else []
  outs = []
  tiered = any(_device_tier(r[0]) is not None for r in requests)
  dts = _out_dtypes(out_dtype, len(requests))
  if dts is not None and tiered:
    return _converted(find_combine_many(requests, return_launches), dts, return_launches)

  def fill(e, i):
    req = requests[i]
    table, ids, seg, weights, combiner, n_rows = req[:6]
    default_row = req[6] if len(req) > 6 else None
    table = _pooled_owner(e, table, tiered)
    ids, seg, w, d, out = table._find_combine_args(ids, seg, weights, n_rows, default_row, dts[i] if dts else None)
    outs.append(out)
    e.combiner = int(combiner)
    e.nnz, e.ids, e.seg, e.weights = ids.numel(), ids.data_ptr(), seg.data_ptr(), (w.data_ptr() if w is not None else None)
    e.n_rows, e.default_row, e.out = int(n_rows), d.data_ptr(), (_rows_out(out) if dts else out.data_ptr())
    return ids, seg, w, d

  c_name, desc_type = (("tfra_multi_tier_find_combine", _capi.TierFindCombineDesc) if tiered else
                       ("tfra_multi_find_combine_typed", _capi.FindCombineTypedDesc) if dts else
                       ("tfra_multi_find_combine", _capi.FindCombineDesc))
  launches = _grouped_call(c_name, desc_type, "find_combine_many", [r[0] for r in requests], fill)
  return (outs, launches) if return_launches else outs


def find_combine_ragged_many(requests, return_launches=False, out_dtype=None):
  """The ragged pooled lookups of a list of tables in ONE C call (tfra_multi_find_combine_ragged; the frame: `_grouped_call`).
  `requests`: a list of (table, row_splits, ids, weights, combiner[, prune[, fill_id[, default_row]]]), the arguments behind
  `table` those of `_DeviceTable.find_combine_ragged`, handled the same way.  A table may occur more than once.  Returns the
  [n_rows, dim] float32 results in the requests' order, each bit-identical to `find_combine_ragged` of its request (with
  return_launches: also the number of kernel launches the call enqueued: one per (value dtype, row-width class, safe-or-not)
  class in the list).  `table` may be a TieredHashTable or a _DeviceTier, as in `find_combine_many`: the request is read in both
  tiers, the fill id too, and the whole list goes through tfra_multi_tier_find_combine_ragged (one launch per (tiered or not,
  value dtype, row-width class, safe-or-not) class); a list without a tiered owner takes the call it always took.
  out_dtype: as `find_combine_many`'s (tfra_multi_find_combine_ragged_typed)."""
  if not requests:
    return ([], 0) if return_launches else []
  outs = []
  tiered = any(_device_tier(r[0]) is not None for r in requests)
  dts = _out_dtypes(out_dtype, len(requests))
  if dts is not None and tiered:
    return _converted(find_combine_ragged_many(requests, return_launches), dts, return_launches)

  def fill(e, i):
    req = requests[i]
    table, row_splits, ids, weights, combiner = req[:5]
    prune = req[5] if len(req) > 5 else False
    fill_id = req[6] if len(req) > 6 else None
    default_row = req[7] if len(req) > 7 else None
    table = _pooled_owner(e, table, tiered)
    rs, ids, w, flags, fill_key, d, out = table._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row,
                                                                          dts[i] if dts else None)
    outs.append(out)
    e.combiner = int(combiner)
    e.n_rows, e.row_splits = rs.numel() - 1, rs.data_ptr()
    e.nnz, e.ids, e.weights = ids.numel(), ids.data_ptr(), (w.data_ptr() if w is not None else None)
    e.flags, e.reserved, e.fill_id = flags, 0, fill_key
    e.default_row, e.out = d.data_ptr(), (_rows_out(out) if dts else out.data_ptr())
    return rs, ids, w, d

  c_name, desc_type = (("tfra_multi_tier_find_combine_ragged", _capi.TierFindCombineRaggedDesc) if tiered else
                       ("tfra_multi_find_combine_ragged_typed", _capi.FindCombineRaggedTypedDesc) if dts else
                       ("tfra_multi_find_combine_ragged", _capi.FindCombineRaggedDesc))
  launches = _grouped_call(c_name, desc_type, "find_combine_ragged_many", [r[0] for r in requests], fill)
  return (outs, launches) if return_launches else outs


def _request_scales(who, grad_scale, n):
  """grad_scale of a grouped call as one entry per request: one scale for all, or a list with one (or None) per request."""
  scales = list(grad_scale) if isinstance(grad_scale, (list, tuple)) else [grad_scale] * n
  if len(scales) != n:
    raise ValueError("%s: %d requests but %d gradient scales" % (who, n, len(scales)))
  return scales


def _pooled_table(owner):
  """The _DeviceTable that prepares a pooled request's operands: the owner's device table, or a tier's upper table."""
  tier = _device_tier(owner)
  return tier._upper if tier is not None else _device_table(owner)


def _request_grads(who, requests, grad_scale, n_rows_of):
  """What the grouped weight gradients decide before the descriptors exist, because which C call it is depends on it: each
  request's gradient as `_weight_grad_out(..., keep_half=True)` prepares it — (tfra_grads or None, tensor), n_rows_of(request) the
  row count it must have (None: its own) — and whether any of them goes down as a half matrix.  The owners are looked at first, in
  the order and with the error `_grouped_call` has for them: a bad owner fails as it did before the gradients were prepared here."""
  scales = _request_scales(who, grad_scale, len(requests))
  device = _owner_device(requests[0][0])
  for r in requests:
    dev = _owner_device(r[0])
    if dev != device:
      raise ValueError("%s: all tables must live on one device (%s and %s)" % (who, device, dev))
  grads = [_pooled_table(r[0])._weight_grad_out(r[5], n_rows_of(r), keep_half=True, grad_scale=sc) for r, sc in zip(requests, scales)]
  return grads, any(t is not None for t, _ in grads)


def _splits_rows(row_splits):
  """n_rows of a ragged request, from the shape of its row_splits alone (None where `_find_combine_ragged_args` will refuse it)."""
  n = torch.as_tensor(row_splits).numel()
  return n - 1 if n >= 1 else None


def find_combine_weight_grad_many(requests, return_launches=False, grad_scale=None):
  """The weight gradients of a list of pooled lookups in ONE C call (tfra_multi_find_combine_backprop_weights; the frame:
  `_grouped_call`).  `requests`: a list of (table, ids, seg, weights, combiner, grad_out[, default_row]), the arguments behind
  `table` those of `_DeviceTable.find_combine_weight_grad`, handled the same way (n_rows is grad_out's).  `table` is a table, a
  TieredHashTable or a _DeviceTier (read in both tiers), in any mix; a table or tier may occur more than once.  Returns the
  float32 [nnz] gradients in the requests' order, each bit-identical to `find_combine_weight_grad` of its request (with
  return_launches: also the number of kernel launches the call enqueued: one that zero-fills all results and writes all rows'
  bounds, and one per (tiered or not, value dtype, row-width class) class in the list).
  grad_scale: one scale for all requests, or a list with one (or None) per request, as `find_combine_weight_grad_typed` takes it.
  As soon as one request's grad_out goes down as a half matrix (contiguous float16 / bfloat16), the call is
  tfra_multi_find_combine_backprop_weights_typed — float32 members ride along as float32 descriptors, float-or-half being one
  more launch-class axis —; otherwise it is the untyped call, as always."""
  if not requests:
    return ([], 0) if return_launches else []
  dws = []
  grads, any_typed = _request_grads("find_combine_weight_grad_many", requests, grad_scale, lambda r: None)

  def fill(e, i):
    req = requests[i]
    table, ids, seg, weights, combiner = req[:5]
    default_row = req[6] if len(req) > 6 else None
    table = _pooled_owner(e, table, True)
    typed, g = grads[i]
    ids, seg, w, d, _ = table._find_combine_args(ids, seg, weights, 0, default_row)
    dw = torch.empty(ids.numel(), dtype=torch.float32, device=table._device)
    dws.append(dw)
    e.combiner = int(combiner)
    e.nnz, e.ids, e.seg, e.weights = ids.numel(), ids.data_ptr(), seg.data_ptr(), (w.data_ptr() if w is not None else None)
    e.n_rows, e.default_row, e.dw_out = g.shape[0], d.data_ptr(), dw.data_ptr()
    e.grad_out = _grads_field(typed, g, any_typed)
    return ids, seg, w, d, g

  c_name, desc_type = (("tfra_multi_find_combine_backprop_weights_typed", _capi.FindCombineWgradTypedDesc) if any_typed else
                       ("tfra_multi_find_combine_backprop_weights", _capi.FindCombineWgradDesc))
  launches = _grouped_call(c_name, desc_type, "find_combine_weight_grad_many", [r[0] for r in requests], fill)
  return (dws, launches) if return_launches else dws


def _grads_field(typed, g, any_typed):
  """A descriptor's grad_out: the tensor's address in an untyped list; in a typed one its tfra_grads, a float32 member's formed here."""
  if not any_typed:
    return g.data_ptr()
  return typed if typed is not None else _capi.Grads(g.data_ptr(), _capi.TFRA_F32, 0, None)


def find_combine_ragged_weight_grad_many(requests, return_launches=False, grad_scale=None):
  """The weight gradients of a list of ragged pooled lookups in ONE C call (tfra_multi_find_combine_ragged_backprop_weights; the
  frame: `_grouped_call`).  `requests`: a list of (table, row_splits, ids, weights, combiner, grad_out[, prune[, fill_id[,
  default_row]]]), the arguments behind `table` those of `_DeviceTable.find_combine_ragged_weight_grad`, handled the same way;
  `table` as in `find_combine_weight_grad_many`.  Returns the float32 [nnz] gradients in the requests' order, each bit-identical
  to `find_combine_ragged_weight_grad` of its request (with return_launches: also the number of kernel launches: one that
  zero-fills all results and one per (tiered or not, value dtype, row-width class, pruning or not) class in the list).
  grad_scale and half gradients as in `find_combine_weight_grad_many` (tfra_multi_find_combine_ragged_backprop_weights_typed)."""
  if not requests:
    return ([], 0) if return_launches else []
  dws = []
  grads, any_typed = _request_grads("find_combine_ragged_weight_grad_many", requests, grad_scale, lambda r: _splits_rows(r[1]))

  def fill(e, i):
    req = requests[i]
    table, row_splits, ids, weights, combiner = req[:5]
    prune = req[6] if len(req) > 6 else False
    fill_id = req[7] if len(req) > 7 else None
    default_row = req[8] if len(req) > 8 else None
    table = _pooled_owner(e, table, True)
    rs, ids, w, flags, fill_key, d, _ = table._find_combine_ragged_args(row_splits, ids, weights, prune, fill_id, default_row)
    typed, g = grads[i]
    dw = torch.empty(ids.numel(), dtype=torch.float32, device=table._device)
    dws.append(dw)
    e.combiner = int(combiner)
    e.n_rows, e.row_splits = rs.numel() - 1, rs.data_ptr()
    e.nnz, e.ids, e.weights = ids.numel(), ids.data_ptr(), (w.data_ptr() if w is not None else None)
    e.flags, e.reserved, e.fill_id = flags, 0, fill_key
    e.default_row, e.dw_out = d.data_ptr(), dw.data_ptr()
    e.grad_out = _grads_field(typed, g, any_typed)
    return rs, ids, w, d, g

  c_name, desc_type = (("tfra_multi_find_combine_ragged_backprop_weights_typed", _capi.FindCombineRaggedWgradTypedDesc) if any_typed
                       else ("tfra_multi_find_combine_ragged_backprop_weights", _capi.FindCombineRaggedWgradDesc))
  launches = _grouped_call(c_name, desc_type, "find_combine_ragged_weight_grad_many", [r[0] for r in requests], fill)
  return (dws, launches) if return_launches else dws


def apply_planned_combined_many(requests, p_list, sync=True, grad_scale=None):
  """The combined write-backs of a list of tables in ONE C call (tfra_multi_apply_planned_combined; the frame: `_grouped_call`).
  grad_scale: one scale for all requests, or a list with one (or None) per request, as in `apply_planned_combined`.  When a
  request's grad_out goes down as a half matrix, the call is tfra_multi_apply_planned_combined_typed (float32 members ride along as
  float32 descriptors); otherwise it is the untyped call, as always.
  `requests`: a list of (table, plan, grad_out, seg, weights, combiner, default_row), the arguments behind `table` those of
  `_DeviceTable.apply_planned_combined`, handled the same way.  `p_list`: the optimizer parameters (`_capi.OptParams`) of each
  request, or one for all.  Each table and each plan occurs once.  Every table ends bit-identical to `apply_planned_combined` of
  its request.  Returns the number of kernel launches the call enqueued — it does not grow with the list."""
  n = len(requests)
  if n == 0:
    return 0
  if isinstance(p_list, _capi.OptParams):
    p_list = [p_list] * n
  if len(p_list) != n:
    raise ValueError("apply_planned_combined_many: %d requests but %d optimizer parameter sets" % (n, len(p_list)))
  scales = list(grad_scale) if isinstance(grad_scale, (list, tuple)) else [grad_scale] * n
  if len(scales) != n:
    raise ValueError("apply_planned_combined_many: %d requests but %d gradient scales" % (n, len(scales)))
  # the arguments first: which call it is depends on how the gradients go down
  args = []
  for (table, plan, grad_out, seg, weights, combiner, default_row), scale in zip(requests, scales):
    args.append(_device_table(table)._apply_combined_args(plan, grad_out, seg, weights, default_row, scale))
  any_typed = any(a[0][0] is not None for a in args)

  def fill(e, i):
    table, plan, combiner = _device_table(requests[i][0]), requests[i][1], requests[i][5]
    (typed, grad_out), seg, w, d = args[i]
    e.combiner, e.table = int(combiner), table._h.value
    e.opt, e.plan = ctypes.addressof(p_list[i]), plan._h.value
    if any_typed:
      e.grad_out = typed if typed is not None else _capi.Grads(grad_out.data_ptr(), _capi.TFRA_F32, 0, None)
    else:
      e.grad_out = grad_out.data_ptr()
    e.seg, e.weights = seg.data_ptr(), (w.data_ptr() if w is not None else None)
    e.n_rows, e.param_default_row = grad_out.shape[0], d.data_ptr()
    return grad_out, seg, w, d, p_list[i]

  c_name, desc_type = (("tfra_multi_apply_planned_combined_typed", _capi.ApplyCombinedTypedDesc) if any_typed else
                       ("tfra_multi_apply_planned_combined", _capi.ApplyCombinedDesc))
  return _over_plans([req[1] for req in requests], _device_table(requests[0][0])._device, sync, _grouped_call,
                     c_name, desc_type, "apply_planned_combined_many", [r[0] for r in requests], fill)


def build_plans_many(plans, ids_list, return_launches=False):
  """The builds of a list of `SparsePlan`s in ONE C call (tfra_multi_sparse_plan_build; the frame: `_grouped_call`), on the CURRENT
  stream of the plans' device: plan i ends as `plans[i].build(ids_list[i])` leaves it — the same CSR per key, bit-identical
  write-backs through it.
  Around the call each plan gets what `SparsePlan.build` does for it: the ids as a contiguous int64 tensor kept alive on the plan,
  the wait for the plan's last use, `record_stream`, and the `_built` event behind the call.  All plans live on one device, have a
  dim > 0 (the assign-only plan is one kernel already) and occur once.  The call's workspace is `device_ops._workspace(device)`,
  which is keyed by the calling thread and the current stream: a build on a side stream has a workspace of its own and never shares the staging ring or
  the scratch of the main stream's grouped calls (`find_combine_many`, `apply_planned_combined_many`), which may be in flight at
  the same time.  Returns the plans (with return_launches: also the number of kernel launches the call enqueued — it does not grow
  with the list)."""
  plans = list(plans)
  n = len(plans)
  if len(ids_list) != n:
    raise ValueError("build_plans_many: %d plans but %d id tensors" % (n, len(ids_list)))
  if n == 0:
    return (plans, 0) if return_launches else plans
  device = plans[0]._device
  for plan in plans:
    if plan._device != device:
      raise ValueError("build_plans_many: all plans must live on one device (%s and %s)" % (device, plan._device))
  stream = torch.cuda.current_stream(device)
  flat = []

  def fill(e, i):
    plan, ids = plans[i], ids_list[i].to(device, torch.int64).contiguous().reshape(-1)
    if plan._used is not None:
      stream.wait_event(plan._used)     # the previous batch's sums/apply still read the plan buffers
    ids.record_stream(stream)
    flat.append(ids)
    e.plan, e.n, e.ids, e.dim = plan._h.value, ids.numel(), (ids.data_ptr() if ids.numel() else None), plan._dim

  launches = _grouped_call("tfra_multi_sparse_plan_build", _capi.PlanBuildDesc, "build_plans_many", plans, fill)
  for plan, ids in zip(plans, flat):
    plan.ids, plan.n = ids, ids.numel()   # keeps the ids alive until the next build
    plan._built.record(stream)
  return (plans, launches) if return_launches else plans


def tier_find_or_insert_many(requests, return_launches=False):
  """The admitting lookups of a list of tiers in ONE C call (tfra_multi_tier_find_or_insert; the frame: `_grouped_call`): one
  chain of launches for the whole list — 6, or 7 with verify, for aligned float32 tiers whose caches are full — where a loop of
  `_DeviceTier.find_or_insert` enqueues as many per tier.  `requests`: a list of (owner, keys[, init_values[, count[, want_rows[,
  verify[, out]]]]]), `owner` a _DeviceTier or a TieredHashTable, the arguments behind it those of `_DeviceTier.find_or_insert`, prepared
  the same way (`_DeviceTier._admit_args`); want_rows (default True) False: admission only, as `_DeviceTier.admit`.  Every tier,
  and every table in any role, may stand ONCE in the list (the call writes): the C call refuses the list otherwise, and a refused
  list changes nothing.  Returns, in the requests' order, (rows, where) or None for a request without want_rows, each what
  `find_or_insert(..., return_where=True)` of its request returns (with return_launches: also the number of kernel launches)."""
  if not requests:
    return ([], 0) if return_launches else []
  outs = []
  tiers = []
  for r in requests:
    tier = _device_tier(r[0])
    if tier is None:
      raise ValueError("tier_find_or_insert_many: every owner must be a TieredHashTable or a _DeviceTier")
    tiers.append(tier)

  def fill(e, i):
    req = tuple(requests[i]) + (None, None, True, False)[len(requests[i]) - 2:]
    _, keys, init_values, count, want_rows, verify = req[:6]
    keys, d, full, out, where = tiers[i]._admit_args(keys, init_values, want_rows, req[6] if len(req) > 6 else None)
    outs.append((out, where) if want_rows else None)
    e.flags, e.tier = (_capi.TIER_VERIFY if verify else 0), tiers[i]._h.value
    e.n, e.d_n, e.keys = keys.numel(), (count.data_ptr() if count is not None else None), keys.data_ptr()
    e.init_values, e.init_is_full, e.reserved = d.data_ptr(), full, 0
    e.values_out, e.where = (out.data_ptr(), where.data_ptr()) if want_rows else (None, None)
    return keys, d, count, out, where

  launches = _grouped_call("tfra_multi_tier_find_or_insert", _capi.TierFindOrInsertDesc, "tier_find_or_insert_many", tiers, fill)
  return (outs, launches) if return_launches else outs


def admit_many(requests):
  """`tier_find_or_insert_many` without outputs — the `_DeviceTier.admit` of a list of tiers in one call.  `requests`: a list of
  (owner, keys[, init_values[, count[, verify]]]), the arguments behind `owner` those of `_DeviceTier.admit`."""
  def widen(r):
    r = tuple(r) + (None, None, False)[len(r) - 2:]
    return (r[0], r[1], r[2], r[3], False, r[4])
  tier_find_or_insert_many([widen(r) for r in requests])


def find_or_insert_many(requests, return_launches=False):
  """The admitting lookups of a list of PLAIN tables in ONE C call (tfra_multi_find_or_insert; the frame: `_grouped_call`): phase 1
  once per copy-granule class of the list and, for the members at max_capacity, phase 2 once per class among them — 1 launch for
  aligned float32 growing tables, 2 with full bounded members — where a loop of `_DeviceTable.find_or_insert` enqueues as many per
  table.  `requests`: a list of (owner, keys[, init_values[, count[, want_rows[, scores[, out]]]]]), `owner` a _DeviceTable or a
  table class that wraps one (CuckooHashTable / HkvHashTable), the arguments behind it those of `_DeviceTable.find_or_insert`,
  prepared the same way; want_rows (default True) False: admission only, as `_DeviceTable.admit`.  Every table may stand ONCE in
  the list (the call writes): the C call refuses the list otherwise, and a refused list changes nothing.  Returns, in the
  requests' order, (rows, exists) or None for a request without want_rows, each what `find_or_insert(..., return_exists=True)` of
  its request returns (with return_launches: also the number of kernel launches)."""
  if not requests:
    return ([], 0) if return_launches else []
  outs = []
  tables = []
  for r in requests:
    if _device_tier(r[0]) is not None:
      raise ValueError("find_or_insert_many: a tiered owner goes through tier_find_or_insert_many")
    tables.append(_device_table(r[0]))

  def fill(e, i):
    t = tables[i]
    req = tuple(requests[i]) + (None, None, True, None, None)[len(requests[i]) - 2:]
    _, keys, init_values, count, want_rows, scores, out = req[:7]
    keys = t._keys(keys)
    n = keys.numel()
    d, full = t._init_rows(init_values, n)
    scores = _scores_for(scores, n, t._device)
    exists = None
    if want_rows:
      out = t._out(keys.shape, out)
      exists = torch.zeros(keys.shape, dtype=torch.bool, device=t._device)
    else:
      out = None
    outs.append((out, exists) if want_rows else None)
    e.flags, e.table = 0, t._h.value
    e.n, e.d_n, e.keys = n, (count.data_ptr() if count is not None else None), keys.data_ptr()
    e.init_values, e.init_is_full, e.reserved = d.data_ptr(), full, 0
    e.scores = scores.data_ptr() if scores is not None else None
    e.values_out, e.found = (out.data_ptr(), exists.data_ptr()) if want_rows else (None, None)
    return keys, d, count, scores, out, exists

  launches = _grouped_call("tfra_multi_find_or_insert", _capi.FindOrInsertDesc, "find_or_insert_many", tables, fill)
  return (outs, launches) if return_launches else outs


def table_admit_many(requests):
  """`find_or_insert_many` without outputs — the `_DeviceTable.admit` of a list of plain tables in one call.  `requests`: a list of
  (owner, keys[, init_values[, count[, scores]]]), the arguments behind `owner` those of `_DeviceTable.admit`."""
  def widen(r):
    r = tuple(r) + (None, None, None)[len(r) - 2:]
    return (r[0], r[1], r[2], r[3], False, r[4])
  find_or_insert_many([widen(r) for r in requests])
