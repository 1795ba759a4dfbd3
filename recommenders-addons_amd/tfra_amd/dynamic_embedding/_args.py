"""Marshalling between torch tensors and the C ABI, and the operand checks of the table calls: the leaf of the Python layer.

Depends on torch and `_capi` only, so `device_ops`, `table_ops` and everything above them import it without a cycle.  The checks
are plain functions over (value_dtype, dim, device, ...): `_DeviceTable`, `_DeviceTier` and the grouped calls apply the same
rule by calling the same function, and each raises before any C call, so a machine without a GPU can test them.
"""
import ctypes

import torch

from .. import _capi

_TORCH2DT = {
    torch.float32: _capi.TFRA_F32,
    torch.float16: _capi.TFRA_F16,
    torch.bfloat16: _capi.TFRA_BF16,
    torch.int8: _capi.TFRA_I8,
    torch.int32: _capi.TFRA_I32,
    torch.int64: _capi.TFRA_I64,
    torch.float64: _capi.TFRA_F64,
}

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
  """The current HIP stream of `device` as a void*.  torch.cuda.current_stream() builds a Stream object through several
  Python layers (5 us per call, 18 calls in one routed multi-GPU step): the raw getter is the same value in 0.3 us."""
  if _raw_stream is not None:
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    return ctypes.c_void_p(_raw_stream(idx if idx is not None else torch.cuda.current_device()))
  return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _grads_arg(grads, device, dim, grad_scale=None, max_elements=None):
  """A gradient matrix as a write-back takes it: (tfra_grads, tensor) when it goes down as it is — a contiguous float16 / bfloat16
  matrix on `device`, inside the typed calls' limits (dim % 4 == 0, 8-byte aligned), with `grad_scale` (a one-element float32
  device tensor, e.g. a GradScaler's inverse scale) read by the kernels — else (None, tensor) with the float32 up-cast, times
  grad_scale where there is one: by the typed calls' definition the same bits.  The tensor is what the call reads: keep it
  alive across the call.  No host read either way.  max_elements: a matrix of that many elements or more does not go down as it is (the
  combined typed calls address grad_out with 32-bit element offsets)."""
  if grad_scale is not None:
    grad_scale = torch.as_tensor(grad_scale)
    if grad_scale.numel() != 1:
      raise ValueError("grad_scale must hold one element, got shape %s" % list(grad_scale.shape))
  scale_down = grad_scale is None or (grad_scale.dtype == torch.float32 and grad_scale.device == device)
  if (grads.dtype in (torch.float16, torch.bfloat16) and grads.device == device and grads.is_contiguous() and grads.numel() and
      dim % 4 == 0 and grads.data_ptr() % 8 == 0 and scale_down and (max_elements is None or grads.numel() < max_elements)):
    return _capi.Grads(grads.data_ptr(), _TORCH2DT[grads.dtype], 0, None if grad_scale is None else grad_scale.data_ptr()), grads
  g = grads.to(device, torch.float32)
  if grad_scale is not None:
    g = g * grad_scale.to(device=device, dtype=torch.float32).reshape(())
  return None, g.contiguous()


_OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _out_dtype(out_dtype):
  """The `out_dtype=` of a lookup: None (the call's own output type: today's path) or one of float32 / float16 / bfloat16, the
  types the typed lookups write (tfra_rows_out); anything else raises TypeError before a launch."""
  if out_dtype is not None and out_dtype not in _OUT_DTYPES:
    raise TypeError("out_dtype must be torch.float32, torch.float16 or torch.bfloat16, got %s" % (out_dtype,))
  return out_dtype


def _rows_out(out):
  """A lookup's output tensor as the typed calls take it (tfra_rows_out).  Keep the tensor alive across the call."""
  return _capi.RowsOut(out.data_ptr(), _TORCH2DT[out.dtype], 0)


def _wide_keys(keys):
  """`keys` as the engine's int64 keys, for a C function that reads `const int64_t*`: int64 keys as they are, int32 keys widened on
  the device (tfra_keys_widen_i32).  Any other dtype raises TypeError before a launch."""
  if keys.dtype == torch.int64:
    return keys.contiguous()
  if keys.dtype != torch.int32:
    raise TypeError("keys must be torch.int64 or torch.int32, got %s" % keys.dtype)
  keys = keys.contiguous()
  wide = torch.empty(keys.shape, dtype=torch.int64, device=keys.device)
  if keys.numel():
    _capi.call("tfra_keys_widen_i32", keys.numel(), _ptr(keys), _ptr(wide), _stream(keys.device))
  return wide


def _narrow_keys(keys, dtype):
  """Engine int64 keys back in the caller's key dtype: int32 keys narrowed on the device (tfra_keys_narrow_i32), int64 as they
  are.  Only keys that came from int32 keys are narrowed, so none can overflow."""
  if dtype == torch.int64:
    return keys
  narrow = torch.empty(keys.shape, dtype=torch.int32, device=keys.device)
  if keys.numel():
    _capi.call("tfra_keys_narrow_i32", keys.numel(), _ptr(keys.contiguous()), _ptr(narrow), None, _stream(keys.device))
  return narrow


def _as_tensor(x, device):
  """`x` as it is when it is a tensor (wherever it lives), else as a tensor on `device`."""
  return x if torch.is_tensor(x) else torch.as_tensor(x, device=device)


def _driver_ids(table, ids, device, widen=True):
  """The ids of a step or route driver, as the int64 buffer its C calls read.  An int32-key table takes int32 ids only — int64 ids
  raise TypeError before any launch, as the table's own ops do, so that no key above 2^31 can enter it — and widens them (or,
  widen=False, keeps them as they are); an int64-key table casts whatever integer ids it is given, as it always has."""
  if table.key_dtype == torch.int32:
    ids = _as_tensor(ids, device)
    if ids.dtype != torch.int32:
      raise TypeError("Signature mismatch. Keys must be dtype %s, got %s." % (torch.int32, ids.dtype))
    ids = ids.to(device).reshape(-1).contiguous()
    return _wide_keys(ids) if widen else ids
  if torch.is_tensor(ids) and ids.dtype == torch.int64 and ids.dim() == 1 and ids.is_contiguous() and ids.device == device:
    return ids
  return torch.as_tensor(ids, device=device).reshape(-1).to(torch.int64).contiguous()


def _score_filter(threshold, pred):
  """(tfra_score_pred, threshold) of a score-filtered call: `pred` is the string "ge" (score >= threshold) or "lt" (score <
  threshold), the threshold an integer in [0, 2^64).  Anything else raises ValueError before a launch."""
  if pred not in ("ge", "lt"):
    raise ValueError("pred must be 'ge' or 'lt', got %r" % (pred,))
  try:
    thr = int(threshold)
  except (TypeError, ValueError):
    raise ValueError("threshold must be an integer in [0, 2^64), got %r" % (threshold,))
  if not 0 <= thr < (1 << 64):
    raise ValueError("threshold must be in [0, 2^64), got %r" % (threshold,))
  return (_capi.SCORE_GE if pred == "ge" else _capi.SCORE_LT), thr


def _as_device(device):
  if device is None or device == "" or device == []:
    device = "cuda:0"
  if isinstance(device, (list, tuple)):
    device = device[0]
  if isinstance(device, str):
    d = device.strip().lower().replace("/", "")
    # TF-style '/GPU:0' / '/device:GPU:0'
    if "gpu" in d:
      device = "cuda:" + d.split(":")[-1]
  dev = torch.device(device)
  if dev.type != "cuda":
    raise RuntimeError(
        "tfra_amd tables live on an MI355X (device %r requested); there is no CPU fallback" %
        (device,))
  if not torch.cuda.is_available():
    raise RuntimeError("no HIP device visible: tfra_amd has no CPU fallback")
  return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


# ---- the operand checks of the table calls ------------------------------------------------------------------------------------
def _rows_on(value_dtype, device, rows, what):
  """`rows` on `device`, contiguous; TypeError unless it has the table's value dtype."""
  d = rows.to(device) if torch.is_tensor(rows) else torch.as_tensor(rows, device=device)
  if d.dtype != value_dtype:
    raise TypeError("%s must be dtype %s, got %s" % (what, value_dtype, d.dtype))
  return d.contiguous()


def _default_rows(value_dtype, dim, device, rows, n_out):
  """The default rows of the `find` family -> (rows, is_full).  The reference's rule: the operand is full — one row per key —
  when it has as many elements as the output (`n_out`), is_full_default = (value_flat.size() == default_flat.size())
  (R/kernels/hkv_hashtable_op_gpu.cu.cc:188-190, cuckoo_hashtable_op.cc:48-50); otherwise its first `dim` elements are the one
  row of every miss, so it needs at least `dim` of them."""
  d = _rows_on(value_dtype, device, rows, "default values")
  full = int(n_out == d.numel())
  if not full and d.numel() < dim:
    raise ValueError("default value needs at least dim=%d elements, got %d" % (dim, d.numel()))
  return d, full


def _admitted_rows(value_dtype, dim, device, rows, n, what="init values"):
  """The rows of the admitting family (find_or_insert and the tier's calls) -> (rows, is_full).  These rows ENTER the table, so
  the rule is strict: [n, dim], or exactly one row of dim elements (one key: the two forms are the same row)."""
  d = _rows_on(value_dtype, device, rows, what)
  full = int(d.numel() == n * dim)
  if not full and d.numel() != dim:
    raise ValueError("%s must be [n, dim] or one row of dim=%d elements, got shape %s" % (what, dim, list(d.shape)))
  return d, full


def _scores_for(scores, n, device, per="key"):
  """The `scores` operand of a write: None, or an empty tensor (HkvHashTableInsert: empty scores tensor == no scores) -> None;
  else int64 on `device`, contiguous, one entry for each of the n keys (of a plan: its n batch positions).  The kernels read n
  entries through a raw pointer, so any other length raises ValueError."""
  if scores is None or scores.numel() == 0:
    return None
  scores = scores.to(device, torch.int64).contiguous()
  if scores.numel() != n:
    raise ValueError("scores must have one entry per %s" % per)
  return scores


def _out_rows(value_dtype, dim, device, shape, out):
  """The `out=` buffer of a lookup whose keys have `shape`: a new [*shape, dim] tensor when None, else `out` once it is known to
  be what the kernel writes n x dim elements into."""
  if out is None:
    return torch.empty(tuple(shape) + (dim,), dtype=value_dtype, device=device)
  n = 1
  for s in shape:
    n *= s
  if out.dtype != value_dtype or out.numel() != n * dim or not out.is_contiguous() or out.device != device:
    raise ValueError("out must be a contiguous %s tensor of %d x %d elements on %s" % (value_dtype, n, dim, device))
  return out


def _cap_for(cap, n):
  """The room of a call's result lists: one entry per key (which always suffices) when None."""
  cap = n if cap is None else int(cap)
  if cap < 0:
    raise ValueError("cap must be >= 0, got %d" % cap)
  return cap


def _trim_to_count(counter, cap, keys, key_dtype, *lists):
  """The `sync` tail of a call that fills lists of up to `cap` entries and counts on beyond it: ONE host read of the counter,
  every list trimmed to min(count, cap), the engine's int64 keys back in the table's key dtype (only the written part: narrowing
  the unwritten tail would read it)."""
  m = min(int(counter.item()), cap)
  return (_narrow_keys(keys[:m], key_dtype),) + tuple(x[:m] for x in lists)


def _check_plan(plan, dim, device):
  """A write-back plan serves a table of the row width it was built for, on its device."""
  if plan._dim != dim or plan._device != device:
    raise ValueError("the plan was built for dim %d on %s" % (plan._dim, plan._device))


def _over_plans(plans, device, sync, fn, *args):
  """fn(*args) — a call that reads the buffers of every plan of `plans` on the current stream of `device` — in the plans' stream
  frame: the stream waits for each build before the call, and each plan's next build waits for the call (`SparsePlan._wait_built`
  / `_mark_used`).  sync=False leaves that ordering to the caller (a captured HIP graph orders them by its edges)."""
  if not sync:
    return fn(*args)
  stream = torch.cuda.current_stream(device)
  for plan in plans:
    plan._wait_built(stream)
  result = fn(*args)
  for plan in plans:
    plan._mark_used(stream)
  return result
