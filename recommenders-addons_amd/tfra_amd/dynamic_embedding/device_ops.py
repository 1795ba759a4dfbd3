"""Device front-end ops that bracket the table calls (N1/N3 of SURVEY.md §8f), as torch-tensor
functions over the C ABI: unique, gather, segment_sum, partition (+stitch)."""
import ctypes
import sys
import threading

import torch

from .. import _capi
from ._args import _grads_arg, _narrow_keys, _ptr, _stream, _wide_keys

class _Workspaces(dict):
  """One thread's workspaces, {(device index, stream): handle}; destroyed when the thread's storage goes (tfra_workspace_destroy
  synchronises the device first, so kernels the thread left queued have finished with the scratch)."""

  def __del__(self):
    if sys.is_finalizing():   # at interpreter exit the workspaces go with the process, as they always did
      return
    for h in self.values():
      try:
        _capi.lib().tfra_workspace_destroy(h)
      except Exception:
        pass


_WS = threading.local()   # .handles: the calling thread's _Workspaces


def _workspace(device):
  """One scratch workspace per (HOST THREAD, device, CURRENT STREAM).  A tfra_workspace serves one call at a time and one stream
  (include/tfra_mi355x.h, tfra_workspace_create): it has no lock of its own, a call that needs more scratch frees the buffer
  after synchronising its OWN stream only, and the persistent sets of tfra_unique / tfra_multi_unique alternate by a parity that
  a call flips on the host.  ctypes releases the GIL for the length of a C call, so two Python threads on one stream (the
  default stream, say) would otherwise be inside the library with the same handle: hence the thread in the key.  Per stream,
  because a workspace's scratch and staging ring are reused from call to call without any event: only the stream's own order
  keeps the next call's kernels behind the previous call's.  (tfra_unique and tfra_multi_unique alone do chain a change of stream
  with an event; nothing here relies on it.)"""
  ws = getattr(_WS, "handles", None)
  if ws is None:
    ws = _WS.handles = _Workspaces()
  key = (device.index, _stream(device).value)
  if key not in ws:
    h = ctypes.c_void_p()
    _capi.call("tfra_workspace_create", device.index, ctypes.byref(h))
    ws[key] = h
  return ws[key]


def unique(ids, ordered=True):
  """tf.unique (first-occurrence order): returns (unique[U], idx[n] int32, num_unique device scalar).  `unique` has the dtype of
  `ids` (int64 or int32, as tf.unique's output has its input's; tfra_unique reads int64 ids, so int32 ids are widened in front of
  it and the uniques narrowed back).

  `unique` is returned as a length-n buffer view trimmed with ONE host read of the count — the
  same sync TF's `tf.unique` output-shape inference imposes (PY/dynamic_embedding_ops.py:99).
  ordered=False: the distinct ids in no particular order (tfra_unique_unordered, two launches instead of three; up to 2^18 ids)
  — all embedding_lookup needs: the order of tf.unique's output is not observable behind the gather."""
  flat = _wide_keys(ids.reshape(-1))
  n = flat.numel()
  dev = flat.device
  uniq = torch.empty(n, dtype=torch.int64, device=dev)
  idx = torch.empty(n, dtype=torch.int32, device=dev)
  cnt = torch.zeros((), dtype=torch.int64, device=dev)
  fn = "tfra_unique" if (ordered or n > (1 << 18)) else "tfra_unique_unordered"
  _capi.call(fn, _workspace(dev), n, _ptr(flat), _ptr(uniq), _ptr(idx), _ptr(cnt), _stream(dev))
  u = int(cnt.item())
  return _narrow_keys(uniq[:u], ids.dtype), idx, cnt


def unique_no_sync(ids):
  """Like `unique` but never reads the count on the host: returns the full-length buffer (in the dtype of `ids`)."""
  flat = _wide_keys(ids.reshape(-1))
  n = flat.numel()
  dev = flat.device
  uniq = torch.empty(n, dtype=torch.int64, device=dev)
  idx = torch.empty(n, dtype=torch.int32, device=dev)
  cnt = torch.zeros((), dtype=torch.int64, device=dev)
  _capi.call("tfra_unique", _workspace(dev), n, _ptr(flat), _ptr(uniq), _ptr(idx), _ptr(cnt), _stream(dev))
  return _narrow_keys(uniq, ids.dtype), idx, cnt


UNIQUE_MANY_MAX_LIST = 1 << 20    # tfra_multi_unique's bounds (include/tfra_mi355x.h): ids in one list,
UNIQUE_MANY_MAX_TOTAL = 1 << 22   # ids in all lists of a call


def _round_up(n, to):
  return (n + to - 1) // to * to


def unique_many(ids_list, want_idx=True, return_launches=False):
  """`unique_no_sync` of a LIST of id tensors in ONE C call (tfra_multi_unique: one insert, one scatter and one index launch over
  all lists, whatever their number).  Returns the list of (uniq, idx, cnt), member i what `unique_no_sync(ids_list[i])` returns:
  the full-length buffer of distinct ids in first-occurrence order in the dtype of the member's ids (int32 ids widened in front
  of the call and narrowed behind it, per member), the int32 inverse index, the count as a device scalar; nothing is read on the
  host.  The lists are independent.  want_idx=False: every `idx` is None and the index launch is left out (two launches: all
  admission needs).  All lists must live on one device (ValueError); the workspace is the one of
  that device's current stream.  The members' buffers are views of one allocation per kind.  A list beyond the call's limits
  (UNIQUE_MANY_MAX_LIST ids in one member, UNIQUE_MANY_MAX_TOTAL in all) takes the loop of `unique_no_sync`.
  return_launches: also the number of kernel launches of the de-duplication itself."""
  n_l = len(ids_list)
  if n_l == 0:
    return ([], 0) if return_launches else []
  dev = ids_list[0].device
  for ids in ids_list:
    if ids.device != dev:
      raise ValueError("unique_many: all lists must live on one device (%s and %s)" % (dev, ids.device))
  sizes = [ids.numel() for ids in ids_list]
  if max(sizes) > UNIQUE_MANY_MAX_LIST or sum(sizes) > UNIQUE_MANY_MAX_TOTAL:
    res = [unique_no_sync(ids) for ids in ids_list]
    res = [(u, i if want_idx else None, c) for u, i, c in res]
    return (res, sum(0 if n == 0 else 3 if n <= (1 << 20) else 6 for n in sizes)) if return_launches else res
  flats = [_wide_keys(ids.reshape(-1)) for ids in ids_list]
  # one allocation per kind; every member's view starts on a 512-byte boundary, as a tensor of its own would
  u_at, i_at, u_end, i_end = [], [], 0, 0
  for n in sizes:
    u_at.append(u_end)
    u_end += _round_up(n, 64)
    i_at.append(i_end)
    i_end += _round_up(n, 128) if want_idx else 0
  uniq_all = torch.empty(u_end, dtype=torch.int64, device=dev)
  idx_all = torch.empty(i_end, dtype=torch.int32, device=dev)
  cnt_all = torch.empty(n_l, dtype=torch.int64, device=dev)   # (the call writes every count, 0 for an empty list)
  descs = (_capi.UniqueDesc * n_l)()
  res = []
  for k, (flat, n) in enumerate(zip(flats, sizes)):
    uniq = uniq_all[u_at[k]:u_at[k] + n]
    idx = idx_all[i_at[k]:i_at[k] + n] if want_idx else None
    cnt = cnt_all[k]
    e = descs[k]
    e.struct_size, e.flags, e.n = ctypes.sizeof(_capi.UniqueDesc), 0, n
    e.ids, e.unique_out = (flat.data_ptr(), uniq.data_ptr()) if n else (None, None)
    e.idx_out = idx.data_ptr() if (want_idx and n) else None
    e.d_num_unique = cnt.data_ptr()
    res.append((uniq, idx, cnt))
  launches = ctypes.c_uint32(0)
  _capi.call("tfra_multi_unique", _workspace(dev), n_l, ctypes.c_void_p(ctypes.addressof(descs)),
             ctypes.c_void_p(ctypes.addressof(launches)), _stream(dev))
  res = [(_narrow_keys(u, ids.dtype), i, c) for (u, i, c), ids in zip(res, ids_list)]
  return (res, int(launches.value)) if return_launches else res


SAFE_ENTRIES_MAX_LIST = 1 << 31    # tfra_multi_safe_entries' bounds (include/tfra_mi355x.h): nnz + n_rows of one list stays below,
SAFE_ENTRIES_MAX_TOTAL = 1 << 24   # entries plus rows of all lists of a call


def safe_entries_fit(sizes):
  """Whether lists of these (nnz, n_rows) fit one tfra_multi_safe_entries call."""
  return (all(nnz + n < SAFE_ENTRIES_MAX_LIST for nnz, n in sizes) and sum(nnz + n for nnz, n in sizes) <= SAFE_ENTRIES_MAX_TOTAL)


def _read_counts(counts):
  """The ONE host read of `safe_entries_many`: every list's two counts."""
  return counts.cpu().tolist()


def safe_entries_many(requests, want_kept=True, want_entries=True, return_launches=False):
  """The kept list and the entry list of a LIST of safe sparse lookups in ONE C call (tfra_multi_safe_entries: at most five
  launches, whatever the number of lists) and ONE host read: the `.cpu()` of the call's [n_lists, 2] counts.  A request is
  (rows, ids, weights, n_rows, prune, fill_id, ragged): `rows` int64 ascending row ids [nnz] or — ragged — row_splits
  [n_rows + 1]; `ids` int64 or int32 [nnz]; `weights` float32 [nnz] or None; `prune`: only entries with weight > 0 are members;
  `fill_id`: the id of a member-less row's entry (weight 1), None: id 0 with weight 0.  All on one device (ValueError).
  Returns per request (kept, entries), each (ids, rows, weights) trimmed to its count or None where it was not asked for:
  kept = the members in input order (weights None where none were given), entries = the members and one entry per member-less row
  in row order (weights None where none were given and fill_id is not None: they would all be 1).  ids come back in the dtype
  they were given in (int32 ids widened in front of the call and narrowed behind it).  want_kept / want_entries: a bool, or one
  per request.  Lists beyond the call's limits raise ValueError (`safe_entries_fit`).
  return_launches: also the number of kernel launches of the builder itself."""
  n_l = len(requests)
  if n_l == 0:
    return ([], 0) if return_launches else []
  kept_of = list(want_kept) if isinstance(want_kept, (list, tuple)) else [bool(want_kept)] * n_l
  ent_of = list(want_entries) if isinstance(want_entries, (list, tuple)) else [bool(want_entries)] * n_l
  dev = requests[0][1].device
  sizes = []
  for rows, ids, w, n, prune, fill, ragged in requests:
    for t in (rows, ids, w):
      if t is not None and t.device != dev:
        raise ValueError("safe_entries_many: all lists must live on one device (%s and %s)" % (dev, t.device))
    nnz, n = ids.numel(), int(n)
    if rows.numel() != (n + 1 if ragged else nnz) or (w is not None and w.numel() != nnz):
      raise ValueError("safe_entries_many: rows %d, ids %d, weights %s for %d rows" %
                       (rows.numel(), nnz, None if w is None else w.numel(), n))
    sizes.append((nnz, n))
  if not safe_entries_fit(sizes):
    raise ValueError("safe_entries_many: the lists are beyond one call's limits")
  # one allocation per kind; every member's view starts on a 512-byte boundary, as a tensor of its own would
  i_end = f_end = 0
  at = []
  for k, (nnz, n) in enumerate(sizes):
    has_w = requests[k][2] is not None
    ent_w = ent_of[k] and (has_w or requests[k][5] is None)
    spans = [nnz if kept_of[k] else 0] * 2 + [nnz + n if ent_of[k] else 0] * 2
    offs = []
    for span in spans:
      offs.append(i_end)
      i_end += _round_up(span, 64)
    for span in (nnz if (kept_of[k] and has_w) else 0, nnz + n if ent_w else 0):
      offs.append(f_end)
      f_end += _round_up(span, 128)
    at.append((offs, has_w, ent_w))
  i_all = torch.empty(i_end, dtype=torch.int64, device=dev)
  f_all = torch.empty(f_end, dtype=torch.float32, device=dev)
  counts = torch.empty((n_l, 2), dtype=torch.int64, device=dev)   # (the call writes every count)
  descs = (_capi.SafeEntriesDesc * n_l)()
  hold, views = [], []
  for k, ((rows, ids, w, _, prune, fill, ragged), (nnz, n)) in enumerate(zip(requests, sizes)):
    offs, has_w, ent_w = at[k]
    rows = rows.reshape(-1).to(torch.int64).contiguous()
    flat = _wide_keys(ids.reshape(-1))
    w = None if w is None else w.reshape(-1).contiguous()
    hold.append((rows, flat, w))
    e = descs[k]
    e.struct_size, e.n_rows, e.nnz = ctypes.sizeof(_capi.SafeEntriesDesc), n, nnz
    e.flags = ((_capi.SAFE_PRUNE if prune else 0) | (_capi.SAFE_FILL if fill is not None else 0) |
               (_capi.SAFE_RAGGED if ragged else 0))
    e.rows, e.ids, e.weights = rows.data_ptr() if rows.numel() else None, flat.data_ptr() if nnz else None, _ptr(w) if nnz else None
    e.fill_id = 0 if fill is None else int(fill)
    v = [None] * 6
    if kept_of[k]:
      v[0], v[1] = i_all[offs[0]:offs[0] + nnz], i_all[offs[1]:offs[1] + nnz]
      v[4] = f_all[offs[4]:offs[4] + nnz] if has_w else None
      # (an empty view has no address of its own: any aligned one serves a buffer of no elements)
      e.kept_ids, e.kept_rows = i_all.data_ptr() + 8 * offs[0], i_all.data_ptr() + 8 * offs[1]
      e.kept_weights = f_all.data_ptr() + 4 * offs[4] if (has_w and nnz) else None
    if ent_of[k]:
      v[2], v[3] = i_all[offs[2]:offs[2] + nnz + n], i_all[offs[3]:offs[3] + nnz + n]
      v[5] = f_all[offs[5]:offs[5] + nnz + n] if ent_w else None
      e.entry_ids, e.entry_rows = i_all.data_ptr() + 8 * offs[2], i_all.data_ptr() + 8 * offs[3]
      e.entry_weights = f_all.data_ptr() + 4 * offs[5] if ent_w else None
    e.d_counts = counts.data_ptr() + 16 * k
    views.append(v)
  launches = ctypes.c_uint32(0)
  _capi.call("tfra_multi_safe_entries", _workspace(dev), n_l, ctypes.c_void_p(ctypes.addressof(descs)),
             ctypes.c_void_p(ctypes.addressof(launches)), _stream(dev))
  host = _read_counts(counts)
  res = []
  for k, v in enumerate(views):
    nk, ne = host[k]
    dt = requests[k][1].dtype
    kept = (_narrow_keys(v[0][:nk], dt), v[1][:nk], None if v[4] is None else v[4][:nk]) if kept_of[k] else None
    ent = (_narrow_keys(v[2][:ne], dt), v[3][:ne], None if v[5] is None else v[5][:ne]) if ent_of[k] else None
    res.append((kept, ent))
  return (res, int(launches.value)) if return_launches else res


FIELD_ENTRIES_MAX_SLOTS = 2048   # tfra_field_entries' bounds (include/tfra_mi355x.h): nslots up to here,
FIELD_ENTRIES_MAX_N = 1 << 31    # n_rows * per_row stays below


def field_entries_fit(n_rows, per_row, nslots):
  """Whether a [n_rows, per_row] block over `nslots` fields fits one tfra_field_entries call."""
  return nslots <= FIELD_ENTRIES_MAX_SLOTS and max(n_rows, per_row, n_rows * per_row) < FIELD_ENTRIES_MAX_N


def _field_block(ids2d, slots2d, nslots, who):
  """(ids [B, S], slots int64 [B, S], nslots) of a field-wise block, shapes checked."""
  if ids2d.dim() != 2:
    raise ValueError("%s: ids must be [batch, per_sample], got shape %s" % (who, list(ids2d.shape)))
  if slots2d.numel() != ids2d.numel() or slots2d.device != ids2d.device:
    raise ValueError("%s: slots must have one element per id, on the ids' device" % who)
  nslots = int(nslots)
  if nslots < 1:
    raise ValueError("%s: nslots must be >= 1, got %d" % (who, nslots))
  return ids2d, slots2d.reshape(ids2d.shape).to(torch.int64), nslots


def _field_entries_torch(ids2d, slots2d, nslots, want_pos=False, want_seg=True, bad=None):
  """`field_entries` in torch ops, on whatever device the block lives (the reference's `_pooling_by_slots`, PY/keras/layers/
  embedding.py:491-513, with the order of ties pinned): the slots clamped into [0, nslots), the bias sample * nslots added, a STABLE
  `torch.sort`, the ids gathered, the splits by `searchsorted`.  The route of blocks beyond the builder's limits and the tests'
  reference."""
  ids, slots, nslots = _field_block(ids2d, slots2d, nslots, "_field_entries_torch")
  b, s = ids.shape
  dev = ids.device
  if bad is not None:
    bad += ((slots < 0) | (slots >= nslots)).sum()
  seg = slots.clamp(0, nslots - 1) + torch.arange(b, dtype=torch.int64, device=dev).reshape(b, 1) * nslots
  seg, order = torch.sort(seg.reshape(-1), stable=True)
  entry_ids = ids.reshape(-1)[order]
  row_splits = torch.searchsorted(seg, torch.arange(b * nslots + 1, dtype=torch.int64, device=dev))
  return entry_ids, row_splits, (order.to(torch.int32) if want_pos else None), (seg if want_seg else None)


def field_entries(ids2d, slots2d, nslots, want_pos=False, want_seg=True, bad=None):
  """The pooling lists of a field-wise embedding in ONE launch (tfra_field_entries; no workspace, nothing read on the host).
  `ids2d` int64 or int32 [batch, per_sample] on a device, `slots2d` any integer dtype, one field in [0, nslots) per id.  Returns
  (entry_ids, row_splits, entry_pos, entry_seg): the ids ordered by (sample, slot, input position) — stable — in the dtype they
  were given in (int32 ids widened in front of the call and narrowed behind it); row_splits int64 [batch * nslots + 1], segment
  sample * nslots + slot owning [row_splits[s], row_splits[s + 1]); entry_pos int32 [n], every entry's input position (want_pos,
  else None); entry_seg int64 [n], every entry's segment (want_seg, else None).  `bad`: an int64 device tensor of one element
  that receives += the number of slots outside [0, nslots); such a slot is clamped into range either way.
  A block beyond the call's limits (`field_entries_fit`) takes `_field_entries_torch`, with the same results."""
  ids, slots, nslots = _field_block(ids2d, slots2d, nslots, "field_entries")
  dev = ids.device
  if dev.type != "cuda":
    raise ValueError("field_entries builds its lists on the device; the ids live on %s" % dev)
  if bad is not None and (bad.dtype != torch.int64 or bad.numel() != 1 or bad.device != dev):
    raise ValueError("field_entries: bad must be an int64 tensor of one element on the ids' device")
  b, s = ids.shape
  if not field_entries_fit(b, s, nslots):
    return _field_entries_torch(ids, slots, nslots, want_pos, want_seg, bad)
  n = b * s
  flat = _wide_keys(ids.reshape(-1))
  slots = slots.contiguous()
  entry_ids = torch.empty(n, dtype=torch.int64, device=dev)
  if b == 0:   # (the call writes nothing for no samples: the one split is the closing one)
    row_splits = torch.zeros(1, dtype=torch.int64, device=dev)
  else:
    row_splits = torch.empty(b * nslots + 1, dtype=torch.int64, device=dev)
  entry_pos = torch.empty(n, dtype=torch.int32, device=dev) if want_pos else None
  entry_seg = torch.empty(n, dtype=torch.int64, device=dev) if want_seg else None
  with torch.cuda.device(dev):   # (the launch goes to the calling thread's current device)
    _capi.call("tfra_field_entries", b, s, nslots, _ptr(flat) if n else None, _ptr(slots) if n else None,
               _ptr(entry_ids) if n else None, _ptr(row_splits), _ptr(entry_pos) if n else None, _ptr(entry_seg) if n else None,
               _ptr(bad), _stream(dev))
  return _narrow_keys(entry_ids, ids.dtype), row_splits, entry_pos, entry_seg


def gather_rows(rows, idx):
  """out[i,:] = rows[idx[i],:]  (tf.gather after unique, PY/dynamic_embedding_ops.py:111)."""
  rows = rows.contiguous()
  idx = idx.contiguous()
  n = idx.numel()
  row_bytes = rows.shape[-1] * rows.element_size()
  out = torch.empty((n, rows.shape[-1]), dtype=rows.dtype, device=rows.device)
  _capi.call("tfra_gather_rows", n, row_bytes, _ptr(rows), _ptr(idx), _ptr(out), _stream(rows.device))
  return out


def scatter_rows(rows, perm, n_out=None):
  """out[perm[i],:] = rows[i,:]  (dynamic_stitch with one flat permutation)."""
  rows = rows.contiguous()
  perm = perm.contiguous()
  n = perm.numel()
  two_d = rows.reshape(n, -1)
  row_bytes = two_d.shape[1] * rows.element_size()
  out = torch.empty((n if n_out is None else n_out, two_d.shape[1]), dtype=rows.dtype, device=rows.device)
  _capi.call("tfra_scatter_rows", n, row_bytes, _ptr(two_d), _ptr(perm), _ptr(out), _stream(rows.device))
  return out


def segment_sum(grads, idx, num_segments_dev, max_segments):
  """unsorted_segment_sum(grads, idx) -> [max_segments, dim]; rows >= *num_segments_dev are unspecified.
  Members of a segment are added in input order, one fp32 add each (sequential CPU order)."""
  grads = grads.contiguous()
  idx = idx.contiguous()
  n = idx.numel()
  dim = grads.shape[-1]
  out = torch.empty((max_segments, dim), dtype=torch.float32, device=grads.device)
  _capi.call("tfra_segment_sum", _workspace(grads.device), n, dim, _ptr(grads), _ptr(idx), _ptr(num_segments_dev),
             max_segments, _ptr(out), _stream(grads.device))
  return out


def reduce_by_key(ids, rows, grad_scale=None):
  """unique + unsorted_segment_sum, parallel per key (hot ids do not serialise) and bit-reproducible.
  Returns (keys[n] buffer in the dtype of `ids`, sums[n,dim] buffer, count device scalar): the first `count` entries are valid,
  in a deterministic but unspecified key order.  The sums are float32.  Contiguous float16 / bfloat16 rows on the ids' device go
  down as they are (tfra_reduce_by_key_typed: the same bits as their float32 up-cast gives), grad_scale — a one-element float32
  device tensor the rows are multiplied by — with them."""
  wide = _wide_keys(ids.reshape(-1))
  dev = wide.device
  n, dim = wide.numel(), rows.shape[-1]
  typed, rows = _grads_arg(rows, dev, dim if 0 < n <= (1 << 18) and dim <= 256 else 1, grad_scale)
  keys = torch.empty(n, dtype=torch.int64, device=dev)
  sums = torch.empty((n, dim), dtype=torch.float32, device=dev)
  cnt = torch.zeros((), dtype=torch.int64, device=dev)
  if typed is not None:
    _capi.call("tfra_reduce_by_key_typed", _workspace(dev), n, _ptr(wide), dim, ctypes.byref(typed), _ptr(keys), _ptr(sums), _ptr(cnt),
               _stream(dev))
  else:
    _capi.call("tfra_reduce_by_key", _workspace(dev), n, _ptr(wide), dim, _ptr(rows), _ptr(keys), _ptr(sums), _ptr(cnt),
               _stream(dev))
  return _narrow_keys(keys, ids.dtype), sums, cnt


PARTITION_MASK_MOD = 0  # int32(key & 0x7fffffff) % N   (int64 keys on a GPU build: default_partition_fn's first branch)
PARTITION_FLOOR_MOD = 1  # key % N, floor mod            (every other case: int32 keys, CPU builds)
PARTITION_HASH = 2  # fmix64(key) % N               (opt-in, Zipf-balanced)


def default_partition_mode(key_dtype):
  """The mode of default_partition_fn for keys of `key_dtype` on a GPU build (PY/dynamic_embedding_variable.py:182-196): mask-mod
  for int64 keys only; int32 keys take `math_ops.mod(keys, shard_num)`, floor mod.  The two differ for negative keys whenever
  the shard count is not a power of two."""
  return PARTITION_FLOOR_MOD if key_dtype == torch.int32 else PARTITION_MASK_MOD


def partition(keys, num_shards, mode=PARTITION_MASK_MOD, n_dev=None):
  """default_partition_fn + dynamic_partition in one pass (PY/dynamic_embedding_variable.py:131-197).
  Returns owner-major keys (in the dtype of `keys`), perm (original index of each output element) and device counts[num_shards].
  n_dev: optional device int64 scalar — only the first min(n, n_dev) keys are partitioned (the buffers
  keep length n; entries past sum(counts) are unspecified)."""
  flat = _wide_keys(keys.reshape(-1))
  n = flat.numel()
  dev = flat.device
  keys_out = torch.empty(n, dtype=torch.int64, device=dev)
  perm = torch.empty(n, dtype=torch.int32, device=dev)
  counts = torch.zeros(num_shards, dtype=torch.int64, device=dev)
  _capi.call("tfra_partition", _workspace(dev), n, None if n_dev is None else _ptr(n_dev), _ptr(flat), num_shards, mode,
             _ptr(keys_out), _ptr(perm), _ptr(counts), _stream(dev))
  return _narrow_keys(keys_out, keys.dtype), perm, counts


def partition_by_owner(owner, num_shards):
  """dynamic_partition of range(n) by a caller-computed owner tensor (custom partitioners)."""
  owner = owner.reshape(-1).to(torch.int32).contiguous()
  n = owner.numel()
  dev = owner.device
  perm = torch.empty(n, dtype=torch.int32, device=dev)
  counts = torch.zeros(num_shards, dtype=torch.int64, device=dev)
  _capi.call("tfra_partition_by_owner", _workspace(dev), n, _ptr(owner), num_shards, _ptr(perm), _ptr(counts),
             _stream(dev))
  return perm, counts


def dynamic_partition(data, partitions, num_partitions):
  """tf.dynamic_partition on the device (K/dynamic_partition_op_gpu.cu.cc): `partitions` indexes the leading
  dims of `data`; returns `num_partitions` tensors, rows in input order.  Like the reference's GPU kernel,
  partition ids outside [0, num_partitions) are discarded (the CPU kernel raises).  The output shapes are
  data dependent: one host read of the counts, as for the TF op."""
  partitions = torch.as_tensor(partitions, device=data.device)
  if tuple(data.shape[:partitions.dim()]) != tuple(partitions.shape):
    raise ValueError("data.shape must start with partitions.shape: %s vs %s" % (list(data.shape), list(partitions.shape)))
  tail = tuple(data.shape[partitions.dim():])
  n = partitions.numel()
  width = 1
  for t in tail:
    width *= t
  if n == 0 or width == 0:
    counts = [0] * num_partitions if n == 0 else torch.bincount(
        partitions.reshape(-1).clamp(0, num_partitions).to(torch.int64), minlength=num_partitions + 1)[:num_partitions].tolist()
    return [torch.empty((c,) + tail, dtype=data.dtype, device=data.device) for c in counts]
  perm, counts = partition_by_owner(partitions.reshape(-1), num_partitions)
  counts = counts.tolist()
  rows = gather_rows(data.reshape(n, width), perm[:sum(counts)])
  return [r.reshape((-1,) + tail) for r in torch.split(rows, counts)]


def dynamic_stitch(indices, data):
  """tf.dynamic_stitch on the device (K/dynamic_stitch_op_gpu.cu.cc): merged[indices[m][i, ...]] =
  data[m][i, ...], first dim = max(index) + 1 (one host read).  Indices are expected to be distinct (what
  dynamic_partition of range(n) produces); rows no index names stay zero."""
  indices = [torch.as_tensor(i) for i in indices]
  data = [torch.as_tensor(d) for d in data]
  dev = data[0].device
  tail = tuple(data[0].shape[indices[0].dim():])
  for i, d in zip(indices, data):
    if tuple(d.shape[:i.dim()]) != tuple(i.shape) or tuple(d.shape[i.dim():]) != tail:
      raise ValueError("data[m].shape must be indices[m].shape + a common suffix")
  width = 1
  for t in tail:
    width *= t
  flat_idx = torch.cat([i.reshape(-1).to(device=dev, dtype=torch.int32) for i in indices]) if indices else None
  n_in = 0 if flat_idx is None else flat_idx.numel()
  n_out = int(flat_idx.max().item()) + 1 if n_in else 0
  out = torch.zeros((n_out,) + tail, dtype=data[0].dtype, device=dev)
  if n_in == 0 or width == 0:
    return out
  rows = torch.cat([d.reshape(-1, width) for d in data]).contiguous()
  _capi.call("tfra_scatter_rows", n_in, width * rows.element_size(), _ptr(rows), _ptr(flat_idx.contiguous()), _ptr(out),
             _stream(dev))
  return out


def select_lowest(keys, status, k):
  """The k keys with the lowest status (int32/int64), ties in input order (restrict policies).  The keys come back in the
  dtype of `keys` (int64 or int32)."""
  key_dtype = keys.dtype
  keys = _wide_keys(keys.reshape(-1))
  status = status.reshape(-1).contiguous()
  if status.dtype not in (torch.int32, torch.int64):
    raise TypeError("status must be int32 or int64")
  n = keys.numel()
  if status.numel() != n or k > n:
    raise ValueError("select_lowest: need one status per key and k <= n")
  out = torch.empty(k, dtype=torch.int64, device=keys.device)
  _capi.call("tfra_select_lowest", _workspace(keys.device), n, _ptr(keys), _ptr(status),
             4 if status.dtype == torch.int32 else 5, k, _ptr(out), _stream(keys.device))
  return _narrow_keys(out, key_dtype)


COMBINERS = {"sum": 0, "mean": 1, "sqrtn": 2}


def sparse_segment_combine(rows, idx, seg, weights, combiner, n_rows):
  """out[r] = combine over {i: seg[i]==r} of weights[i]*rows[idx[i]]  (seg ascending; SparseSegment*)."""
  rows = rows.to(torch.float32).contiguous()
  idx = idx.to(torch.int32).contiguous()
  seg = seg.to(torch.int64).contiguous()
  if idx.numel() != seg.numel():       # T/math_ops_test.py:60-69
    raise ValueError("indices and segment_ids must have the same number of elements: %d vs %d" % (idx.numel(), seg.numel()))
  if weights is not None and torch.as_tensor(weights).numel() != idx.numel():
    raise ValueError("weights must have one element per index")
  w = None if weights is None else weights.to(torch.float32).contiguous()
  dim = rows.shape[-1]
  out = torch.empty((n_rows, dim), dtype=torch.float32, device=rows.device)
  _capi.call("tfra_sparse_segment_combine", _workspace(rows.device), idx.numel(), dim, _ptr(rows), _ptr(idx), _ptr(seg),
             _ptr(w), COMBINERS[combiner], n_rows, _ptr(out), _stream(rows.device))
  return out


def sparse_segment_combine_weight_grad(rows, idx, grad_out, seg, weights, combiner, grad_scale=None):
  """The gradient of `sparse_segment_combine` with respect to its weights (tfra_sparse_segment_combine_backprop_weights):
  float32 [nnz], dw[p] = d loss / d weights[p] for grad_out = d loss / d out [n_rows, dim].  With d_p = grad_out[seg[p]] . rows[idx[p]],
  s = sum_p w_p d_p over the row and W = sum w (mean) | sum w^2 (sqrtn):  sum d_p | mean (d_p - s / W) / W |
  sqrtn (d_p - (s / W) w_p) / sqrt(W); 0 for a row with W == 0 and for an entry whose row lies outside [0, n_rows).
  weights None = all 1 (the gradient with respect to those ones is still returned).  seg ascending.  Bit-identical to
  `_DeviceTable.find_combine_weight_grad` where both apply.
  A contiguous float16 / bfloat16 grad_out goes down as it is, grad_scale — a one-element float32 device tensor the gradient is
  multiplied by, read by the kernel — with it (tfra_sparse_segment_combine_backprop_weights_typed): bit for bit the result for
  grad_out.float() * grad_scale.  Every other grad_out is up-cast, multiplied in torch where a scale is given, and takes the
  untyped call."""
  rows = rows.to(torch.float32).contiguous()
  dev = rows.device
  idx = idx.to(dev, torch.int32).contiguous().reshape(-1)
  seg = seg.to(dev, torch.int64).contiguous().reshape(-1)
  typed, grad_out = _grads_arg(torch.as_tensor(grad_out), dev, 0, grad_scale)   # (dim 0: the chain call takes halves at any dim)
  if rows.dim() != 2 or grad_out.dim() != 2 or grad_out.shape[1] != rows.shape[1]:
    raise ValueError("rows must be [U, dim] and grad_out [n_rows, dim], got %s and %s" % (list(rows.shape), list(grad_out.shape)))
  nnz = idx.numel()
  if seg.numel() != nnz:
    raise ValueError("indices and segment_ids must have the same number of elements: %d vs %d" % (nnz, seg.numel()))
  if weights is not None and torch.as_tensor(weights).numel() != nnz:
    raise ValueError("weights must have one element per index")
  w = None if weights is None else torch.as_tensor(weights, device=dev).to(torch.float32).contiguous().reshape(-1)
  n_rows, dim = grad_out.shape
  out = torch.empty(nnz, dtype=torch.float32, device=dev)
  if typed is not None:
    _capi.call("tfra_sparse_segment_combine_backprop_weights_typed", _workspace(dev), nnz, dim, _ptr(rows), _ptr(idx),
               ctypes.byref(typed), _ptr(seg), _ptr(w), COMBINERS[combiner], n_rows, _ptr(out), _stream(dev))
    return out
  _capi.call("tfra_sparse_segment_combine_backprop_weights", _workspace(dev), nnz, dim, _ptr(rows), _ptr(idx), _ptr(grad_out),
             _ptr(seg), _ptr(w), COMBINERS[combiner], n_rows, _ptr(out), _stream(dev))
  return out


def sparse_segment_combine_backprop(grad_out, seg, weights, combiner):
  """The backward of `sparse_segment_combine` (TF's SparseSegment{Sum,Mean,SqrtN}Grad with the weights multiply):
  entry_grads[e] = (grad_out[seg[e]] / den) * weights[e], den = 1 (sum) | the row's weight sum (mean) | sqrt of the sum of
  its squared weights (sqrtn), 0 for a row whose weight sum is 0.  grad_out [n_rows, dim] float32, seg [nnz] ascending.
  Returns [nnz, dim]."""
  seg = seg.to(torch.int64).contiguous().reshape(-1)
  dev = seg.device
  grad_out = grad_out.to(dev, torch.float32).contiguous()
  if grad_out.dim() != 2:
    raise ValueError("grad_out must be [n_rows, dim], got %s" % (list(grad_out.shape),))
  n_rows, dim = grad_out.shape
  nnz = seg.numel()
  if weights is not None and torch.as_tensor(weights).numel() != nnz:
    raise ValueError("weights must have one element per entry")
  if nnz and n_rows == 0:
    raise ValueError("entries but no rows")
  w = None if weights is None else torch.as_tensor(weights, device=dev).to(torch.float32).contiguous().reshape(-1)
  out = torch.empty((nnz, dim), dtype=torch.float32, device=dev)
  _capi.call("tfra_sparse_segment_combine_backprop", _workspace(dev), nnz, dim, _ptr(grad_out), _ptr(seg), _ptr(w),
             COMBINERS[combiner], n_rows, _ptr(out), _stream(dev))
  return out
