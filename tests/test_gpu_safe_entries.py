"""GPU: tfra_multi_safe_entries / device_ops.safe_entries_many — the kept lists and entry lists of many safe sparse lookups, built
on the device.

Every list is compared element for element with two oracles: `model` below, the header's rule restated row by row in numpy, and
`variable._safe_sparse_args_torch`, the torch preprocessing the builder replaces (where that code accepts the input: it has no
ragged form and no rows outside [0, n_rows)).  ids, rows and counts exactly, weights bit for bit.  The raw calls' buffers are
longer than the lists can get and hold a pattern first: nothing may be written at or beyond nnz (kept) and nnz + n_rows (entry).
The shapes sit around the kernels' tile of 1024 entries or rows."""
import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_ = 1024            # the kernels' tile
PAD = 96             # elements behind every output buffer's specified length
SENT = -7777         # what the int64 outputs and the counts hold before a call
FSENT = 123.25       # and the float outputs
PRUNE, FILL, RAGGED = 1, 2, 4
IMIN, IMAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
WEIGHTS = np.array([-1.0, -0.0, 0.0, 0.5, 2.0, np.nan, np.inf], np.float32)
INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def T(torch, a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def rows_of(rows, nnz, n_rows, ragged):
  """every entry's row, -1 where it has none in [0, n_rows)"""
  if not ragged:
    return np.where((rows >= 0) & (rows < n_rows), rows, -1).astype(np.int64)
  out = np.full(nnz, -1, np.int64)
  for r in range(n_rows):
    out[max(0, rows[r]):max(0, min(nnz, rows[r + 1]))] = r
  return out


def model(rows, ids, w, n_rows, flags, fill_id):
  """(kept ids, rows, weights), (entry ids, rows, weights) by the rule of include/tfra_mi355x.h, row by row"""
  nnz = ids.size
  row = rows_of(rows, nnz, n_rows, bool(flags & RAGGED))
  member = row >= 0
  if (flags & PRUNE) and w is not None:
    with np.errstate(invalid="ignore"):
      member &= w > 0
  kept = (ids[member], row[member], None if w is None else w[member])
  of_row = [[] for _ in range(n_rows)]
  for p in np.nonzero(member)[0]:
    of_row[row[p]].append(p)
  e_ids, e_rows, e_w = [], [], []
  for r in range(n_rows):
    if of_row[r]:
      for p in of_row[r]:
        e_ids.append(ids[p]); e_rows.append(r); e_w.append(np.float32(1.0) if w is None else w[p])
    else:
      e_ids.append(fill_id if flags & FILL else 0); e_rows.append(r); e_w.append(np.float32(1.0 if flags & FILL else 0.0))
  return kept, (np.array(e_ids, np.int64), np.array(e_rows, np.int64), np.array(e_w, np.float32))


def torch_lists(torch, spec):
  """the same lists from `_safe_sparse_args_torch` (tuple form, rows in range), weights None where that code returns None"""
  from tfra_amd.dynamic_embedding import variable
  params = types.SimpleNamespace(_primary=torch.device("cuda", torch.cuda.current_device()), dim=4)
  rows, ids, w, n, flags, fill = spec["rows"], spec["ids"], spec["w"], spec["n_rows"], spec["flags"], spec["fill_id"]
  if flags & RAGGED:
    rows = rows_of(rows, ids.size, n, True)
  combiner = "mean" if (flags & PRUNE) else "sum"
  r, i, ww, n2, ent, _, _ = variable._safe_sparse_args_torch(params, (T(torch, rows), T(torch, ids)), None if w is None else T(torch, w),
                                                             combiner, fill if flags & FILL else None, True, n)
  assert n2 == n
  return (i, r, ww), ent


def batch(rng, nnz, n_rows, empty=0.25, weights=True):
  """ascending rows with about `empty` of the rows left out, ids around zero, weights from WEIGHTS"""
  live = np.nonzero(rng.random(n_rows) >= empty)[0]
  live = live if live.size else np.zeros(1, np.int64)
  rows = np.sort(rng.choice(live, size=nnz)) if (nnz and live.size) else np.zeros(0, np.int64)
  ids = rng.integers(-50, 50, size=rows.size).astype(np.int64)
  w = WEIGHTS[rng.integers(0, WEIGHTS.size, size=rows.size)] if weights else None
  return rows.astype(np.int64), ids, w


def splits_of(rows, n_rows):
  return np.searchsorted(rows, np.arange(n_rows + 1), side="left").astype(np.int64)


def spec_of(rows, ids, w, n_rows, flags, fill_id=0, kept=True, ent=True, ent_w=True):
  return dict(rows=np.asarray(rows, np.int64), ids=np.asarray(ids, np.int64), w=None if w is None else np.asarray(w, np.float32),
              n_rows=n_rows, flags=flags, fill_id=fill_id, kept=kept, ent=ent, ent_w=ent_w)


class Raw:
  """tfra_multi_safe_entries itself over buffers of the test's own, filled with the patterns first"""

  def __init__(self, torch, de, specs):
    from tfra_amd import _capi
    from tfra_amd.dynamic_embedding import _args
    self.torch, self.capi, self.args, self.de, self.specs = torch, _capi, _args, de, specs
    full = lambda n, v, dt: torch.full((n + PAD,), v, dtype=dt, device="cuda")
    self.inp, self.out = [], []
    self.counts = torch.full((len(specs), 2), SENT, dtype=torch.int64, device="cuda")
    self.descs = (_capi.SafeEntriesDesc * len(specs))()
    for k, s in enumerate(specs):
      nnz, n = s["ids"].size, s["n_rows"]
      rows, ids = T(torch, s["rows"]), T(torch, s["ids"])
      w = None if s["w"] is None else T(torch, s["w"])
      self.inp.append((rows, ids, w))
      o = dict(kept_ids=full(nnz, SENT, torch.int64), kept_rows=full(nnz, SENT, torch.int64), kept_weights=full(nnz, FSENT, torch.float32),
               entry_ids=full(nnz + n, SENT, torch.int64), entry_rows=full(nnz + n, SENT, torch.int64),
               entry_weights=full(nnz + n, FSENT, torch.float32))
      self.out.append(o)
      e = self.descs[k]
      e.struct_size, e.flags, e.n_rows, e.nnz = ctypes.sizeof(_capi.SafeEntriesDesc), s["flags"], n, nnz
      e.rows = rows.data_ptr() if rows.numel() else None
      e.ids = ids.data_ptr() if nnz else None
      e.weights = w.data_ptr() if (w is not None and nnz) else None
      e.fill_id = s["fill_id"]
      if s["kept"]:
        e.kept_ids, e.kept_rows = o["kept_ids"].data_ptr(), o["kept_rows"].data_ptr()
        e.kept_weights = o["kept_weights"].data_ptr() if e.weights else None
      if s["ent"]:
        e.entry_ids, e.entry_rows = o["entry_ids"].data_ptr(), o["entry_rows"].data_ptr()
        e.entry_weights = o["entry_weights"].data_ptr() if s["ent_w"] else None
      e.d_counts = self.counts[k].data_ptr()

  def call(self, n_lists=None, descs="own"):
    dev = self.torch.device("cuda", self.torch.cuda.current_device())
    launches = ctypes.c_uint32(99)
    d = ctypes.c_void_p(ctypes.addressof(self.descs)) if descs == "own" else descs
    rc = self.capi.lib().tfra_multi_safe_entries(self.de.device_ops._workspace(dev), len(self.specs) if n_lists is None else n_lists, d,
                                                 ctypes.byref(launches), self.args._stream(dev))
    return rc, launches.value, self.capi.lib().tfra_last_error().decode()

  def untouched(self):
    self.torch.cuda.synchronize()
    return bool((self.counts == SENT).all()) and all(bool((b == (FSENT if b.dtype == self.torch.float32 else SENT)).all())
                                                     for o in self.out for b in o.values())

  def lists(self, k):
    """list k as numpy: counts, kept (ids, rows, w), entries (ids, rows, w), trimmed to the counts; the tails are checked here"""
    s, o = self.specs[k], {n: b.cpu().numpy() for n, b in self.out[k].items()}
    nnz, n = s["ids"].size, s["n_rows"]
    nk, ne = (int(x) for x in self.counts[k].cpu().numpy())
    assert 0 <= nk <= nnz and nk <= ne <= nnz + n, (k, nk, ne)
    has_w = s["w"] is not None and nnz > 0
    for name, length, on in (("kept_ids", nnz, s["kept"]), ("kept_rows", nnz, s["kept"]), ("kept_weights", nnz, s["kept"] and has_w),
                             ("entry_ids", nnz + n, s["ent"]), ("entry_rows", nnz + n, s["ent"]),
                             ("entry_weights", nnz + n, s["ent"] and s["ent_w"])):
      sent = FSENT if name.endswith("weights") else SENT
      tail = o[name][length:] if on else o[name]
      assert (tail == sent).all(), (k, name, "written at or beyond the buffer's length, or where nothing was asked for")
    return (nk, ne), (o["kept_ids"][:nk], o["kept_rows"][:nk], o["kept_weights"][:nk]), \
        (o["entry_ids"][:ne], o["entry_rows"][:ne], o["entry_weights"][:ne])

  def check(self, tag="", with_torch=True):
    for k, s in enumerate(self.specs):
      (nk, ne), kept, ent = self.lists(k)
      mk, me = model(s["rows"], s["ids"], s["w"], s["n_rows"], s["flags"], s["fill_id"])
      assert (nk, ne) == (mk[0].size, me[0].size), (tag, k, nk, ne, mk[0].size, me[0].size)
      tk, te = torch_lists(self.torch, s) if with_torch else (None, None)
      if s["kept"]:
        np.testing.assert_array_equal(kept[0], mk[0], err_msg=str((tag, k)))
        np.testing.assert_array_equal(kept[1], mk[1], err_msg=str((tag, k)))
        if s["w"] is not None and s["ids"].size:
          np.testing.assert_array_equal(bits(kept[2]), bits(mk[2]), err_msg=str((tag, k)))
        if with_torch:
          np.testing.assert_array_equal(kept[0], tk[0].cpu().numpy())
          np.testing.assert_array_equal(kept[1], tk[1].cpu().numpy())
          if tk[2] is not None and s["ids"].size:
            np.testing.assert_array_equal(bits(kept[2]), bits(tk[2].cpu().numpy()))
      if s["ent"]:
        np.testing.assert_array_equal(ent[0], me[0], err_msg=str((tag, k)))
        np.testing.assert_array_equal(ent[1], me[1], err_msg=str((tag, k)))
        if s["ent_w"]:
          np.testing.assert_array_equal(bits(ent[2]), bits(me[2]), err_msg=str((tag, k)))
        if with_torch:
          assert te[0].numel() == ne
          np.testing.assert_array_equal(ent[0], te[0].cpu().numpy())
          np.testing.assert_array_equal(ent[1], te[1].cpu().numpy())
          if te[2] is not None and s["ent_w"]:
            np.testing.assert_array_equal(bits(ent[2]), bits(te[2].cpu().numpy()))


def run(torch, de, specs, tag="", with_torch=True, launches=None):
  r = Raw(torch, de, specs)
  rc, n_launch, msg = r.call()
  assert rc == 0, msg
  if launches is not None:
    assert n_launch == launches, (tag, n_launch)
  r.check(tag, with_torch)
  return r, n_launch


# ---- shapes around the tile -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, T_ - 1, T_, T_ + 1, 2 * T_ + 3])
@pytest.mark.parametrize("nnz", [0, 1, T_ - 1, T_, T_ + 1, 3 * T_ + 5])
def test_tile_edges_tuple_and_ragged(env, nnz, n_rows):
  torch, de = env
  rows, ids, w = batch(np.random.default_rng(nnz * 7 + n_rows), nnz, n_rows)
  sp = splits_of(rows, n_rows)
  specs = [spec_of(rows, ids, w, n_rows, PRUNE | FILL, 77), spec_of(sp, ids, w, n_rows, PRUNE | FILL | RAGGED, 77),
           spec_of(rows, ids, w, n_rows, 0), spec_of(sp, ids, w, n_rows, RAGGED),
           spec_of(rows, ids, None, n_rows, FILL, -3), spec_of(rows, ids, None, n_rows, PRUNE), spec_of(sp, ids, None, n_rows, RAGGED | FILL, -3)]
  for k, s in enumerate(specs):   # one list per call
    run(torch, de, [s], (nnz, n_rows, k), launches=5 if (s["flags"] & PRUNE and s["w"] is not None and nnz) else 3)
  r, _ = run(torch, de, specs, (nnz, n_rows, "grouped"), with_torch=False)   # the tuple and the ragged form give equal lists
  for a, b in ((0, 1), (2, 3), (4, 6)):
    for x, y in zip(r.lists(a)[1] + r.lists(a)[2], r.lists(b)[1] + r.lists(b)[2]):
      np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def _special(name):
  rng = np.random.default_rng(5)
  if name == "all_pruned":
    rows, ids, _ = batch(rng, T_ + 9, 40, weights=False)
    return spec_of(rows, ids, np.full(rows.size, -1.0, np.float32), 40, PRUNE | FILL, 5)
  if name == "all_rows_empty":
    return spec_of([], [], np.zeros(0, np.float32), T_ + 1, PRUNE | FILL, 9)
  if name == "empty_rows_at_both_ends":
    rows, ids, w = batch(rng, 300, 50, empty=0.0)
    return spec_of(rows + 7, ids, w, 50 + 7 + 11, PRUNE)
  if name == "one_row_over_three_tiles":
    nnz = 3 * T_ + 5
    w = WEIGHTS[rng.integers(0, WEIGHTS.size, size=nnz)]
    return spec_of(np.ones(nnz, np.int64), rng.integers(0, 9, size=nnz), w, 3, PRUNE | FILL, 4)
  if name == "pruned_row_over_a_tile_border":
    rows = np.repeat(np.arange(6), [T_ - 4, 7, 5, T_ - 11, 7, 20])   # rows 1 and 4 straddle the borders at 1024 and 2048
    w = np.ones(rows.size, np.float32)
    w[(rows == 1) | (rows == 4)] = np.tile(np.array([-1.0, 0.0, -0.0, np.nan, -2.0, 0.0, -1.0], np.float32), 2)
    return spec_of(rows, np.arange(rows.size), w, 6, PRUNE | FILL, -8)
  if name == "sum_keeps_every_weight":
    rows, ids, w = batch(rng, 2 * T_ + 1, 333)
    return spec_of(rows, ids, w, 333, FILL, 1)
  raise KeyError(name)


@pytest.mark.parametrize("name", ["all_pruned", "all_rows_empty", "empty_rows_at_both_ends", "one_row_over_three_tiles",
                                  "pruned_row_over_a_tile_border", "sum_keeps_every_weight"])
def test_special_batches(env, name):
  torch, de = env
  s = _special(name)
  run(torch, de, [s], name)
  run(torch, de, [dict(s, rows=splits_of(s["rows"], s["n_rows"]), flags=s["flags"] | RAGGED)], name + "/ragged")


@pytest.mark.parametrize("fill_id", [0, -1, IMIN, IMAX])
def test_fill_ids(env, fill_id):
  torch, de = env
  rows, ids, w = batch(np.random.default_rng(3), T_ + 3, 90)
  run(torch, de, [spec_of(rows, ids, w, 90, PRUNE | FILL, fill_id), spec_of(rows, ids, None, 90, FILL, fill_id),
                  spec_of(rows, ids, w, 90, PRUNE, fill_id)], fill_id)   # (without FILL the id is 0 whatever fill_id says)


def test_rows_outside_the_range_are_in_neither_list(env):
  torch, de = env
  rng = np.random.default_rng(8)
  rows, ids, w = batch(rng, T_ + 40, 60)
  rows = np.concatenate([[-9, -9, -1], rows, [60, 60, 61, 1 << 40]]).astype(np.int64)
  ids = np.concatenate([[1, 2, 3], ids, [4, 5, 6, 7]]).astype(np.int64)
  w = np.concatenate([[2, 2, 2], w, [2, 2, 2, 2]]).astype(np.float32)
  sp = splits_of(rows[3:-4], 60) + 3   # the ragged twin: three entries in front of the first split, four behind the last
  specs = [spec_of(rows, ids, w, 60, PRUNE | FILL, 11), spec_of(rows, ids, None, 60, 0), spec_of(rows, ids, w, 60, FILL, 11),
           spec_of(sp, ids, w, 60, PRUNE | FILL | RAGGED, 11), spec_of(sp, ids, None, 60, RAGGED),
           spec_of(rows, ids, w, 0, PRUNE | FILL, 11)]   # no rows at all: every entry lies outside, both counts 0
  r, _ = run(torch, de, specs, "outside", with_torch=False)
  assert r.lists(0)[0] == r.lists(3)[0] and r.lists(1)[0][0] == T_ + 40 and r.lists(5)[0] == (0, 0)


def test_kept_only_entries_only_and_counts_only(env):
  torch, de = env
  rows, ids, w = batch(np.random.default_rng(12), 2 * T_ + 7, T_ + 2)
  n = T_ + 2
  specs = [spec_of(rows, ids, w, n, PRUNE | FILL, 6, ent=False), spec_of(rows, ids, w, n, PRUNE | FILL, 6, kept=False),
           spec_of(rows, ids, w, n, PRUNE | FILL, 6, kept=False, ent=False), spec_of(rows, ids, w, n, PRUNE | FILL, 6, ent_w=False),
           spec_of(rows, ids, None, n, FILL, 6, kept=False, ent_w=False)]
  for k, s in enumerate(specs):
    run(torch, de, [s], ("only", k), launches=4 if k == 2 else 3 if k == 4 else 5)
  run(torch, de, specs, "only/grouped")


# ---- grouped ----------------------------------------------------------------------------------------------------------------------
def _mixed(n_lists):
  rng = np.random.default_rng(100 + n_lists)
  sizes = [(3 * T_ + 5, T_ + 1), (0, 17), (700, 2 * T_ + 3), (5, 0), (T_, T_), (0, 0), (1, 1), (T_ + 1, 3)]
  specs = []
  for k in range(n_lists):
    nnz, n = sizes[k % len(sizes)]
    rows, ids, w = batch(rng, nnz if n else 0, n) if n else (np.zeros(0, np.int64),) * 2 + (np.zeros(0, np.float32),)
    flags = [PRUNE | FILL, PRUNE, FILL, 0][k % 4]
    if k % 3 == 1 and n:
      rows, flags = splits_of(rows, n), flags | RAGGED
    specs.append(spec_of(rows, ids, w if k % 5 != 4 else None, n, flags, k - 4))
  return specs


def test_grouped_lists_equal_their_single_calls(env):
  torch, de = env
  launches = {}
  for n_lists in (1, 2, 26):
    specs = _mixed(n_lists)
    r, launches[n_lists] = run(torch, de, specs, ("mixed", n_lists))
    for k, s in enumerate(specs):
      single = Raw(torch, de, [s])
      assert single.call()[0] == 0
      a, b = single.lists(0), r.lists(k)
      assert a[0] == b[0], (n_lists, k)
      for x, y in zip(a[1] + a[2], b[1] + b[2]):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                      y.view(np.uint32) if y.dtype == np.float32 else y, err_msg=str((n_lists, k)))
  assert launches[2] == launches[26] and launches[26] <= 6, launches


def test_back_to_back_calls_of_changing_layouts(env):
  torch, de = env
  raws = [Raw(torch, de, _mixed(n)) for n in (26, 3, 9, 26, 1, 14, 2, 26, 5, 11)]   # more calls than the staging ring has slots
  for r in raws:
    assert r.call()[0] == 0
  for r in raws:
    r.check("ring", with_torch=False)


# ---- the binding -------------------------------------------------------------------------------------------------------------------
def test_the_binding_trims_in_one_read_and_keeps_int32_ids(env, monkeypatch):
  torch, de = env
  rng = np.random.default_rng(21)
  reqs, specs = [], []
  for k, (nnz, n) in enumerate([(T_ + 3, 50), (0, 9), (300, T_ + 1), (40, 0)]):
    rows, ids, w = batch(rng, nnz if n else 0, n) if n else (np.zeros(0, np.int64),) * 2 + (np.zeros(0, np.float32),)
    ragged = k == 2
    fill = None if k == 1 else 13
    dt = np.int32 if k in (0, 2) else np.int64
    reqs.append((T(torch, splits_of(rows, n) if ragged else rows), T(torch, ids.astype(dt)), T(torch, w) if k != 3 else None, n, k != 3, fill,
                 ragged))
    specs.append(spec_of(rows, ids, w if k != 3 else None, n, (PRUNE if k != 3 else 0) | (FILL if fill is not None else 0), fill or 0))
  reads = []
  real = de.device_ops._read_counts
  monkeypatch.setattr(de.device_ops, "_read_counts", lambda c: (reads.append(tuple(c.shape)), _relaxed(torch, real, c))[1])
  torch.cuda.set_sync_debug_mode("error")   # the builder itself never synchronises; the one read is a function of its own
  try:
    res, launches = de.device_ops.safe_entries_many(reqs, return_launches=True)
  finally:
    torch.cuda.set_sync_debug_mode("default")
  assert reads == [(4, 2)] and launches == 5
  for k, ((kept, ent), s) in enumerate(zip(res, specs)):
    mk, me = model(s["rows"], s["ids"], s["w"], s["n_rows"], s["flags"], s["fill_id"])
    assert kept[0].dtype == reqs[k][1].dtype and ent[0].dtype == reqs[k][1].dtype
    np.testing.assert_array_equal(kept[0].cpu().numpy(), mk[0]); np.testing.assert_array_equal(kept[1].cpu().numpy(), mk[1])
    np.testing.assert_array_equal(ent[0].cpu().numpy(), me[0]); np.testing.assert_array_equal(ent[1].cpu().numpy(), me[1])
    if s["w"] is None:
      assert kept[2] is None and ent[2] is None            # (fill given: the entry weights would all be 1)
    else:
      np.testing.assert_array_equal(bits(kept[2].cpu().numpy()), bits(mk[2]))
      np.testing.assert_array_equal(bits(ent[2].cpu().numpy()), bits(me[2]))
  only = de.device_ops.safe_entries_many(reqs, want_kept=[True, False, False, False], want_entries=False)
  assert only[0][1] is None and only[1] == (None, None) and only[0][0][0].numel() == res[0][0][0].numel()
  with pytest.raises(ValueError):
    de.device_ops.safe_entries_many([(reqs[0][0][:-1],) + reqs[0][1:]])


def _relaxed(torch, fn, *a):
  """fn(*a) with synchronising calls allowed, whatever the mode around it"""
  mode = torch.cuda.get_sync_debug_mode()
  torch.cuda.set_sync_debug_mode("default")
  try:
    return fn(*a)
  finally:
    torch.cuda.set_sync_debug_mode(mode)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
REFUSALS = ["struct_size", "flags", "null_descs", "null_rows", "null_splits", "null_ids", "null_counts", "kept_without_rows",
            "kept_without_weights", "kept_weights_alone", "entries_without_rows", "entry_weights_alone", "overlap", "overlap_counts",
            "int64_misaligned", "float_misaligned", "list_too_long", "total_too_long"]


@pytest.mark.parametrize("what", REFUSALS)
def test_a_refused_call_writes_nothing(env, what):
  torch, de = env
  rng = np.random.default_rng(2)
  specs = []
  for n in (40, 70):
    rows, ids, w = batch(rng, 300, n)
    specs.append(spec_of(rows, ids, w, n, PRUNE | FILL, 3))
  specs.append(dict(specs[1], rows=splits_of(specs[1]["rows"], 70), flags=PRUNE | RAGGED))
  r = Raw(torch, de, specs)
  e, o, code, descs = r.descs[1], r.out[1], INVALID, "own"
  if what == "struct_size":
    e.struct_size -= 8
  elif what == "flags":
    e.flags |= 8
  elif what == "null_descs":
    descs = None
  elif what == "null_rows":
    e.rows = None
  elif what == "null_splits":
    r.descs[2].rows, r.descs[2].nnz = None, 0
  elif what == "null_ids":
    e.ids = None
  elif what == "null_counts":
    e.d_counts = None
  elif what == "kept_without_rows":
    e.kept_rows = None
  elif what == "kept_without_weights":
    e.kept_weights = None
  elif what == "kept_weights_alone":
    e.kept_ids = e.kept_rows = None
  elif what == "entries_without_rows":
    e.entry_rows = None
  elif what == "entry_weights_alone":
    e.entry_ids = e.entry_rows = None
  elif what == "overlap":
    r.descs[2].entry_ids = o["entry_ids"].data_ptr() + 8 * 100
  elif what == "overlap_counts":
    r.descs[2].d_counts = r.counts[1].data_ptr() + 8
  elif what == "int64_misaligned":
    e.entry_rows = o["entry_rows"].data_ptr() + 4
  elif what == "float_misaligned":
    e.kept_weights = o["kept_weights"].data_ptr() + 2
  elif what == "list_too_long":
    e.nnz, code = (1 << 31) - 70, UNSUPPORTED
  elif what == "total_too_long":
    r.descs[0].nnz, e.nnz, code = (1 << 23), (1 << 23) - 100, UNSUPPORTED
  rc, launches, msg = r.call(descs=descs)
  assert rc == code and launches == 0, (rc, msg)
  assert "multi_safe_entries" in msg
  if what != "null_descs":
    assert "descriptor %d" % (2 if what in ("null_splits", "overlap", "overlap_counts") else 1) in msg, msg
  assert r.untouched()
  good = Raw(torch, de, specs)   # and the same descriptors, left alone, are served
  assert good.call()[0] == 0
  good.check(what)
