"""GPU: tfra_field_entries against a NumPy stable sort, exact on all four outputs, through
`device_ops.field_entries` and through the raw call.  Shapes: the reference docstring's, one entry, one field, more fields than
entries, per-sample lengths on both sides of the 64-lane chunk and of the one / two / four wave forms, every slot equal
(stability: positions ascend inside a segment), no samples, no entries, nslots at the cap.  Slots outside [0, nslots) are clamped
and counted, the count accumulating over calls.  Every output stands between guard words that stay intact; a refused call leaves
every output as it was."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64MIN, I64MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
GUARD = 16          # guard words on either side of an output
SENT = -0x5a5a5a5a5a5a5a5b
SENT32 = -0x5a5a5a5b


@pytest.fixture(scope="module")
def env():
  import torch
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import device_ops
  return torch, _capi, device_ops


def model(ids, slots, nslots):
  """(entry_ids, row_splits, entry_pos, entry_seg, bad) by a stable sort on the host"""
  b, s = ids.shape
  bad = int(((slots < 0) | (slots >= nslots)).sum())
  seg = (np.clip(slots, 0, nslots - 1) + np.arange(b, dtype=np.int64).reshape(b, 1) * nslots).reshape(-1)
  order = np.argsort(seg, kind="stable")
  splits = np.searchsorted(seg[order], np.arange(b * nslots + 1), side="left").astype(np.int64)
  return ids.reshape(-1)[order], splits, order.astype(np.int32), seg[order], bad


def block(n_rows, per_row, nslots, seed=0, equal=None):
  rng = np.random.default_rng(1000 * n_rows + 10 * per_row + nslots + seed)
  ids = rng.integers(-(1 << 40), 1 << 40, size=(n_rows, per_row), dtype=np.int64)
  slots = rng.integers(0, nslots, size=(n_rows, per_row), dtype=np.int64) if equal is None else np.full((n_rows, per_row), equal, np.int64)
  return ids, slots


def guarded(torch, n, dtype=None):
  """a buffer of n elements between GUARD sentinel words -> (whole, view)"""
  dtype = dtype or torch.int64
  whole = torch.full((n + 2 * GUARD,), SENT if dtype == torch.int64 else SENT32, dtype=dtype, device="cuda")
  return whole, whole[GUARD:GUARD + n]


def raw(env, n_rows, per_row, nslots, ids, slots, e, rs, pos, seg, bad):
  torch, _capi, dops = env
  p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if torch.is_tensor(t) else t)
  lib = _capi.lib()
  rc = lib.tfra_field_entries(n_rows, per_row, nslots, p(ids), p(slots), p(e), p(rs), p(pos), p(seg), p(bad),
                              dops._stream(torch.device("cuda", torch.cuda.current_device())))
  return rc, lib.tfra_last_error().decode()


def guards_intact(torch, whole, n):
  s = SENT if whole.dtype == torch.int64 else SENT32
  return bool((whole[:GUARD] == s).all()) and bool((whole[GUARD + n:] == s).all())


CASES = [(2, 3, 3), (1, 1, 1), (3, 5, 1), (3, 4, 9), (5, 63, 7), (5, 64, 7), (5, 65, 7), (5, 130, 7), (7, 128, 5), (6, 129, 5),
         (3, 257, 40), (9, 600, 26), (0, 4, 3), (3, 0, 3)]


@pytest.mark.parametrize("n_rows,per_row,nslots", CASES)
def test_kernel_equals_a_stable_sort(env, n_rows, per_row, nslots):
  torch, _capi, dops = env
  ids, slots = block(n_rows, per_row, nslots)
  if (n_rows, per_row, nslots) == (2, 3, 3):   # the reference docstring's block
    ids = np.array([[23, 12, 0], [9, 13, 10]], dtype=np.int64)
    slots = ids % 3
  want = model(ids, slots, nslots)
  n = n_rows * per_row
  ti, ts = torch.from_numpy(ids).cuda(), torch.from_numpy(slots).cuda()
  # the raw call, every output between guard words
  (we, e), (wr, rs), (wq, seg) = guarded(torch, n), guarded(torch, n_rows * nslots + 1), guarded(torch, n)
  wp, pos = guarded(torch, n, torch.int32)
  bad = torch.zeros(1, dtype=torch.int64, device="cuda")
  rc, msg = raw(env, n_rows, per_row, nslots, ti if n else None, ts if n else None, e if n else None, rs, pos if n else None,
                seg if n else None, bad)
  assert rc == 0, msg
  torch.cuda.synchronize()
  if n_rows == 0:   # TFRA_OK and nothing written, the closing split included
    assert bool((wr == SENT).all())
  else:
    assert np.array_equal(rs.cpu().numpy(), want[1])
    if (n_rows, per_row, nslots) == (2, 3, 3):
      assert rs.tolist() == [0, 2, 2, 3, 4, 6, 6] and e.tolist() == [12, 0, 23, 9, 13, 10]
  assert np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(pos.cpu().numpy(), want[2])
  assert np.array_equal(seg.cpu().numpy(), want[3]) and int(bad) == 0
  for whole, m in ((we, n), (wr, n_rows * nslots + 1), (wq, n), (wp, n)):
    assert guards_intact(torch, whole, m)
  # the binding: the same lists, the optional ones only where asked for
  ge, grs, gpos, gseg = dops.field_entries(ti, ts, nslots, want_pos=True)
  assert np.array_equal(ge.cpu().numpy(), want[0]) and np.array_equal(grs.cpu().numpy(), want[1])
  assert np.array_equal(gpos.cpu().numpy(), want[2]) and np.array_equal(gseg.cpu().numpy(), want[3])
  assert grs.dtype == torch.int64 and gpos.dtype == torch.int32 and gseg.dtype == torch.int64
  ge, grs, gpos, gseg = dops.field_entries(ti.to(torch.int32), ts.to(torch.int32), nslots, want_seg=False)
  assert ge.dtype == torch.int32 and gpos is None and gseg is None
  assert np.array_equal(ge.cpu().numpy(), want[0].astype(np.int32)) and np.array_equal(grs.cpu().numpy(), want[1])
  # the torch route gives the same lists
  te, trs, tpos, tseg = dops._field_entries_torch(ti, ts, nslots, want_pos=True)
  assert np.array_equal(te.cpu().numpy(), want[0]) and np.array_equal(trs.cpu().numpy(), want[1])
  assert np.array_equal(tpos.cpu().numpy(), want[2]) and np.array_equal(tseg.cpu().numpy(), want[3])


def test_equal_slots_keep_the_input_order(env):
  """(2, 200, 3), every slot 1: a segment's entries are its sample's ids as they came, positions ascending"""
  torch, _capi, dops = env
  ids, slots = block(2, 200, 3, equal=1)
  e, rs, pos, seg = dops.field_entries(torch.from_numpy(ids).cuda(), torch.from_numpy(slots).cuda(), 3, want_pos=True)
  assert np.array_equal(pos.cpu().numpy(), np.arange(400, dtype=np.int32))
  assert np.array_equal(e.cpu().numpy(), ids.reshape(-1))
  assert rs.tolist() == [0, 0, 200, 200, 200, 400, 400]
  assert np.array_equal(seg.cpu().numpy(), np.repeat(np.array([1, 4], dtype=np.int64), 200))


def test_nslots_at_the_cap(env):
  torch, _capi, dops = env
  cap = dops.FIELD_ENTRIES_MAX_SLOTS
  assert cap >= 1024
  ids, slots = block(2, 300, cap)
  slots[0, :4] = [cap - 1, 0, cap - 1, 0]
  want = model(ids, slots, cap)
  e, rs, pos, seg = dops.field_entries(torch.from_numpy(ids).cuda(), torch.from_numpy(slots).cuda(), cap, want_pos=True)
  assert np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(rs.cpu().numpy(), want[1])
  assert np.array_equal(pos.cpu().numpy(), want[2]) and np.array_equal(seg.cpu().numpy(), want[3])


def test_bad_slots_are_clamped_and_counted(env):
  torch, _capi, dops = env
  nslots = 7
  ids, slots = block(5, 130, nslots, seed=3)
  planted = [(0, 0, -1), (0, 129, nslots), (1, 64, I64MIN), (2, 63, I64MAX), (4, 1, -1), (4, 2, nslots + 100), (4, 128, I64MIN)]
  for b, p, v in planted:
    slots[b, p] = v
  want = model(ids, slots, nslots)
  assert want[4] == len(planted)
  ti, ts = torch.from_numpy(ids).cuda(), torch.from_numpy(slots).cuda()
  bad = torch.full((1,), 100, dtype=torch.int64, device="cuda")
  for call in (1, 2):   # the counter accumulates
    e, rs, pos, seg = dops.field_entries(ti, ts, nslots, want_pos=True, bad=bad)
    assert int(bad) == 100 + call * len(planted)
    assert np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(rs.cpu().numpy(), want[1])
    assert np.array_equal(pos.cpu().numpy(), want[2]) and np.array_equal(seg.cpu().numpy(), want[3])
    assert int(seg.min()) >= 0 and int(seg.max()) < 5 * nslots
  tbad = torch.zeros(1, dtype=torch.int64, device="cuda")
  dops._field_entries_torch(ti, ts, nslots, bad=tbad)
  assert int(tbad) == len(planted)


def test_a_refused_call_writes_nothing(env):
  torch, _capi, dops = env
  cap = dops.FIELD_ENTRIES_MAX_SLOTS
  n_rows, per_row = 3, 40
  n = n_rows * per_row
  ids, slots = block(n_rows, per_row, 5)
  ti, ts = torch.from_numpy(ids).cuda(), torch.from_numpy(slots).cuda()
  room = n_rows * (cap + 1) + 1
  (we, e), (wr, rs), (wq, seg) = guarded(torch, n), guarded(torch, room), guarded(torch, n)
  wp, pos = guarded(torch, n, torch.int32)
  bad = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
  e.fill_(SENT), rs.fill_(SENT), seg.fill_(SENT), pos.fill_(SENT32)
  refusals = [
      ("exceeds", True, dict(nslots=cap + 1)),                                  # beyond the cap: TFRA_ERR_UNSUPPORTED
      ("overlaps", False, dict(seg=e)),                                           # two outputs in one buffer
      ("overlaps", False, dict(seg=e[n // 2:].data_ptr())),                       # ... partly
      ("overlaps", False, dict(bad=rs[3:4])),                                     # the counter inside the splits
      ("overlaps", False, dict(e=ti)),                                            # in place over an input
      ("not 8-byte aligned", False, dict(seg=seg.data_ptr() + 4)),
      ("not 4-byte aligned", False, dict(pos=pos.data_ptr() + 2)),
      ("null row_splits", False, dict(rs=None)),
  ]
  for text, unsupported, change in refusals:
    kw = dict(nslots=5, ids=ti, slots=ts, e=e, rs=rs, pos=pos, seg=seg, bad=bad)
    kw.update(change)
    rc, msg = raw(env, n_rows, per_row, kw["nslots"], kw["ids"], kw["slots"], kw["e"], kw["rs"], kw["pos"], kw["seg"], kw["bad"])
    assert rc != 0 and text in msg, (text, rc, msg)
    assert (rc == -1) == (not unsupported), (text, rc)   # -1: TFRA_ERR_INVALID
  torch.cuda.synchronize()
  for whole in (we, wr, wq):
    assert bool((whole == SENT).all())
  assert bool((wp == SENT32).all()) and int(bad) == SENT
  assert np.array_equal(ti.cpu().numpy(), ids) and np.array_equal(ts.cpu().numpy(), slots)
  # beyond the limits the binding takes the torch route: same lists
  slots_c = np.random.default_rng(5).integers(0, cap + 1, size=(n_rows, per_row), dtype=np.int64)
  want = model(ids, slots_c, cap + 1)
  ge, grs, gpos, gseg = dops.field_entries(ti, torch.from_numpy(slots_c).cuda(), cap + 1, want_pos=True)
  assert np.array_equal(ge.cpu().numpy(), want[0]) and np.array_equal(grs.cpu().numpy(), want[1])
  assert np.array_equal(gpos.cpu().numpy(), want[2]) and np.array_equal(gseg.cpu().numpy(), want[3])
