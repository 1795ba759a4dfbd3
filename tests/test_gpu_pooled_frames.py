"""GPU: the host side of the 14 single pooled calls (forward and weight gradient; tuple and ragged; plain, typed, long, tiered) on the
smallest shape that reaches every branch of it: one table, or one tier over two tables, of 8 keys, dim 8, float32 rows, n_rows = 3,
nnz = 5 with one empty row, mean combiner.  Every refusal is asserted by code and COMPLETE message and leaves a sentinel-filled
output as it was; every early return writes exactly what it should; one live call per entry point is compared bit for bit with the
reference the other tests use for it (its untyped, short or one-table twin; for find_combine itself, find + sparse_segment_combine).
The frames depend on neither dim nor dtype; the kernels are covered by the tests of their units."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -6
F16 = 1
DIM, N_ROWS, NNZ, MEAN = 8, 3, 5, 1
SENTINEL = 0x7B
FWD = ["tfra_table_find_combine", "tfra_table_find_combine_ragged", "tfra_table_find_combine_typed",
       "tfra_table_find_combine_ragged_typed", "tfra_table_find_combine_long", "tfra_table_find_combine_ragged_long",
       "tfra_tier_find_combine", "tfra_tier_find_combine_ragged"]
GRAD = ["tfra_table_find_combine_backprop_weights", "tfra_table_find_combine_ragged_backprop_weights",
        "tfra_table_find_combine_backprop_weights_long", "tfra_table_find_combine_ragged_backprop_weights_long",
        "tfra_tier_find_combine_backprop_weights", "tfra_tier_find_combine_ragged_backprop_weights"]
# the reference of a live call: None = the chain (find + sparse_segment_combine[_weight_grad])
TWIN = {
    "tfra_table_find_combine": None,
    "tfra_table_find_combine_ragged": "tfra_table_find_combine",
    "tfra_table_find_combine_typed": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_typed": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_long": "tfra_table_find_combine",
    "tfra_table_find_combine_ragged_long": "tfra_table_find_combine_ragged",
    "tfra_tier_find_combine": "tfra_table_find_combine",
    "tfra_tier_find_combine_ragged": "tfra_table_find_combine_ragged",
    "tfra_table_find_combine_backprop_weights": None,
    "tfra_table_find_combine_ragged_backprop_weights": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_backprop_weights_long": "tfra_table_find_combine_backprop_weights",
    "tfra_table_find_combine_ragged_backprop_weights_long": "tfra_table_find_combine_ragged_backprop_weights",
    "tfra_tier_find_combine_backprop_weights": "tfra_table_find_combine_backprop_weights",
    "tfra_tier_find_combine_ragged_backprop_weights": "tfra_table_find_combine_ragged_backprop_weights",
}
HINT = {
    ("table", False): " (use tfra_unique + tfra_table_find + tfra_sparse_segment_combine otherwise)",
    ("table", True): " (use tfra_table_find + tfra_sparse_segment_combine_backprop_weights otherwise)",
    ("tier", False): " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine otherwise)",
    ("tier", True): " (use tfra_unique + tfra_tier_find + tfra_sparse_segment_combine_backprop_weights otherwise)",
}
NEEDS_DIM = "needs dim % 4 == 0 and dim <= 256"
TOO_LARGE = "too large (nnz < 2^31, n_rows < 2^30)"
MISALIGNED = "misaligned buffer (out and default_row: 16 bytes)"


def is_grad(name):
  return "backprop" in name


def is_ragged(name):
  return "_ragged" in name


def is_typed(name):
  return name.endswith("_typed")


def owner_kind(name):
  return "tier" if name.startswith("tfra_tier_") else "table"


def prefixes(name):
  """(the prefix of the checks' refusals, the prefix of dw_out's): not uniform across the family, and part of the behaviour"""
  if owner_kind(name) == "tier":
    return (name + ": (out = grad_out) ", name + ": ") if is_grad(name) else (name + ": ", None)
  stem = name[len("tfra_table_"):]
  return (stem + " (out = grad_out): ", stem + ": ") if is_grad(name) else (stem + ": ", None)


def bits(torch, x):
  return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16)


class Env:
  pass


_ENV = []


@pytest.fixture(scope="module")
def env():
  """Made once, left unchanged by every test: a table of keys 1..8 with every key's newest row (the one-table twin); a tier whose
  upper table holds keys 1..4 and the newest row of key 6, and whose lower table holds 5..8 with a stale row of key 6; the same pair
  with dim 6; the batch and the references of the live calls."""
  if _ENV:
    return _ENV[0]
  import torch
  import tfra_amd.dynamic_embedding as de
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tfra_amd.dynamic_embedding.table_ops import _DeviceTable, _DeviceTier, _ptr, _stream
  e = Env()
  e.torch, e.capi, e.lib, e.ptr = torch, _capi, _capi.lib(), _ptr
  cuda = lambda x, dt: torch.tensor(x, dtype=dt, device="cuda")

  def owners(dim, tag):
    tab = lambda n, **kw: _DeviceTable(torch.int64, torch.float32, torch.zeros(dim), "pf_%s_%s" % (n, tag), "cuda:0", dim=dim, **kw)
    table, lower = tab("table"), tab("lower")
    upper = tab("upper", init_capacity=15 * 89, max_capacity=15 * 89, strategy=0)
    return table, upper, lower, _DeviceTier(upper, lower, 64)

  e.table, e.upper, e.lower, e.tier = owners(DIM, "d8")
  e.table6, e.upper6, e.lower6, e.tier6 = owners(6, "d6")
  g = torch.Generator(device="cuda").manual_seed(7)
  keys = torch.arange(1, 9, dtype=torch.int64, device="cuda")
  rows = torch.randn((8, DIM), generator=g, device="cuda")
  e.table.upsert(keys, rows)
  e.upper.upsert(cuda([1, 2, 3, 4, 6], torch.int64), rows[[0, 1, 2, 3, 5]], unique_keys=True)
  e.lower.upsert(keys[4:], rows[4:] + cuda([0, 1, 0, 0], torch.float32).reshape(4, 1))   # key 6 below: stale
  e.dev = e.table.device
  e.ws, e.st = _workspace(e.dev), _stream(e.dev)
  e.ids = cuda([1, 6, 3, 99, 8], torch.int64)             # upper; upper over a stale copy below; upper; in neither; only below
  e.seg = cuda([0, 0, 2, 2, 2], torch.int64)              # row 1 is empty
  e.splits = cuda([0, 2, 2, 5], torch.int64)
  e.weights = torch.rand(NNZ, generator=g, device="cuda") + 0.5
  e.default_row = 0.5 + 0.25 * torch.arange(DIM, dtype=torch.float32, device="cuda")
  e.G = torch.randn((N_ROWS, DIM), generator=g, device="cuda")
  e.fill_key, e.fill_row = 6, rows[5].clone()
  found = e.table.find(e.ids, e.default_row.reshape(1, DIM).repeat(NNZ, 1))
  idx = torch.arange(NNZ, device="cuda")
  e.chain_fwd = de.device_ops.sparse_segment_combine(found, idx, e.seg, e.weights, "mean", N_ROWS)
  e.chain_dw = de.device_ops.sparse_segment_combine_weight_grad(found, idx, e.G, e.seg, e.weights, "mean")
  torch.cuda.synchronize()
  _ENV.append(e)
  return e


def run(e, name, **kw):
  """One call of `name` on the batch with `kw` over its operands (addresses as ctypes.c_void_p or None); returns (rc, message).
  out / grad / dw are addresses; a typed forward takes `out` as the rows of a float16 tfra_rows_out."""
  dim6 = kw.pop("dim6", False)
  tier, table = (e.tier6, e.table6) if dim6 else (e.tier, e.table)
  a = dict(owner=(tier if owner_kind(name) == "tier" else table)._h, ws=e.ws, nnz=NNZ, ids=e.ptr(e.ids), seg=e.ptr(e.seg),
           splits=e.ptr(e.splits), weights=e.ptr(e.weights), combiner=MEAN, n_rows=N_ROWS, flags=0, fill_id=0,
           default_row=e.ptr(e.default_row), out=None, grad=e.ptr(e.G), dw=None)
  assert set(kw) <= set(a), kw
  a.update(kw)
  out = ctypes.byref(e.capi.RowsOut(a["out"].value if a["out"] else None, F16, 0)) if is_typed(name) else a["out"]
  if is_ragged(name):
    args = [a["owner"], a["n_rows"], a["splits"], a["nnz"], a["ids"], a["weights"], a["combiner"], a["flags"], a["fill_id"],
            a["default_row"]]
  else:
    args = [a["owner"], a["ws"], a["nnz"], a["ids"], a["seg"], a["weights"], a["combiner"], a["n_rows"], a["default_row"]]
  args += [a["grad"], a["dw"]] if is_grad(name) else [out]
  rc = getattr(e.lib, name)(*args, e.st)
  return rc, (e.lib.tfra_last_error().decode() if rc else "")


def buffer_of(e, n_bytes=N_ROWS * DIM * 4 + 64):
  return e.torch.full((n_bytes,), SENTINEL, dtype=e.torch.uint8, device="cuda")


def target(name, buf):
  """the operand a call writes, at `buf`"""
  return {"dw" if is_grad(name) else "out": P(buf.data_ptr())}


def live(e, name, **kw):
  """the call's whole output as a tensor: float32 or float16 [n_rows, dim], or float32 [nnz]"""
  torch = e.torch
  buf = buffer_of(e)
  rc, msg = run(e, name, **target(name, buf), **kw)
  assert rc == 0, msg
  torch.cuda.synchronize()
  if is_grad(name):
    n = NNZ * 4
    got = buf[:n].view(torch.float32)
  else:
    n = N_ROWS * DIM * (2 if is_typed(name) else 4)
    got = buf[:n].view(torch.float16 if is_typed(name) else torch.float32).reshape(N_ROWS, DIM)
  assert bool((buf[n:] == SENTINEL).all())
  return got.clone()


@pytest.mark.parametrize("name", FWD + GRAD)
def test_refusals_by_code_and_complete_message(env, name):
  e = env
  buf = buffer_of(e)
  base = target(name, buf)
  checks, dw_prefix = prefixes(name)
  grad, typed = is_grad(name), is_typed(name)
  inp = "grad" if grad else "out"          # the operand the forward's checks look at in the place of out
  inp_at = (lambda off: {"grad": P(e.G.data_ptr() + off)}) if grad else (lambda off: {"out": P(buf.data_ptr() + off)})
  rows_out = "misaligned out.rows (float32: 16 bytes, halves: 8 bytes)"
  matrix = [
      (dict(combiner=3), INVALID, checks + "bad argument"),
      (dict(dim6=True), UNSUPPORTED, checks + NEEDS_DIM + HINT[(owner_kind(name), grad)]),
      (dict(nnz=2**31), UNSUPPORTED, checks + TOO_LARGE),
      (dict(n_rows=2**30), UNSUPPORTED, checks + TOO_LARGE),
      (inp_at(2 if typed else 4), UNSUPPORTED, checks + (rows_out if typed else MISALIGNED)),
      ({inp: None}, INVALID, checks + "null out"),
      (dict(ids=None), INVALID, checks + "null buffer"),
  ]
  if typed:   # a half matrix needs 8 bytes, not the twin's 16
    assert run(e, name, **{**base, **inp_at(8)})[0] == 0
    e.torch.cuda.synchronize()
    buf.fill_(SENTINEL)
  if is_ragged(name):
    matrix += [
        (dict(flags=4), INVALID, checks + "unknown flag bits (TFRA_RAGGED_PRUNE | TFRA_RAGGED_FILL)"),
        (dict(splits=P(e.splits.data_ptr() + 4)), UNSUPPORTED, checks + "misaligned row_splits (8 bytes)"),
        (dict(splits=None), INVALID, checks + "null row_splits"),
    ]
  if grad:
    matrix += [
        (dict(dw=None), INVALID, dw_prefix + "null dw_out"),
        (dict(dw=P(buf.data_ptr() + 2)), UNSUPPORTED, dw_prefix + "misaligned dw_out (4 bytes)"),
    ]
  for kw, code, msg in matrix:
    assert run(e, name, **{**base, **kw}) == (code, msg), kw
  e.torch.cuda.synchronize()
  assert bool((buf == SENTINEL).all())     # nothing was enqueued


@pytest.mark.parametrize("name", FWD)
def test_forward_early_returns(env, name):
  e, torch = env, env.torch
  elem = 2 if is_typed(name) else 4
  buf = buffer_of(e)
  out = target(name, buf)
  # no rows: nothing is written (NULL out would do)
  assert run(e, name, n_rows=0, **out) == (0, "")
  assert run(e, name, n_rows=0, out=None) == (0, "")
  torch.cuda.synchronize()
  assert bool((buf == SENTINEL).all())
  # no entries: all-zero rows of the output's element size, and not a byte more
  assert run(e, name, nnz=0, ids=None, seg=None, weights=None, **out) == (0, "")
  torch.cuda.synchronize()
  n = N_ROWS * DIM * elem
  assert not bool(buf[:n].any()) and bool((buf[n:] == SENTINEL).all())
  if not is_ragged(name):
    return
  # no entries, but a fill row: every row is the row of fill_id, as the untyped twin gives it
  want = e.fill_row.reshape(1, DIM).repeat(N_ROWS, 1)
  twin = live(e, "tfra_table_find_combine_ragged", nnz=0, ids=None, weights=None, flags=2, fill_id=e.fill_key)
  got = live(e, name, nnz=0, ids=None, weights=None, flags=2, fill_id=e.fill_key)
  assert torch.equal(bits(torch, twin), bits(torch, want))
  assert torch.equal(bits(torch, got), bits(torch, twin.to(got.dtype)))


@pytest.mark.parametrize("name", GRAD)
def test_gradient_early_returns(env, name):
  e, torch = env, env.torch
  buf = buffer_of(e)
  dw = target(name, buf)
  # no entries: dw_out is left as it is (NULL would do)
  assert run(e, name, nnz=0, ids=None, seg=None, weights=None, **dw) == (0, "")
  assert run(e, name, nnz=0, ids=None, seg=None, weights=None, dw=None) == (0, "")
  torch.cuda.synchronize()
  assert bool((buf == SENTINEL).all())
  # entries but no rows: every entry is in no row
  assert run(e, name, n_rows=0, **dw) == (0, "")
  torch.cuda.synchronize()
  assert not bool(buf[:NNZ * 4].any()) and bool((buf[NNZ * 4:] == SENTINEL).all())
  # an entry in no row — seg outside [0, n_rows), or outside row_splits' cover — gets 0; the others are the reference's
  seg = torch.tensor([0, 0, 2, 2, 7], dtype=torch.int64, device="cuda")
  splits = torch.tensor([0, 2, 2, 4], dtype=torch.int64, device="cuda")
  got = live(e, name, seg=e.ptr(seg), splits=e.ptr(splits))
  found = e.table.find(e.ids, e.default_row.reshape(1, DIM).repeat(NNZ, 1))
  import tfra_amd.dynamic_embedding as de
  want = de.device_ops.sparse_segment_combine_weight_grad(found, torch.arange(NNZ, device="cuda"), e.G, seg, e.weights, "mean")
  assert int(bits(torch, got)[4]) == 0 and bool(bits(torch, got)[:4].all())
  assert torch.equal(bits(torch, got), bits(torch, want))


@pytest.mark.parametrize("name", FWD + GRAD)
def test_one_live_call_equals_its_reference_bitwise(env, name):
  e, torch = env, env.torch
  got = live(e, name)
  assert bool(torch.isfinite(got.float()).all())
  if TWIN[name] is None:
    want = e.chain_dw if is_grad(name) else e.chain_fwd
  else:
    want = live(e, TWIN[name]).to(got.dtype)
  assert got.shape == want.shape and torch.equal(bits(torch, got), bits(torch, want))
  if not is_grad(name):
    assert not bool(bits(torch, got[1]).any())     # the empty row
  # the tier's second view is read: the cache alone answers key 8 with the default row
  if owner_kind(name) == "tier":
    cache = live(e, TWIN[name], owner=e.upper._h)
    assert not torch.equal(bits(torch, cache), bits(torch, got))
