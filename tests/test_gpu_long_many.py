"""GPU: the grouped pooled calls with long members (tfra_multi_find_combine_long, its ragged form and their *_backprop_weights_long
forms; `long_rows=` of the grouped Python calls).

One list per case over three tables (float32 dim 8, float16 dim 128, bfloat16 dim 256: the three NCH classes and storage types;
the even ids below 600 are resident, the other ids take the default row): the float32 table twice, flagged and not, the two half
tables flagged, and a bfloat16 member of ONE row of 2 100 entries (past the gradient's 2 048-entry LDS park).  The other members'
row lengths are the window edges LENS.  Every member must equal the single *_long call on its descriptor BIT FOR BIT, and a
float64 NumPy restatement under the bound of recursive summation, per element: (L + 4) 2^-24 sum_p |w_p x_p| / |den| for the
forward, L the row's member count, and (L + dim + 4) 2^-24 M_p for the gradient, M_p the gradient's formula with
every term replaced by its magnitude.  Weights lie in [0.5, 1.5], so no denominator is near zero."""
import ctypes

import numpy as np
import pytest

from tests.sparse_helpers import COMB, Calls, T, bits, filled_var

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
MEMBERS = [("float32", 8, True, LENS), ("float32", 8, False, LENS), ("float16", 128, True, LENS), ("bfloat16", 256, True, [2100]),
           ("bfloat16", 256, True, LENS)]
FLAGS = [m[2] for m in MEMBERS]
LONG_CLASSES = 3      # float32 NCH 1, float16 NCH 2, bfloat16 NCH 4 (its two members share one)
FILL = 2              # resident
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  tables = {}
  for vdtype, dim in sorted({m[:2] for m in MEMBERS}):
    dt = getattr(torch, vdtype)
    t = de.CuckooHashTable(torch.int64, dt, torch.full((dim,), 0.375, dtype=dt), name="lm_%s_%d" % (vdtype, dim), dim=dim)
    rows = torch.randn((300, dim), generator=torch.Generator(device="cuda").manual_seed(dim), device="cuda").to(dt)
    t.insert(T(torch, np.arange(0, 600, 2, dtype=np.int64)), rows)
    x = np.full((800, dim), 0.375)
    x[0:600:2] = rows.to(torch.float32).cpu().numpy()
    tables[(vdtype, dim)] = (t, x)
  batches = []
  for k, (vdtype, dim, _, lens) in enumerate(MEMBERS):
    rng = np.random.default_rng(40 + k)
    n = len(lens)
    seg = np.concatenate([np.repeat(np.arange(n), lens), [n + 2] * 3]).astype(np.int64)   # the tail: in no row, outside the cover
    ids = rng.integers(0, 800, size=seg.size).astype(np.int64)
    w = rng.uniform(0.5, 1.5, size=seg.size).astype(np.float32)
    ws = w.copy()                                                                         # the safe run's: a fifth not > 0
    ws[rng.random(seg.size) < 0.2] = -0.5
    ws[rng.random(seg.size) < 0.05] = 0.0
    g = torch.randn((n, dim), generator=torch.Generator(device="cuda").manual_seed(90 + k), device="cuda")
    batches.append(dict(n=n, seg=seg, ids=ids, w=w, ws=ws, rs=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), g=g))
  return torch, de, tables, batches


def reference(x, G, seg, ids, w, member, n, combiner, fill):
  """float64 (out, its bound, dw, its bound) over the member entries; a row without members is x[fill] (zeros for None)."""
  dim = x.shape[1]
  member = member * (seg < n)
  seg = np.minimum(seg, n - 1)
  w = w.astype(np.float64) * member
  E, L = x[ids], np.bincount(seg, weights=member, minlength=n)
  acc, mag = np.zeros((n, dim)), np.zeros((n, dim))
  np.add.at(acc, seg, E * w[:, None])
  np.add.at(mag, seg, np.abs(E * w[:, None]))
  ws = np.bincount(seg, weights=w * w if combiner == "sqrtn" else w, minlength=n)
  den = np.ones(n) if combiner == "sum" else (np.sqrt(ws) if combiner == "sqrtn" else ws)
  ok = den != 0
  safe = np.where(ok, den, 1)
  out, bound = np.where(ok[:, None], acc / safe[:, None], 0), (L + 4)[:, None] * U24 * mag / np.abs(safe)[:, None]
  if fill is not None:
    out[L == 0] = x[fill]
  d, D = (E * G[seg]).sum(1), np.abs(E * G[seg]).sum(1)
  s, S = np.bincount(seg, weights=w * d, minlength=n)[seg], np.bincount(seg, weights=np.abs(w) * D, minlength=n)[seg]
  W, okp = safe[seg], ok[seg] & (member > 0)
  if combiner == "sum":
    dw, M = d, D
  elif combiner == "mean":
    dw, M = (d - s / W) / W, (D + S / np.abs(W)) / np.abs(W)
  else:
    dw, M = (d - (s / ws[seg].clip(1e-300)) * w) / W, (D + (S / ws[seg].clip(1e-300)) * np.abs(w)) / W
  return out, bound, np.where(okp, dw, 0), (L[seg] + dim + 4) * U24 * np.where(okp, M, 0)


def requests(env, form, combiner):
  """(forward requests, gradient requests, per member: the single *_long calls' results) of the case list."""
  torch, de, tables, batches = env
  c, safe = COMB[combiner], form == "ragged_safe"
  fwd, grad, single = [], [], []
  for (vdtype, dim, _, _), b in zip(MEMBERS, batches):
    t = tables[(vdtype, dim)][0]
    ids, seg, rs, w = T(torch, b["ids"]), T(torch, b["seg"]), T(torch, b["rs"]), T(torch, b["ws"] if safe else b["w"])
    if form == "tuple":
      fwd.append((t, ids, seg, w, c, b["n"]))
      grad.append((t, ids, seg, w, c, b["g"]))
      single.append((t.find_combine_long(ids, seg, w, c, b["n"]), t.find_combine_weight_grad_long(ids, seg, w, c, b["g"])))
    else:
      kw = dict(prune=safe, fill_id=FILL if safe else None)
      fwd.append((t, rs, ids, w, c, kw["prune"], kw["fill_id"]))
      grad.append((t, rs, ids, w, c, b["g"], kw["prune"], kw["fill_id"]))
      single.append((t.find_combine_ragged_long(rs, ids, w, c, **kw), t.find_combine_ragged_weight_grad_long(rs, ids, w, c, b["g"], **kw)))
  return fwd, grad, single


def calls_of(form):
  from tfra_amd.dynamic_embedding import table_ops
  return ((table_ops.find_combine_many, table_ops.find_combine_weight_grad_many_long) if form == "tuple" else
          (table_ops.find_combine_ragged_many, table_ops.find_combine_ragged_weight_grad_many_long))


@pytest.mark.parametrize("form", ["tuple", "ragged", "ragged_safe"])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
def test_members_equal_the_single_long_calls_and_the_float64_reference(env, combiner, form):
  torch, de, tables, batches = env
  fwd, grad, single = requests(env, form, combiner)
  short = [i for i, f in enumerate(FLAGS) if not f]
  for many, reqs, which in zip(calls_of(form), (fwd, grad), (0, 1)):
    got, launches = many(reqs, return_launches=True, long_rows=FLAGS)
    assert launches == many([reqs[i] for i in short], return_launches=True)[1] + LONG_CLASSES
    twin, twin_launches = many(reqs, return_launches=True)
    assert many(reqs, return_launches=True, long_rows=False)[1] == many(reqs, return_launches=True, long_rows=[False] * len(reqs))[1] \
        == twin_launches
    for i, ((vdtype, dim, _, _), b) in enumerate(zip(MEMBERS, batches)):
      assert got[i].shape == single[i][which].shape
      assert torch.equal(bits(torch, got[i]), bits(torch, single[i][which])), (i, which)
      assert torch.equal(bits(torch, got[i]), bits(torch, twin[i])), (i, which)
      wv = b["ws"] if form == "ragged_safe" else b["w"]
      member = (wv > 0).astype(np.float64) if form == "ragged_safe" else np.ones(wv.size)
      ref = reference(tables[(vdtype, dim)][1], b["g"].cpu().numpy().astype(np.float64), b["seg"], b["ids"], wv, member, b["n"],
                      combiner, FILL if form == "ragged_safe" else None)
      err = np.abs(got[i].cpu().numpy().astype(np.float64) - ref[2 * which])
      assert np.all(err <= ref[2 * which + 1]), (i, which, float((err - ref[2 * which + 1]).max()))
  for t, _ in tables.values():
    t._table.check_errors()


def wgrad_descs(torch, capi, form, owners, dws):
  """One weight-gradient descriptor per (table handle, tier handle): 40 entries in 2 rows of a dim-8 float32 owner."""
  ragged = form == "ragged"
  typ = capi.FindCombineRaggedWgradDesc if ragged else capi.FindCombineWgradDesc
  ids, seg = torch.arange(40, device="cuda"), torch.arange(40, device="cuda") // 20
  rs, d, g = T(torch, np.int64([0, 20, 40])), torch.zeros(8, device="cuda"), torch.ones((2, 8), device="cuda")
  descs = (typ * len(owners))()
  for e, (table, tier), dw in zip(descs, owners, dws):
    e.struct_size, e.combiner, e.table, e.tier = ctypes.sizeof(typ), 0, table, tier
    e.nnz, e.ids, e.n_rows, e.default_row, e.grad_out, e.dw_out = 40, ids.data_ptr(), 2, d.data_ptr(), g.data_ptr(), dw.data_ptr()
    if ragged:
      e.row_splits = rs.data_ptr()
    else:
      e.seg = seg.data_ptr()
  return descs, (ids, seg, rs, d, g)


@pytest.mark.parametrize("form", ["tuple", "ragged"])
def test_refused_lists_write_nothing(env, form, monkeypatch):
  torch, de, tables, batches = env
  from tfra_amd import _capi
  from tfra_amd.dynamic_embedding import table_ops
  from tfra_amd.dynamic_embedding.device_ops import _workspace
  from tests.test_gpu_tier_pooled import setup_of
  dev = torch.device("cuda", torch.cuda.current_device())
  name = "tfra_multi_find_combine%s_backprop_weights_long" % ("_ragged" if form == "ragged" else "")
  table = tables[("float32", 8)][0]._table._h.value
  tier = table_ops._device_tier(setup_of(torch, 64, "float32").tier)._h.value
  buf = torch.full((100,), 7.0, device="cuda")
  for owners, dws, code, words in (([(table, None), (None, tier)], [buf[:40], buf[40:80]], -6, "plain tables only"),
                                   ([(table, None), (table, None)], [buf[:40], buf[20:60]], -1, "dw_out overlaps the dw_out of descriptor 0")):
    descs, keep = wgrad_descs(torch, _capi, form, owners, dws)
    launches = ctypes.c_uint32(9)
    rc = getattr(_capi.lib(), name)(_workspace(dev), 2, ctypes.c_void_p(ctypes.addressof(descs)),
                                    ctypes.c_void_p(ctypes.addressof(launches)), None, table_ops._stream(dev))
    torch.cuda.synchronize()
    msg = _capi.lib().tfra_last_error().decode()
    assert rc == code and words in msg and "descriptor 1" in msg and launches.value == 0, msg
    assert bool((buf == 7.0).all())
  # the Python layer: one flag per request, or one for the list — refused before any C call
  fwd, grad, _ = requests(env, form, "sum")
  calls = Calls(monkeypatch)
  for many, reqs in zip(calls_of(form), (fwd, grad)):
    with pytest.raises(ValueError, match="long_rows must be one bool or one per request"):
      many(reqs, long_rows=[True] * (len(reqs) - 1))
  assert not calls.n


@pytest.mark.parametrize("safe", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
def test_the_public_many_calls_take_the_long_route(env, monkeypatch, ragged, safe):
  """`*_lookup_sparse_many(..., long_rows=[...])` and `sparse_weights_grad_many` on its wrappers against the per-table calls."""
  torch, de = env[:2]
  from tfra_amd.dynamic_embedding import ragged_embedding_ops as rg
  mod = rg if ragged else de
  fn = "safe_embedding_lookup_sparse" if safe else "embedding_lookup_sparse"
  single, many = getattr(mod, fn), getattr(mod, fn + "_many")
  vs = [filled_var(torch, de, "lm_pub_%d_%d_%d" % (ragged, safe, k), dim=dim, initializer=0.5) for k, dim in enumerate((64, 16))]
  lens, flags = [0, 300, 3, 70], [True, False]
  rng = np.random.default_rng(8)
  seg = np.repeat(np.arange(len(lens)), lens).astype(np.int64)
  ids, w = T(torch, rng.integers(0, 3000, size=seg.size).astype(np.int64)), T(torch, rng.uniform(0.5, 1.5, size=seg.size).astype(np.float32))
  sp = (T(torch, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)), ids) if ragged else (T(torch, seg), ids)
  kw = dict(combiner="mean", return_trainable=True, **({} if ragged else {"num_rows": len(lens)}), **({"default_id": 4} if safe else {}))
  gs = [torch.randn((len(lens), v.dim), generator=torch.Generator(device="cuda").manual_seed(v.dim), device="cuda") for v in vs]
  exp = [single(v, sp, w, long_rows=f, **kw) for v, f in zip(vs, flags)]
  exp_dw = [tw.weights_grad(g) for (_, tw), g in zip(exp, gs)]
  calls = Calls(monkeypatch)
  got = many(vs, [sp, sp], [w, w], long_rows=flags, **kw)
  dws = de.sparse_weights_grad_many([(g, tw) for g, (_, tw) in zip(gs, got)])
  stem = "tfra_multi_find_combine_ragged" if ragged else "tfra_multi_find_combine"
  assert calls[stem + "_long"] == 1 and calls["tfra_multi_find_combine_backprop_weights_long"] == 1 and calls[stem] == 0
  today = many(vs, [sp, sp], [w, w], long_rows=False, **kw)
  assert calls[stem] == 1 and calls[stem + "_long"] == 1
  for k in range(2):
    assert got[k][1]._long_rows is flags[k] and today[k][1]._long_rows is False
    assert torch.equal(bits(torch, got[k][0]), bits(torch, exp[k][0])) and torch.equal(bits(torch, today[k][0]), bits(torch, exp[k][0]))
    assert torch.equal(bits(torch, dws[k]), bits(torch, exp_dw[k]))
