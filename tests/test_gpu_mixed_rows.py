"""GPU: the mixed-row pooled lookup and weight gradient (tfra_table_find_combine_mixed, its ragged form and their
*_backprop_weights_mixed forms; the `mixed_rows` keyword of the sparse lookups).

One crafted batch of 37 rows — two full blocks of 16 and a partial one of 5 — whose lengths take every boundary of a group's
4-entry batch and 16-id load and of the windows of 16, 32 and 64 entries.  With long_from = 64 block 0 has its first and its last
row done by the block and block 1 two neighbouring rows (LDS reuse); the smaller thresholds move that border through every
length, 1 makes every row with an entry the block's and 1000 none.  Ids from 80 values of which the 40 even ones are resident.
long_from changes who computes a row, never the result: every mixed call must equal its twin BIT FOR BIT (torch.equal on int32
views) and lie within the recursive-summation bound of a float64 NumPy reference, per element: (L + 2) 2^-24 sum_p |w_p x_p| /
|den| for the forward, L the row's member count, and (L + dim + 4) 2^-24 M_p for the gradient, M_p the gradient's formula with
every term replaced by its magnitude."""
import numpy as np
import pytest

from tests.sparse_helpers import COMB, Calls, T, bits, filled_var

pytestmark = pytest.mark.gpu

LENS = [129, 0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 1, 3, 65,
        4, 64, 65, 1, 5, 16, 0, 17, 33, 2, 63, 32, 15, 3, 31, 1,
        3, 129, 64, 1, 17]
N = len(LENS)
ZERO_ROW = 5          # its weights are all 0: weight sum 0, and under PRUNE a row whose members are all pruned
LONG_FROM = [1, 5, 17, 64, 0, 1000]
U24 = 2.0 ** -24
CLASSES = [("float32", 4), ("float32", 64), ("float16", 128), ("bfloat16", 256)]
FORMS = {"tuple": None, "ragged": None, "safe_fill_hit": 2, "safe_fill_miss": 3}   # form -> fill id


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  rng = np.random.default_rng(41)
  rs = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
  seg = np.repeat(np.arange(N), LENS).astype(np.int64)
  ids = rng.integers(0, 80, size=seg.size).astype(np.int64)
  w = rng.uniform(0.25, 2.0, size=seg.size).astype(np.float32)
  w[seg == ZERO_ROW] = 0.0
  wp = w.copy()                                          # the PRUNE form's weights: a fifth of them <= 0
  wp[rng.random(seg.size) < 0.15] = -0.5
  wp[rng.random(seg.size) < 0.05] = 0.0
  tables = {}
  for vdtype, dim in CLASSES:
    dt = getattr(torch, vdtype)
    t = de.CuckooHashTable(torch.int64, dt, torch.full((dim,), 0.375, dtype=dt), name="mx_%s_%d" % (vdtype, dim), dim=dim)
    rows = torch.randn((40, dim), generator=torch.Generator(device="cuda").manual_seed(dim), device="cuda").to(dt)
    t.insert(T(torch, np.arange(0, 80, 2, dtype=np.int64)), rows)
    x = np.full((80, dim), 0.375)
    x[0::2] = rows.to(torch.float32).cpu().numpy()
    g = torch.randn((N, dim), generator=torch.Generator(device="cuda").manual_seed(dim + 1), device="cuda")
    tables[(vdtype, dim)] = (t, x, g)
  return torch, de, rs, seg, ids, w, wp, tables


def reference(x, G, seg, ids, w, member, combiner, fill):
  """float64 (out, its bound, dw, its bound) over the member entries; a row without members is x[fill] (zeros for None)."""
  dim = x.shape[1]
  w = w.astype(np.float64) * member
  E, L = x[ids], np.bincount(seg, weights=member, minlength=N)
  acc, mag = np.zeros((N, dim)), np.zeros((N, dim))
  np.add.at(acc, seg, E * w[:, None])
  np.add.at(mag, seg, np.abs(E * w[:, None]))
  ws = np.bincount(seg, weights=w * w if combiner == "sqrtn" else w, minlength=N)
  den = np.ones(N) if combiner == "sum" else (np.sqrt(ws) if combiner == "sqrtn" else ws)
  ok = den != 0
  safe = np.where(ok, den, 1)
  out, bound = np.where(ok[:, None], acc / safe[:, None], 0), (L + 2)[:, None] * U24 * mag / np.abs(safe)[:, None]
  if fill is not None:
    out[L == 0] = x[fill]
  d, D = (E * G[seg]).sum(1), np.abs(E * G[seg]).sum(1)
  s, S = np.bincount(seg, weights=w * d, minlength=N)[seg], np.bincount(seg, weights=np.abs(w) * D, minlength=N)[seg]
  W, okp = safe[seg], ok[seg] & (member > 0)
  if combiner == "sum":
    dw, M = d, D
  elif combiner == "mean":
    dw, M = (d - s / W) / W, (D + S / np.abs(W)) / np.abs(W)
  else:
    dw, M = (d - (s / ws[seg].clip(1e-300)) * w) / W, (D + (S / ws[seg].clip(1e-300)) * np.abs(w)) / W
  return out, bound, np.where(okp, dw, 0), (L[seg] + dim + 4) * U24 * np.where(okp, M, 0)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean", "sqrtn"])
@pytest.mark.parametrize("vdtype,dim", CLASSES)
def test_mixed_forms_equal_their_twins_and_the_float64_reference(env, vdtype, dim, combiner, weighted, form):
  """The twin and the reference once per case, every long_from against them."""
  torch, de, rs, seg, ids, w, wp, tables = env
  t, x, g = tables[(vdtype, dim)]
  safe, fill, c, tab = form.startswith("safe"), FORMS[form], COMB[combiner], t._table
  wn = (wp if safe else w) if weighted else None
  ids_t, seg_t, rs_t, w_t = T(torch, ids), T(torch, seg), T(torch, rs), (None if wn is None else T(torch, wn))
  kw = dict(prune=safe, fill_id=fill)
  if form == "tuple":
    twin, dw_twin = tab.find_combine(ids_t, seg_t, w_t, c, N), tab.find_combine_weight_grad(ids_t, seg_t, w_t, c, g)
  else:
    twin, dw_twin = tab.find_combine_ragged(rs_t, ids_t, w_t, c, **kw), tab.find_combine_ragged_weight_grad(rs_t, ids_t, w_t, c, g, **kw)
  wv = np.ones(ids.size, np.float32) if wn is None else wn
  member = (wv > 0).astype(np.float64) if (safe and weighted) else np.ones(ids.size)
  out, bound, dwr, dbound = reference(x, g.cpu().numpy().astype(np.float64), seg, ids, wv, member, combiner, fill)
  for long_from in LONG_FROM:
    if form == "tuple":
      got = t.find_combine_mixed(ids_t, seg_t, w_t, c, N, long_from=long_from)
      dw = t.find_combine_weight_grad_mixed(ids_t, seg_t, w_t, c, g, long_from=long_from)
    else:
      got = t.find_combine_ragged_mixed(rs_t, ids_t, w_t, c, long_from=long_from, **kw)
      dw = t.find_combine_ragged_weight_grad_mixed(rs_t, ids_t, w_t, c, g, long_from=long_from, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, dim) and tuple(dw.shape) == (ids.size,)
    assert torch.equal(bits(torch, got), bits(torch, twin)), long_from
    assert torch.equal(bits(torch, dw), bits(torch, dw_twin)), long_from
    assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - out) <= bound), long_from
    assert np.all(np.abs(dw.cpu().numpy().astype(np.float64) - dwr) <= dbound), long_from
  tab.check_errors()


@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_a_row_longer_than_the_gradients_lds_park_beside_short_rows(env, combiner):
  """A row of 2100 entries (the gradient parks 2048 in LDS, the rest in dw_out) between short rows of the same block, half of
  the weights pruned."""
  torch, de, rs, seg, ids, w, wp, tables = env
  t, _, g = tables[("float32", 64)]
  rng = np.random.default_rng(5)
  lens = [3, 2100, 0, 17, 70]
  nnz = sum(lens)
  ids_t, rs_t = T(torch, rng.integers(0, 80, size=nnz).astype(np.int64)), T(torch, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
  w_t = T(torch, np.where(rng.random(nnz) < 0.5, 0.0, rng.uniform(0.25, 2.0, size=nnz)).astype(np.float32))
  for prune in (False, True):
    got = t.find_combine_ragged_weight_grad_mixed(rs_t, ids_t, w_t, COMB[combiner], g[:5], prune=prune)
    assert torch.equal(bits(torch, got), bits(torch, t._table.find_combine_ragged_weight_grad(rs_t, ids_t, w_t, COMB[combiner], g[:5],
                                                                                             prune=prune)))
    out = t.find_combine_ragged_mixed(rs_t, ids_t, w_t, COMB[combiner], prune=prune)
    assert torch.equal(bits(torch, out), bits(torch, t._table.find_combine_ragged(rs_t, ids_t, w_t, COMB[combiner], prune=prune)))
  t._table.check_errors()


def test_the_refusals_are_the_twins(env):
  torch, de = env[:2]
  from tfra_amd import _capi
  t = de.CuckooHashTable(torch.int64, torch.float32, torch.zeros(6), name="mx_dim6", dim=6)._table
  ids, seg, g = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, 6, device="cuda")
  for mixed, twin, args in (("find_combine_mixed", "find_combine", (ids, seg, None, 0, 1)),
                            ("find_combine_ragged_mixed", "find_combine_ragged", (seg, ids, None, 0)),
                            ("find_combine_weight_grad_mixed", "find_combine_weight_grad", (ids, seg, None, 0, g)),
                            ("find_combine_ragged_weight_grad_mixed", "find_combine_ragged_weight_grad", (seg, ids, None, 7, g))):
    with pytest.raises(_capi.TfraError) as a:
      getattr(t, mixed)(*args)
    with pytest.raises(_capi.TfraError) as b:
      getattr(t, twin)(*args)
    assert a.value.code == b.value.code and str(a.value).split(": ", 2)[2] == str(b.value).split(": ", 2)[2]   # behind the call's name


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("safe", [False, True])
def test_the_public_path_takes_the_mixed_calls(env, monkeypatch, ragged, safe):
  torch, de, rs, seg, ids, w, wp = env[:7]
  mod = de.ragged_embedding_ops if ragged else de
  fn = mod.safe_embedding_lookup_sparse if safe else mod.embedding_lookup_sparse
  var = filled_var(torch, de, "mx_public_%d%d" % (ragged, safe), initializer=0.5)
  two = filled_var(torch, de, "mx_two_shards_%d%d" % (ragged, safe), initializer=0.5, devices=["cuda:0", "cuda:0"])
  sp, w_t = (T(torch, rs if ragged else seg), T(torch, ids * 37)), T(torch, wp if safe else w)
  g = torch.randn((N, 64), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
  rows = {} if ragged else {"num_rows": N}
  run = lambda v, **kw: fn(v, sp, w_t, combiner="mean", return_trainable=True, **rows, **kw)
  exp, tw0 = run(var)
  dw0 = tw0.weights_grad(g)
  calls = Calls(monkeypatch)
  got, tw = run(var, mixed_rows=True)
  dw = tw.weights_grad(g)
  forward = "tfra_table_find_combine_ragged" if ragged else "tfra_table_find_combine"
  assert calls[forward + "_mixed"] == 1 and calls["tfra_table_find_combine_backprop_weights_mixed"] == 1
  assert calls[forward] == 0 and calls["tfra_table_find_combine_backprop_weights"] == 0
  assert torch.equal(bits(torch, got), bits(torch, exp)) and torch.equal(bits(torch, dw), bits(torch, dw0))
  calls.n.clear()
  out_a, tw_a = run(two, mixed_rows=True)
  dw_a = tw_a.weights_grad(g)
  with_keyword = dict(calls.n)
  calls.n.clear()
  out_b, tw_b = run(two)
  dw_b = tw_b.weights_grad(g)
  assert with_keyword == calls.n and not any(name.endswith("_mixed") for name in with_keyword)
  assert torch.equal(bits(torch, out_a), bits(torch, out_b)) and torch.equal(bits(torch, dw_a), bits(torch, dw_b))
  with pytest.raises(ValueError, match="exclude each other"):
    run(var, mixed_rows=True, long_rows=True)
