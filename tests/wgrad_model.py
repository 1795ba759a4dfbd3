"""The float64 reference of the gradient of the pooled lookup's weights, shared by tests/test_weight_grad_abi.py (which checks it
against torch.autograd on the CPU) and tests/test_gpu_weight_grad.py (a plain module: no fixtures, no tests)."""
import numpy as np


def wgrad_model(E, G, bounds, w, combiner, prune=False):
  """(dw, T, cnt), float64 [nnz]: the gradient of out = A / den (A = sum w x over the row's members; den = 1 | W = sum w |
  sqrt(S), S = sum w^2) with respect to the weights, for the rows bounds[r] = (b, e) of the entry list:
     sum d_p | mean (d_p - s / W) / W | sqrtn (d_p - (s / S) w_p) / sqrt(S),   d_p = G[r] . E[p],  s = sum_p w_p d_p.
  An entry in no row, a pruned entry (prune: weight not > 0) and every entry of a mean / sqrtn row with W / S == 0 get 0.
  T[p]: the sum of the absolute values of all terms of dw[p] (the scale of its forward error bound); cnt[p]: the members of its row."""
  E, G = np.asarray(E, np.float64), np.asarray(G, np.float64)
  nnz = E.shape[0]
  w = np.ones(nnz) if w is None else np.asarray(w, np.float64)
  dw, T, cnt = np.zeros(nnz), np.zeros(nnz), np.zeros(nnz)
  for r, (b, e) in enumerate(bounds):
    if b >= e:
      continue
    mem = np.arange(b, e)
    if prune:
      mem = mem[w[b:e] > 0]
    if mem.size == 0:
      continue
    x, ww = E[mem], w[mem]
    d, da = x @ G[r], np.abs(x) @ np.abs(G[r])
    cnt[mem] = mem.size
    if combiner == "sum":
      dw[mem], T[mem] = d, da
      continue
    s, sa = float(np.sum(ww * d)), float(np.sum(np.abs(ww) * da))
    if combiner == "mean":
      W = float(np.sum(ww))
      if W == 0:
        continue
      dw[mem] = (d - s / W) / W
      T[mem] = da / abs(W) + sa / (W * W)
    else:
      S = float(np.sum(ww * ww))
      if S == 0:
        continue
      dw[mem] = (d - (s / S) * ww) / np.sqrt(S)
      T[mem] = da / np.sqrt(S) + np.abs(ww) * sa / (S * np.sqrt(S))
  return dw, T, cnt


def bounds_of(seg, n_rows):
  """[(b, e)] per row of an ascending seg (entries outside [0, n_rows) are in no row)."""
  seg = np.asarray(seg)
  return [(int(np.searchsorted(seg, r, "left")), int(np.searchsorted(seg, r, "right"))) for r in range(n_rows)]


def chain_autograd(E, G, seg, w, combiner, n_rows):
  """d sum(out * G) / d w in float64 by torch.autograd through the reference's chain (PY/dynamic_embedding_ops.py:233-291):
  gather * w -> segment_sum (index_add) -> divide by sum w (mean) or sqrt(sum w^2) (sqrtn); an empty row is zeros."""
  import torch
  wt = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
  st = torch.tensor(np.asarray(seg, np.int64))
  A = torch.zeros((n_rows, E.shape[1]), dtype=torch.float64).index_add(0, st, torch.tensor(np.asarray(E, np.float64)) * wt[:, None])
  if combiner == "mean":
    den = torch.zeros(n_rows, dtype=torch.float64).index_add(0, st, wt)
  elif combiner == "sqrtn":
    den = torch.zeros(n_rows, dtype=torch.float64).index_add(0, st, wt * wt).sqrt()
  else:
    den = torch.ones(n_rows, dtype=torch.float64)
  has = torch.zeros(n_rows, dtype=torch.bool)
  has[st] = True
  out = torch.where(has[:, None], A / torch.where(has, den, torch.ones_like(den))[:, None], torch.zeros_like(A))
  (out * torch.tensor(np.asarray(G, np.float64))).sum().backward()
  return wt.grad.numpy()
