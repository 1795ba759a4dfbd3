"""GPU: the table under several streams / host threads / rehashes — the threading contract of the drop-in
boundary (any TF inter-op thread may call concurrently on the same table; entry points
are stream-ordered and re-entrant; the library serialises host state and chains streams itself)."""
import threading

import numpy as np
import pytest

import oracle
from tests.test_gpu_int32_surface import SLEEP_CYCLES

pytestmark = pytest.mark.gpu
DIM = 8


@pytest.fixture(scope="module")
def env():
  import torch
  import tfra_amd.dynamic_embedding as de
  return torch, de


def _table(de, torch, name, **kw):
  return de.CuckooHashTable(torch.int64, torch.float32, default_value=torch.full((DIM,), -1.0), name=name, device="cuda:0",
                            dim=DIM, **kw)


def test_two_streams_are_chained_by_the_library(env):
  """insert on stream A, find on stream B, no caller-side synchronisation: the find sees the insert.  Every other round a long
  kernel holds stream A back in front of its call, so that a missing wait shows even when the kernels are short."""
  torch, de = env
  t = _table(de, torch, "conc_streams")
  sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
  n = 200000
  keys = torch.arange(n, device="cuda") * 7919
  vals = (keys.to(torch.float32) * 0.5)[:, None].repeat(1, DIM).contiguous()
  torch.cuda.synchronize()
  for rep in range(5):
    with torch.cuda.stream(sa):
      if rep % 2:
        torch.cuda._sleep(SLEEP_CYCLES)
      t.insert(keys, vals + rep)
    with torch.cuda.stream(sb):
      got, ex = t.lookup(keys, return_exists=True)
    with torch.cuda.stream(sa):
      if rep % 2:
        torch.cuda._sleep(SLEEP_CYCLES)
      t.remove(keys[: n // 2])
    with torch.cuda.stream(sb):
      got2, ex2 = t.lookup(keys, return_exists=True)
      t.insert(keys[: n // 2], vals[: n // 2] + rep)      # restore for the next round
    torch.cuda.synchronize()
    assert bool(ex.all()) and torch.equal(got, vals + rep)
    assert not bool(ex2[: n // 2].any()) and bool(ex2[n // 2:].all())
    assert torch.equal(got2[n // 2:], (vals + rep)[n // 2:])
    assert bool((got2[: n // 2] == -1.0).all())


def test_host_threads_share_one_table(env):
  """8 host threads, each with its own stream, upsert disjoint ranges and read them back while the table
  grows from its minimum size; the union is intact afterwards (export == what the oracle holds)."""
  torch, de = env
  t = _table(de, torch, "conc_threads", init_size=64)
  ora = oracle.CpuTable(DIM)
  per, rounds, nthreads = 20000, 6, 8
  errors = []

  def worker(w):
    try:
      torch.cuda.set_device(0)
      s = torch.cuda.Stream()
      rng = np.random.default_rng(w)
      with torch.cuda.stream(s):
        for r in range(rounds):
          k = (np.arange(per, dtype=np.int64) + (w * rounds + r) * per) * 104729 - 10**9
          v = rng.standard_normal((per, DIM)).astype(np.float32)
          kt, vt = torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda()
          t.insert(kt, vt)
          got, ex = t.lookup(kt, return_exists=True)
          s.synchronize()
          if not bool(ex.all()) or not torch.equal(got, vt):
            errors.append("thread %d round %d: read-back mismatch" % (w, r))
          results[w].append((k, v))
    except Exception as e:  # noqa: BLE001
      errors.append("thread %d: %r" % (w, e))

  results = [[] for _ in range(nthreads)]
  threads = [threading.Thread(target=worker, args=(w,)) for w in range(nthreads)]
  for th in threads:
    th.start()
  for th in threads:
    th.join()
  assert not errors, errors[:3]
  for rs in results:
    for k, v in rs:
      ora.insert(k, v)
  assert int(t.size()) == nthreads * rounds * per
  k, v = t.export()
  o = np.argsort(k.cpu().numpy())
  ek, ev = ora.export_sorted()
  np.testing.assert_array_equal(k.cpu().numpy()[o], ek)
  np.testing.assert_array_equal(v.cpu().numpy()[o], ev)


def test_growth_interleaved_with_finds_erases_and_accum(env):
  """Grow from 16 slots to > 1M keys in uneven batches with erases, accums and finds in between: every
  rehash keeps every key and value (vs the CPU oracle), size stays exact."""
  torch, de = env
  t = _table(de, torch, "conc_growth", init_size=16)
  ora = oracle.CpuTable(DIM)
  rng = np.random.default_rng(3)
  nxt = 0
  for step, n in enumerate([1, 7, 100, 1000, 5000, 30000, 1, 200000, 3, 500000, 64, 400000]):
    k = (np.arange(nxt, nxt + n, dtype=np.int64) * 2654435761) ^ 0x5555
    nxt += n
    v = rng.integers(-100, 100, size=(n, DIM)).astype(np.float32)
    t.insert(torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda())
    ora.insert(k, v)
    if step % 3 == 1:      # erase a slice of what exists
      ek, _ = ora.export_sorted()
      gone = ek[:: 5][: 20000]
      t.remove(torch.from_numpy(gone).cuda())
      ora.remove(gone)
    if step % 4 == 2:      # accum on a mix of present / absent keys with matching and mismatching flags
      ek, _ = ora.export_sorted()
      pres = ek[:: 7][: 5000]
      absent = np.arange(10**15 + step * 10000, 10**15 + step * 10000 + 3000, dtype=np.int64)
      ak = np.concatenate([pres, absent])
      ex = np.concatenate([np.ones(pres.size, bool), np.zeros(absent.size, bool)])
      flip = rng.random(ak.size) < 0.2
      ex = ex ^ flip
      d = rng.integers(-5, 5, size=(ak.size, DIM)).astype(np.float32)
      t.accum(torch.from_numpy(ak).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(ex).cuda())
      ora.accum(ak, d, ex)
    assert int(t.size()) == ora.size()
    probe = (np.arange(max(nxt - 3000, 0), nxt + 50, dtype=np.int64) * 2654435761) ^ 0x5555
    got, gex = t.lookup(torch.from_numpy(probe).cuda(), return_exists=True)
    want, wex = ora.find(probe, np.full(DIM, -1.0, np.float32), return_exists=True)
    np.testing.assert_array_equal(gex.cpu().numpy(), wex)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
  k, v = t.export()
  o = np.argsort(k.cpu().numpy())
  ek, ev = ora.export_sorted()
  np.testing.assert_array_equal(k.cpu().numpy()[o], ek)
  np.testing.assert_array_equal(v.cpu().numpy()[o], ev)
