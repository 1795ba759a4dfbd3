"""The reference engine (oracle kind "reference": the reference's cuckoo table, built into oracle/_ref where the reference tree
exists) as recorded answers, so that its test cases run where it cannot be built.

Where oracle/_ref exists, a case talks to the engine itself.  Where it does not, the engine's C functions are replaced by a
stand-in that checks every call against the call the real engine received when the case was recorded (same function, same
arguments, same input bytes) and answers it with the bytes the real engine wrote then.  `CpuTable` itself (shape checks,
defaults, export order) runs unchanged either way.  Recording, where oracle/_ref exists:

    TFRA_RECORD_REFERENCE=1 python -m pytest tests/test_oracle.py -m "not gpu"

writes tests/golden/ref_engine/<case>.npz for every case that called the engine."""
import contextlib
import ctypes
import hashlib
import lzma
import os
import re

import numpy as np

import oracle

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_engine")
_ITEM = {oracle.DT_F32: 4, oracle.DT_F16: 2, oracle.DT_BF16: 2, oracle.DT_I8: 1, oracle.DT_I32: 4, oracle.DT_I64: 8, oracle.DT_F64: 8}


def _addr(p):
  return p.value if isinstance(p, ctypes.c_void_p) else p


def _read(p, size):
  a = _addr(p)
  return ctypes.string_at(a, size) if a and size else b""


def _write(p, data):
  if data:
    ctypes.memmove(_addr(p), data, len(data))


class _Calls:
  """What one engine call reads and writes, from its arguments and the (dim, item size) of its table: (description of the
  arguments and input bytes, [(bytes, row size) of the row-shaped inputs], [(pointer, size, row size or 0) of every output])."""

  def __init__(self):
    self.tables = {}   # handle -> (ordinal, dim, item)

  def describe(self, name, a, ret=None):
    if name == "create":
      return repr(a), [], []
    o, dim, item = self.tables[_addr(a[0])]
    rs = dim * item
    if name == "find":        # (h, n, keys, out, defaults, full, exists, threads)
      n, full = a[1], a[5]
      d = _read(a[4], (n if full else 1) * rs)
      return (repr((o, n, full, _addr(a[6]) is None)) + _read(a[2], 8 * n).hex() + d.hex(), [(d, rs)],
              [(a[3], n * rs, rs), (a[6], n if _addr(a[6]) else 0, 0)])
    if name in ("insert", "accum"):   # (h, n, keys, values, clear / exists, threads)
      n = a[1]
      v = _read(a[3], n * rs)
      tail = repr(a[4]) if name == "insert" else _read(a[4], n).hex()
      return repr((o, n)) + tail + _read(a[2], 8 * n).hex() + v.hex(), [(v, rs)], []
    if name == "remove":      # (h, n, keys)
      return repr((o, a[1])) + _read(a[2], 8 * a[1]).hex(), [], []
    if name in ("clear", "size"):
      return repr((o,)), [], []
    if name == "dump":        # (h, keys, values, offset, length) -> rows written
      return repr((o, a[3], a[4])), [], [(a[1], 8 * ret, 0), (a[2], ret * rs, rs)]
    raise ValueError(name)


class _Rows:
  """The rows a case has given the engine or received from it so far, numbered in order of first appearance.  An output row equal
  to one of them (a stored value a find returns, a default it falls back to) is kept as its number, any other row as its bytes;
  the recorder and the stand-in see the same inputs in the same order, so both number the rows alike."""

  def __init__(self):
    self.num, self.rows = {}, []

  def _new(self, r):
    self.num[r] = len(self.rows)
    self.rows.append(r)

  def add(self, data, rs):
    for j in range(0, len(data), rs):
      if data[j:j + rs] not in self.num:
        self._new(data[j:j + rs])

  def encode(self, data, rs, refs, lits):
    for j in range(0, len(data), rs):
      r = data[j:j + rs]
      k = self.num.get(r)
      refs.append(-1 if k is None else k)
      if k is None:
        lits.append(r)
        self._new(r)

  def decode(self, n, rs, refs, lits):
    out = []
    for _ in range(n):
      k = next(refs)
      r = self.rows[k] if k >= 0 else lits.take(rs)
      if k < 0:
        self._new(r)
      out.append(r)
    return b"".join(out)


class _Reader:
  def __init__(self, data):
    self.data, self.at = data, 0

  def take(self, size):
    self.at += size
    return self.data[self.at - size:self.at]


def _digest(desc):
  return np.frombuffer(hashlib.sha256(desc.encode()).digest()[:16], np.uint8)


NAMES = ("create", "find", "insert", "accum", "remove", "clear", "size", "dump")


def _recorder(live, log, refs, lits):
  calls, rows = _Calls(), _Rows()

  def wrap(name):
    def f(*a):
      ret = live[name](*a)
      if name == "create" and ret:
        calls.tables[_addr(ret)] = (len(calls.tables), a[1], _ITEM[a[0]])
      desc, ins, outs = calls.describe(name, a, ret)
      for data, rs in ins:
        rows.add(data, rs)
      for ptr, size, rs in outs:
        if rs:
          rows.encode(_read(ptr, size), rs, refs, lits)
        else:
          lits.append(_read(ptr, size))
      # (create: the table's ordinal + 1 is recorded, 0 for a dtype the engine refuses — the stand-in's handle)
      log.append((name, _digest(desc), (calls.tables[_addr(ret)][0] + 1 if ret else 0) if name == "create" else ret))
      return ret
    return f
  fns = {name: wrap(name) for name in NAMES}
  fns["destroy"] = live["destroy"]
  return fns


def _replayer(case, z):
  calls, rows = _Calls(), _Rows()
  state = {"i": 0, "n": int(z["n_calls"])}
  lits = _Reader(lzma.decompress(z["outputs"].tobytes()) if state["n"] else b"")
  refs = iter(z["refs"].tolist() if state["n"] else [])
  state["lits"], state["refs"] = lits, refs

  def wrap(name):
    def f(*a):
      i = state["i"]
      assert i < state["n"], "%s: reference engine call %d (%s) was not recorded" % (case, i, name)
      assert NAMES[z["names"][i]] == name, "%s: reference engine call %d is %s, recorded %s" % (case, i, name, NAMES[z["names"][i]])
      ret = None if z["rets"][i] < 0 else int(z["rets"][i])
      if name == "create" and ret:
        calls.tables[ret] = (ret - 1, a[1], _ITEM[a[0]])
      desc, ins, outs = calls.describe(name, a, ret)
      assert np.array_equal(_digest(desc), z["ins"][i]), "%s: reference engine call %d (%s): arguments differ from the recorded call" % (case, i, name)
      for data, rs in ins:
        rows.add(data, rs)
      for ptr, size, rs in outs:
        _write(ptr, rows.decode(size // rs, rs, refs, lits) if rs else lits.take(size))
      state["i"] = i + 1
      return ret
    return f
  fns = {name: wrap(name) for name in NAMES}
  fns["destroy"] = lambda h: None
  return fns, state


def _path(case):
  return os.path.join(DIR, re.sub(r"[^A-Za-z0-9_.-]+", "_", case) + ".npz")


@contextlib.contextmanager
def installed(case):
  """kind="reference" inside the block: the engine itself, recorded for `case` under TFRA_RECORD_REFERENCE=1; where it is not built,
  the recording of `case`, every call of which the block must make."""
  record = bool(os.environ.get("TFRA_RECORD_REFERENCE"))
  if not record and oracle.available("reference"):
    yield
    return
  saved = oracle._LIBS.pop("reference", None)
  if record:
    log, refs, lits = [], [], []
    oracle._LIBS["reference"] = _recorder(oracle._load("reference"), log, refs, lits)
  else:
    z = np.load(_path(case)) if os.path.exists(_path(case)) else {"n_calls": np.int64(0)}
    oracle._LIBS["reference"], state = _replayer(case, z)
  try:
    yield
  finally:
    oracle._LIBS.pop("reference", None)
    if saved is not None:
      oracle._LIBS["reference"] = saved
  if record:
    if log:
      out = {"n_calls": np.int64(len(log)), "refs": np.array(refs, dtype=np.int32),
             "outputs": np.frombuffer(lzma.compress(b"".join(lits), preset=9 | lzma.PRESET_EXTREME), np.uint8),
             "names": np.array([NAMES.index(name) for name, _, _ in log], dtype=np.int8),
             "ins": np.stack([dig for _, dig, _ in log]),
             "rets": np.array([-1 if ret is None else ret for _, _, ret in log], dtype=np.int64)}   # (-1: the call returns nothing)
      os.makedirs(DIR, exist_ok=True)
      np.savez_compressed(_path(case), **out)
  else:
    assert state["i"] == state["n"], "%s: %d of the %d recorded reference engine calls were made" % (case, state["i"], state["n"])
    lits, refs = state["lits"], state["refs"]
    assert lits.at == len(lits.data) and next(refs, None) is None, "%s: recorded outputs left unread" % case
