"""A field-aware row model of the table, in plain numpy: what every entry point of a table created with `aux_fields = S`
must leave in the `1 + S` vectors of a key (include/tfra_mi355x.h; make_aux_init, csrc/tfra_table.hip; init_aux_fields, csrc/tfra_upsert_device.h).

State: key -> array [1 + S, dim] of the table's STORAGE dtype.  bfloat16 has no numpy type: its rows are held as their
uint16 bit patterns, every other dtype as itself.  All comparisons against the device are made on the rows' bytes.

Rules:
  insert_or_assign       existing key: field 0 replaced, nothing else touched.  New key: field 0 = the value, aux field f =
                         aux_init[f - 1] converted to the value dtype.  Repeated keys of a call: the last occurrence wins.
  insert_field(f)        existing key: field f replaced only.  New key: field f = the value, field 0 = zeros, the other aux
                         fields = aux_init.
  accum_or_assign        on field 0 (tests/test_gpu_accum_own.py): absent & !exists -> insert (aux like insert_or_assign),
                         present & exists -> row += delta with ONE add per element (half / bfloat16: the float32 sum rounded
                         once to nearest even; integers wrap), absent & exists and present & !exists -> nothing.  In index order.
  find_field(f)          hit: the stored field; miss: the default (one row [dim], or per position [n, dim]).
  erase, clear

aux_init conversion (make_aux_init): float32 as is; float16 / bfloat16 round to nearest even; int32 / int8 truncate toward
zero; int64 / float64 tables ignore aux_init: their aux fields start at 0."""
import numpy as np

STORAGE = {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16, "int8": np.int8, "int32": np.int32,
           "int64": np.int64, "float64": np.float64}


def f32_to_bf16_bits(x):
  """float32 array -> bfloat16 bit patterns (uint16), round to nearest even; a NaN keeps its sign and top payload bits and
  gets the quiet bit (f32_to_bf16, csrc/tfra_device.h)."""
  u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
  nan = (u & 0x7fffffff) > 0x7f800000
  r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
  return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_bits_to_f32(b):
  return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def aux_image(dtype_name, x):
  """aux_init value `x` (a float) as one element of the storage dtype."""
  st = STORAGE[dtype_name]
  x = np.float32(x)
  if dtype_name == "float32":
    return x
  if dtype_name == "float16":
    return np.float32(x).astype(np.float16)
  if dtype_name == "bfloat16":
    return f32_to_bf16_bits(np.array([x]))[0]
  if dtype_name in ("int32", "int8"):
    return st(int(np.trunc(x)))
  return st(0)      # int64 / float64


def from_float(dtype_name, x):
  """A float32 array as rows of the storage dtype (for test values): float types rounded to nearest even, integers truncated."""
  x = np.asarray(x, dtype=np.float32)
  if dtype_name == "bfloat16":
    return f32_to_bf16_bits(x).reshape(x.shape)
  if dtype_name in ("float16", "float32", "float64"):
    return x.astype(STORAGE[dtype_name])
  return np.trunc(x).astype(np.int64).astype(STORAGE[dtype_name])


def add_rows(dtype_name, a, b):
  """a + b, one add per element, in the table's arithmetic."""
  if dtype_name == "float16":
    return (a.astype(np.float32) + b.astype(np.float32)).astype(np.float16)
  if dtype_name == "bfloat16":
    return f32_to_bf16_bits(bf16_bits_to_f32(a) + bf16_bits_to_f32(b)).reshape(a.shape)
  with np.errstate(over="ignore"):
    return (a + b).astype(a.dtype)      # integers wrap; float32 / float64 are one IEEE add


def as_bytes(rows):
  """[..., dim] of a storage dtype -> [..., dim * element size] uint8."""
  rows = np.ascontiguousarray(rows)
  return rows.view(np.uint8).reshape(rows.shape[:-1] + (rows.shape[-1] * rows.dtype.itemsize,))


class FieldModel:
  def __init__(self, dtype_name, dim, aux_fields, aux_init=(0.0, 0.0, 0.0, 0.0)):
    self.dtype_name, self.dim, self.S = dtype_name, int(dim), int(aux_fields)
    self.st = STORAGE[dtype_name]
    self.aux = [aux_image(dtype_name, aux_init[f] if f < len(aux_init) else 0.0) for f in range(4)]
    self.rows = {}

  # ---- helpers ----
  def _check_field(self, f):
    if not 0 <= f <= self.S:
      raise ValueError("bad field %d" % f)

  def new_row(self):
    r = np.zeros((1 + self.S, self.dim), self.st)
    for f in range(1, 1 + self.S):
      r[f, :] = self.aux[f - 1]
    return r

  def _vals(self, keys, values):
    keys = np.asarray(keys, np.int64).reshape(-1)
    values = np.asarray(values)
    assert values.dtype == self.st and values.shape == (keys.size, self.dim), (values.dtype, values.shape)
    return keys, values

  def size(self):
    return len(self.rows)

  # ---- writers ----
  def insert_field(self, f, keys, values):
    self._check_field(f)
    keys, values = self._vals(keys, values)
    for i, k in enumerate(keys.tolist()):
      r = self.rows.get(k)
      if r is None:
        r = self.rows[k] = self.new_row()
        r[0, :] = 0
      r[f] = values[i]

  def insert_or_assign(self, keys, values):
    self.insert_field(0, keys, values)

  def accum_or_assign(self, keys, vod, exists):
    keys, vod = self._vals(keys, vod)
    exists = np.asarray(exists, bool).reshape(-1)
    for i, (k, e) in enumerate(zip(keys.tolist(), exists.tolist())):
      r = self.rows.get(k)
      if r is None and not e:
        r = self.rows[k] = self.new_row()
        r[0] = vod[i]
      elif r is not None and e:
        r[0] = add_rows(self.dtype_name, r[0], vod[i])

  def erase(self, keys):
    for k in np.asarray(keys, np.int64).reshape(-1).tolist():
      self.rows.pop(k, None)

  def clear(self):
    self.rows.clear()

  # ---- readers ----
  def find_field(self, f, keys, default):
    """-> (rows [n, dim], exists [n]).  default: [dim] (broadcast) or [n, dim] (per position)."""
    self._check_field(f)
    keys = np.asarray(keys, np.int64).reshape(-1)
    default = np.asarray(default)
    assert default.dtype == self.st
    out = np.empty((keys.size, self.dim), self.st)
    out[:] = default.reshape(-1, self.dim) if default.size != self.dim else default.reshape(1, self.dim)
    ex = np.zeros(keys.size, bool)
    for i, k in enumerate(keys.tolist()):
      r = self.rows.get(k)
      if r is not None:
        out[i] = r[f]
        ex[i] = True
    return out, ex

  def items_field(self, f):
    """key -> bytes of field f, for set comparisons with an export."""
    return {k: as_bytes(r[f]).tobytes() for k, r in self.rows.items()}
