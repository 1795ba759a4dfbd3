"""CPU: the stochastic-rounding option's three spellings agree — the C header's enum, _capi's constant and the Python signatures."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_enum(name):
  text = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  body = re.search(r"typedef enum\s*\{([^}]*)\}\s*tfra_option;", text).group(1)   # (the comments around it speak of values too)
  m = re.search(r"\b%s\s*=\s*(\d+)" % name, body)
  assert m, "%s is not in the header" % name
  return int(m.group(1))


def test_option_value_in_the_header_and_in_capi():
  from tfra_amd import _capi
  assert header_enum("TFRA_OPTION_STOCHASTIC_ROUNDING") == 4 == _capi.OPTION_STOCHASTIC_ROUNDING
  # the options are distinct, and the earlier ones keep their values
  values = {n: header_enum("TFRA_OPTION_" + n) for n in ("CAPTURE_SAFE", "NO_OWNER_TAGS", "KEY_BYTES_ON_DISK", "STOCHASTIC_ROUNDING")}
  assert values == {"CAPTURE_SAFE": 1, "NO_OWNER_TAGS": 2, "KEY_BYTES_ON_DISK": 3, "STOCHASTIC_ROUNDING": 4}
  assert (_capi.OPTION_CAPTURE_SAFE, _capi.OPTION_NO_OWNER_TAGS, _capi.OPTION_KEY_BYTES_ON_DISK) == (1, 2, 3)
  import ctypes
  assert _capi._SIGS["tfra_table_set_option"][2] is ctypes.c_int64   # the seed: all 64 bits


def test_opt_params_keeps_its_layout():
  """The option adds no field to tfra_opt_params: the header's struct and _capi.OptParams list the same members."""
  from tfra_amd import _capi
  text = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  body = re.search(r"typedef struct(?:\s+\w+)?\s*\{([^}]*)\}\s*tfra_opt_params;", text).group(1)
  body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
  names = [n for decl in body.split(";") for n in re.findall(r"\w+", decl) if n not in ("int32_t", "float", "const")]
  assert names == [f[0] for f in _capi.OptParams._fields_]
  assert "seed" not in names and "stochastic" not in " ".join(names)


def test_python_signatures():
  import tfra_amd.dynamic_embedding as de
  from tfra_amd.dynamic_embedding import table_ops
  for cls in (table_ops._DeviceTable, de.HkvHashTable, de.CuckooHashTable, table_ops.TieredHashTable, de.Variable):
    assert list(inspect.signature(cls.set_stochastic_rounding).parameters) == ["self", "seed"], cls
  p = inspect.signature(de.Variable.__init__).parameters
  assert p["stochastic_rounding"].default is None and list(p)[-1] == "stochastic_rounding"
