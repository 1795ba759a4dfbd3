"""CPU: the three spellings of the fused Momentum / Nesterov / RMSProp kinds agree — the C header's enum, _capi's constants and the
Python optimizer classes — and tfra_opt_params keeps the layout it had before them."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_kinds():
  text = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  body = re.search(r"typedef enum\s*\{([^}]*)\}\s*tfra_opt_kind;", text).group(1)
  return {n: int(v) for n, v in re.findall(r"\bTFRA_OPT_(\w+)\s*=\s*(\d+)", body)}


def test_kinds_in_the_header_and_in_capi():
  from tfra_amd import _capi
  kinds = header_kinds()
  assert kinds == {"SGD": 0, "ADAM": 1, "ADAGRAD": 2, "FTRL": 3, "MOMENTUM": 4, "NESTEROV": 5, "RMSPROP": 6}
  assert (_capi.OPT_MOMENTUM, _capi.OPT_NESTEROV, _capi.OPT_RMSPROP) == (4, 5, 6)
  assert (_capi.OPT_SGD, _capi.OPT_ADAM, _capi.OPT_ADAGRAD, _capi.OPT_FTRL) == (0, 1, 2, 3)


def test_opt_params_keeps_its_layout():
  """tfra_opt_params has no size field, so it must not grow: the size and the offsets of the struct before the three kinds (an
  int32, seven floats, one pointer), and the header's members in _capi's order."""
  from tfra_amd import _capi
  P = _capi.OptParams
  assert ctypes.sizeof(P) == 40
  want = {"kind": 0, "lr": 4, "beta1": 8, "beta2": 12, "eps": 16, "l1": 20, "l2": 24, "lr_power": 28, "d_lr": 32}
  assert {n: getattr(P, n).offset for n, _ in P._fields_} == want
  assert [n for n, _ in P._fields_] == list(want)
  text = open(os.path.join(ROOT, "include", "tfra_mi355x.h")).read()
  body = re.search(r"typedef struct(?:\s+\w+)?\s*\{([^}]*)\}\s*tfra_opt_params;", text).group(1)
  body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
  names = [n for decl in body.split(";") for n in re.findall(r"\w+", decl) if n not in ("int32_t", "float", "const")]
  assert names == list(want)
  assert re.search(r"#define\s+TFRA_ABI_VERSION\s+1\b", text) or "TFRA_ABI_VERSION = 1" in text


def test_default_forms_stay_generic():
  import tfra_amd.dynamic_embedding as de
  for opt in (de.optimizers.Momentum(), de.optimizers.Momentum(use_nesterov=True), de.optimizers.RMSProp()):
    assert isinstance(opt, de.optimizers.Generic)
    assert opt.kind is None and opt.params(1) is None
  assert de.optimizers.Momentum(0.05, 0.9, fused=False).kind is None and de.optimizers.RMSProp(fused=False).params(3) is None


def test_fused_forms_fill_the_params():
  from tfra_amd import _capi
  import tfra_amd.dynamic_embedding as de
  f32 = np.float32
  m = de.optimizers.Momentum(0.05, 0.9, fused=True)
  p = m.params(1)
  assert isinstance(p, _capi.OptParams) and m.kind == p.kind == 4
  assert f32(p.lr) == f32(0.05) and f32(p.beta1) == f32(0.9) and not p.d_lr
  n = de.optimizers.Momentum(0.05, 0.9, use_nesterov=True, fused=True)
  p = n.params(1)
  assert n.kind == p.kind == 5 and f32(p.lr) == f32(0.05) and f32(p.beta1) == f32(0.9)
  r = de.optimizers.RMSProp(0.01, 0.9, 0.5, 1e-10, fused=True)
  p = r.params(1)
  assert r.kind == p.kind == 6
  assert f32(p.lr) == f32(0.01) and f32(p.beta1) == f32(0.5) and f32(p.eps) == f32(1e-10)
  # beta2 carries 1 - rho, subtracted in double and rounded once — the oracle's f32(1.0 - rho) — which is NOT the float32 difference
  assert f32(p.beta2) == f32(1.0 - 0.9)
  assert f32(1.0 - 0.9) != f32(1) - f32(0.9)
  assert f32(p.beta2) != f32(1) - f32(0.9)


def test_both_forms_make_the_same_variable():
  import tfra_amd.dynamic_embedding as de
  kw = de.DynamicEmbeddingOptimizer.variable_kwargs
  O = de.optimizers
  assert kw(O.Momentum(0.05, 0.9)) == kw(O.Momentum(0.05, 0.9, fused=True)) == {"aux_fields": 1, "aux_init": (0.0, 0.0, 0.0, 0.0)}
  assert kw(O.Momentum(0.05, 0.9, use_nesterov=True)) == kw(O.Momentum(0.05, 0.9, use_nesterov=True, fused=True))
  assert kw(O.RMSProp(0.01, 0.9, 0.5, 1e-10, 0.1)) == kw(O.RMSProp(0.01, 0.9, 0.5, 1e-10, 0.1, fused=True)) == \
      {"aux_fields": 2, "aux_init": (0.1, 0.0, 0.0, 0.0)}
  for a, b in ((O.Momentum(), O.Momentum(fused=True)), (O.RMSProp(), O.RMSProp(fused=True))):
    assert a.slots == b.slots and a.aux_init() == b.aux_init()
