"""CPU: the ABI of the wide write-backs (256 < dim <= 1024): the header's declarations, the bindings' argument lists, the optimizer's
keyword and which variables can_plan_wide sends down them."""
import inspect
import os
import re
import types

import pytest
import torch

from tfra_amd import _capi
from tfra_amd.dynamic_embedding.optimizer import DynamicEmbeddingOptimizer

TWINS = {"tfra_sparse_plan_build_wide": "tfra_sparse_plan_build", "tfra_table_apply_planned_wide": "tfra_table_apply_planned",
         "tfra_table_apply_planned_combined_wide": "tfra_table_apply_planned_combined",
         "tfra_table_apply_sparse_wide": "tfra_table_apply_sparse"}
HEADER = open(os.path.join(os.path.dirname(__file__), "..", "include", "tfra_mi355x.h")).read()


@pytest.mark.parametrize("name", sorted(TWINS))
def test_declared_with_the_twins_argument_list(name):
  decl = lambda n: re.sub(r"\s+", " ", re.search(r"\nint %s\(([^;]*)\);" % n, HEADER).group(1))
  assert decl(name) == decl(TWINS[name])
  assert _capi._SIGS_WIDE[name] == _capi._SIGS[TWINS[name]]


def test_wide_rows_is_the_last_keyword_and_off():
  params = inspect.signature(DynamicEmbeddingOptimizer.__init__).parameters
  assert list(params)[-1] == "wide_rows" and params["wide_rows"].default is False


def stub(dim, value_dtype=torch.float32, shard_num=1, initializer=0.5, **kw):
  return types.SimpleNamespace(value_dtype=value_dtype, dim=dim, shard_num=shard_num, initializer=initializer, **kw)


@pytest.mark.parametrize("var,want", [(stub(260), True), (stub(1024, torch.bfloat16), True), (stub(256), False), (stub(1028), False),
                                      (stub(258), False), (stub(512, shard_num=2), False),
                                      (stub(512, initializer=lambda n: None), False), (stub(512, stochastic_rounding=7), False)])
def test_can_plan_wide(var, want):
  assert DynamicEmbeddingOptimizer.can_plan_wide(var, 4096) is want
  assert DynamicEmbeddingOptimizer.can_plan_wide(var, (1 << 18) + 1) is False
