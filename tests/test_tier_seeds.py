"""CPU-only: the precondition of the tier tests on the GPU (tests/test_gpu_tier_driver.py, tests/test_gpu_tier_variable.py).  No batch
of their seeds has a key with 15 or more batch keys homed at BOTH of its home buckets of an 89-bucket table (probe_model.homes), so
no batch saturates its own buckets and every key of a lookup can stay in the upper table.  The GPU tests assert the same per batch
against the table's real bucket count; here the seeds are checked where no GPU is needed."""
import numpy as np

from tests import probe_model as pm
from tests import test_gpu_tier_driver as drv
from tests import test_gpu_tier_variable as var


def test_driver_seed_meets_the_precondition():
  _, prefill, batches = drv._universe()
  assert len(batches) == drv.STEPS and all(b.size == drv.BATCH == np.unique(b).size for b in batches)
  assert all(drv._saturated(b, 89) == 0 for b in prefill + batches)


def test_a_crafted_pair_does_saturate():
  keys = pm.craft(89, b0=29, b1=34, count=32)
  assert drv._saturated(keys, 89) == 32


def test_variable_seeds_meet_the_precondition():
  for seed in (23, 29):
    ids, _ = var._batches(seed)
    assert all(drv._saturated(np.unique(i), 89) == 0 for i in ids)
