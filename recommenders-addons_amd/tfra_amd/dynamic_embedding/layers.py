"""`tfra_amd.dynamic_embedding.layers` (also `de.keras.layers`) — mirrors the layers of
`tensorflow_recommenders_addons/dynamic_embedding/python/keras/layers/embedding.py` (PY/keras/layers/embedding.py:111-540):
`Embedding`, `SquashedEmbedding` and `FieldWiseEmbedding`.

The classes are plain Python objects, not `torch.nn.Module`: the parameter is a `Variable` (`.params`), trained through the
wrapper a call returns — `layer(ids, return_trainable=True)` gives `(out, wrapper)` as every lookup of this package does — and
`DynamicEmbeddingOptimizer.apply_gradients` / `apply_combined_gradients`.  The layers own no kernel but one: `FieldWiseEmbedding`
builds its per-field pooling lists on the device (`device_ops.field_entries`, one launch) and hands them to the ragged pooled
lookup, so the admission (`init_on_lookup`, tiered shards), the write-back plan and the fused combined write-back serve it as they
serve any sparse lookup.

Differences from the reference, all of them the package's: the variable is made by `Variable(...)` directly (no sharing by name);
`initializer=None` is the variable's default (a zero row) where the reference draws RandomNormal — pass a callable for random rows;
`max_norm` is refused, as the sparse training paths refuse it."""
import torch

from . import device_ops, ragged_embedding_ops
from .variable import Variable, _pooled_forward, _pooled_training, default_partition_fn, embedding_lookup, embedding_lookup_unique

_LAYER_KWARGS = ("trainable", "bp_v2", "restrict_policy", "init_capacity", "partitioner", "kv_creator", "checkpoint",
                 "short_file_name", "max_norm", "init_on_lookup", "aux_fields", "aux_init")
_REDUCTIONS = {
    "sum": lambda x, d: x.sum(d),
    "mean": lambda x, d: x.mean(d),
    "max": lambda x, d: x.amax(d),
    "min": lambda x, d: x.amin(d),
    "prod": lambda x, d: x.prod(d),
}
_SEGMENT_COMBINERS = {"sum": "sum", "mean": "mean", "sqrtn": "sqrtn", "sqrt_n": "sqrtn"}   # (the reference spells it sqrt_n)


def reduce_pooling(x, combiner="sum"):
  """PY/keras/layers/embedding.py:87-108: a lookup result [batch, s1, ..., sn, dim] reduced to [batch, dim] — axis 1 until two
  axes are left —, a single example's [s, dim] to [dim]."""
  if combiner not in _REDUCTIONS:
    raise ValueError("combiner must be one of %s, got %r" % (sorted(_REDUCTIONS), combiner))
  reduce = _REDUCTIONS[combiner]
  if x.dim() < 2:
    raise ValueError("reduce_pooling need at least dim-2 input.")
  if x.dim() == 2:
    return reduce(x, 0)
  for _ in range(x.dim() - 2):
    x = reduce(x, 1)
  return x


class Embedding:
  """PY/keras/layers/embedding.py:111-294.  ids of any shape -> ids.shape + (embedding_size,): `embedding_lookup_unique`
  (with_unique, the default) or `embedding_lookup`.

  embedding_size, key_dtype, value_dtype, initializer, devices: the `Variable`'s dim, dtypes, initializer and devices.  combiner
  is kept for the subclasses.  **kwargs: trainable, bp_v2, restrict_policy, init_capacity (the variable's init_size), partitioner,
  kv_creator, checkpoint, short_file_name as the reference's; init_on_lookup, aux_fields, aux_init pass through to the `Variable`;
  max_norm other than None raises ValueError; anything else TypeError."""

  def __init__(self, embedding_size, key_dtype=torch.int64, value_dtype=torch.float32, combiner="sum", initializer=None,
               devices=None, name="DynamicEmbeddingLayer", with_unique=True, **kwargs):
    try:
      embedding_size = int(embedding_size)
    except Exception:
      raise TypeError("embedding size must be convertible to integer, but get {}".format(type(embedding_size)))
    for k in kwargs:
      if k not in _LAYER_KWARGS:
        raise TypeError("%s got an unexpected keyword argument %r" % (type(self).__name__, k))
    if kwargs.get("max_norm") is not None:
      raise ValueError("max_norm is not supported by the layers: the gradient through the clip by norm is not formed")
    self.embedding_size = embedding_size
    self.combiner = combiner
    self.max_norm = None
    self.with_unique = bool(with_unique)
    self.name = name
    self.trainable = kwargs.get("trainable", True)
    passed = {k: kwargs[k] for k in ("init_on_lookup", "aux_fields", "aux_init", "short_file_name") if k in kwargs}
    self.params = Variable(key_dtype=key_dtype, value_dtype=value_dtype, dim=embedding_size, devices=devices,
                           partitioner=kwargs.get("partitioner", default_partition_fn),
                           name=name + "-parameter" if name else "EmbeddingParameter", initializer=initializer,
                           trainable=self.trainable, checkpoint=kwargs.get("checkpoint", True),
                           init_size=kwargs.get("init_capacity", 0), kv_creator=kwargs.get("kv_creator", None),
                           restrict_policy=kwargs.get("restrict_policy", None), bp_v2=kwargs.get("bp_v2", False), **passed)

  def _lookup(self, ids, return_trainable, plan_writeback):
    if self.with_unique:
      if plan_writeback:
        raise ValueError("plan_writeback needs with_unique=False: embedding_lookup_unique starts no write-back plan")
      return embedding_lookup_unique(self.params, ids, return_trainable=return_trainable)
    return embedding_lookup(self.params, ids, return_trainable=return_trainable, plan_writeback=plan_writeback)

  def __call__(self, ids, return_trainable=False, plan_writeback=False):
    """ids.shape + (embedding_size,); with return_trainable (out, TrainableWrapper) — over the UNIQUE ids with with_unique, as
    `embedding_lookup_unique` returns it."""
    return self._lookup(ids, return_trainable, plan_writeback)

  call = __call__


BasicEmbedding = Embedding


class SquashedEmbedding(Embedding):
  """PY/keras/layers/embedding.py:348-369: the lookup result squashed to [batch, dim] (`reduce_pooling`), a single example's
  [s] ids to [dim].  combiner: "sum", "mean", "max", "min" or "prod".

  Rank-2 ids [B, S] with "sum" or "mean" over a variable the pooled route serves are ONE launch: the ragged pooled lookup over the
  splits arange(B + 1) * S (no [B, S, dim] rows; S == 0 gives zero rows).  Every other rank or combiner, and every other variable,
  is the lookup followed by the torch reduction.  return_trainable: the pooled route's SparseTrainableWrapper
  (`apply_combined_gradients` with the gradient of the [B, dim] result); elsewhere ValueError."""

  def __init__(self, embedding_size, key_dtype=torch.int64, value_dtype=torch.float32, combiner="sum", initializer=None,
               devices=None, name="DynamicEmbeddingLayer", with_unique=True, **kwargs):
    if combiner not in _REDUCTIONS:
      raise ValueError("combiner must be one of %s, got %r" % (sorted(_REDUCTIONS), combiner))
    super().__init__(embedding_size, key_dtype=key_dtype, value_dtype=value_dtype, combiner=combiner, initializer=initializer,
                     devices=devices, name=name, with_unique=with_unique, **kwargs)

  def __call__(self, ids, return_trainable=False, plan_writeback=False):
    ids = torch.as_tensor(ids, device=self.params._primary)
    why = None
    if ids.dim() != 2:
      why = "ids of rank %d (the pooled route takes rank 2)" % ids.dim()
    elif self.combiner not in ("sum", "mean"):
      why = "combiner %r (the pooled route has sum and mean)" % self.combiner
    elif not (_pooled_training if return_trainable else _pooled_forward)(self.params, None):
      why = "a variable the pooled lookup does not serve (several shards, bp_v2, dim % 4 != 0 or dim > 256, other dtypes)"
    if why is None:
      b, s = ids.shape
      splits = torch.arange(b + 1, dtype=torch.int64, device=ids.device) * s
      return ragged_embedding_ops.embedding_lookup_sparse(self.params, (splits, ids.reshape(-1)), None, combiner=self.combiner,
                                                          return_trainable=return_trainable, plan_writeback=plan_writeback)
    if return_trainable:
      raise ValueError("SquashedEmbedding trains through the pooled route only, not with " + why)
    return reduce_pooling(self._lookup(ids, False, False), self.combiner)

  call = __call__


class FieldWiseEmbedding(Embedding):
  """PY/keras/layers/embedding.py:372-513: every categorical field of a model in ONE table.  ids [batch, per_sample];
  `slot_map_fn(ids)` gives every id its field in [0, nslots); the result is [batch, nslots, dim]: per sample and field the
  combined rows of the field's ids ("sum", "mean" or "sqrtn" — the reference's "sqrt_n" is accepted —; zeros where a sample has
  none).  Within a field the rows are combined in input order (the reference's argsort leaves ties open).

  The call: slots = slot_map_fn(ids); `device_ops.field_entries` orders the ids by (sample, field, position) and writes the
  batch * nslots + 1 splits in one launch; `ragged_embedding_ops.embedding_lookup_sparse` reads them — the pooled lookup where
  the variable has it, else its chain (dim 2, several shards, bp_v2).  return_trainable: (out, SparseTrainableWrapper); the
  gradient `apply_combined_gradients` takes has the result's shape [batch, nslots, dim].  plan_writeback as any sparse lookup's.
  A slot outside [0, nslots) is the caller's error: it is clamped into range and counted (`bad_slots`)."""

  def __init__(self, embedding_size, nslots, slot_map_fn=None, key_dtype=torch.int64, value_dtype=torch.float32, combiner="sum",
               initializer=None, devices=None, name="SlotDynamicEmbeddingLayer", with_unique=True, **kwargs):
    if not callable(slot_map_fn):
      raise ValueError("slot_map_fn is not callable.")
    self.slot_map_fn = slot_map_fn
    try:
      nslots = int(nslots)
    except Exception:
      raise TypeError("nslots should be convertible to int, but get {}".format(type(nslots)))
    if nslots < 1:
      raise ValueError("nslots must be >= 1, got %d" % nslots)
    self.nslots = nslots
    if combiner not in _SEGMENT_COMBINERS:
      raise ValueError("combiner must be one of %s, got %r" % (sorted(_SEGMENT_COMBINERS), combiner))
    super().__init__(embedding_size, key_dtype=key_dtype, value_dtype=value_dtype, combiner=combiner, initializer=initializer,
                     devices=devices, name=name, with_unique=with_unique, **kwargs)
    self._bad = torch.zeros(1, dtype=torch.int64, device=self.params._primary)

  def __call__(self, ids, return_trainable=False, plan_writeback=False):
    if torch.as_tensor(ids).dim() > 2:
      raise NotImplementedError("Input dimension higher than 2 is not implemented yet.")
    ids = torch.as_tensor(ids, device=self.params._primary)
    if ids.dim() != 2:
      raise ValueError("FieldWiseEmbedding takes ids of shape [batch, per_sample], got %s" % list(ids.shape))
    slots = torch.as_tensor(self.slot_map_fn(ids), device=ids.device)
    if slots.numel() != ids.numel():
      raise ValueError("slot_map_fn must return one slot per id: %d slots for %d ids" % (slots.numel(), ids.numel()))
    pooled = (_pooled_training if return_trainable else _pooled_forward)(self.params, None)
    # (the row id of every entry is wanted by the wrapper, and by the chain of a variable the pooled lookup does not serve)
    entry_ids, splits, _, seg = device_ops.field_entries(ids, slots, self.nslots, want_seg=return_trainable or not pooled,
                                                         bad=self._bad)
    shape = (ids.shape[0], self.nslots, self.embedding_size)
    res = ragged_embedding_ops.embedding_lookup_sparse(self.params, (splits, entry_ids), None,
                                                       combiner=_SEGMENT_COMBINERS[self.combiner],
                                                       return_trainable=return_trainable, plan_writeback=plan_writeback,
                                                       entry_seg=seg, out_shape=shape)
    if return_trainable:
      return res[0].reshape(shape), res[1]
    return res.reshape(shape)

  call = __call__

  def bad_slots(self):
    """The number of slots outside [0, nslots) that `slot_map_fn` has returned so far: the layer's ONE host read, optional."""
    return int(self._bad.item())
