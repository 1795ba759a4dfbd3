"""`Variable`, `get_variable`, `embedding_lookup*` — host-side mirror of the reference API.

PY = /root/reference/tensorflow_recommenders_addons/dynamic_embedding/python/ops
  Variable ............... PY/dynamic_embedding_variable.py:453-1262
  default_partition_fn ... PY/dynamic_embedding_variable.py:165-197
  get_variable ........... PY/dynamic_embedding_variable.py:1265-1359
  embedding_lookup ....... PY/dynamic_embedding_variable.py:1362-1530
  embedding_lookup_unique / _sparse / safe_..._sparse  PY/dynamic_embedding_ops.py:64-430
  TrainableWrapper ....... PY/embedding_weights.py:38-540 (prefetch_values / update_op)

A logical table = N physical tables (`devices=[...]`, one shard per entry); every call is
partition -> per-shard table op -> stitch, the partition/stitch being device kernels
(tfra_partition / tfra_scatter_rows) instead of tf.dynamic_partition/dynamic_stitch.
"""
import torch

from . import device_ops, table_ops
from ._args import _as_device, _out_dtype, _score_filter
from .table_ops import CuckooHashTable, HkvHashTable, HkvEvictStrategy, SparsePlan, TieredHashTable


def default_partition_fn(keys, shard_num):
  """PY/dynamic_embedding_variable.py:165-197 on an accelerator build: int64 keys go to ``int32(key & 0x7fffffff) % shard_num``
  (:182-190), keys of any other dtype — int32 — to ``math_ops.mod(keys, shard_num)``, floor mod (:191-196).  Kept as a python
  callable for API parity; the Variable recognises it and runs the fused device partition instead."""
  if shard_num <= 1:
    return torch.zeros(keys.shape, dtype=torch.int32, device=keys.device)
  if keys.dtype == torch.int64:
    return ((keys & 0x7FFFFFFF).to(torch.int32) % shard_num).to(torch.int32)
  return torch.remainder(keys, shard_num).to(torch.int32)    # floor mod: the sign of the divisor, as tf.math.mod


class KVCreator:
  """PY/dynamic_embedding_creator.py:36-78"""

  def __init__(self, config=None):
    self.config = config

  def create(self, **kw):
    raise NotImplementedError


class CuckooHashTableConfig:
  """PY/dynamic_embedding_creator.py:80-88 (empty in the reference too)."""


class CuckooHashTableCreator(KVCreator):
  """PY/dynamic_embedding_creator.py:91-138"""

  def create(self, key_dtype=None, value_dtype=None, default_value=None, name=None, checkpoint=None, init_size=None,
             config=None, device=None, shard_saveable_object_fn=None, **kw):
    return CuckooHashTable(key_dtype=key_dtype, value_dtype=value_dtype, default_value=default_value, name=name,
                           checkpoint=checkpoint, init_size=init_size or 0, config=config or self.config, device=device,
                           **kw)


class HkvHashTableConfig:
  """PY/dynamic_embedding_creator.py:149-169"""

  def __init__(self, init_capacity=1024 * 1024, max_capacity=1024 * 1024, max_hbm_for_values=1024 * 1024 * 1024,
               evict_strategy=HkvEvictStrategy.LRU, step_per_epoch=0, gen_scores_fn=None, reserved_key_start_bit=0):
    self.init_capacity = init_capacity
    self.max_capacity = max_capacity
    self.max_hbm_for_values = max_hbm_for_values
    self.evict_strategy = evict_strategy
    self.step_per_epoch = step_per_epoch
    self.gen_scores_fn = gen_scores_fn
    self.reserved_key_start_bit = reserved_key_start_bit


class HkvHashTableCreator(KVCreator):
  """PY/dynamic_embedding_creator.py:172-230"""

  def create(self, key_dtype=None, value_dtype=None, default_value=None, name=None, checkpoint=None, init_size=None,
             config=None, device=None, shard_saveable_object_fn=None, **kw):
    cfg = config or self.config or HkvHashTableConfig()
    return HkvHashTable(key_dtype=key_dtype, value_dtype=value_dtype, default_value=default_value, name=name,
                        checkpoint=checkpoint, config=cfg, device=device, **kw)


class TieredHashTableConfig:
  """A bounded cache in front of a growing table (`TieredHashTable`).  upper: the HkvHashTableConfig of the cache — LRU or EPOCHLRU,
  init_capacity == max_capacity so that it evicts from the start; lower: the CuckooHashTableConfig of the table below; max_batch:
  the most keys one lookup or insert may carry (the tier driver's staging is sized by it)."""

  def __init__(self, upper=None, lower=None, max_batch=1 << 18):
    self.upper = upper if upper is not None else HkvHashTableConfig()
    self.lower = lower if lower is not None else CuckooHashTableConfig()
    self.max_batch = int(max_batch)


class TieredHashTableCreator(KVCreator):
  """Creates `TieredHashTable` shards: `Variable(kv_creator=TieredHashTableCreator(TieredHashTableConfig(...)))`."""

  def create(self, key_dtype=None, value_dtype=None, default_value=None, name=None, checkpoint=None, init_size=None,
             config=None, device=None, shard_saveable_object_fn=None, **kw):
    cfg = config or self.config or TieredHashTableConfig()
    return TieredHashTable(key_dtype=key_dtype, value_dtype=value_dtype, default_value=default_value, name=name,
                           checkpoint=checkpoint, config=cfg, device=device, init_size=init_size or 0, **kw)


def _has_tiered_shards(var):
  """Whether `var` (a Variable, or anything with its `_tables`) keeps its rows in TieredHashTable shards."""
  return any(isinstance(t, TieredHashTable) for t in getattr(var, "_tables", ()))


def _pooled_reader(shard):
  """What serves a shard's pooled read: a TieredHashTable itself — its `find_combine` / `find_combine_ragged` and their
  `*_weight_grad` forms read both tiers —, else the shard's device table."""
  return shard if isinstance(shard, TieredHashTable) else shard._table


def misses_are_static(var):
  """Whether a key the optimizer write-back does not find may start from the ONE static default row of `var` (a Variable, or
  anything with its `initializer`): there is no callable initializer, or the step's lookup has admitted every key with its own
  row already (init_on_lookup), so the write-back only hits.  The one predicate behind every fused write-back's eligibility."""
  return not callable(var.initializer) or bool(getattr(var, "init_on_lookup", False))


class Variable:
  """A sharded dynamic-embedding table (PY/dynamic_embedding_variable.py:453-692).

  init_on_lookup (opt-in, default False): the lookup of a training step ADMITS.  `embedding_lookup(..., return_trainable=True)` and
  `embedding_lookup_sparse(..., return_trainable=True)` of a non-bp_v2 variable de-duplicate their ids on the device, draw one
  initializer row per unique id and call the table's find_or_insert (`lookup_or_insert`): a never-seen id enters the table with the
  row the model is handed, every position of a repeated id sees that one row, and the admitting lookup reads nothing on the host.  The write-back then
  only hits, so a variable with a callable initializer takes the planned, one-call and combined write-backs (`misses_are_static`),
  and the row that is updated is the row the forward pass returned — with False the write-back draws a second row from the
  initializer for every miss.  Optimizer slots start at aux_init when the lookup admits the key.
  One limit: a key that was looked up but is not resident at write-back time — evicted in between, or not admitted by a table at
  max_capacity under LFU / CUSTOMIZED — is updated from the static default row, as in every fused write-back.  Over tiered shards
  (`TieredHashTableCreator`: a bounded cache in front of a growing table, whole rows moving between them) the lookup leaves every key
  of the batch in the cache, and the same limit has one more case: a batch that fills both home buckets of one of its own keys with
  its own keys (30 slots) cannot keep that key in the cache; its row is safe below, but the write-back restarts it from the default row.
  Plain lookups (`lookup`, `embedding_lookup` without return_trainable, the pooled forward) never admit, with either setting.

  init_on_lookup="plan": True for every predicate above, and `embedding_lookup(..., return_trainable=True)` of repeating ids on a
  one-shard variable whose write-back is the planned one (`DynamicEmbeddingOptimizer.can_plan`) builds the write-back plan of the
  batch on the current stream and looks the ids up THROUGH it (the table's find_or_insert_planned): no tf.unique, no gather, and
  `apply_gradients` takes that same plan — the batch is de-duplicated once per step instead of twice.  Row p of the one draw
  initializer([n, dim]) belongs to batch position p, and a never-seen id enters with the row of its LAST position (with True: row
  j belongs to the j-th distinct id in first-occurrence order), so the two settings admit different rows for the same seed.
  Several shards, more than 2^18 ids, no free plan, the sparse wrapper, or tiered shards: the True route.  (A tier has the planned
  lookup — `TieredHashTable.find_or_insert_planned` — but a step through it was measured 13.0 us below True's 206.6 with spreads that
  sum to 15.0, short of the margin, so the variable does not route to it: DESIGN 4.26.)  Measured (Adam, 131 072 Zipf ids, 10 %
  never seen, us per step): False 153.5, True 159.1, True with plan_writeback 158.5, "plan" 134.5.

  init_on_lookup="pooled": True for every predicate above and for the dense `embedding_lookup`; the TRAINING forms of the sparse
  lookups (`embedding_lookup_sparse`, `safe_embedding_lookup_sparse`, `ragged_embedding_ops.*` and their `*_many` forms, with
  return_trainable=True) of a variable with a callable initializer that meets `can_lookup_combined()`'s other conditions (one
  shard, float32 / float16 / bfloat16, dim % 4 == 0, dim <= 256; not bp_v2, no max_norm) admit first and read once
  (`can_admit_pooled`): the entry ids de-duplicated on the device with the count left there, ONE draw
  initializer([n_entry_ids, dim]) whose row j belongs to unique id j, `admit` (find_or_insert with no rows handed back; over a
  tiered shard `TieredHashTable.admit` with those rows), then the pooled read — no [U, dim] rows, nothing read on the host when
  num_rows is given, and in the `*_many` forms ONE grouped admission (tfra_multi_find_or_insert) from ADMIT_MANY_MIN_TABLES plain
  members on.  Non-training sparse lookups keep the chain and insert nothing (a miss is drawn and stays out: `_read_rows`; with
  True the chain's `embedding_lookup` admits there too); several shards take the True route.
  Limits: (1) with the chain the model sees a drawn row even for a key a full LFU / CUSTOMIZED table does not admit, or one a later
  key of the same batch displaces; with "pooled" such a key reads as the table's static default row, and the write-back restarts
  it from there — the existing limit of every fused write-back.  (2) A seeded random initializer draws [n_entry_ids, dim] here
  against [U, dim] with True, so the two settings admit different rows for the same seed (as "plan" does).  (3) What is admitted
  are the ENTRY ids, the safe form's entry for empty rows (default_id, or 0) among them, where the chain admits the looked-up ids.
  (4) More entry ids than a tier's max_batch: the existing ValueError."""

  def __init__(self, key_dtype=torch.int64, value_dtype=torch.float32, dim=1, devices=None,
               partitioner=default_partition_fn, shared_name=None, name="DynamicEmbedding_Variable", initializer=None,
               trainable=True, checkpoint=True, init_size=0, kv_creator=None, restrict_policy=None, bp_v2=False,
               short_file_name=False, aux_fields=0, aux_init=(0.0, 0.0, 0.0, 0.0), init_on_lookup=False,
               stochastic_rounding=None):
    self.key_dtype = key_dtype
    if isinstance(init_on_lookup, str) or init_on_lookup not in (False, True):
      if init_on_lookup not in ("plan", "pooled"):
        raise ValueError("init_on_lookup must be False, True, \"plan\" or \"pooled\", got %r" % (init_on_lookup,))
    else:
      init_on_lookup = bool(init_on_lookup)
    self.init_on_lookup = init_on_lookup   # (False, True, "plan" or "pooled": truthy means "the lookup admits" for every predicate)
    self.value_dtype = value_dtype
    self.dim = int(dim)
    self.bp_v2 = bp_v2
    self.name = name
    self.trainable = trainable
    self.checkpoint = checkpoint
    self.aux_fields = aux_fields
    self.devices = list(devices) if devices else ["cuda:%d" % torch.cuda.current_device()]
    self.shard_num = len(self.devices)
    self.partition_fn = partitioner
    self.init_size = int(init_size / self.shard_num)  # PY/..._variable.py:597
    self.initializer = initializer
    self.kv_creator = kv_creator if kv_creator else CuckooHashTableCreator()
    # static default row: first element of the initializer (PY/..._variable.py:723-765)
    if initializer is None:
      static_default = 0
    elif callable(initializer):
      static_default = initializer([1, self.dim]).reshape(-1)[0].item()
    else:
      static_default = torch.as_tensor(initializer).reshape(-1)[0].item()
    self._static_default = static_default
    default_value = torch.full((self.dim,), static_default, dtype=value_dtype)
    self._tables = []
    for idx, dev in enumerate(self.devices):
      self._tables.append(
          self.kv_creator.create(key_dtype=key_dtype, value_dtype=value_dtype, default_value=default_value,
                                 name=self._make_name(idx), checkpoint=checkpoint, init_size=self.init_size, device=dev,
                                 dim=self.dim, aux_fields=aux_fields, aux_init=aux_init))
    self._primary = _as_device(self.devices[0])
    self.stochastic_rounding = None
    if stochastic_rounding:
      self.set_stochastic_rounding(stochastic_rounding)
    # PY/dynamic_embedding_variable.py:604-611: the policy CLASS is passed, instantiated on this variable
    if restrict_policy is not None:
      from .restrict_policies import RestrictPolicy
      if not (isinstance(restrict_policy, type) and issubclass(restrict_policy, RestrictPolicy)):
        raise TypeError("restrict_policy must be subclass of RestrictPolicy.")
      self._restrict_policy = restrict_policy(self)
    else:
      self._restrict_policy = None

  @property
  def restrict_policy(self):
    return self._restrict_policy

  def get_slot_variables(self, optimizer):
    """PY/dynamic_embedding_variable.py:1157-1200: the optimizer's state variables of this parameter, sorted by
    name (here: views on the co-located state vectors of the rows)."""
    return sorted((optimizer.get_slot(self, n) for n in optimizer.get_slot_names()), key=lambda v: v.name)

  def restrict(self, num_reserved, **kwargs):
    """PY/dynamic_embedding_variable.py:857-874: no-op without a policy."""
    if self._restrict_policy is not None:
      return self._restrict_policy.apply_restriction(num_reserved, **kwargs)
    return None

  def _make_name(self, table_idx):
    """PY/dynamic_embedding_variable.py:768-770"""
    return "{}_mht_{}of{}".format(self.name.replace("/", "_"), table_idx + 1, self.shard_num)

  @property
  def tables(self):
    return self._tables

  # ---- partition / stitch ------------------------------------------------------------------
  def _partition(self, keys):
    """-> (keys_per_shard, perm, counts_host). perm is None for 1 shard."""
    flat = keys.reshape(-1)
    if self.shard_num <= 1:
      return [flat], None, [flat.numel()]
    if self.partition_fn is default_partition_fn:
      # default_partition_fn's rule follows the key dtype: mask-mod for int64 keys, floor mod for int32 keys
      # (PY/dynamic_embedding_variable.py:182-196; they differ for negative keys when shard_num is not a power of two)
      owner_major, perm, counts = device_ops.partition(flat, self.shard_num, device_ops.default_partition_mode(flat.dtype))
    else:
      owner = self.partition_fn(flat, self.shard_num)
      perm, counts = device_ops.partition_by_owner(owner, self.shard_num)
      owner_major = device_ops.gather_rows(flat.reshape(-1, 1), perm).reshape(-1)
    c = counts.tolist()  # data-dependent shapes: one host read, like tf.dynamic_partition
    return list(torch.split(owner_major, c)), perm, c

  def _split_rows(self, rows, perm, counts):
    """`rows` — [n, width], or a bool vector [n] (gathered as uint8) — in owner-major order, one slice per shard."""
    if perm is None:
      return [rows]
    if rows.dtype == torch.bool:
      return list(torch.split(device_ops.gather_rows(rows.reshape(-1, 1).to(torch.uint8), perm).reshape(-1).to(torch.bool), counts))
    return list(torch.split(device_ops.gather_rows(rows, perm), counts))

  def _fan_out(self, keys, *rows, values=None):
    """The first half of every sharded call -> (keys, perm, counts, shards): `keys` as a tensor on the primary device, the
    partition's permutation (None for 1 shard) and host counts, and per shard the tuple (table, its keys, its slice of each
    operand) on the shard's device.  An operand is one of `rows` ([n, width], or a bool vector [n]), index-aligned with the
    flattened keys; `values`, when given, is the first of them, after the check that it has one row of dim per key."""
    keys = torch.as_tensor(keys, device=self._primary)
    if values is not None:
      values = torch.as_tensor(values, device=self._primary)
      want = tuple(keys.shape) + (self.dim,)
      if tuple(values.shape) != want:
        raise ValueError("Expected shape %s for values, got %s" % (list(want), list(values.shape)))
      rows = (values.reshape(-1, self.dim),) + rows
    kp, perm, counts = self._partition(keys)
    shards = [(t, k.to(t._device)) for t, k in zip(self._tables, kp)]
    for r in rows:
      shards = [s + (x.to(s[0]._device),) for s, x in zip(shards, self._split_rows(r, perm, counts))]
    return keys, perm, counts, shards

  def _stitch_rows(self, parts, perm, shape):
    """The second half: per-shard row tensors (owner-major order) back in batch order on the primary device, [*shape, dim]."""
    if perm is None:
      return parts[0].to(self._primary).reshape(tuple(shape) + (self.dim,))
    return device_ops.scatter_rows(torch.cat([p.to(self._primary) for p in parts], 0), perm).reshape(tuple(shape) + (self.dim,))

  def _scatter_flags(self, parts, perm, shape):
    """Per-shard bool vectors (owner-major order) back in batch order on the primary device, as `lookup` returns its exists."""
    if perm is None:
      return parts[0].to(self._primary).reshape(shape)
    flags = torch.cat([p.to(self._primary) for p in parts], 0).reshape(-1, 1).to(torch.uint8)
    return device_ops.scatter_rows(flags, perm).reshape(-1).to(torch.bool).reshape(shape)

  # ---- table ops ---------------------------------------------------------------------------
  def upsert(self, keys, values, name=None):
    """PY/dynamic_embedding_variable.py:772-804"""
    for t, k, v in self._fan_out(keys, values=values)[3]:
      t.insert(k, v)

  def upsert_and_evict(self, keys, values, name=None):
    """upsert that returns (evicted_keys, evicted_values, evicted_scores) on the primary device: what every shard displaced or
    did not admit because of this call (HkvHashTable.insert_and_evict per shard, concatenated as export does)."""
    for t in self._tables:
      if not hasattr(t, "insert_and_evict"):
        raise NotImplementedError("upsert_and_evict needs bounded tables with scores; %s tables never evict (use an "
                                  "HkvHashTableCreator)" % type(t).__name__)
    out = [t.insert_and_evict(k, v) for t, k, v in self._fan_out(keys, values=values)[3]]
    return tuple(torch.cat([o[j].to(self._primary) for o in out], 0) for j in range(3))

  def accum(self, keys, old_values, new_values, exists, name=None):
    """PY/dynamic_embedding_variable.py:806-855: where(exists, new-old, new) then per-shard accum."""
    exists = torch.as_tensor(exists, device=self._primary).reshape(-1).to(torch.bool)
    old_values = old_values.reshape(-1, self.dim)
    new_values = new_values.reshape(-1, self.dim)
    vod = torch.where(exists[:, None], new_values - old_values, new_values)
    for t, k, v, e in self._fan_out(keys, vod, exists)[3]:
      t.accum(k, v, e)

  def remove(self, keys, name=None):
    """PY/dynamic_embedding_variable.py:877-902"""
    for t, k in self._fan_out(keys)[3]:
      t.remove(k)

  def clear(self, name=None):
    for t in self._tables:
      t.clear()

  def set_stochastic_rounding(self, seed):
    """seed None or 0: off (the default).  Otherwise the fused optimizer write-backs (SGD, Adam, Adagrad, Ftrl) of this float16 /
    bfloat16 variable round the parameter and the slots stochastically instead of to nearest even, so that updates below half a
    storage ulp are kept in the mean; shard i takes seed + i.  The stored bits are a pure function of (seed, write-backs since
    this call, key, element).  Not for CapturedTrainStep (a replayed graph would reuse one set of random bits); the Generic
    optimizers ignore it (Momentum / RMSProp without fused=True among them; with fused=True they round this way too)."""
    seed = 0 if seed is None else int(seed)
    for i, t in enumerate(self._tables):
      t.set_stochastic_rounding((seed + i) & ((1 << 64) - 1) if seed else 0)
    self.stochastic_rounding = seed or None

  def _create_default_values_by_initializer(self, n, device):
    """PY/dynamic_embedding_variable.py:919-931: full-size [n,dim] defaults from the initializer."""
    if self.initializer is None or not callable(self.initializer):
      return None
    return self.initializer([n, self.dim]).to(device=device, dtype=self.value_dtype)

  def lookup(self, keys, return_exists=False, name=None, out_dtype=None):
    """PY/dynamic_embedding_variable.py:933-986.  out_dtype: the rows in float32 / float16 / bfloat16 instead of the value dtype,
    bit for bit `lookup(...).to(out_dtype)`: every plain shard converts in its lookup's kernel (tfra_table_find_typed; the
    conversion commutes with the stitching), a tiered shard's rows are converted behind its call.  The defaults stay in the value dtype."""
    return self._lookup_through("lookup", keys, return_exists, return_exists, _out_dtype(out_dtype))

  def _lookup_through(self, method, keys, shard_exists, return_exists, out_dtype=None):
    """The body of `lookup` and `lookup_or_insert`: every shard's `method` ("lookup" or "find_or_insert") over the shard's keys and
    its defaults — one draw of the callable initializer per shard, else None —, asked for exists when shard_exists, and the
    results stitched back into batch order."""
    keys, perm, _, shards = self._fan_out(keys)
    vals, exs = [], []
    for t, k in shards:
      typed = out_dtype is not None and not isinstance(t, TieredHashTable)   # (the typed lookups: `lookup` on a plain shard)
      kw = {"out_dtype": out_dtype} if typed else {}
      r = getattr(t, method)(k, dynamic_default_values=self._create_default_values_by_initializer(k.numel(), t._device),
                             return_exists=shard_exists, **kw)
      if out_dtype is not None and not typed:   # a tiered shard: its calls are not typed, the rows are converted
        r = (r[0].to(out_dtype), r[1]) if shard_exists else r.to(out_dtype)
      if shard_exists:
        vals.append(r[0])
        exs.append(r[1])
      else:
        vals.append(r)
    v = self._stitch_rows(vals, perm, keys.shape)
    return (v, self._scatter_flags(exs, perm, keys.shape)) if return_exists else v

  def misses_are_static(self):
    """The module's `misses_are_static` of this variable."""
    return misses_are_static(self)

  def admits_on_lookup(self):
    """Whether a training step's lookup admits never-seen keys: init_on_lookup, and a callable initializer to draw their rows
    from (with a static default row a miss reads the row the write-back starts from anyway).  Over tiered shards the lookup
    always admits, static default row or not: a key that is below must be promoted before the write-back, which acts on the cache."""
    return (bool(self.init_on_lookup) and callable(self.initializer)) or _has_tiered_shards(self)

  def lookup_or_insert(self, keys, return_exists=False, name=None):
    """`lookup` that admits (find_or_insert per shard): a key that is not resident enters its table with the row this call
    returns for it — a row of the callable initializer (one draw of [n, dim] per shard, row j for that shard's key j), else
    the static default row — as `upsert` would insert it.  `keys` must be UNIQUE.  exists[i] is False for every key that was
    not resident before the call."""
    return self._lookup_through("find_or_insert", keys, True, return_exists)

  # ---- the read side of a tier (tables in front of something slower) ---------------------------
  def lookup_missed(self, keys, return_exists=False, name=None):
    """`lookup` that also lists its misses (find_missed per shard) -> (rows, missed_keys, missed_positions[, exists]): the keys
    that are not resident and their positions in the flattened batch (int64, index-aligned, in no particular order; a missing
    key that repeats is listed at every position).  Never inserts.  A callable initializer draws the defaults per shard, as
    `lookup` does.  A shard reports positions in its slice of the owner-major key list; they are mapped back through the
    partition's permutation (owner_major = flat[perm]).  A tiered shard lists the keys NEITHER of its tiers holds."""
    keys, perm, counts, shards = self._fan_out(keys)
    vals, exs, mks, mps = [], [], [], []
    off = 0
    for (t, k), count in zip(shards, counts):
      r = t._shard_find_missed(k, self._create_default_values_by_initializer(k.numel(), t._device), return_exists)
      vals.append(r[0])
      mks.append(r[1].to(self._primary))
      pos = r[2].to(self._primary).to(torch.int64)
      mps.append(pos if perm is None else perm[off + pos].to(torch.int64))
      if return_exists:
        exs.append(r[3])
      off += count
    out = (self._stitch_rows(vals, perm, keys.shape), torch.cat(mks, 0), torch.cat(mps, 0))
    return out + (self._scatter_flags(exs, perm, keys.shape),) if return_exists else out

  def assign(self, keys, values, return_found=False, name=None):
    """`upsert` for the keys that are resident; the others change nothing — they are not inserted and nothing is evicted for them
    (assign per shard).  `keys` must be UNIQUE.  -> None, or found (bool, shaped like keys): False = send the row to the tier
    that holds the key.  `size()` never changes.  A tiered shard writes the row in both of its tiers (found: in either)."""
    keys, perm, _, shards = self._fan_out(keys, values=values)
    fs = [t._shard_assign(k, v, return_found) for t, k, v in shards]
    return self._scatter_flags(fs, perm, keys.shape) if return_found else None

  def contains(self, keys, name=None):
    """A bool tensor shaped like keys: True where the key is resident (contains per shard; no row is read)."""
    keys, perm, _, shards = self._fan_out(keys)
    return self._scatter_flags([t.contains(k) for t, k in shards], perm, keys.shape)

  def can_lookup_combined(self):
    """Whether `lookup_combined` serves this variable: one shard, a static default row (no callable initializer), float32 /
    float16 / bfloat16 rows with dim % 4 == 0 and dim <= 256 — the conditions of the planned write-back (`can_plan`)."""
    from .optimizer import PLANNED_VALUE_DTYPES
    return (self.shard_num == 1 and not callable(self.initializer) and self.value_dtype in PLANNED_VALUE_DTYPES and
            self.dim % 4 == 0 and self.dim <= 256)

  def can_admit_pooled(self):
    """Whether a TRAINING sparse lookup of this variable takes the pooled route by admitting first (init_on_lookup="pooled"): a
    callable initializer to draw the admitted rows from, and `can_lookup_combined()`'s other conditions.  (Without a callable
    initializer `can_lookup_combined()` itself holds.)"""
    from .optimizer import PLANNED_VALUE_DTYPES
    return (self.init_on_lookup == "pooled" and callable(self.initializer) and self.shard_num == 1 and
            self.value_dtype in PLANNED_VALUE_DTYPES and self.dim % 4 == 0 and self.dim <= 256)

  def lookup_combined(self, ids, seg, weights, combiner, n_rows, name=None, out_dtype=None):
    """The forward of embedding_lookup_sparse as one pooled read (tfra_table_find_combine): [n_rows, dim] float32,
    out[r] = combiner over the entries p with seg[p] == r, in input order, of weights[p] * (row of ids[p], the default row on a
    miss).  seg ascending; weights None = all 1; combiner "sum" / "mean" / "sqrtn".  Bit-identical to
    unique -> lookup -> device_ops.sparse_segment_combine, without the unique pass and its host read.  Never inserts.
    out_dtype: the result in float32 / float16 / bfloat16, rounded in the lookup's kernel (tfra_table_find_combine_typed; a tier
    converts behind its call): bit for bit `lookup_combined(...).to(out_dtype)`."""
    t, ids = self._combined_operands(ids, ragged=False)
    if _out_dtype(out_dtype) is not None:
      return _pooled_reader(t).find_combine_typed(ids, seg, weights, device_ops.COMBINERS[combiner], n_rows, t._default_value,
                                                  out_dtype=out_dtype)
    return _pooled_reader(t).find_combine(ids, seg, weights, device_ops.COMBINERS[combiner], n_rows, t._default_value)

  def admit_entries(self, entry_ids):
    """Ahead of the pooled forward of a TRAINING step over tiered shards: the entry ids — the ids the step's write-back will touch,
    the safe form's entries for empty rows among them — de-duplicated on the device (`device_ops.unique_no_sync`) and admitted
    into the cache with the static default row (`TieredHashTable.admit`, the count left on the device).  A key from below comes
    up with its optimizer slots, a never-seen key enters as the write-back would have started it, so `apply_combined_gradients`
    only hits.  Nothing is read on the host.  More entry ids than the tier's max_batch: ValueError.
    An init_on_lookup="pooled" variable (`can_admit_pooled`), tiered or not, admits its entry ids the same way with ONE draw
    initializer([n_entry_ids, dim]) in the place of the static default row, row j for unique id j (`_admission_rows`).  Any
    other variable without tiered shards: nothing to do."""
    ids = self._admissible_entries(entry_ids)
    if ids is not None and ids.numel():
      t = self._tables[0]
      uniq, _, cnt = device_ops.unique_no_sync(ids)
      t.admit(uniq, self._admission_rows(ids.numel()), count=cnt)

  def _admission_rows(self, n):
    """The init rows `admit_entries` admits n entry ids with: one draw of the initializer, [n, dim], for an init_on_lookup="pooled"
    variable; else the shard's static default row."""
    t = self._tables[0]
    return self._create_default_values_by_initializer(n, t._device) if self.can_admit_pooled() else t._default_value

  def _admissible_entries(self, entry_ids):
    """`admit_entries`' check, with nothing enqueued: the flat entry ids on the shard's device (None: neither tiered shards nor
    `can_admit_pooled`), or its ValueError for more entry ids than the tier's max_batch.  The grouped forms run it for ALL their
    members before the first admission (`_check_entries_many`)."""
    tiered = _has_tiered_shards(self)
    if not tiered and not self.can_admit_pooled():
      return None
    t = self._tables[0]
    ids = torch.as_tensor(entry_ids, device=t._device).reshape(-1)
    if tiered and ids.numel() > t._tier.max_batch:
      raise ValueError("a pooled training lookup over a tiered variable admits its entry ids in one call: %d entry ids exceed the "
                       "tier's max_batch (%d)" % (ids.numel(), t._tier.max_batch))
    return ids

  def _combined_operands(self, ids, ragged):
    """-> (the one shard, the flat ids on its device) of a pooled read — the forward or the weight gradient, over one table or a
    tier (`_pooled_reader` serves the shard) —; ValueError unless `can_lookup_combined()`."""
    if not (self.can_lookup_combined() or self.can_admit_pooled()):
      raise ValueError("%s needs one shard, a static default row, float32 / float16 / bfloat16 rows, dim %% 4 == 0 and dim <= 256; "
                       "use %s" % (("lookup_combined_ragged", "ragged_embedding_ops.embedding_lookup_sparse") if ragged else
                                   ("lookup_combined", "embedding_lookup_sparse")))
    return self._tables[0], torch.as_tensor(ids, device=self._primary).reshape(-1)

  def lookup_combined_ragged(self, row_splits, ids, weights, combiner, prune=False, fill_id=None, name=None, out_dtype=None):
    """`lookup_combined` over a ragged batch (tfra_table_find_combine_ragged): [n_rows, dim] float32, row r combining the entries
    [row_splits[r], row_splits[r + 1]) — bit-identical to `lookup_combined` on the row ids the splits stand for, in one launch.
    prune / fill_id: safe_embedding_lookup_sparse's pruning by weight and its default_id (`_DeviceTable.find_combine_ragged`).
    Under `can_lookup_combined()`'s conditions.  Never inserts; nothing is read on the host.  out_dtype: as `lookup_combined`'s."""
    t, ids = self._combined_operands(ids, ragged=True)
    if _out_dtype(out_dtype) is not None:
      return _pooled_reader(t).find_combine_ragged(row_splits, ids, weights, device_ops.COMBINERS[combiner], prune=prune,
                                                   fill_id=fill_id, default_row=t._default_value, out_dtype=out_dtype)
    return _pooled_reader(t).find_combine_ragged(row_splits, ids, weights, device_ops.COMBINERS[combiner], prune=prune,
                                                 fill_id=fill_id, default_row=t._default_value)

  def lookup_combined_weight_grad(self, ids, seg, weights, combiner, grad_out, name=None):
    """The gradient of `lookup_combined` with respect to `weights` (tfra_table_find_combine_backprop_weights): float32 [nnz] from
    grad_out = d loss / d result, [n_rows, dim].  The rows are read from the table as they are now, as the forward reads them
    (the default row on a miss); nothing is inserted and no [nnz, dim] tensor exists.  weights None = all 1.  A tiered shard is
    read in both tiers (tfra_tier_find_combine_backprop_weights: the cache's row, else the lower table's), nothing moves.  Under
    `can_lookup_combined()`'s conditions."""
    t, ids = self._combined_operands(ids, ragged=False)
    return _pooled_reader(t).find_combine_weight_grad(ids, seg, weights, device_ops.COMBINERS[combiner], grad_out, t._default_value)

  def lookup_combined_ragged_weight_grad(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None, name=None):
    """`lookup_combined_weight_grad` for `lookup_combined_ragged` (tfra_table_find_combine_ragged_backprop_weights): bit-identical to
    it on the row ids the splits stand for, in one launch.  prune: the entries the forward prunes get exactly 0; fill_id: the
    entries of a row that takes the fill row get 0.  A tiered shard is read in both tiers
    (tfra_tier_find_combine_ragged_backprop_weights).  Under `can_lookup_combined()`'s conditions."""
    t, ids = self._combined_operands(ids, ragged=True)
    return _pooled_reader(t).find_combine_ragged_weight_grad(row_splits, ids, weights, device_ops.COMBINERS[combiner], grad_out,
                                                             prune=prune, fill_id=fill_id, default_row=t._default_value)

  def lookup_combined_weight_grad_typed(self, ids, seg, weights, combiner, grad_out, grad_scale=None, name=None):
    """`lookup_combined_weight_grad` that takes grad_out as a half model's dense part hands it back: a contiguous float16 /
    bfloat16 grad_out and grad_scale (a one-element float32 device tensor the gradient is multiplied by) go down as they are
    (tfra_table_find_combine_backprop_weights_typed; a tiered shard: tfra_tier_find_combine_backprop_weights_typed), bit for bit
    the result for grad_out.float() * grad_scale.  Every other grad_out is up-cast, multiplied in torch where a scale is given,
    and takes `lookup_combined_weight_grad`'s call.  (A method beside it, whose parameter list stays as it is.)"""
    t, ids = self._combined_operands(ids, ragged=False)
    return _pooled_reader(t).find_combine_weight_grad_typed(ids, seg, weights, device_ops.COMBINERS[combiner], grad_out,
                                                            t._default_value, grad_scale=grad_scale)

  def lookup_combined_ragged_weight_grad_typed(self, row_splits, ids, weights, combiner, grad_out, prune=False, fill_id=None,
                                               grad_scale=None, name=None):
    """`lookup_combined_ragged_weight_grad` with grad_out and grad_scale as `lookup_combined_weight_grad_typed` takes them
    (tfra_table_find_combine_ragged_backprop_weights_typed; a tiered shard: the tier's typed call)."""
    t, ids = self._combined_operands(ids, ragged=True)
    return _pooled_reader(t).find_combine_ragged_weight_grad_typed(row_splits, ids, weights, device_ops.COMBINERS[combiner], grad_out,
                                                                   prune=prune, fill_id=fill_id, default_row=t._default_value,
                                                                   grad_scale=grad_scale)

  def export(self, name=None):
    """PY/dynamic_embedding_variable.py:988-1007"""
    ks, vs = [], []
    for t in self._tables:
      k, v = t.export()
      ks.append(k.to(self._primary))
      vs.append(v.to(self._primary))
    return torch.cat(ks, 0), torch.cat(vs, 0)

  def size(self, index=None, name=None):
    """PY/dynamic_embedding_variable.py:1133-1155"""
    if index is not None:
      return self._tables[index].size()
    return torch.stack([t.size().to(self._primary) for t in self._tables]).sum()

  # ---- score-filtered forms (tables with per-key scores: HkvHashTable shards) -----------------
  def _scored_tables(self, what):
    """The shards, once every one of them is known to keep scores; NotImplementedError (before any table is touched) when not."""
    for t in self._tables:
      if not hasattr(t, "export_if"):
        raise NotImplementedError("%s needs per-key scores; %s tables have evict strategy NONE (use an HkvHashTableCreator)"
                                  % (what, type(t).__name__))
    return self._tables

  def export_if(self, threshold, pred="ge", name=None):
    """(keys, values, scores) of every shard's entries whose score matches, concatenated as export does."""
    _score_filter(threshold, pred)
    ks, vs, ss = [], [], []
    for t in self._scored_tables("export_if"):
      k, v, s = t.export_if(threshold, pred)
      ks.append(k.to(self._primary))
      vs.append(v.to(self._primary))
      ss.append(s.to(self._primary))
    return torch.cat(ks, 0), torch.cat(vs, 0), torch.cat(ss, 0)

  def remove_if(self, threshold, pred="lt", name=None):
    """Erases the matching entries of every shard; their total number (device int64 scalar, as size)."""
    _score_filter(threshold, pred)
    return torch.stack([t.remove_if(threshold, pred).to(self._primary) for t in self._scored_tables("remove_if")]).sum()

  def size_if(self, threshold, pred="ge", name=None):
    _score_filter(threshold, pred)
    return torch.stack([t.size_if(threshold, pred).to(self._primary) for t in self._scored_tables("size_if")]).sum()

  def save_delta(self, dirpath, threshold, pred="ge", proc_size=1, proc_rank=0, buffer_size=4194304, append_to_file=False):
    """save_to_file_system's per-shard embedding files for the matching entries only; returns the number of entries written.
    The files have save_to_file_system's names and format.  To restore, load the base and then each shard's delta with the
    device table's `load` (it does not clear; load_from_file_system does).  The optimizer's state vectors are not part of a
    delta."""
    _score_filter(threshold, pred)
    suffix = "_rank{}_size{}".format(proc_rank, proc_size) if proc_size > 1 else ""
    total = 0
    for idx, t in enumerate(self._scored_tables("save_delta")):
      total += t.save_delta_to_file_system(dirpath, threshold, pred, file_name=self._make_name(idx) + suffix, dirpath_env=None,
                                           append_to_file=append_to_file, buffer_size=buffer_size)
    return total

  def _slot_file_names(self, optimizer):
    """{field: base file name} of the co-located state vectors.  With the optimizer: the reference's slot-variable
    names `<param>/<opt>/<slot>` (create_slots, PY/dynamic_embedding_optimizer.py:870-904; each is a table of its own
    there and is checkpointed as `<param>_<opt>_<slot>_mht_<i>of<N>`), else `<param>_slot<f>`."""
    if optimizer is not None:
      return {v.field: v.name.replace("/", "_") for v in self.get_slot_variables(optimizer)}
    return {f: "%s_slot%d" % (self.name.replace("/", "_"), f) for f in range(1, self.aux_fields + 1)}

  def save_to_file_system(self, dirpath, proc_size=1, proc_rank=0, buffer_size=4194304, optimizer=None):
    """Per-shard files `<name>_mht_<i>of<N>[_rank<r>_size<s>]-keys/-values`
    (PY/dynamic_embedding_variable.py:1009-1060) — and the same for every optimizer slot of the rows (the reference
    saves its slot variables as tables of their own; not saving them would silently reset Adam's m / v, Adagrad's and
    FTRL's accumulators on restore).  The optimizer's step count (`DynamicEmbeddingOptimizer.iterations`, Adam's bias
    correction) is the OPTIMIZER's state, not the variable's: the reference keeps it in the Keras optimizer's own
    checkpoint, and so must the caller here (`deo.iterations` is a plain int)."""
    import os
    suffix = "_rank{}_size{}".format(proc_rank, proc_size) if proc_size > 1 else ""
    slots = self._slot_file_names(optimizer)
    for idx, t in enumerate(self._tables):
      t.save_to_file_system(dirpath, file_name=self._make_name(idx) + suffix, dirpath_env=None, buffer_size=buffer_size)
      for f, base in slots.items():
        t._checkpoint_table().save(os.path.join(dirpath, "{}_mht_{}of{}{}".format(base, idx + 1, self.shard_num, suffix)), buffer_size,
                                   field=f)

  def load_from_file_system(self, dirpath, proc_size=1, proc_rank=0, buffer_size=4194304, optimizer=None):
    """Reload; when the shard count changed, every `_mht_` file is re-read and re-partitioned
    through partition_fn (PY/dynamic_embedding_variable.py:200-450, 1062-1131).  Slot files written by
    save_to_file_system are restored into the rows' state vectors after the embedding itself."""
    import os
    import numpy as np
    own = self.name.replace("/", "_") + "_mht_"
    listing = os.listdir(dirpath)
    files = sorted(f[:-len("-keys")] for f in listing if f.endswith("-keys") and f.startswith(own))
    slots = self._slot_file_names(optimizer)

    def slot_files(base):
      return sorted(f[:-len("-keys")] for f in listing if f.endswith("-keys") and f.startswith(base + "_mht_"))

    # The slot files are named after the optimizer's slot variables when an optimizer is passed, `<param>_slot<f>` when not.
    # Saving one way and restoring the other must not silently reset Adam's m / v or FTRL's accumulators: when the expected
    # names are absent, the other scheme is looked for — by EXACT base name only (`<param>_<OptClass>_<slot>` for the known
    # optimizer classes, mapped to the field by slot NAME; or `<param>_slot<f>`), never by prefix: a sibling variable
    # `<param>_2` or `<param>_user` in the same directory is not this variable's state.  State files of this variable that
    # match neither scheme completely are an error, not a skip.
    if self.aux_fields:
      prefix = self.name.replace("/", "_") + "_"
      siblings = {n.replace("/", "_") for n in _VARIABLES if n != self.name}
      missing = [f for f, base in slots.items() if not slot_files(base)]
      if missing:
        generic = {f: prefix + "slot%d" % f for f in slots}
        layouts = {cls: tuple(sl) for cls, sl in _known_slot_layouts().items() if len(sl) == self.aux_fields}
        named = {cls: {i + 1: prefix + cls + "_" + sname for i, sname in enumerate(sl)} for cls, sl in layouts.items()}
        named = {cls: m for cls, m in named.items() if not any(b in siblings for b in m.values())}
        if optimizer is None:
          complete = [cls for cls, m in named.items() if all(slot_files(b) for b in m.values())]
          if len(complete) == 1 and len(missing) == len(slots):
            slots = dict(named[complete[0]])
        else:
          if all(slot_files(generic[f]) for f in missing) and not any(generic[f] in siblings for f in missing):
            for f in missing:
              slots[f] = generic[f]
        still = [f for f, base in slots.items() if not slot_files(base)]
        if still:
          # is there ANY state file that can only be this variable's?  (exact bases of either scheme)
          cands = set(generic.values())
          for m in named.values():
            cands.update(m.values())
          found = sorted(b for b in cands if b not in siblings and slot_files(b))
          if found:
            raise ValueError("load_from_file_system: %r holds optimizer-state files %s of variable %r, but they do not cover slot "
                             "field(s) %s (saved with another optimizer?); pass the optimizer the checkpoint was saved with"
                             % (dirpath, found, self.name, still))

    same = all(self._make_name(i) in files for i in range(self.shard_num)) and len(files) == self.shard_num
    if same and proc_size == 1:
      for idx, t in enumerate(self._tables):
        t.load_from_file_system(dirpath, file_name=self._make_name(idx), dirpath_env=None, buffer_size=buffer_size)
        for f, base in slots.items():
          p = os.path.join(dirpath, "{}_mht_{}of{}".format(base, idx + 1, self.shard_num))
          if os.path.exists(p + "-keys"):
            t._checkpoint_table().load(p, buffer_size, field=f)
      return
    self.clear()
    key_np = np.int32 if self.key_dtype == torch.int32 else np.int64   # the key files hold raw keys of the key dtype
    for fn in files:
      keys = np.fromfile(os.path.join(dirpath, fn + "-keys"), dtype=key_np)
      vals = torch.from_numpy(np.fromfile(os.path.join(dirpath, fn + "-values"), dtype=np.uint8)).view(
          self.value_dtype).reshape(-1, self.dim)
      self.upsert(torch.from_numpy(keys).to(self._primary), vals.to(self._primary))
    for t in self._tables:          # once per shard: the table the state vectors go into holds every embedding row from here on
      t._checkpoint_flush()
    for f, base in slots.items():   # re-sharded restore of the state vectors: through the same partitioner
      for fn in slot_files(base):
        keys = torch.from_numpy(np.fromfile(os.path.join(dirpath, fn + "-keys"), dtype=key_np)).to(self._primary)
        vals = torch.from_numpy(np.fromfile(os.path.join(dirpath, fn + "-values"), dtype=np.uint8)).view(
            self.value_dtype).reshape(-1, self.dim).to(self._primary)
        for t, k, v in self._fan_out(keys, vals)[3]:
          if k.numel():
            t._checkpoint_table().upsert(k, v, field=f)
    for t in self._tables:
      t._checkpoint_loaded()


_VARIABLES = {}


def _known_slot_layouts():
  """{optimizer class name: slot names in field order} of the optimizers this package ships (the `<opt>` and `<slot>` parts of
  the reference's slot-variable names `<param>/<opt>/<slot>`, PY/dynamic_embedding_optimizer.py:870-904)."""
  from . import optimizer as _o
  out = {}
  for cls in (_o.Adam, _o.Adagrad, _o.Ftrl, _o.Momentum, _o.RMSProp):
    sl = cls.slots if cls.slots else cls().slots
    if sl:
      out[cls.__name__] = tuple(sl)
  return out


def get_variable(name, key_dtype=torch.int64, value_dtype=torch.float32, dim=1, devices=None,
                 partitioner=default_partition_fn, shared_name="get_variable", initializer=None, trainable=True,
                 checkpoint=True, init_size=0, kv_creator=None, restrict_policy=None, bp_v2=False, init_on_lookup=False, **kw):
  """PY/dynamic_embedding_variable.py:1265-1359: create-or-reuse by name.  init_on_lookup: see `Variable`."""
  if name in _VARIABLES:
    return _VARIABLES[name]
  v = Variable(key_dtype=key_dtype, value_dtype=value_dtype, dim=dim, devices=devices, partitioner=partitioner,
               shared_name=shared_name, name=name, initializer=initializer, trainable=trainable, checkpoint=checkpoint,
               init_size=init_size, kv_creator=kv_creator, restrict_policy=restrict_policy, bp_v2=bp_v2, init_on_lookup=init_on_lookup, **kw)
  _VARIABLES[name] = v
  return v


PLAN_AT_LOOKUP_MIN_IDS = 8192   # below this the write-back plan is not worth a second stream
PLAN_POOL_MAX = 8


def _plan_at_lookup(params, ids):
  """The id-only half of the optimizer write-back of `ids` (the de-duplication plan, SparsePlan), started on the
  Variable's second stream at LOOKUP time: the ids of a training step are known when it looks them up (the reference
  keeps them in the TrainableWrapper, PY/embedding_weights.py:38-120) and the plan needs nothing else, so it builds while
  the lookup, the model's forward and backward run — no look-ahead into the next batch is needed.  Returns None when
  the write-back of this variable / batch is not the planned one."""
  if not _wants_plan_at_lookup(params, ids):
    return None
  plan = _pool_plan(params)
  if plan is None:
    return None   # more lookups in flight than plans: this one takes the one-call write-back
  pool = params._plan_pool
  if pool["stream"] is None:
    pool["stream"] = torch.cuda.Stream(device=params._primary)
  side = pool["stream"]
  side.wait_stream(torch.cuda.current_stream(params._primary))   # the ids may still be being produced
  with torch.cuda.stream(side):
    plan.build(ids)
  return plan


def _wants_plan_at_lookup(params, ids):
  """Whether the write-back of `ids` into this variable is the planned one and the batch is worth a plan built at lookup time."""
  from .optimizer import DynamicEmbeddingOptimizer
  n = ids.numel()
  return not (n < PLAN_AT_LOOKUP_MIN_IDS or params.bp_v2 or not DynamicEmbeddingOptimizer.can_plan(params, n) or not ids.is_cuda)


_GROUP_PLAN_STREAMS = {}   # device -> the side stream of the grouped lookups' plan builds


def _plans_at_lookup_many(device, members):
  """`_plan_at_lookup` for the grouped members of one device (`members`: [(i, params, entry ids)]): the same eligibility rule per
  variable, a plan from each variable's own pool, and ONE grouped build (`table_ops.build_plans_many`) on ONE side stream of the
  device, which waits for the current stream once — instead of one side stream, one wait and three launches per variable.
  Returns {i: plan} for the members that got a plan, or None when at most one member is eligible: a group of one keeps
  `_plan_at_lookup` on that variable's own stream."""
  want = [m for m in members if _wants_plan_at_lookup(m[1], m[2])]
  if len(want) < 2:
    return None
  got = []
  for i, params, ids in want:
    plan = _pool_plan(params)
    if plan is not None:   # (None: more lookups in flight than plans, this one takes the one-call write-back)
      got.append((i, params, ids, plan))
  if not got:
    return {}
  side = _GROUP_PLAN_STREAMS.get(device)
  if side is None:
    side = _GROUP_PLAN_STREAMS[device] = torch.cuda.Stream(device=device)
  side.wait_stream(torch.cuda.current_stream(device))   # the ids may still be being produced
  try:
    with torch.cuda.stream(side):
      table_ops.build_plans_many([g[3] for g in got], [g[2] for g in got])
  except Exception:
    for _, params, _, plan in got:
      _release_plan(params, plan)
    raise
  return {i: plan for i, _, _, plan in got}


def _pool_plan(params):
  """A free plan of the Variable's pool (a new one while fewer than PLAN_POOL_MAX exist), or None."""
  pool = params.__dict__.setdefault("_plan_pool", {"free": [], "made": 0, "stream": None})
  if pool["free"]:
    return pool["free"].pop()
  if pool["made"] < PLAN_POOL_MAX:
    pool["made"] += 1
    return SparsePlan(params._primary, params.dim)
  return None


def _release_plan(params, plan):
  pool = getattr(params, "_plan_pool", None)
  if pool is not None and plan is not None:
    pool["free"].append(plan)   # (its next build waits for the event of its last use: SparsePlan.build)


def _clip_rows(result, max_norm):
  """clip_by_norm over the embedding axis (None: as it is)"""
  if max_norm is None:
    return result
  norm = result.to(torch.float32).norm(dim=-1, keepdim=True)
  scale = max_norm / torch.maximum(norm, torch.full_like(norm, max_norm))
  return (result * scale).to(result.dtype)


class TrainableWrapper:
  """The local [N,dim] "shadow" of the rows of one lookup (PY/embedding_weights.py:38-540):
  refilled from the table on read (`prefetch_values`), written back by `update_op`."""

  def __init__(self, params, ids, max_norm=None, plan_writeback=False, out_dtype=None):
    """out_dtype: the first read goes through the typed lookup where the route has one (`prefetch_values`)."""
    self.params = params
    self.ids = ids
    self.max_norm = max_norm
    self._out_dtype = out_dtype
    self._values = None
    self.exists = None
    self.plan = _plan_at_lookup(params, ids) if plan_writeback else None
    self.prefetch_values()

  def take_plan(self):
    """The write-back plan started at lookup time (or None); the caller applies it once and hands it back to the pool."""
    plan, self.plan = self.plan, None
    return plan

  def __del__(self):
    try:
      if self.plan is not None:
        _release_plan(self.params, self.take_plan())
    except Exception:
      pass

  _ids_are_unique = False   # (SparseTrainableWrapper: its ids are tf.unique's output already)

  def prefetch_values(self):
    """PY/embedding_weights.py:163-170.  An init_on_lookup variable (not bp_v2) admits here: `_lookup_admitting`."""
    if self.params.bp_v2:
      r, self.exists = self.params.lookup(self.ids, return_exists=True)
    elif self.params.admits_on_lookup() and self.ids.numel():
      r = self._lookup_admitting()
    else:
      # (the typed lookup, embedding_lookup's out_dtype: only this route has one, and only unclipped — max_norm clips the value
      # dtype's rows, bp_v2 keeps them for accum, an admitting lookup returns what it inserts; those are converted by the caller)
      typed = self.__dict__.get("_out_dtype") if self.max_norm is None else None
      r = self.params.lookup(self.ids) if typed is None else self.params.lookup(self.ids, out_dtype=typed)
    self._values = self.transform(r)
    return self._values

  def _lookup_admitting(self):
    """The lookup of an init_on_lookup variable: the ids de-duplicated on the device in first-occurrence order (tfra_unique — a
    seeded initializer then fills the table reproducibly), ONE draw initializer([n, dim]) whose row j belongs to unique id j,
    find_or_insert over the unique buffer with the count left on the device, and the rows gathered back through the inverse
    index: every position of an id sees one row, and the table holds it.  No host read.  (Several shards: the unique ids are
    trimmed with one host read and go through `Variable.lookup_or_insert`.)
    init_on_lookup="plan" (one shard that is not tiered, ids that may repeat, a plan to be had: `_plan_for_lookup`): no unique and no gather — the
    ids go through their write-back plan (find_or_insert_planned), row p of the one draw belongs to batch position p and an id
    that is not resident takes the row of its last position."""
    params, ids = self.params, self.ids
    if params.shard_num == 1:
      t = params._tables[0]
      planned = params.init_on_lookup == "plan" and not self._ids_are_unique and not _has_tiered_shards(params)   # (a tier: the True route — DESIGN 4.26)
      plan = self._plan_for_lookup() if planned else None
      init = params._create_default_values_by_initializer(ids.numel(), t._device)
      if plan is not None:
        return t.find_or_insert_planned(plan, dynamic_default_values=init)
      if self._ids_are_unique:
        return t.find_or_insert(ids.to(t._device), dynamic_default_values=init)
      uniq, idx, cnt = device_ops.unique_no_sync(ids.to(t._device))
      rows = t.find_or_insert(uniq, dynamic_default_values=init, count=cnt)
      return device_ops.gather_rows(rows, idx)   # (idx < count everywhere: rows beyond the count are never read)
    if self._ids_are_unique:
      return params.lookup_or_insert(ids)
    uniq, idx, _ = device_ops.unique(ids)
    return device_ops.gather_rows(params.lookup_or_insert(uniq), idx)

  def _plan_for_lookup(self):
    """init_on_lookup="plan": the write-back plan of this wrapper's ids, to look them up through — the one `plan_writeback` started
    (on its side stream; the lookup waits for it), else one built now on the CURRENT stream, because the lookup depends on it.
    It stays `self.plan`, so `apply_gradients` takes it (`take_plan`).  None: the write-back of this batch is not the planned one,
    or no plan is free — the caller takes the unique + find_or_insert + gather route."""
    from .optimizer import DynamicEmbeddingOptimizer
    if self.plan is None:
      params, ids = self.params, self.ids
      if not ids.is_cuda or not DynamicEmbeddingOptimizer.can_plan(params, ids.numel()):
        return None
      plan = _pool_plan(params)
      if plan is None:
        return None
      try:
        plan.build(ids)
      except Exception:
        _release_plan(params, plan)
        raise
      self.plan = plan
    return self.plan

  def transform(self, result):
    """PY/embedding_weights.py:497-521: optional clip_by_norm over the embedding axis."""
    return _clip_rows(result, self.max_norm)

  def read_value(self):
    return self._values

  def update_op(self, new_values, old_values=None):
    """PY/embedding_weights.py:434-444: upsert (or accum when bp_v2) the post-optimizer rows."""
    if self.params.bp_v2:
      old = self._values if old_values is None else old_values
      self.params.accum(self.ids, old, new_values, self.exists)
    else:
      self.params.upsert(self.ids, new_values)
    if self.params.restrict_policy is not None:  # PY/embedding_weights.py:441-442
      self.params.restrict_policy.apply_update(self.ids)
    self._values = new_values


class SparseTrainableWrapper(TrainableWrapper):
  """The TrainableWrapper of an embedding_lookup_sparse / safe_embedding_lookup_sparse.  `ids` (the lookup's unique ids),
  `read_value`, `update_op` and `apply_gradients` with a [n_unique, dim] gradient are those of TrainableWrapper; it also
  keeps what the combiner's backward needs — the entry ids, their rows (`seg`, ascending), weights, the combiner, the
  number of rows and the shape of the result — so that the gradient of the RESULT can be applied
  (`DynamicEmbeddingOptimizer.apply_combined_gradients`) or turned into the rows' gradient (`grad_of`).

  The entry list follows the reference's safe_embedding_lookup_sparse (PY/dynamic_embedding_ops.py:374-408): entries pruned
  for their weight are not in it, and every row left empty adds one entry (row, default_id or 0, weight 1) — with
  default_id=None that entry's gradient is zero (the reference's `where`), but its key still reaches the write-back.

  A wrapper made behind the pooled forward (`lookup_ids`: the lookup's ids as given, instead of `ids` / `idx` / `n_unique`) has
  not de-duplicated anything yet: `ids`, `_idx`, `_n_unique`, `exists` and the rows behind `read_value()` are resolved on their
  first access — tf.unique of the lookup's ids and a lookup of the unique ids, as the eager wrapper does at construction (the
  rows are then those the table holds at that moment).  `apply_combined_gradients` needs none of them.

  `weights_grad` is the gradient of the result with respect to the caller's sp_weights; for it the wrapper keeps the lookup's ids
  as given (`_pooled_ids`, a reference that survives the lazy resolution) and, behind a safe lookup that pruned by weight, the
  caller's weights (`_caller_weights`: `_note_pruned`), from which the pruned positions are found when the gradient is asked for."""

  _LAZY = ("ids", "_idx", "_n_unique", "exists", "_values")
  _ids_are_unique = True

  def __init__(self, params, ids, idx, n_unique, seg, weights, combiner, n_rows, out_shape, entry_ids, entry_seg,
               entry_weights, max_norm=None, plan_writeback=False, lookup_ids=None, entry_plan=None):
    """entry_plan: a plan over `entry_ids` whose build is already enqueued (the grouped lookup starts its members' plans in one
    call); the wrapper owns it from here on, as one made with plan_writeback."""
    if lookup_ids is None:
      super().__init__(params, ids, max_norm=max_norm)
      self._idx, self._n_unique = idx, n_unique
    else:
      self.params, self.max_norm, self.plan = params, max_norm, None
    self._lookup_ids = self._pooled_ids = lookup_ids
    self._caller_weights = None
    self.combiner = combiner
    self.n_rows = int(n_rows)
    self.out_shape = tuple(out_shape)
    self._seg, self._weights = seg, weights   # the lookup's own entries (grad_of)
    self.entry_ids, self.seg, self.weights = entry_ids, entry_seg, entry_weights
    self.entry_plan = entry_plan if entry_plan is not None else (_plan_at_lookup(params, entry_ids) if plan_writeback else None)

  def __getattr__(self, name):   # only reached for attributes not set yet
    if name in SparseTrainableWrapper._LAZY and self.__dict__.get("_lookup_ids") is not None:
      uniq, self._idx, self._n_unique = device_ops.unique(self._lookup_ids)
      self._lookup_ids, self.ids, self._values, self.exists = None, uniq.reshape(-1), None, None
      self.prefetch_values()
      return self.__dict__[name]
    raise AttributeError("%s has no attribute %r" % (type(self).__name__, name))

  def take_entry_plan(self):
    """The write-back plan over the entry ids started at lookup time (or None); handed back to the pool after its use."""
    plan, self.entry_plan = self.entry_plan, None
    return plan

  def __del__(self):
    try:
      if self.entry_plan is not None:
        _release_plan(self.params, self.take_entry_plan())
    except Exception:
      pass
    super().__del__()

  def check_grad_out(self, grad_out, keep_half=False):
    """grad_out as [n_rows, dim] float32; ValueError unless it has the shape of the lookup's result.  keep_half: a float16 /
    bfloat16 gradient keeps its dtype (for the typed combined write-back): the same check, reshaped, and no copy in another dtype."""
    grad_out = torch.as_tensor(grad_out, device=self.params._primary)
    if tuple(grad_out.shape) != self.out_shape:
      raise ValueError("the gradient of a sparse lookup must have the shape of its result %s, got %s" %
                       (list(self.out_shape), list(grad_out.shape)))
    if keep_half and grad_out.dtype in (torch.float16, torch.bfloat16):
      return grad_out.reshape(self.n_rows, self.params.dim)
    return grad_out.reshape(self.n_rows, self.params.dim).to(torch.float32).contiguous()

  def grad_of(self, grad_out):
    """The gradient with respect to the trainable's rows, [n_unique, dim] in the order of `ids`, from the gradient of the
    lookup's result: the combiner's backward of every looked-up entry, summed per unique id (no host sync).  (Entries that
    safe_embedding_lookup_sparse adds for empty rows are not rows of this lookup; apply_combined_gradients writes them.)"""
    g = self.check_grad_out(grad_out)
    eg = device_ops.sparse_segment_combine_backprop(g, self._seg, self._weights, self.combiner)
    n = self.ids.numel()
    return device_ops.segment_sum(eg, self._idx, self._n_unique, n)


  def weights_grad(self, grad_out, grad_scale=None):
    """The gradient of the lookup's result with respect to the VALUES of the sp_weights the caller passed: float32, the caller's
    length and order, from grad_out = d loss / d result (the result's shape).  Entries the safe form pruned get 0; the entries
    it adds for empty rows are not the caller's and do not appear; a row that took `default_id` contributes nothing.
    The table's rows are read AS THEY ARE AT CALL TIME: call it before the step's write-back (`apply_combined_gradients`), or
    the gradient is that of the updated rows.
    A variable the pooled forward serves, tiered or not, is read straight from the table (`Variable.lookup_combined_weight_grad`:
    no [nnz, dim] rows; a tier is read in both tables); every other one — several shards, a callable initializer, bp_v2, other
    dims or dtypes — goes through a lookup of the unique ids and `device_ops.sparse_segment_combine_weight_grad`.  The two routes
    give the same bits for the same rows.
    Nothing is read on the host on the pooled route, pruned or not (the pruned positions are filled by a masked scatter).
    A float16 / bfloat16 grad_out and grad_scale (a one-element float32 device tensor, as in `apply_combined_gradients`) go down
    as they are on both routes (tfra_table_find_combine_backprop_weights_typed, a tier's typed call, or
    tfra_sparse_segment_combine_backprop_weights_typed): the SAME half gradient serves the write-back and this call with no
    conversion pass.  Every other gradient — float32, or a half one that is not contiguous — is read as its float32 up-cast times
    the scale, by the typed calls' definition the same bits.  No host read either way.
    ValueError for a lookup made without sp_weights, with max_norm (the clip's own gradient is not formed, as in
    `apply_combined_gradients`), or for a grad_out of another shape."""
    if self.max_norm is not None:
      raise ValueError("weights_grad does not support max_norm: the clip's gradient is not formed")
    if self._weights is None:
      raise ValueError("weights_grad needs a lookup made with sp_weights")
    g = self.check_grad_out(grad_out, keep_half=True)
    if self._pooled_ids is not None and _pooled_training(self.params, None):
      if g.dtype == torch.float32 and grad_scale is None:   # the method it always took
        dw = self.params.lookup_combined_weight_grad(self._pooled_ids, self._seg, self._weights, self.combiner, g)
      else:
        dw = self.params.lookup_combined_weight_grad_typed(self._pooled_ids, self._seg, self._weights, self.combiner, g,
                                                           grad_scale=grad_scale)
    else:
      rows = self.params.lookup(self.ids).to(torch.float32)
      dw = device_ops.sparse_segment_combine_weight_grad(rows, self._idx, g, self._seg, self._weights, self.combiner,
                                                         grad_scale=grad_scale)
    if self._caller_weights is None:
      return dw
    cw = torch.as_tensor(self._caller_weights, dtype=torch.float32, device=dw.device).reshape(-1)
    # dw holds one value per kept entry, in order: `_safe_sparse_args` kept exactly the entries with weight > 0.  masked_scatter_
    # fills the kept positions from dw in order, on the device (no host read, unlike a boolean-mask assignment)
    return torch.zeros(cw.numel(), dtype=torch.float32, device=dw.device).masked_scatter_(cw > 0, dw)


def sparse_weights_grad_many(grads_and_wrappers, grad_scale=None):
  """`SparseTrainableWrapper.weights_grad` of a LIST of lookups (a many-table model's weighted sparse features):
  `grads_and_wrappers` is a list of (grad_out, wrapper), and result i is what `wrapper.weights_grad(grad_out)` returns, bit for
  bit and in the caller's length.  The wrappers on the pooled route — made behind the pooled forward, of a variable it still
  serves (`_pooled_forward`), tiered or not — are read by ONE grouped call per device
  (`table_ops.find_combine_weight_grad_many`: tfra_multi_find_combine_backprop_weights, whose launch count does not grow with the
  list); what a safe lookup pruned is filled in per member afterwards, as `weights_grad` fills it.  Every other wrapper — several
  shards, a callable initializer, bp_v2, other dims or dtypes — is served by its own `weights_grad`, so no list is refused.
  The ValueErrors are `weights_grad`'s (no sp_weights, max_norm, a grad_out of another shape), raised for the whole list before
  anything is enqueued.  As there, the tables' rows are read as they are at call time: call it before the step's write-back.
  Half gradients and grad_scale as in `weights_grad`: a group with a half member is ONE
  tfra_multi_find_combine_backprop_weights_typed call (float32 members ride along); a group without one takes the untyped call."""
  pairs = list(grads_and_wrappers)
  checked = []
  for grad_out, tw in pairs:
    if tw.max_norm is not None:
      raise ValueError("weights_grad does not support max_norm: the clip's gradient is not formed")
    if tw._weights is None:
      raise ValueError("weights_grad needs a lookup made with sp_weights")
    checked.append(tw.check_grad_out(grad_out, keep_half=True))
  results = [None] * len(pairs)
  groups = {}   # device -> [i]
  for i, (grad_out, tw) in enumerate(pairs):
    if tw._pooled_ids is not None and _pooled_training(tw.params, None):
      groups.setdefault(tw.params._primary, []).append(i)
    else:
      results[i] = tw.weights_grad(grad_out, grad_scale=grad_scale)
  for members in groups.values():
    reqs = []
    for i in members:
      tw = pairs[i][1]
      t, ids = tw.params._combined_operands(tw._pooled_ids, ragged=False)
      reqs.append((_pooled_reader(t), ids, tw._seg, tw._weights, device_ops.COMBINERS[tw.combiner], checked[i], t._default_value))
    for i, dw in zip(members, table_ops.find_combine_weight_grad_many(reqs, grad_scale=grad_scale)):
      cw = pairs[i][1]._caller_weights
      if cw is not None:   # (weights_grad: the kept positions are filled from dw in order, on the device)
        cw = torch.as_tensor(cw, dtype=torch.float32, device=dw.device).reshape(-1)
        dw = torch.zeros(cw.numel(), dtype=torch.float32, device=dw.device).masked_scatter_(cw > 0, dw)
      results[i] = dw
  return results


def _note_pruned(tw, sparse_weights, combiner):
  """Behind a safe lookup: the wrapper remembers the caller's weights when entries were pruned by them (weights given and the
  combiner not "sum": `_safe_sparse_args`), so that `weights_grad` can answer in the caller's length and order.  A reference
  only: constructing the wrapper stays as cheap as it is."""
  if tw is not None and sparse_weights is not None and combiner != "sum":
    tw._caller_weights = sparse_weights
  return tw


def _as_out_dtype(result, out_dtype):
  """A lookup's result in the caller's out_dtype (None: as it is): the conversion of the routes that have no typed lookup."""
  return result if out_dtype is None or result.dtype == out_dtype else result.to(out_dtype)


def embedding_lookup(params, ids, partition_strategy=None, name=None, validate_indices=None, max_norm=None,
                     return_trainable=False, plan_writeback=False, out_dtype=None):
  """PY/dynamic_embedding_variable.py:1362-1530.  A miss returns the initializer row and does NOT
  insert (keys enter the table on the optimizer write-back).

  plan_writeback (with return_trainable): start the id-only half of the optimizer write-back of these ids now, on the
  Variable's second stream, so that it builds while the model's forward and backward run and `apply_gradients` finds it
  ready (no look-ahead into the next batch needed).  Opt-in: it pays when there is work between lookup and
  apply_gradients; back to back (bench shape, 131 072 ids) the extra Python — a stream context and three events — costs
  more than the overlap gains: 96 us per step against 75 us for lookup + one-call apply_sparse.

  out_dtype: the embeddings in float32 / float16 / bfloat16 instead of the value dtype (a bfloat16 model over a float32 table),
  bit for bit `embedding_lookup(...).to(out_dtype)`.  The plain lookup converts in its kernel (`Variable.lookup`); max_norm, bp_v2
  and an admitting lookup (init_on_lookup) run as they do and their result is converted.  The wrapper, its plan and the
  write-back are today's: the typed write-backs take the half gradient that comes back."""
  ids = torch.as_tensor(ids, device=params._primary)
  tw = TrainableWrapper(params, ids.reshape(-1), max_norm=max_norm, plan_writeback=return_trainable and plan_writeback,
                        out_dtype=_out_dtype(out_dtype))
  emb = _as_out_dtype(tw.read_value(), out_dtype).reshape(tuple(ids.shape) + (params.dim,))
  return (emb, tw) if return_trainable else emb


def embedding_lookup_unique(params, ids, partition_strategy=None, name=None, validate_indices=None, max_norm=None,
                            return_trainable=False, out_dtype=None):
  """PY/dynamic_embedding_ops.py:64-117: unique -> lookup -> gather.  out_dtype: `embedding_lookup`'s, on the unique rows (the
  gather copies them)."""
  ids = torch.as_tensor(ids, device=params._primary)
  uniq, idx, _ = device_ops.unique(ids)
  r = embedding_lookup(params, uniq, max_norm=max_norm, return_trainable=return_trainable, out_dtype=out_dtype)
  ue, tw = r if return_trainable else (r, None)
  emb = device_ops.gather_rows(ue, idx).reshape(tuple(ids.shape) + (params.dim,))
  return (emb, tw) if return_trainable else emb


def _pooled_forward(params, max_norm):
  """Whether embedding_lookup_sparse reads through `Variable.lookup_combined`: the variable qualifies, nothing is clipped
  (max_norm acts on the unique rows) and the wrapper needs no `exists` at lookup time (bp_v2)."""
  return max_norm is None and not params.bp_v2 and params.can_lookup_combined()


def _read_rows(params, ids, max_norm):
  """The rows of `ids` for a sparse lookup that is NOT a training step's (and for the safe form's default_id row): `embedding_lookup`
  as it is — which, through its wrapper, admits for an init_on_lookup variable —, but for init_on_lookup="pooled" a read that
  inserts nothing: a miss is drawn and stays out (the setting's training lookups have admitted what the write-back will touch)."""
  if params.init_on_lookup == "pooled":
    return _clip_rows(params.lookup(ids), max_norm)
  return embedding_lookup(params, ids, max_norm=max_norm)


def _pooled_training(params, max_norm):
  """`_pooled_forward` for the TRAINING forms (return_trainable) and what reads through their wrappers: also a variable that
  reaches the pooled read by admitting its entry ids with drawn rows first (init_on_lookup="pooled": `Variable.can_admit_pooled`).
  The one predicate of every training call site."""
  return _pooled_forward(params, max_norm) or (max_norm is None and not params.bp_v2 and params.can_admit_pooled())


def embedding_lookup_sparse(params, sp_ids, sp_weights=None, partition_strategy=None, name="embedding_lookup_sparse",
                            combiner="mean", max_norm=None, return_trainable=False, num_rows=None, plan_writeback=False,
                            _entries=None, _out_shape=None, out_dtype=None):
  """PY/dynamic_embedding_ops.py:120-293.  `sp_ids` = (indices[nnz,2] or row_ids[nnz], values[nnz]);
  `sp_weights` = matching weight values or None.  Segment combine sum / mean / sqrtn over rows.

  return_trainable: also returns a SparseTrainableWrapper; `DynamicEmbeddingOptimizer.apply_combined_gradients` applies the
  gradient of the result through it.  plan_writeback (with return_trainable): build the write-back plan over the entry ids
  at lookup time, on the Variable's second stream (as embedding_lookup's plan_writeback).

  out_dtype: the result in float32 / float16 / bfloat16, bit for bit `embedding_lookup_sparse(...).to(out_dtype)`: the pooled
  read rounds in its kernel (`Variable.lookup_combined`), the op chain's float32 result is converted.  The wrapper is today's."""
  _check_combiner(combiner)
  _out_dtype(out_dtype)
  indices, ids = sp_ids
  indices = torch.as_tensor(indices, device=params._primary)
  seg = (indices[:, 0] if indices.dim() == 2 else indices).to(torch.int64)
  ids = torch.as_tensor(ids, device=params._primary)
  w = sp_weights if sp_weights is None else torch.as_tensor(sp_weights, dtype=torch.float32, device=params._primary)
  pooled = _pooled_training(params, max_norm) if return_trainable else _pooled_forward(params, max_norm)
  if not pooled:
    uniq, idx, cnt = device_ops.unique(ids)
  n = int(seg.max().item()) + 1 if num_rows is None else num_rows
  if return_trainable:
    e_ids, e_seg, e_w = _entries if _entries is not None else (ids.reshape(-1), seg, w)   # ids keep their key dtype
    shape = _out_shape if _out_shape is not None else (n, params.dim)
  if pooled:
    # the pooled read: one probe + row read per entry, combined in registers — no unique pass, no [U, dim] rows, no host read of
    # a count (the result is bit-identical to the chain below).  Over tiered shards a training step first brings its entry ids
    # into the cache (`Variable.admit_entries`), and the read sees both tiers either way; an init_on_lookup="pooled" variable
    # admits them with drawn rows there, which is what lets it read here at all
    if return_trainable:
      params.admit_entries(e_ids)
    out = params.lookup_combined(ids, seg, w, combiner, n) if out_dtype is None else params.lookup_combined(
        ids, seg, w, combiner, n, out_dtype=out_dtype)
    if not return_trainable:
      return out
    return out, SparseTrainableWrapper(params, None, None, None, seg, w, combiner, n, shape, e_ids, e_seg, e_w, max_norm=max_norm,
                                       plan_writeback=plan_writeback, lookup_ids=ids)
  if return_trainable:
    tw = SparseTrainableWrapper(params, uniq.reshape(-1), idx, cnt, seg, w, combiner, n, shape, e_ids, e_seg, e_w,
                                max_norm=max_norm, plan_writeback=plan_writeback)
    ue = tw.read_value()
  else:
    tw = None
    ue = _read_rows(params, uniq, max_norm)
  # gather + weights + segment combine fused in one kernel (reads the unique rows through idx)
  out = _as_out_dtype(device_ops.sparse_segment_combine(ue, idx, seg, w, combiner, n), out_dtype)
  return (out, tw) if return_trainable else out


def _per_table(value, n, what):
  """`value` as a list of n: a scalar is repeated, a list / tuple must have n entries."""
  if isinstance(value, (list, tuple)):
    if len(value) != n:
      raise ValueError("%s: %d entries for %d tables" % (what, len(value), n))
    return list(value)
  return [value] * n


def _check_combiner(combiner):
  if combiner not in ("mean", "sqrtn", "sum"):
    raise ValueError("combiner must be one of 'mean', 'sqrtn' or 'sum'")


def _rows_in_one_read(rows, unknown):
  """rows[i] = the highest row id + 1 for every (i, row ids) of `unknown` — members of one device, each with at least one entry —
  from one host read for all of them."""
  if unknown:
    for (i, _), top in zip(unknown, torch.stack([r.max() for _, r in unknown]).tolist()):
      rows[i] = int(top) + 1


def _check_entries_many(members):
  """At the head of a grouped training lookup, for its pooled `members` [(variable, entry ids)]: the max_batch ValueError of
  `Variable.admit_entries` for ALL tiered members before the first admission is enqueued — a refused list has admitted and read
  nothing."""
  for params, entry_ids in members:
    params._admissible_entries(entry_ids)


# The shortest list of distinct tiers that `_admit_entries_many` admits with the grouped call.  One tier alone is slower grouped
# (37.2 against 29.6 us); two are faster grouped there (44.5 against 54.1 us), but a list of two keeps one
# tfra_tier_find_or_insert per member, which tests/test_gpu_tier_pooled_many.py holds: the chain that grows with the list is what
# the grouped call is for, and from three tiers on it takes it.
ADMIT_MANY_MIN_TIERS = 3
# The same for the plain init_on_lookup="pooled" members and tfra_multi_find_or_insert, measured: with no never-seen
# id in the batch three tables are level (19.2 against 19.9 us, inside the spreads) and four are the first list the grouped call wins
# beyond the sum of both spreads (25.5 against 23.1 us); with a tenth never seen it is ahead from two on.
ADMIT_MANY_MIN_TABLES = 4


def _admit_entries_many(params_list, entry_ids):
  """Ahead of the ONE grouped read of a training step: `Variable.admit_entries(entry_ids[i])` for every member i of `entry_ids`
  (index -> the entry ids its wrapper will write back; a member that is neither tiered nor init_on_lookup="pooled": nothing).
  Admission moves rows between the tiers and never changes them, so the one read behind all admissions returns what a read behind
  each would.  The members (of one device) whose tiers are distinct are admitted by ONE grouped call (`table_ops.admit_many`:
  tfra_multi_tier_find_or_insert, whose launch count does not grow with the list) when there are ADMIT_MANY_MIN_TIERS of them or
  more, each member's entry ids de-duplicated on the device first as `admit_entries` does — for all members of the grouped
  admissions, tiered and plain, by ONE grouped call (`device_ops.unique_many`: tfra_multi_unique) —; a tier that stands in the list again
  has its later occurrences admitted by the single call behind the grouped one — the order of the loop of single calls.  A
  shorter list keeps the loop of `admit_entries`.
  The plain (not tiered) init_on_lookup="pooled" members go the same way through `table_ops.table_admit_many`
  (tfra_multi_find_or_insert) from ADMIT_MANY_MIN_TABLES distinct tables on, each with its own draw (`Variable._admission_rows`);
  the draws are made in the list's order whichever call admits them."""
  first, later, seen = {True: [], False: []}, [], set()   # tiered -> [(params, flat)]
  for i, ids in entry_ids.items():
    params = params_list[i]
    flat = params._admissible_entries(ids)
    if flat is None or not flat.numel():
      continue
    tiered = _has_tiered_shards(params)
    owner = params._tables[0]._tier if tiered else params._tables[0]._table
    (later if id(owner) in seen else first[tiered]).append((params, flat))
    seen.add(id(owner))
  kinds = ((True, ADMIT_MANY_MIN_TIERS, table_ops.admit_many), (False, ADMIT_MANY_MIN_TABLES, table_ops.table_admit_many))
  # the unique ids of ALL members that take a grouped admission, tiered and plain together: one grouped de-duplication
  # (tfra_multi_unique; admission has no use for the inverse index) ahead of both admissions
  grouped = [flat for tiered, least, _ in kinds if len(first[tiered]) >= least for _, flat in first[tiered]]
  uniques = iter(device_ops.unique_many(grouped, want_idx=False))
  for tiered, least, many in kinds:
    if len(first[tiered]) < least:
      for params, flat in first[tiered]:
        params.admit_entries(flat)
      continue
    reqs = []
    for params, flat in first[tiered]:
      t = params._tables[0]
      uniq, _, cnt = next(uniques)
      if tiered:
        reqs.append((t, uniq, params._admission_rows(flat.numel()), cnt))
      else:   # (the scores `admit` of the shard would pass: `_gen_scores`)
        reqs.append((t, uniq, params._admission_rows(flat.numel()), cnt, t._gen_scores(uniq)))
    many(reqs)
  for params, flat in later:
    params.admit_entries(flat)


def _wrap_grouped(device, params_list, members, outs, entry_ids, plan_writeback, wrapper, results):
  """results[i] = (out, SparseTrainableWrapper) behind a grouped forward, for the members (i, ...) of `device` and their `outs`.
  The members' write-back plans over entry_ids[i]: one grouped build on one side stream (None: at most one member takes a plan,
  and its wrapper starts it as the single lookup does: own_plan).  `wrapper(member, own_plan, entry_plan)` makes the wrapper."""
  started = _plans_at_lookup_many(device, [(m[0], params_list[m[0]], entry_ids[m[0]]) for m in members]) if plan_writeback else None
  for m, out in zip(members, outs):
    results[m[0]] = (out, wrapper(m, plan_writeback and started is None, None if started is None else started.get(m[0])))


def embedding_lookup_sparse_many(params_list, sp_ids_list, sp_weights_list=None, combiner="mean", max_norm=None,
                                 return_trainable=False, num_rows=None, plan_writeback=False, _entries_list=None,
                                 _out_shapes=None, out_dtype=None):
  """`embedding_lookup_sparse` of a LIST of variables (a many-table model's sparse features): result i is what
  `embedding_lookup_sparse(params_list[i], sp_ids_list[i], sp_weights_list[i], ...)` returns, bit for bit — with return_trainable
  the (result, SparseTrainableWrapper) pair, the wrapper built behind the pooled forward.  `combiner` and `num_rows` are scalars
  or per-table lists.  The variables the pooled forward serves (`_pooled_forward`) are read by ONE grouped call per device
  (`table_ops.find_combine_many`: tfra_multi_find_combine, whose launch count does not grow with the list) — a tiered variable
  among them: it joins its device's group with the shard itself as owner (`_pooled_reader`), the group then goes through
  tfra_multi_tier_find_combine and the member is read in both tiers; with return_trainable its entry ids are admitted into the
  cache first (`_admit_entries_many`: ONE grouped admission of the device's tiered members from three on, then the one read) —; every other variable
  takes `embedding_lookup_sparse` as it is, so no list is refused.  With return_trainable and plan_writeback the grouped members
  that a single lookup would give a plan (`_plan_at_lookup`'s rule, per variable) get theirs from ONE grouped build per device on
  one side stream (`_plans_at_lookup_many`: tfra_multi_sparse_plan_build).  Where num_rows is absent, the grouped variables' row counts
  come from one host read per device, not one per table.  out_dtype: one of float32 / float16 / bfloat16 for every result, as the
  single form's: a group of plain tables is rounded in the grouped call's kernels (tfra_multi_find_combine_typed, the same launch
  count), a group with a tiered member and every single-form member are converted."""
  _out_dtype(out_dtype)
  n_t = len(params_list)
  if len(sp_ids_list) != n_t:
    raise ValueError("sp_ids_list: %d entries for %d tables" % (len(sp_ids_list), n_t))
  weights = _per_table(None if sp_weights_list is None else list(sp_weights_list), n_t, "sp_weights_list")
  combiners = _per_table(combiner, n_t, "combiner")
  rows = _per_table(num_rows, n_t, "num_rows")
  entries = _per_table(None if _entries_list is None else list(_entries_list), n_t, "_entries_list")
  shapes = _per_table(None if _out_shapes is None else list(_out_shapes), n_t, "_out_shapes")
  for c in combiners:
    _check_combiner(c)
  results = [None] * n_t
  pooled = _pooled_training if return_trainable else _pooled_forward
  if return_trainable:
    _check_entries_many([(p, entries[i][0] if entries[i] is not None else sp_ids_list[i][1])
                         for i, p in enumerate(params_list) if pooled(p, max_norm)])
  groups = {}   # device -> [(i, ids, seg, w)]
  for i, params in enumerate(params_list):
    if not pooled(params, max_norm):
      results[i] = embedding_lookup_sparse(params, sp_ids_list[i], weights[i], combiner=combiners[i], max_norm=max_norm,
                                           return_trainable=return_trainable, num_rows=rows[i], plan_writeback=plan_writeback,
                                           _entries=entries[i], _out_shape=shapes[i], out_dtype=out_dtype)
      continue
    indices, ids = sp_ids_list[i]
    indices = torch.as_tensor(indices, device=params._primary)
    seg = (indices[:, 0] if indices.dim() == 2 else indices).to(torch.int64)
    ids = torch.as_tensor(ids, device=params._primary)
    w = weights[i] if weights[i] is None else torch.as_tensor(weights[i], dtype=torch.float32, device=params._primary)
    groups.setdefault(params._primary, []).append((i, ids, seg, w))
  for device, members in groups.items():
    _rows_in_one_read(rows, [(m[0], m[2]) for m in members if rows[m[0]] is None])
    if return_trainable:
      ent = {i: (entries[i] if entries[i] is not None else (ids.reshape(-1), seg, w))   # ids keep their key dtype
             for i, ids, seg, w in members}
      _admit_entries_many(params_list, {i: e[0] for i, e in ent.items()})   # (tiered members; ahead of the ONE read)
    reqs = []
    for i, ids, seg, w in members:
      t = params_list[i]._tables[0]
      reqs.append((_pooled_reader(t), ids.reshape(-1), seg, w, device_ops.COMBINERS[combiners[i]], rows[i], t._default_value))
    outs = table_ops.find_combine_many(reqs) if out_dtype is None else table_ops.find_combine_many(reqs, out_dtype=out_dtype)
    if not return_trainable:
      for (i, ids, seg, w), out in zip(members, outs):
        results[i] = out
      continue

    def wrapper(member, own_plan, entry_plan):
      i, ids, seg, w = member
      params, n = params_list[i], rows[i]
      return SparseTrainableWrapper(params, None, None, None, seg, w, combiners[i], n,
                                    shapes[i] if shapes[i] is not None else (n, params.dim), *ent[i], max_norm=max_norm,
                                    plan_writeback=own_plan, lookup_ids=ids, entry_plan=entry_plan)

    _wrap_grouped(device, params_list, members, outs, {i: e[0] for i, e in ent.items()}, plan_writeback, wrapper, results)
  return results


def _safe_sparse_rows(params, sp_ids, sparse_weights, num_rows):
  """The head of safe_embedding_lookup_sparse's preprocessing (PY/dynamic_embedding_ops.py:356-367): the operands on the
  variable's device, the rank > 2 flattening and the number of rows.  (rows, ids, w, n, lead)."""
  dense_shape = None
  if len(sp_ids) == 3:
    indices, ids, dense_shape = sp_ids
    dense_shape = [int(x) for x in dense_shape]
  else:
    indices, ids = sp_ids
  indices = torch.as_tensor(indices, device=params._primary)
  ids = torch.as_tensor(ids, device=params._primary)
  lead = None
  if indices.dim() == 2 and indices.shape[1] > 2:
    if dense_shape is None:
      raise ValueError("sparse ids of rank > 2 need their dense_shape: sp_ids = (indices, values, dense_shape)")
    lead = dense_shape[:-1]
    rows = torch.zeros(indices.shape[0], dtype=torch.int64, device=indices.device)
    for d in range(len(lead)):                       # row-major flattening of the leading dims
      rows = rows * lead[d] + indices[:, d].to(torch.int64)
    n = 1
    for d in lead:
      n *= d
  else:
    rows = (indices[:, 0] if indices.dim() == 2 else indices).to(torch.int64)
    if dense_shape is not None:
      n = dense_shape[0]
    elif num_rows is not None:
      n = num_rows
    else:
      n = int(rows.max().item()) + 1 if rows.numel() else 0
  w = None
  if sparse_weights is not None:
    w = torch.as_tensor(sparse_weights, dtype=torch.float32, device=params._primary)
  return rows, ids, w, n, lead


def _safe_sparse_lists_torch(params, rows, ids, w, n, combiner, default_id, return_trainable):
  """The two lists of the preprocessing in torch (boolean masks, `nonzero`, a stable sort: four host reads): the kept entries
  (rows, ids, w) and — for a trainable — the entry list.  The route of batches beyond `device_ops.safe_entries_many`'s limits
  and of tensors that do not live on a GPU, and what the device route is tested against."""
  keep = None
  if w is not None:
    if combiner != "sum":
      keep = w > 0
  if keep is not None:
    rows, ids, w = rows[keep], ids[keep], w[keep]
  entries = None
  if return_trainable:
    # the trainable's entries (sparse_fill_empty_rows, :379-391): one (row, default_id or 0, weight 1) per empty row, merged
    # into row order; with default_id=None the reference's `where` zeroes that entry's gradient — weight 0 does the same here
    # (a row whose weight sum is 0 has gradient 0, and a sum combiner multiplies by the weight)
    has = torch.zeros(n, dtype=torch.bool, device=params._primary)
    has[rows] = True
    er = torch.nonzero(~has).reshape(-1)
    all_rows = torch.cat([rows.to(torch.int64), er])
    all_ids = torch.cat([ids.reshape(-1),
                         torch.full(er.shape, 0 if default_id is None else int(default_id), dtype=ids.dtype, device=er.device)])
    ew = 0.0 if default_id is None else 1.0
    all_w = torch.cat([torch.ones(rows.numel(), dtype=torch.float32, device=er.device) if w is None else w,
                       torch.full((er.numel(),), ew, dtype=torch.float32, device=er.device)])
    order = torch.sort(all_rows, stable=True).indices
    entries = (all_ids[order].contiguous(), all_rows[order].contiguous(),
               None if (w is None and default_id is not None) else all_w[order].contiguous())
  return rows, ids, w, entries


def _safe_sparse_args_torch(params, sp_ids, sparse_weights, combiner, default_id, return_trainable, num_rows):
  """`_safe_sparse_args` with both lists made in torch."""
  rows, ids, w, n, lead = _safe_sparse_rows(params, sp_ids, sparse_weights, num_rows)
  rows, ids, w, entries = _safe_sparse_lists_torch(params, rows, ids, w, n, combiner, default_id, return_trainable)
  out_shape = (tuple(lead) if lead is not None else (n,)) + (params.dim,)
  return rows, ids, w, n, entries, out_shape, lead


def _safe_sparse_args(params, sp_ids, sparse_weights, combiner, default_id, return_trainable, num_rows):
  """The preprocessing of safe_embedding_lookup_sparse (PY/dynamic_embedding_ops.py:356-408): pruning by weight, the rank > 2
  flattening, the number of rows and — for a trainable — the entry list with one entry per empty row.  Returns what
  `embedding_lookup_sparse` is then called with and what `_safe_sparse_finish` needs: (rows, ids, w, n, entries, out_shape, lead).
  The kept entries and the entry list are built on the device (`_safe_sparse_args_many`)."""
  return _safe_sparse_args_many([params], [sp_ids], [sparse_weights], [combiner], [default_id], return_trainable, [num_rows])[0]


def _safe_sparse_args_many(params_list, sp_ids_list, weights, combiners, default_ids, return_trainable, num, ragged=False):
  """`_safe_sparse_args` of every member, bit for bit, with the kept lists and the entry lists of all members of a device from ONE
  `device_ops.safe_entries_many` (one C call, one host read of all counts).  ragged: sp_ids_list[i] is (row_splits int64, ids)
  with `num[i]` rows, and the member's `rows` are the row ids the splits stand for; the splits go to the builder as they are.
  A non-training member asks for its kept list only, and for nothing where it does not prune.  A member whose lists exceed the
  builder's limits, or whose tensors are not on a GPU, takes `_safe_sparse_lists_torch`."""
  n_t = len(params_list)
  heads = [(sp_ids_list[i][0], sp_ids_list[i][1], weights[i], num[i], None) if ragged else
           _safe_sparse_rows(params_list[i], sp_ids_list[i], weights[i], num[i]) for i in range(n_t)]
  lists = [None] * n_t   # member -> (rows, ids, w, entries)
  groups = {}            # device -> members the builder serves
  for i, (rows, ids, w, n, lead) in enumerate(heads):
    prune = w is not None and combiners[i] != "sum"
    if not (prune or return_trainable):
      lists[i] = (rows, ids, w, None)   # nothing to build (a ragged member never gets here: its forward needs no lists)
    elif rows.is_cuda and ids.dtype in (torch.int32, torch.int64) and device_ops.safe_entries_fit([(ids.numel(), n)]):
      groups.setdefault(rows.device, []).append(i)
  for members in groups.values():
    while members:   # (as many calls as the limit on a call's total asks for: one, for any batch a step sees)
      take, total = [], 0
      for i in members:
        if total + heads[i][1].numel() + heads[i][3] > device_ops.SAFE_ENTRIES_MAX_TOTAL:
          break
        take.append(i)
        total += heads[i][1].numel() + heads[i][3]
      members = members[len(take):]
      reqs, kept = [], []
      for i in take:
        rows, ids, w, n, _ = heads[i]
        prune = w is not None and combiners[i] != "sum"
        reqs.append((rows, ids, w, n, prune, default_ids[i], ragged))
        kept.append(prune or ragged)   # (a ragged member that keeps everything still takes its row ids from the kept list)
      built = device_ops.safe_entries_many(reqs, want_kept=kept, want_entries=return_trainable)
      for i, (k, ent) in zip(take, built):
        rows, ids, w, n, _ = heads[i]
        if w is not None and combiners[i] != "sum":
          rows, ids, w = k[1], k[0], k[2]
        elif ragged:
          rows = k[1]
        lists[i] = (rows, ids, w, ent)
  args = []
  for i, (rows, ids, w, n, lead) in enumerate(heads):
    if lists[i] is None:
      if ragged:
        from .ragged_embedding_ops import row_ids_of
        rows = row_ids_of(rows, ids.numel())
      lists[i] = _safe_sparse_lists_torch(params_list[i], rows, ids, w, n, combiners[i], default_ids[i], return_trainable)
    rows, ids, w, entries = lists[i]
    args.append((rows, ids, w, n, entries, (tuple(lead) if lead is not None else (n,)) + (params_list[i].dim,), lead))
  return args


def _safe_sparse_finish(params, res, rows, n, default_id, max_norm, lead):
  """The end of safe_embedding_lookup_sparse: the embedding of `default_id` in the rows left empty (:392-408), the leading dims
  restored (:411-424)."""
  if default_id is not None and n:
    empty = torch.ones(n, dtype=torch.bool, device=res.device)
    empty[rows] = False
    d = _read_rows(params, torch.tensor([default_id], dtype=params.key_dtype, device=params._primary), max_norm).to(torch.float32)
    res = torch.where(empty[:, None], d.to(res.dtype), res)   # (res: float32, or the caller's out_dtype — the select commutes with it)
  if lead is not None:
    res = res.reshape(tuple(lead) + (res.shape[-1],))
  return res


def safe_embedding_lookup_sparse(params, sp_ids, sparse_weights=None, combiner="mean", default_id=None,
                                 name="safe_embedding_lookup_sparse", partition_strategy=None, max_norm=None,
                                 return_trainable=False, num_rows=None, plan_writeback=False, out_dtype=None):
  """PY/dynamic_embedding_ops.py:296-430.  `sp_ids` = (indices[nnz, R], values[nnz][, dense_shape[R]]) — a
  SparseTensor of rank R >= 2 (or row ids [nnz] for rank 2).  Semantics of the reference, NOT of
  `tf.nn.safe_embedding_lookup_sparse`: ids are never pruned (any int64 is a legal key, negative ones too,
  T/dynamic_embedding_ops_test.py:1007-1050); entries with weight <= 0 are dropped unless combiner == "sum"
  (`_prune_invalid_weights`, :374-376); rows left without entries yield zeros, or the embedding of
  `default_id` (`sparse_fill_empty_rows`, :379-408); leading dims are flattened for the lookup and restored
  on the result (:356-367, 411-424).  out_dtype: `embedding_lookup_sparse`'s; the default_id row is converted the same way."""
  _check_combiner(combiner)
  _out_dtype(out_dtype)
  rows, ids, w, n, entries, out_shape, lead = _safe_sparse_args(params, sp_ids, sparse_weights, combiner, default_id,
                                                                 return_trainable, num_rows)
  out = embedding_lookup_sparse(params, (rows, ids), w, combiner=combiner, max_norm=max_norm,
                                return_trainable=return_trainable, num_rows=n, plan_writeback=plan_writeback,
                                _entries=entries, _out_shape=out_shape, out_dtype=out_dtype)
  res, tw = out if return_trainable else (out, None)
  res = _safe_sparse_finish(params, res, rows, n, default_id, max_norm, lead)
  return (res, _note_pruned(tw, sparse_weights, combiner)) if return_trainable else res


def safe_embedding_lookup_sparse_many(params_list, sp_ids_list, sparse_weights_list=None, combiner="mean", default_id=None,
                                      max_norm=None, return_trainable=False, num_rows=None, plan_writeback=False, out_dtype=None):
  """`safe_embedding_lookup_sparse` of a LIST of variables: result i is what the single form returns for table i, bit for bit
  (out_dtype: one for every result, as `embedding_lookup_sparse_many`'s).
  `combiner`, `default_id` and `num_rows` are scalars or per-table lists.  The preprocessing is the single form's
  (`_safe_sparse_args_many`: all tables' kept lists and entry lists from one builder call and one host read per device); the
  lookups go through `embedding_lookup_sparse_many`, one grouped call per device for the variables the pooled forward serves.  Row counts that neither a dense_shape nor num_rows gives are read in one host read per device."""
  n_t = len(params_list)
  if len(sp_ids_list) != n_t:
    raise ValueError("sp_ids_list: %d entries for %d tables" % (len(sp_ids_list), n_t))
  weights = _per_table(None if sparse_weights_list is None else list(sparse_weights_list), n_t, "sparse_weights_list")
  combiners = _per_table(combiner, n_t, "combiner")
  default_ids = _per_table(default_id, n_t, "default_id")
  num = _per_table(num_rows, n_t, "num_rows")
  for c in combiners:
    _check_combiner(c)
  unknown = {}   # device -> [(i, row ids)]: rank 2, no dense_shape, no num_rows, at least one entry
  for i, params in enumerate(params_list):
    if num[i] is None and len(sp_ids_list[i]) == 2:
      indices = torch.as_tensor(sp_ids_list[i][0], device=params._primary)
      if indices.numel() and (indices.dim() == 1 or indices.shape[1] <= 2):
        unknown.setdefault(params._primary, []).append((i, indices[:, 0] if indices.dim() == 2 else indices))
  for members in unknown.values():
    _rows_in_one_read(num, members)
  args = _safe_sparse_args_many(params_list, sp_ids_list, weights, combiners, default_ids, return_trainable, num)
  outs = embedding_lookup_sparse_many(params_list, [(a[0], a[1]) for a in args], [a[2] for a in args], combiner=combiners,
                                      max_norm=max_norm, return_trainable=return_trainable, num_rows=[a[3] for a in args],
                                      plan_writeback=plan_writeback, _entries_list=[a[4] for a in args],
                                      _out_shapes=[a[5] for a in args], out_dtype=out_dtype)
  results = []
  for i, (rows, ids, w, n, entries, out_shape, lead) in enumerate(args):
    res, tw = outs[i] if return_trainable else (outs[i], None)
    res = _safe_sparse_finish(params_list[i], res, rows, n, default_ids[i], max_norm, lead)
    results.append((res, _note_pruned(tw, weights[i], combiners[i])) if return_trainable else res)
  return results
