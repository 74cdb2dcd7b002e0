"""The fused-layout branch of the parameter-server path — host-side mirror of ``PartitionedHashTable`` in
monolith/native_training/distributed_ps.py (:611, :830-870 the sharding op's outputs, :1003-1150 lookup,
:1275-1400 apply_gradients), from per-feature ragged ids to the dense tower's inputs and back:

  sharding_sparse_fids (dedup, shard, fid_offset / feature_offset / nfl_offset, one fid list per table and PS) ->
  per PS one raw_lookup over its fid lists -> the flat results cut into one [rows, dim] view per pre-output
  index -> fused_embedding_to_layout;
  fused_embedding_to_layout_grad into per-PS flat gradients -> per PS one raw_apply_gradients.

``num_ps`` local ``MultiHashTable``s stand in for the parameter servers, all on one device, as in
``DistributedMultiTypeHashTable``.  PS ``i`` owns the ids with ``uint64(id) % num_ps == i`` (the sharding op's
unsigned remainder, parse_sparse_feature.cc:203) of every table.  The tables are reached through the raw calls
only: segment retrievers, an attached filter or a touched-key set act as they do there.

Out of scope: protobuf parsing, op versions 3-5, transfer_float16, the sync all-to-all path.
"""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from monolith_amd import distribution_ops, entry
from monolith_amd.multi_hash_table_ops import MultiHashTable, Ragged


class _Plan:
  """What a lookup leaves for the gradient: the packer's result, every PS's ragged ids, where every
  pre-output index lies in its PS's flat buffer."""

  def __init__(self, sharded, raggeds, views, flat_sizes):
    self.sharded, self.raggeds, self.views, self.flat_sizes = sharded, raggeds, views, flat_sizes


class PartitionedHashTable:
  """reference distributed_ps.py:611: the tables of ``configs`` on ``num_ps`` parameter servers, looked up and
  updated through the layouts of ``feature_cfgs`` (``distribution_ops.FeatureConfigs``; every feature's table is
  one of ``configs`` and its slice_dims add up to that table's dim)."""

  def __init__(self, num_ps: int, configs: Dict[str, entry.HashTableConfigInstance],
               feature_cfgs: distribution_ops.FeatureConfigs, name_suffix: str = "", device: Optional[int] = None,
               unique: bool = True):
    if not isinstance(num_ps, int) or isinstance(num_ps, bool) or num_ps < 1:
      raise ValueError("PartitionedHashTable: num_ps must be an int >= 1, got %r" % (num_ps,))
    self._num_ps, self._cfgs, self._unique = num_ps, feature_cfgs, bool(unique)
    self._tables: List[MultiHashTable] = []
    self._plan: Optional[_Plan] = None
    try:
      for i in range(num_ps):
        self._tables.append(MultiHashTable(configs, name_suffix="%s_pht%d" % (name_suffix, i), device=device))
      dim_of = dict(zip(self._tables[0].table_names, self._tables[0].get_table_dim_sizes()))
      for name, fc in feature_cfgs.feature_configs.items():
        if fc.table not in dim_of:
          raise ValueError("PartitionedHashTable: feature %s names the table %s, which is not configured" %
                           (name, fc.table))
        if sum(fc.slice_dims) != dim_of[fc.table]:
          raise ValueError("PartitionedHashTable: the slice_dims of feature %s add up to %d, table %s has dim %d" %
                           (name, sum(fc.slice_dims), fc.table, dim_of[fc.table]))
      self._dim_of = dim_of
    except Exception:
      self.close()
      raise

  def close(self):
    for t in self._tables:
      t.close()
    self._tables, self._plan = [], None

  @property
  def num_ps(self) -> int:
    return self._num_ps

  @property
  def tables(self) -> Tuple[MultiHashTable, ...]:
    """The per-PS tables, PS 0 first."""
    return tuple(self._tables)

  @property
  def unique(self) -> bool:
    return self._unique

  def _cut(self, sharded):
    """-> per PS (ragged ids over ALL of the PS's tables, flat floats), per pre-output index (PS, float offset,
    rows, dim)."""
    ix, ks, ps = sharded.index, sharded.key_start_host, self._num_ps
    F = len(ix.feature_names)
    t_of = {n: t for t, n in enumerate(ix.table_names)}
    raggeds, flat_sizes, views = [], [], [None] * (F * ps)
    for s in range(ps):
      lo = s * F
      splits, at = [0], 0
      for name in self._tables[0].table_names:   # (sorted, as the packer's tables are)
        t = t_of.get(name)
        if t is not None:
          dim, tfc, first = self._dim_of[name], ix.table_feature_count[t], ix.table_first[t]
          for j in range(tfc):
            rows = int(ks[lo + first + j + 1] - ks[lo + first + j])
            views[first * ps + s * tfc + j] = (s, at, rows, dim)
            at += rows * dim
          splits.append(int(ks[lo + first + tfc] - ks[lo]))
        else:
          splits.append(splits[-1])
      raggeds.append(Ragged(sharded.fid_list_flat[int(ks[lo]):int(ks[lo + F])],
                            np.ascontiguousarray(splits, dtype=np.int64)))
      flat_sizes.append(at)
    return raggeds, views, flat_sizes

  @staticmethod
  def _views_of(flats, views):
    return [flats[s][at:at + rows * dim].view(rows, dim) for s, at, rows, dim in views]

  def lookup(self, features, shared_features=(), batch_size: Optional[int] = None) -> List[torch.Tensor]:
    """reference :1003-1150: the layouts' tensors (layouts in sorted-name order) of ``features`` — {feature name:
    (values, row_splits)}, a feature of ``shared_features`` one list (``distribution_ops.sharding_sparse_fids``).
    The plan stays for ``apply_gradients``."""
    sharded = distribution_ops.sharding_sparse_fids(features, self._cfgs, self._num_ps, self._unique, shared_features,
                                                    batch_size)
    raggeds, views, flat_sizes = self._cut(sharded)
    flats = [self._tables[s].raw_lookup(raggeds[s]) for s in range(self._num_ps)]
    self._plan = _Plan(sharded, raggeds, views, flat_sizes)
    return distribution_ops.fused_embedding_to_layout(self._views_of(flats, views), sharded.fid_offset,
                                                      sharded.feature_offset, sharded.nfl_offset, sharded.batch_size,
                                                      self._cfgs)

  def apply_gradients(self, layout_grads: List[torch.Tensor], global_step: int = 0,
                      req_time: int = 0) -> "PartitionedHashTable":
    """reference :1275-1400: the layouts' gradients (one per tensor ``lookup`` returned) scattered back onto the
    looked-up rows and applied on the PS that owns each id, with the plan of the last ``lookup``.  With
    ``unique=False`` an id's occurrences are separate rows of the update, applied one after the other."""
    p = self._plan
    if p is None:
      raise RuntimeError("PartitionedHashTable.apply_gradients: no lookup to take the plan from")
    dev = p.sharded.fid_offset.device
    flats = [torch.empty(n, dtype=torch.float32, device=dev) for n in p.flat_sizes]
    grads = self._views_of(flats, p.views)
    distribution_ops.fused_embedding_to_layout_grad(grads, p.sharded.fid_offset, p.sharded.feature_offset,
                                                    p.sharded.nfl_offset, p.sharded.batch_size, list(layout_grads),
                                                    self._cfgs, out=grads)
    for s in range(self._num_ps):
      self._tables[s].raw_apply_gradients(p.raggeds[s], flats[s], global_step=global_step, req_time=req_time)
    return self
