"""TouchedKeySet on MI355X — host-side mirror of monolith/native_training/touched_key_set_ops.py.

The reference's resource is a HopscotchHashSet<FID> of ``capacity`` keys that drops the whole set when
an insert finds it over capacity; the table bridge fills one with (id, table) on every Optimize /
BatchOptimize / Reinitialize and the parameter-sync client drains it.  Here the set lives on the GPU
(mhte_touched_key_set_* of include/monolith_amd_hash_table.h): an insert is a handful of launches on
the current stream with no host synchronisation, so ids that never leave the device can be recorded.
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from monolith_amd import _lib
from monolith_amd._lib import check, vp


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class TouchedKeySet:
  """``capacity`` defaults to the reference's 64 MB / 32 bytes per key; ``concurrency_level`` is
  accepted for signature parity (the device set has no lock stripes).  ``max_insert`` (0 = capacity +
  1) bounds the ids of one device call and with them the memory: 16 bytes x the power of two >=
  2 * (capacity + 1 + max_insert); longer inputs are cut into several calls."""
  NAME_PREFIX = "MonolithTouchedKeySet"

  def __init__(self, capacity: int = 2_097_152, concurrency_level: int = 1024, name_suffix: str = "",
               device: Optional[int] = None, max_insert: int = 0):
    del concurrency_level
    self._lib = _lib.lib()
    self._capacity = int(capacity)
    self._name = "_".join([TouchedKeySet.NAME_PREFIX, name_suffix])
    self._device = (torch.cuda.current_device() if torch.cuda.is_available() else 0) if device is None else int(device)
    h = C.c_void_p()
    check(self._lib.mhte_touched_key_set_create(self._capacity, int(max_insert), self._device, C.byref(h)))
    self._h = h

  @property
  def capacity(self) -> int:
    return self._capacity

  @property
  def handle(self):
    return self._h

  @property
  def name(self) -> str:
    return self._name

  def stats(self) -> Tuple[int, int, int, int]:
    """(size, keys dropped by clears, clears, capacity); waits for the current stream."""
    out = (C.c_int64 * 4)()
    check(self._lib.mhte_touched_key_set_stats(self._h, out, _stream()))
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])

  @property
  def size(self) -> int:
    return self.stats()[0]

  def insert_async(self, ids: torch.Tensor, n_dev: Optional[torch.Tensor] = None, tag: int = 0) -> "TouchedKeySet":
    """Enqueues the insert of ``ids`` (of its first ``n_dev[0]`` entries when ``n_dev``, a uint32-sized
    device counter, is given) under ``tag``; nothing comes back to the host."""
    ids = ids.to(device="cuda:%d" % self._device, dtype=torch.int64).contiguous().reshape(-1)
    check(self._lib.mhte_touched_key_set_insert(self._h, vp(ids), ids.numel(), vp(n_dev), int(tag), _stream()))
    return self

  def insert(self, ids: torch.Tensor) -> int:
    """touched_key_set_ops.insert: returns the number of keys this call dropped (total_dropped_num)."""
    before = self.stats()[1]
    self.insert_async(ids)
    return self.stats()[1] - before

  def steal_pairs(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """GetAndClear: (ids int64 [n], tags int32 [n]) in no particular order; the set is empty afterwards."""
    dev = "cuda:%d" % self._device
    cap = self.stats()[0]
    ids = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    tags = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    n = (C.c_int64 * 1)()
    check(self._lib.mhte_touched_key_set_steal(self._h, vp(ids), vp(tags), cap, n, _stream()))
    return ids[:n[0]], tags[:n[0]]

  def steal(self) -> torch.Tensor:
    """touched_key_set_ops.steal: the ids (int64) of the set, which is empty afterwards."""
    return self.steal_pairs()[0]

  def close(self):
    if getattr(self, "_h", None):
      if torch.cuda.is_available():
        torch.cuda.synchronize(self._device)
      self._lib.mhte_touched_key_set_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass


def create_touched_key_set(capacity: int = 2_097_152, concurrency_level: int = 1024, name_suffix: str = "",
                           device: Optional[int] = None, max_insert: int = 0) -> TouchedKeySet:
  return TouchedKeySet(capacity, concurrency_level, name_suffix, device, max_insert)
