"""Device-side dedup / packing ops around the table — host-side mirror of
monolith/native_training/distribution_ops.py (reference :80-190) for the ops that sit on the hot
path: ``unique_key_with_value_and_offset``, ``fill_with_offset_map`` and its gradient.

Two API levels:
  * the reference signatures (ragged key, value_offset ragged-of-ragged, value_buffer), for drop-in
    call sites and parity tests against the reference's docstring examples;
  * ``DedupWorkspace`` — the same computation in the form the fused MI355X step uses
    (unique ids, inverse index, CSR occurrence lists, unique count left on the device so that
    dedup -> lookup -> scatter -> segment-sum -> optimize runs without a host round trip).
"""
import ctypes as C
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from monolith_amd import _lib
from monolith_amd._lib import check, vp
from monolith_amd.multi_hash_table_ops import Ragged, _stream


class UniqueResult(NamedTuple):
  unique_ids: torch.Tensor    # int64 [n]   (first n_unique entries valid), first-occurrence order
  inverse: torch.Tensor       # int32 [n]   unique index of every position
  seg_off: torch.Tensor       # int32 [n+1] CSR offsets of each unique id's occurrence list
  seg_pos: torch.Tensor       # int32 [n]   positions, grouped by unique id, occurrence order
  n_unique_dev: torch.Tensor  # int32 [1]
  n_unique: Optional[int]     # host copy when requested
  list_end: Optional[torch.Tensor] = None  # int32 [n]: set by unique_unordered, where seg_off holds
                                           # the list STARTS and the lists are not in CSR order


class DedupWorkspace:
  """Scratch + entry points for the device dedup (libmhte.so: mhte_unique & co)."""

  def __init__(self, device: Optional[int] = None):
    if not torch.cuda.is_available():
      raise _lib.MhteError(_lib.MHTE_UNAVAILABLE, "DedupWorkspace needs a HIP device")
    self._lib = _lib.lib()
    self._device = torch.cuda.current_device() if device is None else int(device)
    h = C.c_void_p()
    check(self._lib.mhte_dedup_ws_create(self._device, C.byref(h)))
    self._h = h

  def close(self):
    if getattr(self, "_h", None):
      torch.cuda.synchronize(self._device)
      self._lib.mhte_dedup_ws_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def unique(self, ids: torch.Tensor, want_host_count: bool = True,
             out: Optional[UniqueResult] = None) -> UniqueResult:
    """First-occurrence-order unique with occurrence lists (unique_mapping_ops.cc:82-114)."""
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
    n = ids.numel()
    dev = ids.device
    if out is None:
      uids = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
      inverse = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
      seg_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
      seg_pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
      nu = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
      uids, inverse, seg_off, seg_pos, nu = out[:5]
    host = (C.c_int64 * 1)()
    check(self._lib.mhte_unique(self._h, vp(ids), n, vp(uids), vp(inverse), vp(seg_off),
                                vp(seg_pos), vp(nu), host if want_host_count else None,
                                _stream()))
    return UniqueResult(uids, inverse, seg_off, seg_pos, nu,
                        host[0] if want_host_count else None)

  def step_dedup(self, ids: torch.Tensor, uids: torch.Tensor, n_unique_dev: torch.Tensor):
    """Run dedup of the FIRST batch of a pipelined step (mhte_step_dedup): unique ids in
    unspecified order + count on the device; the occurrence runs stay in this workspace for
    ``MultiHashTable.table_step_backward``."""
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
    check(self._lib.mhte_step_dedup(self._h, vp(ids), ids.numel(), vp(uids),
                                    vp(n_unique_dev), _stream()))

  def unique_unordered(self, ids: torch.Tensor, want_host_count: bool = False,
                       out: Optional[UniqueResult] = None) -> UniqueResult:
    """Same key set and occurrence lists as ``unique`` with an unspecified numbering of the unique
    ids (mhte_unique_unordered, 3 launches instead of 5) — what the unpipelined fused backward needs.  In the
    result ``seg_off[u]`` / ``list_end[u]`` bound the positions of unique id u inside seg_pos."""
    assert ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous()
    n = ids.numel()
    dev = ids.device
    if out is None or out.list_end is None:
      uids = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
      inverse = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
      lst_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
      lst_end = torch.empty(n + 1, dtype=torch.int32, device=dev)
      seg_pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
      nu = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
      uids, inverse, lst_start, seg_pos, nu = out[:5]
      lst_end = out.list_end
    host = (C.c_int64 * 1)()
    check(self._lib.mhte_unique_unordered(self._h, vp(ids), n, vp(uids), vp(inverse),
                                          vp(lst_start), vp(lst_end), vp(seg_pos), vp(nu),
                                          host if want_host_count else None, _stream()))
    return UniqueResult(uids, inverse, lst_start, seg_pos, nu,
                        host[0] if want_host_count else None, lst_end)

  def gather_rows(self, src: torch.Tensor, index: torch.Tensor, n: int, dim: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[p] = src[index[p]] — FillWithOffsetMap in gather form (unique_mapping_ops.cc:225-242)."""
    if out is None:
      out = torch.empty((n, dim), dtype=torch.float32, device=src.device)
    check(self._lib.mhte_gather_rows(vp(src), vp(index), n, dim, vp(out), _stream()))
    return out

  def segment_sum(self, grads: torch.Tensor, u: UniqueResult, dim: int,
                  out: Optional[torch.Tensor] = None, exact_order: bool = False) -> torch.Tensor:
    """out[k] = sum of grads over the occurrence list of unique id k
    (FillWithOffsetMapGradient, unique_mapping_ops.cc:307-324).  Rows >= n_unique are untouched."""
    n = grads.numel() // dim
    if out is None:
      out = torch.zeros((max(n, 1), dim), dtype=torch.float32, device=grads.device)
    check(self._lib.mhte_segment_sum(self._h, vp(grads), vp(u.inverse), vp(u.seg_off),
                                     vp(u.seg_pos), vp(u.n_unique_dev), n, dim, vp(out),
                                     exact_order, _stream()))
    return out


_default_ws = {}


def _ws(device) -> DedupWorkspace:
  d = device.index if isinstance(device, torch.device) else int(device)
  if d not in _default_ws:
    _default_ws[d] = DedupWorkspace(d)
  return _default_ws[d]


class _UniqueKeyWithValueAndOffsetResult(NamedTuple):
  unique_key: Ragged                 # values int64 [U], row_splits host [T+1]
  value_offset: torch.Tensor         # int64 [n]: float offsets into value_buffer
  value_offset_split: torch.Tensor   # int64 [U+1]: list boundaries per unique key
  value_buffer: Optional[torch.Tensor]


def unique_key_with_value_and_offset(key: Ragged, dims: List[int], generate_buffer=True):
  """reference distribution_ops.py:86-118 / ops/unique_mapping_ops.cc:51-155.

  key = [[0, 1, 0], [0]], dims = [2, 3] =>
    unique_key = [[0, 1], [0]], value_offset = [[[0, 4], [2]], [[6]]], buffer length 9.
  The ragged-of-ragged value_offset is returned flat (values + per-unique-key splits); the outer
  split is unique_key.row_splits, exactly the three tensors the reference op emits."""
  T = len(dims)
  if key.row_splits.size != T + 1:
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT,
        "RaggedKey should have %d but got %d" % (T, key.row_splits.size - 1))
  dev = key.values.device
  ws = _ws(dev)
  L = _lib.lib()
  n = key.values.numel()
  uniq_parts, splits = [], [0]
  value_offset = torch.empty(n, dtype=torch.int64, device=dev)
  vo_split_parts = []
  value_base = 0
  for t in range(T):
    lo, hi = int(key.row_splits[t]), int(key.row_splits[t + 1])
    ids = key.values[lo:hi].contiguous()
    r = ws.unique(ids, want_host_count=True)
    U = r.n_unique
    uniq_parts.append(r.unique_ids[:U])
    if hi > lo:
      vos = torch.empty(hi - lo + 1, dtype=torch.int64, device=dev)
      check(L.mhte_value_offsets(vp(r.seg_off), vp(r.seg_pos), vp(r.n_unique_dev),
                                 hi - lo, value_base, dims[t], lo, vp(value_offset[lo:hi]), vp(vos),
                                 _stream()))
      # the reference emits cumulative list ends after a leading 0
      vo_split_parts.append(vos[1:U + 1])
    splits.append(splits[-1] + U)
    value_base += (hi - lo) * dims[t]
  zero = torch.zeros(1, dtype=torch.int64, device=dev)
  value_offset_split = torch.cat([zero] + vo_split_parts) if vo_split_parts else zero
  unique_key = Ragged(torch.cat(uniq_parts) if uniq_parts else key.values[:0],
                      np.ascontiguousarray(splits, dtype=np.int64))
  buf = torch.zeros(value_base, dtype=torch.float32, device=dev) if generate_buffer else None
  return _UniqueKeyWithValueAndOffsetResult(unique_key, value_offset, value_offset_split, buf)


def _all_vec4(dims):
  return all(d % 4 == 0 for d in dims)


def fill_with_offset_map(pos: Ragged, value: torch.Tensor, value_offset_map: torch.Tensor,
                         value_offset_map_split: torch.Tensor, value_buffer: torch.Tensor,
                         dims: List[int]) -> torch.Tensor:
  """reference distribution_ops.py:121-148 / ops/unique_mapping_ops.cc:204-268."""
  T = len(dims)
  if pos.row_splits.size != T + 1:
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT, "Pos's first dim doesn't match dim size. %d v.s. %d" %
        (pos.row_splits.size - 1, T))
  expected = int(sum(int(pos.row_splits[t + 1] - pos.row_splits[t]) * dims[t] for t in range(T)))
  if value.numel() < expected:
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT,
        "Value size doesn't match expected size. expected: %d, actual: %d. " %
        (expected, value.numel()))
  L = _lib.lib()
  vec = 1 if _all_vec4(dims) else 0
  voff = 0
  for t in range(T):
    lo, hi = int(pos.row_splits[t]), int(pos.row_splits[t + 1])
    if hi > lo:
      check(L.mhte_fill_with_offset_map(vp(pos.values[lo:hi]), hi - lo,
                                        vp(value[voff:]), vp(value_offset_map),
                                        vp(value_offset_map_split), dims[t], vec,
                                        vp(value_buffer), _stream()))
    voff += (hi - lo) * dims[t]
  return value_buffer


def fill_with_offset_map_gradient(pos: Ragged, grad: torch.Tensor, grad_offset_map: torch.Tensor,
                                  grad_offset_map_split: torch.Tensor,
                                  dims: List[int]) -> torch.Tensor:
  """ops/unique_mapping_ops.cc:284-329: backprop_grad[i] = sum over offsets of pos[i]."""
  T = len(dims)
  total = int(sum(int(pos.row_splits[t + 1] - pos.row_splits[t]) * dims[t] for t in range(T)))
  out = torch.empty(total, dtype=torch.float32, device=grad.device)
  L = _lib.lib()
  vec = 1 if _all_vec4(dims) else 0
  ooff = 0
  for t in range(T):
    lo, hi = int(pos.row_splits[t]), int(pos.row_splits[t + 1])
    if hi > lo:
      check(L.mhte_fill_with_offset_map_gradient(vp(pos.values[lo:hi]), hi - lo,
                                                 vp(grad), vp(grad_offset_map),
                                                 vp(grad_offset_map_split), dims[t], vec,
                                                 vp(out[ooff:]), _stream()))
    ooff += (hi - lo) * dims[t]
  return out


# ---------------------------------------------------------------------------------------------
# the step right after the exchange (reference distribution_ops.py:671-760, embedding_combiners.py)
# ---------------------------------------------------------------------------------------------
def _ptr_array(tensors):
  arr = (C.c_void_p * len(tensors))(*[C.c_void_p(t.data_ptr()) for t in tensors])
  return arr


def fused_gather_embeddings_by_input(fused_embeddings: torch.Tensor,
                                     fused_embedding_offsets: List[torch.Tensor],
                                     embedding_dims: List[int]) -> List[torch.Tensor]:
  """distribution_ops.fused_gather_embeddings_by_input (reference :671-675): for every merged slot i,
  rows of ``embedding_dims[i]`` floats gathered from the flat fused buffer at the given offsets."""
  assert fused_embeddings.is_cuda and fused_embeddings.dtype == torch.float32
  offs = [o.to(device=fused_embeddings.device, dtype=torch.int32).contiguous()
          for o in fused_embedding_offsets]
  outs = [torch.empty((o.numel(), d), dtype=torch.float32, device=fused_embeddings.device)
          for o, d in zip(offs, embedding_dims)]
  n = (C.c_int64 * len(offs))(*[o.numel() for o in offs])
  dims = (C.c_int32 * len(offs))(*[int(d) for d in embedding_dims])
  check(_lib.lib().mhte_fused_gather_embeddings_by_input(vp(fused_embeddings.contiguous()),
                                                         len(offs), _ptr_array(offs), n,
                                                         dims, _ptr_array(outs), _stream()))
  return outs


def fused_gather_embeddings_by_input_gradient(fused_embeddings_size: int, grads: List[torch.Tensor],
                                              embedding_offsets: List[torch.Tensor],
                                              embedding_dims: List[int], scale=1.0):
  """reference :678-686: the flat gradient of the fused buffer.  No float atomics: rows that share an
  offset are grouped and added in row order (rows numbered input after input, ``acc = acc + g * scale``
  from 0, each row with its own dim columns), inputs taken in chunks of 32, added chunk after chunk.
  Two rows must either share an offset or cover disjoint ranges.  ``MHTE_POOL_ATOMICS=1`` selects the
  reference's atomic form (arrival order).
  ``scale``: a Python float, or a 0-d float32 device tensor (``clip_ops.global_norm_and_scale``) that is
  read on the device — nothing comes back to the host and a captured graph replays with its current value."""
  dev = grads[0].device
  offs = [o.to(device=dev, dtype=torch.int32).contiguous() for o in embedding_offsets]
  gs = [g.to(device=dev, dtype=torch.float32).contiguous() for g in grads]
  out = torch.empty(int(fused_embeddings_size), dtype=torch.float32, device=dev)
  n = (C.c_int64 * len(offs))(*[o.numel() for o in offs])
  dims = (C.c_int32 * len(offs))(*[int(d) for d in embedding_dims])
  if isinstance(scale, torch.Tensor):
    if not (scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1):
      raise TypeError("fused_gather_embeddings_by_input_gradient: scale must be a float or a 0-d float32 "
                      "tensor on the GPU")
    check(_lib.lib().mhte_fused_gather_embeddings_by_input_gradient_dev_scale(
        vp(out), out.numel(), len(offs), _ptr_array(gs), _ptr_array(offs), n,
        dims, vp(scale), _stream()))
    return out
  check(_lib.lib().mhte_fused_gather_embeddings_by_input_gradient(
      vp(out), out.numel(), len(offs), _ptr_array(gs), _ptr_array(offs), n,
      dims, scale, _stream()))
  return out


def _reduce(id_indices, id_values, id_length, mode, indices_sorted):
  idx = id_indices.reshape(-1).to(dtype=torch.int64).contiguous()
  vals = id_values.to(dtype=torch.float32).contiguous()
  assert vals.is_cuda and idx.is_cuda and vals.dim() == 2 and idx.numel() == vals.shape[0]
  batch = int(id_length[0]) if not isinstance(id_length, int) else id_length
  out = torch.empty((batch, vals.shape[1]), dtype=torch.float32, device=vals.device)
  check(_lib.lib().mhte_reduce_rows(vp(idx), vp(vals), idx.numel(), vals.shape[1], batch, mode,
                                    indices_sorted, vp(out), _stream()))
  return out


def reduce_sum(id_indices, id_values, id_length, indices_sorted: bool = True):
  """distribution_ops.reduce_sum (reduce_op.cc:29-51).  ``indices_sorted``: row indices ascend, as
  a sparse / ragged input's do — sequential, bit-identical accumulation."""
  return _reduce(id_indices, id_values, id_length, 0, indices_sorted)


def reduce_mean(id_indices, id_values, id_length, indices_sorted: bool = True):
  """distribution_ops.reduce_mean (reduce_op.cc:55-87)."""
  return _reduce(id_indices, id_values, id_length, 1, indices_sorted)


def reduce_sqrtn(id_indices, id_values, id_length, indices_sorted: bool = True):
  """distribution_ops.reduce_sqrtn (ReduceSquareNorm, reduce_op.cc:91-125): sqrt of the sum of
  squares."""
  return _reduce(id_indices, id_values, id_length, 2, indices_sorted)


# ---------------------------------------------------------------------------------------------
# fused reduce-and-split pooling (reference distribution_ops.py:802-884; PoolingHelper of feature.py:501-541)
# ---------------------------------------------------------------------------------------------
def _split_plan(splits, rows, dims, slice_dims, dev):
  """-> (fused row splits on the device, the ctypes arrays of the plan); ``slice_dims`` is flattened as the
  reference flattens it (distribution_ops.py:852-862)."""
  flat_slice_dims, row_split_splits = [], [0]
  for s in slice_dims:
    flat_slice_dims.extend(int(d) for d in s)
  for sp in splits:
    row_split_splits.append(row_split_splits[-1] + int(sp.shape[0]))
  fused = [sp.to(device=dev, dtype=torch.int32).reshape(-1) for sp in splits]
  fused_splits = (torch.cat(fused) if len(fused) != 1 else fused[0]).contiguous()
  n = len(rows)
  return (fused_splits, flat_slice_dims, (C.c_int32 * len(row_split_splits))(*row_split_splits),
          (C.c_int64 * max(n, 1))(*rows), (C.c_int32 * max(n, 1))(*dims),
          (C.c_int32 * max(len(flat_slice_dims), 1))(*flat_slice_dims))


def _aligned_slices(batch: int, flat_slice_dims: List[int], dev) -> List[torch.Tensor]:
  """[batch, d] tensors carved from ONE allocation, every start 16-byte aligned (the reference's
  FusedAlignedOutputAllocator): the 16-byte path applies to each of them."""
  starts, total = [], 0
  for d in flat_slice_dims:
    starts.append(total)
    total += (batch * d + 3) // 4 * 4
  buf = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
  return [buf[o:o + batch * d].view(batch, d) for o, d in zip(starts, flat_slice_dims)]


def fused_reduce_and_split_gpu(splits: List[torch.Tensor], embeddings: List[torch.Tensor],
                               slice_dims: List[List[int]]) -> List[torch.Tensor]:
  """distribution_ops.fused_reduce_and_split_gpu (reference :838-871, MonolithFusedReduceAndSplitGPU).

  Args:
    splits: list of N 'row_splits' of fid ragged tensors (batch size + 1 entries each)
    embeddings: list of N embeddings, the i-th [n_i, dim_i]
    slice_dims: list of N slice_dims; sum(slice_dims[i]) = dim_i
  Output:
    reduced: M output tensors, the i-th of shape [bs, flat_slice_dims[i]], where
    flat_slice_dims = concat(slice_dims) and M = len(flat_slice_dims): the sum of every feature's rows per
    batch row, in row order from +0 (the reference's bits), cut into the feature's column slices.  One launch."""
  if len(splits) != len(embeddings) or len(slice_dims) != len(embeddings):
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT, "fused_reduce_and_split_gpu: %d splits, %d embeddings, %d slice_dims" %
        (len(splits), len(embeddings), len(slice_dims)))
  dev = embeddings[0].device if embeddings else torch.device("cuda")
  embs = [e.to(device=dev, dtype=torch.float32).contiguous() for e in embeddings]
  assert all(e.dim() == 2 for e in embs)
  fused_splits, flat, rss, rows, dims, sdims = _split_plan(
      splits, [int(e.shape[0]) for e in embs], [int(e.shape[1]) for e in embs], slice_dims, dev)
  batch = max(int(splits[0].shape[0]) - 1, 0) if splits else 0
  outs = _aligned_slices(batch, flat, dev)
  check(_lib.lib().mhte_fused_reduce_and_split(
      vp(fused_splits), rss, _ptr_array(embs), rows, dims, len(embs), sdims, len(flat),
      _ptr_array(outs), _stream()))
  return outs


def fused_reduce_and_split_gpu_grad(splits: List[torch.Tensor], embeddings: List[torch.Tensor],
                                    slice_grads: List[torch.Tensor],
                                    slice_dims: List[List[int]]) -> List[torch.Tensor]:
  """The gradient of ``fused_reduce_and_split_gpu`` (reference :874-884, MonolithFusedReduceAndSplitGPUGrad):
  for every embedding (only its shape is used) a gradient of the same shape — row r takes the feature's
  slice gradients, side by side, at the batch row whose range holds r; a row outside every range is 0."""
  if len(splits) != len(embeddings) or len(slice_dims) != len(embeddings):
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT, "fused_reduce_and_split_gpu_grad: %d splits, %d embeddings, %d slice_dims" %
        (len(splits), len(embeddings), len(slice_dims)))
  dev = slice_grads[0].device if slice_grads else torch.device("cuda")
  fused_splits, flat, rss, rows, dims, sdims = _split_plan(
      splits, [int(e.shape[0]) for e in embeddings], [int(e.shape[1]) for e in embeddings], slice_dims, dev)
  batch = max(int(splits[0].shape[0]) - 1, 0) if splits else 0
  if len(slice_grads) != len(flat) or any(tuple(g.shape) != (batch, d) for g, d in zip(slice_grads, flat)):
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT,
        "fused_reduce_and_split_gpu_grad: slice_grads must be [bs = %d, d] for d in %s" % (batch, flat))
  gs = [g.to(device=dev, dtype=torch.float32).contiguous() for g in slice_grads]
  grads = [torch.empty((int(e.shape[0]), int(e.shape[1])), dtype=torch.float32, device=dev)
           for e in embeddings]
  check(_lib.lib().mhte_fused_reduce_and_split_grad(
      vp(fused_splits), rss, rows, dims, len(grads), sdims, len(flat),
      _ptr_array(gs), _ptr_array(grads), _stream()))
  return grads


def _row_splits_of_sorted(id_indices: torch.Tensor, batch: int) -> torch.Tensor:
  idx = id_indices.reshape(-1).to(dtype=torch.int64).contiguous()
  edges = torch.arange(batch + 1, dtype=torch.int64, device=idx.device)
  return torch.searchsorted(idx, edges).to(torch.int32)


def _unsorted_route(name):
  raise NotImplementedError(
      "%s: indices_sorted=False has no device path; reduce_sum(..., indices_sorted=False) followed by "
      "torch.split is the route for row indices in any order" % name)


def fused_reduce_sum_and_split(id_indices: torch.Tensor, id_values: torch.Tensor, id_length,
                               split_dims: List[int], indices_sorted: bool = True) -> List[torch.Tensor]:
  """distribution_ops.fused_reduce_sum_and_split (reference :802-826, MonolithFusedReduceSumAndSplit): very
  similar to a sparse reduce_sum, combined with a fused split.

  Args:
    id_indices: 1-D tensor, the batch row of every row of id_values (ascending).
    id_values: 2-D tensor, a list of actual values.
    id_length: the batch size.
    split_dims: dimensions of the split vectors; sum(split_dims) = id_values.shape[1].
  Output:
    reduced: M output tensors, the i-th of shape [bs, split_dims[i]]."""
  if not indices_sorted:
    _unsorted_route("fused_reduce_sum_and_split")
  batch = id_length if isinstance(id_length, int) else int(torch.as_tensor(id_length).reshape(-1)[0])
  assert id_values.is_cuda and id_values.dim() == 2 and id_indices.numel() == id_values.shape[0]
  splits = _row_splits_of_sorted(id_indices.to(id_values.device), batch)
  return fused_reduce_and_split_gpu([splits], [id_values], [list(split_dims)])


def fused_reduce_sum_and_split_gradient(id_indices: torch.Tensor, grads: List[torch.Tensor],
                                        split_dims: List[int], indices_sorted: bool = True) -> torch.Tensor:
  """MonolithFusedReduceSumAndSplitGradient (reference :829-835): the gradient of id_values,
  [len(id_indices), sum(split_dims)] — row i is the slices' gradients at batch row id_indices[i]."""
  if not indices_sorted:
    _unsorted_route("fused_reduce_sum_and_split_gradient")
  dev = grads[0].device
  batch = int(grads[0].shape[0])
  splits = _row_splits_of_sorted(id_indices.to(dev), batch)
  shape = torch.empty((int(id_indices.numel()), int(sum(split_dims))), device="meta")
  return fused_reduce_and_split_gpu_grad([splits], [shape], list(grads), [list(split_dims)])[0]


# ---------------------------------------------------------------------------------------------
# fused_embedding_to_layout (reference distribution_ops.fused_embedding_to_layout and its gradient;
# configuration messages of idl/matrix/proto/example.proto:176-221 as plain Python objects)
# ---------------------------------------------------------------------------------------------
class PoolingType:
  SUM, MEAN, FIRSTN = 0, 1, 3


class OutType:
  CONCAT, STACK, ADDN, NONE = 0, 1, 2, 3


class SliceConfig:
  def __init__(self, feature_name: str, start: int, end: int):
    self.feature_name, self.start, self.end = feature_name, int(start), int(end)


class OutConfig:
  """slice_configs in order; shape: list of per-tensor dims (first dim -1 = batch): one tensor for
  CONCAT / STACK / ADDN, one per slice for NONE."""

  def __init__(self, slice_configs: List[SliceConfig], out_type: int, shape: List[List[int]]):
    self.slice_configs, self.out_type, self.shape = list(slice_configs), out_type, [list(s) for s in shape]


class FeatureConfig:
  def __init__(self, table: str, pooling_type: int = PoolingType.SUM, slice_dims=(),
               max_sequence_length: int = 0):
    self.table, self.pooling_type = table, pooling_type
    self.slice_dims, self.max_sequence_length = list(slice_dims), int(max_sequence_length)


class FeatureConfigs:
  def __init__(self, feature_configs, out_configs):
    self.feature_configs, self.out_configs = dict(feature_configs), dict(out_configs)


def _layout_plan(cfgs: FeatureConfigs, batch_size: int):
  """-> (slices ctypes array, output shapes in op order).  Mirrors the op's constructor
  (runtime/ops/fused_embedding_to_layout.cc:240-284): features are indexed by sorted name, layouts
  are emitted in sorted-name order, a slice takes its feature's pooling type."""
  feature_names = sorted(cfgs.feature_configs)
  slices, shapes = [], []
  for ln in sorted(cfgs.out_configs):
    oc = cfgs.out_configs[ln]
    base = len(shapes)
    for sh in oc.shape:
      shapes.append([batch_size if (i == 0 and d == -1) else d for i, d in enumerate(sh)])
    offset = 0
    for i, sc in enumerate(oc.slice_configs):
      fc = cfgs.feature_configs[sc.feature_name]
      dim = sc.end - sc.start
      s = _lib.LayoutSlice()
      s.feature_idx = feature_names.index(sc.feature_name)
      s.start, s.dim = sc.start, dim
      s.pooling, s.max_sequence_length = fc.pooling_type, fc.max_sequence_length
      s.out_type = oc.out_type
      if len(oc.shape) == 1:
        s.out_index = base
        row = int(np.prod(shapes[base][1:]))
        if oc.out_type == OutType.CONCAT:
          s.out_offset = offset
          offset += dim
        elif oc.out_type == OutType.STACK:
          s.out_offset = i * dim
        else:
          s.out_offset = 0
        s.out_row_floats = row
      else:                          # NONE: one tensor per slice
        s.out_index = base + i
        s.out_offset = 0
        s.out_row_floats = int(np.prod(shapes[base + i][1:]))
      slices.append(s)
  return (_lib.LayoutSlice * len(slices))(*slices), shapes


def _layout_common(embeddings_list, fid_offset, feature_offset, nfl_offset):
  dev = embeddings_list[0].device
  embs = [e.to(device=dev, dtype=torch.float32).contiguous() for e in embeddings_list]
  stride = (C.c_int32 * len(embs))(*[int(e.shape[1]) if e.dim() == 2 else 1 for e in embs])
  count = (C.c_int64 * len(embs))(*[e.numel() for e in embs])
  fo = fid_offset.to(device=dev).contiguous()
  assert fo.dtype in (torch.int64, torch.uint64)
  fe = feature_offset.to(device=dev, dtype=torch.int32).contiguous()
  nf = nfl_offset.to(device=dev).contiguous()
  assert nf.dtype in (torch.int32, torch.uint32)
  return dev, embs, stride, count, fo, fe, nf


def fused_embedding_to_layout(embeddings_list: List[torch.Tensor], fid_offset: torch.Tensor,
                              feature_offset: torch.Tensor, nfl_offset: torch.Tensor, batch_size: int,
                              feature_cfgs: FeatureConfigs,
                              one_fid_unique_rows: bool = False) -> List[torch.Tensor]:
  """MonolithEmbeddingToLayout: the layouts' tensors, layouts in sorted-name order.
  ``one_fid_unique_rows``: MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS (float4 copies)."""
  dev, embs, stride, count, fo, fe, nf = _layout_common(embeddings_list, fid_offset, feature_offset,
                                                        nfl_offset)
  slices, shapes = _layout_plan(feature_cfgs, int(batch_size))
  outs = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes]
  lens = (C.c_int64 * len(outs))(*[o.numel() for o in outs])
  check(_lib.lib().mhte_embedding_to_layout(
      _ptr_array(embs), stride, count, len(embs), vp(fo), fo.numel(), vp(fe), fe.numel(), vp(nf),
      nf.numel(), int(batch_size), slices, len(slices), _ptr_array(outs), lens, len(outs),
      _lib.MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS if one_fid_unique_rows else 0, _stream()))
  return outs


def fused_embedding_to_layout_grad(embeddings_list: List[torch.Tensor], fid_offset: torch.Tensor,
                                   feature_offset: torch.Tensor, nfl_offset: torch.Tensor,
                                   batch_size: int, tensors_grad: List[torch.Tensor],
                                   feature_cfgs: FeatureConfigs, one_fid_unique_rows: bool = False,
                                   out: List[torch.Tensor] = None) -> List[torch.Tensor]:
  """MonolithEmbeddingToLayoutGrad: gradients of ``embeddings_list`` (same shapes; ``out``: buffers
  to write them into, e.g. views of one flat gradient)."""
  dev, embs, stride, count, fo, fe, nf = _layout_common(embeddings_list, fid_offset, feature_offset,
                                                        nfl_offset)
  slices, shapes = _layout_plan(feature_cfgs, int(batch_size))
  assert len(tensors_grad) == len(shapes)
  tg = [g.to(device=dev, dtype=torch.float32).contiguous() for g in tensors_grad]
  grads = out if out is not None else [torch.empty_like(e) for e in embs]
  lens = (C.c_int64 * len(tg))(*[g.numel() for g in tg])
  check(_lib.lib().mhte_embedding_to_layout_grad(
      _ptr_array(grads), stride, count, len(embs), vp(fo), fo.numel(), vp(fe), fe.numel(), vp(nf),
      nf.numel(), int(batch_size), slices, len(slices), _ptr_array(tg), lens, len(tg),
      _lib.MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS if one_fid_unique_rows else 0, _stream()))
  return grads


# ---- the fused-layout packer: from per-feature ragged ids to the layout op's inputs and the PS fid lists ---------
# (reference ShardingSparseFids at op version 2: data/kernels/parse_sparse_feature.cc:106-155, :187-240, :259-424,
# parse_sparse_feature.h:620-990)
SHARDING_TILE = 4096   # ids a workgroup of the packer's stable sort ranks at a time (kGsWaves * kGsRound)
_UINT32 = getattr(torch, "uint32", None)
_UINT64 = getattr(torch, "uint64", None)


class ShardingIndex(NamedTuple):
  """The index arithmetic of a configuration (parse_sparse_feature.cc:106-155): features and tables in sorted-name
  order; per feature its table, its place among the table's features and its place in table-major order."""
  feature_names: List[str]
  table_names: List[str]
  table_index: List[int]
  feature_in_table_index: List[int]
  table_feature_count: List[int]
  table_first: List[int]            # [n_tables + 1]: the table's first feature in table-major order
  pre_output_index: List[int]       # per feature, for a given ps_num: table_first * ps_num

  @staticmethod
  def of(feature_cfgs: "FeatureConfigs", ps_num: int) -> "ShardingIndex":
    names = sorted(feature_cfgs.feature_configs)
    tables = sorted({feature_cfgs.feature_configs[n].table for n in names})
    t_of = {t: i for i, t in enumerate(tables)}
    count = [0] * len(tables)
    t_idx, fit = [], []
    for n in names:
      t = t_of[feature_cfgs.feature_configs[n].table]
      t_idx.append(t)
      fit.append(count[t])
      count[t] += 1
    first = [0]
    for c in count:
      first.append(first[-1] + c)
    return ShardingIndex(names, tables, t_idx, fit, count, first, [first[t] * ps_num for t in t_idx])


class ShardedFids(NamedTuple):
  fid_offset: torch.Tensor              # uint64 [N], input order
  feature_offset: torch.Tensor          # int32 [R + 1]
  nfl_offset: torch.Tensor              # uint32 [F + 1]
  batch_size: int
  fid_list: Optional[List[torch.Tensor]]          # [table_index * ps_num + shard]: views of fid_list_flat
  fid_list_row_splits: Optional[List[np.ndarray]]  # the same index: table_feature_count + 1 entries each, host
  fid_list_flat: torch.Tensor           # int64 [N]: the placed ids, PS after PS (see ``ps_ragged``)
  key_start: torch.Tensor               # int64 [F * ps_num + 2] on the device (mhte_sharding_sparse_fids)
  row_splits_flat: torch.Tensor         # int64 [F * ps_num + n_tables * ps_num] on the device: every list's row_splits
  list_bounds: torch.Tensor             # int64 [n_tables * ps_num, 2] on the device: start, size in fid_list_flat
  key_start_host: Optional[np.ndarray]  # None in the plan variant
  index: ShardingIndex
  ps_num: int

  def ps_ragged(self, shard: int) -> Ragged:
    """What PS ``shard`` looks up: its ids of every table, tables in sorted-name order (values: a view)."""
    ks, F = self.key_start_host, len(self.index.feature_names)
    lo = shard * F
    splits = np.ascontiguousarray([ks[lo + f] - ks[lo] for f in self.index.table_first], dtype=np.int64)
    return Ragged(self.fid_list_flat[int(ks[lo]):int(ks[lo + F])], splits)

  def pre_output_sizes(self) -> np.ndarray:
    """ids per pre-output index (the rows of the layout op's embeddings_list entries)."""
    ks, F, ix = self.key_start_host, len(self.index.feature_names), self.index
    out = np.zeros(F * self.ps_num, dtype=np.int64)
    for t, tfc in enumerate(ix.table_feature_count):
      for s in range(self.ps_num):
        lo, k0 = s * F + ix.table_first[t], ix.table_first[t] * self.ps_num + s * tfc
        out[k0:k0 + tfc] = np.diff(ks[lo:lo + tfc + 1])
    return out


def _sharding_feature(name, x, shared, dev):
  """-> (values, row_splits or None when implied, host row_splits?)"""
  what = "sharding_sparse_fids: feature %s" % name
  if isinstance(x, torch.Tensor):
    values, rs = x, None
    if not shared:
      raise TypeError("%s: only a shared feature is a single list; give (values, row_splits)" % what)
  else:
    values, rs = x[0], x[1]
  if not isinstance(values, torch.Tensor) or values.dtype != torch.int64:
    raise TypeError("%s: ids must be an int64 torch tensor, got %s" %
                    (what, values.dtype if isinstance(values, torch.Tensor) else type(values).__name__))
  if not values.is_cuda:
    raise TypeError("%s: ids must be on the GPU (there is no CPU path)" % what)
  if values.dim() != 1 or not values.is_contiguous():
    raise ValueError("%s: ids must be a contiguous 1-d tensor" % what)
  if dev is not None and values.device != dev:
    raise ValueError("%s: ids are on %s, other features on %s" % (what, values.device, dev))
  n = values.numel()
  if rs is None:
    rs = np.array([0, n], dtype=np.int64)
  if isinstance(rs, torch.Tensor):
    if rs.dtype != torch.int64 or not rs.is_cuda or rs.dim() != 1 or not rs.is_contiguous() or rs.numel() < 1:
      raise TypeError("%s: row_splits on the device must be a contiguous 1-d int64 tensor" % what)
  else:
    rs = _checked_row_splits(rs, n)
  n_rows = (rs.numel() if isinstance(rs, torch.Tensor) else rs.size) - 1
  if shared and n_rows != 1:
    raise ValueError("%s: a shared feature has one row, got %d" % (what, n_rows))
  return values, rs, n_rows


def _sharding_sparse_fids(features, feature_cfgs, ps_num, unique, shared_features, batch_size, want_host):
  what = "sharding_sparse_fids"
  if not isinstance(ps_num, int) or isinstance(ps_num, bool):
    raise TypeError("%s: ps_num must be an int, got %r" % (what, ps_num))
  ix = ShardingIndex.of(feature_cfgs, max(ps_num, 1))
  shared_features = set(shared_features)
  unknown = sorted((set(features) | shared_features) - set(ix.feature_names))
  if unknown:
    raise _lib.InvalidArgumentError(_lib.MHTE_INVALID_ARGUMENT,
                                    "%s: no feature config for %s" % (what, ", ".join(unknown)))
  if not features:
    raise ValueError("%s: no features" % what)
  dev, parsed, host_rs, batch = None, {}, [], batch_size
  for name in ix.feature_names:
    if name not in features:
      continue
    shared = name in shared_features
    values, rs, n_rows = _sharding_feature(name, features[name], shared, dev)
    dev = values.device
    if not shared:
      if batch is not None and n_rows != batch:
        raise ValueError("%s: feature %s has %d rows, the batch %d" % (what, name, n_rows, batch))
      batch = n_rows
    if not isinstance(rs, torch.Tensor):
      host_rs.append(rs)
    parsed[name] = (values, rs, n_rows)
  if batch is None:
    raise ValueError("%s: batch_size is needed when every feature is shared" % what)
  # the host row_splits of the call travel in one upload
  rs_dev = torch.from_numpy(np.concatenate(host_rs)).to(dev) if host_rs else None
  F, T = len(ix.feature_names), len(ix.table_names)
  feats = (_lib.ShardFeature * F)()
  n_total = rows = at = 0
  for f, name in enumerate(ix.feature_names):
    x = feats[f]
    x.table_index, x.feature_in_table_index = ix.table_index[f], ix.feature_in_table_index[f]
    x.shared = int(name in shared_features)
    if name not in parsed:
      continue
    values, rs, n_rows = parsed[name]
    x.values, x.n_ids, x.n_rows = values.data_ptr(), values.numel(), n_rows
    if isinstance(rs, torch.Tensor):
      x.row_splits = rs.data_ptr()
    else:
      x.row_splits = rs_dev.data_ptr() + 8 * at
      at += rs.size
    n_total += values.numel()
    rows += n_rows
  n_pre, n_lists = F * max(ps_num, 0), T * max(ps_num, 0)
  fid_offset = torch.empty(n_total, dtype=torch.int64, device=dev)
  feature_offset = torch.empty(rows + 1, dtype=torch.int32, device=dev)
  nfl_offset = torch.empty(F + 1, dtype=torch.int32, device=dev)
  fid_list = torch.empty(n_total, dtype=torch.int64, device=dev)
  key_start = torch.empty(n_pre + 2, dtype=torch.int64, device=dev)
  rs_flat = torch.empty(n_pre + n_lists, dtype=torch.int64, device=dev)
  bounds = torch.empty((n_lists, 2), dtype=torch.int64, device=dev)
  host = np.empty(n_pre + 2, dtype=np.int64) if want_host else None
  tfc = (C.c_int32 * T)(*ix.table_feature_count)
  with torch.cuda.device(dev):
    check(_lib.lib().mhte_sharding_sparse_fids(
        feats, F, tfc, T, ps_num, int(bool(unique)), vp(fid_offset), vp(feature_offset), vp(nfl_offset), vp(fid_list),
        vp(key_start), vp(rs_flat), vp(bounds), None if host is None else host.ctypes.data_as(C.c_void_p), _stream()))
  if _UINT64 is not None and _UINT32 is not None:   # (the bits are the op's; older torch keeps the signed containers)
    fid_offset, nfl_offset = fid_offset.view(_UINT64), nfl_offset.view(_UINT32)
  lists = splits = None
  if host is not None:
    lists, splits = [], []
    for t in range(T):
      for s in range(ps_num):
        lo = s * F + ix.table_first[t]
        ks = host[lo:lo + ix.table_feature_count[t] + 1]
        lists.append(fid_list[int(ks[0]):int(ks[-1])])
        splits.append(np.ascontiguousarray(ks - ks[0]))
  return ShardedFids(fid_offset, feature_offset, nfl_offset, int(batch), lists, splits, fid_list, key_start, rs_flat,
                     bounds, host, ix, ps_num)


def sharding_sparse_fids(features, feature_cfgs: FeatureConfigs, ps_num: int, unique: bool = True,
                         shared_features=(), batch_size: Optional[int] = None) -> ShardedFids:
  """ShardingSparseFids at op version 2 for parsed ids on the device (mhte_sharding_sparse_fids): dedups
  (``unique``) and shards every feature's ids and emits what ``fused_embedding_to_layout`` takes — ``fid_offset``,
  ``feature_offset``, ``nfl_offset`` — beside the fid lists of every (table, shard) with their row_splits
  (index ``table_index * ps_num + shard``, tables and features in sorted-name order).

  ``features``: {feature name: (values, row_splits)} — int64 ids on the GPU, row_splits of batch + 1 entries on
  the host (numpy, as ``Ragged`` carries them) or on the device (int64); a feature named in ``shared_features``
  is a single list: a 1-d tensor, or (values, [0, n]).  A configured feature the batch does not carry has no
  rows.  ``shard = uint64(id) % ps_num``.  Every size comes back in one host read; ``sharding_sparse_fids_plan``
  reads nothing back."""
  return _sharding_sparse_fids(features, feature_cfgs, ps_num, unique, shared_features, batch_size, True)


def sharding_sparse_fids_plan(features, feature_cfgs: FeatureConfigs, ps_num: int, unique: bool = True,
                              shared_features=(), batch_size: Optional[int] = None) -> ShardedFids:
  """``sharding_sparse_fids`` with everything left on the device, for callers who chain on the stream: no wait,
  no host copy — ``fid_list`` / ``fid_list_row_splits`` / ``key_start_host`` are None; the lists are described by
  ``list_bounds`` and ``row_splits_flat``, and ``key_start[-1]`` is the status word (bit 0: invalid row_splits)."""
  return _sharding_sparse_fids(features, feature_cfgs, ps_num, unique, shared_features, batch_size, False)


def lookup_gradient(id_indices: torch.Tensor, id_values: torch.Tensor,
                    input_grads: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
  """MonolithHashTableLookupGradient (runtime/ops/hash_table_lookup_op.cc:110-147): the gradient of a
  lookup gathered back per (batch row, id) pair of a sparse id tensor — ``ids[i] = id_values[i]``,
  ``output_grads[i] = input_grads[id_indices[i, 0]]``.  ``id_indices`` [n, k] int64 (column 0 = the
  batch row), ``id_values`` [n] int64, ``input_grads`` [rows, dim] float32."""
  assert id_indices.dim() == 2 and id_values.dim() == 1 and input_grads.dim() == 2
  if id_indices.shape[0] != id_values.shape[0]:
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT, "id_indices's first dim and id_values dim should be same. Got %dv.s. %d" %
        (id_indices.shape[0], id_values.shape[0]))
  dev = input_grads.device
  idx = id_indices.to(dev, torch.int64).contiguous()
  val = id_values.to(dev, torch.int64).contiguous()
  g = input_grads.to(torch.float32).contiguous()
  n, dim = int(val.numel()), int(g.shape[1])
  out_ids = torch.empty(n, dtype=torch.int64, device=dev)
  out = torch.empty((n, dim), dtype=torch.float32, device=dev)
  _lib.check(_lib.lib().mhte_lookup_gradient(
      _lib.vp(idx), n, idx.shape[1], _lib.vp(val), _lib.vp(g), g.shape[0], dim, _lib.vp(out_ids),
      _lib.vp(out),
      _lib.C.c_void_p(torch.cuda.current_stream().cuda_stream)))
  return out_ids, out


# ---- aligned flat concat / split: the allreduce side of the deferred clip -------------------------------
_WIRE = {torch.float32: 0, torch.float16: 1}


def _numel_of(x) -> int:
  if isinstance(x, torch.Tensor):
    return x.numel()
  n = 1
  for d in x:   # a shape
    n *= int(d)
  return n


def aligned_flat_offsets(numels: List[int], align: int = 16) -> List[int]:
  """FusedAlignedOutputAllocator's rule (runtime/ops/alloc_utils.h:50-95): ``n + 1`` offsets in elements,
  tensor i starts at the sum of ``round_up(numels[j], align)`` over j < i, the last entry is the aligned
  total.  ``align`` is in elements, a power of two in [4, 1024]; the default of 16 floats is the 64-byte
  EIGEN_MAX_ALIGN_BYTES / sizeof(float) of TF's builds (the reference's value depends on its build)."""
  n = len(numels)
  lens = (C.c_int64 * max(n, 1))(*[int(v) for v in numels])
  offs = (C.c_int64 * (n + 1))()
  check(_lib.lib().mhte_aligned_flat_offsets(lens, n, int(align), offs))
  return list(offs)


def aligned_flat_concat(tensors: List[torch.Tensor], scale=1.0, wire_dtype: torch.dtype = torch.float32,
                        align: int = 16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
  """MonolithAlignedFlatConcat (runtime/ops/aligned_concat_split.cu.cc:32-57, :63-109): the flattened tensors
  times ``scale`` in one flat buffer, every tensor's start aligned to ``align`` elements
  (``aligned_flat_offsets``), the padding +0 — one launch.  ``scale``: a Python float, or a 0-d float32
  device tensor (``clip_ops.global_norm_and_scale``) that is read on the device.  ``wire_dtype``
  torch.float16 rounds every product to nearest-even on the way out (the FP16Compressor of the reference's
  allreduce; values beyond 65504 become inf).  ``out``: a 1-d contiguous buffer of ``wire_dtype`` with the
  aligned total's elements to fill instead of a new one."""
  if not isinstance(tensors, list):
    raise TypeError("tensors should be a list")
  if wire_dtype not in _WIRE:
    raise TypeError("aligned_flat_concat: wire_dtype must be torch.float32 or torch.float16")
  ins = []
  for t in tensors:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
      raise TypeError("aligned_flat_concat: the tensors must be float32 tensors on the GPU")
    ins.append(t if t.is_contiguous() else t.contiguous())
  if not ins and out is None:
    raise ValueError("aligned_flat_concat: an empty list has no device to keep the result on")
  n = len(ins)
  total = aligned_flat_offsets([t.numel() for t in ins], align)[-1]
  if out is None:
    out = torch.empty(total, dtype=wire_dtype, device=ins[0].device)
  elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == wire_dtype and out.dim() == 1 and
            out.is_contiguous() and out.numel() == total):
    raise ValueError("aligned_flat_concat: out must be a contiguous 1-d %s tensor on the GPU with %d elements" %
                     (wire_dtype, total))
  pin = (C.c_void_p * max(n, 1))(*[C.c_void_p(t.data_ptr()) for t in ins])
  lens = (C.c_int64 * max(n, 1))(*[t.numel() for t in ins])
  if isinstance(scale, torch.Tensor):
    if not (scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1):
      raise TypeError("aligned_flat_concat: scale must be a float or a 0-d float32 tensor on the GPU")
    host, dev = 1.0, vp(scale)
  else:
    host, dev = float(scale), None
  check(_lib.lib().mhte_aligned_flat_concat(pin, lens, n, int(align), host, dev, _WIRE[wire_dtype], vp(out),
                                            total, _stream()))
  return out


def aligned_flat_split(like, flat: torch.Tensor, post_scale: Optional[float] = None,
                       align: int = 16) -> List[torch.Tensor]:
  """MonolithAlignedFlatSplit (runtime/ops/aligned_concat_split.cu.cc:111-128): the tensors of a flat buffer
  with the shapes of ``like`` (tensors, read for their shapes only, or shapes).  A float32 ``flat`` with
  ``post_scale=None`` launches nothing: the results are VIEWS of ``flat`` at ``aligned_flat_offsets``,
  zero-copy as the reference's ``get_slice`` is.  Otherwise one launch computes
  ``float(flat) * post_scale`` first — a float32 ``flat`` in place, a float16 one into a new float32
  buffer (``post_scale=None`` is then 1) — and the results are views of that."""
  if not isinstance(like, (list, tuple)):
    raise TypeError("like should be a list")
  if not (isinstance(flat, torch.Tensor) and flat.dtype in _WIRE and flat.dim() == 1 and flat.is_contiguous()):
    raise TypeError("aligned_flat_split: flat must be a contiguous 1-d float32 or float16 tensor")
  shapes = [tuple(x.shape) if isinstance(x, torch.Tensor) else tuple(int(d) for d in x) for x in like]
  offs = aligned_flat_offsets([_numel_of(s) for s in shapes], align)
  if flat.numel() != offs[-1]:
    raise ValueError("aligned_flat_split: flat has %d elements, the shapes need %d" % (flat.numel(), offs[-1]))
  if flat.dtype != torch.float32 or post_scale is not None:
    if not flat.is_cuda:
      raise TypeError("aligned_flat_split: decoding needs a flat buffer on the GPU")
    dst = flat if flat.dtype == torch.float32 else torch.empty(flat.numel(), dtype=torch.float32, device=flat.device)
    check(_lib.lib().mhte_aligned_flat_decode(vp(flat), _WIRE[flat.dtype], flat.numel(),
                                              1.0 if post_scale is None else float(post_scale), vp(dst), _stream()))
    flat = dst
  return [flat[o:o + _numel_of(s)].view(s) for o, s in zip(offs, shapes)]


# ---- split by indices: the shard split of the parameter-server path --------------------------------------
# (reference distribution_ops.py:27-78, :175-190; runtime/ops/split_by_indices_op.cc:28-118, :188-243)
# mhte_split_launch_counts' order
SPLIT_COUNTER_NAMES = ("rows/vec1", "rows/vec4", "gradient/vec1", "gradient/vec4", "plan", "plan/ragged")
_SPLIT_ELEM_BYTES = {torch.float32: 4, torch.int64: 8}


class SplitPlan(NamedTuple):
  pos: torch.Tensor                         # int64 [n]: the stable permutation, split after split; -1 behind the last
  sizes: torch.Tensor                       # int64 [num_splits]
  split_row_splits: Optional[torch.Tensor]  # int64 [num_splits, T + 1] when row_splits were given
  n_bad: torch.Tensor                       # int64 [1]: the indices outside [0, num_splits)


def split_launch_counts():
  """{form: launches of this process} (mhte_split_launch_counts): which mover ran, how many plans."""
  out = (C.c_int64 * len(SPLIT_COUNTER_NAMES))()
  check(_lib.lib().mhte_split_launch_counts(out, len(SPLIT_COUNTER_NAMES)))
  return dict(zip(SPLIT_COUNTER_NAMES, [int(x) for x in out]))


def _split_indices(what, indices, num_splits):
  if not isinstance(num_splits, int) or isinstance(num_splits, bool):
    raise TypeError("%s: num_splits must be an int, got %r" % (what, num_splits))
  if not isinstance(indices, torch.Tensor):
    raise TypeError("%s: indices must be a torch tensor, got %s" % (what, type(indices).__name__))
  if indices.dtype != torch.int64:
    raise TypeError("%s: indices must be int64, got %s" % (what, indices.dtype))
  if not indices.is_cuda:
    raise TypeError("%s: indices must be on the GPU (there is no CPU path)" % what)
  return indices.reshape(-1).contiguous()


def _checked_row_splits(row_splits, n):
  rs = np.ascontiguousarray(row_splits, dtype=np.int64).reshape(-1)
  if rs.size < 1 or rs[0] != 0 or rs[-1] != n or (np.diff(rs) < 0).any():
    raise _lib.InvalidArgumentError(_lib.MHTE_INVALID_ARGUMENT, "The input ragged tensor is invalid.")
  return rs


def _plan(indices, num_splits, row_splits, want_host):
  """-> (SplitPlan, host array sizes | split_row_splits | n_bad or None); ``indices`` checked and flat."""
  n, dev = indices.numel(), indices.device
  R = 0 if row_splits is None else row_splits.size
  pos = torch.empty(n, dtype=torch.int64, device=dev)
  sizes = torch.empty(max(num_splits, 0), dtype=torch.int64, device=dev)
  srs = torch.empty((max(num_splits, 0), R), dtype=torch.int64, device=dev) if R else None
  n_bad = torch.empty(1, dtype=torch.int64, device=dev)
  host = np.empty(max(num_splits, 0) * (1 + R) + 1, dtype=np.int64) if want_host else None
  with torch.cuda.device(dev):
    check(_lib.lib().mhte_split_plan(vp(indices), n, num_splits,
                                     None if row_splits is None else row_splits.ctypes.data_as(C.c_void_p), R,
                                     vp(pos), vp(sizes), vp(srs), vp(n_bad),
                                     None if host is None else host.ctypes.data_as(C.c_void_p), _stream()))
  return SplitPlan(pos, sizes, srs, n_bad), host


def split_plan(indices: torch.Tensor, num_splits: int, row_splits=None) -> SplitPlan:
  """The partition behind ``split_by_indices`` / ``ragged_split_by_indices`` with everything left on the device
  (mhte_split_plan): nothing is read back and nothing waits, for callers who chain on the stream.  ``row_splits``:
  the host boundaries of a ragged input; the plan then carries every split's row_splits as a device table."""
  indices = _split_indices("split_plan", indices, num_splits)
  rs = None if row_splits is None else _checked_row_splits(row_splits, indices.numel())
  return _plan(indices, num_splits, rs, False)[0]


def _bad_indices(what, n_bad, num_splits):
  if n_bad:
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT, "%s: %d indices are outside [0, %d)" % (what, n_bad, num_splits))


def _move_rows(tensor, pos):
  """packed[q] = tensor[pos[q]] (mhte_split_rows); ``tensor`` contiguous, its first dim = len(pos)."""
  n = pos.numel()
  packed = torch.empty_like(tensor)
  if n:
    with torch.cuda.device(tensor.device):
      check(_lib.lib().mhte_split_rows(vp(tensor), n, tensor.numel() // n, _SPLIT_ELEM_BYTES[tensor.dtype], vp(pos),
                                       vp(packed), _stream()))
  return packed


def _cut(packed, sizes):
  out, off = [], 0
  for s in sizes:
    out.append(packed[off:off + int(s)])
    off += int(s)
  return out


def _split_forward(indices, tensor, num_splits):
  what = "split_by_indices"
  indices = _split_indices(what, indices, num_splits)
  if not isinstance(tensor, torch.Tensor):
    raise TypeError("%s: tensor must be a torch tensor, got %s" % (what, type(tensor).__name__))
  if tensor.dtype not in _SPLIT_ELEM_BYTES:
    raise TypeError("%s: tensor must be float32 or int64, got %s" % (what, tensor.dtype))
  if not tensor.is_cuda:
    raise TypeError("%s: tensor must be on the GPU (there is no CPU path)" % what)
  if tensor.device != indices.device:
    raise ValueError("%s: tensor is on %s, indices on %s" % (what, tensor.device, indices.device))
  n = indices.numel()
  if tensor.dim() < 1 or tensor.shape[0] != n or (n and tensor.numel() == 0):
    raise ValueError("%s: tensor must hold one non-empty element per index: shape %s, %d indices" %
                     (what, tuple(tensor.shape), n))
  tensor = tensor if tensor.is_contiguous() else tensor.contiguous()
  plan, host = _plan(indices, num_splits, None, True)
  _bad_indices(what, int(host[-1]), num_splits)
  sizes = [int(s) for s in host[:num_splits]]
  return _cut(_move_rows(tensor, plan.pos), sizes), plan, sizes


class _SplitByIndices(torch.autograd.Function):
  """reference distribution_ops.py:37-43: the registered gradient is MonolithSplitByIndicesGradient."""

  @staticmethod
  def forward(ctx, indices, tensor, num_splits):
    splits, plan, sizes = _split_forward(indices, tensor, num_splits)
    ctx.save_for_backward(plan.pos, plan.sizes)
    ctx.sizes, ctx.shape = sizes, tuple(tensor.shape)
    return tuple(splits)

  @staticmethod
  def backward(ctx, *grads):
    pos, sizes_dev = ctx.saved_tensors
    n, shape = pos.numel(), ctx.shape
    out = torch.empty(shape, dtype=torch.float32, device=pos.device)
    if n == 0:
      return None, out, None
    gs = []
    for g, s in zip(grads, ctx.sizes):
      want = (s,) + shape[1:]
      if g is None:
        g = torch.zeros(want, dtype=torch.float32, device=pos.device)
      if tuple(g.shape) != want:
        raise ValueError("split_by_indices: a gradient of shape %s for a split of shape %s" % (tuple(g.shape), want))
      gs.append(g.to(dtype=torch.float32).contiguous())
    with torch.cuda.device(pos.device):
      check(_lib.lib().mhte_split_rows_grad(_ptr_array(gs), vp(sizes_dev), len(gs), n, out.numel() // n, 4, vp(pos),
                                            vp(out), _stream()))
    return None, out, None


def split_by_indices(indices: torch.Tensor, tensor: torch.Tensor, num_splits: int) -> List[torch.Tensor]:
  """reference distribution_ops.py:27-34 (MonolithSplitByIndices, split_by_indices_op.cc:28-75): split the elements
  of ``tensor`` (float32 or int64, one per index along its first dim, any trailing shape) into ``num_splits``
  tensors by ``indices``; inside a split the elements keep their input order.  The results are views of one
  packed buffer.  A float32 tensor is differentiable (MonolithSplitByIndicesGradient).  The sizes come back to
  the host, which is where the shapes of the results live; an index outside [0, num_splits) is an
  InvalidArgumentError."""
  if isinstance(tensor, torch.Tensor) and tensor.dtype == torch.float32:
    return list(_SplitByIndices.apply(indices, tensor, num_splits))
  return _split_forward(indices, tensor, num_splits)[0]


def ragged_split_by_indices(indices: torch.Tensor, num: Ragged,
                            num_splits: int) -> Tuple[List[Ragged], List[Ragged]]:
  """reference distribution_ops.py:46-78 (MonolithRaggedSplitByIndices, split_by_indices_op.cc:188-243): split an
  int64 ragged tensor into ``num_splits`` ragged tensors by ``indices``; returns the split ragged tensors and the
  original position of every number.  For example,
    indices = [0, 1, 0, 1], num = [[4, 3, 2], [1]], num_splits = 2
    ===> [[[4, 2], []], [[3], [1]]],  [[[0, 2], []], [[1], [3]]]
  Values and positions stay on the device; every split's row_splits is on the host."""
  what = "ragged_split_by_indices"
  indices = _split_indices(what, indices, num_splits)
  values = num.values
  if not (isinstance(values, torch.Tensor) and values.dtype == torch.int64 and values.is_cuda):
    raise TypeError("%s: num.values must be an int64 tensor on the GPU (there is no CPU path)" % what)
  values = values.reshape(-1).contiguous()
  if values.numel() != indices.numel():
    raise _lib.InvalidArgumentError(
        _lib.MHTE_INVALID_ARGUMENT, "Ragged tensor values size must match indices size. Got %d v.s. %d" %
        (values.numel(), indices.numel()))
  rs = _checked_row_splits(num.row_splits, indices.numel())
  plan, host = _plan(indices, num_splits, rs, True)
  _bad_indices(what, int(host[-1]), num_splits)
  sizes = [int(s) for s in host[:num_splits]]
  table = host[num_splits:num_splits + num_splits * rs.size].reshape(num_splits, rs.size)
  vals, poss = _cut(_move_rows(values, plan.pos), sizes), _cut(plan.pos, sizes)
  splits = [np.ascontiguousarray(table[s]) for s in range(num_splits)]
  return ([Ragged(v, r) for v, r in zip(vals, splits)], [Ragged(p, r) for p, r in zip(poss, splits)])


def finalize_shared_tensor(shared_tensor_handles: List[torch.Tensor], dtype=None, shape=None) -> torch.Tensor:
  """reference distribution_ops.py:175-190: the shared buffer the fills wrote into.  ``fill_with_offset_map``
  returns the buffer it was given, so the handles must all be that one tensor (the *same handle* repeated); the
  list only carries the fills' order.  ``dtype`` / ``shape`` (None entries: unknown) are checked against it."""
  if not isinstance(shared_tensor_handles, (list, tuple)) or not shared_tensor_handles:
    raise ValueError("finalize_shared_tensor: needs a non-empty list of handles")
  first = shared_tensor_handles[0]
  for h in shared_tensor_handles:
    if not isinstance(h, torch.Tensor):
      raise TypeError("finalize_shared_tensor: a handle must be a torch tensor, got %s" % type(h).__name__)
    if (h.data_ptr() != first.data_ptr() or h.numel() != first.numel() or h.dtype != first.dtype or
        h.device != first.device):
      raise _lib.InvalidArgumentError(_lib.MHTE_INVALID_ARGUMENT,
                                      "finalize_shared_tensor: the handles are not the same shared tensor")
  if dtype is not None and first.dtype != dtype:
    raise TypeError("finalize_shared_tensor: the shared tensor is %s, not %s" % (first.dtype, dtype))
  if shape is not None:
    first = first.reshape([-1 if d is None else int(d) for d in shape])
  return first
