"""The gradient clip and the dense allreduce of a training step on MI355X — host-side mirror of the part of
monolith/native_training/feature_utils.py that sits between ``compute_gradients`` and the optimizers:
``allreduce_cond`` (reference :48-99, fusion ``'one'``) and the clip / allreduce order of
``apply_gradients_with_var_optimizer`` (reference :209-270).

In synchronous GPU training the reference does not clip the dense gradients where it computes their norm: it
keeps ``scale = min(clip_norm / norm, 1)`` as a tensor (``cond_defer_clip``, :251-260) and hands it to
``MonolithAlignedFlatConcat``, which multiplies while it packs all dense gradients into one aligned flat
buffer; one allreduce (average) runs over that buffer, optionally cast to fp16 (``enable_allreduce_fp16``),
and ``MonolithAlignedFlatSplit`` cuts the result back into the gradients' shapes without a copy.  The same
scale goes to the sparse side (``fused_gather_embeddings_by_input_gradient(scale=...)``,
``clip_ops.scale_tensors``).  Here the norm, the scale, the concat and the way back are device work only
(``clip_ops``, ``distribution_ops.aligned_flat_concat`` / ``aligned_flat_split``): no function of this module
waits for the GPU or reads a device value.

The collective itself is the caller's: ``torch.distributed.all_reduce`` by default, any callable otherwise.

``clip_allreduce_and_apply`` goes one step further, to the reference's ``var_opt.apply_gradients``: the dense
optimizers of ``monolith_amd.optimizers`` read the flat buffer where the allreduce left it (or the gradient
list with the deferred scale), so neither a clipped nor a decoded copy of the gradients is written.

fp16 on the wire: every product is rounded to fp16 before the ranks' buffers are added, and the SUM is formed
in fp16 by the collective — it overflows to inf beyond 65504 although the average would fit, and gradients
below 6e-8 vanish.  That is the reference's behaviour too (its FP16Compressor casts before the allreduce);
the clip bounds the norm of one rank's gradients, not the sum over the ranks.

Not restated: the ``'grouped'`` fusion and the un-fused allreduce of the reference, ``ClipByNorm`` and
``ClipByValue``, the norm warm-up, and the summaries.
"""
import enum
from typing import Callable, List, Optional, Tuple

import torch

from monolith_amd import clip_ops
from monolith_amd import distribution_ops


class GradClipType(enum.Enum):
  """feature_utils.GradClipType (reference :102-107)."""
  ClipByNorm = 1
  ClipByGlobalNorm = 2
  ClipByValue = 3
  ClipByDenseAndSparse = 4
  NoClip = 5


def _world_of(group) -> int:
  import torch.distributed as dist  # pylint: disable=import-outside-toplevel
  if dist.is_available() and dist.is_initialized():
    return dist.get_world_size(group)
  return 1


def allreduce_cond(grads: List[Optional[torch.Tensor]], scale=1, fp16: bool = False, group=None,
                   allreduce: Optional[Callable[[torch.Tensor], Optional[torch.Tensor]]] = None,
                   world: Optional[int] = None, align: int = 16) -> List[Optional[torch.Tensor]]:
  """feature_utils.allreduce_cond with fusion ``'one'`` (reference :48-81): the average over the ranks of
  ``grad * scale`` for every gradient of the list.  ``None`` entries keep their places (``map_to_output``),
  and a list of ``None`` only is returned as it is.

  concat (``scale`` applied, fp16 wire when ``fp16``) -> ``allreduce(flat)`` -> split with
  ``post_scale = 1 / world``.  ``scale``: a Python number or a 0-d float32 device tensor.  ``allreduce``
  takes the flat buffer and sums it over the ranks, in place or into the buffer it returns; the default is
  ``torch.distributed.all_reduce(flat, SUM, group)``.  ``world`` defaults to the group's size; with
  ``torch.distributed`` not initialised it is 1 and there is no collective.  With one rank and an fp32 wire
  the results are views of the concat's buffer and nothing else is launched (a factor of exactly 1)."""
  wo_none = [g for g in grads if g is not None]
  if not wo_none:
    return grads
  if world is None:
    world = _world_of(group)
  world = int(world)
  if world < 1:
    raise ValueError("allreduce_cond: world must be >= 1, got %d" % world)
  flat = distribution_ops.aligned_flat_concat(wo_none, scale=scale,
                                              wire_dtype=torch.float16 if fp16 else torch.float32, align=align)
  if allreduce is not None:
    reduced = allreduce(flat)
    flat = flat if reduced is None else reduced
  elif world > 1:
    import torch.distributed as dist  # pylint: disable=import-outside-toplevel
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
  post_scale = None if world == 1 else 1.0 / world
  reduced = distribution_ops.aligned_flat_split(wo_none, flat, post_scale=post_scale, align=align)
  it = iter(reduced)
  return [None if g is None else next(it) for g in grads]


def _device_of(tensors) -> torch.device:
  for t in tensors:
    if t is not None:
      return t.device
  return torch.device("cuda")


def _norms_and_scales(dense_grads, sparse_grads, clip_type, clip_norm, sparse_clip_norm):
  """The norms of apply_gradients_with_var_optimizer (reference :211-234) -> ``(dense_norm, dense_scale,
  sparse_scale)``: 0-d device tensors; the dense pair is ``None`` where nothing clips the dense side."""
  if not isinstance(clip_type, GradClipType):
    raise TypeError("clip_type must be a GradClipType")
  if clip_type in (GradClipType.ClipByNorm, GradClipType.ClipByValue):
    raise NotImplementedError("clip_and_allreduce: %s is not restated here" % clip_type.name)
  dense = [g for g in dense_grads if g is not None]
  sparse = [g for g in sparse_grads if g is not None]
  dense_norm = dense_scale = sparse_scale = None
  if clip_type == GradClipType.ClipByGlobalNorm and clip_norm is not None and dense + sparse:
    dense_norm, dense_scale = clip_ops.global_norm_and_scale(dense + sparse, clip_norm)
    sparse_clip_norm = sparse_clip_norm or clip_norm
    if float(sparse_clip_norm) == float(clip_norm):
      sparse_scale = dense_scale
    else:   # the same norm against another bound: computed again, on the device
      sparse_scale = clip_ops.global_norm_and_scale(dense + sparse, sparse_clip_norm)[1]
  elif clip_type == GradClipType.ClipByDenseAndSparse:
    if clip_norm is not None and dense:
      dense_norm, dense_scale = clip_ops.global_norm_and_scale(dense, clip_norm)
    if sparse_clip_norm is not None and sparse:
      sparse_scale = clip_ops.global_norm_and_scale(sparse, sparse_clip_norm)[1]
  if sparse_scale is None:
    sparse_scale = torch.ones((), dtype=torch.float32, device=_device_of(list(dense_grads) + list(sparse_grads)))
  return dense_norm, dense_scale, sparse_scale


def clip_and_allreduce(dense_grads: List[Optional[torch.Tensor]], sparse_grads: List[Optional[torch.Tensor]],
                       clip_type: GradClipType = GradClipType.ClipByGlobalNorm,
                       clip_norm: Optional[float] = None, sparse_clip_norm: Optional[float] = None,
                       use_allreduce: bool = False, fp16: bool = False, group=None, allreduce=None,
                       world: Optional[int] = None,
                       align: int = 16) -> Tuple[List[Optional[torch.Tensor]], torch.Tensor]:
  """The clip and the dense allreduce of apply_gradients_with_var_optimizer (reference :209-270, :298-303)
  -> ``(dense_grads_out, sparse_scale)``.

  * ``ClipByGlobalNorm`` with a ``clip_norm``: ONE norm over dense + sparse gradients (:213-216);
    ``sparse_clip_norm`` defaults to ``clip_norm``.
  * ``ClipByDenseAndSparse``: one norm over the dense gradients, and one over the sparse ones when there is a
    ``sparse_clip_norm`` (:231-234).
  * ``NoClip`` (or no ``clip_norm``): both scales are 1.
  Norm and ``scale = norm > clip ? clip / norm : 1`` come from ``clip_ops.global_norm_and_scale`` and stay on
  the device.  With ``use_allreduce`` the dense clip is deferred (``cond_defer_clip``, :251-260): the scale is
  multiplied in by the concat of ``allreduce_cond``.  Without it the dense gradients are clipped by
  ``clip_ops.clip_by_global_norm`` with that norm and nothing is reduced.  The sparse side is always
  deferred: ``sparse_scale`` is a 0-d float32 device tensor for
  ``distribution_ops.fused_gather_embeddings_by_input_gradient(scale=...)`` and ``clip_ops.scale_tensors``.
  ``None`` gradients keep their places and take no part in a norm."""
  dense_norm, dense_scale, sparse_scale = _norms_and_scales(dense_grads, sparse_grads, clip_type, clip_norm,
                                                            sparse_clip_norm)
  dense = [g for g in dense_grads if g is not None]
  if use_allreduce:
    out = allreduce_cond(dense_grads, scale=1 if dense_scale is None else dense_scale, fp16=fp16, group=group,
                         allreduce=allreduce, world=world, align=align)
  elif dense_norm is not None and dense:
    clipped, _ = clip_ops.clip_by_global_norm(dense, clip_norm, use_norm=dense_norm)
    it = iter(clipped)
    out = [None if g is None else next(it) for g in dense_grads]
  else:
    out = list(dense_grads)
  return out, sparse_scale


def clip_allreduce_and_apply(optimizer, grads_and_vars, sparse_grads: List[Optional[torch.Tensor]],
                             clip_type: GradClipType = GradClipType.ClipByGlobalNorm,
                             clip_norm: Optional[float] = None, sparse_clip_norm: Optional[float] = None,
                             use_allreduce: bool = False, fp16: bool = False, group=None, allreduce=None,
                             world: Optional[int] = None, update_slots: bool = True) -> torch.Tensor:
  """``clip_and_allreduce`` with the dense apply at its end (reference :209-270 down to
  ``var_opt.apply_gradients``) -> ``sparse_scale``.  ``optimizer``: an ``optimizers.AdamomOptimizer`` or
  ``RmspropOptimizer``; ``grads_and_vars``: the dense (gradient, variable) pairs in the optimizer's order.

  Norms and scales as in ``clip_and_allreduce``.  The dense clip is ALWAYS deferred here and no clipped copy
  of the gradients is written:
  * with ``use_allreduce``: concat (the scale multiplied in, fp16 wire when ``fp16``, the optimizer's
    ``align``) -> the collective -> ``optimizer.apply_flat(flat, post_scale=1 / world)``, which reads the
    gradients where the allreduce left them.  Every variable needs a gradient: the flat buffer has the layout
    of the optimizer's slots.
  * without: ``optimizer.apply_gradients(..., grad_scale=dense_scale)``; ``None`` gradients are skipped.
  Both multiply by ``scale = norm > clip_norm ? clip_norm / norm : 1``, as the reference's synchronous path
  does (``cond_defer_clip``).  ``clip_and_allreduce`` without ``use_allreduce`` goes through
  ``clip_by_global_norm``, whose ``t * clip_norm / max(norm, clip_norm)`` rounds differently: the two agree to
  a few ulp, not bit for bit."""
  pairs = list(grads_and_vars)
  dense_grads = [g for g, _ in pairs]
  _, dense_scale, sparse_scale = _norms_and_scales(dense_grads, sparse_grads, clip_type, clip_norm,
                                                   sparse_clip_norm)
  scale = 1.0 if dense_scale is None else dense_scale
  if not use_allreduce:
    optimizer.apply_gradients(pairs, grad_scale=scale, update_slots=update_slots)
    return sparse_scale
  if any(g is None for g in dense_grads):
    raise ValueError("clip_allreduce_and_apply: with use_allreduce every variable needs a gradient")
  if world is None:
    world = _world_of(group)
  world = int(world)
  if world < 1:
    raise ValueError("clip_allreduce_and_apply: world must be >= 1, got %d" % world)
  flat = distribution_ops.aligned_flat_concat(dense_grads, scale=scale,
                                              wire_dtype=torch.float16 if fp16 else torch.float32,
                                              align=optimizer.align)
  if allreduce is not None:
    reduced = allreduce(flat)
    flat = flat if reduced is None else reduced
  elif world > 1:
    import torch.distributed as dist  # pylint: disable=import-outside-toplevel
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
  optimizer.apply_flat(flat, variables=[v for _, v in pairs], post_scale=None if world == 1 else 1.0 / world,
                       update_slots=update_slots)
  return sparse_scale
