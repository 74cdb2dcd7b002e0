"""Layer ops on MI355X — host-side mirror of monolith/native_training/layers/layer_ops.py (:24-46).

``ffm`` is the feature cross of the GroupInt / FFM layer (``feature_cross.GroupInt``): every feature of the left
group against every feature of the right group, as the element-wise product (``'multiply'``, ``[B, L R D]``) or
its sum over the embedding dimension (``'dot'``, ``[B, L R]``).  Forward and gradient are one launch each of the
hand-written kernels behind ``mhte_ffm`` / ``mhte_ffm_grad`` (include/monolith_amd_hash_table.h,
csrc/mhte_ffm_kernels.h): a fixed tree of individually rounded fp32 operations, the reference's per-element order,
the same bits on every run.  No function of this module waits for the GPU or reads a device value, so forward and
backward can be captured into a graph.

Tensors are 2-D float32 on the GPU; a tensor that is not contiguous is copied first.
"""
import ctypes as C
from typing import Tuple

import torch

from monolith_amd import _lib
from monolith_amd._lib import check, vp
from monolith_amd.multi_hash_table_ops import _stream

INT_TYPES = ("multiply", "dot")   # the set GroupInt admits (feature_cross.py:80); the index is the ABI's int_type

# mhte_ffm_launch_counts' order: kernel, interaction, lane shape, where the operands are read from
COUNTER_NAMES = tuple("%s/%s/%s/%s" % (k, i, v, f) for k in ("forward", "gradient") for i in INT_TYPES
                      for v in ("vec4", "vec1") for f in ("lds", "direct"))


def _int_type(int_type) -> int:
  if int_type not in INT_TYPES:
    raise ValueError("ffm: int_type must be 'multiply' or 'dot', got %r" % (int_type,))
  return INT_TYPES.index(int_type)


def _operands(what, dim_size, **tensors):
  """Checked and contiguous, in the order given."""
  if not isinstance(dim_size, int) or isinstance(dim_size, bool) or dim_size < 1:
    raise ValueError("%s: dim_size must be an int >= 1, got %r" % (what, dim_size))
  first = None
  out = []
  for name, t in tensors.items():
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
    if t.dtype != torch.float32:
      raise TypeError("%s: %s must be float32, got %s" % (what, name, t.dtype))
    if t.dim() != 2:
      raise ValueError("%s: the %s tensor of ffm is not 2D (shape %s)" % (what, name, tuple(t.shape)))
    if first is None:
      first = (name, t)
    else:
      if t.device != first[1].device:
        raise ValueError("%s: %s is on %s, %s on %s" % (what, name, t.device, first[0], first[1].device))
      if t.shape[0] != first[1].shape[0]:
        raise ValueError("%s: the batch size of %s and %s tensor are not match (%d, %d)" %
                         (what, first[0], name, first[1].shape[0], t.shape[0]))
    out.append(t)
  for name, t in tensors.items():
    if not t.is_cuda:
      raise TypeError("%s: %s must be on the GPU (there is no CPU path)" % (what, name))
  return [t if t.is_contiguous() else t.contiguous() for t in out]


def _ffm_forward(left, right, dim_size, int_type):
  it = _int_type(int_type)
  left, right = _operands("ffm", dim_size, left=left, right=right)
  nl, nr = left.shape[1] // dim_size, right.shape[1] // dim_size
  cols = nl * nr if it else nl * nr * dim_size
  out = torch.empty((left.shape[0], cols), dtype=torch.float32, device=left.device)
  with torch.cuda.device(left.device):
    check(_lib.lib().mhte_ffm(vp(left), left.shape[1], vp(right), right.shape[1], left.shape[0], dim_size, it,
                              vp(out), cols, _stream()))
  return out, left, right


def ffm_grad(grad: torch.Tensor, left: torch.Tensor, right: torch.Tensor, dim_size: int,
             int_type: str = "multiply") -> Tuple[torch.Tensor, torch.Tensor]:
  """The op FFMGrad -> (left_grad, right_grad), shaped like ``left`` and ``right`` (columns beyond the last whole
  feature hold +0).  ``grad`` is ``[B, L R D]`` for ``'multiply'`` and ``[B, L R]`` for ``'dot'``; another number
  of features is refused ("the in/out shape not match")."""
  it = _int_type(int_type)
  grad, left, right = _operands("ffm_grad", dim_size, grad=grad, left=left, right=right)
  left_grad, right_grad = torch.empty_like(left), torch.empty_like(right)
  with torch.cuda.device(left.device):
    check(_lib.lib().mhte_ffm_grad(vp(grad), grad.shape[1], vp(left), left.shape[1], vp(right), right.shape[1],
                                   left.shape[0], dim_size, it, vp(left_grad), vp(right_grad), _stream()))
  return left_grad, right_grad


class _Ffm(torch.autograd.Function):
  """layer_ops.py:35-46: the registered gradient of FFM is FFMGrad of the op's own inputs."""

  @staticmethod
  def forward(ctx, left, right, dim_size, int_type):
    out, left_c, right_c = _ffm_forward(left, right, dim_size, int_type)
    ctx.save_for_backward(left_c, right_c)
    ctx.dim_size, ctx.int_type = dim_size, int_type
    return out

  @staticmethod
  def backward(ctx, grad):
    left, right = ctx.saved_tensors
    left_grad, right_grad = ffm_grad(grad, left, right, ctx.dim_size, ctx.int_type)
    return left_grad, right_grad, None, None


def ffm(left: torch.Tensor, right: torch.Tensor, dim_size: int, int_type: str = "multiply") -> torch.Tensor:
  """The op FFM (layer_ops.py:24-32).  ``left`` ``[B, L * dim_size]``, ``right`` ``[B, R * dim_size]`` ->
  ``[B, L * R * dim_size]`` (``'multiply'``) or ``[B, L * R]`` (``'dot'``); differentiable in both operands."""
  _int_type(int_type)
  return _Ffm.apply(left, right, dim_size, int_type)


def ffm_launch_counts():
  """{form: launches of this process} (mhte_ffm_launch_counts): which kernel instantiation a shape reached."""
  out = (C.c_int64 * len(COUNTER_NAMES))()
  check(_lib.lib().mhte_ffm_launch_counts(out, len(COUNTER_NAMES)))
  return dict(zip(COUNTER_NAMES, [int(x) for x in out]))
