"""Layer ops on MI355X — host-side mirror of monolith/native_training/layers/layer_ops.py (:24-46).

``ffm`` is the feature cross of the GroupInt / FFM layer (``feature_cross.GroupInt``): every feature of the left
group against every feature of the right group, as the element-wise product (``'multiply'``, ``[B, L R D]``) or
its sum over the embedding dimension (``'dot'``, ``[B, L R]``).  Forward and gradient are one launch each of the
hand-written kernels behind ``mhte_ffm`` / ``mhte_ffm_grad`` (include/monolith_amd_hash_table.h,
csrc/mhte_ffm_kernels.h): a fixed tree of individually rounded fp32 operations, the reference's per-element order,
the same bits on every run.  No function of this module waits for the GPU or reads a device value, so forward and
backward can be captured into a graph.

``feature_insight`` is the other op of that module with a registered gradient (layer_ops.py:49-85): the
block-diagonal product of the concatenated embeddings ``[B, E]`` with the first dense layer's kernel ``[E, K]``, one
block per feature (``segment_sizes``), ``[B, F K]``; its gradient ``feature_insight_grad``; and, with
``aggregate=True``, the per-feature sum of squares ``[B, F]``, which one fused kernel computes without the
``[B, F K]`` intermediate.  They sit behind ``mhte_feature_insight`` / ``mhte_feature_insight_grad``
(csrc/mhte_fi_kernels.h): exact fp32 ``fmaf`` chains in a fixed order, no atomics, the same bits on every run.

Tensors are 2-D float32 on the GPU; a tensor that is not contiguous is copied first.
"""
import ctypes as C
from typing import Optional, Sequence, Tuple

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


# ---- FeatureInsight (layer_ops.py:49-85) ------------------------------------------------------------------------
# mhte_feature_insight_launch_counts' order
FI_COUNTER_NAMES = ("forward", "aggregate", "input_grad", "weight_grad", "slab_sum")
# mhte_feature_insight_plan's order
FI_PLAN_NAMES = ("row_block", "column_tile", "stage", "inline_segments", "groups", "slab_rows", "slabs",
                 "forward_workspace_bytes", "grad_workspace_bytes")


def _fi_sizes(what, segment_sizes):
  """-> the list as a ctypes int32 array (layer_ops.py:53: ``assert segment_sizes``)."""
  try:
    sizes = list(segment_sizes)
  except TypeError:
    raise TypeError("%s: segment_sizes must be a sequence of ints, got %s" % (what, type(segment_sizes).__name__))
  if not sizes:
    raise ValueError("%s: segment_sizes must not be empty" % what)
  for v in sizes:
    if not isinstance(v, int) or isinstance(v, bool):
      raise TypeError("%s: segment_sizes must hold ints, got %r" % (what, v))
    if not -2 ** 31 <= v < 2 ** 31:
      raise ValueError("%s: segment_sizes must hold 32-bit ints, got %r" % (what, v))
  return (C.c_int32 * len(sizes))(*sizes), len(sizes)


def _fi_operands(what, **tensors):
  """Checked and contiguous, in the order given; ``weight`` comes last."""
  out = []
  first = None
  for name, t in tensors.items():
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
    if t.dtype != torch.float32:
      raise TypeError("%s: %s must be float32, got %s" % (what, name, t.dtype))
    if t.dim() != 2:
      raise ValueError("%s: %s is not 2D (shape %s)" % (what, name, tuple(t.shape)))
    if first is None:
      first = (name, t)
    elif t.device != first[1].device:
      raise ValueError("%s: %s is on %s, %s on %s" % (what, name, t.device, first[0], first[1].device))
    out.append(t)
  inp, weight = tensors["input_embedding"], tensors["weight"]
  if inp.shape[1] != weight.shape[0]:   # layer_ops.py:54
    raise ValueError("%s: the columns of input_embedding and the rows of weight do not match (%d, %d)" %
                     (what, inp.shape[1], weight.shape[0]))
  if "grad" in tensors and tensors["grad"].shape[0] != inp.shape[0]:
    raise ValueError("%s: the batch size of grad and input_embedding do not match (%d, %d)" %
                     (what, tensors["grad"].shape[0], inp.shape[0]))
  for name, t in tensors.items():
    if not t.is_cuda:
      raise TypeError("%s: %s must be on the GPU (there is no CPU path)" % (what, name))
  return [t if t.is_contiguous() else t.contiguous() for t in out]


def _fi_forward(input_embedding, weight, segment_sizes, aggregate):
  sizes, nseg = _fi_sizes("feature_insight", segment_sizes)
  inp, w = _fi_operands("feature_insight", input_embedding=input_embedding, weight=weight)
  cols = nseg if aggregate else nseg * w.shape[1]
  out = torch.empty((inp.shape[0], cols), dtype=torch.float32, device=inp.device)
  with torch.cuda.device(inp.device):
    check(_lib.lib().mhte_feature_insight(vp(inp), vp(w), inp.shape[0], inp.shape[1], w.shape[1], sizes, nseg,
                                          int(aggregate), vp(out), cols, _stream()))
  return out, inp, w


def feature_insight_grad(grad: torch.Tensor, input_embedding: torch.Tensor, weight: torch.Tensor,
                         segment_sizes: Sequence[int], want_input: bool = True,
                         want_weight: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
  """The op FeatureInsightGrad -> (input_embedding_grad, weight_grad), shaped like their operands; ``grad`` is
  ``[B, F K]``.  A gradient that is not wanted is ``None``; asking for one alone gives the same bits as asking for
  both."""
  what = "feature_insight_grad"
  if not (want_input or want_weight):
    raise ValueError("%s: at least one of want_input and want_weight" % what)
  sizes, nseg = _fi_sizes(what, segment_sizes)
  grad, inp, w = _fi_operands(what, grad=grad, input_embedding=input_embedding, weight=weight)
  input_grad = torch.empty_like(inp) if want_input else None
  weight_grad = torch.empty_like(w) if want_weight else None
  with torch.cuda.device(inp.device):
    check(_lib.lib().mhte_feature_insight_grad(vp(grad), grad.shape[1], vp(inp), vp(w), inp.shape[0], inp.shape[1],
                                               w.shape[1], sizes, nseg,
                                               vp(input_grad) if want_input else None,
                                               vp(weight_grad) if want_weight else None, _stream()))
  return input_grad, weight_grad


class _FeatureInsight(torch.autograd.Function):
  """layer_ops.py:74-85: the registered gradient of FeatureInsight is FeatureInsightGrad of the op's own inputs."""

  @staticmethod
  def forward(ctx, input_embedding, weight, segment_sizes):
    out, inp, w = _fi_forward(input_embedding, weight, segment_sizes, False)
    ctx.save_for_backward(inp, w)
    ctx.segment_sizes = list(segment_sizes)
    return out

  @staticmethod
  def backward(ctx, grad):
    inp, w = ctx.saved_tensors
    input_grad, weight_grad = feature_insight_grad(grad, inp, w, ctx.segment_sizes, ctx.needs_input_grad[0],
                                                   ctx.needs_input_grad[1])
    return input_grad, weight_grad, None


def feature_insight(input_embedding: torch.Tensor, weight: torch.Tensor, segment_sizes: Sequence[int],
                    aggregate: bool = False) -> torch.Tensor:
  """The op FeatureInsight (layer_ops.py:49-71).  ``input_embedding`` ``[B, E]``, ``weight`` ``[E, K]``,
  ``segment_sizes`` F ints whose sum is E -> ``[B, F K]``, differentiable in both operands; with ``aggregate``
  -> ``[B, F]``, the sum over each feature's K columns of the squared output.

  ``aggregate=True`` takes the fused kernel (no ``[B, F K]`` intermediate, no workspace) when neither operand
  requires a gradient or gradients are disabled.  Otherwise it is the plain op followed by the torch square and
  sum: the reference's own composition, differentiable through the op's gradient.  The two forms agree within the
  rounding of the K-term sum, not in bits.  The reference's only caller of this form writes a summary and never
  differentiates."""
  if not isinstance(aggregate, (bool, int)) or aggregate not in (0, 1):
    raise TypeError("feature_insight: aggregate must be a bool, got %r" % (aggregate,))
  if not aggregate:
    _fi_sizes("feature_insight", segment_sizes)
    _fi_operands("feature_insight", input_embedding=input_embedding, weight=weight)
    return _FeatureInsight.apply(input_embedding, weight, list(segment_sizes))
  needs_grad = torch.is_grad_enabled() and isinstance(input_embedding, torch.Tensor) and \
      isinstance(weight, torch.Tensor) and (input_embedding.requires_grad or weight.requires_grad)
  if not needs_grad:
    return _fi_forward(input_embedding, weight, segment_sizes, True)[0]
  out = feature_insight(input_embedding, weight, segment_sizes, False)
  return (out * out).view(out.shape[0], len(segment_sizes), weight.shape[1]).sum(dim=2)


def feature_insight_plan(B: int, E: int, K: int, F: int):
  """{row_block, column_tile, stage, inline_segments, groups, slab_rows, slabs, forward_workspace_bytes,
  grad_workspace_bytes} of a call (mhte_feature_insight_plan): a function of the shape alone, no device needed."""
  out = (C.c_int64 * len(FI_PLAN_NAMES))()
  check(_lib.lib().mhte_feature_insight_plan(int(B), int(E), int(K), int(F), out, len(FI_PLAN_NAMES)))
  return dict(zip(FI_PLAN_NAMES, [int(x) for x in out]))


def feature_insight_launch_counts():
  """{form: launches of this process} (mhte_feature_insight_launch_counts)."""
  out = (C.c_int64 * len(FI_COUNTER_NAMES))()
  check(_lib.lib().mhte_feature_insight_launch_counts(out, len(FI_COUNTER_NAMES)))
  return dict(zip(FI_COUNTER_NAMES, [int(x) for x in out]))
