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

``cin_layer`` is one layer of the compressed interaction network (feature_cross.py:694-794, ``feature_cross.CIN``)
behind ``mhte_cin_layer`` / ``mhte_cin_layer_grad`` (csrc/mhte_cin_kernels.h): fp32 MFMA GEMMs whose A operand, the
reference's ``[B, D, H m]`` outer product, is formed in registers and never stored.

``dcn_cross`` is the cross stack of a Deep & Cross network (feature_cross.py:445-690, ``feature_cross.DCN``, the
vector and matrix forms) behind ``mhte_dcn_layer`` / ``mhte_dcn_layer_grad`` (csrc/mhte_dcn_kernels.h): per layer one
launch whose epilogue does the bias, the multiply by ``x0`` and the residual, and a gradient that carries the stack's
running ``dx0`` as an operand.

``can_unit`` is the Co-Action Network's unit (feature_cross.py:345-440, ``feature_cross.CAN``) behind
``mhte_can_forward`` / ``mhte_can_grad`` (csrc/mhte_can_kernels.h): every sample's own small MLP, cut out of its item
embedding, runs over its user rows as a chain of fp32 MFMAs that never leaves the registers; one launch forward, one
backward, nothing saved but the two inputs.

``autoint`` is the self-attention stack of AutoInt (feature_trans.py:31-93, ``feature_trans.AutoInt``) behind
``mhte_autoint_forward`` / ``mhte_autoint_grad`` (csrc/mhte_autoint_kernels.h): a workgroup per sample keeps the state
in LDS through all layers, the scores and the softmax in registers; one launch forward, one backward.

Tensors are float32 on the GPU; a tensor that is not contiguous is copied first.
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


# ---- the CIN layer (feature_cross.py:694-794) -------------------------------------------------------------------
CIN_ACTIVATIONS = (None, "relu")   # the index is the ABI's activation
# mhte_cin_launch_counts' order
CIN_COUNTER_NAMES = ("forward", "forward_last", "input_grad", "weight_grad", "slab_sum")
# mhte_cin_plan's order
CIN_PLAN_NAMES = ("row_block", "column_tiles", "k_chunk", "slab_rows", "slabs", "workspace_bytes")


def _cin_activation(what, activation) -> int:
  if activation not in CIN_ACTIVATIONS:
    raise NotImplementedError("%s: activation must be None or 'relu', got %r" % (what, activation))
  return CIN_ACTIVATIONS.index(activation)


def _cin_operands(what, shapes, **tensors):
  """Checked and contiguous, in the order given; ``shapes``: {name: the shape it must have}; None is passed on."""
  out = []
  first = None
  for name, t in tensors.items():
    if t is None:
      out.append(None)
      continue
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
    if t.dtype != torch.float32:
      raise TypeError("%s: %s must be float32, got %s" % (what, name, t.dtype))
    if first is None:
      first = (name, t)
    elif t.device != first[1].device:
      raise ValueError("%s: %s is on %s, %s on %s" % (what, name, t.device, first[0], first[1].device))
    if name in shapes and tuple(t.shape) != tuple(shapes[name]):
      raise ValueError("%s: %s must have the shape %s, got %s" % (what, name, tuple(shapes[name]), tuple(t.shape)))
    out.append(t)
  for name, t in tensors.items():
    if t is not None and not t.is_cuda:
      raise TypeError("%s: %s must be on the GPU (there is no CPU path)" % (what, name))
  return [t if t is None or t.is_contiguous() else t.contiguous() for t in out]


def _cin_dims(what, x0, xl, weight):
  for name, t, nd in (("x0", x0, 3), ("xl", xl, 3), ("weight", weight, 2)):
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
    if t.dim() != nd:
      raise ValueError("%s: %s is not %dD (shape %s)" % (what, name, nd, tuple(t.shape)))
  B, m, D = x0.shape
  H, U = xl.shape[1], weight.shape[1]
  return B, m, D, H, U, {"xl": (B, H, D), "weight": (H * m, U), "bias": (U,), "xnext": (B, U, D),
                         "dxnext": (B, U, D), "dpooled": (B, U)}


def _cin_forward(x0, xl, weight, bias, activation, want_next):
  what = "cin_layer"
  act = _cin_activation(what, activation)
  B, m, D, H, U, shapes = _cin_dims(what, x0, xl, weight)
  x0, xl, weight, bias = _cin_operands(what, shapes, x0=x0, xl=xl, weight=weight, bias=bias)
  xnext = torch.empty((B, U, D), dtype=torch.float32, device=x0.device) if want_next else None
  pooled = torch.empty((B, U), dtype=torch.float32, device=x0.device)
  with torch.cuda.device(x0.device):
    check(_lib.lib().mhte_cin_layer(vp(x0), vp(xl), vp(weight), vp(bias), B, m, D, H, U, act, vp(xnext), vp(pooled),
                                    _stream()))
  return xnext, pooled, (x0, xl, weight)


def cin_layer_grad(dxnext: Optional[torch.Tensor], dpooled: torch.Tensor, x0: torch.Tensor, xl: torch.Tensor,
                   weight: torch.Tensor, xnext: Optional[torch.Tensor], activation=None, want_x0: bool = True,
                   want_xl: bool = True, want_weight: bool = True, want_bias: bool = True):
  """-> (dx0, dxl, dweight, dbias) of ``cin_layer``, shaped like their operands.  ``dxnext`` is None for a layer
  whose ``xnext`` was not used; ``xnext`` (the layer's saved output) is needed with ``'relu'`` only.  A gradient
  that is not wanted is ``None``; asking for one alone gives the same bits as asking for all."""
  what = "cin_layer_grad"
  act = _cin_activation(what, activation)
  if not (want_x0 or want_xl or want_weight or want_bias):
    raise ValueError("%s: at least one of want_x0, want_xl, want_weight and want_bias" % what)
  if act and xnext is None:
    raise ValueError("%s: 'relu' needs xnext, the layer's saved output" % what)
  B, m, D, H, U, shapes = _cin_dims(what, x0, xl, weight)
  dxnext, dpooled, x0, xl, weight, xnext = _cin_operands(what, shapes, dxnext=dxnext, dpooled=dpooled, x0=x0, xl=xl,
                                                         weight=weight, xnext=xnext)
  dx0 = torch.empty_like(x0) if want_x0 else None
  dxl = torch.empty_like(xl) if want_xl else None
  dweight = torch.empty_like(weight) if want_weight else None
  dbias = torch.empty((U,), dtype=torch.float32, device=x0.device) if want_bias else None
  with torch.cuda.device(x0.device):
    check(_lib.lib().mhte_cin_layer_grad(vp(dxnext), vp(dpooled), vp(x0), vp(xl), vp(weight), vp(xnext), B, m, D, H,
                                         U, act, vp(dx0), vp(dxl), vp(dweight), vp(dbias), _stream()))
  return dx0, dxl, dweight, dbias


class _CinLayer(torch.autograd.Function):
  """One layer of CIN.call (feature_cross.py:786-792) with the gradient of its own inputs."""

  @staticmethod
  def forward(ctx, x0, xl, weight, bias, activation, want_next):
    # relu's mask is read from the layer's output: a differentiated relu layer keeps it even when it is not returned
    keep = want_next or (activation is not None and any(ctx.needs_input_grad[:4]))
    xnext, pooled, (x0_c, xl_c, w_c) = _cin_forward(x0, xl, weight, bias, activation, keep)
    ctx.save_for_backward(x0_c, xl_c, w_c, *((xnext,) if keep else ()))
    ctx.activation, ctx.want_next = activation, want_next
    return (xnext, pooled) if want_next else pooled

  @staticmethod
  def backward(ctx, *grads):
    x0, xl, w = ctx.saved_tensors[:3]
    xnext = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
    dxnext, dpooled = grads if ctx.want_next else (None, grads[0])
    if dpooled is None:
      dpooled = torch.zeros((x0.shape[0], w.shape[1]), dtype=torch.float32, device=x0.device)
    need = ctx.needs_input_grad[:4]
    if not any(need):
      return (None,) * 6
    return cin_layer_grad(dxnext, dpooled, x0, xl, w, xnext, ctx.activation, *need) + (None, None)


def cin_layer(x0: torch.Tensor, xl: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, activation=None,
              want_next: bool = True) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
  """One CIN layer (feature_cross.py:786-794).  ``x0`` ``[B, m, D]``, ``xl`` ``[B, H, D]`` (the first layer passes
  ``x0``), ``weight`` ``[H m, U]`` with the channel index ``h m + j``, ``bias`` ``[U]`` -> ``(xnext, pooled)``:
  ``xnext`` ``[B, U, D]``, the next layer's ``xl`` (None with ``want_next=False``: a last layer never writes it), and
  ``pooled`` ``[B, U]``, the sum over the embedding dimension.  ``activation`` is None or ``'relu'``.
  Differentiable in ``x0``, ``xl``, ``weight`` and ``bias``.  The ``[B, D, H m]`` outer product of the reference
  is never stored."""
  _cin_activation("cin_layer", activation)
  if want_next:
    return _CinLayer.apply(x0, xl, weight, bias, activation, True)
  return None, _CinLayer.apply(x0, xl, weight, bias, activation, False)


def cin_plan(B: int, m: int, D: int, H: int, U: int):
  """{row_block, column_tiles, k_chunk, slab_rows, slabs, workspace_bytes} of a call (mhte_cin_plan): a function of
  the shape alone, no device needed."""
  out = (C.c_int64 * len(CIN_PLAN_NAMES))()
  check(_lib.lib().mhte_cin_plan(int(B), int(m), int(D), int(H), int(U), out, len(CIN_PLAN_NAMES)))
  return dict(zip(CIN_PLAN_NAMES, [int(x) for x in out]))


def cin_launch_counts():
  """{form: launches of this process} (mhte_cin_launch_counts)."""
  out = (C.c_int64 * len(CIN_COUNTER_NAMES))()
  check(_lib.lib().mhte_cin_launch_counts(out, len(CIN_COUNTER_NAMES)))
  return dict(zip(CIN_COUNTER_NAMES, [int(x) for x in out]))


# ---- the DCN cross layer (feature_cross.py:445-690) ---------------------------------------------------------------
DCN_TYPES = ("vector", "matrix")   # the index is the ABI's type; the reference's 'mixed' is not built
# mhte_dcn_launch_counts' order
DCN_COUNTER_NAMES = ("matrix_forward", "matrix_forward_no_aux", "matrix_input_grad", "matrix_weight_grad",
                     "matrix_slab_sum", "vector_forward", "vector_forward_no_aux", "vector_grad", "vector_slab_sum")
# mhte_dcn_plan's order
DCN_PLAN_NAMES = ("row_block", "column_span", "k_chunk", "slab_rows", "slabs", "workspace_bytes")


def _dcn_type(what, dcn_type) -> int:
  if dcn_type not in DCN_TYPES:
    raise NotImplementedError("%s: dcn_type must be 'vector' or 'matrix', got %r" % (what, dcn_type))
  return DCN_TYPES.index(dcn_type)


def _dcn_dims(what, x0, typ):
  if not isinstance(x0, torch.Tensor):
    raise TypeError("%s: x0 must be a torch tensor, got %s" % (what, type(x0).__name__))
  if x0.dim() != 2:
    raise ValueError("%s: x0 is not 2D (shape %s)" % (what, tuple(x0.shape)))
  B, d = x0.shape
  return B, d, {"xl": (B, d), "weight": (d, d) if typ else (d, 1), "bias": (1, d), "dxnext": (B, d),
                "aux": (B, d) if typ else (B,), "dx0_acc": (B, d)}


def dcn_layer(x0: torch.Tensor, xl: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, dcn_type="matrix",
              want_aux: bool = True):
  """One DCN cross layer (feature_cross.py:564-568), no autograd: ``x0``, ``xl`` ``[B, d]``, ``weight`` ``[d, 1]``
  (``'vector'``) or ``[d, d]`` (``'matrix'``), ``bias`` ``[1, d]`` -> ``(xnext, aux)``.  ``aux`` is what
  ``dcn_layer_grad`` needs of the forward (``s`` ``[B]`` / ``u`` ``[B, d]``); with ``want_aux=False`` it is None and
  never written.  ``dcn_cross`` is the differentiable stack."""
  what = "dcn_layer"
  typ = _dcn_type(what, dcn_type)
  B, d, shapes = _dcn_dims(what, x0, typ)
  x0, xl, weight, bias = _cin_operands(what, shapes, x0=x0, xl=xl, weight=weight, bias=bias)
  xnext = torch.empty_like(x0)
  aux = torch.empty(shapes["aux"], dtype=torch.float32, device=x0.device) if want_aux else None
  with torch.cuda.device(x0.device):
    check(_lib.lib().mhte_dcn_layer(vp(x0), vp(xl), vp(weight), vp(bias), B, d, typ, vp(xnext), vp(aux), _stream()))
  return xnext, aux


def dcn_layer_grad(dxnext: torch.Tensor, x0: torch.Tensor, xl: torch.Tensor, weight: torch.Tensor,
                   aux: Optional[torch.Tensor], dcn_type="matrix", first: bool = False,
                   dx0_acc: Optional[torch.Tensor] = None, want_x0: bool = True, want_xl: bool = True,
                   want_weight: bool = True, want_bias: bool = True):
  """-> (dx0, dxl, dweight, dbias) of ``dcn_layer``, shaped like their operands.  ``dx0 = dx0_acc + (this layer's
  part)``; a contiguous ``dx0_acc`` is updated in place and returned as ``dx0``.  ``first=True`` is a stack's first
  layer, whose ``xl`` is ``x0``: its ``dxl`` is added into ``dx0`` and returned as None.  A gradient that is not wanted
  is None; asking for one alone gives the same bits as asking for all."""
  what = "dcn_layer_grad"
  typ = _dcn_type(what, dcn_type)
  if not (want_x0 or want_xl or want_weight or want_bias):
    raise ValueError("%s: at least one of want_x0, want_xl, want_weight and want_bias" % what)
  if want_x0 and aux is None:
    raise ValueError("%s: dx0 needs aux, what the forward saved" % what)
  if first and not want_x0:
    raise ValueError("%s: first=True needs want_x0 (the layer's input gradient is dx0)" % what)
  B, d, shapes = _dcn_dims(what, x0, typ)
  dxnext, x0, xl, weight, aux, dx0_acc = _cin_operands(what, shapes, dxnext=dxnext, x0=x0, xl=xl, weight=weight,
                                                       aux=aux, dx0_acc=dx0_acc)
  dx0 = (dx0_acc if dx0_acc is not None else torch.empty_like(x0)) if want_x0 else None
  dxl = torch.empty_like(x0) if want_xl and not first else None
  dweight = torch.empty_like(weight) if want_weight else None
  dbias = torch.empty((1, d), dtype=torch.float32, device=x0.device) if want_bias else None
  with torch.cuda.device(x0.device):
    check(_lib.lib().mhte_dcn_layer_grad(vp(dxnext), vp(x0), vp(xl), vp(weight), vp(aux), B, d, typ, int(bool(first)),
                                         vp(dx0_acc), vp(dx0), vp(dxl), vp(dweight), vp(dbias), _stream()))
  return dx0, dxl, dweight, dbias


class _DcnCross(torch.autograd.Function):
  """The whole stack of DCN.call (feature_cross.py:560-606) as one node: L forward launches, and backward L input
  gradient launches from the last layer to the first with one dx0 buffer carried through them."""

  @staticmethod
  def forward(ctx, x0, dcn_type, n, keep, *params):
    kernels, biases = params[:n], params[n:]
    xl, saved = x0, []
    for w, b in zip(kernels, biases):
      xnext, aux = dcn_layer(x0, xl, w, b, dcn_type, want_aux=keep)
      saved += [xl, aux]
      xl = xnext
    if keep:
      ctx.save_for_backward(*kernels, *saved)
    ctx.dcn_type, ctx.n = dcn_type, n
    return xl

  @staticmethod
  def backward(ctx, g):
    n = ctx.n
    kernels, saved = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
    x0 = saved[0]
    dx0, dws, dbs = None, [None] * n, [None] * n
    for i in reversed(range(n)):
      dx0, g, dws[i], dbs[i] = dcn_layer_grad(g, x0, saved[2 * i], kernels[i], saved[2 * i + 1], ctx.dcn_type,
                                              first=i == 0, dx0_acc=dx0)
    return (dx0, None, None, None) + tuple(dws) + tuple(dbs)


def dcn_cross(x0: torch.Tensor, kernels: Sequence[torch.Tensor], biases: Sequence[torch.Tensor],
              dcn_type="matrix") -> torch.Tensor:
  """The cross stack of a Deep & Cross network (feature_cross.py:560-606): ``xl = x0`` and, per layer,
  ``xl = x0 * (xl @ kernel) + bias + xl`` (``'vector'``, kernel ``[d, 1]``) or ``xl = x0 * (xl @ kernel + bias) + xl``
  (``'matrix'``, kernel ``[d, d]``), bias ``[1, d]`` -> ``[B, d]``.  Differentiable in ``x0`` and every kernel and
  bias as ONE autograd node: one launch per layer forward; backward one input-gradient and one weight-gradient
  launch per layer (the vector form does both in one) plus a slab sum where the plan has several slabs, and no torch
  arithmetic.  Under ``torch.no_grad()`` nothing is saved or written for a backward."""
  what = "dcn_cross"
  _dcn_type(what, dcn_type)
  kernels, biases = tuple(kernels), tuple(biases)
  if not kernels or len(kernels) != len(biases):
    raise ValueError("%s: as many kernels as biases, at least one (got %d and %d)" % (what, len(kernels), len(biases)))
  keep = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                         for t in (x0,) + kernels + biases)
  return _DcnCross.apply(x0, dcn_type, len(kernels), keep, *kernels, *biases)


def dcn_plan(B: int, d: int, dcn_type="matrix"):
  """{row_block, column_span, k_chunk, slab_rows, slabs, workspace_bytes} of a call (mhte_dcn_plan): a function of
  the shape alone, no device needed."""
  out = (C.c_int64 * len(DCN_PLAN_NAMES))()
  check(_lib.lib().mhte_dcn_plan(int(B), int(d), _dcn_type("dcn_plan", dcn_type), out, len(DCN_PLAN_NAMES)))
  return dict(zip(DCN_PLAN_NAMES, [int(x) for x in out]))


def dcn_launch_counts():
  """{form: launches of this process} (mhte_dcn_launch_counts)."""
  out = (C.c_int64 * len(DCN_COUNTER_NAMES))()
  check(_lib.lib().mhte_dcn_launch_counts(out, len(DCN_COUNTER_NAMES)))
  return dict(zip(DCN_COUNTER_NAMES, [int(x) for x in out]))


# ---- the CAN co-action unit (feature_cross.py:345-440) ------------------------------------------------------------
CAN_ACTIVATIONS = (None, "relu")   # the index is the ABI's activation; the reference's 'tanh' / 'sigmoid' are not built
CAN_MAX_DIM, CAN_MAX_LAYERS = 32, 8
CAN_COUNTER_NAMES = ("forward", "grad")   # mhte_can_launch_counts' order
# mhte_can_plan's order
CAN_PLAN_NAMES = ("rows_per_tile", "padded_d", "tiles_per_sample", "samples_per_workgroup", "lds_bytes",
                  "workspace_bytes")


def _can_dims(what, user, item, layer_num, activation, is_seq, is_stacked):
  """-> (B, F, T, d, the ABI's activation, {name: the shape it must have}); every refusal that needs no device."""
  if activation not in CAN_ACTIVATIONS:
    raise NotImplementedError("%s: activation must be None or 'relu', got %r" % (what, activation))
  if not isinstance(layer_num, int) or isinstance(layer_num, bool) or not 1 <= layer_num <= CAN_MAX_LAYERS:
    raise ValueError("%s: layer_num must be an int in [1, %d], got %r" % (what, CAN_MAX_LAYERS, layer_num))
  for name, t in (("user", user), ("item", item)):
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
  rank = 2 + bool(is_seq) + bool(is_stacked)
  if user.dim() != rank:
    raise ValueError("%s: user must be %dD for is_seq=%s, is_stacked=%s (shape %s)"
                     % (what, rank, bool(is_seq), bool(is_stacked), tuple(user.shape)))
  if item.dim() != 2:
    raise ValueError("%s: item is not 2D (shape %s)" % (what, tuple(item.shape)))
  B, d = int(user.shape[0]), int(user.shape[-1])
  F = int(user.shape[1]) if is_stacked else 1
  T = int(user.shape[-2]) if is_seq else 1
  if not 1 <= d <= CAN_MAX_DIM:
    raise ValueError("%s: d must be in [1, %d], got %d" % (what, CAN_MAX_DIM, d))
  if F < 1 or T < 1:
    raise ValueError("%s: F and T must be >= 1, got user of shape %s" % (what, tuple(user.shape)))
  if int(item.shape[0]) != B:
    raise ValueError("%s: user has B = %d, item B = %d" % (what, B, int(item.shape[0])))
  P = layer_num * d * (d + 1)
  if int(item.shape[1]) != P:
    raise ValueError("%s: item must be layer_num * d * (d + 1) = %d wide, got %d" % (what, P, int(item.shape[1])))
  res = (B, F, d) if is_stacked else (B, d)
  return B, F, T, d, CAN_ACTIVATIONS.index(activation), {"user": tuple(user.shape), "item": (B, P), "dout": res}


def can_forward(user: torch.Tensor, item: torch.Tensor, layer_num: int = 2, activation="relu", is_seq: bool = False,
                is_stacked: bool = True) -> torch.Tensor:
  """CAN.call (feature_cross.py:386-430), no autograd: ``user`` ``[B, F, T, d]`` (stacked sequence), ``[B, F, d]``
  (stacked), ``[B, T, d]`` (sequence) or ``[B, d]``, ``item`` ``[B, layer_num d (d + 1)]`` -> ``[B, F, d]`` (stacked)
  or ``[B, d]`` (always, also at ``B = 1``).  ``h = act(h @ W_i + b_i)`` on every layer with sample b's ``W_i``,
  ``b_i`` cut out of ``item[b]``, then the sum over ``T``.  One launch; ``activation`` None or ``'relu'`` (``'tanh'``
  and ``'sigmoid'`` are not built), ``1 <= d <= 32``, ``1 <= layer_num <= 8``; ``B = 0`` returns an empty result
  without a launch."""
  what = "can_forward"
  B, F, T, d, act, shapes = _can_dims(what, user, item, layer_num, activation, is_seq, is_stacked)
  user, item = _cin_operands(what, shapes, user=user, item=item)
  out = torch.empty(shapes["dout"], dtype=torch.float32, device=user.device)
  if B:
    with torch.cuda.device(user.device):
      check(_lib.lib().mhte_can_forward(vp(user), vp(item), B, F, T, d, layer_num, act, vp(out), _stream()))
  return out


def can_grad(dout: torch.Tensor, user: torch.Tensor, item: torch.Tensor, layer_num: int = 2, activation="relu",
             is_seq: bool = False, is_stacked: bool = True, want_user: bool = True, want_item: bool = True):
  """-> (duser, ditem) of ``can_forward``, shaped like ``user`` and ``item``, in one launch that recomputes the
  layers (nothing of the forward is needed).  A gradient that is not wanted is None; asking for one alone gives the
  same bits as asking for both."""
  what = "can_grad"
  if not (want_user or want_item):
    raise ValueError("%s: at least one of want_user and want_item" % what)
  B, F, T, d, act, shapes = _can_dims(what, user, item, layer_num, activation, is_seq, is_stacked)
  dout, user, item = _cin_operands(what, shapes, dout=dout, user=user, item=item)
  duser = torch.empty_like(user) if want_user else None
  ditem = torch.empty_like(item) if want_item else None
  if B:
    with torch.cuda.device(user.device):
      check(_lib.lib().mhte_can_grad(vp(dout), vp(user), vp(item), B, F, T, d, layer_num, act, vp(duser), vp(ditem),
                                     _stream()))
  return duser, ditem


class _CanUnit(torch.autograd.Function):
  """CAN.call as one node: one launch forward, one backward; saves its two inputs and nothing else."""

  @staticmethod
  def forward(ctx, user, item, layer_num, activation, is_seq, is_stacked):
    ctx.save_for_backward(user, item)
    ctx.form = (layer_num, activation, is_seq, is_stacked)
    return can_forward(user, item, layer_num, activation, is_seq, is_stacked)

  @staticmethod
  def backward(ctx, g):
    user, item = ctx.saved_tensors
    want = ctx.needs_input_grad[:2]
    duser, ditem = can_grad(g, user, item, *ctx.form, want_user=want[0], want_item=want[1])
    return duser, ditem, None, None, None, None


def can_unit(user: torch.Tensor, item: torch.Tensor, layer_num: int = 2, activation="relu", is_seq: bool = False,
             is_stacked: bool = True) -> torch.Tensor:
  """``can_forward``, differentiable in ``user`` and ``item`` as ONE autograd node: one launch forward, one backward,
  no torch arithmetic; the node saves its two inputs only.  Under ``torch.no_grad()`` the forward alone runs."""
  return _CanUnit.apply(user, item, layer_num, activation, bool(is_seq), bool(is_stacked))


def can_plan(B: int, F: int, T: int, d: int, layer_num: int):
  """{rows_per_tile, padded_d, tiles_per_sample, samples_per_workgroup, lds_bytes, workspace_bytes} of a call
  (mhte_can_plan): a function of the shape alone, no device needed."""
  out = (C.c_int64 * len(CAN_PLAN_NAMES))()
  check(_lib.lib().mhte_can_plan(int(B), int(F), int(T), int(d), int(layer_num), out, len(CAN_PLAN_NAMES)))
  return dict(zip(CAN_PLAN_NAMES, [int(x) for x in out]))


def can_launch_counts():
  """{kernel: launches of this process} (mhte_can_launch_counts)."""
  out = (C.c_int64 * len(CAN_COUNTER_NAMES))()
  check(_lib.lib().mhte_can_launch_counts(out, len(CAN_COUNTER_NAMES)))
  return dict(zip(CAN_COUNTER_NAMES, [int(x) for x in out]))


# ---- AutoInt (feature_trans.py:31-93) -------------------------------------------------------------------------------
AUTOINT_MAX_N, AUTOINT_MAX_K, AUTOINT_MAX_LAYERS = 128, 64, 8
AUTOINT_COUNTER_NAMES = ("forward", "grad")   # mhte_autoint_launch_counts' order
# mhte_autoint_plan's order
AUTOINT_PLAN_NAMES = ("tile", "row_tiles", "padded_k", "samples_per_workgroup", "lds_bytes_forward", "lds_bytes_grad",
                      "workspace_bytes")


def _autoint_dims(what, x, layer_num):
  """-> (B, n, k); every refusal that needs no device."""
  if not isinstance(layer_num, int) or isinstance(layer_num, bool) or not 1 <= layer_num <= AUTOINT_MAX_LAYERS:
    raise ValueError("%s: layer_num must be an int in [1, %d], got %r" % (what, AUTOINT_MAX_LAYERS, layer_num))
  if not isinstance(x, torch.Tensor):
    raise TypeError("%s: x must be a torch tensor, got %s" % (what, type(x).__name__))
  if x.dim() != 3:
    raise ValueError("%s: x is not 3D (shape %s)" % (what, tuple(x.shape)))
  B, n, k = (int(s) for s in x.shape)
  if not 1 <= n <= AUTOINT_MAX_N:
    raise ValueError("%s: n must be in [1, %d], got %d" % (what, AUTOINT_MAX_N, n))
  if not 1 <= k <= AUTOINT_MAX_K:
    raise ValueError("%s: k must be in [1, %d], got %d" % (what, AUTOINT_MAX_K, k))
  return B, n, k


def autoint_forward(x: torch.Tensor, layer_num: int = 1, want_states: bool = False):
  """AutoInt.call's loop (feature_trans.py:71-80), no autograd: ``x`` ``[B, n, k]`` -> ``(out [B, n, k], states)``.
  Per layer ``X <- softmax(X X^T, -1) X``, the whole stack in one launch.  ``states`` is ``[layer_num - 1, B, n, k]``
  (``X_1 .. X_{L-1}``, what ``autoint_grad`` needs) when ``want_states`` and ``layer_num > 1``, else None; ``out`` has
  the same bits either way.  ``1 <= n <= 128``, ``1 <= k <= 64``, ``1 <= layer_num <= 8``; ``B = 0`` returns an empty
  result without a launch."""
  what = "autoint_forward"
  B, n, k = _autoint_dims(what, x, layer_num)
  x, = _cin_operands(what, {}, x=x)
  out = torch.empty_like(x)
  states = None
  if want_states and layer_num > 1:
    states = torch.empty((layer_num - 1, B, n, k), dtype=torch.float32, device=x.device)
  if B:
    with torch.cuda.device(x.device):
      check(_lib.lib().mhte_autoint_forward(vp(x), B, n, k, layer_num, vp(out), vp(states), _stream()))
  return out, states


def autoint_grad(dout: torch.Tensor, x: torch.Tensor, states: Optional[torch.Tensor], out: torch.Tensor,
                 layer_num: int = 1) -> torch.Tensor:
  """-> dx of ``autoint_forward`` in one launch that walks the layers last to first; ``states`` and ``out`` are the
  forward's (``states`` None exactly when ``layer_num == 1``).  ``out`` is checked like an operand and not read:
  the kernel takes ``delta_i = dO_i . O_i`` as ``sum_j P_ij dP_ij``, which is exactly ``dP_ii`` where the softmax
  saturates."""
  what = "autoint_grad"
  B, n, k = _autoint_dims(what, x, layer_num)
  if (states is None) != (layer_num == 1):
    raise ValueError("%s: states must be None exactly when layer_num == 1 (layer_num = %d)" % (what, layer_num))
  shapes = {"dout": (B, n, k), "out": (B, n, k), "states": (layer_num - 1, B, n, k)}
  dout, x, states, out = _cin_operands(what, shapes, dout=dout, x=x, states=states, out=out)
  dx = torch.empty_like(x)
  if B:
    with torch.cuda.device(x.device):
      check(_lib.lib().mhte_autoint_grad(vp(dout), vp(x), vp(states), vp(out), B, n, k, layer_num, vp(dx), _stream()))
  return dx


class _AutoInt(torch.autograd.Function):
  """The whole stack as one node: one launch forward, one backward; saves x, the states and out."""

  @staticmethod
  def forward(ctx, x, layer_num):
    out, states = autoint_forward(x, layer_num, want_states=True)
    ctx.layer_num = layer_num
    ctx.save_for_backward(*((x, out) if states is None else (x, out, states)))
    return out

  @staticmethod
  def backward(ctx, g):
    x, out, *states = ctx.saved_tensors
    return autoint_grad(g, x, states[0] if states else None, out, ctx.layer_num), None


def autoint(x: torch.Tensor, layer_num: int = 1) -> torch.Tensor:
  """``autoint_forward``'s ``out``, differentiable in ``x`` as ONE autograd node for the whole stack: one launch
  forward, one backward, no torch arithmetic.  Under ``torch.no_grad()``, or when ``x`` needs no gradient, no states
  buffer is passed; otherwise the node saves ``x``, ``states`` and ``out``."""
  if isinstance(x, torch.Tensor) and not (torch.is_grad_enabled() and x.requires_grad):
    return autoint_forward(x, layer_num)[0]
  return _AutoInt.apply(x, layer_num)


def autoint_plan(B: int, n: int, k: int, layer_num: int):
  """{tile, row_tiles, padded_k, samples_per_workgroup, lds_bytes_forward, lds_bytes_grad, workspace_bytes} of a call
  (mhte_autoint_plan): a function of the shape alone, no device needed."""
  out = (C.c_int64 * len(AUTOINT_PLAN_NAMES))()
  check(_lib.lib().mhte_autoint_plan(int(B), int(n), int(k), int(layer_num), out, len(AUTOINT_PLAN_NAMES)))
  return dict(zip(AUTOINT_PLAN_NAMES, [int(v) for v in out]))


def autoint_launch_counts():
  """{kernel: launches of this process} (mhte_autoint_launch_counts)."""
  out = (C.c_int64 * len(AUTOINT_COUNTER_NAMES))()
  check(_lib.lib().mhte_autoint_launch_counts(out, len(AUTOINT_COUNTER_NAMES)))
  return dict(zip(AUTOINT_COUNTER_NAMES, [int(v) for v in out]))
