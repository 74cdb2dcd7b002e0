"""Losses on MI355X — host-side mirror of monolith/native_training/losses/inbatch_auc_loss.py.

``inbatch_auc_loss`` is the op pair InbatchAucLoss / InbatchAucLossGrad (runtime/ops/inbatch_auc_loss.cc): the
sum of ``log sigmoid(logit[i] - logit[j])`` over every (positive, negative) pair of the batch, the leg between the
dense tower's logit and the ``dy`` of ``DenseMlp.backward``.  The sign is the reference's (the loss is <= 0,
callers negate).  Loss and gradient are the hand-written kernels behind ``mhte_inbatch_auc_loss`` /
``mhte_inbatch_auc_loss_grad`` (include/monolith_amd_hash_table.h, csrc/mhte_auc_kernels.h): fp32 terms, fp64 sums
in a fixed order, the same bits on every run.  No function of this module waits for the GPU or reads a device
value, so forward and backward can be captured into a graph.

Tensors are float32, contiguous and on the GPU, of any shape; label and logit hold the same number of elements.
"""
import ctypes as C
from typing import Union

import torch

from monolith_amd import _lib
from monolith_amd._lib import check, vp
from monolith_amd.multi_hash_table_ops import _stream

# mhte_inbatch_auc_launch_counts' order
COUNTER_NAMES = ("count", "scan", "scatter", "pair/loss", "pair/loss+grad", "pair/grad", "final/loss",
                 "final/loss+grad", "final/grad")


def _operands(what, label, logit, neg_weight):
  for name, t in (("label", label), ("logit", logit)):
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
    if t.dtype != torch.float32:
      raise TypeError("%s: %s must be float32, got %s" % (what, name, t.dtype))
    if not t.is_contiguous():
      raise ValueError("%s: %s must be contiguous" % (what, name))
  if label.numel() != logit.numel():
    raise ValueError("%s: the label and logit not match (%d and %d elements)" % (what, label.numel(), logit.numel()))
  neg_weight = float(neg_weight)
  if not 0.0 < neg_weight <= 1.0:
    raise ValueError("%s: neg_weight must be in (0, 1], got %r" % (what, neg_weight))
  if label.device != logit.device:
    raise ValueError("%s: label is on %s, logit on %s" % (what, label.device, logit.device))
  for name, t in (("label", label), ("logit", logit)):
    if not t.is_cuda:
      raise TypeError("%s: %s must be on the GPU (there is no CPU path)" % (what, name))
  return neg_weight


def _forward(label, logit, neg_weight, want_grad):
  """-> (loss as a 0-d tensor, the unit gradient shaped like logit or None)"""
  neg_weight = _operands("inbatch_auc_loss", label, logit, neg_weight)
  loss = torch.empty((), dtype=torch.float32, device=logit.device)
  unit = torch.empty_like(logit) if want_grad else None
  with torch.cuda.device(logit.device):
    check(_lib.lib().mhte_inbatch_auc_loss(vp(label), vp(logit), logit.numel(), neg_weight, vp(loss), vp(unit),
                                           _stream()))
  return loss, unit


def inbatch_auc_loss_grad(label: torch.Tensor, logit: torch.Tensor, grad: Union[float, torch.Tensor],
                          neg_weight: float = 1.0) -> torch.Tensor:
  """The op InbatchAucLossGrad -> logit_grad, shaped like ``logit``.  ``grad``: a float, or a 0-d float32 tensor on
  the GPU that is read on the device."""
  what = "inbatch_auc_loss_grad"
  grad_dev = None
  if isinstance(grad, torch.Tensor):
    if not (grad.is_cuda and grad.dtype == torch.float32 and grad.numel() == 1):
      raise TypeError("%s: grad must be a float or a 0-d float32 tensor on the GPU" % what)
    grad_dev, grad = grad, 1.0
  neg_weight = _operands(what, label, logit, neg_weight)
  out = torch.empty_like(logit)
  with torch.cuda.device(logit.device):
    check(_lib.lib().mhte_inbatch_auc_loss_grad(vp(label), vp(logit), logit.numel(), float(grad), vp(grad_dev),
                                                neg_weight, vp(out), _stream()))
  return out


class _InbatchAucLoss(torch.autograd.Function):
  """inbatch_auc_loss.py: the registered gradient of InbatchAucLoss is InbatchAucLossGrad of the op's own inputs.
  Here the forward leaves the gradient for grad = 1 (its terms share the loss's exponentials) and the backward
  scales it by the upstream gradient on the device."""

  @staticmethod
  def forward(ctx, label, logit, neg_weight):
    loss, unit = _forward(label, logit, neg_weight, want_grad=True)
    ctx.save_for_backward(unit)
    return loss

  @staticmethod
  def backward(ctx, grad):
    (unit,) = ctx.saved_tensors
    if unit.numel() == 0:
      return None, unit, None
    grad = grad.to(torch.float32).reshape(())
    pin = (C.c_void_p * 1)(C.c_void_p(unit.data_ptr()))
    out = torch.empty_like(unit)
    pout = (C.c_void_p * 1)(C.c_void_p(out.data_ptr()))
    lens = (C.c_int64 * 1)(unit.numel())
    with torch.cuda.device(unit.device):
      check(_lib.lib().mhte_scale_tensors_dev(pin, pout, lens, 1, vp(grad), _stream()))
    return None, out, None


def inbatch_auc_loss(label: torch.Tensor, logit: torch.Tensor, neg_weight: float = 1.0) -> torch.Tensor:
  """The op InbatchAucLoss -> a 0-d float32 tensor, differentiable in ``logit`` (the gradient has its shape).
  ``label[i] > 0`` marks a positive, ``-10000 < label[i] <= 0`` a negative, anything else is ignored."""
  return _InbatchAucLoss.apply(label, logit, neg_weight)


def inbatch_auc_launch_counts():
  """{form: launches of this process} (mhte_inbatch_auc_launch_counts)."""
  out = (C.c_int64 * len(COUNTER_NAMES))()
  check(_lib.lib().mhte_inbatch_auc_launch_counts(out, len(COUNTER_NAMES)))
  return dict(zip(COUNTER_NAMES, [int(x) for x in out]))


# ---- the batch softmax loss (native_training/losses/batch_softmax_loss.py) ------------------------------------
# ``batch_softmax_loss`` is the sampling-bias-corrected in-batch softmax of the two-tower model, the consumer of the
# interval that ``entry.BatchSoftmaxOptimizer`` keeps per item id:
#   z_ij = (q^_i . i^_j) / temperature + log(max(item_step_interval_j, 1)),  loss = -sum_i r_i (z_ii - lse_i)
# with both operands l2-normalised when ``normalize``.  The kernels behind ``mhte_batch_softmax_loss`` /
# ``mhte_batch_softmax_loss_grad`` (csrc/mhte_bsm_kernels.h) never store the B x B matrix, take the row maximum
# before the exponential (the reference's unshifted exp overflows in fp32; this is the one defined deviation) and
# give the same bits on every run.  query and item are [B, k] float32, contiguous, on the GPU; item_step_interval
# and r hold B elements.

# mhte_batch_softmax_launch_counts' order
BSM_COUNTER_NAMES = ("prep", "row/forward", "row/grad", "col", "final/lse", "final/grad")
# mhte_batch_softmax_plan's order
BSM_PLAN_NAMES = ("row_block", "column_tile", "row_chunks", "column_chunks", "workspace_bytes")


def _bsm_operands(what, query, item, item_step_interval, r, normalize, temperature):
  """-> (B, k, normalize as 0 / 1, temperature as a float)"""
  named = (("query", query), ("item", item), ("item_step_interval", item_step_interval), ("r", r))
  for name, t in named:
    if not isinstance(t, torch.Tensor):
      raise TypeError("%s: %s must be a torch tensor, got %s" % (what, name, type(t).__name__))
    if t.dtype != torch.float32:
      raise TypeError("%s: %s must be float32, got %s" % (what, name, t.dtype))
    if not t.is_contiguous():
      raise ValueError("%s: %s must be contiguous" % (what, name))
  if query.dim() != 2 or item.dim() != 2 or query.shape != item.shape:
    raise ValueError("%s: query and item must be [B, k] of one shape, got %s and %s" %
                     (what, tuple(query.shape), tuple(item.shape)))
  B, k = int(query.shape[0]), int(query.shape[1])
  for name, t in named[2:]:
    if t.numel() != B:
      raise ValueError("%s: %s must hold B = %d elements, got %d" % (what, name, B, t.numel()))
  if not 1 <= k <= 256:
    raise ValueError("%s: k must be in [1, 256], got %d" % (what, k))
  if B >= 1 << 24:
    raise ValueError("%s: B must be below 2^24, got %d" % (what, B))
  if not isinstance(normalize, (bool, int)) or normalize not in (0, 1):
    raise TypeError("%s: normalize must be a bool, got %r" % (what, normalize))
  temperature = float(temperature)
  if not temperature > 0.0:
    raise ValueError("temperature should be positive, while got %r" % temperature)
  for name, t in named[1:]:
    if t.device != query.device:
      raise ValueError("%s: query is on %s, %s on %s" % (what, query.device, name, t.device))
  for name, t in named:
    if not t.is_cuda:
      raise TypeError("%s: %s must be on the GPU (there is no CPU path)" % (what, name))
  return B, k, int(bool(normalize)), temperature


def _bsm_forward(query, item, item_step_interval, r, normalize, temperature, want_q, want_i):
  """-> (loss as a 0-d tensor, unit dquery or None, unit ditem or None)"""
  B, k, norm, temp = _bsm_operands("batch_softmax_loss", query, item, item_step_interval, r, normalize, temperature)
  loss = torch.empty((), dtype=torch.float32, device=query.device)
  uq = torch.empty_like(query) if want_q else None
  ui = torch.empty_like(item) if want_i else None
  with torch.cuda.device(query.device):
    check(_lib.lib().mhte_batch_softmax_loss(vp(query), vp(item), vp(item_step_interval), vp(r), B, k, norm, temp,
                                             vp(loss), vp(uq), vp(ui), _stream()))
  return loss, uq, ui


def batch_softmax_loss_grad(query: torch.Tensor, item: torch.Tensor, item_step_interval: torch.Tensor,
                            r: torch.Tensor, grad: Union[float, torch.Tensor], normalize: bool = True,
                            temperature: float = 1.0, want_query: bool = True, want_item: bool = True):
  """The gradients of ``batch_softmax_loss`` scaled by ``grad`` -> (dquery or None, ditem or None).  ``grad``: a
  float, or a 0-d float32 tensor on the GPU that is read on the device."""
  what = "batch_softmax_loss_grad"
  grad_dev = None
  if isinstance(grad, torch.Tensor):
    if not (grad.is_cuda and grad.dtype == torch.float32 and grad.numel() == 1):
      raise TypeError("%s: grad must be a float or a 0-d float32 tensor on the GPU" % what)
    grad_dev, grad = grad, 1.0
  if not (want_query or want_item):
    raise ValueError("%s: at least one of want_query and want_item" % what)
  B, k, norm, temp = _bsm_operands(what, query, item, item_step_interval, r, normalize, temperature)
  dq = torch.empty_like(query) if want_query else None
  di = torch.empty_like(item) if want_item else None
  with torch.cuda.device(query.device):
    check(_lib.lib().mhte_batch_softmax_loss_grad(vp(query), vp(item), vp(item_step_interval), vp(r), B, k, norm, temp,
                                                  float(grad), vp(grad_dev), vp(dq), vp(di), _stream()))
  return dq, di


class _BatchSoftmaxLoss(torch.autograd.Function):
  """The forward leaves the gradients for an upstream gradient of 1 for whichever of query and item require one
  (from the same prepared operands and row statistics); the backward scales them on the device."""

  @staticmethod
  def forward(ctx, query, item, item_step_interval, r, normalize, temperature):
    want_q, want_i = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    loss, uq, ui = _bsm_forward(query, item, item_step_interval, r, normalize, temperature, want_q, want_i)
    ctx.wants = (want_q, want_i)
    ctx.save_for_backward(*[t for t in (uq, ui) if t is not None])
    return loss

  @staticmethod
  @torch.autograd.function.once_differentiable   # (the saved unit gradients are constants: no second derivative)
  def backward(ctx, grad):
    units = list(ctx.saved_tensors)
    outs = [torch.empty_like(u) for u in units]
    live = [(u, o) for u, o in zip(units, outs) if u.numel()]
    if live:
      grad = grad.to(torch.float32).reshape(())
      n = len(live)
      pin = (C.c_void_p * n)(*[C.c_void_p(u.data_ptr()) for u, _ in live])
      pout = (C.c_void_p * n)(*[C.c_void_p(o.data_ptr()) for _, o in live])
      lens = (C.c_int64 * n)(*[u.numel() for u, _ in live])
      with torch.cuda.device(units[0].device):
        check(_lib.lib().mhte_scale_tensors_dev(pin, pout, lens, n, vp(grad), _stream()))
    it = iter(outs)
    dq = next(it) if ctx.wants[0] else None
    di = next(it) if ctx.wants[1] else None
    return dq, di, None, None, None, None


def batch_softmax_loss(query: torch.Tensor, item: torch.Tensor, item_step_interval: torch.Tensor, r: torch.Tensor,
                       normalize: bool = True, temperature: float = 1.0) -> torch.Tensor:
  """batch_softmax_loss.py -> a 0-d float32 tensor, differentiable in ``query`` and ``item``.
  ``item_step_interval``: the moving average of the global-step interval between an item's occurrences
  (``entry.BatchSoftmaxOptimizer``); ``r``: the per-example reward."""
  return _BatchSoftmaxLoss.apply(query, item, item_step_interval, r, normalize, temperature)


def batch_softmax_plan(B: int, k: int):
  """{row_block, column_tile, row_chunks, column_chunks, workspace_bytes} for a [B, k] call
  (mhte_batch_softmax_plan): a function of the shape alone, no device needed."""
  out = (C.c_int64 * len(BSM_PLAN_NAMES))()
  check(_lib.lib().mhte_batch_softmax_plan(int(B), int(k), out, len(BSM_PLAN_NAMES)))
  return dict(zip(BSM_PLAN_NAMES, [int(x) for x in out]))


def batch_softmax_launch_counts():
  """{form: launches of this process} (mhte_batch_softmax_launch_counts)."""
  out = (C.c_int64 * len(BSM_COUNTER_NAMES))()
  check(_lib.lib().mhte_batch_softmax_launch_counts(out, len(BSM_COUNTER_NAMES)))
  return dict(zip(BSM_COUNTER_NAMES, [int(x) for x in out]))
