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
