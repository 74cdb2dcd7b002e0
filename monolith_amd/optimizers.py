"""Dense optimizers on MI355X — host-side mirror of monolith/native_training/optimizers/: ``AdamomOptimizer``
(adamom.py, the reference's ``ResourceApplyAdamom`` is CPU only) and ``RmspropOptimizer`` (rmsprop.py,
``ResourceApplyRmsprop`` V1 / V2).

One launch applies the update to ALL variables (include/monolith_amd_hash_table.h, "dense optimizers";
csrc/mhte_dense_opt_core.h states the arithmetic, tests/dense_opt_truth.py restates it).  The gradient is read
where the step left it: a list of tensors (``apply_gradients``) or the aligned flat buffer of the allreduce,
fp32 or fp16 (``apply_flat``: no fp32 copy of the gradients is written).  The gradient scale and the learning
rate may be 0-d float32 device tensors — the deferred clip's scale (``clip_ops.global_norm_and_scale``), a
schedule that stays on the device — and are then read by the kernel.  Nothing here waits for the GPU or reads
a device value, so an apply can be captured into a graph (up to ``_lib.DENSE_OPT_INLINE`` variables).

Variables are contiguous float32 GPU tensors, updated in place.  The slots are FLAT: one float32 buffer per
slot name in the layout of ``distribution_ops.aligned_flat_offsets(numels, align)`` — the layout of the flat
gradient buffer — and ``get_slot`` returns views of them.
"""
import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from monolith_amd import _lib
from monolith_amd._lib import check, vp
from monolith_amd.distribution_ops import _WIRE, aligned_flat_offsets
from monolith_amd.multi_hash_table_ops import _stream

Scalar = Union[float, torch.Tensor]


def _host_or_dev(x, what) -> Tuple[float, Optional[torch.Tensor]]:
  """A Python number or a 0-d float32 device tensor -> (host value, device word or None)."""
  if isinstance(x, torch.Tensor):
    if not (x.is_cuda and x.dtype == torch.float32 and x.numel() == 1):
      raise TypeError("%s must be a float or a 0-d float32 tensor on the GPU" % what)
    return 1.0, x
  return float(x), None


class _DenseOptimizer:
  """What the two optimizers share: the fixed variable list, the flat slots, the two gradient sources."""
  _NAME = ""
  _SLOTS: Tuple[str, ...] = ()

  def __init__(self, learning_rate, weight_decay: float, use_v2: bool, align: int):
    self._learning_rate = learning_rate
    self._weight_decay = float(weight_decay)
    self._use_v2 = bool(use_v2)
    self._align = int(align)
    aligned_flat_offsets([], self._align)   # (refuses a bad align now, not at the first apply)
    self._vars: Optional[List[torch.Tensor]] = None
    self._numels: List[int] = []
    self._offsets: List[int] = []
    self._slots: Dict[str, torch.Tensor] = {}
    self._pending: Optional[dict] = None   # a state loaded before the variables are known

  # ---- the variables and their slots --------------------------------------------------------------------
  @property
  def align(self) -> int:
    return self._align

  def get_slot_names(self) -> List[str]:
    return list(self._SLOTS)

  def _check_vars(self, variables: Sequence[torch.Tensor]):
    for v in variables:
      if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()):
        raise TypeError("%s: the variables must be contiguous float32 tensors on the GPU" % self._NAME)

  def _create_slots(self, variables: Sequence[torch.Tensor]):
    """The first apply fixes the variable list (identity and order) and creates the zero slots."""
    variables = list(variables)
    if not variables:
      raise ValueError("%s: an empty variable list has no device to keep the slots on" % self._NAME)
    self._check_vars(variables)
    numels = [v.numel() for v in variables]
    offsets = aligned_flat_offsets(numels, self._align)
    dev = variables[0].device
    if self._pending is not None:
      st = self._pending
      if list(st["numels"]) != numels:
        raise ValueError("%s: the loaded state is for variables of %s elements, these have %s" %
                         (self._NAME, list(st["numels"]), numels))
      slots = {k: st[k].to(device=dev, dtype=torch.float32, copy=True).contiguous() for k in self._SLOTS}
      self._pending = None
    else:
      slots = {k: torch.zeros(offsets[-1], dtype=torch.float32, device=dev) for k in self._SLOTS}
    self._vars, self._numels, self._offsets, self._slots = variables, numels, offsets, slots

  def _bind(self, variables: Optional[Sequence[torch.Tensor]]):
    if self._vars is None:
      if variables is None:
        raise ValueError("%s: the first apply needs the variables" % self._NAME)
      self._create_slots(variables)
    elif variables is not None:
      variables = list(variables)
      if len(variables) != len(self._vars) or any(a is not b for a, b in zip(variables, self._vars)):
        raise ValueError("%s: the variable list is fixed by the first apply (identity and order); "
                         "this call brings another one" % self._NAME)
      self._check_vars(self._vars)   # (a variable may have been moved or re-laid since)

  def get_slot(self, var: torch.Tensor, name: str) -> torch.Tensor:
    """The slot ``name`` of ``var``: a view of the flat slot buffer with the variable's shape."""
    if name not in self._SLOTS:
      raise KeyError("%s has the slots %s, not '%s'" % (self._NAME, list(self._SLOTS), name))
    if self._vars is not None:
      for i, v in enumerate(self._vars):
        if v is var:
          o = self._offsets[i]
          return self._slots[name][o:o + self._numels[i]].view(var.shape)
    raise KeyError("%s: not a variable of this optimizer" % self._NAME)

  def state_dict(self) -> dict:
    """The flat slot buffers (references, not copies) plus the variables' numels and the alignment."""
    if self._vars is None:
      raise ValueError("%s: no slots before the first apply" % self._NAME)
    st = {k: self._slots[k] for k in self._SLOTS}
    st["numels"] = list(self._numels)
    st["align"] = self._align
    return st

  def load_state_dict(self, state: dict):
    """Copies the flat slot buffers of ``state`` in, padding included.  Before the first apply the state is
    kept and adopted when the variables are known."""
    if int(state["align"]) != self._align:
      raise ValueError("%s: the state was saved with align %d, this optimizer has %d" %
                       (self._NAME, int(state["align"]), self._align))
    numels = [int(x) for x in state["numels"]]
    total = aligned_flat_offsets(numels, self._align)[-1]
    for k in self._SLOTS:
      t = state[k]
      if not (isinstance(t, torch.Tensor) and t.dim() == 1 and t.numel() == total):
        raise ValueError("%s: slot '%s' of the state must be a 1-d tensor of %d elements" % (self._NAME, k, total))
    if self._vars is None:
      self._pending = {"numels": numels, **{k: state[k] for k in self._SLOTS}}
      return
    if numels != self._numels:
      raise ValueError("%s: the state is for variables of %s elements, these have %s" %
                       (self._NAME, numels, self._numels))
    for k in self._SLOTS:
      self._slots[k].copy_(state[k])

  # ---- the apply ----------------------------------------------------------------------------------------
  def _lr(self) -> Scalar:
    lr = self._learning_rate
    return lr() if callable(lr) else lr   # (the reference's _call_if_callable, per apply)

  def _call(self, pvar, lens, n, slot_elems, pgrad, flat, wire, gs, gs_dev, lr, lr_dev, update_slots):
    raise NotImplementedError

  def _apply(self, grads: Optional[List[Optional[torch.Tensor]]], flat: Optional[torch.Tensor], scale: Scalar,
             update_slots: bool):
    n = len(self._vars)
    pvar = (C.c_void_p * n)(*[C.c_void_p(v.data_ptr()) for v in self._vars])
    lens = (C.c_int64 * n)(*self._numels)
    pgrad = None
    if grads is not None:
      pgrad = (C.c_void_p * n)(*[C.c_void_p(0 if g is None else g.data_ptr()) for g in grads])
    gs, gs_dev = _host_or_dev(scale, "%s: the gradient scale" % self._NAME)
    lr, lr_dev = _host_or_dev(self._lr(), "%s: learning_rate" % self._NAME)
    self._call(pvar, lens, n, self._offsets[-1], pgrad, vp(flat), 0 if flat is None else _WIRE[flat.dtype],
               gs, vp(gs_dev), lr, vp(lr_dev), 1 if update_slots else 0)

  def apply_gradients(self, grads_and_vars, grad_scale: Scalar = 1.0, update_slots: bool = True):
    """One launch: every variable with a gradient takes the step with ``grad * grad_scale``; a variable whose
    gradient is ``None`` is skipped, slots included.  ``grad_scale``: a float or a 0-d float32 device tensor."""
    pairs = list(grads_and_vars)
    self._bind([v for _, v in pairs])
    grads = []
    for g, v in pairs:
      if g is not None:
        if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32):
          raise TypeError("%s: the gradients must be float32 tensors on the GPU" % self._NAME)
        if g.numel() != v.numel():
          raise ValueError("%s: a gradient of %d elements for a variable of %d" % (self._NAME, g.numel(), v.numel()))
        g = g if g.is_contiguous() else g.contiguous()
      grads.append(g)
    self._apply(grads, None, grad_scale, update_slots)

  def apply_flat(self, flat: torch.Tensor, variables: Optional[Sequence[torch.Tensor]] = None,
                 post_scale: Optional[Scalar] = None, update_slots: bool = True):
    """One launch: the gradients are read straight from ``flat``, the aligned flat buffer the allreduce left
    (``distribution_ops.aligned_flat_concat`` with this optimizer's ``align``), float32 or float16, each times
    ``post_scale`` (``1 / world``; ``None`` is 1).  The same bits as ``aligned_flat_split`` followed by
    ``apply_gradients``, without the fp32 copy of the gradients."""
    self._bind(variables)
    if not (isinstance(flat, torch.Tensor) and flat.is_cuda and flat.dtype in _WIRE and flat.dim() == 1 and
            flat.is_contiguous()):
      raise TypeError("%s: flat must be a contiguous 1-d float32 or float16 tensor on the GPU" % self._NAME)
    if flat.numel() != self._offsets[-1]:
      raise ValueError("%s: flat has %d elements, the variables need %d" %
                       (self._NAME, flat.numel(), self._offsets[-1]))
    self._apply(None, flat, 1.0 if post_scale is None else post_scale, update_slots)


class AdamomOptimizer(_DenseOptimizer):
  """optimizers/adamom.py AdamomOptimizer: slots ``m``, ``v``, ``c``."""
  _NAME = "AdamomOptimizer"
  _SLOTS = ("m", "v", "c")

  def __init__(self, learning_rate: Union[float, Callable[[], Scalar], torch.Tensor] = 5e-6,
               ada_decay: float = 0.9999, mom_decay: float = 0.99, epsilon: float = 1e-6,
               weight_decay: float = 0.0, use_v2: bool = False, align: int = 16):
    super().__init__(learning_rate, weight_decay, use_v2, align)
    self._ada_decay, self._mom_decay, self._epsilon = float(ada_decay), float(mom_decay), float(epsilon)

  def _call(self, pvar, lens, n, slot_elems, pgrad, flat, wire, gs, gs_dev, lr, lr_dev, update_slots):
    s = self._slots
    check(_lib.lib().mhte_dense_apply_adamom(pvar, lens, n, self._align, vp(s["m"]), vp(s["v"]), vp(s["c"]),
                                             slot_elems, pgrad, flat, wire, gs, gs_dev, lr, lr_dev,
                                             self._ada_decay, self._mom_decay, self._epsilon, self._weight_decay,
                                             update_slots, 1 if self._use_v2 else 0, _stream()))


class RmspropOptimizer(_DenseOptimizer):
  """optimizers/rmsprop.py RmspropOptimizer: slots ``m``, ``v``.  Without ``update_slots`` an apply changes
  nothing, the variables included (as the reference's kernel does)."""
  _NAME = "RmspropOptimizer"
  _SLOTS = ("m", "v")

  def __init__(self, learning_rate: Union[float, Callable[[], Scalar], torch.Tensor] = 5e-6,
               beta1: float = 0.99, beta2: float = 0.999, epsilon: float = 1e-8, weight_decay: float = 0.0,
               use_v2: bool = False, align: int = 16):
    super().__init__(learning_rate, weight_decay, use_v2, align)
    self._beta1, self._beta2, self._epsilon = float(beta1), float(beta2), float(epsilon)

  def _call(self, pvar, lens, n, slot_elems, pgrad, flat, wire, gs, gs_dev, lr, lr_dev, update_slots):
    s = self._slots
    check(_lib.lib().mhte_dense_apply_rmsprop(pvar, lens, n, self._align, vp(s["m"]), vp(s["v"]), slot_elems,
                                              pgrad, flat, wire, gs, gs_dev, lr, lr_dev, self._beta1,
                                              self._beta2, self._epsilon, self._weight_decay, update_slots,
                                              1 if self._use_v2 else 0, _stream()))
