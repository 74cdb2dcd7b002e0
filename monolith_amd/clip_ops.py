"""Clip by global norm on MI355X — host-side mirror of monolith/native_training/clip_ops.py.

The reference clips every gradient of a model by one global norm (feature_utils.apply_gradients,
``GradClipType.ClipByGlobalNorm``): the dense gradients through ``clip_by_global_norm``, the sparse ones
through a scale tensor ``min(clip_norm / norm, 1)`` that travels into
``fused_gather_embeddings_by_input_gradient`` and in front of ``fused_embedding_to_layout_grad``.  Here the
norm is one fixed summation tree (include/monolith_amd_hash_table.h, csrc/mhte_clip_kernels.h: the same
bits on every run), and norm and scale stay on the device: no function of this module waits for the GPU
or reads a device value, so the whole path can be captured into a graph and replayed.

Tensors are float32 and on the GPU; a tensor that is not contiguous is copied first (and can then not be
clipped in place).
"""
import ctypes as C
from typing import List, Optional, Tuple, Union

import torch

from monolith_amd import _lib
from monolith_amd._lib import check, vp
from monolith_amd.multi_hash_table_ops import _stream

_INF = float("inf")


def _plan(t_list, inplace, what, want_out=True):
  """-> (inputs, outputs, the two pointer arrays, lens, n); outputs are the inputs when ``inplace``."""
  ins = []
  for t in t_list:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
      raise TypeError("%s: the tensors must be float32 tensors on the GPU" % what)
    if inplace and not t.is_contiguous():
      raise ValueError("%s: inplace=True needs contiguous tensors" % what)
    ins.append(t if t.is_contiguous() else t.contiguous())
  outs = ins if inplace or not want_out else [torch.empty_like(t) for t in ins]
  n = len(ins)
  pin = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in ins])
  pout = (C.c_void_p * n)(*[C.c_void_p(t.data_ptr()) for t in outs])
  lens = (C.c_int64 * n)(*[t.numel() for t in ins])
  return ins, outs, pin, pout, lens, n


def _result_block(t_list):
  return torch.empty(4, dtype=torch.float32, device=t_list[0].device)


def global_norm_and_scale(t_list: List[torch.Tensor], clip_norm: float) -> Tuple[torch.Tensor, torch.Tensor]:
  """(global norm, min(clip_norm / norm, 1)) as 0-d views of one device result block — the deferred branch
  of feature_utils' cond_defer_clip: the scale goes to ``scale_tensors`` and to
  ``distribution_ops.fused_gather_embeddings_by_input_gradient(scale=...)`` without leaving the GPU."""
  if not isinstance(t_list, list):
    raise TypeError("t_list should be a list")
  if not t_list:
    raise ValueError("global_norm_and_scale: an empty list has no device to keep the result on")
  ins, _, pin, _, lens, n = _plan(t_list, False, "global_norm_and_scale", want_out=False)
  res = _result_block(ins)
  check(_lib.lib().mhte_global_l2_reduce(pin, lens, n, float(clip_norm), vp(res), _stream()))
  return res[1], res[2]


def _global_norm(t_list: List[torch.Tensor]) -> Optional[torch.Tensor]:
  """clip_ops._global_norm (reference :25-30): sqrt(GlobalL2Reduce(t_list)) as a 0-d device tensor."""
  if len(t_list) == 0:
    return None
  return global_norm_and_scale(list(t_list), _INF)[0]


def clip_by_global_norm(t_list: List[torch.Tensor], clip_norm: float,
                        use_norm: Union[None, float, torch.Tensor] = None,
                        inplace: bool = False):
  """clip_ops.clip_by_global_norm (reference :33-80) -> (list_clipped, global_norm):
  ``t * clip_norm / max(global_norm, clip_norm)``; an infinite norm gives NaN everywhere, a norm that is
  not above ``clip_norm`` gives the inputs' values.  ``use_norm``: a Python float (MonolithClipByGlobalNorm
  with the norm known to the host) or a 0-d device tensor (the norm never leaves the GPU); without it the
  fused form computes the norm (MonolithClipByGlobalNormFused) and returns it as a 0-d device tensor.
  The inputs are modified only with ``inplace=True``; the clipped list is then the inputs themselves."""
  if not isinstance(t_list, list):
    raise TypeError("t_list should be a list")
  if len(t_list) == 0:
    return t_list, 0
  ins, outs, pin, pout, lens, n = _plan(t_list, inplace, "clip_by_global_norm")
  L = _lib.lib()
  if use_norm is None:
    res = _result_block(ins)
    check(L.mhte_clip_by_global_norm_fused(pin, pout, lens, n, float(clip_norm), vp(res), _stream()))
    return outs, res[1]
  if isinstance(use_norm, torch.Tensor):
    if not (use_norm.is_cuda and use_norm.dtype == torch.float32 and use_norm.numel() == 1):
      raise TypeError("clip_by_global_norm: use_norm must be a float or a 0-d float32 tensor on the GPU")
    check(L.mhte_clip_by_global_norm_dev(pin, pout, lens, n, vp(use_norm), float(clip_norm), _stream()))
    return outs, use_norm
  check(L.mhte_clip_by_global_norm(pin, pout, lens, n, float(use_norm), float(clip_norm), _stream()))
  return outs, use_norm


def scale_tensors(t_list: List[torch.Tensor], scale_tensor: torch.Tensor, inplace: bool = False):
  """``[t * scale_tensor for t in t_list]`` in one launch, the factor read on the device — the multiply the
  reference does per layout tensor with ``layout_tensors_grad_scale`` (distribution_ops.py:535-549).  With
  ``inplace=True`` and a factor of exactly 1 nothing is loaded or stored."""
  if not isinstance(t_list, list):
    raise TypeError("t_list should be a list")
  if not (isinstance(scale_tensor, torch.Tensor) and scale_tensor.is_cuda and
          scale_tensor.dtype == torch.float32 and scale_tensor.numel() == 1):
    raise TypeError("scale_tensors: scale_tensor must be a 0-d float32 tensor on the GPU")
  if len(t_list) == 0:
    return t_list
  _, outs, pin, pout, lens, n = _plan(t_list, inplace, "scale_tensors")
  check(_lib.lib().mhte_scale_tensors_dev(pin, pout, lens, n, vp(scale_tensor), _stream()))
  return outs
