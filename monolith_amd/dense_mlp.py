"""The dense tower downstream of the embedding path on the MI355X matrix cores (C ABI
mhte_dense_mlp_*, csrc/mhte_gemm_kernels.h): the ranking MLP that consumes
``fused_embedding_to_layout``'s output — a stack of Dense + ReLU layers ending in one logit
(native_training/layers/mlp.py) — as hand-written bf16 MFMA GEMMs with fp32 master weights, fp32
accumulation and SGD inside ``backward``.

  mlp = DenseMlp([1024, 1024, 512, 256, 1], max_batch=65536)
  y = mlp.forward(x)                 # x [B, 1024] fp32 on the GPU -> y [B] fp32
  dx = mlp.backward(dy, lr=1e-3)     # dy [B] = dLoss/dy; SGD step on every layer; dx [B, 1024]

With an optimizer outside the tower (data-parallel training, a clip over dense and sparse gradients together,
the dense optimizers of ``monolith_amd.optimizers``) the gradients leave the tower and the parameters come
back, one launch each for all layers (mhte_dense_mlp_backward_grads / mhte_dense_mlp_load_params):

  variables = mlp.variables()                       # fp32 copies of the masters: the optimizer's variables
  opt = optimizers.AdamomOptimizer(learning_rate=...)   # binds the variables at its first apply
  # every step
  y = mlp.forward(x)
  dx, grads = mlp.backward_grads(dy)                # [dW_0, db_0, ..., dW_last, db_last]; no SGD
  sparse_scale = feature_utils.clip_allreduce_and_apply(opt, zip(grads, variables), sparse_grads,
                                                        clip_norm=..., use_allreduce=True)
  mlp.load_params(variables)                        # masters and bf16 copies; does not synchronise

``backward(dy, lr)`` from the same state leaves exactly ``p - lr * g`` for the exported ``g``.

Widths (but the final 1) and batches are multiples of 128 (the GEMM tile).  No fallback: without the
library or a GPU every call raises."""
import ctypes as C

import torch

from . import _lib


class DenseMlp:
  def __init__(self, widths, max_batch, device=None):
    self.widths = [int(w) for w in widths]
    self.max_batch = int(max_batch)
    self._lib = _lib.lib()
    import os
    if os.environ.get("MHTE_DENSE_LIBRARY"):   # development builds of the tower alone (scripts/dbg/gemm_dev.hip)
      self._lib = _lib.bind(C.CDLL(os.environ["MHTE_DENSE_LIBRARY"]), only_present=True)
    self._device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    arr = (C.c_int32 * len(self.widths))(*self.widths)
    h = C.c_void_p()
    _lib.check(self._lib.mhte_dense_mlp_create(arr, len(self.widths), self.max_batch, self._device.index,
                                               C.byref(h)))
    self._h = h
    self._batch = 0

  @property
  def n_layers(self):
    return len(self.widths) - 1

  def _stream(self):
    return C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

  def set_params(self, layer, weight, bias):
    """weight [out, in] (torch.nn.Linear's layout; [1, in] or [in] for the last layer), bias [out]."""
    w = weight.detach().to(self._device, torch.float32).contiguous()
    b = bias.detach().to(self._device, torch.float32).contiguous()
    assert w.numel() == self.widths[layer] * self.widths[layer + 1] and b.numel() == self.widths[layer + 1]
    _lib.check(self._lib.mhte_dense_mlp_set_params(self._h, layer, _lib.vp(w), _lib.vp(b),
                                                   self._stream()))
    torch.cuda.current_stream(self._device).synchronize()   # (w, b may be temporaries)

  def get_params(self, layer):
    w = torch.empty(self.widths[layer + 1], self.widths[layer], dtype=torch.float32, device=self._device)
    b = torch.empty(self.widths[layer + 1], dtype=torch.float32, device=self._device)
    _lib.check(self._lib.mhte_dense_mlp_get_params(self._h, layer, _lib.vp(w), _lib.vp(b),
                                                   self._stream()))
    return w, b

  def forward(self, x, out=None):
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == self.widths[0]
    B = x.shape[0]
    y = out if out is not None else torch.empty(B, dtype=torch.float32, device=self._device)
    _lib.check(self._lib.mhte_dense_mlp_forward(self._h, _lib.vp(x), B, _lib.vp(y), self._stream()))
    self._batch = B
    self._keep = x
    return y

  def backward(self, dy, lr, need_dx=True, out=None):
    assert dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == self._batch
    dx = None
    if need_dx:
      dx = out if out is not None else torch.empty(self._batch, self.widths[0], dtype=torch.float32,
                                                   device=self._device)
    _lib.check(self._lib.mhte_dense_mlp_backward(self._h, _lib.vp(dy), _lib.vp(dx), lr, self._stream()))
    return dx

  def param_shapes(self):
    """[(out, in), (out,)] per layer in the order of ``variables`` / ``backward_grads``: GEMM layers, then the
    row-dot layer ((1, in), (1,))."""
    shapes = []
    for l in range(self.n_layers):
      shapes += [(self.widths[l + 1], self.widths[l]), (self.widths[l + 1],)]
    return shapes

  def _checked(self, what, tensors):
    """``tensors``: fp32, contiguous, on this device, with the numels of ``param_shapes`` -> the two pointer
    tables (weights, biases) of the C ABI."""
    shapes = self.param_shapes()
    if not isinstance(tensors, (list, tuple)) or len(tensors) != len(shapes):
      raise ValueError("%s: a list of %d tensors [W_0, b_0, ..., W_last, b_last], got %s" %
                       (what, len(shapes), len(tensors) if isinstance(tensors, (list, tuple)) else type(tensors)))
    for i, (t, s) in enumerate(zip(tensors, shapes)):
      name = "%s[%d] (%s of layer %d)" % (what, i, "bias" if i % 2 else "weight", i // 2)
      if not (isinstance(t, torch.Tensor) and t.device == self._device and t.dtype == torch.float32):
        raise TypeError("%s must be a float32 tensor on %s" % (name, self._device))
      if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
      n = s[0] * (s[1] if len(s) == 2 else 1)
      if t.numel() != n:
        raise ValueError("%s must have %d elements, got %d" % (name, n, t.numel()))
    n = self.n_layers
    return ((C.c_void_p * n)(*[t.data_ptr() for t in tensors[0::2]]),
            (C.c_void_p * n)(*[t.data_ptr() for t in tensors[1::2]]))

  def backward_grads(self, dy, need_dx=True, out=None, grads=None):
    """The backward of ``backward`` WITHOUT the SGD step -> ``(dx, grads)``; ``grads`` =
    ``[dW_0, db_0, ..., dW_last, db_last]`` (fp32, ``param_shapes``), new tensors unless given.  The
    parameters keep their bits; ``backward(dy, lr)`` from the same state leaves ``p - lr * g``.  Given tensors
    may be views into one flat buffer at ``distribution_ops.aligned_flat_offsets`` (the allreduce buffer)."""
    assert dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous() and dy.numel() == self._batch
    if grads is None:
      grads = [torch.empty(s, dtype=torch.float32, device=self._device) for s in self.param_shapes()]
    wg, bg = self._checked("grads", grads)
    dx = None
    if need_dx:
      dx = out if out is not None else torch.empty(self._batch, self.widths[0], dtype=torch.float32,
                                                   device=self._device)
    _lib.check(self._lib.mhte_dense_mlp_backward_grads(self._h, _lib.vp(dy), _lib.vp(dx), wg, bg, self._stream()))
    return dx, list(grads)

  def variables(self):
    """A fresh list ``[W_0, b_0, ..., W_last, b_last]`` of fp32 COPIES of the master parameters: the variables
    an optimizer owns (``load_params`` brings them back)."""
    out = []
    for l in range(self.n_layers):
      out += list(self.get_params(l))
    return out

  def load_params(self, variables):
    """All parameters from ``variables`` (the order and shapes of ``variables()``) into the masters and the bf16
    copies, in one launch.  Does not synchronise: the list is kept until the next call, so that temporaries
    stay alive; tensors the caller keeps must not change before the stream has passed the call."""
    w, b = self._checked("variables", variables)
    _lib.check(self._lib.mhte_dense_mlp_load_params(self._h, w, b, self._stream()))
    self._loaded = list(variables)

  GEMM_ROLES = ("forward", "dgrad", "dgrad_input", "wgrad")

  def launch_counts(self):
    """{role: (launches with the 128 x 128 tile, with the 256 x 256 tile)} of this handle's GEMMs since
    it was created (mhte_dense_mlp_launch_counts): which instantiation a shape reached."""
    out = (C.c_int64 * 8)()
    _lib.check(self._lib.mhte_dense_mlp_launch_counts(self._h, out))
    return {r: (int(out[2 * i]), int(out[2 * i + 1])) for i, r in enumerate(self.GEMM_ROLES)}

  def close(self):
    if getattr(self, "_h", None):
      torch.cuda.synchronize(self._device)
      self._lib.mhte_dense_mlp_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass
