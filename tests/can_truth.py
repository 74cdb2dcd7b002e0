"""The truth of the CAN tests: the reference's CAN.call (feature_cross.py:386-430) in float64, its gradients by
float64 autograd on the CPU, and the bound of every element.

One composition, written with torch so that autograd differentiates the very same lines, serves three purposes: the
value, the gradients, and (run a second time on the absolute values of every operand and upstream gradient with the
SAME relu masks) the sum of the absolute values of each element's terms.  An fp32 sum of n terms taken in any order
is within (n - 1) 2^-24 sum|terms| of the exact sum; the products and the bias add the rest of
``(n + 4) 2^-24 abs_run``, n the element's longest chain of sums.  Through the layers the lengths add:
  out     L (d + 1) + T          per layer d products and the bias, then the T rows of the feature
  duser   L (d + 1) + T + L d    the forward chain, then per layer the d terms of dpre W_i^T
  ditem   L (d + 1) + T + L d + R   the chains, then the R = F T rows of the sample
with L = layer_num.

A pre-activation within its own bound of 0 could flip relu's mask and move a gradient by whole terms: the truth
asserts that none is, so no element is ever left out of a comparison (the share left out is 0 by construction).
"""
import numpy as np
import torch

U24 = 2.0 ** -24


def call(user, item, layer_num, masks):
  """user [B, F, T, d], item [B, P]; masks[i]: None, 'relu' or a [B, F, T, d] tensor of 0 / 1
  -> (pre-activations, masks as tensors or None, out [B, F, d])."""
  B, _, _, d = user.shape
  h, pres, used = user, [], []
  for i in range(layer_num):
    o = i * d * (d + 1)
    weight = item[:, o:o + d * d].reshape(B, 1, d, d)
    bias = item[:, o + d * d:o + d * (d + 1)].reshape(B, 1, 1, d)
    pre = torch.matmul(h, weight) + bias
    mask = (pre.detach() > 0).to(pre.dtype) if isinstance(masks[i], str) else masks[i]
    h = pre if mask is None else pre * mask
    pres.append(pre), used.append(mask)
  return pres, used, h.sum(2)


def truth(user, item, dout, layer_num, relu, is_seq, is_stacked):
  """Operands in the form's own shapes -> {name: (truth, bound)} for out, duser, ditem, in those shapes."""
  B, d = user.shape[0], user.shape[-1]
  F = user.shape[1] if is_stacked else 1
  T = user.shape[-2] if is_seq else 1
  t = lambda a, *s: torch.tensor(np.asarray(a, dtype=np.float64)).reshape(*s)   # noqa: E731
  ops, up = [t(user, B, F, T, d), t(item, B, -1)], t(dout, B, F, d)
  pres, masks, _ = call(*ops, layer_num, ["relu" if relu else None] * layer_num)
  if relu:
    pres_abs = call(*[o.abs() for o in ops], layer_num, [None] * layer_num)[0]
    for i, (pre, pre_abs) in enumerate(zip(pres, pres_abs)):
      assert bool((pre.abs() > ((i + 1) * (d + 1) + 4) * U24 * pre_abs).all()), \
          "a pre-activation lies within its bound of 0: other seed"

  def run(ops, up):
    ops = [o.clone().requires_grad_() for o in ops]
    out = call(*ops, layer_num, masks)[2]
    return [out.detach()] + list(torch.autograd.grad((out * up).sum(), ops))

  val, ab = run(ops, up), run([o.abs() for o in ops], up.abs())
  n_out = layer_num * (d + 1) + T
  n = (n_out, n_out + layer_num * d, n_out + layer_num * d + F * T)
  shapes = ((B, F, d) if is_stacked else (B, d), user.shape, item.shape)
  return {k: (v.reshape(s).numpy(), (c + 4) * U24 * a.reshape(s).numpy())
          for k, v, a, c, s in zip(("out", "duser", "ditem"), val, ab, n, shapes)}
