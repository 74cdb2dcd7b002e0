"""The truth of the CIN tests: the loop body of the reference's CIN.call (feature_cross.py:786-794) in float64, its
gradients by float64 autograd on the CPU, and the bound of every element.

One composition, written with torch so that autograd differentiates the very same lines, serves three purposes:
the value, the gradients, and (run a second time on the absolute values of every operand and upstream gradient
with the SAME relu mask) the sum of the absolute values of each element's terms.  An fp32 sum of n terms taken in
any order is within (n - 1) 2^-24 sum|terms| of the exact sum; the products and the bias add the rest of
``(n + 4) 2^-24 abs_run``, n the element's longest sum.  Through a chain of layers the lengths add.

A pre-activation within its own bound of 0 could flip relu's mask and move a gradient by whole terms: the truth
asserts that none is, so no element is ever left out of a comparison.
"""
import numpy as np
import torch

U24 = 2.0 ** -24


def layer(x0, xl, w, bias, mask):
  """x0 [B, D, m], xl [B, D, H], w [H m, U], bias [U]; mask: None, 'relu' or a [B, D, U] tensor of 0 / 1
  -> (pre-activation, mask as a tensor or None, out [B, D, U], pooled [B, U])."""
  B, D, m = x0.shape
  z = torch.einsum("bdh,bdm->bdhm", xl, x0).reshape(B, D, xl.shape[2] * m)
  pre = z @ w + bias
  if isinstance(mask, str):
    mask = (pre.detach() > 0).to(pre.dtype)
  out = pre if mask is None else pre * mask
  return pre, mask, out, out.sum(1)


def _t(a):
  return None if a is None else torch.tensor(np.asarray(a, dtype=np.float64))


def _far_from_zero(pre, pre_abs, n):
  assert bool((pre.abs() > (n + 4) * U24 * pre_abs).all()), "a pre-activation lies within its bound of 0: other seed"


def layer_truth(x0, xl, w, bias, relu, dxnext, dpooled):
  """Operands in the kernels' layout (x0 [B, m, D], xl [B, H, D], dxnext [B, U, D] or None) -> {name: (truth,
  bound)} for xnext, pooled, dx0, dxl, dw, dbias, in that layout."""
  ops = [_t(x0).transpose(1, 2), _t(xl).transpose(1, 2), _t(w), _t(bias)]
  ups = [None if dxnext is None else _t(dxnext).transpose(1, 2), _t(dpooled)]
  (B, D, m), H, U = ops[0].shape, ops[1].shape[2], ops[2].shape[1]
  pre, mask, _, _ = layer(*ops, "relu" if relu else None)
  if relu:
    _far_from_zero(pre, layer(*[o.abs() for o in ops], None)[0], H * m + 1)

  def run(ops, ups):
    ops = [o.clone().requires_grad_() for o in ops]
    _, _, out, pooled = layer(*ops, mask)
    loss = (pooled * ups[1]).sum() + (0 if ups[0] is None else (out * ups[0]).sum())
    return [out.detach(), pooled.detach()] + list(torch.autograd.grad(loss, ops))

  val, ab = run(ops, ups), run([o.abs() for o in ops], [None if u is None else u.abs() for u in ups])
  names = ("xnext", "pooled", "dx0", "dxl", "dw", "dbias")
  n = (H * m + 1, H * m + 1 + D, U * H, U + D, B * D, B * D)
  lay = lambda name, a: a.transpose(1, 2).numpy() if name in ("xnext", "dx0", "dxl") else a.numpy()   # noqa: E731
  return {k: (lay(k, v), (c + 4) * U24 * lay(k, a)) for k, v, a, c in zip(names, val, ab, n)}


def chain_truth(x, kernels, biases, relu, upstream):
  """CIN.call on x [B, m, D] with relu (or nothing) on every layer but the last -> {name: (truth, bound)} for
  result [B, sum U], dx and d<parameter name>, the parameters named kernel_i / bias_i."""
  B, m, D = x.shape
  L = len(kernels)
  hs = [m] + [k.shape[1] for k in kernels[:-1]]
  n_fwd = [h * m + 1 + D for h in hs]

  def forward(xin, ks, bs, masks):
    x0 = xin.transpose(1, 2)
    xl, pres, used, pooled = x0, [], [], []
    for i in range(L):
      pre, mk, xl, p = layer(x0, xl, ks[i], bs[i], masks[i])
      pres.append(pre), used.append(mk), pooled.append(p)
    return pres, used, torch.cat(pooled, 1)

  ops = [_t(x)] + [_t(k) for k in kernels] + [_t(b) for b in biases]
  pres, masks, _ = forward(ops[0], ops[1:1 + L], ops[1 + L:], ["relu" if relu and i < L - 1 else None for i in range(L)])
  pres_abs = forward(ops[0].abs(), [o.abs() for o in ops[1:1 + L]], [o.abs() for o in ops[1 + L:]], [None] * L)[0]
  for i in range(L - 1 if relu else 0):
    _far_from_zero(pres[i], pres_abs[i], sum(n_fwd[:i + 1]))

  def run(ops, up):
    ops = [o.clone().requires_grad_() for o in ops]
    res = forward(ops[0], ops[1:1 + L], ops[1 + L:], masks)[2]
    return [res.detach()] + list(torch.autograd.grad((res * up).sum(), ops))

  val, ab = run(ops, _t(upstream)), run([o.abs() for o in ops], _t(upstream).abs())
  names = ["result", "dx"] + ["dkernel_%d" % i for i in range(L)] + ["dbias_%d" % i for i in range(L)]
  n_grad = sum(n_fwd) + sum(k.shape[1] * h for k, h in zip(kernels, hs)) + B * D
  return {k: (v.numpy(), ((sum(n_fwd) if k == "result" else n_grad) + 4) * U24 * a.numpy())
          for k, v, a in zip(names, val, ab)}
