"""The truth of the DCN tests: the Vector and Matrix branches of the reference's DCN.call (feature_cross.py:564-568)
in float64, their gradients by float64 autograd on the CPU, and the bound of every element.

One composition, written with torch so that autograd differentiates the very same lines, serves three purposes: the
value, the gradients, and (run a second time on the absolute values of every operand and upstream gradient) the sum
of the absolute values of each element's terms.  An fp32 sum of n terms taken in any order is within
(n - 1) 2^-24 sum|terms| of the exact sum; the products, the bias and the residual add the rest of
``(n + 4) 2^-24 abs_run``, n the element's longest sum: d + 2 forward, 2 d + 2 for dxl (du's product, the row of w,
g), d + 6 for dx0 (the forward's u or s, then a product and two adds), B + d for dw and dbias.  Through a chain of
layers the lengths add.  There is no activation, so no element is ever left out of a comparison.
"""
import numpy as np
import torch

U24 = 2.0 ** -24


def layer(x0, xl, w, bias, matrix):
  """x0, xl [B, d], w [d, d] or [d, 1], bias [1, d] -> (xnext, aux): the reference's two lines."""
  if matrix:
    u = torch.matmul(xl, w) + bias
    return x0 * u + xl, u
  s = torch.matmul(xl, w)
  return x0 * s + bias + xl, s[:, 0]


def _t(a):
  return torch.tensor(np.asarray(a, dtype=np.float64))


def layer_truth(matrix, x0, xl, w, bias, g, dx0_acc):
  """-> {name: (truth, bound)} for xnext, aux, dx0 (= dx0_acc + the layer's part), dx0_alone (without dx0_acc), dxl,
  dw, dbias."""
  B, d = x0.shape

  def run(ops, g, acc):
    ops = [o.clone().requires_grad_() for o in ops]
    xnext, aux = layer(*ops, matrix)
    dx0, dxl, dw, db = torch.autograd.grad((xnext * g).sum(), ops)
    return [xnext.detach(), aux.detach(), acc + dx0, dx0, dxl, dw, db]

  ops = [_t(x0), _t(xl), _t(w), _t(bias)]
  val, ab = run(ops, _t(g), _t(dx0_acc)), run([o.abs() for o in ops], _t(g).abs(), _t(dx0_acc).abs())
  names = ("xnext", "aux", "dx0", "dx0_alone", "dxl", "dw", "dbias")
  n = (d + 2, d + 2, d + 6, d + 6, 2 * d + 2, B + d, B + d)
  return {k: (v.numpy(), (c + 4) * U24 * a.numpy()) for k, v, a, c in zip(names, val, ab, n)}


def chain_truth(matrix, x, kernels, biases, upstream):
  """DCN.call on x [B, d] -> {name: (truth, bound)} for result, dx and d<parameter name>, the parameters named
  kernel_i / bias_i."""
  B, d = x.shape
  L = len(kernels)

  def run(ops, up):
    ops = [o.clone().requires_grad_() for o in ops]
    xl = ops[0]
    for i in range(L):
      xl = layer(ops[0], xl, ops[1 + i], ops[1 + L + i], matrix)[0]
    return [xl.detach()] + list(torch.autograd.grad((xl * up).sum(), ops))

  ops = [_t(x)] + [_t(k) for k in kernels] + [_t(b) for b in biases]
  val, ab = run(ops, _t(upstream)), run([o.abs() for o in ops], _t(upstream).abs())
  names = ["result", "dx"] + ["dkernel_%d" % i for i in range(L)] + ["dbias_%d" % i for i in range(L)]
  n_fwd = L * (d + 2)
  n_grad = n_fwd + L * (2 * d + 2) + B + d
  return {k: (v.numpy(), ((n_fwd if k == "result" else n_grad) + 4) * U24 * a.numpy())
          for k, v, a in zip(names, val, ab)}
