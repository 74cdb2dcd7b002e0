"""The truth of the AutoInt tests: the three lines of the reference's AutoInt.call (feature_trans.py:75-80) composed
in torch, used three ways: in float64 for ``out``, through float64 autograd for ``dx`` given ``dout``, and in float32
on the CPU for the comparison error.  Per tensor

    bound = 4 * ( max|ref32 - truth| + 2^-24 * max|truth| )

a scalar, compared elementwise.  The softmax's terms are no polynomial in the operands, so the tolerance is measured
against an fp32 evaluation of the reference; the floor covers shapes where that evaluation is exact (n == 1); the
margin 4 leaves room for the device's exp and the MFMA's sum order.
"""
import numpy as np
import torch

U24, MARGIN = 2.0 ** -24, 4.0


def stack(x, layer_num):
  for _ in range(layer_num):
    x = torch.matmul(torch.softmax(torch.matmul(x, x.transpose(1, 2)), dim=-1), x)
  return x


def run(x, dout, layer_num, dtype):
  x = torch.tensor(np.asarray(x), dtype=dtype).requires_grad_()
  out = stack(x, layer_num)
  dx, = torch.autograd.grad((out * torch.tensor(np.asarray(dout), dtype=dtype)).sum(), x)
  return {"out": out.detach().numpy(), "dx": dx.numpy()}


def truth(x, dout, layer_num):
  """x, dout [B, n, k] float32 -> {name: (float64 truth, scalar bound)} for out and dx."""
  t64, t32 = run(x, dout, layer_num, torch.float64), run(x, dout, layer_num, torch.float32)
  return {name: (t, MARGIN * (float(np.abs(t32[name].astype(np.float64) - t).max()) + U24 * float(np.abs(t).max())))
          for name, t in t64.items()}
