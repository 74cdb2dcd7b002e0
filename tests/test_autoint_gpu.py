"""GPU suite of AutoInt (csrc/mhte_autoint_kernels.h, mhte_autoint_host.h, monolith_amd/layer_ops.py,
feature_trans.AutoInt) against the float64 truth of tests/autoint_truth.py within its bounds.  Every case checks
besides: a second call repeats the first one's bits, out has the same bits with and without the states buffer.

Measured on an MI355X (the largest share of its bound any case of this file used): out 0.396, dx 0.735; the module's
out 0.239, dx 0.487.  Every case prints its shares."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autoint_truth as T  # noqa: E402
from monolith_amd import layer_ops  # noqa: E402
from monolith_amd.feature_trans import AutoInt  # noqa: E402

pytestmark = pytest.mark.gpu

USED = {}
ROW_TILES = {15: 1, 16: 1, 17: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3, 128: 4}
CASES = ([(1, 1, 1, 1, 1), (2, 5, 3, 2, 1), (3, 10, 8, 3, 1)] + [(2, n, 5, 2, 1) for n in ROW_TILES] +
         [(2, 17, k, 2, 1) for k in (1, 3, 4, 15, 16, 17, 32, 33, 64)] + [(2, 7, k, 2, 1) for k in (3, 4, 64)] +
         [(2, 17, 5, L, 1) for L in (1, 3, 8)] + [(1, 128, 64, 2, 1), (2, 33, 17, 2, 6), (2, 40, 16, 3, 0.25)])
assert len(set(CASES)) == len(CASES)   # (2, 17, 5, 2), the k = 5 width edge, is among the n edges


def inputs(case):
  B, n, k, L, scale = case
  rng = np.random.default_rng(B + 10 * n + 1000 * k + 100000 * L)
  return [(rng.uniform(-1, 1, (B, n, k)) * s).astype(np.float32) for s in (scale, 1)]


def dev(a, offset=0):
  # with ``offset`` a view one float into its storage: 4-byte aligned only
  if not offset:
    return torch.from_numpy(a).cuda()
  store = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
  store[offset:offset + a.size] = torch.from_numpy(a).cuda().ravel()
  v = store[offset:offset + a.size].view(a.shape)
  assert v.data_ptr() % 16 == 4 * offset
  return v


def run(x, dout, L, offset=0):
  """-> {name: numpy} of the forward and the gradient call, after the bit checks."""
  x, dout = dev(x, offset), dev(dout, offset)
  bare, none = layer_ops.autoint_forward(x, L)
  out, states = layer_ops.autoint_forward(x, L, want_states=True)
  assert none is None and (states is None) == (L == 1) and torch.equal(bare, out)
  again = layer_ops.autoint_forward(x, L, want_states=True)
  assert torch.equal(again[0], out) and (L == 1 or torch.equal(again[1], states))
  dx = layer_ops.autoint_grad(dout, x, states, out, L)
  assert torch.equal(dx, layer_ops.autoint_grad(dout, x, states, out, L))
  return {"out": out.cpu().numpy(), "dx": dx.cpu().numpy()}


def within(got, truth, what, tag=""):
  for name, g in got.items():
    want, bound = truth[name]
    assert g.shape == want.shape, (what, name)
    share = float(np.abs(g.astype(np.float64) - want).max()) / bound
    USED[tag + name] = max(USED.get(tag + name, 0.0), share)
    print("%s %s: share of the bound %.3f (largest so far %.3f)" % (what, tag + name, share, USED[tag + name]))
    assert share <= 1, "%s %s: %.3g of its bound %.3g" % (what, name, share, bound)


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d-L%d-s%s" % c for c in CASES])
def test_stack_and_gradient_within_bounds(case):
  B, n, k, L, scale = case
  if (B, k, L, scale) == (2, 5, 2, 1) and n in ROW_TILES:
    assert layer_ops.autoint_plan(B, n, k, L)["row_tiles"] == ROW_TILES[n]
  x, dout = inputs(case)
  within(run(x, dout, L), T.truth(x, dout, L), str(case))


@pytest.mark.parametrize("case", [(3, 17, 10, 2, 1), (2, 7, 20, 3, 1)])
def test_operands_4_byte_aligned_only(case):
  x, dout = inputs(case)
  aligned, shifted = run(x, dout, case[3]), run(x, dout, case[3], offset=1)
  assert all(np.array_equal(aligned[name].view(np.uint32), shifted[name].view(np.uint32)) for name in aligned)


def test_module_through_autograd():
  x, dout = inputs((3, 39, 16, 3, 1))
  xt, up = torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(dout).cuda()
  counts = lambda: tuple(layer_ops.autoint_launch_counts()[name] for name in ("forward", "grad"))  # noqa: E731
  c0 = counts()
  with torch.no_grad():
    bare = AutoInt(3, "stack")(xt)
  c1 = counts()
  assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0)
  layer = AutoInt(3, "stack")
  out = layer(xt)
  out.backward(up)
  c2 = counts()
  assert (c2[0] - c1[0], c2[1] - c1[1]) == (1, 1)
  assert torch.equal(bare, out) and not list(layer.parameters())
  with torch.no_grad():
    concat, listed, kept = AutoInt(3)(xt), AutoInt(3, None)(xt), AutoInt(3, "concat", keep_list=True)(xt)
  assert concat.shape == (3, 39 * 16) and torch.equal(concat, out.reshape(3, -1))
  assert len(listed) == 39 and all(t.shape == (3, 16) for t in listed) and torch.equal(torch.stack(listed, 1), out)
  assert isinstance(kept, list) and len(kept) == 1 and torch.equal(kept[0], concat)
  got = {"out": out.detach().cpu().numpy(), "dx": xt.grad.cpu().numpy()}
  within(got, T.truth(x, dout, 3), "through autograd:", "module ")
