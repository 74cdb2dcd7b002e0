"""GPU suite of the CIN layer (csrc/mhte_cin_kernels.h, mhte_cin_host.h, monolith_amd/layer_ops.py,
feature_cross.CIN) against the float64 truth of tests/cin_truth.py within its derived bounds.  Every layer case
checks besides: a second call repeats the first one's bits, a gradient asked for alone has the bits it has in the
full call, every zero is +0.

Measured on an MI355X (the largest share of its bound any layer case of this file used): xnext 0.19, pooled 0.12,
dx0 0.24, dxl 0.20, dw 0.23, dbias 0.18; the module's elements stay below 0.01 of their chained bounds.  Every case
prints its shares."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cin_truth as T  # noqa: E402
from monolith_amd import layer_ops  # noqa: E402
from monolith_amd.feature_cross import CIN  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("xnext", "pooled", "dx0", "dxl", "dw", "dbias")
USED = dict.fromkeys(NAMES, 0.0)


def plan_shapes():
  """The shapes that depend on the plan, each asserted to reach what it names."""
  out = []
  kc = layer_ops.cin_plan(3, 1, 4, 16, 5)["k_chunk"]   # m = 1: K = H
  for H in (kc - 1, kc, kc + 1):
    assert layer_ops.cin_plan(3, 1, 4, H, 5)["k_chunk"] == kc
    out.append((3, 1, 4, H, 5))
  rows = layer_ops.cin_plan(1, 2, 1, 2, 3)["slab_rows"]
  p = layer_ops.cin_plan(rows + 1, 2, 1, 2, 3)
  assert p["slab_rows"] == rows and p["slabs"] == 2 and p["workspace_bytes"] == 2 * 5 * 3 * 4
  out.append((rows + 1, 2, 1, 2, 3))
  span = 32 * layer_ops.cin_plan(2, 2, 3, 2, 512)["column_tiles"]
  assert layer_ops.cin_plan(2, 2, 3, 2, span + 3)["column_tiles"] * 32 == span
  out.append((2, 2, 3, 2, span + 3))
  return out


SHAPES = [(1, 1, 1, 1, 1), (5, 3, 1, 3, 1), (5, 2, 3, 2, 31), (5, 2, 3, 2, 33), (3, 5, 10, 5, 7), (2, 4, 16, 4, 32),
          (3, 4, 32, 6, 8), (2, 3, 33, 3, 5), (9, 7, 12, 9, 40),
          (2, 35, 3, 2, 5),     # m > 32: an h cut into two chunks, the kernels' wide-m instances
          (4, 5, 8, 30, 40)] + plan_shapes()   # H m + 1 = 151: two blocks of K rows in the weight gradient


def inputs(seed, shape):
  B, m, D, H, U = shape
  rng = np.random.default_rng(seed)
  u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)   # noqa: E731
  return dict(x0=u(B, m, D), xl=u(B, H, D), w=u(H * m, U), bias=u(U), dxnext=u(B, U, D), dpooled=u(B, U))


def dev(a, offset=0):
  """On the GPU; with ``offset`` a view one float into its storage (4-byte aligned only)."""
  if a is None:
    return None
  if not offset:
    return torch.from_numpy(a).cuda()
  store = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
  store[offset:offset + a.size] = torch.from_numpy(a).cuda().ravel()
  v = store[offset:offset + a.size].view(a.shape)
  assert v.data_ptr() % 16 == 4 * offset
  return v


def run_layer(inp, act, offset=0):
  """-> {name: numpy} of the forward and the full gradient call, after the bit checks of repeats and single asks."""
  t = {k: dev(v, offset) for k, v in inp.items()}
  with torch.no_grad():
    xnext, pooled = layer_ops.cin_layer(t["x0"], t["xl"], t["w"], t["bias"], act)
    again = layer_ops.cin_layer(t["x0"], t["xl"], t["w"], t["bias"], act)
    last = layer_ops.cin_layer(t["x0"], t["xl"], t["w"], t["bias"], act, want_next=False)
  assert torch.equal(again[0], xnext) and torch.equal(again[1], pooled) and last[0] is None
  assert torch.equal(last[1], pooled)
  args = (t["dxnext"], t["dpooled"], t["x0"], t["xl"], t["w"], xnext, act)
  grads = layer_ops.cin_layer_grad(*args)
  for a, b in zip(grads, layer_ops.cin_layer_grad(*args)):
    assert torch.equal(a, b)
  for i in range(4):   # asked for alone
    alone = layer_ops.cin_layer_grad(*args, *[j == i for j in range(4)])
    assert torch.equal(alone[i], grads[i]) and all(alone[j] is None for j in range(4) if j != i)
  return dict(zip(NAMES, [x.cpu().numpy() for x in (xnext, pooled) + tuple(grads)]))


def within(got, truth, what):
  for name, g in got.items():
    want, bound = truth[name]
    err = np.abs(g.astype(np.float64) - want)
    share = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0
    USED[name] = max(USED[name], share)
    print("%s %s: share of the bound %.3f (largest so far %.3f)" % (what, name, share, USED[name]))
    assert (err <= bound).all(), "%s %s: %.3g of its bound" % (what, name, share)
    assert not (np.signbit(g) & (g == 0)).any(), "%s %s holds -0" % (what, name)


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_and_gradients_within_bounds(shape, act):
  inp = inputs(sum(shape), shape)
  truth = T.layer_truth(inp["x0"], inp["xl"], inp["w"], inp["bias"], act == "relu", inp["dxnext"], inp["dpooled"])
  within(run_layer(inp, act), truth, "%s %s" % (shape, act))


@pytest.mark.parametrize("shape", [(3, 5, 10, 5, 7), (9, 7, 12, 9, 40)], ids=lambda s: "x".join(map(str, s)))
def test_operands_4_byte_aligned_only(shape):
  inp = inputs(sum(shape), shape)
  aligned, shifted = run_layer(inp, "relu"), run_layer(inp, "relu", offset=1)
  for name in NAMES:
    assert np.array_equal(aligned[name].view(np.uint32), shifted[name].view(np.uint32)), name


def test_module_through_autograd():
  rng = np.random.default_rng(7)
  x = rng.uniform(-1, 1, (7, 3, 10)).astype(np.float32)
  up = rng.uniform(-1, 1, (7, 5 + 33 + 4)).astype(np.float32)
  torch.manual_seed(7)
  layer = CIN([5, 33, 4], "relu")
  xt = torch.from_numpy(x).cuda().requires_grad_()
  before = layer_ops.cin_launch_counts()
  result = layer(xt)
  after = layer_ops.cin_launch_counts()
  assert (after["forward"] - before["forward"], after["forward_last"] - before["forward_last"]) == (2, 1)
  with torch.no_grad():   # biases start at zero: move them, so that their part of every sum is checked
    for i in range(3):
      getattr(layer, "bias_%d" % i).copy_(torch.from_numpy(rng.uniform(-1, 1, layer.hidden_uints[i]).astype(np.float32)))
  result = layer(xt)
  result.backward(torch.from_numpy(up).cuda())
  params = dict(layer.named_parameters())
  assert [tuple(params["kernel_%d" % i].shape) for i in range(3)] == [(9, 5), (15, 33), (99, 4)]
  truth = T.chain_truth(x, [params["kernel_%d" % i].detach().cpu().numpy() for i in range(3)],
                        [params["bias_%d" % i].detach().cpu().numpy() for i in range(3)], True, up)
  got = {"result": result.detach().cpu().numpy(), "dx": xt.grad.cpu().numpy()}
  got.update({"d" + k: v.grad.cpu().numpy() for k, v in params.items()})
  assert set(got) == set(truth)
  for name, g in got.items():
    want, bound = truth[name]
    err = np.abs(g.astype(np.float64) - want)
    print("module %s: share of the bound %.3f" % (name, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert (err <= bound).all(), name


def test_forward_and_backward_in_one_graph():
  shape = (40, 3, 4, 5, 6)   # B D = 160 rows: more than one slab
  p = layer_ops.cin_plan(*shape)
  assert p["slabs"] > 1
  a, b = inputs(1, shape), inputs(2, shape)
  eager = run_layer(b, "relu")
  t = {k: dev(v) for k, v in a.items()}
  outs = {}

  def step():
    outs["xnext"], outs["pooled"] = layer_ops.cin_layer(t["x0"], t["xl"], t["w"], t["bias"], "relu")
    grads = layer_ops.cin_layer_grad(t["dxnext"], t["dpooled"], t["x0"], t["xl"], t["w"], outs["xnext"], "relu")
    outs.update(zip(NAMES[2:], grads))

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s), torch.no_grad():
    step()   # the workspace grows outside the capture
    torch.cuda.synchronize()
    before = layer_ops.cin_launch_counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
      step()
    after = layer_ops.cin_launch_counts()
  assert {k: after[k] - before[k] for k in after} == dict(forward=1, forward_last=0, input_grad=1, weight_grad=1,
                                                          slab_sum=1)
  for k, v in b.items():
    t[k].copy_(torch.from_numpy(v).cuda())
  for _ in range(3):   # several replays, each against the eager result
    graph.replay()
    torch.cuda.synchronize()
    for name in NAMES:
      assert np.array_equal(outs[name].cpu().numpy().view(np.uint32), eager[name].view(np.uint32)), name
