"""GPU suite of the DCN cross layer (csrc/mhte_dcn_kernels.h, mhte_dcn_host.h, monolith_amd/layer_ops.py,
feature_cross.DCN) against the float64 truth of tests/dcn_truth.py within its derived bounds.  Every layer case
checks besides: a second call repeats the first one's bits, a gradient asked for alone has the bits it has in the
full call, a first layer's dx0 is dx0 + dxl of the plain call, every zero is +0.

Measured on an MI355X (the largest share of its bound any layer case of this file used): xnext 0.21, aux 0.16,
dx0 0.11 (0.15 without dx0_acc, 0.04 for a first layer against dx0 + dxl), dxl 0.10, dw 0.06, dbias 0.06; the
module's result stays below 0.04 and its gradients below 0.02 of their chained bounds.  Every case prints its
shares."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dcn_truth as T  # noqa: E402
from monolith_amd import layer_ops  # noqa: E402
from monolith_amd.feature_cross import DCN  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("xnext", "aux", "dx0", "dxl", "dw", "dbias")
USED = {}


def plan_shapes(typ):
  """The shapes that depend on the plan, each asserted to reach what it names."""
  plan = lambda B, d: layer_ops.dcn_plan(B, d, typ)   # noqa: E731
  kc = plan(3, 5)["k_chunk"]
  out = [(3, kc - 1), (3, kc), (3, kc + 1)]
  assert all(plan(*s)["k_chunk"] == kc for s in out)
  span = plan(2, 100)["column_span"]
  # matrix: a second workgroup column; vector: the next register form of the kernel
  assert plan(2, span + 3)["column_span"] == (span if typ == "matrix" else 4 * span)
  out.append((2, span + 3))
  rows = plan(1, 8)["slab_rows"]
  p = plan(rows + 1, 8)
  assert p["slab_rows"] == rows and p["slabs"] == 2
  assert p["workspace_bytes"] == (2 * 9 * 8 * 4 if typ == "matrix" else 2 * 2 * 8 * 4)
  out.append((rows + 1, 8))
  return out


SHAPES = [(1, 1), (5, 31), (5, 32), (5, 33), (3, 65), (127, 8), (129, 8)]
CASES = [(t, s) for t in layer_ops.DCN_TYPES for s in SHAPES + plan_shapes(t)]


def inputs(seed, typ, shape):
  B, d = shape
  rng = np.random.default_rng(seed)
  u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)   # noqa: E731
  return dict(x0=u(B, d), xl=u(B, d), w=u(d, d if typ == "matrix" else 1), bias=u(1, d), g=u(B, d), acc=u(B, d))


def dev(a, offset=0):
  """On the GPU; with ``offset`` a view one float into its storage (4-byte aligned only)."""
  if not offset:
    return torch.from_numpy(a).cuda()
  store = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
  store[offset:offset + a.size] = torch.from_numpy(a).cuda().ravel()
  v = store[offset:offset + a.size].view(a.shape)
  assert v.data_ptr() % 16 == 4 * offset
  return v


def run_layer(inp, typ, offset=0):
  """-> {name: numpy} of the forward and the full gradient call (plus dx0_alone, dx0_first), after the bit checks."""
  t = {k: dev(v, offset) for k, v in inp.items()}
  acc = lambda: dev(inp["acc"], offset)   # noqa: E731 (the call adds into it)
  xnext, aux = layer_ops.dcn_layer(t["x0"], t["xl"], t["w"], t["bias"], typ)
  again = layer_ops.dcn_layer(t["x0"], t["xl"], t["w"], t["bias"], typ)
  bare = layer_ops.dcn_layer(t["x0"], t["xl"], t["w"], t["bias"], typ, want_aux=False)
  assert torch.equal(again[0], xnext) and torch.equal(again[1], aux)
  assert torch.equal(bare[0], xnext) and bare[1] is None
  args = (t["g"], t["x0"], t["xl"], t["w"], aux, typ)
  grads = layer_ops.dcn_layer_grad(*args, False, acc())
  for a, b in zip(grads, layer_ops.dcn_layer_grad(*args, False, acc())):
    assert torch.equal(a, b)
  for i in range(4):   # asked for alone
    alone = layer_ops.dcn_layer_grad(*args, False, acc(), *[j == i for j in range(4)])
    assert torch.equal(alone[i], grads[i]) and all(alone[j] is None for j in range(4) if j != i)
  first = layer_ops.dcn_layer_grad(*args, True, acc())
  assert first[1] is None and torch.equal(first[2], grads[2]) and torch.equal(first[3], grads[3])
  out = dict(zip(NAMES, [x.cpu().numpy() for x in (xnext, aux) + tuple(grads)]))
  out["dx0_alone"] = layer_ops.dcn_layer_grad(*args, False, None, True, False, False, False)[0].cpu().numpy()
  out["dx0_first"] = first[0].cpu().numpy()
  return out


def within(got, truth, what):
  for name, g in got.items():
    want, bound = truth[name]
    err = np.abs(g.astype(np.float64) - want.reshape(g.shape))
    share = float(np.max(err / np.maximum(bound.reshape(g.shape), 1e-300)))
    USED[name] = max(USED.get(name, 0.0), share)
    print("%s %s: share of the bound %.3f (largest so far %.3f)" % (what, name, share, USED[name]))
    assert (err <= bound.reshape(g.shape)).all(), "%s %s: %.3g of its bound" % (what, name, share)
    assert not (np.signbit(g) & (g == 0)).any(), "%s %s holds -0" % (what, name)


@pytest.mark.parametrize("typ,shape", CASES, ids=["%s-%dx%d" % ((t,) + s) for t, s in CASES])
def test_layer_and_gradients_within_bounds(typ, shape):
  inp = inputs(sum(shape), typ, shape)
  truth = T.layer_truth(typ == "matrix", inp["x0"], inp["xl"], inp["w"], inp["bias"], inp["g"], inp["acc"])
  got = run_layer(inp, typ)
  # a first layer: dx0 + dxl of the plain call, within the two bounds
  truth["dx0_first"] = (got["dx0"].astype(np.float64) + got["dxl"], truth["dx0"][1] + truth["dxl"][1])
  within(got, truth, "%s %s" % (typ, shape))


@pytest.mark.parametrize("typ", layer_ops.DCN_TYPES)
def test_operands_4_byte_aligned_only(typ):
  inp = inputs(3, typ, (9, 67))
  aligned, shifted = run_layer(inp, typ), run_layer(inp, typ, offset=1)
  for name in aligned:
    assert np.array_equal(aligned[name].view(np.uint32), shifted[name].view(np.uint32)), name


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("typ", layer_ops.DCN_TYPES)
def test_module_through_autograd(typ, layers):
  rng = np.random.default_rng(7)
  x, up = (rng.uniform(-1, 1, (9, 40)).astype(np.float32) for _ in range(2))
  torch.manual_seed(7)
  layer = DCN(layers, typ)
  xt = torch.from_numpy(x).cuda().requires_grad_()
  fwd, fwd_bare = typ + "_forward", typ + "_forward_no_aux"
  dxk = "matrix_input_grad" if typ == "matrix" else "vector_grad"
  c0 = layer_ops.dcn_launch_counts()
  with torch.no_grad():   # (builds the parameters) writes no aux
    bare = layer(xt)
  c1 = layer_ops.dcn_launch_counts()
  assert (c1[fwd] - c0[fwd], c1[fwd_bare] - c0[fwd_bare]) == (0, layers)
  with torch.no_grad():   # biases start at zero: move them, so that their part of every sum is checked
    for i in range(layers):
      getattr(layer, "bias_%d" % i).copy_(torch.from_numpy(rng.uniform(-1, 1, (1, 40)).astype(np.float32)))
  result = layer(xt)
  result.backward(torch.from_numpy(up).cuda())
  c2 = layer_ops.dcn_launch_counts()
  assert (c2[fwd] - c1[fwd], c2[fwd_bare] - c1[fwd_bare], c2[dxk] - c1[dxk]) == (layers, 0, layers)
  assert bare.shape == result.shape == (9, 40)
  params = dict(layer.named_parameters())
  assert tuple(params["kernel_0"].shape) == ((40, 40) if typ == "matrix" else (40, 1))
  assert tuple(params["bias_0"].shape) == (1, 40)
  truth = T.chain_truth(typ == "matrix", x, [params["kernel_%d" % i].detach().cpu().numpy() for i in range(layers)],
                        [params["bias_%d" % i].detach().cpu().numpy() for i in range(layers)], up)
  got = {"result": result.detach().cpu().numpy(), "dx": xt.grad.cpu().numpy()}
  got.update({"d" + k: v.grad.cpu().numpy() for k, v in params.items()})
  assert set(got) == set(truth)
  within(got, truth, "module %s x%d" % (typ, layers))
