"""GPU suite of the CAN co-action unit (csrc/mhte_can_kernels.h, mhte_can_host.h, monolith_amd/layer_ops.py,
feature_cross.CAN) against the float64 truth of tests/can_truth.py within its derived bounds.  Every case checks
besides: a second call repeats the first one's bits, a gradient asked for alone has the bits it has in the full call,
every zero is +0.

Measured on an MI355X (the largest share of its bound any case of this file used): out 0.083, duser 0.074, ditem 0.095; the
module's out 0.021, duser 0.028, ditem 0.007.  Every case prints its shares."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import can_truth as T  # noqa: E402
from monolith_amd import layer_ops  # noqa: E402
from monolith_amd.feature_cross import CAN  # noqa: E402

pytestmark = pytest.mark.gpu

USED = {}
SEQ_STACKED, STACKED, SEQ, PLAIN = (True, True), (False, True), (True, False), (False, False)   # (is_seq, is_stacked)
FORM = {SEQ_STACKED: "seq_stacked", STACKED: "stacked", SEQ: "seq", PLAIN: "plain"}


def plan_cases():
  """The shapes that depend on the plan, each asserted to reach what it names: (B, F, T, d, L, form)."""
  out = []
  for d in (4, 17):   # one tile size each
    rows = layer_ops.can_plan(1, 1, 1, d, 2)["rows_per_tile"]
    for R, tiles in ((rows - 1, 1), (rows, 1), (rows + 1, 2)):
      assert layer_ops.can_plan(2, 1, R, d, 2)["tiles_per_sample"] == tiles
      out.append((2, 1, R, d, 2, SEQ))
    # a feature whose rows lie on both sides of a tile boundary: here the feature of row rows - 1
    F, Ts = 3, rows // 2 - 1
    assert (rows - 1) // Ts == rows // Ts < F and rows % Ts and layer_ops.can_plan(2, F, Ts, d, 2)["tiles_per_sample"] == 2
    out.append((2, F, Ts, d, 2, SEQ_STACKED))
  spw = layer_ops.can_plan(1, 2, 3, 4, 2)["samples_per_workgroup"]
  out.append((spw + 1, 2, 3, 4, 2, SEQ_STACKED))
  return out


CASES = ([(1, 1, 1, 1, 1, SEQ_STACKED), (3, 10, 12, 10, 2, SEQ_STACKED), (3, 10, 1, 10, 2, STACKED),
          (2, 1, 1, 10, 2, PLAIN), (1, 1, 1, 5, 2, PLAIN)] +
         [(2, 3, 5, d, 2, SEQ_STACKED) for d in (3, 15, 16, 17, 32)] +
         [(2, 3, 5, 4, L, SEQ_STACKED) for L in (1, 3, 8)] + plan_cases())
assert (2, 3, 7, 4, 2, SEQ_STACKED) in CASES   # the issue's example of a straddling feature


def inputs(seed, case):
  B, F, Ts, d, L, (is_seq, is_stacked) = case
  rng = np.random.default_rng(seed)
  u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)   # noqa: E731
  shape = (B,) + ((F,) if is_stacked else ()) + ((Ts,) if is_seq else ()) + (d,)
  return dict(user=u(*shape), item=u(B, L * d * (d + 1)), dout=u(*((B, F, d) if is_stacked else (B, d))))


def dev(a, offset=0):
  """On the GPU; with ``offset`` a view one float into its storage (4-byte aligned only)."""
  if not offset:
    return torch.from_numpy(a).cuda()
  store = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
  store[offset:offset + a.size] = torch.from_numpy(a).cuda().ravel()
  v = store[offset:offset + a.size].view(a.shape)
  assert v.data_ptr() % 16 == 4 * offset
  return v


def run(inp, case, act, offset=0):
  """-> {name: numpy} of the forward and the full gradient call, after the bit checks."""
  L, form = case[4], case[5]
  t = {k: dev(v, offset) for k, v in inp.items()}
  out = layer_ops.can_forward(t["user"], t["item"], L, act, *form)
  assert torch.equal(out, layer_ops.can_forward(t["user"], t["item"], L, act, *form))
  args = (t["dout"], t["user"], t["item"], L, act) + form
  duser, ditem = layer_ops.can_grad(*args)
  for a, b in zip((duser, ditem), layer_ops.can_grad(*args)):
    assert torch.equal(a, b)
  only_user, only_item = layer_ops.can_grad(*args, want_item=False), layer_ops.can_grad(*args, want_user=False)
  assert torch.equal(only_user[0], duser) and only_user[1] is None
  assert torch.equal(only_item[1], ditem) and only_item[0] is None
  return {"out": out.cpu().numpy(), "duser": duser.cpu().numpy(), "ditem": ditem.cpu().numpy()}


def within(got, truth, what):
  for name, g in got.items():
    want, bound = truth[name]
    assert g.shape == want.shape, (what, name)
    err = np.abs(g.astype(np.float64) - want)
    share = float(np.max(err / np.maximum(bound, 1e-300)))
    USED[name] = max(USED.get(name, 0.0), share)
    print("%s %s: share of the bound %.3f (largest so far %.3f)" % (what, name, share, USED[name]))
    assert (err <= bound).all(), "%s %s: %.3g of its bound" % (what, name, share)
    assert not (np.signbit(g) & (g == 0)).any(), "%s %s holds -0" % (what, name)


@pytest.mark.parametrize("act", layer_ops.CAN_ACTIVATIONS, ids=["none", "relu"])
@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%dx%d-L%d-%s" % (c[:5] + (FORM[c[5]],)) for c in CASES])
def test_unit_and_gradients_within_bounds(case, act):
  inp = inputs(sum(case[:5]), case)
  truth = T.truth(inp["user"], inp["item"], inp["dout"], case[4], act == "relu", *case[5])
  within(run(inp, case, act), truth, "%s %s" % (case, act))


@pytest.mark.parametrize("case", [(3, 3, 7, 10, 2, SEQ_STACKED), (3, 2, 1, 20, 3, STACKED)])
def test_operands_4_byte_aligned_only(case):
  inp = inputs(3, case)
  aligned, shifted = run(inp, case, "relu"), run(inp, case, "relu", offset=1)
  for name in aligned:
    assert np.array_equal(aligned[name].view(np.uint32), shifted[name].view(np.uint32)), name


def test_module_through_autograd():
  case = (3, 10, 12, 10, 2, SEQ_STACKED)
  inp = inputs(11, case)
  layer = CAN(2, "relu", is_seq=True, is_stacked=True)
  user, item = (torch.from_numpy(inp[k]).cuda().requires_grad_() for k in ("user", "item"))
  c0 = layer_ops.can_launch_counts()
  with torch.no_grad():
    bare = layer((user, item))
  c1 = layer_ops.can_launch_counts()
  assert (c1["forward"] - c0["forward"], c1["grad"] - c0["grad"]) == (1, 0)
  out = layer((user, item))
  out.backward(torch.from_numpy(inp["dout"]).cuda())
  c2 = layer_ops.can_launch_counts()
  assert (c2["forward"] - c1["forward"], c2["grad"] - c1["grad"]) == (1, 1)
  assert torch.equal(bare, out) and not list(layer.parameters())
  got = {"out": out.detach().cpu().numpy(), "duser": user.grad.cpu().numpy(), "ditem": item.grad.cpu().numpy()}
  within(got, T.truth(inp["user"], inp["item"], inp["dout"], 2, True, True, True), "module")
