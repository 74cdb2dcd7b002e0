"""CPU suite of the CAN co-action unit: the truth of the GPU suite against a plain loop, the plan (a function of
the shape alone, no device) and every refusal, each raised by name before any device call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import can_truth as T  # noqa: E402
from monolith_amd import _lib, layer_ops  # noqa: E402
from monolith_amd.feature_cross import CAN  # noqa: E402


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("is_seq,is_stacked,shape", [(True, True, (2, 3, 4, 3)), (False, True, (2, 3, 3)),
                                                     (True, False, (2, 4, 3)), (False, False, (1, 3))])
def test_truth_against_a_plain_loop(is_seq, is_stacked, shape, relu):
  L, (B, d) = 2, (shape[0], shape[-1])
  rng = np.random.default_rng(5)
  user, item = rng.uniform(-1, 1, shape), rng.uniform(-1, 1, (B, L * d * (d + 1)))
  F, Ts = shape[1] if is_stacked else 1, shape[-2] if is_seq else 1
  rows, want = user.reshape(B, F, Ts, d), np.zeros((B, F, d))
  for b in range(B):
    for f in range(F):
      for t in range(Ts):
        h = rows[b, f, t]
        for i in range(L):
          o = i * d * (d + 1)
          pre = np.array([sum(h[k] * item[b, o + k * d + j] for k in range(d)) + item[b, o + d * d + j]
                          for j in range(d)])
          h = np.maximum(pre, 0) if relu else pre
        want[b, f] += h
  res = (B, F, d) if is_stacked else (B, d)
  got = T.truth(user, item, np.ones(res), L, relu, is_seq, is_stacked)
  assert got["out"][0].shape == res and got["duser"][0].shape == shape and got["ditem"][0].shape == item.shape
  np.testing.assert_allclose(got["out"][0], want.reshape(res), rtol=0, atol=1e-14)
  assert all((bound >= 0).all() for _, bound in got.values())


@pytest.mark.parametrize("shape", [(65536, 10, 12, 10, 2), (1, 1, 1, 1, 1), (0, 4, 50, 16, 8), (7, 3, 7, 17, 3),
                                   (5, 1, 33, 32, 8)])
def test_plan_is_a_function_of_the_shape(shape):
  B, F, Ts, d, L = shape
  p = layer_ops.can_plan(*shape)
  pd = 16 if d <= 16 else 32
  assert p == layer_ops.can_plan(*shape) and {**p, "tiles_per_sample": 0} == {**layer_ops.can_plan(B + 9, *shape[1:]),
                                                                             "tiles_per_sample": 0}
  assert (p["rows_per_tile"], p["padded_d"], p["tiles_per_sample"]) == (pd, pd, -(-F * Ts // pd))
  assert p["samples_per_workgroup"] == 1 and p["workspace_bytes"] == 0
  assert p["lds_bytes"] == 4 * (L * pd * (pd + 1) + L * pd + 2 * pd * (pd + 1)) <= 65536


def abi(fn, **over):
  a = dict(B=4, F=2, T=3, d=5, L=2, act=1)
  a.update(over)
  one = C.c_void_p(16)   # never dereferenced: every refusal comes before the first device call
  p = lambda k: a.get(k, one)   # noqa: E731
  lib, dims = _lib.lib(), (a["B"], a["F"], a["T"], a["d"], a["L"], a["act"])
  if fn == "can_forward":
    return lib.mhte_can_forward(p("user"), one, *dims, one, None)
  return lib.mhte_can_grad(one, p("user"), one, *dims, p("duser"), p("ditem"), None)


REFUSALS = [(dict(d=33), "d must be in \\[1, 32\\]"), (dict(L=9), "layer_num must be in \\[1, 8\\]"),
            (dict(F=0), "F must be >= 1"), (dict(T=0), "T must be >= 1"),
            (dict(F=2 ** 16, T=2 ** 15), "F \\* T must be at most 2\\^30"), (dict(B=-1), "B must be >= 0"),
            (dict(act=2), "activation must be 0"), (dict(user=None), "null argument: user"),
            (dict(user=C.c_void_p(18)), "user must be 4-byte aligned")]


@pytest.mark.parametrize("fn", ["can_forward", "can_grad"])
@pytest.mark.parametrize("over,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_entry_points_refuse_on_the_host(fn, over, message):
  with pytest.raises(_lib.InvalidArgumentError, match="%s: %s" % (fn, message)):
    _lib.check(abi(fn, **over))


def test_python_and_module_refusals():
  with pytest.raises(_lib.InvalidArgumentError, match="can_grad: null argument: duser and ditem"):
    _lib.check(abi("can_grad", duser=None, ditem=None))
  with pytest.raises(_lib.InvalidArgumentError, match="can_plan: d must be in"):
    layer_ops.can_plan(1, 1, 1, 33, 2)
  with pytest.raises(_lib.InvalidArgumentError, match="can_plan: n must be 6"):
    _lib.check(_lib.lib().mhte_can_plan(1, 1, 1, 1, 1, (C.c_int64 * 5)(), 5))
  with pytest.raises(_lib.InvalidArgumentError, match="can_launch_counts: n must be 2"):
    _lib.check(_lib.lib().mhte_can_launch_counts((C.c_int64 * 4)(), 4))
  user, item = torch.zeros(2, 3, 4), torch.zeros(2, 2 * 4 * 5)
  for fn, lead in ((layer_ops.can_unit, ()), (layer_ops.can_grad, (torch.zeros(2, 3, 4),))):
    what = "can_grad" if lead else "can_forward"   # (can_unit refuses through can_forward)
    with pytest.raises(ValueError, match=what + ": d must be in \\[1, 32\\], got 33"):
      fn(*lead, torch.zeros(2, 3, 33), torch.zeros(2, 2 * 33 * 34))
    with pytest.raises(ValueError, match=what + ": layer_num must be an int in \\[1, 8\\], got 9"):
      fn(*lead, user, torch.zeros(2, 9 * 4 * 5), 9)
    with pytest.raises(ValueError, match=what + ": item must be layer_num \\* d \\* \\(d \\+ 1\\) = 40 wide, got 39"):
      fn(*lead, user, item[:, :39])
    with pytest.raises(ValueError, match=what + ": user has B = 2, item B = 3"):
      fn(*lead, user, torch.zeros(3, 40))
    for act in ("tanh", "sigmoid"):
      with pytest.raises(NotImplementedError, match=what + ": activation must be None or 'relu', got '%s'" % act):
        fn(*lead, user, item, 2, act)
    with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
      fn(*lead, user, item)
  with pytest.raises(ValueError, match="can_grad: at least one of want_user"):
    layer_ops.can_grad(user, user, item, want_user=False, want_item=False)
  with pytest.raises(NotImplementedError, match="CAN: activation must be None or 'relu', got 'tanh'"):
    CAN(activation="tanh")
  with pytest.raises(ValueError, match="CAN: layer_num must be an int in"):
    CAN(layer_num=9)
  assert CAN().get_config() == {"layer_num": 2, "activation": "relu", "is_seq": False, "is_stacked": True}
