"""CPU suite of AutoInt: the truth of the GPU suite against a plain loop, the plan (a function of the shape alone, no
device) and every refusal, each raised by name before any device call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import autoint_truth as T  # noqa: E402
from monolith_amd import _lib, layer_ops  # noqa: E402
from monolith_amd.feature_trans import AutoInt  # noqa: E402


def loop(x, L):
  n, k = len(x), len(x[0])
  for _ in range(L):
    new = []
    for i in range(n):
      s = [sum(x[i][c] * x[j][c] for c in range(k)) for j in range(n)]
      e = [float(np.exp(v - max(s))) for v in s]
      new.append([sum(e[j] / sum(e) * x[j][c] for j in range(n)) for c in range(k)])
    x = new
  return x


@pytest.mark.parametrize("shape", [(2, 3, 2, 1), (1, 4, 3, 3)])
def test_truth_against_a_plain_loop(shape):
  B, n, k, L = shape
  x, dout = np.random.default_rng(5).uniform(-1, 1, (2, B, n, k)).astype(np.float32)
  got = T.truth(x, dout, L)
  want = np.array([loop(x[b].astype(np.float64).tolist(), L) for b in range(B)])
  np.testing.assert_allclose(got["out"][0], want, rtol=0, atol=1e-14)
  assert all(0 < bound < 1e-4 for _, bound in got.values())


@pytest.mark.parametrize("shape", [(65536, 39, 16, 3), (1, 1, 1, 1), (0, 16, 17, 8), (7, 17, 33, 2), (5, 128, 64, 8),
                                   (3, 65, 5, 1)])
def test_plan_is_a_function_of_the_shape(shape):
  B, n, k, L = shape
  p = layer_ops.autoint_plan(*shape)
  tile = 16 if n <= 16 else 32
  rows, pk = -(-n // tile) * tile, -(-k // tile) * tile
  assert p == layer_ops.autoint_plan(*shape) == layer_ops.autoint_plan(B + 9, n, k, 1 + L % 8)
  assert (p["tile"], p["row_tiles"], p["padded_k"]) == (tile, rows // tile, pk) and p["row_tiles"] <= 4
  assert p["samples_per_workgroup"] == 1 and p["workspace_bytes"] == 0
  assert p["lds_bytes_forward"] == 4 * 2 * rows * (pk + 1) <= 163840
  assert p["lds_bytes_grad"] == 4 * (3 * rows * (pk + 1) + 3 * rows) <= 163840


def abi(fn, **over):
  a = {**dict(B=4, n=5, k=3, L=2), **over}
  one = C.c_void_p(16)   # never dereferenced: every refusal comes before the first device call
  p = lambda name: a.get(name, one)   # noqa: E731
  lib, dims = _lib.lib(), (a["B"], a["n"], a["k"], a["L"])
  if fn == "autoint_forward":
    return lib.mhte_autoint_forward(p("x"), *dims, p("out"), p("states"), None)
  return lib.mhte_autoint_grad(one, p("x"), p("states"), p("out"), *dims, one, None)


REFUSALS = [(dict(n=0), "n must be in \\[1, 128\\]"), (dict(n=129), "n must be in \\[1, 128\\]"),
            (dict(k=65), "k must be in \\[1, 64\\]"), (dict(L=9), "layer_num must be in \\[1, 8\\]"),
            (dict(B=-1), "B must be >= 0"), (dict(B=2 ** 31), "B must be below 2\\^31"), (dict(x=None), "null argument: x"),
            (dict(out=None), "null argument: out"), (dict(x=C.c_void_p(18)), "x must be 4-byte aligned"),
            (dict(states=C.c_void_p(18)), "states must be 4-byte aligned")]


@pytest.mark.parametrize("fn", ["autoint_forward", "autoint_grad"])
@pytest.mark.parametrize("over,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_entry_points_refuse_on_the_host(fn, over, message):
  with pytest.raises(_lib.InvalidArgumentError, match="%s: %s" % (fn, message)):
    _lib.check(abi(fn, **over))


def test_python_and_module_refusals():
  x, lib, bad, buf = torch.zeros(2, 5, 3), _lib.lib(), _lib.InvalidArgumentError, (C.c_int64 * 5)()
  checks = [(bad, "autoint_grad: null argument: states", lambda: _lib.check(abi("autoint_grad", states=None))),
            (bad, "autoint_grad: states must be NULL when layer_num", lambda: _lib.check(abi("autoint_grad", L=1))),
            (bad, "autoint_plan: k must be in", lambda: layer_ops.autoint_plan(1, 1, 65, 2)),
            (bad, "autoint_plan: n_out must be 7", lambda: _lib.check(lib.mhte_autoint_plan(1, 1, 1, 1, buf, 5))),
            (bad, "autoint_launch_counts: n_out must be 2", lambda: _lib.check(lib.mhte_autoint_launch_counts(buf, 5))),
            (ValueError, "autoint_grad: states must be None exactly when layer_num == 1",
             lambda: layer_ops.autoint_grad(x, x, None, x, 2)),
            (ValueError, "autoint_grad: states must have the shape \\(1, 2, 5, 3\\)",
             lambda: layer_ops.autoint_grad(x, x, x, x, 2)),
            (ValueError, "AutoInt: layer_num must be an int in \\[1, 8\\], got 0", lambda: AutoInt(layer_num=0)),
            (ValueError, "AutoInt: out_type must be 'concat', 'stack' or None", lambda: AutoInt(out_type="sum")),
            (ValueError, "AutoInt: the input must be a \\[B, num_feat, emb\\] tensor", lambda: AutoInt()(x[0]))]
  for what, fn in (("autoint_forward", lambda t, L=2: layer_ops.autoint(t, L)),
                   ("autoint_grad", lambda t, L=2: layer_ops.autoint_grad(x, t, x[None], x, L))):
    checks += [(ValueError, what + ": layer_num must be an int in \\[1, 8\\], got 9", lambda fn=fn: fn(x, 9)),
               (TypeError, what + ": x must be a torch tensor, got list", lambda fn=fn: fn([1.0])),
               (ValueError, what + ": x is not 3D", lambda fn=fn: fn(x[0])),
               (ValueError, what + ": n must be in \\[1, 128\\], got 129", lambda fn=fn: fn(torch.zeros(1, 129, 3))),
               (ValueError, what + ": k must be in \\[1, 64\\], got 65", lambda fn=fn: fn(torch.zeros(1, 5, 65))),
               (TypeError, what + ": x must be float32", lambda fn=fn: fn(x.double())),
               (TypeError, what + ": .* must be on the GPU", lambda fn=fn: fn(x))]   # last: there is no CPU path
  for error, message, call in checks:
    with pytest.raises(error, match=message):
      call()
  assert AutoInt().get_config() == {"layer_num": 1, "out_type": "concat", "keep_list": False}
