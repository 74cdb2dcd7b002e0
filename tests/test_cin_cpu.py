"""CPU suite of the CIN layer: the plan (a function of the shape alone, no device) and every refusal of the entry
points, which are checked on the host before any device call."""
import ctypes as C

import pytest
import torch

from monolith_amd import _lib, layer_ops
from monolith_amd.feature_cross import CIN

SHAPE = dict(B=4, m=3, D=5, H=3, U=7)


@pytest.mark.parametrize("shape", [(65536, 26, 16, 128, 128), (65536, 39, 10, 200, 200), (33, 2, 1, 2, 3),
                                   (1, 1, 1, 1, 1), (0, 64, 128, 512, 512), (7, 33, 10, 5, 33)])
def test_plan_is_a_function_of_the_shape(shape):
  B, m, D, H, U = shape
  p = layer_ops.cin_plan(*shape)
  assert p == layer_ops.cin_plan(*shape)
  assert p["row_block"] == 128 and p["column_tiles"] == (1 if U <= 32 else 2 if U <= 64 else 4)
  mp2 = (m + 1) // 2
  assert p["k_chunk"] == ((16 // mp2) * m if mp2 <= 16 else 32)
  ceil = lambda a, b: -(-a // b)   # noqa: E731
  tiles = ceil(H * m + 1, 128) * ceil(U, 32 * p["column_tiles"])
  wanted = min(64, max(1, ceil(2048, tiles)))
  rows = max(32, ceil(ceil(B * D, wanted), 32) * 32)
  assert p["slab_rows"] == rows and p["slabs"] == max(1, ceil(B * D, rows))
  assert p["workspace_bytes"] == (p["slabs"] * (H * m + 1) * U * 4 if p["slabs"] > 1 else 0)


def call(fn, **over):
  a = dict(SHAPE, activation=0)
  a.update(over)
  one = C.c_void_p(16)   # never dereferenced: every refusal comes before the first device call
  L = _lib.lib()
  if fn == "cin_layer":
    return L.mhte_cin_layer(one, one, one, one, a["B"], a["m"], a["D"], a["H"], a["U"], a["activation"], None, one,
                            None)
  outs = [a.get(k, one) for k in ("dx0", "dxl", "dw", "dbias")]
  return L.mhte_cin_layer_grad(None, one, one, one, one, a.get("xnext"), a["B"], a["m"], a["D"], a["H"], a["U"],
                               a["activation"], *outs, None)


REFUSALS = [(dict(m=0), "m must be in"), (dict(D=0), "D must be in"), (dict(H=0), "H must be in"),
            (dict(U=0), "U must be in"), (dict(m=65), "m must be in"), (dict(D=129), "D must be in"),
            (dict(H=513), "H must be in"), (dict(U=513), "U must be in"), (dict(B=-1), "B must be >= 0"),
            (dict(B=2 ** 30 // 5 + 1), "B \\* D must be at most 2\\^30"), (dict(activation=2), "activation must be 0")]


@pytest.mark.parametrize("fn", ["cin_layer", "cin_layer_grad"])
@pytest.mark.parametrize("over,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_entry_points_refuse_on_the_host(fn, over, message):
  with pytest.raises(_lib.InvalidArgumentError, match="%s: %s" % (fn, message)):
    _lib.check(call(fn, **over))


def test_gradient_plan_and_module_refusals():
  with pytest.raises(_lib.InvalidArgumentError, match="cin_layer_grad: null argument: dx0, dxl, dw and dbias"):
    _lib.check(call("cin_layer_grad", dx0=None, dxl=None, dw=None, dbias=None))
  with pytest.raises(_lib.InvalidArgumentError, match="cin_layer_grad: null argument: xnext"):
    _lib.check(call("cin_layer_grad", activation=1))
  with pytest.raises(_lib.InvalidArgumentError, match="cin_plan: m must be in"):
    layer_ops.cin_plan(1, 65, 1, 1, 1)
  with pytest.raises(_lib.InvalidArgumentError, match="cin_plan: n must be 6"):
    _lib.check(_lib.lib().mhte_cin_plan(1, 1, 1, 1, 1, (C.c_int64 * 5)(), 5))
  with pytest.raises(_lib.InvalidArgumentError, match="cin_launch_counts: n must be 5"):
    _lib.check(_lib.lib().mhte_cin_launch_counts((C.c_int64 * 4)(), 4))
  x = torch.zeros(2, 3, 4)
  with pytest.raises(NotImplementedError, match="activation must be None or 'relu', got 'tanh'"):
    CIN([3], "tanh")
  with pytest.raises(NotImplementedError, match="cin_layer: activation must be None or 'relu'"):
    layer_ops.cin_layer(x, x, torch.zeros(9, 2), torch.zeros(2), "tanh")
  with pytest.raises(ValueError, match=r"cin_layer: weight must have the shape \(9, 2\), got \(8, 2\)"):
    layer_ops.cin_layer(x, x, torch.zeros(8, 2), torch.zeros(2))
  with pytest.raises(TypeError, match="cin_layer: x0 must be float32"):
    layer_ops.cin_layer(x.double(), x.double(), torch.zeros(9, 2), torch.zeros(2))
  with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
    layer_ops.cin_layer(x, x, torch.zeros(9, 2), torch.zeros(2))
  with pytest.raises(ValueError, match="cin_layer_grad: at least one of want_x0"):
    layer_ops.cin_layer_grad(None, torch.zeros(2, 2), x, x, torch.zeros(9, 2), None, None, False, False, False, False)
  assert CIN([5, 4], "relu").get_config() == {"hidden_uints": [5, 4], "activation": "relu",
                                              "initializer": "glorot_uniform", "regularizer": None}
