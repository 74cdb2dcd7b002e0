"""CPU suite of the DCN cross layer: the plan (a function of the shape alone, no device) and every refusal of the
entry points, which are checked on the host before any device call."""
import ctypes as C

import pytest
import torch

from monolith_amd import _lib, layer_ops
from monolith_amd.feature_cross import DCN

ceil = lambda a, b: -(-a // b)   # noqa: E731


@pytest.mark.parametrize("typ", layer_ops.DCN_TYPES)
@pytest.mark.parametrize("shape", [(65536, 1024), (65536, 512), (33, 8), (1, 1), (0, 4096), (524288, 4096), (7, 65)])
def test_plan_is_a_function_of_the_shape(shape, typ):
  B, d = shape
  p = layer_ops.dcn_plan(B, d, typ)
  assert p == layer_ops.dcn_plan(B, d, typ)
  if typ == "matrix":
    span = 32 if d <= 32 else 64 if d <= 64 else 128
    assert (p["row_block"], p["column_span"], p["k_chunk"]) == (128, span, 32)
    wanted = min(64, max(1, ceil(2048, ceil(d + 1, 128) * ceil(d, span))))
    rows = max(32, ceil(ceil(B, wanted), 32) * 32)
    per_slab = (d + 1) * d * 4
  else:
    vpl = 1 if d <= 64 else 4 if d <= 256 else 16 if d <= 1024 else 64
    assert (p["row_block"], p["column_span"], p["k_chunk"]) == (64, 64 * vpl, 64)
    rows = max(64, ceil(ceil(B, 512), 64) * 64)
    per_slab = 2 * d * 4
  assert p["slab_rows"] == rows and p["slabs"] == max(1, ceil(B, rows)) and p["slabs"] * p["slab_rows"] >= B
  assert p["workspace_bytes"] == (p["slabs"] * per_slab if p["slabs"] > 1 else 0)


def call(fn, **over):
  a = dict(B=4, d=5, type=1, first=0)
  a.update(over)
  one = C.c_void_p(16)   # never dereferenced: every refusal comes before the first device call
  p = lambda k: a.get(k, one)   # noqa: E731
  L = _lib.lib()
  if fn == "dcn_layer":
    return L.mhte_dcn_layer(p("x0"), one, one, p("bias"), a["B"], a["d"], a["type"], one, None, None)
  return L.mhte_dcn_layer_grad(one, p("x0"), one, one, p("aux"), a["B"], a["d"], a["type"], a["first"], None,
                               p("dx0"), p("dxl"), p("dw"), p("dbias"), None)


REFUSALS = [(dict(d=0), "d must be in"), (dict(d=4097), "d must be in"), (dict(B=-1), "B must be >= 0"),
            (dict(B=2 ** 31 // 5 + 1), "B \\* d must be at most 2\\^31"), (dict(type=2), "type must be 0"),
            (dict(x0=None), "null argument: x0"), (dict(x0=C.c_void_p(18)), "x0 must be 4-byte aligned")]


@pytest.mark.parametrize("fn", ["dcn_layer", "dcn_layer_grad"])
@pytest.mark.parametrize("over,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_entry_points_refuse_on_the_host(fn, over, message):
  with pytest.raises(_lib.InvalidArgumentError, match="%s: %s" % (fn, message)):
    _lib.check(call(fn, **over))


def test_gradient_plan_and_module_refusals():
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_layer: null argument: bias"):
    _lib.check(call("dcn_layer", bias=None))
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_layer_grad: null argument: dx0, dxl, dw and dbias"):
    _lib.check(call("dcn_layer_grad", dx0=None, dxl=None, dw=None, dbias=None))
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_layer_grad: null argument: aux"):
    _lib.check(call("dcn_layer_grad", aux=None))
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_layer_grad: null argument: dx0 \\(a first"):
    _lib.check(call("dcn_layer_grad", first=1, dx0=None))
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_plan: d must be in"):
    layer_ops.dcn_plan(1, 4097)
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_plan: n must be 6"):
    _lib.check(_lib.lib().mhte_dcn_plan(1, 1, 1, (C.c_int64 * 5)(), 5))
  with pytest.raises(_lib.InvalidArgumentError, match="dcn_launch_counts: n must be 9"):
    _lib.check(_lib.lib().mhte_dcn_launch_counts((C.c_int64 * 4)(), 4))
  x, w, b = torch.zeros(2, 3), torch.zeros(3, 3), torch.zeros(1, 3)
  with pytest.raises(NotImplementedError, match="dcn_layer: dcn_type must be 'vector' or 'matrix', got 'mixed'"):
    layer_ops.dcn_layer(x, x, w, b, "mixed")
  with pytest.raises(ValueError, match=r"dcn_layer: weight must have the shape \(3, 1\), got \(3, 3\)"):
    layer_ops.dcn_layer(x, x, w, b, "vector")
  with pytest.raises(ValueError, match="dcn_layer: x0 is not 2D"):
    layer_ops.dcn_layer(x[0], x, w, b)
  with pytest.raises(TypeError, match="dcn_layer: x0 must be float32"):
    layer_ops.dcn_layer(x.double(), x, w, b)
  with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
    layer_ops.dcn_cross(x, [w], [b])
  with pytest.raises(ValueError, match="dcn_cross: as many kernels as biases"):
    layer_ops.dcn_cross(x, [w], [])
  with pytest.raises(ValueError, match="dcn_layer_grad: at least one of want_x0"):
    layer_ops.dcn_layer_grad(x, x, x, w, x, "matrix", False, None, False, False, False, False)
  with pytest.raises(ValueError, match="dcn_layer_grad: dx0 needs aux"):
    layer_ops.dcn_layer_grad(x, x, x, w, None)
  for kw, name in ((dict(dcn_type="mixed"), "dcn_type"), (dict(allow_kernel_norm=True), "allow_kernel_norm"),
                   (dict(use_dropout=True), "use_dropout"), (dict(initializer="zeros"), "initializer")):
    with pytest.raises(NotImplementedError, match="DCN: " + name):
      DCN(**kw)
  assert DCN(2, "vector").get_config() == {
      "layer_num": 2, "dcn_type": "vector", "initializer": None, "regularizer": None, "num_experts": 1, "low_rank": 0,
      "allow_kernel_norm": False, "use_dropout": False, "keep_prob": 0.95, "mode": "train"}
