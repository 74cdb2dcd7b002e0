"""GPU test (-m gpu) of the dense tower's gradient export and parameter load (mhte_dense_mlp_backward_grads /
mhte_dense_mlp_load_params; mlp_export_grads_kernel and mlp_load_params_kernel of csrc/mhte_gemm_kernels.h).

The operands are the exact ones of tests/test_dense_mlp_exact_gpu.py (small integers, lr a power of two: every
fp32 sum of the kernels is exact, whatever its order), and its float64 reference ``RefExact`` applies SGD
exactly, so the exact gradient of a step is ``g_ref = (p_before - p_after) / lr`` in float64.  Every comparison
of T1 - T5 is on all bits, without a tolerance; T6 compares with the numpy truth of the dense optimizers on the
raw bits, as tests/test_dense_optimizers_gpu.py does for the same optimizer (``DT.assert_same_bits``)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_opt_truth as DT  # noqa: E402
import test_dense_mlp_exact_gpu as exact  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd import feature_utils as FU  # noqa: E402
from monolith_amd import optimizers as O  # noqa: E402
from monolith_amd.dense_mlp import DenseMlp  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = 0x7fc12345   # a NaN pattern planted where nothing may be written


@functools.lru_cache(maxsize=None)
def truth(name, batch=None, reseed=0):
  """One exact step of a case on the reference (second draw of w_last) -> the case and, per parameter in the
  order [W_0, b_0, ..., W_last, b_last], ``before`` (fp32), ``g_ref`` (float64) and ``after`` (float64); y, dx."""
  case = exact.make_case(name, batch=batch, reseed=reseed)
  nl = len(case["widths"]) - 2
  ref = exact.RefExact(case["widths"])
  for l in range(nl):
    ref.set_params(l, case["w"][l], case["b"][l])
  ref.set_params(nl, case["last"][1], case["b_last"])
  before = [p.clone() for l in range(nl + 1) for p in (ref.w[l], ref.b[l])]
  y = ref.forward(case["x"])
  dx = ref.backward(case["dy"], case["lr"])
  after = [p for l in range(nl + 1) for p in (ref.w[l], ref.b[l])]
  g_ref = [(b - a) / case["lr"] for b, a in zip(before, after)]
  assert all(bool((g != 0).any()) for g in g_ref)
  return {"case": case, "before": [b.to(torch.float32) for b in before], "g_ref": g_ref, "after": after, "y": y,
          "dx": dx}


def tower(t, max_batch=None):
  """A tower holding the case's integers, after the forward of its batch (y compared)."""
  mlp = DenseMlp(t["case"]["widths"], max_batch=max_batch or t["case"]["batch"])
  load(mlp, t)
  return mlp


def load(mlp, t):
  mlp.load_params(t["before"])
  exact._same(mlp.forward(t["case"]["x"]), t["y"], "y")


def params(mlp):
  return [p for l in range(mlp.n_layers) for p in mlp.get_params(l)]


def same_list(got, exp, what, as_f64=False):
  assert len(got) == len(exp)
  for i, (g, e) in enumerate(zip(got, exp)):
    name = "%s: %s of layer %d" % (what, "bias" if i % 2 else "weight", i // 2)
    exact._same(g.to(F64) if as_f64 else g, e, name)


def off4(shape):
  """An uninitialised fp32 tensor whose pointer lies 4 bytes behind a 16-byte boundary."""
  n = int(np.prod(shape))
  v = torch.empty(n + 1, dtype=torch.float32, device="cuda")[1:]
  assert v.data_ptr() % 16 == 4
  return v.view(shape)


# ---- T1. the export equals the reference gradient, and changes nothing
@pytest.mark.parametrize("name", ["one_workgroup", "tile128_deep"])
def test_export_equals_the_reference_gradient(name):
  t = truth(name)
  mlp = tower(t)
  counts = mlp.launch_counts()
  dx, grads = mlp.backward_grads(t["case"]["dy"])
  exact._same(dx, t["dx"], "dx")
  assert [tuple(g.shape) for g in grads] == mlp.param_shapes()
  same_list(grads, t["g_ref"], "exported", as_f64=True)
  same_list(params(mlp), t["before"], "parameters after backward_grads")
  nl = mlp.n_layers - 1
  delta = exact._counts_delta(mlp, counts)
  assert delta == {"forward": (0, 0), "dgrad": (nl - 1, 0), "dgrad_input": (1, 0), "wgrad": (nl, 0)}, delta
  # the bf16 copies too: the same logits, and the same gradients into given tensors, without dx
  exact._same(mlp.forward(t["case"]["x"]), t["y"], "y after backward_grads")
  given = [torch.empty_like(g) for g in grads]
  dx2, again = mlp.backward_grads(t["case"]["dy"], need_dx=False, grads=given)
  assert dx2 is None and all(a is g for a, g in zip(again, given))
  same_list(given, grads, "exported again")
  mlp.close()


# ---- T2. twin towers: SGD inside against export, p - lr g, load
@pytest.mark.parametrize("name", ["one_workgroup", "tile128_deep"])
def test_twin_towers(name):
  t = truth(name)
  case, lr = t["case"], t["case"]["lr"]
  inside, outside = tower(t), tower(t)
  dx_in = inside.backward(case["dy"], lr)
  dx_out, grads = outside.backward_grads(case["dy"])
  exact._same(dx_out, dx_in, "dx")
  variables = outside.variables()
  same_list(variables, t["before"], "variables()")
  outside.load_params([p - lr * g for p, g in zip(variables, grads)])
  same_list(params(outside), params(inside), "parameters of the twin")
  same_list(params(inside), t["after"], "parameters after the step", as_f64=True)
  # the next step reads wb (forward) and wt (dgrad) as load_params wrote them
  exact._same(outside.forward(case["x"]), inside.forward(case["x"]), "y of the next forward")
  dx_in, g_in = inside.backward_grads(case["dy"])
  dx_out, g_out = outside.backward_grads(case["dy"])
  exact._same(dx_out, dx_in, "dx of the next step")
  same_list(g_out, g_in, "gradients of the next step")
  inside.close()
  outside.close()


# ---- T3. stale slabs: the slabs of THIS batch only
def test_stale_slabs_of_a_larger_batch_are_not_summed():
  big, small = truth("batches"), truth("batches", batch=128, reseed=2)
  mlp = tower(big, max_batch=2048)
  mlp.backward(big["case"]["dy"], big["case"]["lr"])     # 16 slabs, all written
  same_list(params(mlp), big["after"], "parameters after the step at B = 2048", as_f64=True)
  load(mlp, small)
  dx, grads = mlp.backward_grads(small["case"]["dy"])     # 2 slabs; 14 hold the larger batch's values
  exact._same(dx, small["dx"], "dx")
  same_list(grads, small["g_ref"], "exported at B = 128", as_f64=True)
  mlp.close()


# ---- T4. alignment forms
def test_destinations_and_sources_four_bytes_off():
  t = truth("tile128_deep")
  mlp = DenseMlp(t["case"]["widths"], max_batch=t["case"]["batch"])
  src = []
  for p in t["before"]:
    v = off4(p.shape)
    v.copy_(p)
    src.append(v)
  mlp.load_params(src)
  same_list(params(mlp), t["before"], "parameters loaded from sources 4 bytes off")
  exact._same(mlp.forward(t["case"]["x"]), t["y"], "y")
  grads = [off4(s) for s in mlp.param_shapes()]
  dx, _ = mlp.backward_grads(t["case"]["dy"], grads=grads)
  exact._same(dx, t["dx"], "dx")
  same_list(grads, t["g_ref"], "exported 4 bytes off", as_f64=True)
  mlp.close()


@pytest.mark.parametrize("name", ["one_workgroup", "tile128_deep"])
def test_export_into_one_flat_buffer(name):
  t = truth(name)
  mlp = tower(t)
  shapes = mlp.param_shapes()
  numels = [int(np.prod(s)) for s in shapes]
  offs = D.aligned_flat_offsets(numels)
  flat = torch.full((offs[-1],), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
  views = [flat[o:o + n].view(s) for o, n, s in zip(offs, numels, shapes)]
  assert all(v.data_ptr() % 16 == 0 for v in views)
  mlp.backward_grads(t["case"]["dy"], need_dx=False, grads=views)
  same_list(views, t["g_ref"], "exported into the flat buffer", as_f64=True)
  pad = torch.ones(offs[-1], dtype=torch.bool, device="cuda")
  for o, n in zip(offs, numels):
    pad[o:o + n] = False
  assert int(pad.sum()) == offs[-1] - sum(numels) > 0
  assert bool((flat.view(torch.int32)[pad] == SENTINEL).all()), "the padding was written"
  # the views are what aligned_flat_split hands out: the buffer is the allreduce buffer as it stands
  same_list(D.aligned_flat_split(shapes, flat), views, "aligned_flat_split of the buffer")
  mlp.close()


# ---- T5. two simulated ranks
def test_two_ranks_equal_the_full_batch():
  t = truth("one_workgroup", batch=256)
  case, lr = t["case"], t["case"]["lr"]
  full = tower(t)
  full.backward(case["dy"], lr)
  same_list(params(full), t["after"], "parameters of the full-batch tower", as_f64=True)
  ranks, grads = [], []
  for lo in (0, 128):
    mlp = DenseMlp(case["widths"], max_batch=128)
    mlp.load_params(t["before"])
    exact._same(mlp.forward(case["x"][lo:lo + 128].contiguous()), t["y"][lo:lo + 128], "y of a half")
    grads.append(mlp.backward_grads(case["dy"][lo:lo + 128].contiguous(), need_dx=False)[1])
    ranks.append(mlp)
  flats = [D.aligned_flat_concat(g) for g in grads]
  for r, mlp in enumerate(ranks):
    calls = []

    def add_other(flat, other=flats[1 - r]):
      calls.append(1)
      flat.add_(other)

    mean = FU.allreduce_cond(grads[r], allreduce=add_other, world=2)
    assert calls == [1]
    same_list([2 * g for g in mean], t["g_ref"], "sum of the ranks' gradients", as_f64=True)
    mlp.load_params([p - (2 * lr) * g for p, g in zip(mlp.variables(), mean)])
    same_list(params(mlp), params(full), "parameters of rank %d" % r)
    mlp.close()
  full.close()


# ---- T6. a real optimizer
def test_adamom_on_exported_gradients():
  t = truth("tile128_deep")
  mlp = tower(t)
  _, grads = mlp.backward_grads(t["case"]["dy"], need_dx=False)
  variables = mlp.variables()
  opt = O.AdamomOptimizer(use_v2=False, align=16, **DT.HYPER["adamom"])
  opt.apply_gradients(zip(grads, variables))
  mlp.load_params(variables)
  model = DT.Model("adamom", [b.cpu().numpy() for b in t["before"]], watch=DT.Tracker())
  model.step([g.to(torch.float32).cpu().numpy() for g in t["g_ref"]])
  for i, (v, p, want) in enumerate(zip(variables, params(mlp), model.vars)):
    DT.assert_same_bits(v.cpu().numpy(), want, "variable %d" % i)
    assert not np.array_equal(want, t["before"][i].cpu().numpy())
    exact._same(p, v.view(p.shape), "parameter %d of the tower" % i)
  mlp.close()


# ---- more than 16 GEMM layers: the layer table is cut into two launches
def test_a_tower_of_seventeen_gemm_layers():
  """[128] x 18 + [1] at B = 128: both kernels take one launch for layers 0 - 15 and one for layer 16 and the
  row-dot layer.  No exact reference at this depth; what holds for any finite operands is the contract itself:
  get_params returns what load_params was given, and backward(lr) with lr a power of two equals p - lr * g on
  all bits (lr * g is exact, the subtraction is the one rounding on both sides).  Weights near the identity
  and a positive input keep every gate open, so that every layer has a gradient."""
  widths, B, lr = [128] * 18 + [1], 128, 2.0 ** -6
  gen = torch.Generator().manual_seed(17)
  given = []
  for l in range(17):
    given += [(torch.eye(128) + 0.01 * torch.randn(128, 128, generator=gen)).cuda(),
              (0.1 * torch.rand(128, generator=gen)).cuda()]
  given += [torch.randn(1, 128, generator=gen).cuda(), torch.randn(1, generator=gen).cuda()]
  x = torch.rand(B, 128, generator=gen).cuda()
  dy = torch.randn(B, generator=gen).cuda()
  inside, outside = DenseMlp(widths, max_batch=B), DenseMlp(widths, max_batch=B)
  for mlp in (inside, outside):
    mlp.load_params(given)
    same_list(params(mlp), given, "parameters of the deep tower as loaded")
  exact._same(outside.forward(x), inside.forward(x), "y")
  dx_in = inside.backward(dy, lr)
  dx_out, grads = outside.backward_grads(dy)
  exact._same(dx_out, dx_in, "dx")
  assert all(bool(torch.isfinite(g).all()) and bool((g != 0).any()) for g in grads)
  same_list(params(outside), given, "parameters after backward_grads")
  outside.load_params([p - lr * g for p, g in zip(given, grads)])
  same_list(params(outside), params(inside), "parameters of the deep twin")
  exact._same(outside.forward(x), inside.forward(x), "y of the next forward")   # (wb of all 17 layers)
  exact._same(outside.backward_grads(dy)[0], inside.backward_grads(dy)[0], "dx of the next step")   # (wt)
  inside.close()
  outside.close()


# ---- T7. refusals, on the host
def _tables(tensors):
  n = len(tensors) // 2
  return ((C.c_void_p * n)(*[x.data_ptr() for x in tensors[0::2]]),
          (C.c_void_p * n)(*[x.data_ptr() for x in tensors[1::2]]))


def _refused(status, code, text):
  assert status == code, (status, _lib.lib().mhte_last_error().decode())
  assert _lib.lib().mhte_last_error().decode() == text


def test_refusals():
  L = _lib.lib()
  t = truth("one_workgroup")
  mlp = DenseMlp(t["case"]["widths"], max_batch=128)
  h, dy, vp = mlp._h, t["case"]["dy"], _lib.vp
  grads = [torch.empty(s, device="cuda") for s in mlp.param_shapes()]
  wg, bg = _tables(grads)
  inval, op = _lib.MHTE_INVALID_ARGUMENT, "dense_mlp_backward_grads: "
  # before any forward
  _refused(L.mhte_dense_mlp_backward_grads(h, vp(dy), None, wg, bg, None), _lib.MHTE_FAILED_PRECONDITION,
           "dense mlp: backward without a forward")
  load(mlp, t)
  before = params(mlp)
  _refused(L.mhte_dense_mlp_backward_grads(h, None, None, wg, bg, None), inval, op + "null argument: dy")
  _refused(L.mhte_dense_mlp_backward_grads(h, vp(dy), None, None, bg, None), inval, op + "null argument: weight_grads")
  _refused(L.mhte_dense_mlp_backward_grads(h, vp(dy), None, wg, None, None), inval, op + "null argument: bias_grads")
  hole = (C.c_void_p * 2)(grads[0].data_ptr(), None)
  _refused(L.mhte_dense_mlp_backward_grads(h, vp(dy), None, hole, bg, None), inval,
           op + "null argument: weight_grads[1]")
  odd = (C.c_void_p * 2)(grads[1].data_ptr() + 2, grads[3].data_ptr())
  _refused(L.mhte_dense_mlp_backward_grads(h, vp(dy), None, wg, odd, None), inval,
           op + "bias_grads[0] must be 4-byte aligned")
  _refused(L.mhte_dense_mlp_backward_grads(h, vp(dy), dy.data_ptr() + 1, wg, bg, None), inval,
           op + "dx must be 4-byte aligned")
  op = "dense_mlp_load_params: "
  _refused(L.mhte_dense_mlp_load_params(h, None, bg, None), inval, op + "null argument: weights")
  _refused(L.mhte_dense_mlp_load_params(h, wg, None, None), inval, op + "null argument: biases")
  _refused(L.mhte_dense_mlp_load_params(h, wg, hole, None), inval, op + "null argument: biases[1]")
  _refused(L.mhte_dense_mlp_load_params(h, odd, bg, None), inval, op + "weights[0] must be 4-byte aligned")
  # the wrapper: sizes, dtype, device
  with pytest.raises(ValueError, match=r"grads\[0\] \(weight of layer 0\) must have 16384 elements, got 16256"):
    mlp.backward_grads(dy, grads=[grads[0][:127]] + grads[1:])
  with pytest.raises(ValueError, match=r"variables\[3\] \(bias of layer 1\) must have 1 elements, got 2"):
    mlp.load_params(grads[:3] + [torch.zeros(2, device="cuda")])
  with pytest.raises(TypeError, match=r"variables\[1\] \(bias of layer 0\) must be a float32 tensor on cuda"):
    mlp.load_params([grads[0], grads[1].cpu(), grads[2], grads[3]])
  with pytest.raises(ValueError, match=r"a list of 4 tensors"):
    mlp.backward_grads(dy, grads=grads[:2])
  # nothing was launched by a refused call: the parameters stand, and the tower still works
  same_list(params(mlp), before, "parameters after the refusals")
  _, got = mlp.backward_grads(dy, need_dx=False)
  same_list(got, t["g_ref"], "exported after the refusals", as_f64=True)
  mlp.close()
