"""CPU suite of the FFM feature cross (csrc/mhte_ffm_core.h, mhte_ffm_host.h, monolith_amd/layer_ops.py,
monolith_amd/feature_cross.py): the numpy truth (tests/ffm_truth.py) is pinned against float64 on exact inputs and
against a float64 autograd composition on the reference test's shape; the element functions of the core header,
compiled for the host, equal the truth bit for bit in their float and their four-float form; the host's choice of
kernel form equals its restatement here; every argument the entry points can refuse on the host is refused there,
with the entry point's name and the argument; a valid call without a device is refused loudly; the symbols are on
the surface and the ABI version stands; the Python functions and the GroupInt layer check their arguments."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffm_truth as FT  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import feature_cross, layer_ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
FAKE = 0x10000   # a "device pointer" the host never follows
F = np.float32


# ---- the truth is pinned ------------------------------------------------------------------------------------
def _einsum64(left, right, grad, L, R, D, int_type):
  le = left[:, :L * D].astype(np.float64).reshape(-1, L, D)
  ri = right[:, :R * D].astype(np.float64).reshape(-1, R, D)
  B = le.shape[0]
  if int_type == "multiply":
    out = np.einsum("bld,brd->blrd", le, ri).reshape(B, -1)
    g = grad[:, :L * R * D].astype(np.float64).reshape(B, L, R, D)
    lg = np.einsum("blrd,brd->bld", g, ri)
    rg = np.einsum("blrd,bld->brd", g, le)
  else:
    out = np.einsum("bld,brd->blr", le, ri).reshape(B, -1)
    g = grad.astype(np.float64).reshape(B, L, R)
    lg = np.einsum("blr,brd->bld", g, ri)
    rg = np.einsum("blr,bld->brd", g, le)
  lgf, rgf = np.zeros(left.shape), np.zeros(right.shape)
  lgf[:, :L * D], rgf[:, :R * D] = lg.reshape(B, -1), rg.reshape(B, -1)
  return out, lgf, rgf


@pytest.mark.parametrize("int_type", FT.INT_TYPES)
@pytest.mark.parametrize("extra", [(0, 0), (1, 3)], ids=["whole features", "trailing columns"])
def test_truth_equals_float64_on_exact_inputs(int_type, extra):
  """Small integers: every product and every sum is exact in float32, so any order gives the float64 value."""
  B, L, R, D = 5, 3, 4, 6
  rng = np.random.default_rng(3)
  left = rng.integers(-8, 9, size=(B, L * D + extra[0])).astype(F)
  right = rng.integers(-8, 9, size=(B, R * D + extra[1])).astype(F)
  grad = rng.integers(-8, 9, size=(B, L * R * (1 if int_type == "dot" else D))).astype(F)
  out = FT.forward(left, right, D, int_type)
  lg, rg = FT.gradient(grad, left, right, D, int_type)
  want = _einsum64(left, right, grad, L, R, D, int_type)
  assert out.dtype == F and lg.dtype == F and rg.dtype == F
  for got, w in zip((out, lg, rg), want):
    assert got.shape == w.shape and np.array_equal(got.astype(np.float64), w)
  assert lg.shape == left.shape and rg.shape == right.shape
  if extra[0]:   # +0 bits in the trailing columns
    assert not FT.bits(lg[:, L * D:]).any() and not FT.bits(rg[:, R * D:]).any()


@pytest.mark.parametrize("int_type", FT.INT_TYPES)
def test_truth_on_the_reference_test_s_shape(int_type):
  """layer_ops_test.py:29-115: B = 8, L = 10, R = 12, D = 4; loss = sum(out)."""
  B, L, R, D = 8, 10, 12, 4
  left, right, _ = FT.case(11, B, L, R, D, int_type)
  out = FT.forward(left, right, D, int_type)
  assert left.shape == (8, 40) and right.shape == (8, 48)
  assert out.shape == ((8, 480) if int_type == "multiply" else (8, 120))
  lg, rg = FT.gradient(np.ones_like(out), left, right, D, int_type)
  assert lg.shape == (8, 40) and rg.shape == (8, 48)
  tl = torch.tensor(left, dtype=torch.float64, requires_grad=True)
  tr = torch.tensor(right, dtype=torch.float64, requires_grad=True)
  prod = tl.reshape(B, L, 1, D) * tr.reshape(B, 1, R, D)
  comp = prod.reshape(B, -1) if int_type == "multiply" else prod.sum(-1).reshape(B, -1)
  comp.sum().backward()
  for got, want in ((out, comp.detach()), (lg, tl.grad), (rg, tr.grad)):
    want = want.numpy()
    err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
    print(int_type, "relative error against float64 autograd: %.3g" % err)
    assert err <= 1e-5


def test_truth_starts_every_sum_from_plus_zero():
  """An all-zero operand: products of both signs of zero; 0 + (-0) is +0, so every sum has the bits of +0."""
  B, L, R, D = 2, 2, 3, 4
  left, right, grad = FT.case(5, B, L, R, D, "dot")
  left[:] = F(0.0)
  assert (np.signbit(right) & (right != 0)).any()
  prod = (left.reshape(B, L, 1, D) * right.reshape(B, 1, R, D))
  assert np.signbit(prod).any()   # (-0 products exist)
  out = FT.forward(left, right, D, "dot")
  assert not FT.bits(out).any()
  lg, rg = FT.gradient(grad, left, right, D, "dot")
  assert not FT.bits(rg).any() and FT.bits(lg).any()
  with pytest.raises(ValueError, match="the in/out shape not match"):
    FT.gradient(grad[:, :-1], left, right, D, "dot")


# ---- the element functions and the form selection on the host -------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  exe = str(tmp_path_factory.mktemp("ffm") / "ffm_host")
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMHTE_HOST_ONLY", "-ffp-contract=off",
                         "-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         os.path.join(ROOT, "tests", "ffm_host_driver.cc"), "-o", exe])
  return exe


def _drive(driver, tmp_path, int_type, left, right, grad, D, vec):
  path = str(tmp_path / "case.bin")
  with open(path, "wb") as f:
    f.write(struct.pack("<6i", FT.INT_TYPES.index(int_type), left.shape[0], left.shape[1], right.shape[1],
                        grad.shape[1], D))
    f.write(left.tobytes() + right.tobytes() + grad.tobytes())
  text = subprocess.run([driver, "case", path, str(vec)], capture_output=True, text=True, check=True).stdout
  return np.array([int(x, 16) for x in text.split()], dtype=np.uint32).view(F)


@pytest.mark.parametrize("int_type", FT.INT_TYPES)
@pytest.mark.parametrize("D", [1, 3, 4, 17])
def test_core_arithmetic_on_the_host_equals_the_truth(int_type, D, driver, tmp_path):
  B, L, R = 4, 3, 5
  # trailing columns: fewer than D, and multiples of 4 where the four-float form is driven too
  extra = (0, 0) if D in (1, 4) else (1, 2)
  left, right, grad = FT.case(40 + D, B, L, R, D, int_type, *extra)
  if int_type == "dot":
    left[1] = F(0.0)   # a row whose products are zeros of both signs
  out = FT.forward(left, right, D, int_type)
  lg, rg = FT.gradient(grad, left, right, D, int_type)
  want = np.concatenate([out.ravel(), lg.ravel(), rg.ravel()])
  assert np.isfinite(want).all() and np.any(want != 0)
  for vec in ((1, 4) if D % 4 == 0 else (1,)):
    got = _drive(driver, tmp_path, int_type, left, right, grad, D, vec)
    FT.assert_same_bits(got, want, "%s D=%d vec=%d" % (int_type, D, vec))


_form_truth = FT.kernel_forms   # the restatement of the host's choice, shared with the GPU suite


FORM_CASES = [(1, 1, 1), (1, 5, 3), (5, 1, 4), (10, 12, 16), (3, 7, 17), (6, 6, 64), (2, 2, 4), (13, 13, 16),
              (16, 16, 32), (48, 48, 32), (10, 12, 4), (1, 129, 64), (128, 128, 4), (130, 130, 1), (64, 64, 64),
              (1, 1, 4096), (1, 1, 4097), (1, 1, 8192)]


@pytest.mark.parametrize("aligned", [1, 0])
def test_form_selection_equals_its_restatement(aligned, driver):
  seen = set()
  for L, R, D in FORM_CASES:
    text = subprocess.run([driver, "form", str(L), str(R), str(D), str(aligned)], capture_output=True, text=True,
                          check=True).stdout
    got = [tuple(int(x) for x in line.split()) for line in text.splitlines()]
    assert got == _form_truth(L, R, D, aligned), (L, R, D, aligned, got)
    seen.update(g[3] for g in got)
  # the cases the GPU suite relies on: the 288 KiB slab goes direct, the 32 KiB one is staged
  assert _form_truth(48, 48, 32, 1)[2][1] == 0 and _form_truth(16, 16, 32, 1)[2][1] == 1
  assert _form_truth(13, 13, 16, 1)[0][2] == 19 and _form_truth(13, 13, 16, 1)[2][2] == 5
  if aligned:
    assert seen == set(range(16))   # the list reaches every form
  assert len(layer_ops.COUNTER_NAMES) == 16 and layer_ops.COUNTER_NAMES == FT.COUNTERS
  assert layer_ops.COUNTER_NAMES[0] == "forward/multiply/vec4/lds"
  assert layer_ops.COUNTER_NAMES[8 + 4 + 2 + 1] == "gradient/dot/vec1/direct"


# ---- the refusals, before any device call ---------------------------------------------------------------------
def _fwd(left=FAKE, left_cols=40, right=2 * FAKE, right_cols=48, batch=8, D=4, it=0, out=3 * FAKE, out_cols=None):
  L = _lib.lib()
  if out_cols is None:
    nl, nr = (left_cols // D, right_cols // D) if D >= 1 and left_cols >= 0 and right_cols >= 0 else (0, 0)
    out_cols = nl * nr if it == 1 else nl * nr * D
  st = L.mhte_ffm(left, left_cols, right, right_cols, batch, D, it, out, out_cols, None)
  return st, L.mhte_last_error().decode()


def _grad(grad=4 * FAKE, grad_cols=None, left=FAKE, left_cols=40, right=2 * FAKE, right_cols=48, batch=8, D=4, it=0,
          lg=5 * FAKE, rg=6 * FAKE):
  L = _lib.lib()
  if grad_cols is None:
    nl, nr = (left_cols // D, right_cols // D) if D >= 1 and left_cols >= 0 and right_cols >= 0 else (0, 0)
    grad_cols = nl * nr if it == 1 else nl * nr * D
  st = L.mhte_ffm_grad(grad, grad_cols, left, left_cols, right, right_cols, batch, D, it, lg, rg, None)
  return st, L.mhte_last_error().decode()


def _invalid(fn, name, needle, **kw):
  st, msg = fn(**kw)
  assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
  assert msg.startswith(name + ": "), msg
  assert needle in msg, msg


@pytest.mark.parametrize("it", [0, 1], ids=FT.INT_TYPES)
def test_forward_refuses_invalid_arguments_on_the_host(it):
  bad = lambda needle, **kw: _invalid(_fwd, "ffm", needle, it=it, **kw)  # noqa: E731
  bad("null argument: left", left=None)
  bad("null argument: right", right=None)
  bad("null argument: out", out=None)
  bad("batch must be >= 0, got -1", batch=-1)
  bad("left_cols must be >= 0, got -4", left_cols=-4)
  bad("right_cols must be >= 0, got -8", right_cols=-8)
  bad("dim_size must be >= 1, got 0", D=0)
  bad("dim_size must be >= 1, got -2", D=-2)
  bad("out_cols must be %d" % (120 if it else 480), out_cols=479)
  bad("out_cols must be %d" % (120 if it else 480), out_cols=(480 if it else 120))
  bad("out_cols must be", out_cols=-1)
  bad("left must be 4-byte aligned", left=FAKE + 2)
  bad("right must be 4-byte aligned", right=2 * FAKE + 1)
  bad("out must be 4-byte aligned", out=3 * FAKE + 3)
  bad("batch must be below 2^31", batch=2 ** 31)
  bad("left_cols must be below 2^31", left_cols=2 ** 31)
  bad("right_cols must be below 2^31", right_cols=2 ** 33)
  bad("overflows the kernels' 32-bit row index", left_cols=2 ** 20, right_cols=2 ** 20, D=1)
  bad("overflows the kernels' 32-bit row index", left_cols=2 ** 30, right_cols=2 ** 30, D=4)
  _invalid(_fwd, "ffm", "int_type must be 0 (multiply) or 1 (dot), got 2", it=2, out_cols=480)
  _invalid(_fwd, "ffm", "int_type must be 0 (multiply) or 1 (dot), got -1", it=-1, out_cols=480)


@pytest.mark.parametrize("it", [0, 1], ids=FT.INT_TYPES)
def test_gradient_refuses_invalid_arguments_on_the_host(it):
  bad = lambda needle, **kw: _invalid(_grad, "ffm_grad", needle, it=it, **kw)  # noqa: E731
  for name, key in (("grad", "grad"), ("left", "left"), ("right", "right"), ("left_grad", "lg"), ("right_grad", "rg")):
    bad("null argument: " + name, **{key: None})
    bad(name + " must be 4-byte aligned", **{key: 7 * FAKE + 2})
  bad("batch must be >= 0, got -3", batch=-3)
  bad("left_cols must be >= 0", left_cols=-1)
  bad("right_cols must be >= 0", right_cols=-1)
  bad("grad_cols must be >= 0, got -1", grad_cols=-1)
  bad("dim_size must be >= 1, got 0", D=0)
  bad("the in/out shape not match", grad_cols=(119 if it else 476))
  bad("the in/out shape not match", grad_cols=(480 if it else 120))
  bad("the in/out shape not match", grad_cols=0)
  bad("grad_cols must be below 2^31", grad_cols=2 ** 31)
  bad("batch must be below 2^31", batch=2 ** 40)
  bad("overflows the kernels' 32-bit row index", left_cols=2 ** 20, right_cols=2 ** 20, D=1)
  _invalid(_grad, "ffm_grad", "int_type must be 0 (multiply) or 1 (dot), got 7", it=7, grad_cols=480)


def test_launch_counts_refusals():
  L = _lib.lib()
  out = (C.c_int64 * 16)()
  assert L.mhte_ffm_launch_counts(None, 16) == _lib.MHTE_INVALID_ARGUMENT
  assert "ffm_launch_counts: null argument: out" in L.mhte_last_error().decode()
  assert L.mhte_ffm_launch_counts(out, 8) == _lib.MHTE_INVALID_ARGUMENT
  assert "n must be 16, got 8" in L.mhte_last_error().decode()
  assert L.mhte_ffm_launch_counts(out, 16) == _lib.MHTE_OK   # needs no device
  assert sorted(layer_ops.ffm_launch_counts()) == sorted(layer_ops.COUNTER_NAMES)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_a_valid_call_without_a_device_is_unavailable():
  for it in (0, 1):
    for kw in ({}, {"batch": 0}, {"left_cols": 0, "left": None}, {"left_cols": 41, "right_cols": 51},
               {"left": FAKE + 4, "right": 2 * FAKE + 4}, {"D": 1}, {"D": 17}):
      for fn in (_fwd, _grad):
        st, msg = fn(it=it, **kw)
        assert st == _lib.MHTE_UNAVAILABLE, (fn.__name__, kw, st, msg)
        assert "no CPU fallback" in msg
  # multiply: integer division of the gradient's width, as of the operands' — 483 / 4 is 120 features
  st, msg = _grad(it=0, grad_cols=483)
  assert st == _lib.MHTE_UNAVAILABLE, msg
  assert not any(layer_ops.ffm_launch_counts().values())


# ---- the surface ----------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in ("mhte_ffm", "mhte_ffm_grad", "mhte_ffm_launch_counts"):
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  for word in ("ffm_ops.cc", "ffm_kernels.h:46-157", "the in/out shape not match"):
    assert word in text, word
  p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
  sig = _lib.signatures()
  assert sig["mhte_ffm"] == (i32, [p, i64, p, i64, i64, i32, i32, p, i64, p])
  assert sig["mhte_ffm_grad"] == (i32, [p, i64, p, i64, p, i64, i64, i32, i32, p, p, p])
  assert sig["mhte_ffm_launch_counts"] == (i32, [p, i32])


# ---- the Python mirror ----------------------------------------------------------------------------------------
def test_python_argument_contract():
  a, b = torch.zeros(8, 40), torch.zeros(8, 48)
  for fn, args in ((layer_ops.ffm, (a, b, 4)), (layer_ops.ffm_grad, (torch.zeros(8, 480), a, b, 4))):
    for bad in ("sum", "Dot", None, 0):
      with pytest.raises(ValueError, match="int_type must be 'multiply' or 'dot', got %s" % re.escape(repr(bad))):
        fn(*args, int_type=bad)
  with pytest.raises(ValueError, match="the left tensor of ffm is not 2D"):
    layer_ops.ffm(torch.zeros(8, 10, 4), b, 4)
  with pytest.raises(ValueError, match="the right tensor of ffm is not 2D"):
    layer_ops.ffm(a, torch.zeros(48), 4)
  with pytest.raises(ValueError, match="the grad tensor of ffm is not 2D"):
    layer_ops.ffm_grad(torch.zeros(8, 120, 4), a, b, 4)
  with pytest.raises(TypeError, match="right must be float32"):
    layer_ops.ffm(a, b.double(), 4)
  with pytest.raises(TypeError, match="left must be float32"):
    layer_ops.ffm(a.half(), b, 4, "dot")
  with pytest.raises(TypeError, match="left must be a torch tensor"):
    layer_ops.ffm(a.numpy(), b, 4)
  with pytest.raises(ValueError, match="batch size of left and right tensor are not match"):
    layer_ops.ffm(a, torch.zeros(7, 48), 4)
  with pytest.raises(ValueError, match="batch size of grad and right tensor are not match"):
    layer_ops.ffm_grad(torch.zeros(8, 480), a, torch.zeros(9, 48), 4)
  for bad in (0, -4, 4.0, True):
    with pytest.raises(ValueError, match="dim_size must be an int >= 1"):
      layer_ops.ffm(a, b, bad)
  with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
    layer_ops.ffm(a, b, 4)


def test_group_int_argument_contract():
  G = feature_cross.GroupInt
  assert feature_cross.FFM is G
  with pytest.raises(NotImplementedError, match="use_attention=True"):
    G(use_attention=True)
  with pytest.raises(NotImplementedError, match="use_attention=True"):
    G(interaction_type="multiply", use_attention=True, attention_units=[8, 1])
  with pytest.raises(ValueError, match="use_attention needs interaction_type 'multiply'"):
    G(interaction_type="dot", use_attention=True)
  G(interaction_type="dot", use_attention=False)
  with pytest.raises(ValueError, match="interaction_type must be 'multiply' or 'dot', got 'sum'"):
    G(interaction_type="sum")
  layer = G(interaction_type="dot", out_type="stack", keep_list=True)
  cfg = layer.get_config()
  assert cfg["interaction_type"] == "dot" and cfg["keep_list"] is True and cfg["out_type"] == "stack"
  assert cfg["use_attention"] is False
  with pytest.raises(ValueError, match="at least one tensor"):
    layer(([], [torch.zeros(2, 4)]))
  with pytest.raises(TypeError, match="must be on the GPU"):
    layer(([torch.zeros(2, 4)] * 3, [torch.zeros(2, 4)] * 2))
