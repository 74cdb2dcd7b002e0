"""CPU suite of FeatureInsight (csrc/mhte_fi_core.h, mhte_fi_host.h, monolith_amd/layer_ops.py): the numpy truth
(tests/feature_insight_truth.py) equals fp64 bit for bit on exact inputs and reproduces the reference's own example
(tests/golden/feature_insight_kat.json); the element and chain functions of the core header, compiled for the host,
equal the truth's fp32 definition bit for bit; the plan equals its restatement and the entry point, reports no
workspace for the forward and stays small for the gradient; every argument the entry points can refuse on the host
is refused there; a valid call without a device is refused loudly; the symbols are on the surface and the ABI
version stands; the Python functions check their arguments."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import feature_insight_truth as FT  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import layer_ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
KAT = os.path.join(ROOT, "tests", "golden", "feature_insight_kat.json")
FAKE = 0x10000   # a "device pointer" the host never follows
F = np.float32


# ---- the truth is pinned ------------------------------------------------------------------------------------
def test_fmaf_rounds_once():
  # a b = 2^-24 (1 - 2^-46) lies just BELOW half an ulp of c = 1 + 2^-23: the sum rounds down to c.  Rounding it to
  # 53 bits first lands ON the middle of two fp32 values, and a second rounding (ties to even) then goes up.
  a, b, c = F(2.0 ** -24 * (1 + 2.0 ** -23)), F(1 - 2.0 ** -23), F(1 + 2.0 ** -23)
  assert float(a) * float(b) == 2.0 ** -24 * (1 - 2.0 ** -46)                      # exact in fp64
  assert float(F(np.float64(a) * np.float64(b) + np.float64(c))) == 1 + 2.0 ** -22  # the double rounding
  assert float(FT.fmaf(a, b, c)) == 1 + 2.0 ** -23                                  # the single one
  assert float(FT.fmaf(-a, b, -c)) == -(1 + 2.0 ** -23)
  assert float(FT.fmaf(F(3), F(5), F(7))) == 22.0
  assert FT.bits(FT.fmaf(F(-0.0), F(3.0), F(0.0))).ravel()[0] == 0                   # -0 + +0 = +0


@pytest.mark.parametrize("what", ["plain", "aggregate"])
def test_truth_equals_fp64_bit_for_bit_on_exact_inputs(what):
  sizes, K, B = [1, 8, 7, 3], 33, 37
  x, w, g = FT.inputs(1, B, sizes, K, exact=8 if what == "plain" else 3)
  t, d = FT.Truth(x, w, sizes, g), FT.Fp32(x, w, sizes)
  if what == "plain":
    assert np.abs(t.out).max() < 2 ** 24 and np.array_equal(d.out().astype(np.float64), t.out)
    assert np.array_equal(d.input_grad(g).astype(np.float64), t.input_grad)
    assert np.array_equal(d.weight_grad(g).astype(np.float64), t.weight_grad)
  else:
    assert np.abs(t.agg).max() < 2 ** 24 and np.array_equal(d.agg().astype(np.float64), t.agg)
  assert t.out.any() and t.weight_grad.any()


def test_truth_bit_for_bit_over_several_slabs_and_a_long_segment():
  sizes, K, B = [200, 0, 5], 3, 300
  x, w, g = FT.inputs(2, B, sizes, K, exact=8)
  assert FT.plan(B, sum(sizes), K, len(sizes))["slabs"] >= 3
  t, d = FT.Truth(x, w, sizes, g), FT.Fp32(x, w, sizes)
  assert np.array_equal(d.out().astype(np.float64), t.out) and not d.out()[:, K:2 * K].any()
  assert np.array_equal(d.input_grad(g).astype(np.float64), t.input_grad)
  assert np.array_equal(d.weight_grad(g).astype(np.float64), t.weight_grad)


def _kat():
  with open(KAT) as f:
    k = json.load(f)
  x = np.array(k["input"], dtype=F).reshape(k["batch"], -1)
  w = np.array(k["weight"], dtype=F).reshape(-1, k["k"])
  g = np.ones((k["batch"], len(k["segment_sizes"]) * k["k"]), dtype=F)
  return k, x, w, g


def test_truth_reproduces_the_reference_example_within_its_bound():
  k, x, w, g = _kat()
  assert k["segment_sizes"] == [3, 2, 4] and (k["k"], k["batch"]) == (2, 3) and k["grad_is"] == "ones"
  t, d = FT.Truth(x, w, k["segment_sizes"], g), FT.Fp32(x, w, k["segment_sizes"])
  b = t.bounds()
  np.testing.assert_allclose(np.array(k["out"])[0], [0.22, 0.22, 0.17, 0.53, 2.10, 2.14], atol=1e-6)
  np.testing.assert_allclose(np.array(k["agg"])[0], [0.0968, 0.3098, 8.9896], atol=1e-6)
  for name, got in (("out", d.out()), ("agg", d.agg()), ("input_grad", d.input_grad(g)),
                    ("weight_grad", d.weight_grad(g))):
    want = np.array(k[name])
    assert np.abs(getattr(t, name) - want).max() <= 1e-15 * np.abs(want).max(), name   # the fp64 value
    assert (np.abs(got.astype(np.float64) - want) <= b[name]).all(), name               # the fp32 definition
    assert (b[name] <= 32 * FT.U * np.abs(want)).all()   # all terms positive: a few ulp


# ---- the core header on the host ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  exe = str(tmp_path_factory.mktemp("fi") / "fi_host")
  subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-DMHTE_HOST_ONLY", "-ffp-contract=off",
                         "-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         os.path.join(ROOT, "tests", "fi_host_driver.cc"), "-o", exe])
  return exe


def _run(exe, *args):
  return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout


def test_constants_on_the_host(driver):
  consts = dict((k, int(v)) for k, v in (line.split() for line in _run(driver, "consts").splitlines()))
  assert consts == dict(tile=FT.TILE, stage=FT.STAGE, lanes=FT.LANES, inline=FT.INLINE, max_segments=FT.MAX_SEGMENTS,
                        max_slabs=FT.MAX_SLABS, target_groups=FT.TARGET_GROUPS, counters=len(FT.COUNTERS),
                        max_extent=FT.MAX_BATCH)
  assert FT.MAX_SEGMENTS >= 1024
  assert layer_ops.FI_COUNTER_NAMES == FT.COUNTERS and layer_ops.FI_PLAN_NAMES == FT.PLAN_NAMES


@pytest.mark.parametrize("sizes,K,B", [([3, 2, 4], 2, 3), ([1, 8, 7, 3], 33, 37), ([0, 40, 0, 1, 0], 17, 200),
                                       ([9], 1, 1), ([33, 31], 5, 0)])
def test_core_functions_equal_the_fp32_definition_bit_for_bit(driver, tmp_path, sizes, K, B):
  x, w, g = FT.inputs(3, B, sizes, K)
  src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
  np.concatenate([x.ravel(), w.ravel(), g.ravel()]).tofile(src)
  _run(driver, "op", src, dst, B, K, len(sizes), *sizes)
  got = np.fromfile(dst, dtype=F)
  d = FT.Fp32(x, w, sizes)
  E, nseg = sum(sizes), len(sizes)
  want = [d.out(), d.agg(), d.input_grad(g), d.weight_grad(g)]
  assert got.size == sum(a.size for a in want) == B * nseg * K + B * nseg + B * E + E * K
  at = 0
  for name, a in zip(("out", "agg", "input_grad", "weight_grad"), want):
    assert np.array_equal(FT.bits(got[at:at + a.size]), FT.bits(a).ravel()), name
    at += a.size


PLAN_SHAPES = [(0, 9, 2, 3), (1, 1, 1, 1), (3, 9, 2, 3), (63, 0, 5, 2), (64, 416, 64, 26), (65, 416, 64, 26),
               (129, 9, 2, 3), (300, 205, 3, 3), (4096, 416, 64, 26), (65536, 416, 64, 26), (65536, 416, 1024, 26),
               (65536, 4096, 1024, 1), (1000, 129, 7, 129), (100, 4096, 1, 4096), (FT.MAX_BATCH, 8, 1, 2),
               (5, FT.MAX_COLS, 1, 1), (5, 1, FT.MAX_COLS, 1)]


def test_plan_equals_its_restatement_and_the_entry_point(driver):
  for B, E, K, nseg in PLAN_SHAPES:
    want = FT.plan(B, E, K, nseg)
    assert [int(v) for v in _run(driver, "plan", B, E, K, nseg).split()] == [want[n] for n in FT.PLAN_NAMES]
    out = (C.c_int64 * 9)()
    assert _lib.lib().mhte_feature_insight_plan(B, E, K, nseg, out, 9) == _lib.MHTE_OK
    assert list(out) == [want[n] for n in FT.PLAN_NAMES], (B, E, K, nseg)
    assert layer_ops.feature_insight_plan(B, E, K, nseg) == want
    # every row is in exactly one slab, no slab is empty; the forward needs no workspace in either mode
    assert want["slab_rows"] % FT.TILE == 0 and 1 <= want["slabs"] <= FT.MAX_SLABS
    assert (want["slabs"] - 1) * want["slab_rows"] < max(B, 1) <= want["slabs"] * want["slab_rows"]
    assert want["forward_workspace_bytes"] == 0
    assert want["groups"] == (nseg + FT.INLINE - 1) // FT.INLINE


def test_the_gradient_workspace_stays_below_the_size_of_grad():
  B, nseg, K, E = 65536, 26, 1024, 416
  p = FT.plan(B, E, K, nseg)
  assert 0 < p["grad_workspace_bytes"] < 4 * B * nseg * K
  assert p["grad_workspace_bytes"] < 64 << 20                     # 5 slabs of 1.7 MB
  assert FT.plan(B, E, 64, nseg)["slabs"] == 64 and FT.plan(B, E, 64, nseg)["grad_workspace_bytes"] < 8 << 20


# ---- the refusals, before any device call ---------------------------------------------------------------------
def _sizes(sizes):
  return None if sizes is None else (C.c_int32 * len(sizes))(*sizes)


def _fwd(input=FAKE, weight=2 * FAKE, batch=8, in_cols=9, k=2, sizes=(3, 2, 4), n_segments=None, aggregate=0,
         out=3 * FAKE, out_cols=None):
  L = _lib.lib()
  n = (len(sizes) if sizes is not None else 3) if n_segments is None else n_segments
  if out_cols is None:
    out_cols = n if aggregate == 1 else n * k
  st = L.mhte_feature_insight(input, weight, batch, in_cols, k, _sizes(sizes), n, aggregate, out, out_cols, None)
  return st, L.mhte_last_error().decode()


def _grad(grad=4 * FAKE, grad_cols=None, input=FAKE, weight=2 * FAKE, batch=8, in_cols=9, k=2, sizes=(3, 2, 4),
          n_segments=None, input_grad=5 * FAKE, weight_grad=6 * FAKE):
  L = _lib.lib()
  n = (len(sizes) if sizes is not None else 3) if n_segments is None else n_segments
  if grad_cols is None:
    grad_cols = n * k
  st = L.mhte_feature_insight_grad(grad, grad_cols, input, weight, batch, in_cols, k, _sizes(sizes), n, input_grad,
                                   weight_grad, None)
  return st, L.mhte_last_error().decode()


def _invalid(fn, name, needle, **kw):
  st, msg = fn(**kw)
  assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
  assert msg.startswith(name + ": "), msg
  assert needle in msg, msg


@pytest.mark.parametrize("fn,name", [(_fwd, "feature_insight"), (_grad, "feature_insight_grad")],
                         ids=["forward", "gradient"])
def test_entry_points_refuse_invalid_arguments_on_the_host(fn, name):
  bad = lambda needle, **kw: _invalid(fn, name, needle, **kw)  # noqa: E731
  for arg in ("input", "weight"):
    bad("null argument: " + arg, **{arg: None})
    bad(arg + " must be 4-byte aligned", **{arg: 9 * FAKE + 2})
  bad("null argument: segment_sizes", sizes=None)
  bad("batch must be >= 0, got -1", batch=-1)
  bad("batch must be at most 2^30 - 64, got %d" % (FT.MAX_BATCH + 1), batch=FT.MAX_BATCH + 1)
  bad("k must be in [1, %d], got 0" % FT.MAX_COLS, k=0)
  bad("k must be in [1, %d], got -3" % FT.MAX_COLS, k=-3)
  bad("k must be in [1, %d], got %d" % (FT.MAX_COLS, FT.MAX_COLS + 1), k=FT.MAX_COLS + 1)
  bad("in_cols must be in [0, %d], got -1" % FT.MAX_COLS, in_cols=-1)
  bad("in_cols must be in [0, %d], got %d" % (FT.MAX_COLS, FT.MAX_COLS + 1), in_cols=FT.MAX_COLS + 1)
  bad("n_segments must be in [1, 4096], got 0", n_segments=0)
  bad("n_segments must be in [1, 4096], got -1", n_segments=-1)
  bad("n_segments must be in [1, 4096], got 4097", sizes=(0,) * 4097)
  bad("segment_sizes[1] must be >= 0, got -2", sizes=(7, -2, 4))
  bad("the sum of segment_sizes must be in_cols = 9, got 8", sizes=(3, 1, 4))
  bad("the sum of segment_sizes must be in_cols = 9, got 10", sizes=(3, 3, 4))
  bad("batch * n_segments * k must fit 2^60 elements", batch=FT.MAX_BATCH, k=FT.MAX_COLS, sizes=(0,) * 4095 + (9,))
  if fn is _fwd:
    bad("null argument: out", out=None)
    bad("out must be 4-byte aligned", out=3 * FAKE + 1)
    bad("out_cols must be 6 (n_segments * k), got 3", out_cols=3)
    bad("out_cols must be 3 (n_segments), got 6", aggregate=1, out_cols=6)
    for v in (2, -1, 256):
      bad("aggregate must be 0 or 1, got %d" % v, aggregate=v, out_cols=6)
  else:
    bad("null argument: grad", grad=None)
    bad("grad must be 4-byte aligned", grad=4 * FAKE + 2)
    bad("grad_cols must be 6 (n_segments * k), got 5", grad_cols=5)
    bad("null argument: input_grad and weight_grad", input_grad=None, weight_grad=None)
    bad("input_grad must be 4-byte aligned", input_grad=5 * FAKE + 3)
    bad("weight_grad must be 4-byte aligned", weight_grad=6 * FAKE + 1)


def test_plan_and_launch_counts_refusals():
  L = _lib.lib()
  out = (C.c_int64 * 9)()
  for args, needle in (((8, 9, 2, 3, None, 9), "feature_insight_plan: null argument: out"),
                       ((8, 9, 2, 3, out, 5), "feature_insight_plan: n must be 9, got 5"),
                       ((-1, 9, 2, 3, out, 9), "feature_insight_plan: batch must be >= 0"),
                       ((8, 9, 0, 3, out, 9), "feature_insight_plan: k must be in [1,"),
                       ((8, 9, 2, 0, out, 9), "feature_insight_plan: n_segments must be in [1, 4096]"),
                       ((8, 9, 2, 4097, out, 9), "feature_insight_plan: n_segments must be in [1, 4096]")):
    assert L.mhte_feature_insight_plan(*args) == _lib.MHTE_INVALID_ARGUMENT
    assert needle in L.mhte_last_error().decode()
  assert L.mhte_feature_insight_launch_counts(None, 5) == _lib.MHTE_INVALID_ARGUMENT
  assert "feature_insight_launch_counts: null argument: out" in L.mhte_last_error().decode()
  assert L.mhte_feature_insight_launch_counts(out, 4) == _lib.MHTE_INVALID_ARGUMENT
  assert "n must be 5, got 4" in L.mhte_last_error().decode()
  assert L.mhte_feature_insight_launch_counts(out, 5) == _lib.MHTE_OK   # needs no device
  assert tuple(layer_ops.feature_insight_launch_counts()) == FT.COUNTERS


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_a_valid_call_without_a_device_is_unavailable():
  empty = {"batch": 0, "input": None}
  for kw in ({}, empty, {"sizes": (0, 9, 0)}, {"sizes": (9,)}, {"in_cols": 0, "sizes": (0, 0), "input": None,
                                                                "weight": None},
             {"input": FAKE + 4, "weight": 2 * FAKE + 12}):
    for fn in (_fwd, _grad):
      st, msg = fn(**kw)
      assert st == _lib.MHTE_UNAVAILABLE, (fn.__name__, kw, st, msg)
      assert "no CPU fallback" in msg
  assert _fwd(aggregate=1)[0] == _lib.MHTE_UNAVAILABLE
  assert _fwd(batch=0, input=None, out=None)[0] == _lib.MHTE_UNAVAILABLE
  assert _grad(batch=0, input=None, grad=None)[0] == _lib.MHTE_UNAVAILABLE
  for kw in ({"input_grad": None}, {"weight_grad": None}):
    assert _grad(**kw)[0] == _lib.MHTE_UNAVAILABLE
  assert not any(layer_ops.feature_insight_launch_counts().values())


# ---- the surface ----------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in ("mhte_feature_insight", "mhte_feature_insight_grad", "mhte_feature_insight_plan",
            "mhte_feature_insight_launch_counts"):
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  for word in ("feature_insight_ops.cc", "feature_insight_kernels.cc:70-83", ":148-160", "layer_ops.py:49-85"):
    assert word in text, word
  p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
  sig = _lib.signatures()
  assert sig["mhte_feature_insight"] == (i32, [p, p, i64, i64, i32, p, i32, i32, p, i64, p])
  assert sig["mhte_feature_insight_grad"] == (i32, [p, i64, p, p, i64, i64, i32, p, i32, p, p, p])
  assert sig["mhte_feature_insight_plan"] == (i32, [i64, i64, i32, i32, p, i32])
  assert sig["mhte_feature_insight_launch_counts"] == (i32, [p, i32])
  for name in ("feature_insight", "feature_insight_grad", "feature_insight_plan", "feature_insight_launch_counts"):
    assert callable(getattr(layer_ops, name))


# ---- the Python mirror ----------------------------------------------------------------------------------------
def test_python_argument_contract():
  x, w, g = torch.zeros(8, 9), torch.zeros(9, 2), torch.zeros(8, 6)
  sizes = [3, 2, 4]
  fns = ((lambda a, b, s: layer_ops.feature_insight(a, b, s), "feature_insight"),
         (lambda a, b, s: layer_ops.feature_insight(a, b, s, aggregate=True), "feature_insight"),
         (lambda a, b, s: layer_ops.feature_insight_grad(g, a, b, s), "feature_insight_grad"))
  for fn, name in fns:
    with pytest.raises(ValueError, match="%s: segment_sizes must not be empty" % name):
      fn(x, w, [])
    with pytest.raises(TypeError, match="segment_sizes must hold ints, got 2.0"):
      fn(x, w, [3, 2.0, 4])
    with pytest.raises(TypeError, match="segment_sizes must be a sequence of ints"):
      fn(x, w, 9)
    with pytest.raises(TypeError, match="input_embedding must be float32"):
      fn(x.double(), w, sizes)
    with pytest.raises(TypeError, match="weight must be float32"):
      fn(x, w.half(), sizes)
    with pytest.raises(TypeError, match="weight must be a torch tensor"):
      fn(x, w.numpy(), sizes)
    with pytest.raises(ValueError, match="input_embedding is not 2D"):
      fn(torch.zeros(72), w, sizes)
    with pytest.raises(ValueError, match="weight is not 2D"):
      fn(x, torch.zeros(9, 2, 1), sizes)
    with pytest.raises(ValueError, match=r"columns of input_embedding and the rows of weight do not match \(9, 8\)"):
      fn(x, torch.zeros(8, 2), sizes)
    with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
      fn(x, w, sizes)
  with pytest.raises(TypeError, match="aggregate must be a bool"):
    layer_ops.feature_insight(x, w, sizes, aggregate="yes")
  with pytest.raises(ValueError, match=r"the batch size of grad and input_embedding do not match \(7, 8\)"):
    layer_ops.feature_insight_grad(torch.zeros(7, 6), x, w, sizes)
  with pytest.raises(TypeError, match="grad must be float32"):
    layer_ops.feature_insight_grad(g.double(), x, w, sizes)
  with pytest.raises(ValueError, match="at least one of want_input and want_weight"):
    layer_ops.feature_insight_grad(g, x, w, sizes, want_input=False, want_weight=False)
