"""CPU suite of clip by global norm: the numpy truth the GPU suite compares against (tests/clip_ops_truth.py,
the fixed summation tree of csrc/mhte_clip_kernels.h) meets its error bound against float64 and reproduces
the reference test's expected values (clip_ops_test.py:39-58, committed as data); every argument the entry
points can refuse on the host is refused there, with the entry point's name; a valid call without a device is
refused loudly; the new symbols are on the whole surface."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ops_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
SYMBOLS = ["mhte_global_l2_reduce", "mhte_clip_by_global_norm", "mhte_clip_by_global_norm_dev",
           "mhte_clip_by_global_norm_fused", "mhte_scale_tensors_dev",
           "mhte_fused_gather_embeddings_by_input_gradient_dev_scale"]
FAKE = 0x10000   # a "device pointer" the host never follows


# ---- the truth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "two_rounds", "many", "dense"])
def test_truth_meets_its_bound_against_float64(name):
  tensors = getattr(T, "set_" + name)()
  got, K = T.tree_sumsq(tensors)
  chunks = sum(-(-t.size // T.CH) for t in tensors)
  assert K == -(-chunks // T.W) and K == {"edges": 1, "two_rounds": 2, "many": 1, "dense": 2}[name]
  ref = sum(float(np.sum(t.astype(np.float64) ** 2)) for t in tensors)
  rel = abs(float(got) - ref) / ref
  print("%s: rel %.3g bound %.3g" % (name, rel, T.gamma(K)))
  assert rel <= T.gamma(K)


def test_truth_bound_values():
  assert T.gamma(1) == pytest.approx(2.1e-6, rel=0.02) and T.gamma(2) == pytest.approx(3.0e-6, rel=0.02)


def test_truth_reference_first_case_exactly():
  c = T.load_kat()["clip"][0]
  ss, norm, scale = T.norm_and_scale(c["inputs"], c["clip_norm"])
  assert (ss, norm) == (np.float32(25.0), np.float32(5.0))
  outs, norm2 = T.clip(c["inputs"], c["clip_norm"])
  assert norm2 == np.float32(5.0)
  np.testing.assert_array_equal(T.bits(outs[0]), T.bits(np.array([-2.4, 0, 0], np.float32)))
  np.testing.assert_array_equal(T.bits(outs[1]), T.bits(np.array([3.2, 0, 0], np.float32)))


def test_truth_reproduces_the_reference_cases():
  kat = T.load_kat()
  assert [c["name"] for c in kat["clip"]] == ["simple", "uneven shapes", "no clipping", "zero norm",
                                              "exploded grad"]
  for c in kat["clip"]:
    outs, _ = T.clip(c["inputs"], c["clip_norm"])
    for o, e in zip(outs, c["expected"]):
      assert o.shape == e.shape
      if c["name"] == "exploded grad":
        assert np.isnan(o).all() and np.isnan(e).all()
      else:
        assert not np.isnan(o).any()          # zero norm: zeros, not NaN
        np.testing.assert_array_equal(T.bits(o), T.bits(e))
  for c in kat["norm"]:
    assert float(T.norm_and_scale(c["inputs"], np.inf)[1]) == c["expected"]
  assert len(kat["dense_shapes"]) == 53


def test_truth_empty_and_nan():
  assert T.norm_and_scale([], 1.0) == (np.float32(0), np.float32(0), np.float32(1))
  assert T.norm_and_scale([np.zeros(0, np.float32)], 1.0) == (np.float32(0), np.float32(0), np.float32(1))
  _, norm, scale = T.norm_and_scale([np.array([np.nan, 1.0], np.float32)], 1.0)
  assert np.isnan(norm) and scale == np.float32(1)   # a NaN norm passes the inputs through


# ---- the entry points on the host ---------------------------------------------------------------------
def _lists(lens, null_in=(), null_out=()):
  n = len(lens)
  ins = (C.c_void_p * max(n, 1))(*[None if i in null_in else FAKE + 65536 * i for i in range(n)])
  outs = (C.c_void_p * max(n, 1))(*[None if i in null_out else 64 * FAKE + 65536 * i for i in range(n)])
  ln = (C.c_int64 * max(n, 1))(*lens)
  return ins, outs, ln


def _call(entry, lens=(8, 0, 5), n=None, clip_norm=1.0, null=(), null_in=(), null_out=()):
  """-> (status, message) of one entry point on a plan of fake device pointers."""
  L = _lib.lib()
  ins, outs, ln = _lists(list(lens), null_in, null_out)
  n = len(lens) if n is None else n
  a = {"inputs": ins, "outputs": outs, "lens": ln, "result": C.c_void_p(FAKE - 64), "dev": C.c_void_p(FAKE - 128)}
  for k in null:
    a[k] = None
  cn, n32 = C.c_float(clip_norm), C.c_int32(n)
  if entry == "global_l2_reduce":
    st = L.mhte_global_l2_reduce(a["inputs"], a["lens"], n32, cn, a["result"], None)
  elif entry == "clip_by_global_norm":
    st = L.mhte_clip_by_global_norm(a["inputs"], a["outputs"], a["lens"], n32, C.c_float(5.0), cn, None)
  elif entry == "clip_by_global_norm_dev":
    st = L.mhte_clip_by_global_norm_dev(a["inputs"], a["outputs"], a["lens"], n32, a["dev"], cn, None)
  elif entry == "clip_by_global_norm_fused":
    st = L.mhte_clip_by_global_norm_fused(a["inputs"], a["outputs"], a["lens"], n32, cn, a["result"], None)
  elif entry == "scale_tensors_dev":
    st = L.mhte_scale_tensors_dev(a["inputs"], a["outputs"], a["lens"], n32, a["dev"], None)
  else:
    raise AssertionError(entry)
  return st, L.mhte_last_error().decode()


ENTRIES = {   # entry -> (its pointer arguments, has outputs, has clip_norm)
    "global_l2_reduce": (("inputs", "lens", "result"), False, True),
    "clip_by_global_norm": (("inputs", "outputs", "lens"), True, True),
    "clip_by_global_norm_dev": (("inputs", "outputs", "lens", "dev"), True, True),
    "clip_by_global_norm_fused": (("inputs", "outputs", "lens", "result"), True, True),
    "scale_tensors_dev": (("inputs", "outputs", "lens", "dev"), True, False),
}


def _invalid(entry, needle, **kw):
  st, msg = _call(entry, **kw)
  assert st == _lib.MHTE_INVALID_ARGUMENT, (entry, kw, st, msg)
  assert msg.startswith(entry + ": "), msg
  assert needle in msg, msg


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_invalid_arguments_are_refused_on_the_host(entry):
  ptrs, has_out, has_clip = ENTRIES[entry]
  for k in ptrs:
    _invalid(entry, "null argument", null=(k,))
    _invalid(entry, "null argument", null=(k,), lens=(), n=0)   # also of an empty call
  _invalid(entry, "n must be >= 0", n=-1)
  _invalid(entry, "tensor 2 has the negative length -5", lens=(8, 0, -5))
  _invalid(entry, "null argument", null_in=(0,))
  st, msg = _call(entry, null_in=(0,))
  assert "[0]" in msg
  if has_out:
    _invalid(entry, "null argument: outputs[2]", null_out=(2,))
  if has_clip:
    _invalid(entry, "clip_norm", clip_norm=-1.0)
    _invalid(entry, "clip_norm", clip_norm=float("nan"))


def test_gather_gradient_dev_scale_refuses_a_null_scale():
  L = _lib.lib()
  one = (C.c_void_p * 1)(FAKE)
  n = (C.c_int64 * 1)(4)
  dims = (C.c_int32 * 1)(4)
  st = L.mhte_fused_gather_embeddings_by_input_gradient_dev_scale(C.c_void_p(FAKE), C.c_int64(64), C.c_int32(1), one,
                                                                  one, n, dims, None, None)
  msg = L.mhte_last_error().decode()
  assert st == _lib.MHTE_INVALID_ARGUMENT and "fused_gather_embeddings_by_input_gradient_dev_scale" in msg, msg
  assert "scale_dev" in msg


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_valid_call_without_a_device_is_unavailable(entry):
  for kw in ({}, {"lens": (), "n": 0}, {"null_in": (1,), "null_out": (1,)}):   # (an empty tensor's pointers may be null)
    st, msg = _call(entry, **kw)
    assert st == _lib.MHTE_UNAVAILABLE, (entry, kw, st, msg)
    assert "no CPU fallback" in msg


# ---- the surface --------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in SYMBOLS:
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  # each declaration's comment cites the reference op it stands for
  for op in ("GlobalL2Reduce", "MonolithClipByGlobalNorm", "MonolithClipByGlobalNormFused",
             "layout_tensors_grad_scale", "MonolithFusedGatherEmbeddingsByInputGradient"):
    assert op in text, op
  sig = _lib.signatures()
  assert sig["mhte_global_l2_reduce"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p,
                                                      C.c_void_p])
  assert sig["mhte_clip_by_global_norm"][1][4:6] == [C.c_float, C.c_float]


def test_header_still_compiles_as_c99():
  r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr


# ---- the Python mirror --------------------------------------------------------------------------------
def test_clip_ops_argument_contract():
  from monolith_amd import clip_ops
  with pytest.raises(TypeError, match="t_list should be a list"):
    clip_ops.clip_by_global_norm((torch.zeros(3),), 1.0)
  with pytest.raises(TypeError, match="t_list should be a list"):
    clip_ops.clip_by_global_norm(torch.zeros(3), 1.0)
  empty = []
  got = clip_ops.clip_by_global_norm(empty, 1.0)
  assert got[0] is empty and got[1] == 0 and isinstance(got, tuple)
  assert clip_ops._global_norm([]) is None
  with pytest.raises(TypeError):
    clip_ops.scale_tensors([torch.zeros(3)], 0.5)       # the scale is a device tensor
  with pytest.raises(TypeError):
    clip_ops.clip_by_global_norm([torch.zeros(3)], 1.0)  # host tensors are not clipped here
