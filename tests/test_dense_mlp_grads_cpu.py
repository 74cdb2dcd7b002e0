"""CPU suite of the dense tower's gradient export and parameter load (mhte_dense_mlp_backward_grads /
mhte_dense_mlp_load_params, monolith_amd/dense_mlp.py): what needs no device.  The two symbols are declared,
exported and typed from the header, the ABI version stands, a null handle is refused on the host with the entry
point's name, the Python wrapper checks the tensors it is given, and the exact reference of
tests/test_dense_mlp_exact_gpu.py holds its own conditions for the operands of the two-rank test of
tests/test_dense_mlp_grads_gpu.py (case ``one_workgroup`` at B = 256 and its two halves)."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_dense_mlp_exact_gpu as exact  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd.dense_mlp import DenseMlp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
FAKE = 0x10000   # a "device pointer" the host never follows
NAMES = ("mhte_dense_mlp_backward_grads", "mhte_dense_mlp_load_params")


def test_symbols_declared_exported_and_typed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in NAMES:
    assert s in declared and s in _lib.EXPORTS and hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  p, i32 = C.c_void_p, C.c_int32
  sig = _lib.signatures()
  assert sig["mhte_dense_mlp_backward_grads"] == (i32, [p, p, p, p, p, p])
  assert sig["mhte_dense_mlp_load_params"] == (i32, [p, p, p, p])
  # the existing entry points keep their signatures
  assert sig["mhte_dense_mlp_backward"] == (i32, [p, p, p, C.c_float, p])
  for word in ("must be 4-byte aligned", "dense mlp: backward without a forward", "mhte_aligned_flat_offsets",
               "one launch per 16 layers"):
    assert word in text, word


def test_a_null_handle_is_refused_on_the_host():
  L = _lib.lib()
  tab = (C.c_void_p * 2)(FAKE, 2 * FAKE)
  st = L.mhte_dense_mlp_backward_grads(None, FAKE, None, tab, tab, None)
  assert st == _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_last_error().decode() == "dense_mlp_backward_grads: null argument: m"
  st = L.mhte_dense_mlp_load_params(None, tab, tab, None)
  assert st == _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_last_error().decode() == "dense_mlp_load_params: null argument: m"


def _wrapper(widths):
  """A DenseMlp without a handle: the argument checks of the wrapper run before any call into the library."""
  m = DenseMlp.__new__(DenseMlp)
  m.widths, m._device, m._h = list(widths), torch.device("cpu"), None
  return m


def test_python_wrapper_checks_its_tensors():
  m = _wrapper([256, 128, 1])
  assert m.param_shapes() == [(128, 256), (128,), (1, 128), (1,)]
  good = [torch.zeros(s) for s in m.param_shapes()]
  w, b = m._checked("grads", good)
  assert list(w) == [good[0].data_ptr(), good[2].data_ptr()] and list(b) == [good[1].data_ptr(), good[3].data_ptr()]
  m._checked("variables", [good[0].view(-1), good[1], good[2].view(128), good[3]])   # numel counts, not the shape
  with pytest.raises(ValueError, match=r"grads: a list of 4 tensors .* got 3"):
    m._checked("grads", good[:3])
  with pytest.raises(ValueError, match=r"variables: a list of 4 tensors"):
    m._checked("variables", good[0])
  with pytest.raises(ValueError, match=r"grads\[1\] \(bias of layer 0\) must have 128 elements, got 127"):
    m._checked("grads", [good[0], torch.zeros(127), good[2], good[3]])
  with pytest.raises(ValueError, match=r"grads\[2\] \(weight of layer 1\) must have 128 elements, got 256"):
    m._checked("grads", [good[0], good[1], torch.zeros(2, 128), good[3]])
  with pytest.raises(TypeError, match=r"variables\[0\] \(weight of layer 0\) must be a float32 tensor on cpu"):
    m._checked("variables", [good[0].double()] + good[1:])
  with pytest.raises(TypeError, match=r"variables\[3\] \(bias of layer 1\) must be a float32 tensor"):
    m._checked("variables", good[:3] + [None])
  with pytest.raises(ValueError, match=r"grads\[0\] \(weight of layer 0\) must be contiguous"):
    m._checked("grads", [torch.zeros(256, 128).t()] + good[1:])


def test_reference_conditions_hold_for_the_two_rank_case():
  """T5's operands: RefExact's own assertions (exact fp32 sums, open gates, rounded activations) on the full
  B = 256 problem and on both halves, with the learning rates the test applies (lr and 2 lr)."""
  case = exact.make_case("one_workgroup", batch=256, device="cpu")
  lr = case["lr"]
  for lo, hi, rate in ((0, 256, lr), (0, 128, 2 * lr), (128, 256, 2 * lr)):
    ref = exact.RefExact(case["widths"])
    ref.set_params(0, case["w"][0], case["b"][0])
    ref.set_params(1, case["last"][1], case["b_last"])
    ref.forward(case["x"][lo:hi])
    ref.backward(case["dy"][lo:hi], rate)
    assert ref.margin and max(ref.margin.values()) < 1.0, ref.margin
