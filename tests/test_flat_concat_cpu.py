"""CPU suite of the aligned flat concat / split (csrc/mhte_flat_host.h, monolith_amd/distribution_ops.py): the
layout rule against its numpy restatement (tests/flat_concat_truth.py); every argument the entry points can
refuse on the host is refused there, with the entry point's name and the argument; a valid call without a
device is refused loudly; the new symbols are on the surface and the ABI version stands; the no-launch form
of the split is view arithmetic."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flat_concat_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
SYMBOLS = ["mhte_aligned_flat_offsets", "mhte_aligned_flat_concat", "mhte_aligned_flat_decode"]
FAKE = 0x10000   # a "device pointer" the host never follows
LENS = [0, 1, 15, 16, 17, 0, 4096, 4097, 1000003, 5]


# ---- the layout rule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [4, 16, 1024])
def test_offsets_equal_the_truth(align):
  n = len(LENS)
  lens = (C.c_int64 * n)(*LENS)
  offs = (C.c_int64 * (n + 1))()
  assert _lib.lib().mhte_aligned_flat_offsets(lens, n, align, offs) == _lib.MHTE_OK
  exp = T.offsets(LENS, align)
  assert list(offs) == exp
  assert all(o % align == 0 for o in exp) and exp[1] == 0 and exp[2] == align   # an empty tensor occupies nothing
  assert D.aligned_flat_offsets(LENS, align) == exp
  assert D.aligned_flat_offsets([], align) == [0]


def test_offsets_default_alignment_is_64_bytes():
  assert D.aligned_flat_offsets([1, 17, 16]) == [0, 16, 48, 64]


def test_offsets_refusals():
  L = _lib.lib()
  one = (C.c_int64 * 1)(5)
  two = (C.c_int64 * 2)()

  def bad(needle, lens=one, n=1, align=16, offs=two):
    st = L.mhte_aligned_flat_offsets(lens, n, align, offs)
    msg = L.mhte_last_error().decode()
    assert st == _lib.MHTE_INVALID_ARGUMENT and msg.startswith("aligned_flat_offsets: ") and needle in msg, (st, msg)

  bad("null argument: lens", lens=None)
  bad("null argument: offsets", offs=None)
  bad("n must be >= 0", n=-1)
  bad("tensor 0 has the negative length -3", lens=(C.c_int64 * 1)(-3))
  for a in (0, 1, 2, 3, 12, 2048, -16):
    bad("align_elems", align=a)
  with pytest.raises(_lib.InvalidArgumentError, match="align_elems"):
    D.aligned_flat_offsets([3], align=24)


# ---- the concat's refusals, before any device call ----------------------------------------------------
def _concat(lens=(8, 0, 5), n=None, align=16, null=(), null_in=(), wire=0, out=64 * FAKE, out_elems=None,
            scale_dev=None):
  L = _lib.lib()
  lens = list(lens)
  m = len(lens)
  ins = (C.c_void_p * max(m, 1))(*[None if i in null_in else FAKE + 65536 * i for i in range(m)])
  ln = (C.c_int64 * max(m, 1))(*lens)
  a = {"inputs": ins, "lens": ln}
  for k in null:
    a[k] = None
  if out_elems is None:
    out_elems = T.offsets([max(v, 0) for v in lens], align if align in (4, 16, 1024) else 16)[-1]
  st = L.mhte_aligned_flat_concat(a["inputs"], a["lens"], m if n is None else n, align, 0.5, scale_dev, wire,
                                  C.c_void_p(out) if out is not None else None, out_elems, None)
  return st, L.mhte_last_error().decode()


def _invalid(needle, **kw):
  st, msg = _concat(**kw)
  assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
  assert msg.startswith("aligned_flat_concat: "), msg
  assert needle in msg, msg


def test_concat_refuses_invalid_arguments_on_the_host():
  _invalid("null argument: inputs", null=("inputs",))
  _invalid("null argument: lens", null=("lens",))
  _invalid("null argument: inputs", null=("inputs",), lens=(), n=0)   # also of an empty call
  _invalid("n must be >= 0", n=-1)
  _invalid("tensor 2 has the negative length -5", lens=(8, 0, -5))
  _invalid("null argument: inputs[0]", null_in=(0,))
  for a in (0, 1, 2, 3, 24, 2048, -4):
    _invalid("align_elems must be a power of two in [4, 1024], got %d" % a, align=a)
  _invalid("out_elems must be the aligned total 32, got 31", out_elems=31)
  _invalid("out_elems must be the aligned total 32, got 13", out_elems=13)      # the unaligned total
  _invalid("out_elems must be the aligned total 2048, got 32", align=1024, out_elems=32)
  _invalid("out must be 16-byte aligned", out=64 * FAKE + 8)
  _invalid("null argument: out", out=None)
  _invalid("wire", wire=2)
  # 2^31 chunks of 4096 elements: more than the 32-bit chunk index addresses
  _invalid("2^31 chunks", lens=(2 ** 43,))
  _invalid("2^31 chunks", lens=(2 ** 42, 7, 2 ** 42))


def test_decode_refuses_invalid_arguments_on_the_host():
  L = _lib.lib()

  def bad(needle, flat=FAKE, wire=0, total=64, out=2 * FAKE):
    st = L.mhte_aligned_flat_decode(flat, wire, total, 0.5, out, None)
    msg = L.mhte_last_error().decode()
    assert st == _lib.MHTE_INVALID_ARGUMENT and msg.startswith("aligned_flat_decode: ") and needle in msg, (st, msg)

  bad("total_elems must be >= 0", total=-1)
  bad("wire", wire=3)
  bad("null argument: flat", flat=None)
  bad("null argument: out", out=None)
  bad("not decoded in place", wire=1, out=FAKE)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_a_valid_call_without_a_device_is_unavailable():
  L = _lib.lib()
  for kw in ({}, {"lens": (), "n": 0}, {"null_in": (1,)}, {"wire": 1}, {"align": 1024},
             {"scale_dev": C.c_void_p(FAKE - 64)}, {"lens": (0, 0)}):   # (an empty tensor's pointer may be null)
    st, msg = _concat(**kw)
    assert st == _lib.MHTE_UNAVAILABLE, (kw, st, msg)
    assert "no CPU fallback" in msg
  for wire, out in ((0, FAKE), (0, 2 * FAKE), (1, 2 * FAKE)):   # (fp32 may be decoded in place)
    st = L.mhte_aligned_flat_decode(FAKE, wire, 64, 0.5, out, None)
    assert st == _lib.MHTE_UNAVAILABLE and "no CPU fallback" in L.mhte_last_error().decode()


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
  for op in ("MonolithAlignedFlatConcat", "MonolithAlignedFlatSplit", "FusedAlignedOutputAllocator"):
    assert op in text, op
  sig = _lib.signatures()
  assert sig["mhte_aligned_flat_offsets"] == (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p])
  assert sig["mhte_aligned_flat_concat"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p])
  assert sig["mhte_aligned_flat_decode"] == (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p,
                                                         C.c_void_p])


# ---- the Python mirror --------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [4, 16, 1024])
def test_split_without_a_launch_is_view_arithmetic(align):
  like = [torch.zeros(s) for s in T.EDGE_SHAPES]
  off = T.offsets([t.numel() for t in like], align)
  flat = torch.arange(off[-1], dtype=torch.float32)
  got = D.aligned_flat_split(like, flat, align=align)
  assert len(got) == len(like)
  for g, t, o in zip(got, like, off):
    assert g.shape == t.shape and g.dtype == torch.float32
    assert g.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    if g.numel():
      assert g.data_ptr() == flat.data_ptr() + 4 * o
      np.testing.assert_array_equal(g.numpy().ravel(), np.arange(o, o + g.numel(), dtype=np.float32))
  # shapes alone do as well, and the element count is checked
  by_shape = D.aligned_flat_split([tuple(t.shape) for t in like], flat, align=align)
  assert [g.data_ptr() for g in by_shape] == [g.data_ptr() for g in got]
  with pytest.raises(ValueError, match="elements"):
    D.aligned_flat_split(like, flat[:-1], align=align)


def test_python_argument_contract():
  with pytest.raises(TypeError, match="tensors should be a list"):
    D.aligned_flat_concat(torch.zeros(3))
  with pytest.raises(TypeError, match="float32 tensors on the GPU"):
    D.aligned_flat_concat([torch.zeros(3)])              # host tensors are not packed here
  with pytest.raises(TypeError, match="wire_dtype"):
    D.aligned_flat_concat([torch.zeros(3)], wire_dtype=torch.bfloat16)
  with pytest.raises(ValueError, match="empty list"):
    D.aligned_flat_concat([])
  with pytest.raises(TypeError, match="flat must be"):
    D.aligned_flat_split([torch.zeros(3)], torch.zeros(16, dtype=torch.float64))
  with pytest.raises(TypeError, match="on the GPU"):
    D.aligned_flat_split([torch.zeros(3)], torch.zeros(16), post_scale=0.5)   # a decode is device work
  from monolith_amd import feature_utils as F
  nones = [None, None]
  assert F.allreduce_cond(nones) is nones
  assert [e.name for e in F.GradClipType] == ["ClipByNorm", "ClipByGlobalNorm", "ClipByValue", "ClipByDenseAndSparse",
                                              "NoClip"]
