"""CPU suite of the segment retrievers (quantization-aware training): the NumPy truth the GPU tests
compare with (tests/qat_truth.py) against the reference's own known-answer tests and its own
fake_quantizer.h; the compressors of entry.py; the comp_config arm of the serialized-config reader
(csrc/mhte_proto_config.h), in the manner of tests/test_proto_config_cpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from monolith_amd import _lib, entry
from tests import ckpt_proto as P
from tests import qat_truth as Q

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------- the reference's KATs
def test_fake_quantizer_known_answers():
  """compressor/fake_quantizer_test.cc:29-47, exact"""
  r = 5.0
  k = np.float32(5.0) / np.float32(128)
  q = lambda x: Q.fake_quant(np.array([x], dtype=np.float32), r)[0]   # noqa: E731
  assert q(100.0) < 5.0
  assert q(0.0) == 0.0
  assert abs(q(3.5) - np.float32(3.5)) < k
  assert q(k * np.float32(1.4)) == k
  assert q(k * np.float32(1.6)) == k * np.float32(2)
  assert q(-k * np.float32(1.4)) == -k
  assert q(-k * np.float32(1.6)) == -k * np.float32(2)
  assert q(np.nan) == 0
  # the range is asymmetric, and the conversion passes through an integer: no negative zero
  assert q(1e6) == np.float32(127) * k and q(-1e6) == np.float32(-128) * k
  for x in (-0.0, -1e-9, -float(k) * 0.49):
    out = Q.fake_quant(np.array([x], dtype=np.float32), r)
    assert out.view(np.uint32)[0] == 0, x


def test_hash_net_known_answers():
  """compressor/hash_net_quantizer_test.cc:24-44 and retriever/hash_net_retriever_test.cc:47-50, to 1e-4
  relative, in the reference's own float32 arithmetic: 1 - y^2 cancels where scale * w is about 5, so one
  ulp of tanh is 3e-4 of the gradient there (0.005442613 recorded; float32 NumPy gives 0.005442916, the
  float64 evaluation 0.005443621).  Everywhere else the float64 truth agrees to 1e-4 as well."""
  rel = 1e-4
  for dtype in (np.float32, np.float64):
    m = Q.HashNet(step_size=1000, dtype=dtype)        # the proto's defaults: 1.0, 10000, 0.1
    assert m.scale == 1.0
    assert m.forward(1.0) == pytest.approx(0.07615941, rel=rel)
    assert m.forward(2.0) == pytest.approx(0.09640275, rel=rel)
    assert m.backward(2.0, 1.0, 0) == pytest.approx(0.00706508, rel=rel)
    assert m.backward(2.0, 2.0, 999) == pytest.approx(0.01413016, rel=rel)
    g1, g2 = m.backward(2.0, 100.0, 1000), m.backward(2.0, 200.0, 1001)
    if dtype is np.float32:
      assert g1 == pytest.approx(0.005442613, rel=rel)
      assert g2 == pytest.approx(0.01088523, rel=rel)
    assert m.forward(2.0) == pytest.approx(0.09998888, rel=rel)
    assert m.scale == pytest.approx(2.44948974, rel=1e-6)
    m = Q.HashNet(step_size=100, dtype=dtype)
    assert m.backward(1.0, 1.0, 100) == pytest.approx(0.35840667 * float(m.amplitude), rel=rel)
  # the cap
  assert Q.hash_net_scale(10**9, 1.0, 10.0) == 10.0


# -------------------------------------------------------------- the sweep against the reference header
@pytest.mark.skipif(not os.path.isdir(REF) or shutil.which("g++") is None,
                    reason="needs the reference's sources and g++")
@pytest.mark.parametrize("r", [1.0, 5.0, 0.3])
def test_fake_quant_truth_is_the_reference_header_bit_for_bit(r, tmp_path):
  exe = str(tmp_path / "qat_ref_driver")
  b = subprocess.run(["g++", "-O2", "-std=c++17", "-I" + REF, os.path.join(HERE, "qat_ref_driver.cc"), "-o", exe],
                     capture_output=True, text=True)
  assert b.returncode == 0, b.stderr
  x = Q.fake_quant_sweep(r)
  assert x.size == 201129
  out = subprocess.run([exe, repr(r)], input=x.tobytes(), capture_output=True, check=True).stdout
  ref = np.frombuffer(out, dtype=np.float32)
  got = Q.fake_quant(x, r)
  assert ref.size == x.size
  mism = np.flatnonzero(ref.view(np.uint32) != got.view(np.uint32))
  assert mism.size == 0, (mism.size, x[mism[:5]], ref[mism[:5]], got[mism[:5]])
  # the inputs whose quotient is exactly integral are in the sweep: a division one ulp off flips them
  step = np.float32(r) / np.float32(128)
  f = np.where(x >= 0, x + step / np.float32(2), x - step / np.float32(2)).astype(np.float32)
  qf = (f / step).astype(np.float32)
  exact = np.isfinite(qf) & (qf == np.trunc(qf)) & (np.abs(qf) <= 129)
  assert exact.sum() >= 200


# ------------------------------------------------------------------------------------------ entry.py
def test_entry_accepts_the_four_compressors_and_refuses_anything_else():
  mk = lambda c: entry.CombineAsSegment(4, entry.ZerosInitializer(), entry.SgdOptimizer(0.1), c)   # noqa: E731
  assert mk(None).compressor is None
  assert mk(entry.Fp32Compressor()).compressor.retriever() == (_lib.MHTE_RETRIEVER_RAW, ())
  assert mk(entry.Fp16Compressor()).compressor.retriever() == (_lib.MHTE_RETRIEVER_RAW, ())
  assert mk(entry.FixedR8Compressor()).compressor.retriever() == (_lib.MHTE_RETRIEVER_FAKE_QUANT_R8, (1.0,))
  assert mk(entry.FixedR8Compressor(fixed_range=0.3)).compressor.r == pytest.approx(0.3)
  one = mk(entry.OneBitCompressor()).compressor
  assert (one.step_size, one.amplitude) == (200, 0.05)          # reference entry.py:469
  assert one.retriever() == (_lib.MHTE_RETRIEVER_HASH_NET, (200.0, 1.0, 10000.0, 0.05))
  assert mk(entry.OneBitCompressor(step_size=7, amplitude=0.1)).compressor.retriever()[1][0] == 7.0
  for c in (entry.Fp32Compressor, entry.Fp16Compressor, entry.FixedR8Compressor, entry.OneBitCompressor):
    assert issubclass(c, entry.Compressor)
  for bad in (object(), "fp16", entry.Compressor(), 8):
    with pytest.raises(NotImplementedError):
      mk(bad)


# ---------------------------------------------------------------------------------- the proto reader
def _varint(n):
  out = bytearray()
  while n >= 0x80:
    out.append((n & 0x7f) | 0x80)
    n >>= 7
  out.append(n)
  return bytes(out)


def _ld(field, payload):
  return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def _f32(field, v):
  return _varint((field << 3) | 5) + np.float32(v).tobytes()


def _i64(field, v):
  return _varint((field << 3) | 0) + _varint(v & ((1 << 64) - 1))


def comp_config(arm, body=b""):
  """wire bytes of Segment.comp_config (field 3) = FloatCompressorConfig{<arm>: {body}}; the restated
  descriptors of tests/ckpt_proto.py do not carry the field"""
  return _ld(3, _ld(arm, body))


def one_table(comp=b"", serving=False, opt="adagrad"):
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("t")
  c = m.configs.add()
  c.cuckoo.SetInParent()
  s = c.entry_config.segments.add()
  s.dim_size = 4
  s.init_config.zeros.dim_size = 4
  getattr(s.opt_config, opt).learning_rate = 0.1
  if comp:
    s.MergeFromString(comp)
  if serving:
    c.entry_config.entry_type = 2
  return m.SerializeToString()


needs_no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only: with a device the create succeeds")


def _create(blob):
  L = _lib.lib()
  h = C.c_void_p()
  lrs = (C.c_float * 64)()
  st = L.mhte_multi_table_create_from_proto(blob, C.c_int64(len(blob)), None, C.c_uint64(0), C.c_float(0.0),
                                            C.c_int32(0), b"qat_cpu_test", lrs, C.c_int32(64), C.byref(h))
  return st, L.mhte_last_error().decode()


def test_the_comp_config_survives_the_independent_encoder():
  """(the unknown field must reach the serialized bytes for the cases below to mean anything)"""
  assert comp_config(4, _i64(2, 7)) in one_table(comp_config(4, _i64(2, 7)))


@needs_no_device
@pytest.mark.parametrize("case", ["fp32", "fp16", "fixed_r8_default", "fixed_r8_r", "one_bit_default",
                                  "one_bit_fields", "dim_size_only"])
def test_every_comp_config_arm_parses(case):
  comp = {"fp32": comp_config(1), "fp16": comp_config(2), "fixed_r8_default": comp_config(3),
          "fixed_r8_r": comp_config(3, _f32(2, 0.3)), "one_bit_default": comp_config(4),
          "one_bit_fields": comp_config(4, _i64(2, 4) + _f32(3, 2.0) + _f32(4, 9.0) + _f32(5, 0.05)),
          "dim_size_only": comp_config(4, _i64(1, 4))}[case]
  st, msg = _create(one_table(comp))
  assert st == _lib.MHTE_UNAVAILABLE, (case, st, msg)     # accepted: it gets as far as the missing device


@needs_no_device
@pytest.mark.parametrize("step_size", [0, -1, -200])
def test_one_bit_step_size_must_be_positive(step_size):
  st, msg = _create(one_table(comp_config(4, _i64(2, step_size))))
  assert st == _lib.MHTE_INVALID_ARGUMENT and "step_size" in msg, (st, msg)


@needs_no_device
@pytest.mark.parametrize("comp", [b"", comp_config(3), comp_config(4)])
def test_serving_entries_stay_refused(comp):
  st, msg = _create(one_table(comp, serving=True))
  assert st == _lib.MHTE_INVALID_ARGUMENT and "SERVING" in msg, (st, msg)


@needs_no_device
def test_a_truncated_comp_config_is_refused():
  bad = one_table(_ld(3, _ld(3, _f32(2, 0.3))[:-2]))   # the arm's length runs past the comp_config
  st, msg = _create(bad)
  assert st == _lib.MHTE_INVALID_ARGUMENT and msg, (st, msg)
