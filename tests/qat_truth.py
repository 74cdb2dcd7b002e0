"""NumPy restatement of the reference's quantization-aware-training quantizers: the truth the
segment-retriever tests compare the engine with (tests/test_qat_truth_cpu.py checks the restatement
itself, against the reference's known-answer tests and, where the reference's sources are present,
against its own fake_quantizer.h compiled in place).

FakeQuantizer (compressor/fake_quantizer.h:26-70): float32 throughout, the quotient truncated THROUGH
AN INTEGER type.  HashNetQuantizer (compressor/hash_net_quantizer.h:33-70): float64 arithmetic on
float32 inputs — the engine's float32 tanhf / powf are compared with it to a tolerance."""
import numpy as np


def fake_quant(x, r):
  """FakeQuantizer(r).Quantize(x), bit for bit (inputs whose quotient leaves int range, +-inf
  included, are undefined behaviour in the reference and not defined here either)."""
  x = np.asarray(x, dtype=np.float32)
  step = np.float32(r) / np.float32(128)
  half = step / np.float32(2)
  nan = np.isnan(x)
  f = np.where(nan, np.float32(0), x).astype(np.float32)
  f = np.where(f >= 0, f + half, f - half).astype(np.float32)
  q = (f / step).astype(np.float32)             # correctly rounded fp32 division
  n = np.clip(q.astype(np.int64), -128, 127)    # truncation through an integer: -0.4 -> 0 -> +0.0
  n = np.where(nan, 0, n)
  return (n.astype(np.float32) * step).astype(np.float32)


def fake_quant_sweep(r, n_random=200000, seed=0):
  """The inputs the restatement was checked on against the reference's header for range ``r``: every
  rounding boundary (k + 1/2) * step for k in -140..140 with the float on each side, every grid point
  k * step, +-0, NaN, +-1e6 and ``n_random`` uniform draws in +-2r."""
  r32 = np.float32(r)
  step = r32 / np.float32(128)
  k = np.arange(-140, 141, dtype=np.float32)
  bound = ((k + np.float32(0.5)) * step).astype(np.float32)
  grid = (k * step).astype(np.float32)
  pts = [bound, np.nextafter(bound, np.float32(np.inf)), np.nextafter(bound, np.float32(-np.inf)), grid,
         np.array([0.0, -0.0, np.nan, 1e6, -1e6], dtype=np.float32),
         np.random.RandomState(seed).uniform(-2 * float(r), 2 * float(r), n_random).astype(np.float32)]
  return np.concatenate(pts).astype(np.float32)


def hash_net_scale(global_step, init_scale=1.0, max_scale=10000.0, dtype=np.float64):
  """the scale HashNetQuantizer::Backward sets at a ``global_step`` that its step_size divides"""
  t = dtype
  s = t(np.float32(init_scale)) * np.sqrt(t(1) + t(np.float32(0.005)) * t(np.float32(global_step)))
  return float(min(t(s), t(np.float32(max_scale))))


class HashNet:
  """HashNetQuantizer(step_size, init_scale, max_scale, amplitude) with its scale state.  ``dtype``:
  float64, the truth the engine is compared with; float32 restates the reference's own arithmetic (its
  known-answer tests were recorded in it: where scale * w is about 5, 1 - tanh^2 cancels and one ulp of
  the float32 tanh is 3e-4 of the result)."""

  def __init__(self, step_size=200, init_scale=1.0, max_scale=10000.0, amplitude=0.1, dtype=np.float64):
    self.t = dtype
    self.step_size, self.init_scale, self.max_scale = int(step_size), float(np.float32(init_scale)), max_scale
    self.amplitude = dtype(np.float32(amplitude))
    self.scale = dtype(self.init_scale)

  def forward(self, w):
    return self.amplitude * np.tanh(self.scale * np.asarray(w, dtype=np.float32).astype(self.t))

  def backward(self, w, g, global_step):
    """-> g scaled by the derivative at the stored weight w; moves the scale first where due"""
    if int(global_step) % self.step_size == 0:
      self.scale = self.t(hash_net_scale(global_step, self.init_scale, self.max_scale, self.t))
    y = np.tanh(self.scale * np.asarray(w, dtype=np.float32).astype(self.t))
    return np.asarray(g, dtype=np.float32).astype(self.t) * (self.amplitude * self.scale * (self.t(1) - y * y))
