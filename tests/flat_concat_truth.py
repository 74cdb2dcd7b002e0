"""The numpy truth of the aligned flat concat / split (csrc/mhte_flat_kernels.h): the round-up rule of the
offsets, the concat — one float32 product per element, then numpy's cast for the fp16 wire (round to
nearest-even, overflow to inf, subnormals kept), +0 in the padding — and the decode."""
import numpy as np

EDGE_SHAPES = [(0,), (1,), (3,), (15,), (16,), (17,), (4095,), (4096,), (4097,), (8193,), (3, 5), (2, 3, 7), (64, 65),
               (0, 4)]
NAN_BITS = 0x7fc00000   # the quiet NaN numpy and the device both produce from it


def offsets(numels, align=16):
  """n + 1 offsets: tensor i starts at the sum of round_up(numels[j], align) over j < i."""
  assert align >= 1 and align & (align - 1) == 0
  off = [0]
  for n in numels:
    off.append(off[-1] + ((int(n) + align - 1) & ~(align - 1)))
  return off


def concat(arrays, scale=1.0, wire=np.float32, align=16):
  off = offsets([a.size for a in arrays], align)
  out = np.zeros(off[-1], wire)
  with np.errstate(over="ignore", invalid="ignore", under="ignore"):
    for a, o in zip(arrays, off):
      out[o:o + a.size] = (np.asarray(a, np.float32).ravel() * np.float32(scale)).astype(wire)
  return out


def decode(flat, post_scale=1.0):
  with np.errstate(over="ignore", invalid="ignore", under="ignore"):
    return flat.astype(np.float32) * np.float32(post_scale)


def split(like, flat, align=16):
  off = offsets([a.size for a in like], align)
  return [flat[o:o + a.size].reshape(a.shape) for a, o in zip(like, off)]


def raw(a):
  """The raw bits of a float32 or float16 array."""
  a = np.ascontiguousarray(a)
  return a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


# ---- the input sets of the suites (seeded; list order is part of the contract) ---------------------------
def set_edges(seed=11):
  rng = np.random.default_rng(seed)
  return [rng.standard_normal(s).astype(np.float32) for s in EDGE_SHAPES]


def set_seeded(count, seed):
  """``count`` tensors of seeded lengths 1 .. 300."""
  rng = np.random.default_rng(seed)
  return [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(1, 301, count)]


def set_two_roundings(scale, count=256, seed=17):
  """Values x for which the order "float32 product, then fp16 conversion" shows: the float32 product x * scale
  is inexact and lands exactly on a tie between two fp16 neighbours, so that converting the exact product in
  one step rounds to the other neighbour for about every second of them.  -> (x [count], the fp16 bits of the
  one-step conversion) — the caller checks that the two orders differ."""
  rng = np.random.default_rng(seed)
  s = np.float32(scale)
  found = []
  while sum(f.size for f in found) < count:
    x = rng.uniform(0.5, 4.0, 1 << 20).astype(np.float32)
    p = x * s
    exact = x.astype(np.float64) * np.float64(s)
    tie = (p.view(np.uint32) & 0x1fff) == 0x1000     # the 13 bits fp16 drops: exactly one half
    found.append(x[tie & (exact != p.astype(np.float64))])
  x = np.concatenate(found)[:count]
  one_step = (x.astype(np.float64) * np.float64(s)).astype(np.float16)
  return x, one_step.view(np.uint16)


def set_fp16_edges():
  """Values whose fp16 conversion is the point: overflow (beyond 65504, and the tie 65520 that rounds to inf),
  the subnormal range (below 2^-14) down to the tie at 2^-25 and below it, ties between two fp16 neighbours
  (to even both ways), -0 and NaN; repeated with both signs to 4 full chunks and a ragged end."""
  pos = np.array([65504.0, 65519.996, 65520.0, 70000.0, 1e30, 3.0e-5, 6.1e-5, 5.9604645e-8, 2.9802322e-8,
                  2.9802326e-8, 1.0e-8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20,
                  2048.0 + 1.0, 2048.0 + 3.0, 0.1, 1.0 / 3.0, 0.0, 1.4e-45, 1.1754942e-38], np.float32)
  base = np.concatenate([pos, -pos, np.array([NAN_BITS], np.uint32).view(np.float32)])
  return [np.resize(base, 4 * 4096 + 37), np.resize(base[::-1], 45), base.copy()]
