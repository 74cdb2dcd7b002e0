"""The numpy truth of clip by global norm (csrc/mhte_clip_kernels.h), in float32: the fixed summation tree
of the sum of squares, restated — chunks of 4096 floats per tensor, 1024 workgroups that take chunks
w, w + 1024, ..., a thread's (chunk, r, k) chain into one accumulator, the halvings 128 .. 1 over a
workgroup's 256 accumulators and 512 .. 1 over the 1024 partials — and the clip x * (clip / norm)."""
import json
import os

import numpy as np

W, T, CH = 1024, 256, 4096
U = 2.0 ** -24

EDGE_LENS = [0, 1, 3, 4, 5, 4095, 4096, 4097, 8191, 12289]


def tree_sumsq(tensors):
  """-> (sum of squares as np.float32, rounds of chunks per workgroup)."""
  chunks = []
  for t in tensors:
    t = np.asarray(t, np.float32).ravel()
    if t.size == 0:
      continue
    pad = (-t.size) % CH
    chunks.append(np.concatenate([t, np.zeros(pad, np.float32)]).reshape(-1, CH))
  C = sum(c.shape[0] for c in chunks)
  if C == 0:
    return np.float32(0), 0
  allc = np.concatenate(chunks, 0)
  K = -(-C // W)
  allc = np.concatenate([allc, np.zeros((K * W - C, CH), np.float32)], 0)
  a = allc.reshape(K, W, 4, T, 4)   # [round][workgroup w][float4 row r][thread t][component k]
  acc = np.zeros((W, T), np.float32)
  with np.errstate(over="ignore", invalid="ignore"):
    for k in range(K):
      for r in range(4):
        for c in range(4):
          v = a[k, :, r, :, c]
          acc = acc + v * v           # product and sum rounded to fp32 one after the other
    s = T // 2
    while s:
      acc = acc[:, :s] + acc[:, s:2 * s]
      s //= 2
    p = acc[:, 0]
    s = W // 2
    while s:
      p = p[:s] + p[s:2 * s]
      s //= 2
  return np.float32(p[0]), K


def gamma(K):
  """The relative error bound of the tree against the exact sum: m roundings on any path from an input to
  the result — one per product, one per add of a thread's chain of 16 K addends, 8 + 10 tree levels."""
  m = 16 * K + 19
  return m * U / (1 - m * U)


def norm_and_scale(tensors, clip_norm):
  """-> (sum, norm, scale) as np.float32: norm = sqrt(sum), scale = norm > clip ? clip / norm : 1."""
  ss, _ = tree_sumsq(tensors)
  with np.errstate(invalid="ignore"):
    norm = np.sqrt(ss, dtype=np.float32)
    scale = np.float32(clip_norm) / norm if norm > np.float32(clip_norm) else np.float32(1)
  return ss, norm, np.float32(scale)


def clip(tensors, clip_norm, use_norm=None):
  """-> (clipped list, norm): x * np.float32(clip / norm) in float32; the inputs' bits when not clipped."""
  if use_norm is None:
    _, norm, scale = norm_and_scale(tensors, clip_norm)
  else:
    norm = np.float32(use_norm)
    scale = np.float32(clip_norm) / norm if norm > np.float32(clip_norm) else np.float32(1)
  outs = []
  with np.errstate(invalid="ignore"):
    for t in tensors:
      t = np.asarray(t, np.float32)
      outs.append(t.copy() if scale == np.float32(1) else t * np.float32(scale))
  return outs, norm


def bits(a):
  return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def load_kat():
  """The expectations of the reference's clip_ops_test.py:39-58, :83-87 (data: inputs, clip_norm, expected)
  and the dense gradient shapes of its "large grad" case (:60-68)."""
  with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_ops_kat.json")) as f:
    kat = json.load(f)

  for c in kat["clip"]:
    c["inputs"] = [np.array([float(v) for v in row], np.float32) for row in c["inputs"]]
    c["expected"] = [np.array([float(v) for v in row], np.float32) for row in c["expected"]]
  for c in kat["norm"]:
    c["inputs"] = [np.array([float(v) for v in row], np.float32) for row in c["inputs"]]
    c["expected"] = float(c["expected"])
  kat["dense_shapes"] = [tuple(s) for s in kat["dense_shapes"]]
  return kat


# ---- the input sets of the suites (seeded; list order is part of the contract) ---------------------------
def set_edges(seed=3):
  rng = np.random.default_rng(seed)
  return [rng.standard_normal(n).astype(np.float32) for n in EDGE_LENS]


def set_two_rounds(seed=4):
  rng = np.random.default_rng(seed)
  return [rng.standard_normal(W * CH + 5).astype(np.float32), rng.standard_normal(7).astype(np.float32)]


def set_many(seed=5):
  rng = np.random.default_rng(seed)
  return [rng.standard_normal(3000).astype(np.float32) for _ in range(150)]


def set_dense(seed=6):
  rng = np.random.default_rng(seed)
  return [rng.uniform(size=s).astype(np.float32) for s in load_kat()["dense_shapes"]]
