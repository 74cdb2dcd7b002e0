"""The numpy truth of the fused reduce-and-split pooling ops (shared by the CPU and GPU test files) and
the seeded inputs of the GPU cases.

The truth adds ONE row at a time into an fp32 accumulator that starts at +0 — the sequential chain of the
reference kernel (`sum = T(0); sum += ...`) and of the CPU op (accumulation into a zeroed output) —
vectorised over the batch rows and looped over the position inside the row."""
import json
import os

import numpy as np

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_reduce_split_kat.json")


def load_kat():
  with open(KAT) as f:
    return json.load(f)


def splits_of_sorted(id_indices, batch):
  """row_splits [batch + 1] of ascending row indices."""
  return np.searchsorted(np.asarray(id_indices, np.int64), np.arange(batch + 1)).astype(np.int32)


def truth_forward(row_splits, emb, slice_dims):
  """-> list of [bs, d] float32 arrays, one per slice of this feature."""
  rs = np.asarray(row_splits, np.int64)
  emb = np.asarray(emb, np.float32)
  bs, dim = rs.size - 1, emb.shape[1]
  assert sum(slice_dims) == dim
  lens = rs[1:] - rs[:-1]
  acc = np.zeros((bs, dim), np.float32)   # +0
  order = np.argsort(-lens, kind="stable")   # batch rows, longest first: the rows with a p-th id are a prefix
  by_len = lens[order]
  for p in range(int(lens.max()) if bs else 0):
    k = int(np.searchsorted(-by_len, -p, side="left"))   # rows with lens > p
    rows = order[:k]
    acc[rows] = acc[rows] + emb[rs[rows] + p]   # one fp32 add per element, in row order
  cuts = np.cumsum(slice_dims)[:-1]
  return [np.ascontiguousarray(a) for a in np.split(acc, cuts, axis=1)]


def truth_gradient(row_splits, n_rows, slice_grads):
  """-> [n_rows, sum d]: row r = the slice gradients, side by side, at the batch row whose range holds r;
  0 for the rows before rs[0] and from rs[bs] on."""
  rs = np.asarray(row_splits, np.int64)
  g = np.concatenate([np.asarray(x, np.float32) for x in slice_grads], axis=1)
  out = np.zeros((n_rows, g.shape[1]), np.float32)
  lens = rs[1:] - rs[:-1]
  rowids = np.repeat(np.arange(rs.size - 1), lens)
  out[rs[0]:rs[-1]] = g[rowids]
  return out


def bits(a):
  return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ---- seeded inputs of the order-sensitive GPU cases ---------------------------------------------------
DIMS = (16, 32, 64)
SLICES = {16: [4, 12], 32: [8, 8, 16], 64: [16, 48]}


def order_sensitive_case(seed, bs, n_features=26, long_row=2048):
  """26 features of dims 16/32/64 cycled: skewed row lengths (half the rows empty, mean about 2, one row of
  `long_row` ids), values = normal * 2**randint(-20, 20) (any re-association changes bits), a row whose
  only addend is -0.0, a row of three -0.0, an empty feature, features whose ranges leave a head and a
  tail of rows uncovered.  -> list of dicts (row_splits int32, emb float32, slice_dims)."""
  rng = np.random.default_rng(seed)
  feats = []
  for i in range(n_features):
    dim = DIMS[i % 3]
    lens = rng.geometric(0.25, size=bs) * (rng.random(bs) < 0.5)
    if i == 3:
      lens[:] = 0                      # an empty feature: n_i = 0
    if i == 0:
      lens[bs // 3] = long_row
    if i == 1:
      lens[5], lens[6], lens[7] = 1, 0, 3
    head, tail = (3, 5) if i % 4 == 2 else (0, 0)
    rs = (head + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    n = int(rs[-1]) + tail
    emb = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-20, 21, size=(n, dim)))).astype(np.float32)
    if i == 1:
      emb[rs[5]] = -0.0
      emb[rs[7]:rs[8]] = -0.0
    feats.append({"row_splits": rs, "emb": emb, "slice_dims": SLICES[dim]})
  return feats
