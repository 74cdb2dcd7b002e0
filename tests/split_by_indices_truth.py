"""Numpy truth of the split-by-indices ops: the reference's loops restated from their semantics
(MonolithSplitByIndices, MonolithSplitByIndicesGradient, MonolithRaggedSplitByIndices).  The ops only move and
count, so every comparison made with these is on raw bits."""
import numpy as np

COUNTERS = ("rows/vec1", "rows/vec4", "gradient/vec1", "gradient/vec4", "plan", "plan/ragged")


def bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(got, want, what=""):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
  assert np.array_equal(bits(got), bits(want)), what


def plan(indices, num_splits):
  """-> (pos, sizes, n_bad): the elements walked in order, each appended to its split; an index outside
  [0, num_splits) belongs to no split.  pos is the splits' positions one split after the other, -1 behind."""
  lists = [[] for _ in range(num_splits)]
  n_bad = 0
  for i, s in enumerate(np.asarray(indices, np.int64).tolist()):
    if 0 <= s < num_splits:
      lists[s].append(i)
    else:
      n_bad += 1
  sizes = np.array([len(l) for l in lists], np.int64)
  pos = np.full(len(indices), -1, np.int64)
  flat = [i for l in lists for i in l]
  pos[:len(flat)] = flat
  return pos, sizes, n_bad


def split(indices, tensor, num_splits):
  """The split: num_splits arrays, element i of ``tensor`` appended to split indices[i] in input order."""
  tensor = np.asarray(tensor)
  lists = [[] for _ in range(num_splits)]
  for i, s in enumerate(np.asarray(indices, np.int64).tolist()):
    lists[s].append(i)
  return [tensor[np.array(l, np.int64)] if l else np.zeros((0,) + tensor.shape[1:], tensor.dtype) for l in lists]


def gradient(indices, grads, shape):
  """The gradient of ``split``: element i takes the row of its split's gradient that it became."""
  out = np.zeros(shape, grads[0].dtype if len(grads) else np.float32)
  cursor = [0] * len(grads)
  for i, s in enumerate(np.asarray(indices, np.int64).tolist()):
    out[i] = grads[s][cursor[s]]
    cursor[s] += 1
  return out


def split_row_splits(indices, row_splits, num_splits):
  """[num_splits, T + 1]: how many elements of every split lie in front of each boundary.  The reference's walk:
  a boundary is emitted when the walk reaches it, for every split at once — empty rows repeat the count, and the
  boundaries at n (trailing empty rows) are emitted after the last element."""
  row_splits = np.asarray(row_splits, np.int64)
  out = np.zeros((num_splits, row_splits.size), np.int64)
  offsets = [0] * num_splits
  t = 1
  idx = np.asarray(indices, np.int64).tolist()
  i = 0
  while True:
    while t < row_splits.size and i == row_splits[t]:
      for s in range(num_splits):
        out[s, t] = offsets[s]
      t += 1
    if i >= len(idx):
      break
    if 0 <= idx[i] < num_splits:
      offsets[idx[i]] += 1
    i += 1
  assert t == row_splits.size, "The input ragged tensor is invalid."
  return out


def ragged_split(indices, values, row_splits, num_splits):
  """-> (splits, positions): per split a (values, row_splits) pair, and the same with the original positions."""
  values = np.asarray(values, np.int64)
  assert values.size == len(indices), "Ragged tensor values size must match indices size"
  pos = split(indices, np.arange(len(indices), dtype=np.int64), num_splits)
  vals = split(indices, values, num_splits)
  rs = split_row_splits(indices, row_splits, num_splits)
  return [(v, rs[s]) for s, v in enumerate(vals)], [(p, rs[s]) for s, p in enumerate(pos)]


def to_lists(values, row_splits):
  """A ragged pair as nested lists."""
  v = np.asarray(values).tolist()
  return [v[int(a):int(b)] for a, b in zip(row_splits[:-1], row_splits[1:])]


def mover_form(elem_bytes, element_size, aligned16):
  """The movers' rule: 16-byte accesses when a row is whole 16-byte words and every buffer is 16-byte aligned."""
  return "vec4" if (aligned16 and (element_size * elem_bytes) % 16 == 0) else "vec1"


def indices_for(pattern, n, num_splits, seed=0):
  """The index patterns of the GPU suite."""
  rng = np.random.RandomState(seed + 7 * n + num_splits)
  a = np.arange(n, dtype=np.int64)
  if pattern == "uniform":
    return rng.randint(0, num_splits, size=n).astype(np.int64)
  if pattern == "one split":
    return np.full(n, num_splits - 1, np.int64)
  if pattern == "alternating":
    return a % min(2, num_splits)
  if pattern == "ascending":
    return a * num_splits // max(n, 1)
  if pattern == "descending":
    return (num_splits - 1) - a * num_splits // max(n, 1)
  if pattern == "one empty":   # split num_splits // 2 never occurs (with one split: nothing is left out)
    v = rng.randint(0, num_splits, size=n).astype(np.int64)
    if num_splits > 1:
      v[v == num_splits // 2] = (num_splits // 2 + 1) % num_splits
    return v
  raise ValueError(pattern)


PATTERNS = ("uniform", "one split", "alternating", "ascending", "descending", "one empty")
