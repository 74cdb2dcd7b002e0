"""Plain numpy models of the ops that follow the embedding exchange, float32 throughout: the gather per merged
slot and its gradient (map_id_to_embedding.cu.cc:31-118), the ragged reductions (reduce_op.cc:29-125) and the
lookup gradient (hash_table_lookup_op.cc:110-147).  tests/test_post_exchange_truth_cpu.py holds them against
the reference's goldens; tests/test_post_exchange_forms_gpu.py holds the kernels against them bit for bit.

Every sum is a Python loop in the order the project defines, one fp32 rounding per operation."""
import numpy as np

F32 = np.float32


def gather(fused, offs, dims):
  """outputs[i][j, :] = fused[offs[i][j] : offs[i][j] + dims[i]]."""
  fused = np.asarray(fused, F32)
  return [fused[np.asarray(o, np.int64)[:, None] + np.arange(d)[None, :]].reshape(len(o), d)
          for o, d in zip(offs, dims)]


def gather_grad(fused_len, grads, offs, dims, scale, chunk=32):
  """The gradient of the gather, in the order this project defines:

    * the inputs are taken in chunks of ``chunk`` (32), chunk after chunk;
    * inside a chunk the rows that share an offset form one key, visited in global row order (rows are
      numbered input after input, row after row);
    * ``acc = 0``, then ``acc = acc + g[j, :dim_i] * scale`` per row: the product is rounded to fp32 first
      (no fused multiply-add), and a row contributes its own ``dim_i`` columns — the key is as wide as the
      widest of its rows, a column a narrower row does not have gets nothing from it;
    * then ``out[off : off + width] = out[off : off + width] + acc``, ``out`` starting as zeros.

  Rows must either share an offset or cover disjoint ranges.  With at most 32 inputs and one dim per offset
  this is the reference's sum (one GpuAtomicAdd per element, map_id_to_embedding.cu.cc:105-117) with the
  addends in row order."""
  out = np.zeros(int(fused_len), F32)
  sc = F32(scale)
  for c0 in range(0, len(grads), chunk):
    acc = {}
    for i in range(c0, min(c0 + chunk, len(grads))):
      d = int(dims[i])
      prod = (np.asarray(grads[i], F32).reshape(-1, d) * sc).astype(F32)
      o = np.asarray(offs[i], np.int64)
      for j in range(o.size):
        a = acc.get(int(o[j]))
        if a is None:
          a = np.zeros(d, F32)
        elif a.size < d:
          a = np.concatenate([a, np.zeros(d - a.size, F32)])
        a[:d] = a[:d] + prod[j]
        acc[int(o[j])] = a
    for off, a in acc.items():
      out[off:off + a.size] = out[off:off + a.size] + a
  return out


def reduce(ind, vals, batch, mode):
  """mode 0: ReduceSum (reduce_op.cc:46-49), 1: ReduceMean (:75-85, sum * (1.0f / count), an empty output is
  0 * inf = NaN), 2: ReduceSquareNorm (:110-120, sqrt of the sum of squares) — rows added one after the other
  in index order.  An index outside [0, batch) is skipped: that is this project's contract, the reference
  indexes unchecked."""
  vals = np.asarray(vals, F32)
  dim = vals.shape[1]
  acc = np.zeros((int(batch), dim), F32)
  cnt = np.zeros(int(batch), np.int64)
  for i, b in enumerate(np.asarray(ind, np.int64).reshape(-1)):
    if 0 <= b < batch:
      acc[b] = acc[b] + (vals[i] * vals[i] if mode == 2 else vals[i])
      cnt[b] += 1
  with np.errstate(divide="ignore", invalid="ignore"):
    if mode == 1:
      acc = acc * (F32(1.0) / cnt.astype(F32))[:, None]
    if mode == 2:
      acc = np.sqrt(acc)
  return acc.astype(F32)


def lookup_gradient(id_indices, id_values, input_grads):
  """(ids, grads): ids[i] = id_values[i], grads[i] = input_grads[id_indices[i, 0]]."""
  return np.asarray(id_values, np.int64).copy(), np.asarray(input_grads, F32)[np.asarray(id_indices)[:, 0]]
