"""The numpy models of tests/post_exchange_truth.py against the reference's own goldens
(distribution_ops_test.py:221-352, the numbers tests/test_parity_gpu.py quotes) and two hand-worked cases for
what the goldens do not reach: the chunk order of the gather gradient and rows of different widths on one
offset.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import post_exchange_truth as T  # noqa: E402

F32 = np.float32


def test_gather_golden():
  """distribution_ops_test.py:221-249."""
  fused = np.array([1.1, 1.2, 1.3, 2.1, 2.2, 3.1, 3.2, 3.3, 4.1, 4.2, 4.3, 5.1, 5.2, 6.1, 6.2, 6.3,
                    7.1, 7.2, 8.1, 8.2, 9.1, 9.2], F32)
  outs = T.gather(fused, [[13, 0, 5, 13, 8, 13], [16, 18, 11, 11, 16, 20, 3]], [3, 2])
  np.testing.assert_array_equal(outs[0], np.array([[6.1, 6.2, 6.3], [1.1, 1.2, 1.3], [3.1, 3.2, 3.3],
                                                   [6.1, 6.2, 6.3], [4.1, 4.2, 4.3], [6.1, 6.2, 6.3]], F32))
  np.testing.assert_array_equal(outs[1], np.array([[7.1, 7.2], [8.1, 8.2], [5.1, 5.2], [5.1, 5.2], [7.1, 7.2],
                                                   [9.1, 9.2], [2.1, 2.2]], F32))


def test_gather_gradient_golden():
  """distribution_ops_test.py:251-304 with its 888x tiling and its tolerance (rtol 1e-7 * 888)."""
  k = 888
  grads = [np.array([[1.1, 1.2, 1.3], [2.1, 2.2, 2.3], [3.1, 3.2, 3.3], [4.1, 4.2, 4.3], [5.1, 5.2, 5.3],
                     [6.1, 6.2, 6.3]] * k, F32),
           np.array([[1.4, 1.5], [2.4, 2.5], [3.4, 3.5], [4.4, 4.5], [5.4, 5.5], [6.4, 6.5], [7.4, 7.5]] * k, F32)]
  offs = [np.array([13, 0, 5, 13, 8, 13] * k), np.array([16, 18, 11, 11, 16, 20, 3] * k)]
  exp = np.array([2.1, 2.2, 2.3, 7.4, 7.5, 3.1, 3.2, 3.3, 5.1, 5.2, 5.3, 7.8, 8.0, 11.3, 11.6, 11.9,
                  6.8, 7.0, 2.4, 2.5, 6.4, 6.5]) * k
  out = T.gather_grad(22, grads, offs, [3, 2], 1.0)
  assert out.dtype == F32
  np.testing.assert_allclose(out, exp, rtol=1e-7 * k)
  np.testing.assert_allclose(T.gather_grad(22, grads, offs, [3, 2], 0.5), exp * 0.5, rtol=1e-7 * k)


def test_reduce_goldens():
  """distribution_ops_test.py:306-352."""
  idx = np.array([[0], [0], [1]])
  np.testing.assert_array_equal(T.reduce(idx, [[4, 4], [2, 2], [1, 1]], 2, 1), [[3, 3], [1, 1]])
  np.testing.assert_array_equal(T.reduce(idx, [[1, 1], [2, 2], [4, 4]], 2, 0), [[3, 3], [4, 4]])
  np.testing.assert_allclose(T.reduce(idx, [[3, 3], [4, 4], [2, 2]], 2, 2), [[5, 5], [2, 2]])


def test_reduce_empty_outputs_and_skipped_indices():
  vals = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], F32)
  ind = np.array([2, -1, 2, 3])                       # -1 and 3 lie outside [0, 3)
  np.testing.assert_array_equal(T.reduce(ind, vals, 3, 0), [[0, 0], [0, 0], [6, 8]])
  m = T.reduce(ind, vals, 3, 1)
  assert np.isnan(m[:2]).all()                        # 0 * (1 / 0)
  np.testing.assert_array_equal(m[2], [3, 4])
  np.testing.assert_array_equal(T.reduce(ind, vals, 3, 2)[2], np.sqrt(np.array([26, 40], F32)))
  assert T.reduce(np.zeros(0, np.int64), np.zeros((0, 2), F32), 2, 0).tolist() == [[0, 0], [0, 0]]


def test_gather_gradient_chunk_order_by_hand():
  """2^24 + 1 + 1 in fp32: row after row inside one chunk it is (2^24 + 1) + 1 = 2^24 (both additions round
  back to even); with the second and third addend in a later chunk it is 2^24 + (1 + 1) = 2^24 + 2."""
  big = F32(2.0 ** 24)
  grads = [np.array([[big]], F32), np.array([[5.0]], F32), np.array([[1.0]], F32), np.array([[1.0]], F32)]
  offs = [[0], [1], [0], [0]]
  one_chunk = T.gather_grad(2, grads, offs, [1, 1, 1, 1], 1.0)
  np.testing.assert_array_equal(one_chunk, [big, 5.0])
  two_chunks = T.gather_grad(2, grads, offs, [1, 1, 1, 1], 1.0, chunk=2)
  np.testing.assert_array_equal(two_chunks, [big + F32(2.0), 5.0])
  # the product is rounded before it is added: 3 * 0.37f, not 3 * 0.37
  np.testing.assert_array_equal(T.gather_grad(1, [np.array([[3.0]], F32)], [[0]], [1], 0.37),
                                [F32(3.0) * F32(0.37)])


def test_gather_gradient_mixed_widths_by_hand():
  """A row of dim 2 and a row of dim 4 on offset 0: the key is 4 wide, columns 2 and 3 come from the wide row
  alone (the reference adds every element of every row)."""
  grads = [np.array([[1, 2]], F32), np.array([[10, 20, 30, 40], [5, 6, 7, 8]], F32)]
  out = T.gather_grad(9, grads, [[0], [0, 4]], [2, 4], 1.0)
  np.testing.assert_array_equal(out, [11, 22, 30, 40, 5, 6, 7, 8, 0])
  # the same with the wide row first
  out = T.gather_grad(9, grads[::-1], [[0, 4], [0]], [4, 2], 2.0)
  np.testing.assert_array_equal(out, [22, 44, 60, 80, 10, 12, 14, 16, 0])


def test_lookup_gradient_by_hand():
  g = np.array([[1, 2], [3, 4], [5, 6]], F32)
  ids, out = T.lookup_gradient(np.array([[2, 9], [0, 9], [2, 9]]), [7, 8, 9], g)
  np.testing.assert_array_equal(ids, [7, 8, 9])
  np.testing.assert_array_equal(out, [[5, 6], [1, 2], [5, 6]])
