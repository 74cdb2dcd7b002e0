"""The numpy models of tests/dedup_truth.py against the project's independent CPU oracle (oracle/), and the
coverage conditions of the batches tests/test_dedup_forms_gpu.py runs: a failure in the second half means the
INPUTS no longer reach a kernel branch, not that a kernel is wrong.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dedup_truth as T  # noqa: E402
import oracle as O  # noqa: E402

LAYOUTS = ["runs", "shuffled", "strided"]
F32 = np.float32


def _counts_by_key(ids):
  keys, counts = np.unique(ids, return_counts=True)
  return dict(zip(keys.tolist(), counts.tolist()))


# ------------------------------------------------------------------------------ the truth against the oracle
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lengths,n", [(T.LADDER, 8193), (T.SEG_LADDER, T.SEG_TOTALS[1]),
                                       ([T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N)])
def test_unique_first_occurrence_equals_oracle(lengths, n, layout):
  ids = T.ladder_batch(lengths, n, layout, seed=3, special=((2, T.INT64_MIN), (3, 0), (4, T.INT64_MAX)))
  uids, inverse, seg_off, seg_pos = T.unique_first_occurrence(ids)
  uk, uks, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, n], [1])
  np.testing.assert_array_equal(uids, uk)
  assert uks.tolist() == [0, uids.size]
  np.testing.assert_array_equal(seg_off, vos)       # list splits
  np.testing.assert_array_equal(seg_pos, vo)        # offsets (dim 1: the positions themselves)
  np.testing.assert_array_equal(uids[inverse], ids)
  if layout == "runs":                              # CSR order is batch order, bounds are the prefix sums
    np.testing.assert_array_equal(seg_pos, np.arange(n))
    np.testing.assert_array_equal(seg_off[:len(lengths) + 1], np.concatenate([[0], np.cumsum(lengths)]))


def test_unique_first_occurrence_by_hand():
  uids, inverse, seg_off, seg_pos = T.unique_first_occurrence([7, -3, 7, 7, T.INT64_MIN, -3])
  assert uids.tolist() == [7, -3, T.INT64_MIN]
  assert inverse.tolist() == [0, 1, 0, 0, 2, 1]
  assert seg_off.tolist() == [0, 3, 5, 6]
  assert seg_pos.tolist() == [0, 2, 3, 1, 5, 4]
  assert [a.size for a in T.unique_first_occurrence(np.zeros(0, np.int64))] == [0, 0, 1, 0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", [1, 7, 64])
def test_segment_sum_seq32_equals_oracle_bit_for_bit(dim, layout):
  n = 8193
  ids = T.ladder_batch(T.LADDER, n, layout, seed=4)
  g = np.random.default_rng(dim).standard_normal((n, dim)).astype(F32)
  uids, _, seg_off, seg_pos = T.unique_first_occurrence(ids)
  U = uids.size
  _, _, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, n], [dim])
  exp = O.fill_with_offset_map_gradient(np.arange(U), [0, U], g.ravel(), vo, vos, [dim]).reshape(U, dim)
  got = T.segment_sum_seq32(g, seg_off, seg_pos)
  assert got.dtype == F32
  np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
  # the float64 sum is the same sum: it differs from the sequential float32 one by rounding alone
  f64 = T.segment_sum_f64(g, seg_off, seg_pos)
  bound = np.add.reduceat(np.abs(g.astype(np.float64))[seg_pos], seg_off[:-1], axis=0)
  lens = np.diff(seg_off)[:, None]
  assert np.all(np.abs(got - f64) <= lens * 2.0 ** -24 * bound + 1e-30)


def test_segment_sum_seq32_order_by_hand():
  """2^24 + 1 + 1 in float32 is 2^24 one addition after the other (both round back to even), 2^24 + 2 in
  any other association."""
  big = F32(2.0 ** 24)
  g = np.array([[1.0], [big], [1.0], [5.0]], F32)
  out = T.segment_sum_seq32(g, [0, 3, 4], [1, 0, 2, 3])
  np.testing.assert_array_equal(out, [[big], [5.0]])
  np.testing.assert_array_equal(T.segment_sum_f64(g, [0, 3, 4], [1, 0, 2, 3]), [[2.0 ** 24 + 2], [5.0]])


# ------------------------------------------------------------------------------------ coverage conditions
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("lengths,n", [(T.LADDER, t) for t in T.LADDER_TOTALS] +
                         [(T.SEG_LADDER, t) for t in T.SEG_TOTALS] +
                         [([T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N)])
def test_ladder_batch_multiplicities(lengths, n, layout):
  ids = T.ladder_batch(lengths, n, layout, seed=9)
  assert ids.dtype == np.int64 and ids.shape == (n,)
  counts = np.sort(np.unique(ids, return_counts=True)[1])
  np.testing.assert_array_equal(counts, np.sort(list(lengths) + [1] * (n - sum(lengths))))
  assert (ids < 0).any() and (ids > 0).any()
  # the same seed gives the same keys in every layout, key k with lengths[k] occurrences
  runs = T.ladder_batch(lengths, n, "runs", seed=9)
  by_key = _counts_by_key(ids)
  off = 0
  for length in lengths:
    assert by_key[int(runs[off])] == length
    off += length


def test_ladder_batch_special_ids():
  special = ((0, T.INT64_MIN), (1, 0), (2, T.INT64_MAX))
  for layout in LAYOUTS:
    by_key = _counts_by_key(T.ladder_batch([33, 32, 2], 4100, layout, seed=1, special=special))
    assert (by_key[T.INT64_MIN], by_key[0], by_key[T.INT64_MAX]) == (33, 32, 2)
    assert len(by_key) == 3 + 4100 - 67


@pytest.mark.parametrize("lengths,n", [(T.LADDER, t) for t in T.LADDER_TOTALS] +
                         [([T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N), ([33, 32, 2], 4100)])
def test_strided_reaches_every_block(lengths, n):
  """Every key of length >= 8 lies in min(len, nblocks) distinct 1024-blocks.  The one exception is
  arithmetic: the last block of n = 8193 has ONE position, so one key can reach it — there the longest keys
  get the last block's positions and every other key reaches all the blocks before it."""
  ids = T.ladder_batch(lengths, n, "strided", seed=9)
  runs = T.ladder_batch(lengths, n, "runs", seed=9)
  nblocks = (n + T.BLOCK - 1) // T.BLOCK
  last_cap = n - T.BLOCK * (nblocks - 1)
  long_keys = [length for length in lengths if length >= 8]
  rank_by_len = np.argsort(np.argsort(-np.asarray(lengths), kind="stable"), kind="stable")
  off = 0
  for k, length in enumerate(lengths):
    blocks = np.unique(np.flatnonzero(ids == runs[off]) // T.BLOCK)
    off += length
    if length < 8:
      continue
    reachable = nblocks if (last_cap >= len(long_keys) or rank_by_len[k] < last_cap) else nblocks - 1
    assert blocks.size >= min(length, reachable), (k, length, blocks.size)


@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_seg_ladder_reaches_every_window_class(G):
  seen = []
  for n in T.SEG_TOTALS:
    assert n < 16384
    ids = T.ladder_batch(T.SEG_LADDER, n, "runs", seed=2)
    _, _, seg_off, seg_pos = T.unique_first_occurrence(ids)
    np.testing.assert_array_equal(seg_pos, np.arange(n))
    classes = T.classify_windows(seg_off, n, G)
    assert set("abcdefgh") <= classes, (G, n, sorted(set("abcdefgh") - classes))
    seen.append(classes)
  assert "j" in seen[0] and "i" in seen[1]


def test_classify_windows_by_hand():
  # WIN = 16, NG = 16: [0,16) inside, [16,48) on both bounds, [48,53) inside, [53,69) mid to mid, [69,72),
  # [72,112) from mid-window over two whole windows to a bound
  off = np.concatenate([[0], np.cumsum([16, 32, 5, 16, 3, 40])])
  assert T.classify_windows(off, 112, 16) == set("abcdej")
  assert T.classify_windows(off[:2], 16, 16) == set("aj")
  assert T.classify_windows([0, 5, 16 * 17 + 3], 16 * 17 + 3, 16) == set("aefi")       # 18 windows > NG = 16
  assert T.classify_windows([0, 8 * 16 * 16 + 1], 8 * 16 * 16 + 1, 16) == set("efgi")  # per = 9
  assert T.classify_windows([0, 16 * 16 * 16 + 1], 16 * 16 * 16 + 1, 16) == set("efghi")


def test_chunk_batch_straddles_the_bitmap_chunk():
  ids, (straddle, second, first) = T.chunk_straddle_batch()
  n = T.CHUNK_N
  assert ids.shape == (n,) and n > T.BM_BITS
  pos = np.flatnonzero(ids == straddle)
  assert pos.size == T.CHUNK_LEN and T.BM_BITS - 1 in pos and T.BM_BITS in pos
  assert (pos < T.BM_BITS - 1).any() and (pos > T.BM_BITS).any()
  pos = np.flatnonzero(ids == second)
  assert pos.size == T.CHUNK_LEN and pos.min() >= T.BM_BITS
  pos = np.flatnonzero(ids == first)
  assert pos.size == T.CHUNK_LEN and pos.max() < T.BM_BITS
  counts = np.unique(ids, return_counts=True)[1]
  assert (counts == T.CHUNK_LEN).sum() == T.CHUNK_KEYS
  assert (counts == 1).sum() == n - T.CHUNK_KEYS * T.CHUNK_LEN
  assert (counts > T.LIGHT_MAX).sum() > 256      # more heavy lists than heavy workgroups here as well


@pytest.mark.parametrize("layout", ["shuffled", "strided"])
def test_heavy_batch_has_the_maximal_heavy_count(layout):
  ids = T.ladder_batch([T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N, layout, seed=6)
  counts = np.unique(ids, return_counts=True)[1]
  assert ids.size == T.HEAVY_N == 9900
  assert (counts > T.LIGHT_MAX).sum() == T.HEAVY_N // (T.LIGHT_MAX + 1) == 300 > 256


@pytest.mark.parametrize("pattern", ["equal", "distinct", "alternating"])
def test_tiny_batches(pattern):
  for n in (1, 2, 33, 512, 513, 2049):
    ids = T.tiny_batch(n, pattern)
    want = {"equal": 1, "distinct": n, "alternating": min(n, 2)}[pattern]
    assert ids.shape == (n,) and np.unique(ids).size == want
    if pattern == "alternating" and n > 2:
      assert ids[0] == ids[2] != ids[1]
