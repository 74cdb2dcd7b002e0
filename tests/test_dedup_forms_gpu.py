"""The list-building dedup and the ops that read its lists at every size edge (-m gpu): ``mhte_unique``,
``mhte_unique_unordered`` (csrc/mhte_kernels.h ``dd_*``), ``mhte_segment_sum`` (``segsum_*``),
``mhte_gather_rows`` and the chunk role of ``sum_apply_kernel`` behind the unpipelined ``SparseStep``.

Expected values come from the plain numpy models of tests/dedup_truth.py, whose batches put a case on each
side of every size constant of these kernels (the table at the top of that file; tests/test_dedup_truth_cpu.py
asserts that they do).  Every output is handed in full of a sentinel and a few elements longer than the call
may write, so an element that was never written, or written past the end, shows.

Bars: ids, counts, numbers, list bounds and positions exactly.  Sums of INTEGER gradients in [-8, 8] exactly,
in either summation order: every partial sum is an integer below 2^24, so every association of the sum has
the same bits and a dropped, doubled or misrouted row cannot hide.  Sums of normal gradients: bit for bit
where the order is the sequential one (``exact_order=True``), else RTOL_TREE / ATOL_SUM of
tests/test_parity_gpu.py (measured and recorded there) against the float64 sum."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dedup_truth as T  # noqa: E402
from monolith_amd import distribution_ops as D, synthetic as S  # noqa: E402
from monolith_amd.fused_step import SparseStep  # noqa: E402
from test_parity_gpu import ATOL_SUM, RTOL_TREE, ids_t, make, sgd_cfg, val_t  # noqa: E402

PAD = 8                              # elements past the end of every output, which must keep the sentinel
SENT_I32 = -7
SENT_I64 = 0x5A5A5A5A5A5A5A5A
SENT_F32 = np.float32(-12345.678)    # no sum of integers, and far from any sum of the normal gradients
SPECIAL = ((0, T.INT64_MIN), (1, 0), (2, T.INT64_MAX))
LAYOUTS = ["runs", "shuffled", "strided"]


# ------------------------------------------------------------------------------------------------- cases
def _cases():
  c = {}
  for n in (1, 2, 33, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049):
    for pattern in ("equal", "distinct", "alternating"):
      c["tiny-%s-%d" % (pattern, n)] = functools.partial(T.tiny_batch, n, pattern)
  for n in T.LADDER_TOTALS:
    for layout in LAYOUTS:
      c["ladder-%s-%d" % (layout, n)] = functools.partial(T.ladder_batch, T.LADDER, n, layout, 21)
  for layout in ("shuffled", "strided"):
    c["heavy300x33-%s" % layout] = functools.partial(T.ladder_batch, [T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N,
                                                     layout, 22)
  c["bitmap-chunks"] = lambda: T.chunk_straddle_batch()[0]
  # INT64_MIN (the reserved key), 0 and INT64_MAX together in one batch
  c["special-min-singleton"] = functools.partial(T.ladder_batch, [1, 5, 40], 2100, "shuffled", 23, SPECIAL)
  c["special-min-list32"] = functools.partial(T.ladder_batch, [32, 33, 3], 2100, "shuffled", 24, SPECIAL)
  c["special-min-strided33"] = functools.partial(T.ladder_batch, [33, 32, 2], 4100, "strided", 25, SPECIAL)
  c["special-min-alone"] = lambda: np.array([T.INT64_MIN], np.int64)
  return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _case(name):
  """(ids, first-occurrence truth) of a case, built once and shared: read-only."""
  ids = CASES[name]()
  ids.setflags(write=False)
  truth = T.unique_first_occurrence(ids)
  for a in truth:
    a.setflags(write=False)
  return ids, truth


# ---------------------------------------------------------------------------------------------- callers
def _i32(n):
  return torch.full((n,), SENT_I32, dtype=torch.int32, device="cuda")


def _result_buffers(n, unordered):
  return D.UniqueResult(torch.full((n + PAD,), SENT_I64, dtype=torch.int64, device="cuda"), _i32(n + PAD),
                        _i32(n + 1 + PAD), _i32(n + PAD), _i32(1), None, _i32(n + 1 + PAD) if unordered else None)


def run_ordered(ws, ids):
  return ws.unique(ids_t(np.array(ids)), want_host_count=True, out=_result_buffers(ids.size, False))


def run_unordered(ws, ids):
  return ws.unique_unordered(ids_t(np.array(ids)), want_host_count=True, out=_result_buffers(ids.size, True))


def _np(t):
  return t.cpu().numpy()


def _split(t, k, what):
  """The first k elements; everything after them must still hold the sentinel."""
  a = _np(t)
  sent = SENT_I64 if a.dtype == np.int64 else SENT_I32
  assert (a[k:] == sent).all(), "%s: written past element %d" % (what, k)
  return a[:k].astype(np.int64)


def check_ordered(r, ids, truth=None):
  """n_unique (host and device word), unique_ids, inverse, seg_off, seg_pos: all equal the truth."""
  n = ids.size
  uids, inverse, seg_off, seg_pos = truth if truth is not None else T.unique_first_occurrence(ids)
  U = uids.size
  assert r.n_unique == U and int(r.n_unique_dev.item()) == U
  if n == 0:
    assert int(_np(r.seg_off)[0]) == 0
    return
  np.testing.assert_array_equal(_split(r.unique_ids, U, "unique_ids"), uids)
  np.testing.assert_array_equal(_split(r.inverse, n, "inverse"), inverse)
  np.testing.assert_array_equal(_split(r.seg_off, U + 1, "seg_off"), seg_off)
  np.testing.assert_array_equal(_split(r.seg_pos, n, "seg_pos"), seg_pos)


def check_unordered(r, ids):
  """Unspecified numbering, so: the same key set, a numbering that maps back to the ids, lists that tile
  [0, n), hold a permutation of the positions, belong to their owner, have the key's multiplicity and — past
  kLightMax entries — ascend.  All lists, vectorised."""
  n = ids.size
  keys, counts = np.unique(ids, return_counts=True)
  U = keys.size
  assert r.n_unique == U and int(r.n_unique_dev.item()) == U
  if n == 0:
    return
  uids = _split(r.unique_ids, U, "unique_ids")
  inverse = _split(r.inverse, n, "inverse")
  start, end = _split(r.seg_off, U, "list_start"), _split(r.list_end, U, "list_end")
  pos = _split(r.seg_pos, n, "seg_pos")
  assert inverse.min() >= 0 and inverse.max() < U
  np.testing.assert_array_equal(uids[inverse], ids)
  np.testing.assert_array_equal(np.sort(uids), keys)
  order = np.argsort(start, kind="stable")
  assert start[order][0] == 0 and end[order][-1] == n and (end > start).all()
  np.testing.assert_array_equal(start[order][1:], end[order][:-1])          # the lists tile [0, n)
  np.testing.assert_array_equal(np.sort(pos), np.arange(n))                  # a permutation of the positions
  lens = end - start
  owner = np.repeat(order, lens[order])                                      # the list that slot q lies in
  np.testing.assert_array_equal(inverse[pos], owner)
  np.testing.assert_array_equal(lens, counts[np.searchsorted(keys, uids)])   # the key's multiplicity
  inside_heavy = (owner[1:] == owner[:-1]) & (lens[owner[1:]] > T.LIGHT_MAX)
  assert (np.diff(pos)[inside_heavy] > 0).all(), "a list of more than 32 positions does not ascend"


# ============================================================================ a. dedup at the size edges
@pytest.mark.parametrize("name", list(CASES))
def test_ordered_dedup_equals_truth(name):
  ids, truth = _case(name)
  check_ordered(run_ordered(D.DedupWorkspace(), ids), ids, truth)


@pytest.mark.parametrize("name", list(CASES))
def test_unordered_dedup_lists(name):
  ids, _ = _case(name)
  ws = D.DedupWorkspace()
  check_unordered(run_unordered(ws, ids), ids)


# ============================================================================ b. one workspace, many calls
def _int_grads(seed, n, dim):
  return np.random.default_rng(seed).integers(-8, 9, size=(n, dim)).astype(np.float32)


def _sums_by_key(ids_list, grads_list):
  """(distinct keys, int64 sum of the gradient rows of each key over all the batches)."""
  ids = np.concatenate(ids_list)
  g = np.concatenate([np.asarray(x).astype(np.int64) for x in grads_list])
  keys, inv = np.unique(ids, return_inverse=True)
  total = np.zeros((keys.size, g.shape[1]), np.int64)
  np.add.at(total, inv.reshape(-1), g)
  return keys, total


def _fused_backward(mt, ws, r, g, n, dim, exact_order=False):
  lrs = np.ascontiguousarray(mt.learning_rate[:1])
  grad_u = torch.full((n, dim), float(SENT_F32), dtype=torch.float32, device="cuda")
  mt.table_sum_optimize_n("emb", ws, r, val_t(g), grad_u, lrs, S.update_time(0), exact_order=exact_order,
                          n_max=n)


def test_one_workspace_alternating_sizes():
  """Ordered and unordered calls of different sizes on ONE workspace: the scratch is cleared once, at its
  largest capacity, and every later call relies on the call before it having left its slots empty
  (clean-after-use) — also where the capacity shrinks (8192 -> 600), for an empty batch, and across the
  capacity switch at 513.  Then the readers of the workspace's own state (``work`` items, ``arrive``
  counters): segment sum and fused backward on the last ordered result, and the fused backward twice more on
  a ladder batch, whose multi-chunk lists count arrivals."""
  dim = 8
  ws = D.DedupWorkspace()
  seq = [("ordered", T.ladder_batch(T.LADDER, 8192, "shuffled", 31)),
         ("unordered", T.ladder_batch([33, 32, 100, 2], 600, "shuffled", 32)),
         ("ordered", np.zeros(0, np.int64)),
         ("unordered", T.ladder_batch(T.LADDER, 8193, "strided", 33)),
         ("ordered", T.ladder_batch([257, 31], 513, "shuffled", 34)),
         ("unordered", T.ladder_batch([T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N, "strided", 35)),
         ("ordered", T.tiny_batch(1, "equal", seed=36))]
  assert [ids.size for _, ids in seq] == [8192, 600, 0, 8193, 513, 9900, 1]
  for form, ids in seq:
    if form == "ordered":
      r = run_ordered(ws, ids)
      check_ordered(r, ids)
    else:
      check_unordered(run_unordered(ws, ids), ids)
  # the last ordered result (n = 1): a stale work item of the 300 heavy lists before it would be applied
  last_ids = seq[-1][1]
  g = _int_grads(37, 1, dim)
  out = torch.full((1 + PAD, dim), float(SENT_F32), dtype=torch.float32, device="cuda")
  ws.segment_sum(val_t(g), r, dim, out=out, exact_order=False)
  np.testing.assert_array_equal(_np(out)[:1], g)
  assert (_np(out)[1:] == SENT_F32).all()
  mt = make({"emb": sgd_cfg(dim)})
  _fused_backward(mt, ws, r, g, 1, dim)
  assert mt.size("emb") == 1
  np.testing.assert_array_equal(_np(mt.lookup({"emb": ids_t(last_ids)})["emb"]), -g)
  # and a batch with multi-chunk lists on the same workspace, twice: the second run counts its arrivals on
  # the counters the first one left
  ids = T.ladder_batch(T.LADDER, 8193, "strided", 38)
  r = run_ordered(ws, ids)
  check_ordered(r, ids)
  g = _int_grads(39, ids.size, dim)
  _fused_backward(mt, ws, r, g, ids.size, dim)
  _fused_backward(mt, ws, r, g, ids.size, dim)
  keys, total = _sums_by_key([last_ids, ids, ids], [_int_grads(37, 1, dim), g, g])
  assert mt.size("emb") == keys.size
  np.testing.assert_array_equal(_np(mt.lookup({"emb": ids_t(keys)})["emb"]), (-total).astype(np.float32))


# ================================================== c. segment sum and gather_rows on every lane shape
VEC4_DIMS = [4, 32, 36, 64, 68, 128, 132, 256, 260, 516]      # G = 8, 8, 16, 16, 32, 32, 64, 64, 64 x 2, 64 x 3
VEC1_DIMS = [1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 130]         # G = 8, 8, 8, 16, 16, 32, 32, 64, 64, 64 x 2, 64 x 3
SHAPES = [(4, d) for d in VEC4_DIMS] + [(1, d) for d in VEC1_DIMS]


def _buf(a, vec, rows_extra=0, fill=None):
  """``a`` [rows, dim] on the device, ``rows_extra`` more rows of ``fill`` behind it.  vec == 4: 16-byte
  aligned.  vec == 1 with a dim that is a multiple of 4: one float into a larger allocation, so that the
  entry point cannot take float4 lanes (any other dim never does)."""
  a = np.ascontiguousarray(a, np.float32)
  rows, dim = a.shape
  mis = vec == 1 and dim % 4 == 0
  flat = torch.empty((rows + rows_extra) * dim + 4, dtype=torch.float32, device="cuda")
  off = 1 if mis else 0
  v = flat[off:off + (rows + rows_extra) * dim].view(rows + rows_extra, dim)
  v[:rows].copy_(torch.from_numpy(a))
  if rows_extra:
    v[rows:] = float(fill)
  assert v.is_contiguous() and v.data_ptr() % 16 == (4 if mis else 0)
  return v


def _sentinel_rows(rows, dim, vec):
  return _buf(np.full((rows, dim), SENT_F32, np.float32), vec)


@functools.lru_cache(maxsize=None)
def _listed(name):
  """(workspace, ordered result on the device, ids, truth) of a segment-sum batch, deduplicated once."""
  if name.startswith("seg-"):
    ids = T.ladder_batch(T.SEG_LADDER, int(name[4:]), "runs", 41)
  else:
    ids = T.ladder_batch(T.LADDER, 8193, "shuffled", 42)
  truth = T.unique_first_occurrence(ids)
  ws = D.DedupWorkspace()
  r = run_ordered(ws, ids)
  check_ordered(r, ids, truth)
  return ws, r, ids, truth


def _segment_sum(name, g, dim, vec, exact_order):
  """Rows [0, U) of the result; rows [U, n + 1) must still hold the sentinel, no row below U may."""
  ws, r, ids, truth = _listed(name)
  n, U = ids.size, truth[0].size
  out = _sentinel_rows(n + 1, dim, vec)
  ws.segment_sum(g, r, dim, out=out, exact_order=exact_order)
  got = _np(out)
  assert (got[U:] == SENT_F32).all(), "a row at or past n_unique was written"
  assert not (got[:U] == SENT_F32).any(), "an element of a row below n_unique was never written"
  return got[:U]


def _check_integer_sums(name, dim, vec, seed):
  _, _, ids, (_, _, seg_off, seg_pos) = _listed(name)
  g = _int_grads(seed, ids.size, dim)
  exp = T.segment_sum_f64(g, seg_off, seg_pos)
  assert np.abs(exp).max() < 2 ** 24
  exp = exp.astype(np.float32)
  g_dev = _buf(g, vec)
  for exact_order in (False, True):
    np.testing.assert_array_equal(_segment_sum(name, g_dev, dim, vec, exact_order), exp,
                                  err_msg="exact_order=%s" % exact_order)


@pytest.mark.parametrize("n", T.SEG_TOTALS)
@pytest.mark.parametrize("vec,dim", SHAPES)
def test_segment_sum_integer_gradients_every_shape(vec, dim, n):
  _check_integer_sums("seg-%d" % n, dim, vec, seed=dim)


@pytest.mark.parametrize("dim", [8, 64, 260])
def test_segment_sum_integer_gradients_interleaved_lists(dim):
  """LADDER, shuffled: the lists are interleaved in the batch and the window bounds fall anywhere."""
  _check_integer_sums("ladder", dim, 4, seed=100 + dim)


@pytest.mark.parametrize("n", T.SEG_TOTALS)
@pytest.mark.parametrize("vec,dim", SHAPES)
def test_segment_sum_normal_gradients_every_shape(vec, dim, n):
  name = "seg-%d" % n
  _, _, _, (_, _, seg_off, seg_pos) = _listed(name)
  g = S.grad_batch(7, n, dim)
  g_dev = _buf(g, vec)
  exact = _segment_sum(name, g_dev, dim, vec, True)
  np.testing.assert_array_equal(exact.view(np.uint32), T.segment_sum_seq32(g, seg_off, seg_pos).view(np.uint32))
  fast = _segment_sum(name, g_dev, dim, vec, False)
  f64 = T.segment_sum_f64(g, seg_off, seg_pos)
  print("dim %d vec %d n %d: |fast - f64| max %.3g (bar %.3g + %.3g |x|)" %
        (dim, vec, n, np.abs(fast - f64).max(), ATOL_SUM, RTOL_TREE))
  np.testing.assert_allclose(fast, f64, rtol=RTOL_TREE, atol=ATOL_SUM)
  again = _segment_sum(name, g_dev, dim, vec, False)
  np.testing.assert_array_equal(fast.view(np.uint32), again.view(np.uint32))   # the same bits run to run


@pytest.mark.parametrize("n", T.SEG_TOTALS)
@pytest.mark.parametrize("vec,dim", SHAPES)
def test_gather_rows_every_shape(vec, dim, n):
  ws, r, ids, (uids, inverse, _, _) = _listed("seg-%d" % n)
  src = np.random.default_rng(dim).standard_normal((uids.size, dim)).astype(np.float32)
  out = _sentinel_rows(n + 1, dim, vec)
  ws.gather_rows(_buf(src, vec), r.inverse, n, dim, out=out)
  got = _np(out)
  np.testing.assert_array_equal(got[:n].view(np.uint32), src[inverse].view(np.uint32))
  assert (got[n:] == SENT_F32).all(), "an element beyond [n, dim] was written"


# ======================================================= d. the fused backward with integer gradients
@pytest.mark.parametrize("exact_order", [False, True])
@pytest.mark.parametrize("dim", [8, 13, 64, 100, 256, 300])
def test_fused_backward_integer_gradients(dim, exact_order):
  """Two unpipelined steps (``forward`` without ``next_ids``: unordered dedup + mhte_table_sum_optimize_n;
  dim 300: the wide-row route over the ordered dedup, segment sum and optimize) on an SGD table, zeros
  initializer, lr 1: a key's row is minus the integer sum of its gradients, whichever way they were added.
  The list lengths 255 .. 2049 are one chunk of kChunk = 256, exactly two, a last chunk of one entry, and
  at G = 64 (dim 256, NG = 4) four chunks (per = 1) and five (per = 2) for the last arriver."""
  n = 8193
  batches = [T.ladder_batch(T.LADDER, n, "shuffled", 51), T.ladder_batch(T.LADDER, n, "strided", 51)]
  grads = [_int_grads(52 + s, n, dim) for s in range(2)]
  keys, total = _sums_by_key(batches, grads)
  assert np.abs(total).max() < 2 ** 24
  mt = make({"emb": sgd_cfg(dim)})
  step = SparseStep(mt, "emb", n, exact_order=exact_order)
  for s in range(2):
    emb = step.forward(ids_t(batches[s]))
    if s == 1:   # the rows the first step left, for every occurrence
      k1, t1 = _sums_by_key(batches[:1], grads[:1])
      np.testing.assert_array_equal(_np(emb), (-t1).astype(np.float32)[np.searchsorted(k1, batches[1])])
    assert step.n_unique() == keys.size
    step.backward(val_t(grads[s]), S.update_time(s))
  assert mt.size("emb") == keys.size
  np.testing.assert_array_equal(_np(mt.lookup({"emb": ids_t(keys)})["emb"]), (-total).astype(np.float32))
