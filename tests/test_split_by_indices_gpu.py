"""GPU suite of the split-by-indices ops (mhte_split_plan / mhte_split_rows / mhte_split_rows_grad,
monolith_amd/distribution_ops.py).  Every comparison is with the numpy truth (tests/split_by_indices_truth.py) on
raw bits: the ops only move and count.  The C ABI cases run on buffers that start as a NaN pattern with guard
words on both sides; the guards must stay intact, the inputs unchanged; the launch counters
(mhte_split_launch_counts) must show the form each case calls for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import split_by_indices_truth as ST  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd._lib import check  # noqa: E402
from monolith_amd.multi_hash_table_ops import Ragged  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8                 # 4-byte words on each side of a buffer
NAN_WORD = 0x7FC0BEEF     # a quiet NaN no computation produces
GUARD_WORD = 0x7FC0CAFE


class Buf:
  """A float32 or int64 array at ``off`` 4-byte words into storage of its own: off 0 is 16-byte aligned, off 1
  has ptr % 16 == 4, off 2 ptr % 16 == 8 (an int64 array the kernels index must be 8-byte aligned).  Payload and
  guards start as NaN patterns."""

  def __init__(self, shape, dtype, off, data=None):
    self.shape, self.dtype = tuple(shape), np.dtype(dtype)
    n = int(np.prod(self.shape, dtype=np.int64)) * (self.dtype.itemsize // 4)
    words = np.full(GUARD + off + n + GUARD, GUARD_WORD, np.uint32)
    words[GUARD + off:GUARD + off + n] = (NAN_WORD if data is None else
                                          np.ascontiguousarray(data, self.dtype).reshape(-1).view(np.uint32))
    self.store = torch.from_numpy(words.view(np.int32)).cuda()
    self.lo, self.n = GUARD + off, n
    self.ptr = self.store.data_ptr() + 4 * self.lo
    assert self.store.data_ptr() % 16 == 0

  def vp(self):
    return C.c_void_p(self.ptr)

  def read(self, what):
    """The payload; the guards must be untouched."""
    words = self.store.cpu().numpy().view(np.uint32)
    assert (words[:self.lo] == GUARD_WORD).all() and (words[self.lo + self.n:] == GUARD_WORD).all(), \
        "%s: a guard word was overwritten" % what
    return words[self.lo:self.lo + self.n].copy().view(self.dtype).reshape(self.shape)


def stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def counts_delta(before):
  after = D.split_launch_counts()
  return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def run_plan(indices, num_splits, row_splits=None, off=0, what=""):
  """mhte_split_plan on guarded buffers against the truth; -> (pos, sizes) as the device wrote them."""
  indices = np.asarray(indices, np.int64)
  n = indices.size
  rs = None if row_splits is None else np.ascontiguousarray(row_splits, np.int64)
  R = 0 if rs is None else rs.size
  d_idx = Buf((n,), np.int64, off, indices)
  d_pos, d_sizes = Buf((n,), np.int64, off), Buf((num_splits,), np.int64, off)
  d_srs, d_bad = Buf((num_splits, R), np.int64, off), Buf((1,), np.int64, off)
  host = np.full(num_splits * (1 + R) + 1, -77, np.int64)
  before = D.split_launch_counts()
  check(_lib.lib().mhte_split_plan(d_idx.vp(), n, num_splits, None if rs is None else rs.ctypes.data_as(C.c_void_p),
                                   R, d_pos.vp(), d_sizes.vp(), d_srs.vp() if R else None, d_bad.vp(),
                                   host.ctypes.data_as(C.c_void_p), stream()))
  ran = counts_delta(before)
  want_pos, want_sizes, want_bad = ST.plan(indices, num_splits)
  pos, sizes = d_pos.read(what + " pos"), d_sizes.read(what + " sizes")
  ST.same_bits(pos, want_pos, what + " pos")
  ST.same_bits(sizes, want_sizes, what + " sizes")
  assert d_bad.read(what + " n_bad").tolist() == [want_bad], what
  ST.same_bits(d_idx.read(what + " indices"), indices, what + " indices")   # only read
  srs = d_srs.read(what + " split_row_splits")
  if R:
    ST.same_bits(srs, ST.split_row_splits(indices, rs, num_splits), what + " split_row_splits")
  ST.same_bits(host, np.concatenate([want_sizes, srs.reshape(-1), [want_bad]]).astype(np.int64), what + " host_out")
  want_ran = {} if n == 0 else ({"plan": 1, "plan/ragged": 1} if R else {"plan": 1})
  assert ran == want_ran, (what, ran)
  return pos, sizes


# every wavefront (64), workgroup (256), wavefront-quarter (1 024) and tile (4 096) boundary of the partition pass
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 7, 16385]
NUM_SPLITS = [1, 2, 3, 8, 64, 65, 1000, 1024]


@pytest.mark.parametrize("num_splits", NUM_SPLITS)
@pytest.mark.parametrize("n", SIZES)
def test_partition_sizes_split_counts_and_patterns(n, num_splits):
  """(num_splits > n is every case with few elements and 1 000 or 1 024 splits.)"""
  for pattern in ST.PATTERNS:
    what = "n=%d num_splits=%d %s" % (n, num_splits, pattern)
    indices = ST.indices_for(pattern, n, num_splits)
    assert indices.size == n and (n == 0 or (0 <= indices.min() and indices.max() < num_splits)), what
    if pattern == "one empty" and num_splits > 1 and n:
      assert not (indices == num_splits // 2).any()
    run_plan(indices, num_splits, what=what)


def test_int64_buffers_at_an_8_byte_offset():
  run_plan(ST.indices_for("uniform", 4097, 65), 65, row_splits=[0, 5, 5, 4097], off=2, what="off=2")


def test_same_call_twice_gives_identical_pos():
  indices = ST.indices_for("uniform", 3 * 4096 + 7, 64)
  a, _ = run_plan(indices, 64, what="first")
  b, _ = run_plan(indices, 64, what="second")
  ST.same_bits(a, b, "determinism")


# ---- ragged boundaries --------------------------------------------------------------------------------------
def _row_splits(T, n, where):
  """T rows over n elements with empty rows at ``where`` (front / middle / end / all)."""
  if where == "all":
    assert n == 0
    return np.zeros(T + 1, np.int64)
  rng = np.random.RandomState(T + n)
  empty = {"front": {0}, "middle": {T // 2}, "end": {T - 1}}[where] if T > 1 else set()
  lens = np.array([0 if t in empty else 1 + rng.randint(0, 50) for t in range(T)], np.float64)
  cuts = np.floor(np.cumsum(lens) / lens.sum() * n).astype(np.int64)
  cuts[-1] = n
  rs = np.concatenate([[0], cuts])
  for t in empty:
    assert rs[t + 1] == rs[t]
  return rs


@pytest.mark.parametrize("where", ["front", "middle", "end", "all"])
@pytest.mark.parametrize("T", [1, 4, 26])
def test_ragged_boundaries(T, where):
  # ("all": an input without elements — every row of every split is empty)
  for n, num_splits in ((0, 1), (0, 3), (0, 1000)) if where == "all" else \
      ((257, 2), (4097, 8), (4097, 65), (16385, 1024)):
    rs = _row_splits(T, n, where)
    what = "T=%d %s n=%d num_splits=%d" % (T, where, n, num_splits)
    run_plan(ST.indices_for("uniform", n, num_splits), num_splits, row_splits=rs, what=what)


def test_invalid_row_splits_are_refused():
  idx = torch.zeros(4, dtype=torch.int64, device="cuda")
  for rs in ([0, 3], [1, 4], [0, 3, 2, 4]):
    with pytest.raises(_lib.InvalidArgumentError, match="The input ragged tensor is invalid."):
      D.ragged_split_by_indices(idx, Ragged(idx, np.array(rs, np.int64)), 2)
    with pytest.raises(_lib.InvalidArgumentError, match="The input ragged tensor is invalid."):
      D.split_plan(idx, 2, rs)
  with pytest.raises(_lib.InvalidArgumentError, match="Ragged tensor values size must match indices size"):
    D.ragged_split_by_indices(idx, Ragged(idx[:3], np.array([0, 3], np.int64)), 2)


# ---- the row movers -----------------------------------------------------------------------------------------
MOVER_CASES = [(np.float32, e) for e in (1, 2, 3, 4, 16, 17, 64)] + [(np.int64, e) for e in (1, 2)]
OFFS = pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4 bytes in"])


def mover_forms(dtype, element_size, off):
  v = ST.mover_form(np.dtype(dtype).itemsize, element_size, off == 0)
  return {"rows/" + v: 1, "gradient/" + v: 1}


@OFFS
@pytest.mark.parametrize("case", MOVER_CASES, ids=lambda c: "%s-e%d" % (np.dtype(c[0]).name, c[1]))
def test_row_movers(case, off):
  dtype, e = case
  n, num_splits = 1025, 5
  what = "%s e=%d off=%d" % (np.dtype(dtype).name, e, off)
  rng = np.random.RandomState(e + off)
  indices = ST.indices_for("one empty", n, num_splits)
  indices[::97] = -1   # some rows belong to no split: they move nowhere
  pos, sizes, n_bad = ST.plan(indices, num_splits)
  placed = n - n_bad
  data = rng.randint(-2 ** 31, 2 ** 31, size=(n, e)).astype(np.int64)
  data = data.astype(np.int32).view(np.float32) if dtype == np.float32 else data * 2 ** 31 + 5   # any bits: NaNs too
  d_in, d_pos, d_out = Buf((n, e), dtype, off, data), Buf((n,), np.int64, 0, pos), Buf((n, e), dtype, off)
  before = D.split_launch_counts()
  esz = np.dtype(dtype).itemsize
  check(_lib.lib().mhte_split_rows(d_in.vp(), n, e, esz, d_pos.vp(), d_out.vp(), stream()))
  got = d_out.read(what + " packed")
  ST.same_bits(got[:placed], data[pos[:placed]], what + " packed")
  assert (ST.bits(got[placed:]).view(np.uint32) == NAN_WORD).all(), what + ": a row behind the last was written"
  ST.same_bits(d_in.read(what), data, what + " input")
  # the gradient: one buffer per split, rows of any bits
  grads = [rng.randint(-2 ** 31, 2 ** 31, size=(int(s), e)).astype(np.int64) for s in sizes]
  grads = [g.astype(np.int32).view(np.float32) if dtype == np.float32 else g * 2 ** 31 + 3 for g in grads]
  d_g = [Buf(g.shape, dtype, off, g) for g in grads]
  d_sizes, d_ig = Buf((num_splits,), np.int64, 0, sizes), Buf((n, e), dtype, off)
  tab = (C.c_void_p * num_splits)(*[b.ptr for b in d_g])
  check(_lib.lib().mhte_split_rows_grad(tab, d_sizes.vp(), num_splits, n, e, esz, d_pos.vp(), d_ig.vp(), stream()))
  assert counts_delta(before) == mover_forms(dtype, e, off), what
  got = d_ig.read(what + " input_grads")
  good = (indices >= 0)
  want = ST.gradient(np.where(good, indices, 0)[good], grads, (int(good.sum()), e))
  ST.same_bits(got[good], want, what + " input_grads")
  assert (ST.bits(got[~good]).view(np.uint32) == NAN_WORD).all(), what + ": a row of no split was written"
  for b, g in zip(d_g, grads):
    ST.same_bits(b.read(what), g, what + " grads")


def test_every_mover_form_is_reached_by_a_case():
  reached = {"plan", "plan/ragged"}   # (test_partition_*, test_ragged_boundaries: run_plan asserts them)
  for dtype, e in MOVER_CASES:
    for off in (0, 1):
      reached.update(mover_forms(dtype, e, off))
  assert reached == set(ST.COUNTERS)


# ---- errors -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_splits", [1, 3, 1024])
def test_out_of_range_indices_are_counted_and_left_out(num_splits):
  n = 4097
  indices = ST.indices_for("uniform", n, num_splits)
  indices[5::11] = -1
  indices[7::13] = num_splits
  indices[0] = -2 ** 63
  indices[n - 1] = 2 ** 63 - 1
  indices[100] = 2 ** 32          # (its low 32 bits are a valid split)
  indices[101] = 2 ** 32 + num_splits - 1
  pos, sizes = run_plan(indices, num_splits, row_splits=[0, 100, 100, n], what="bad indices")
  good = (indices >= 0) & (indices < num_splits)
  assert sizes.sum() == good.sum() and (pos[int(good.sum()):] == -1).all()
  dev = torch.from_numpy(indices).cuda()
  with pytest.raises(_lib.InvalidArgumentError, match="indices are outside"):
    D.split_by_indices(dev, dev.clone(), num_splits)
  with pytest.raises(_lib.InvalidArgumentError, match="indices are outside"):
    D.ragged_split_by_indices(dev, Ragged(dev.clone(), np.array([0, n], np.int64)), num_splits)
  plan = D.split_plan(dev, num_splits)   # the no-synchronise form reports it on the device
  assert int(plan.n_bad.item()) == int((~good).sum())


def test_bad_split_counts_are_refused():
  dev = torch.zeros(4, dtype=torch.int64, device="cuda")
  for bad in (0, 1025):
    with pytest.raises(_lib.InvalidArgumentError, match="num_splits must be in"):
      D.split_by_indices(dev, dev, bad)


# ---- the Python ops -----------------------------------------------------------------------------------------
def test_reference_examples_through_the_python_ops():
  ids = torch.tensor([0, 1, 2, 2, 3], dtype=torch.int64, device="cuda")
  splits = D.split_by_indices(torch.remainder(ids, 3), ids, 3)
  assert [s.tolist() for s in splits] == [[0, 3], [1], [2, 2]]
  assert len({s.untyped_storage().data_ptr() for s in splits}) == 1   # views of one packed buffer
  # gradient (all ones) and the empty gradient
  indices = torch.tensor([0, 1, 0], dtype=torch.int64, device="cuda")
  tensor = torch.tensor([[0, 0], [1, 1], [2, 2]], dtype=torch.float32, device="cuda", requires_grad=True)
  splits = D.split_by_indices(indices, tensor, 3)
  assert [tuple(s.shape) for s in splits] == [(2, 2), (1, 2), (0, 2)]
  grad, = torch.autograd.grad([s.sum() for s in splits], tensor)
  assert grad.tolist() == [[1, 1], [1, 1], [1, 1]]
  empty = torch.zeros(0, dtype=torch.float32, device="cuda", requires_grad=True)
  splits = D.split_by_indices(torch.zeros(0, dtype=torch.int64, device="cuda"), empty, 3)
  assert [tuple(s.shape) for s in splits] == [(0,)] * 3
  grad, = torch.autograd.grad(sum(s.sum() for s in splits), empty)
  assert grad.tolist() == []
  # ragged: six rows of which four are empty, then the docstring's example
  indices = torch.tensor([0, 1, 0, 1], dtype=torch.int64, device="cuda")
  values = torch.tensor([4, 3, 2, 1], dtype=torch.int64, device="cuda")
  for rs in ([0, 0, 0, 3, 4, 4, 4], [0, 3, 4]):
    splits, pos = D.ragged_split_by_indices(indices, Ragged(values, np.array(rs, np.int64)), 2)
    want_s, want_p = ST.ragged_split([0, 1, 0, 1], [4, 3, 2, 1], rs, 2)
    for got, want in ((splits, want_s), (pos, want_p)):
      for g, (wv, wr) in zip(got, want):
        assert g.values.dtype == torch.int64 and g.values.is_cuda and isinstance(g.row_splits, np.ndarray)
        ST.same_bits(g.values.cpu().numpy(), wv)
        ST.same_bits(g.row_splits, wr)
  assert [ST.to_lists(s.values.cpu().numpy(), s.row_splits) for s in splits] == [[[4, 2], []], [[3], [1]]]
  assert [ST.to_lists(p.values.cpu().numpy(), p.row_splits) for p in pos] == [[[0, 2], []], [[1], [3]]]


@pytest.mark.parametrize("shape", [(4097,), (4097, 3), (1000, 2, 4)], ids=str)
def test_autograd_backward_equals_the_truth(shape):
  n, num_splits = shape[0], 7
  rng = np.random.RandomState(len(shape))
  indices = ST.indices_for("one empty", n, num_splits)
  data = rng.standard_normal(shape).astype(np.float32)
  tensor = torch.from_numpy(data).cuda().requires_grad_(True)
  splits = D.split_by_indices(torch.from_numpy(indices).cuda(), tensor, num_splits)
  want = ST.split(indices, data, num_splits)
  for g, w in zip(splits, want):
    ST.same_bits(g.detach().cpu().numpy(), w, "forward %s" % (shape,))
  ups = [rng.standard_normal(w.shape).astype(np.float32) for w in want]
  torch.autograd.backward(splits, [torch.from_numpy(u).cuda() for u in ups])
  ST.same_bits(tensor.grad.cpu().numpy(), ST.gradient(indices, ups, shape), "backward %s" % (shape,))
  # int64 takes the same mover and is not differentiable
  ints = torch.from_numpy(indices * 3 - 1).cuda()
  for g, w in zip(D.split_by_indices(torch.from_numpy(indices).cuda(), ints, num_splits),
                  ST.split(indices, indices * 3 - 1, num_splits)):
    ST.same_bits(g.cpu().numpy(), w, "int64")


def test_split_plan_stays_on_the_device():
  indices = ST.indices_for("uniform", 4097, 8)
  rs = np.array([0, 0, 1000, 4097, 4097], np.int64)
  plan = D.split_plan(torch.from_numpy(indices).cuda(), 8, rs)
  want_pos, want_sizes, _ = ST.plan(indices, 8)
  assert all(t.is_cuda and t.dtype == torch.int64 for t in plan)
  ST.same_bits(plan.pos.cpu().numpy(), want_pos)
  ST.same_bits(plan.sizes.cpu().numpy(), want_sizes)
  ST.same_bits(plan.split_row_splits.cpu().numpy(), ST.split_row_splits(indices, rs, 8))
  assert plan.n_bad.tolist() == [0]
  assert D.split_plan(torch.from_numpy(indices).cuda(), 8).split_row_splits is None
