"""Every kernel form of the ops that follow the embedding exchange (-m gpu): the gather per merged slot, its
gradient with a host and a device scale, the ragged reductions, the grouping sort behind the gradient and
the unsorted reduce, and the lookup gradient (csrc/mhte_pool_kernels.h, csrc/mhte_group_kernels.h,
``fused_gather<>`` / ``mhte_reduce_rows`` / ``mhte_lookup_gradient`` in csrc/mhte.hip).

The expected values come from the plain numpy models of tests/post_exchange_truth.py.  Every comparison is
bit for bit (``view(np.uint32)``); the one exception is the NaN of an empty mean, whose sign and payload are
no part of the contract (x86 gives 0 * inf the sign bit, the GPU does not): NaNs must sit in the same places.
Every output buffer is handed in full of NaN through the C ABI, so a float the call leaves out shows.

Preconditions the cases keep:
  * gather gradient: two rows either share an offset or their ranges [offset, offset + dim) are disjoint
    (overlapping ranges would have two lane groups own the same floats: a race, not tested), and every range
    lies inside the fused buffer;
  * reductions: an index outside [0, batch) goes to the two default forms only (the sort maps it to its
    `limit` key or the list kernel returns on it; the sorted kernel only compares) — never to the
    float-atomic form (MHTE_POOL_ATOMICS=1), which uses the index as an address unchecked.

Sizes are the smallest that select the branch: about 3 000 rows per gather input (lists of 1, 2, 3, 4, 5 and
600 addends per launch), 40 inputs of 200 rows for the chunks of 32, batch 37 for the reductions (16 lane
groups per workgroup: three workgroups, the last one partial)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import post_exchange_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd.multi_hash_table_ops import _stream  # noqa: E402
from test_alignment_forms_gpu import _al  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = np.float32(0.37)
NAN = float("nan")


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, exp, what=""):
  """Bit for bit; NaNs in the same places."""
  got, exp = np.asarray(got), np.asarray(exp, dtype=np.float32)
  assert got.dtype == np.float32 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
  nan = np.isnan(exp)
  np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + " (NaN places)")
  np.testing.assert_array_equal(_bits(np.where(nan, np.float32(0), got)), _bits(np.where(nan, np.float32(0), exp)),
                                err_msg=what)


def _nan(*shape):
  return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _ptrs(tensors):
  return (C.c_void_p * max(len(tensors), 1))(*[C.c_void_p(t.data_ptr()) for t in tensors])


def _i32(offs):
  return [torch.from_numpy(np.ascontiguousarray(o, dtype=np.int32)).cuda() for o in offs]


# ------------------------------------------------------------------------------------------ raw callers
def raw_gather(fused, offs, dims):
  """mhte_fused_gather_embeddings_by_input into outputs that hold NaN."""
  fused_t, offs_t = _al(fused), _i32(offs)
  outs = [_nan(int(o.numel()), int(d)) for o, d in zip(offs_t, dims)]
  n = (C.c_int64 * max(len(dims), 1))(*[o.numel() for o in offs_t])
  dm = (C.c_int32 * max(len(dims), 1))(*[int(d) for d in dims])
  _lib.check(_lib.lib().mhte_fused_gather_embeddings_by_input(_lib.vp(fused_t), len(dims), _ptrs(offs_t), n, dm,
                                                              _ptrs(outs), _stream()))
  return [o.cpu().numpy() for o in outs]


def raw_gather_grad(fused_len, grads, offs, dims, scale=SCALE, device_scale=False):
  """mhte_fused_gather_embeddings_by_input_gradient[_dev_scale] into a buffer that holds NaN."""
  offs_t = _i32(offs)
  grads_t = [_al(np.asarray(g, np.float32).reshape(-1, int(d))) for g, d in zip(grads, dims)]
  out = _nan(int(fused_len))
  n = (C.c_int64 * max(len(dims), 1))(*[o.numel() for o in offs_t])
  dm = (C.c_int32 * max(len(dims), 1))(*[int(d) for d in dims])
  L = _lib.lib()
  if device_scale:
    sc = torch.tensor(float(scale), dtype=torch.float32, device="cuda")
    _lib.check(L.mhte_fused_gather_embeddings_by_input_gradient_dev_scale(
        _lib.vp(out), int(fused_len), len(dims), _ptrs(grads_t), _ptrs(offs_t), n, dm, _lib.vp(sc), _stream()))
  else:
    _lib.check(L.mhte_fused_gather_embeddings_by_input_gradient(
        _lib.vp(out), int(fused_len), len(dims), _ptrs(grads_t), _ptrs(offs_t), n, dm, float(scale), _stream()))
  return out.cpu().numpy()


def raw_reduce(ind, vals, batch, mode, sorted_):
  vals = np.array(vals, dtype=np.float32)       # (copies: a shared case is read-only)
  idx = torch.from_numpy(np.array(ind, dtype=np.int64)).cuda()
  v = _al(vals)
  out = _nan(int(batch), vals.shape[1])
  _lib.check(_lib.lib().mhte_reduce_rows(_lib.vp(idx), _lib.vp(v), idx.numel(), vals.shape[1], int(batch), mode,
                                         1 if sorted_ else 0, _lib.vp(out), _stream()))
  return out.cpu().numpy()


def raw_lookup_gradient(idx, ids, g):
  idx_t = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
  ids_t = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).cuda()
  g_t = _al(g)
  n, dim = int(ids_t.numel()), int(g_t.shape[1])
  out_ids = torch.full((n,), -1, dtype=torch.int64, device="cuda")
  out = _nan(n, dim)
  _lib.check(_lib.lib().mhte_lookup_gradient(_lib.vp(idx_t), n, idx_t.shape[1], _lib.vp(ids_t), _lib.vp(g_t),
                                             g_t.shape[0], dim, _lib.vp(out_ids), _lib.vp(out), _stream()))
  return out_ids.cpu().numpy(), out.cpu().numpy()


# ----------------------------------------------------------------------------------------- gather cases
def _slots_with_lists(rng, n, long=600):
  """A slot number per row: one slot with ``long`` rows, two each with 2, 3, 4 and 5 rows, every other row a
  slot of its own; then the rows are shuffled, so that the rows of a list are not neighbours."""
  sizes = [long] + [2, 3, 4, 5] * 2
  sizes += [1] * (n - sum(sizes))
  slot = np.repeat(np.arange(len(sizes)), sizes)
  return slot[rng.permutation(n)], len(sizes)


def _check_gather_both_ways(fused_len, offs, dims, seed, device_scale, what):
  """Forward against numpy indexing, gradient against the sequential model, at scale 0.37 from the host
  and (``device_scale``) from a device word: the same bits."""
  rng = np.random.default_rng(seed)
  fused = rng.standard_normal(fused_len).astype(np.float32)
  for got, exp in zip(raw_gather(fused, offs, dims), T.gather(fused, offs, dims)):
    _same(got, exp, what + ": forward")
  grads = [rng.standard_normal((len(o), d)).astype(np.float32) for o, d in zip(offs, dims)]
  exp = T.gather_grad(fused_len, grads, offs, dims, SCALE)
  host = raw_gather_grad(fused_len, grads, offs, dims)
  _same(host, exp, what + ": gradient, host scale")
  if device_scale:
    _same(raw_gather_grad(fused_len, grads, offs, dims, device_scale=True), host, what + ": gradient, device scale")


@pytest.mark.parametrize("dims,device_scale", [
    ([16, 32, 64], True),            # float4, one trip; 64 is the widest single addend of the fast path
    ([64, 68, 132, 260], False),     # float4: a single addend wider than the lane group, second and fifth trip
    ([1, 9, 13, 33], False),         # scalar, second and fifth trip of 8 lanes
    ([8, 6], False),                 # one dim that is no multiple of 4 sends the whole launch scalar
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else ("dev" if v else "host"))
def test_gather_widths(dims, device_scale):
  rng = np.random.default_rng(31)
  base, offs = 0, []
  for d in dims:
    slot, n_slots = _slots_with_lists(rng, 3000)
    offs.append(base + slot * 2 * d)          # (every second slot of the buffer: nothing points at the others)
    base += n_slots * 2 * d
  _check_gather_both_ways(base, offs, dims, 32, device_scale, "dims %s" % dims)


def test_gather_unaligned_destinations_with_float4_dims():
  """Dims [4, 8] and 16-byte aligned buffers select the float4 kernels; a third of the destinations start 1, 2
  or 3 floats into their slot: the `o & 3` branch of the gradient (single addends and lists), and in the
  forward the scalar rows inside an `aligned` launch beside float4 rows."""
  rng = np.random.default_rng(33)
  dims = [4, 8]
  base, offs = 0, []
  for d in dims:
    slot, n_slots = _slots_with_lists(rng, 3000)
    shift = np.where(np.arange(n_slots) % 3 == 0, 1 + (np.arange(n_slots) // 3) % 3, 0)   # per slot: 1 2 3 or 0
    shift[0] = 2                              # the list of 600
    shift[1:9] = [0, 1, 0, 2, 3, 0, 1, 0]     # the lists of 2 .. 5: both kinds
    offs.append(base + slot * (d + 4) + shift[slot])
    base += n_slots * (d + 4)
  assert all((np.asarray(o) % 4 != 0).sum() > len(o) // 4 for o in offs)
  _check_gather_both_ways(base, offs, dims, 34, True, "unaligned destinations")


@pytest.mark.parametrize("cycle", [(4, 8, 16), (3, 4, 8)], ids=["float4", "scalar"])
def test_gather_40_inputs_in_chunks_of_32_and_8(cycle):
  """Inputs 32 .. 39 go out in a second launch: its tables are indexed from input 32 on, and its gradient
  launch must read the destinations the first one wrote (`fresh` = 0).  Input i >= 32 shares offsets with
  input i - 33 (input 32: input 2), which has the same dim; the rest of its rows lie in a region of its own,
  written by the second chunk only."""
  rng = np.random.default_rng(35)
  dims = [cycle[i % 3] for i in range(40)]
  n, slots = 200, 120
  region, base = [], 0
  for d in dims:
    region.append(base)
    base += slots * d
  offs = [region[i] + rng.integers(0, slots, n) * dims[i] for i in range(40)]
  for i in range(32, 40):
    p = i - 33 if i > 32 else 2
    assert dims[p] == dims[i]
    offs[i][::2] = rng.choice(offs[p], n // 2)              # shared with the first chunk
    offs[i][1] = region[p] + slots * dims[p] - dims[p]      # (the partner's last slot, used or not)
  _check_gather_both_ways(base, offs, dims, 36, True, "40 inputs")
  # the chunks are what makes this case: the same rows as ONE chunk add up in another order
  grads = [np.random.default_rng(36 + i).standard_normal((n, d)).astype(np.float32) for i, d in enumerate(dims)]
  assert not np.array_equal(_bits(T.gather_grad(base, grads, offs, dims, SCALE)),
                            _bits(T.gather_grad(base, grads, offs, dims, SCALE, chunk=64)))


@pytest.mark.parametrize("dims", [[4, 8, 16, 8, 4], [3, 8, 4, 8, 5]], ids=["float4", "scalar"])
def test_gather_empty_inputs(dims):
  """Inputs 0, 2 and 4 of five without rows (first, middle, last in the `start[]` searches); then all five
  empty; a fused buffer most of which nothing points at."""
  rng = np.random.default_rng(37)
  fused_len = 50000
  offs, base = [], 0
  for i, d in enumerate(dims):
    n = 0 if i % 2 == 0 else 700
    offs.append(base + rng.integers(0, 40, n) * d)
    base += 40 * d
  _check_gather_both_ways(fused_len, offs, dims, 38, False, "inputs 0, 2, 4 empty")
  none = [np.zeros(0, np.int64)] * 5
  got = raw_gather_grad(fused_len, [np.zeros((0, d), np.float32) for d in dims], none, dims)
  _same(got, np.zeros(fused_len, np.float32), "all five inputs empty")
  assert [o.shape for o in raw_gather(np.ones(8, np.float32), none, dims)] == [(0, d) for d in dims]


def test_gather_no_inputs_through_the_abi():
  _same(raw_gather_grad(1001, [], [], []), np.zeros(1001, np.float32), "n_inputs = 0")
  _same(raw_gather_grad(1001, [], [], [], device_scale=True), np.zeros(1001, np.float32), "n_inputs = 0, device scale")
  assert raw_gather(np.ones(8, np.float32), [], []) == []


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7])
def test_gather_key_counts_that_are_no_multiple_of_four(n):
  """A lane group of the float4 gradient takes kGatherGradKeys = 4 keys: unique offsets, so n keys."""
  rng = np.random.default_rng(39)
  dims = [8]
  offs = [rng.permutation(n + 2)[:n] * 8]
  _check_gather_both_ways((n + 2) * 8, offs, dims, 40 + n, False, "%d keys" % n)


@pytest.mark.parametrize("dims", [[4, 8], [3, 8]], ids=["float4", "scalar"])
def test_gather_gradient_mixed_widths_on_one_offset(dims):
  """Input 0 is narrower than input 1 and half of input 1's offsets are offsets of input 0.  Rows are numbered
  input after input, so the narrow row comes first in every shared list: a key that took its width from its
  first addend dropped columns dims[0] .. 7 of the wide rows (the reference adds every element of every row,
  map_id_to_embedding.cu.cc:105-117; tests/post_exchange_truth.py).  Slots are 8 floats apart: ranges are
  equal at their start or disjoint."""
  rng = np.random.default_rng(41)
  n, slots = 1000, 300
  o0 = rng.integers(0, slots, n) * 8
  o1 = (slots + rng.integers(0, slots, n)) * 8
  o1[::2] = rng.choice(o0, n // 2)
  o1[1] = o0[0]
  offs = [o0, o1]
  fused_len = 2 * slots * 8
  grads = [rng.standard_normal((n, d)).astype(np.float32) for d in dims]
  exp = T.gather_grad(fused_len, grads, offs, dims, SCALE)
  shared = np.intersect1d(o0, o1)
  assert shared.size > 100 and np.all(exp[shared[:, None] + np.arange(8)] != 0)   # (the columns in question)
  got = raw_gather_grad(fused_len, grads, offs, dims)
  _same(got, exp, "mixed widths %s" % dims)
  _same(raw_gather_grad(fused_len, grads, offs, dims, device_scale=True), got, "mixed widths, device scale")
  # the wide input first: the same sums in another order
  exp_r = T.gather_grad(fused_len, grads[::-1], offs[::-1], dims[::-1], SCALE)
  _same(raw_gather_grad(fused_len, grads[::-1], offs[::-1], dims[::-1]), exp_r, "mixed widths, wide input first")


# ------------------------------------------------------------------------------------------ reduce_rows
LENS = (0, 1, 3, 4, 5, 8, 9)     # both sides of the 4-rows-in-flight unroll


def _segments(batch, long_at=None, empty=()):
  lens = np.array([LENS[b % len(LENS)] for b in range(batch)])
  if long_at is not None:
    lens[long_at] = 1000
  lens[list(empty)] = 0
  return np.repeat(np.arange(batch), lens)


@functools.lru_cache(maxsize=None)
def _reduce_case(dim, batch, sorted_):
  """(indices, values, [expected per mode]); the unsorted form is the sorted data under a fixed permutation.
  Built once per shape and shared: nothing writes to it."""
  rng = np.random.default_rng(1000 * dim + batch)
  if batch == 37:
    ind = _segments(37, long_at=20, empty=(0, 36))
  else:
    ind = _segments(batch)
    if ind.size == 0:          # batch 1: its one segment would be LENS[0] = 0 rows
      ind = np.zeros(5, np.int64)
  vals = rng.standard_normal((ind.size, dim)).astype(np.float32)
  if not sorted_:
    perm = np.random.default_rng(7).permutation(ind.size)
    ind, vals = ind[perm], vals[perm]
  exp = [T.reduce(ind, vals, batch, mode) for mode in range(3)]
  for a in (ind, vals, *exp):
    a.setflags(write=False)
  return ind, vals, exp


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("dim", [1, 4, 7, 64, 68, 100, 129])
def test_reduce_rows_widths_and_segment_lengths(dim, sorted_):
  """Batch 37: outputs 0 and 36 empty, segment lengths 0 1 3 4 5 8 9 in turn, output 20 with 1 000 rows.  Dims
  of one float4 trip (4, 64), two (68, 100), scalar with one trip (1, 7) and nine (129)."""
  ind, vals, exp = _reduce_case(dim, 37, sorted_)
  for mode in range(3):
    _same(raw_reduce(ind, vals, 37, mode, sorted_), exp[mode], "dim %d mode %d" % (dim, mode))


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("dim", [4, 7])
@pytest.mark.parametrize("batch", [1, 17])
def test_reduce_rows_batch_edges(batch, dim, sorted_):
  ind, vals, exp = _reduce_case(dim, batch, sorted_)
  for mode in range(3):
    _same(raw_reduce(ind, vals, batch, mode, sorted_), exp[mode], "batch %d dim %d mode %d" % (batch, dim, mode))


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("dim", [4, 7])
def test_reduce_rows_without_rows(dim, sorted_):
  """n = 0, batch 5: zeros for sum and sqrtn, NaN for mean."""
  ind, vals = np.zeros(0, np.int64), np.zeros((0, dim), np.float32)
  for mode in range(3):
    got = raw_reduce(ind, vals, 5, mode, sorted_)
    if mode == 1:
      assert np.isnan(got).all()
    else:
      _same(got, np.zeros((5, dim), np.float32), "mode %d" % mode)
    _same(got, T.reduce(ind, vals, 5, mode))


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("dim", [4, 7])
@pytest.mark.parametrize("batch", [512, 513])
def test_reduce_rows_ignores_indices_out_of_range(batch, dim, sorted_):
  """Default forms only (see the header).  Batch 512: the index `batch` is the sort's `limit` key, sorted last
  and cut off; batch 513: it lies in [batch, limit = 1024) and the list kernel returns on it; -1 becomes the
  `limit` key either way.  Sorted input: -1 in front, `batch` at the back, which the binary searches pass by."""
  rng = np.random.default_rng(batch + dim)
  ind = np.sort(rng.integers(0, batch, 3000))
  ind[ind == 3] = 4                                   # (an empty output among them)
  bad_lo, bad_hi = np.full(5, -1), np.full(6, batch)
  ind = np.concatenate([bad_lo, ind, bad_hi])
  vals = rng.standard_normal((ind.size, dim)).astype(np.float32)
  if not sorted_:
    perm = rng.permutation(ind.size)
    ind, vals = ind[perm], vals[perm]
  for mode in range(3):
    _same(raw_reduce(ind, vals, batch, mode, sorted_), T.reduce(ind, vals, batch, mode),
          "batch %d dim %d mode %d" % (batch, dim, mode))


CHILD = r"""
import os, sys
import numpy as np, torch
assert os.environ.get("MHTE_POOL_ATOMICS") == "1" and os.environ.get("MHTE_NO_REBUILD") == "1"
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import post_exchange_truth as T
from monolith_amd import distribution_ops as D
rng = np.random.default_rng(13)
batch = 37
lens = rng.integers(0, 9, batch)
lens[[0, 11, 36]] = 0            # empty outputs: first, middle, last
lens[20] = 200
ind = np.repeat(np.arange(batch), lens)
ind = ind[rng.permutation(ind.size)]          # every index lies in [0, batch): this form indexes unchecked
assert ind.min() >= 0 and ind.max() < batch
for dim in (4, 7):
  # integers in [-8, 8], at most 200 rows per output: every sum and sum of squares is exact in fp32 in any order
  vals = rng.integers(-8, 9, (ind.size, dim)).astype(np.float32)
  for mode, fn in ((0, D.reduce_sum), (1, D.reduce_mean), (2, D.reduce_sqrtn)):
    got = fn(torch.from_numpy(ind[:, None]).cuda(), torch.from_numpy(vals).cuda(), [batch], False).cpu().numpy()
    exp = T.reduce(ind, vals, batch, mode)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), ("NaN places", dim, mode)
    assert nan.any() == (mode == 1)
    assert np.array_equal(np.where(nan, np.float32(0), got).view(np.uint32),
                          np.where(nan, np.float32(0), exp).view(np.uint32)), ("differs from the model", dim, mode)
print("ATOMIC-REDUCE-OK")
"""


def test_reduce_rows_in_the_float_atomic_form():
  """reduce_rows_atomic_kernel + reduce_rows_finish_kernel.  MHTE_POOL_ATOMICS is read once per process: a fresh
  child with its own time limit.  A child that ends with a fault status ends the session — nothing more is
  started on the GPU behind a fault."""
  env = dict(os.environ, MHTE_POOL_ATOMICS="1", MHTE_NO_REBUILD="1")
  try:
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=240)
  except subprocess.TimeoutExpired:
    pytest.exit("the float-atomic child ran into its time limit: nothing more is started on the GPU", returncode=3)
  if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
    pytest.exit("the float-atomic child ended with status %d: nothing more is started on the GPU\n%s" %
                (r.returncode, r.stderr[-2000:]), returncode=3)
  assert r.returncode == 0 and "ATOMIC-REDUCE-OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])


# --------------------------------------------------------------------------------------- grouping sizes
def _grouping_case(n, batch):
  """Unsorted reduce_sum at dim 4 against np.add.at (unbuffered: row after row), one output holding a fifth
  of the rows."""
  rng = np.random.default_rng(n * 31 + batch)
  ind = rng.integers(0, batch, n)
  ind[rng.random(n) < 0.2] = min(7, batch - 1)
  vals = rng.standard_normal((n, 4)).astype(np.float32)
  exp = np.zeros((batch, 4), np.float32)
  np.add.at(exp, ind, vals)
  _same(raw_reduce(ind, vals, batch, 0, False), exp, "n %d batch %d" % (n, batch))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193])
def test_grouping_sizes_at_the_wavefront_and_tile_edges(n, monkeypatch):
  """64 keys per wavefront step, 1 024 per wavefront, 4 096 per tile of the sort and of the run compaction."""
  monkeypatch.delenv("MHTE_GROUP_DD", raising=False)
  _grouping_case(n, 300)


@pytest.mark.parametrize("batch,form", [(1, "sort"), (2, "sort"), (512, "sort"), (513, "sort"), (2**19, "sort"),
                                        (2**19 + 1, "sort"), (513, "dedup"), (2**19 + 1, "dedup")])
def test_grouping_pass_counts(batch, form, monkeypatch):
  """Key bits + 1 = 2, 2, 10, 11, 20, 21: one pass of 2 bits, one of 10, two of 6 + 5, two of 10 + 10, three of
  7; and the list-building dedup (MHTE_GROUP_DD=1, read per call) at the two sizes just past a boundary."""
  if form == "dedup":
    monkeypatch.setenv("MHTE_GROUP_DD", "1")
  else:
    monkeypatch.delenv("MHTE_GROUP_DD", raising=False)
  _grouping_case(5000, batch)


# -------------------------------------------------------------------------------------- lookup gradient
@pytest.mark.parametrize("index_cols", [1, 3])
@pytest.mark.parametrize("dim", [1, 4, 9, 33, 36, 260])
def test_lookup_gradient_widths(dim, index_cols):
  """8 lanes per row: float4 with one trip (4), two (36) and nine (260); scalar with one (1), two (9) and five
  (33).  Column 0 of the index matrix is the row; the others hold values that would be out of range."""
  rng = np.random.default_rng(dim)
  n, rows = 4099, 37
  idx = rng.integers(10**6, 10**7, (n, index_cols))
  idx[:, 0] = rng.integers(0, rows, n)
  ids = rng.integers(-2**62, 2**62, n)
  g = rng.standard_normal((rows, dim)).astype(np.float32)
  exp_ids, exp = T.lookup_gradient(idx, ids, g)
  got_ids, got = raw_lookup_gradient(idx, ids, g)
  np.testing.assert_array_equal(got_ids, exp_ids)
  _same(got, exp, "dim %d" % dim)


def test_lookup_gradient_beyond_one_row_per_lane_group():
  """The grid is capped at 65 536 workgroups = 2 097 152 lane groups: five rows more, and groups 0 .. 4 take a
  second row."""
  rng = np.random.default_rng(3)
  n, rows = 2_097_152 + 5, 37
  idx = rng.integers(0, rows, (n, 1))
  ids = np.arange(n, dtype=np.int64) * 3 - 7
  g = rng.standard_normal((rows, 4)).astype(np.float32)
  got_ids, got = raw_lookup_gradient(idx, ids, g)
  np.testing.assert_array_equal(got_ids, ids)
  assert np.array_equal(_bits(got), _bits(g[idx[:, 0]]))
