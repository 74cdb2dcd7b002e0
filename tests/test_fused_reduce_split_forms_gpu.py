"""Every form of the fused reduce-and-split pooling (-m gpu): ``reduce_split_kernel<EXT, FWD>``
(csrc/mhte_pool_split_kernels.h) as ``reduce_split_launch`` (csrc/mhte.hip) plans it, through the C ABI
(mhte_fused_reduce_and_split, mhte_fused_reduce_and_split_grad).

The expected values are the sequential fp32 chains of tests/fused_reduce_split_truth.py.  Every comparison is on
uint32 bit patterns: no tolerance, no element left out.  Every output (forward slices, embedding gradients) is
handed in as a quiet-NaN pattern no computation produces, in storage of its own between guard words, so a float
the call leaves out and a store next to a buffer both show; after every call the guards and every input
(row_splits; embeddings in the forward; slice gradients in the gradient) are compared with their host copies.
Every case asserts through ``T.plan`` — a mirror of the planner's documented rules — that its shape still selects
the form it is named for.

Branch                                              reached by
  tables in the kernel arguments / EXT              lane groups [inline] / [ext_units], [ext_slices], grid stride,
                                                    65 600 units
  EXT by slices alone (> 96 slices, <= 32 units)    lane groups [ext_slices]
  forward / gradient                                every case but the two clamps and bs = 0 runs both
  float4 / scalar lanes, inline and EXT             lane groups (split_load feeds float4 units in both EXT forms)
  log2g = 0 .. 6, both lane kinds                   lane groups
  col0 > 0, last unit narrower than the first       wider than one unit (float4 260, 516; scalar 65, 129, 200)
  slice search: first, a middle, the last slice     wider than one unit ([256, 4, 256], [64, 1, 64]); lane groups
                                                    [ext_slices] (100 slices under 2 units)
  the 16-deep loop and its 4-wide tail              the length cycle 0, 1, 3, 4, 5, 15, 16, 17, 19, 20, 31, 32, 33,
                                                    36, 48 of every bs = 37 case; rows of 16 and 17 times -0.0
  b >= bs at once, one and two workgroups           batch edges (bs 1, 3, 4, 5 | 255, 256, 257)
  grid stride and the prefetched splits (nb, n0,    grid stride (bs = 600 on 64 row blocks, both lane kinds, beside
  n1), beside units that do not stride              one-lane units that do not stride; a row of 40 ids in pass two)
  unit_base > 0                                     65 600 units
  a feature on 4-byte accesses by itself            per-feature fallback (embedding, slice pointer, slice start)
  the clamp of the forward                          clamp, forward
  the clamp of the gradient                         clamp, gradient
  head/tail fill without / with its stride loop     uncovered rows (0,0) (1,0) (0,1) / (5,3000) (3000,5); lane groups
                                                    (head 3, tail 5)
  bs = 0 (gradient: every row +0)                   bs = 0
  the Python wrappers                               wrappers on the wide case

Preconditions the cases keep:
  * gradient: monotone row_splits (overlapping ranges would have two lane groups store to the same rows: a race,
    not tested) — the clamp of the gradient is therefore driven by splits that only start below 0 and end above n;
  * every read stays inside an allocation: the malformed splits of the clamp cases point at most 9 rows outside
    the matrix, which lies between 32 rows of NaN pattern on either side (more than the excursion plus the 16 rows
    in flight), so a clamp that failed reads NaN (wrong bits) or stores into guard rows, never outside storage.

Sizes are the smallest that select the branch."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_reduce_split_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd._lib import check, vp  # noqa: E402
from monolith_amd.multi_hash_table_ops import _stream  # noqa: E402

GUARD = 8                 # floats on each side of a buffer, at least
NAN_WORD = 0x7FC0BEEF     # a quiet NaN no computation produces
GUARD_WORD = 0x7FC0CAFE   # (a NaN too: an input read outside its payload gives wrong bits)
EVERY_LANE_KIND = {(v, g) for v in (False, True) for g in range(7)}


class Buf:
  """[rows, cols] float32 at ``off`` floats into storage of its own: off 0 is 16-byte aligned, off 1 has
  ptr() % 16 == 4.  The payload starts as ``data`` (an input) or as the NaN pattern (an output); guard words on
  both sides, at least ``guard_rows`` rows of them."""

  def __init__(self, rows, cols, off=0, data=None, guard_rows=0):
    n = rows * cols
    g = max(GUARD, (guard_rows * cols + 3) // 4 * 4)
    words = np.full(g + off + n + g, GUARD_WORD, np.uint32)
    self.host = None if data is None else T.bits(data).reshape(rows, cols).copy()
    words[g + off:g + off + n] = NAN_WORD if data is None else self.host.ravel()
    self.store = torch.from_numpy(words.view(np.int32)).cuda()
    self.lo, self.n, self.shape = g + off, n, (rows, cols)
    assert self.store.data_ptr() % 16 == 0 and self.ptr() % 16 == 4 * off

  def ptr(self, at=0):
    """The address of float ``at`` of the payload."""
    return self.store.data_ptr() + 4 * (self.lo + at)

  def read(self, what):
    """The payload's bit patterns; the guards must be untouched."""
    words = self.store.cpu().numpy().view(np.uint32)
    assert (words[:self.lo] == GUARD_WORD).all() and (words[self.lo + self.n:] == GUARD_WORD).all(), \
        "%s: a guard word was overwritten" % what
    return words[self.lo:self.lo + self.n].reshape(self.shape)

  def unchanged(self, what):
    np.testing.assert_array_equal(self.read(what), self.host, err_msg="%s: an input was written" % what)


def _same(got_bits, want, what):
  want = T.bits(want)
  assert got_bits.shape == want.shape, (what, got_bits.shape, want.shape)
  np.testing.assert_array_equal(got_bits, want, err_msg=what)


def _ptrs(addresses):
  return (C.c_void_p * max(len(addresses), 1))(*addresses)


def _i32(values):
  return (C.c_int32 * max(len(values), 1))(*[int(v) for v in values])


# ------------------------------------------------------------------------------------------ raw callers
def raw_forward(row_splits, n_splits, emb_ptrs, emb_rows, emb_dims, flat_slice_dims, out_ptrs):
  """mhte_fused_reduce_and_split on host lists; row_splits (concatenated, int32) must come back unchanged."""
  rs = np.ascontiguousarray(row_splits, np.int32)
  rs_t = torch.from_numpy(rs.copy()).cuda()
  rss = _i32(np.concatenate([[0], np.cumsum(n_splits)]))
  check(_lib.lib().mhte_fused_reduce_and_split(
      vp(rs_t), rss, _ptrs(emb_ptrs), (C.c_int64 * len(emb_rows))(*emb_rows), _i32(emb_dims), len(emb_dims),
      _i32(flat_slice_dims), len(flat_slice_dims), _ptrs(out_ptrs), _stream()))
  torch.cuda.synchronize()
  np.testing.assert_array_equal(rs_t.cpu().numpy(), rs, err_msg="row_splits were written")


def raw_gradient(row_splits, n_splits, emb_rows, emb_dims, flat_slice_dims, slice_grad_ptrs, grad_ptrs):
  """mhte_fused_reduce_and_split_grad on host lists."""
  rs = np.ascontiguousarray(row_splits, np.int32)
  rs_t = torch.from_numpy(rs.copy()).cuda()
  rss = _i32(np.concatenate([[0], np.cumsum(n_splits)]))
  check(_lib.lib().mhte_fused_reduce_and_split_grad(
      vp(rs_t), rss, (C.c_int64 * len(emb_rows))(*emb_rows), _i32(emb_dims), len(emb_dims),
      _i32(flat_slice_dims), len(flat_slice_dims), _ptrs(slice_grad_ptrs), _ptrs(grad_ptrs), _stream()))
  torch.cuda.synchronize()
  np.testing.assert_array_equal(rs_t.cpu().numpy(), rs, err_msg="row_splits were written")


def _lists(feats):
  return (np.concatenate([f["row_splits"] for f in feats]), [f["row_splits"].size for f in feats],
          [int(f["emb"].shape[0]) for f in feats], [int(f["emb"].shape[1]) for f in feats],
          [int(d) for f in feats for d in f["slice_dims"]])


def _aligned(feats, emb_off, slice_off):
  return [emb_off.get(i, 0) == 0 and all(slice_off.get((i, k), 0) == 0 for k in range(len(f["slice_dims"])))
          for i, f in enumerate(feats)]


def forward(feats, emb_off=None, slice_off=None, guard_rows=0, what="forward"):
  """The forward on buffers of their own (emb_off[i], slice_off[(i, k)]: 1 puts embedding i / slice k of feature
  i one float in) -> (the outputs' bits per feature, side by side [bs, dim]; the plan)."""
  emb_off, slice_off = emb_off or {}, slice_off or {}
  rs, n_splits, rows, dims, flat = _lists(feats)
  bs = n_splits[0] - 1
  embs = [Buf(*f["emb"].shape, off=emb_off.get(i, 0), data=f["emb"], guard_rows=guard_rows)
          for i, f in enumerate(feats)]
  outs = [[Buf(bs, d, off=slice_off.get((i, k), 0)) for k, d in enumerate(f["slice_dims"])]
          for i, f in enumerate(feats)]
  raw_forward(rs, n_splits, [e.ptr() for e in embs], rows, dims, flat, [o.ptr() for fo in outs for o in fo])
  for i, e in enumerate(embs):
    e.unchanged("%s: embedding %d" % (what, i))
  got = [np.concatenate([o.read("%s: feature %d, slice %d" % (what, i, k)) for k, o in enumerate(fo)], 1)
         for i, fo in enumerate(outs)]
  return got, T.plan_of(feats, _aligned(feats, emb_off, slice_off))


def gradient(feats, grads, grad_off=None, slice_off=None, guard_rows=0, what="gradient"):
  """The gradient (grads[i][k]: [bs, d] of slice k of feature i) -> (the embedding gradients' bits per feature;
  the plan)."""
  grad_off, slice_off = grad_off or {}, slice_off or {}
  rs, n_splits, rows, dims, flat = _lists(feats)
  sg = [[Buf(*g.shape, off=slice_off.get((i, k), 0), data=g) for k, g in enumerate(gs)] for i, gs in enumerate(grads)]
  out = [Buf(n, d, off=grad_off.get(i, 0), guard_rows=guard_rows) for i, (n, d) in enumerate(zip(rows, dims))]
  raw_gradient(rs, n_splits, rows, dims, flat, [b.ptr() for fb in sg for b in fb], [o.ptr() for o in out])
  for i, fb in enumerate(sg):
    for k, b in enumerate(fb):
      b.unchanged("%s: slice gradient %d of feature %d" % (what, k, i))
  return ([o.read("%s: gradient of feature %d" % (what, i)) for i, o in enumerate(out)],
          T.plan_of(feats, _aligned(feats, grad_off, slice_off)))


def want_forward(f):
  """[bs, dim]: the chain over the ranges the header's clamp makes of the feature's row_splits."""
  s0, s1 = T.clamped_splits(f["row_splits"], f["emb"].shape[0])
  return np.concatenate(T.truth_forward_ranges(s0, s1, f["emb"], f["slice_dims"]), 1)


def want_gradient(f, gs):
  s0, s1 = T.clamped_splits(f["row_splits"], f["emb"].shape[0])
  return T.truth_gradient_ranges(s0, s1, f["emb"].shape[0], gs)


def both(feats, seed, what, **offs):
  """Forward and gradient against the truth -> (forward bits, gradient bits, the plan, the slice gradients)."""
  got, p = forward(feats, what=what + " forward", **offs)
  for i, f in enumerate(feats):
    _same(got[i], want_forward(f), "%s: forward, feature %d (dim %d)" % (what, i, f["emb"].shape[1]))
  grads = T.slice_grads_of(np.random.default_rng(seed), feats)
  goff = {"grad_off": offs.get("emb_off"), "slice_off": offs.get("slice_off")}
  ggot, gp = gradient(feats, grads, what=what + " gradient", **goff)
  assert gp == p
  for i, f in enumerate(feats):
    _same(ggot[i], want_gradient(f, grads[i]), "%s: gradient, feature %d (dim %d)" % (what, i, f["emb"].shape[1]))
  return got, ggot, p, grads


# ------------------------------------------------------------- 1. lane groups, both lane kinds, inline and EXT
@pytest.mark.parametrize("tables", ["inline", "ext_units", "ext_slices"])
def test_lane_groups_of_both_kinds(tables):
  """bs = 37, the length cycle; float4 features of 1 .. 64 lanes and scalar features of 1 .. 64 columns: both lane
  kinds at every log2g from 0 to 6, with the tables in the kernel arguments, in device memory because of 33 units,
  and in device memory because of 123 slices under 23 units."""
  feats = T.lane_group_case(tables)
  got, ggot, p, _ = both(feats, 1101, "lane groups [%s]" % tables)
  assert T.lane_kinds(p) == EVERY_LANE_KIND
  assert (p["n_units"], p["n_slices"], p["ext"]) == {"inline": (21, 23, False), "ext_units": (33, 35, True),
                                                     "ext_slices": (23, 123, True)}[tables]
  # 16 and 17 addends of -0.0 (the deep loop alone, the deep loop and a tail of one): +0.0 in every bit
  i = [f["emb"].shape[1] for f in feats].index(9)
  lens = np.diff(feats[i]["row_splits"])
  for n in (16, 17):
    b = int(np.flatnonzero(lens == n)[0])
    rows = feats[i]["emb"][feats[i]["row_splits"][b]:feats[i]["row_splits"][b + 1]]
    assert rows.shape == (n, 9) and (T.bits(rows) == 0x80000000).all()
    assert not got[i][b].any()
  # the head of 3 and the tail of 5 uncovered rows of the dim-36 (float4) and dim-17 (scalar) features are +0
  for dim in (36, 17):
    i = [f["emb"].shape[1] for f in feats].index(dim)
    rs = feats[i]["row_splits"]
    assert rs[0] == 3 and rs[-1] + 5 == ggot[i].shape[0]
    assert not ggot[i][:3].any() and not ggot[i][-5:].any()


# ------------------------------------------------------------------------- 2. features wider than one unit
@functools.lru_cache(maxsize=None)
def _wide():
  feats = T.wide_case()
  got, ggot, p, grads = both(feats, 1102, "wider than one unit")
  return feats, got, ggot, p, grads


def test_features_wider_than_one_unit():
  """float4 dim 260 [8, 252] (units of 64 lanes and of 1, the unit edge at column 256 inside slice 1) and 516
  [256, 4, 256] (a slice that starts at a unit edge, a one-lane slice); scalar 65 [65], 129 [64, 1, 64] and 200
  [7, 193]: col0 > 0, a last unit narrower than the first, the slice search ending on a first, a middle and a last
  slice — on data whose columns all differ."""
  feats, _, _, p, _ = _wide()
  assert not p["ext"] and [f["vec"] for f in p["features"]] == [True, True, False, False, False]
  assert all(len(f["units"]) > 1 and f["units"][-1][0] > 0 and f["units"][-1][1] < f["units"][0][1]
             for f in p["features"])


# ---------------------------------------------------------------------------------------- 3. batch edges
@pytest.mark.parametrize("bs", [1, 3, 4, 5, 255, 256, 257])
def test_batch_edges(bs):
  """float4 dim 256 (4 lane groups per workgroup) beside scalar dim 1 (256 per workgroup): one row, fewer rows than
  one workgroup's lane groups, and the edges of one and two workgroups of either unit."""
  rng = np.random.default_rng(1103)
  lens = [np.array([17]), np.array([17])] if bs == 1 else [T.cycle_lengths(bs, 2), T.cycle_lengths(bs, 7)]
  feats = [T.feature(rng, lens[0], 256, [256]), T.feature(rng, lens[1], 1, [1])]
  _, _, p, _ = both(feats, 1203, "batch edges, bs = %d" % bs)
  assert T.lane_kinds(p) == {(True, 6), (False, 0)} and not p["ext"]
  assert p["gx"] == (bs + 3) // 4   # row blocks for the 64-lane unit; the 1-lane unit needs (bs + 255) / 256


# --------------------------------------------------------------------------- 4. grid stride at a small shape
def test_grid_stride_at_a_small_shape():
  """60 scalar features of dim 321 and 40 float4 features of dim 1028: 560 units, so 64 row blocks.  A 64-lane
  unit covers 256 batch rows per pass and bs = 600 takes three (the last with 88 rows), prefetching the next row's
  splits; the features' one-lane last units hold all 600 rows in three of their 64 row blocks and do not stride.
  Mean row length about 1, half the rows empty; batch row 300 (second pass) of the first feature of either kind
  has 40 ids: prefetched splits feed the deep loop."""
  bs = 600
  rng = np.random.default_rng(1104)
  feats = []
  for i in range(100):
    lens = rng.geometric(0.5, size=bs) * (rng.random(bs) < 0.5)
    if i in (0, 60):
      lens[300] = 40
    dim, sl = (321, [100, 221]) if i < 60 else (1028, [512, 516])
    feats.append(T.feature(rng, lens, dim, sl, head=i % 3, tail=i % 2))
  _, _, p, _ = both(feats, 1204, "grid stride")
  assert (p["n_units"], p["ext"], p["gx"], p["need"]) == (560, True, 64, 150)
  assert (False, 6) in T.lane_kinds(p) and (True, 6) in T.lane_kinds(p)
  assert 2 * p["gx"] * 4 < bs <= 3 * p["gx"] * 4 and bs - 2 * p["gx"] * 4 == 88 and p["gx"] * 4 <= 300 < 2 * p["gx"] * 4
  assert bs <= p["gx"] * 256 and (False, 0) in T.lane_kinds(p) and (True, 0) in T.lane_kinds(p)


# ------------------------------------------------------------------------------ 5. more than 65 535 units
def test_more_than_65535_units():
  """1 025 scalar features of dim 4 096 in slices [4095, 1], bs = 2, row lengths 1 and 2: 65 600 units in two
  grid.y chunks; unit 65 535, the first of the second chunk, is feature 1 023's last (col0 4 032).  Embeddings,
  outputs, slice gradients and gradients are one allocation each, the tables point into them; every feature is
  checked, 1 022, 1 023 and 1 024 on both sides of the chunk edge among them."""
  F, dim, bs, n = 1025, 4096, 2, 3
  p = T.plan([dim] * F, [[dim - 1, 1]] * F, True, bs)
  units = [(i,) + u for i, f in enumerate(p["features"]) for u in f["units"]]
  assert len(units) == 65600 and units[65535] == (1023, 4032, 64, 6) and not p["features"][1023]["vec"]
  rng = np.random.default_rng(1105)
  E = T.scaled_normal(rng, (F, n, dim))
  SG = rng.standard_normal((F, bs, dim)).astype(np.float32)   # the slice gradients, side by side

  def sliced(a):   # [F, bs, dim] -> [F, bs * dim]: slice 0 [bs, dim - 1], then slice 1 [bs, 1]
    return np.concatenate([a[:, :, :dim - 1].reshape(F, -1), a[:, :, dim - 1:].reshape(F, -1)], 1)

  rs, n_splits = np.tile(np.array([0, 1, 3], np.int32), F), [bs + 1] * F
  rows, dims, flat = [n] * F, [dim] * F, [dim - 1, 1] * F
  slice_at = [i * bs * dim + k for i in range(F) for k in (0, bs * (dim - 1))]
  emb, out = Buf(F, n * dim, data=E), Buf(F, bs * dim)
  raw_forward(rs, n_splits, [emb.ptr(i * n * dim) for i in range(F)], rows, dims, flat,
              [out.ptr(a) for a in slice_at])
  emb.unchanged("65 600 units: embeddings")
  acc = np.zeros((F, bs, dim), np.float32)
  acc[:, 0] = acc[:, 0] + E[:, 0]
  acc[:, 1] = (acc[:, 1] + E[:, 1]) + E[:, 2]
  got, want = out.read("65 600 units: outputs"), T.bits(sliced(acc))
  wrong = np.flatnonzero((got != want).any(axis=1))
  assert wrong.size == 0, "forward: features %s differ" % wrong[:20]
  sg, grad = Buf(F, bs * dim, data=sliced(SG)), Buf(F, n * dim)
  raw_gradient(rs, n_splits, rows, dims, flat, [sg.ptr(a) for a in slice_at],
               [grad.ptr(i * n * dim) for i in range(F)])
  sg.unchanged("65 600 units: slice gradients")
  got, want = grad.read("65 600 units: gradients"), T.bits(SG[:, [0, 1, 1]].reshape(F, -1))
  wrong = np.flatnonzero((got != want).any(axis=1))
  assert wrong.size == 0, "gradient: features %s differ" % wrong[:20]


# ------------------------------------------------------------- 6. per-feature fallback beside float4 neighbours
def test_a_feature_falls_back_to_4_byte_accesses_by_itself():
  """Five features of dim 32 in slices [8, 24], every buffer aligned but: feature 1's embedding (in the gradient
  its gradient) one float in; feature 2's second slice one float in; feature 3 cut [6, 26].  Features 0 and 4 stay
  float4 (8 lanes), 1 to 3 run on floats (32 lanes); the same bits as the truth and as the all-aligned run."""
  rng = np.random.default_rng(1106)
  base = T.cycle_case(rng, [(32, [8, 24])] * 5, 37, {32: (2, 1)})
  feats = [dict(f) for f in base]
  feats[3]["slice_dims"] = [6, 26]
  full = [rng.standard_normal((37, 32)).astype(np.float32) for _ in feats]
  cut = lambda fs: [np.split(g, np.cumsum(f["slice_dims"])[:-1], 1) for f, g in zip(fs, full)]  # noqa: E731
  fwd0, p0 = forward(base, what="all aligned")
  grad0, _ = gradient(base, cut(base), what="all aligned")
  assert all(f == {"vec": True, "units": [(0, 32, 3)]} for f in p0["features"])
  offs = {1: 1}, {(2, 1): 1}
  fwd1, p1 = forward(feats, emb_off=offs[0], slice_off=offs[1], what="fallback")
  grad1, gp1 = gradient(feats, cut(feats), grad_off=offs[0], slice_off=offs[1], what="fallback")
  assert p1 == gp1 and [f["vec"] for f in p1["features"]] == [True, False, False, False, True]
  assert [f["units"] for f in p1["features"]] == [[(0, 32, 3)]] + [[(0, 32, 5)]] * 3 + [[(0, 32, 3)]]
  for i, f in enumerate(feats):
    _same(fwd1[i], want_forward(f), "fallback: forward, feature %d" % i)
    _same(grad1[i], want_gradient(f, cut(feats)[i]), "fallback: gradient, feature %d" % i)
    np.testing.assert_array_equal(fwd1[i], fwd0[i], err_msg="forward of feature %d against the aligned run" % i)
    np.testing.assert_array_equal(grad1[i], grad0[i], err_msg="gradient of feature %d against the aligned run" % i)


# --------------------------------------------------------------------------------------------- 7, 8. the clamps
N_CLAMP = 40
MALFORMED = [-7, -1, 3, 9, 20, 14, 16, 16, 18, 20, 22, N_CLAMP + 1, N_CLAMP + 9]    # forward: any row_splits
BEYOND = [-7, -1, 3, 9, 14, 20, 20, 22, 30, 38, N_CLAMP, N_CLAMP + 1, N_CLAMP + 9]  # gradient: monotone ones


def _clamp_feats(rs, seed):
  rng = np.random.default_rng(seed)
  rs = np.array(rs, np.int32)
  assert rs.size == 13
  return [{"row_splits": rs, "emb": T.scaled_normal(rng, (N_CLAMP, dim)), "slice_dims": [dim]} for dim in (8, 5)]


def test_the_forward_clamps_malformed_row_splits():
  """One float4 (dim 8) and one scalar (dim 5) feature, bs = 12, 40 rows; the splits hold -7 and -1 at the front,
  the descending pair 20, 14 in the middle and n + 1, n + 9 at the back.  s0 = clamp(rs[b], 0, n), s1 =
  clamp(rs[b + 1], s0, n): the ranges reach outside by 9 rows at most, and the matrix lies between 32 rows of NaN
  pattern, so a clamp that failed reads NaN; the range 22 .. 41 is 18 rows once clamped (the deep loop and a
  tail).  Forward only: ranges 9 .. 20 and 14 .. 16 overlap."""
  feats = _clamp_feats(MALFORMED, 1107)
  s0, s1 = T.clamped_splits(MALFORMED, N_CLAMP)
  np.testing.assert_array_equal(s0, [0, 0, 3, 9, 20, 14, 16, 16, 18, 20, 22, 40])
  np.testing.assert_array_equal(s1, [0, 3, 9, 20, 20, 16, 16, 18, 20, 22, 40, 40])
  assert max(0 - min(MALFORMED), max(MALFORMED) - N_CLAMP) + T.kernel_constants()["kSplitDeep"] < 32
  got, p = forward(feats, guard_rows=32, what="clamp")
  assert [f["vec"] for f in p["features"]] == [True, False]
  for i, f in enumerate(feats):
    _same(got[i], want_forward(f), "clamp: forward, feature %d" % i)
    assert not np.isnan(got[i].view(np.float32)).any()


def test_the_gradient_clamps_row_splits_beyond_the_matrix():
  """Monotone splits only — overlapping ranges would have two lane groups store to the same rows — that start
  below 0 (-7, -1) and end above n (n + 1, n + 9).  The gradient lies between 32 guard rows: rows inside the
  clamped ranges hold their batch row's slice gradients (every row is covered: no fill), the guards are untouched."""
  feats = _clamp_feats(BEYOND, 1108)
  assert (np.diff(BEYOND) >= 0).all()
  grads = T.slice_grads_of(np.random.default_rng(1208), feats)
  got, p = gradient(feats, grads, guard_rows=32, what="clamp")
  assert [f["vec"] for f in p["features"]] == [True, False]
  s0, s1 = T.clamped_splits(BEYOND, N_CLAMP)
  assert s0[0] == 0 and s1[-1] == N_CLAMP and (s0[1:] == s1[:-1]).all()
  for i, f in enumerate(feats):
    _same(got[i], want_gradient(f, grads[i]), "clamp: gradient, feature %d" % i)
    for b in range(12):
      assert (got[i][s0[b]:s1[b]] == T.bits(grads[i][0][b])).all()


# --------------------------------------------------------------------------- 9. uncovered rows of the gradient
@pytest.mark.parametrize("head,tail", [(0, 0), (1, 0), (0, 1), (5, 3000), (3000, 5)])
def test_uncovered_rows_of_the_gradient(head, tail):
  """float4 dim 256 (one row block: 4 lane groups in its grid) and scalar dim 3 (64 lane groups), bs = 4: no
  uncovered row, a head alone, a tail alone, and a head and a tail of which one is larger than either unit's number
  of lane groups (the `r += stride` loop).  Uncovered rows are +0 in every bit, covered rows exact."""
  rng = np.random.default_rng(1109)
  lens = np.array([2, 0, 5, 1])
  feats = [T.feature(rng, lens, 256, [256], head, tail), T.feature(rng, lens, 3, [3], head, tail)]
  _, ggot, p, _ = both(feats, 1209, "uncovered rows (%d, %d)" % (head, tail))
  assert p["gx"] == 1 and T.lane_kinds(p) == {(True, 6), (False, 2)}
  for g in ggot:
    assert g.shape[0] == head + 8 + tail
    assert not g[:head].any() and not g[head + 8:].any() and g[head:head + 8].all()


def test_gradient_of_an_empty_batch_is_all_plus_zero():
  """bs = 0 with 9 rows in either feature: one row split (4) each, null slice-gradient pointers.  Every row +0."""
  rows, dims = [9, 9], [256, 3]
  p = T.plan(dims, [[256], [3]], True, 0)
  assert p["gx"] == 1 and p["need"] == 1
  out = [Buf(n, d) for n, d in zip(rows, dims)]
  raw_gradient([4, 4], [1, 1], rows, dims, dims, [None, None], [o.ptr() for o in out])
  for i, o in enumerate(out):
    assert not o.read("bs = 0: gradient of feature %d" % i).any()
  # the forward of an empty batch has nothing to write
  emb = [Buf(n, d, data=np.ones((n, d), np.float32)) for n, d in zip(rows, dims)]
  raw_forward([4, 4], [1, 1], [e.ptr() for e in emb], rows, dims, dims, [None, None])
  for i, e in enumerate(emb):
    e.unchanged("bs = 0: embedding %d" % i)


# ----------------------------------------------------------------------------------- 10. the Python wrappers
def test_the_python_wrappers_give_the_bits_of_the_raw_calls():
  feats, got, ggot, _, grads = _wide()
  splits = [torch.from_numpy(f["row_splits"]).cuda() for f in feats]
  embs = [torch.from_numpy(f["emb"]).cuda() for f in feats]
  slice_dims = [f["slice_dims"] for f in feats]
  outs = D.fused_reduce_and_split_gpu(splits, embs, slice_dims)
  assert len(outs) == sum(len(s) for s in slice_dims)
  k = 0
  for i, s in enumerate(slice_dims):
    w = np.concatenate([T.bits(o.cpu().numpy()) for o in outs[k:k + len(s)]], 1)
    np.testing.assert_array_equal(w, got[i], err_msg="wrapper forward, feature %d" % i)
    k += len(s)
  flat = [torch.from_numpy(g).cuda() for gs in grads for g in gs]
  wg = D.fused_reduce_and_split_gpu_grad(splits, embs, flat, slice_dims)
  for i, g in enumerate(wg):
    np.testing.assert_array_equal(T.bits(g.cpu().numpy()), ggot[i], err_msg="wrapper gradient, feature %d" % i)
