"""CPU suite: the host side of mhte_fused_reduce_and_split / ..._grad (MonolithFusedReduceAndSplitGPU and
its gradient, runtime/ops/reduce_op.cu.cc:392-475) — the plan is validated before any device call, a valid
plan without a device is refused loudly — and the numpy truth the GPU suite compares against reproduces
the reference test's expected values (distribution_ops_test.py:374-416, committed as data)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_reduce_split_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402

FAKE = 0x10000   # a "device pointer" the host never follows


def _call(grad, row_split_splits, emb_rows, emb_dims, slice_dims, n_features=None, null=()):
  """-> (status, message) of the entry point on a plan given as host lists; device pointers are fakes."""
  L = _lib.lib()
  nf = len(emb_dims) if n_features is None else n_features
  rss = (C.c_int32 * max(len(row_split_splits), 2))(*row_split_splits)
  rows = (C.c_int64 * max(len(emb_rows), 1))(*emb_rows)
  dims = (C.c_int32 * max(len(emb_dims), 1))(*emb_dims)
  sd = (C.c_int32 * max(len(slice_dims), 1))(*slice_dims)
  embs = (C.c_void_p * max(len(emb_dims), 1))(*[FAKE + 256 * i for i in range(len(emb_dims))])
  outs = (C.c_void_p * max(len(slice_dims), 1))(*[2 * FAKE + 256 * i for i in range(len(slice_dims))])
  a = {"row_splits": C.c_void_p(FAKE), "row_split_splits": rss, "ptrs": embs, "emb_rows": rows,
       "emb_dims": dims, "slice_dims": sd, "slice_ptrs": outs}
  for k in null:
    a[k] = None
  if grad:
    st = L.mhte_fused_reduce_and_split_grad(a["row_splits"], a["row_split_splits"], a["emb_rows"], a["emb_dims"],
                                            C.c_int32(nf), a["slice_dims"], C.c_int32(len(slice_dims)),
                                            a["slice_ptrs"], a["ptrs"], None)
  else:
    st = L.mhte_fused_reduce_and_split(a["row_splits"], a["row_split_splits"], a["ptrs"], a["emb_rows"],
                                       a["emb_dims"], C.c_int32(nf), a["slice_dims"],
                                       C.c_int32(len(slice_dims)), a["slice_ptrs"], None)
  return st, L.mhte_last_error().decode()


# two features of dims 8 and 4, batch size 3 (4 row splits each), slices [8] and [2, 2]
VALID = dict(row_split_splits=[0, 4, 8], emb_rows=[5, 7], emb_dims=[8, 4], slice_dims=[8, 2, 2])


def _invalid(grad, needle, **change):
  st, msg = _call(grad, **{**VALID, **change})
  assert st == _lib.MHTE_INVALID_ARGUMENT, (st, msg)
  assert needle in msg, msg
  assert ("fused_reduce_and_split_grad" if grad else "fused_reduce_and_split:") in msg, msg


@pytest.mark.parametrize("grad", [False, True])
def test_null_arguments_are_invalid(grad):
  for k in ("row_splits", "row_split_splits", "ptrs", "emb_rows", "emb_dims", "slice_dims", "slice_ptrs"):
    _invalid(grad, "null argument", null=(k,))


@pytest.mark.parametrize("grad", [False, True])
def test_no_features_is_invalid(grad):
  _invalid(grad, "n_features must be > 0", n_features=0)
  _invalid(grad, "n_features must be > 0", n_features=-2)


@pytest.mark.parametrize("grad", [False, True])
def test_a_non_positive_dim_is_invalid(grad):
  _invalid(grad, "embedding 1 has the non-positive dim 0", emb_dims=[8, 0])
  _invalid(grad, "embedding 0 has the non-positive dim -8", emb_dims=[-8, 4])
  _invalid(grad, "slice 2 has the non-positive dim 0", slice_dims=[8, 4, 0])
  _invalid(grad, "slice 1 has the non-positive dim -1", slice_dims=[8, -1, 5])


@pytest.mark.parametrize("grad", [False, True])
def test_a_feature_with_another_number_of_row_splits_is_invalid(grad):
  _invalid(grad, "feature 1 has 5 row splits, feature 0 has 4", row_split_splits=[0, 4, 9])
  _invalid(grad, "feature 1 has 3 row splits, feature 0 has 4", row_split_splits=[0, 4, 7])
  _invalid(grad, "feature 0 has no row splits", row_split_splits=[0, 0, 0])


@pytest.mark.parametrize("grad", [False, True])
def test_slice_dims_that_do_not_add_up_are_invalid(grad):
  _invalid(grad, "sum(slice_dims) = 11 differs from sum(emb_dims) = 12", slice_dims=[8, 2, 1])
  _invalid(grad, "sum(slice_dims) = 14 differs from sum(emb_dims) = 12", slice_dims=[8, 2, 4])


@pytest.mark.parametrize("grad", [False, True])
def test_a_slice_that_straddles_two_features_is_invalid(grad):
  _invalid(grad, "straddles features 0 and 1", slice_dims=[6, 4, 2])
  _invalid(grad, "slice 1 ", slice_dims=[4, 6, 2])


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
@pytest.mark.parametrize("grad", [False, True])
def test_a_valid_plan_without_a_device_is_unavailable(grad):
  st, msg = _call(grad, **VALID)
  assert st == _lib.MHTE_UNAVAILABLE, (st, msg)
  assert "no CPU fallback" in msg


def test_unsorted_indices_name_the_route():
  idx = torch.tensor([1, 0], dtype=torch.int64)
  vals = torch.ones(2, 3)
  with pytest.raises(NotImplementedError, match=r"reduce_sum\(\.\.\., indices_sorted=False\)"):
    D.fused_reduce_sum_and_split(idx, vals, 2, [2, 1], indices_sorted=False)
  with pytest.raises(NotImplementedError, match=r"reduce_sum\(\.\.\., indices_sorted=False\)"):
    D.fused_reduce_sum_and_split_gradient(idx, [torch.ones(2, 2), torch.ones(2, 1)], [2, 1], indices_sorted=False)


# ---- the truth procedure against the reference's expected values ----------------------------------------
def test_truth_reproduces_the_reference_forward_cases():
  cases = T.load_kat()["forward"]
  assert len(cases) == 3
  for c in cases:
    rs = T.splits_of_sorted(c["id_indices"], c["id_length"])
    got = T.truth_forward(rs, np.asarray(c["id_values"], np.float32), c["split_dims"])
    assert len(got) == len(c["expected"])
    for g, e in zip(got, c["expected"]):
      e = np.asarray(e, np.float32)
      assert g.shape == e.shape and g.dtype == np.float32
      np.testing.assert_array_equal(T.bits(g), T.bits(e))


def test_truth_reproduces_the_reference_gradient_case():
  (c,) = T.load_kat()["gradient"]
  rs = T.splits_of_sorted(c["id_indices"], c["id_length"])
  got = T.truth_gradient(rs, len(c["id_indices"]), c["slice_grads"])
  np.testing.assert_array_equal(T.bits(got), T.bits(np.asarray(c["expected"], np.float32)))


def test_truth_adds_in_row_order_from_plus_zero():
  # a row of -0.0 alone gives +0.0; (big + small) - big loses small, big - big + small keeps it
  emb = np.array([[-0.0], [1e8], [1.0], [-1e8], [1e8], [-1e8], [1.0]], np.float32)
  got = T.truth_forward([0, 1, 4, 7, 7], emb, [1])[0]
  np.testing.assert_array_equal(T.bits(got), T.bits(np.array([[0.0], [0.0], [1.0], [0.0]], np.float32)))
  # uncovered head and tail rows of the gradient are 0
  g = T.truth_gradient([1, 2, 2, 4], 6, [np.array([[1.], [2.], [3.]], np.float32)])
  np.testing.assert_array_equal(g[:, 0], [0, 1, 3, 3, 0, 0])


# ---- the helpers of the forms suite (tests/test_fused_reduce_split_forms_gpu.py) ---------------------------
def test_clamped_splits_by_hand():
  # a negative, a descending and two too-large entries, n = 10
  s0, s1 = T.clamped_splits([-3, 2, 6, 4, 9, 12, 11], 10)
  np.testing.assert_array_equal(s0, [0, 2, 6, 4, 9, 10])
  np.testing.assert_array_equal(s1, [2, 6, 6, 9, 10, 10])
  # monotone splits inside the matrix are left alone
  s0, s1 = T.clamped_splits([1, 1, 4, 7], 7)
  np.testing.assert_array_equal(s0, [1, 1, 4])
  np.testing.assert_array_equal(s1, [1, 4, 7])
  # an empty matrix: every range is empty
  s0, s1 = T.clamped_splits([-1, 3, 5], 0)
  assert not s0.any() and not s1.any()


def test_truth_for_explicit_ranges():
  emb = np.arange(12, dtype=np.float32).reshape(6, 2)
  rs = [0, 2, 2, 5]
  for a, b in zip(T.truth_forward(rs, emb, [1, 1]), T.truth_forward_ranges(rs[:-1], rs[1:], emb, [1, 1])):
    np.testing.assert_array_equal(T.bits(a), T.bits(b))
  # overlapping and backwards ranges: rows 1-3, then 0-1, then an inverted (empty) range
  (got,) = T.truth_forward_ranges([1, 0, 4], [4, 2, 3], emb, [2])
  np.testing.assert_array_equal(got, [[2 + 4 + 6, 3 + 5 + 7], [0 + 2, 1 + 3], [0, 0]])
  g = [np.array([[1.], [2.], [3.]], np.float32)]
  np.testing.assert_array_equal(T.truth_gradient_ranges([1, 2, 2], [2, 2, 4], 6, g),
                                T.truth_gradient([1, 2, 2, 4], 6, g))
  with pytest.raises(AssertionError, match="overlapping"):
    T.truth_gradient_ranges([0, 1], [2, 3], 4, [np.ones((2, 1), np.float32)])


def test_the_planner_constants_the_cases_were_sized_for():
  assert T.kernel_constants() == {"kSplitInlineUnits": 32, "kSplitInlineSlices": 96, "kSplitUnitCols": 64,
                                  "kSplitDeep": 16}


def test_plan_of_the_lane_group_case():
  every = {(v, g) for v in (False, True) for g in range(7)}
  p = T.plan_of(T.lane_group_case("inline"))
  assert (p["n_units"], p["n_slices"], p["ext"]) == (21, 23, False) and T.lane_kinds(p) == every
  assert [f["vec"] for f in p["features"]] == [True] * 12 + [False] * 9
  assert p["features"][0]["units"] == [(0, 4, 0)] and p["features"][11]["units"] == [(0, 256, 6)]
  assert p["features"][12]["units"] == [(0, 1, 0)] and p["features"][20]["units"] == [(0, 64, 6)]
  p = T.plan_of(T.lane_group_case("ext_units"))
  assert (p["n_units"], p["n_slices"], p["ext"]) == (33, 35, True) and T.lane_kinds(p) == every
  p = T.plan_of(T.lane_group_case("ext_slices"))
  assert (p["n_units"], p["n_slices"], p["ext"]) == (23, 123, True) and T.lane_kinds(p) == every
  assert p["features"][21] == {"vec": True, "units": [(0, 256, 6), (256, 144, 6)]}
  # bs = 37: a 64-lane unit has 4 lane groups per workgroup
  assert p["need"] == 10 and p["gx"] == 10
  # nothing is float4 once a pointer is not aligned
  assert not any(f["vec"] for f in T.plan_of(T.lane_group_case("inline"), aligned=False)["features"])


def test_plan_of_the_shapes_the_other_cases_rely_on():
  # a feature of 100 slices of 1: 2 scalar units, the tables in device memory by slices alone
  p = T.plan([100], [[1] * 100], True, 37)
  assert p["features"] == [{"vec": False, "units": [(0, 64, 6), (64, 36, 6)]}] and p["ext"]
  # the wide case: col0 > 0 and a narrower last unit in both lane kinds, inline
  p = T.plan_of(T.wide_case())
  assert [f["vec"] for f in p["features"]] == [True, True, False, False, False] and not p["ext"]
  assert p["features"][0]["units"] == [(0, 256, 6), (256, 4, 0)]
  assert p["features"][1]["units"] == [(0, 256, 6), (256, 256, 6), (512, 4, 0)]
  assert p["features"][2]["units"] == [(0, 64, 6), (64, 1, 0)]
  assert p["features"][3]["units"] == [(0, 64, 6), (64, 64, 6), (128, 1, 0)]
  assert p["features"][4]["units"] == [(0, 64, 6), (64, 64, 6), (128, 64, 6), (192, 8, 3)]
  # grid stride at a small shape: 560 units, 64 row blocks against a need of 150
  dims, slices = [321] * 60 + [1028] * 40, [[100, 221]] * 60 + [[512, 516]] * 40
  p = T.plan(dims, slices, True, 600)
  assert (p["n_units"], p["ext"], p["gx"], p["need"]) == (560, True, 64, 150)
  assert p["features"][0]["units"][-1] == (320, 1, 0) and p["features"][60]["units"][-1] == (1024, 4, 0)
  assert not p["features"][0]["vec"] and p["features"][60]["vec"]
  # more than 65 535 units: unit 65 535 is feature 1 023's last
  p = T.plan([4096] * 1025, [[4095, 1]] * 1025, True, 2)
  assert p["n_units"] == 65600 and p["ext"] and p["gx"] == 1
  units = [(i, f["vec"]) + u for i, f in enumerate(p["features"]) for u in f["units"]]
  assert units[65535] == (1023, False, 4032, 64, 6) and units[65536] == (1024, False, 0, 64, 6)
  # a feature falls back on its own: a misaligned pointer or a slice start that is no multiple of 4
  p = T.plan([32] * 5, [[8, 24], [8, 24], [8, 24], [6, 26], [8, 24]], [True, False, False, True, True], 37)
  assert [f["vec"] for f in p["features"]] == [True, False, False, False, True]
  assert p["features"][0]["units"] == [(0, 32, 3)] and p["features"][1]["units"] == [(0, 32, 5)]
  # batch edges: float4 dim 256 has 4 lane groups per workgroup, scalar dim 1 has 256
  for bs, gx in ((1, 1), (3, 1), (4, 1), (5, 2), (255, 64), (256, 64), (257, 65)):
    p = T.plan([256, 1], [[256], [1]], True, bs)
    assert p["gx"] == gx and T.lane_kinds(p) == {(True, 6), (False, 0)}


def test_the_lane_group_data_is_order_sensitive_at_every_length():
  """Reversing the rows inside a range changes the bits of at least one column of every range with 3 or more
  addends, for every feature at least 8 columns wide (a narrower feature can hold a range whose few columns each
  have one dominant addend): the data tells a re-associated chain from the sequential one at every length the
  16-deep loop and its 4-wide tail distinguish."""
  lengths = set()
  for f in T.lane_group_case("ext_slices"):
    rs, emb = f["row_splits"].astype(np.int64), f["emb"]
    if emb.shape[1] < 8:
      continue
    rev = emb.copy()
    for b in range(rs.size - 1):
      rev[rs[b]:rs[b + 1]] = emb[rs[b]:rs[b + 1]][::-1]
    a = np.concatenate(T.truth_forward(rs, emb, f["slice_dims"]), 1)
    r = np.concatenate(T.truth_forward(rs, rev, f["slice_dims"]), 1)
    differs = (T.bits(a) != T.bits(r)).any(axis=1)
    lens = np.diff(rs)
    zeros = np.array([not emb[rs[b]:rs[b + 1]].any() for b in range(lens.size)])   # (the rows of -0.0)
    check = (lens >= 3) & ~zeros
    assert differs[check].all(), (emb.shape[1], lens[check & ~differs])
    lengths.update(int(x) for x in lens[check])
  assert lengths == {x for x in T.LENGTH_CYCLE if x >= 3}
