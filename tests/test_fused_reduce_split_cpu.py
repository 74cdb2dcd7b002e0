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
