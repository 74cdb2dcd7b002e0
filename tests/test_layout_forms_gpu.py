"""fused_embedding_to_layout: every kernel form ``layout_plan`` (csrc/mhte_layout_plan.h) chooses on the host (-m gpu).

The op has more host-chosen forms than any other: ``layout_rows_kernel`` with or without the zero fill in
front, ``layout_copy_kernel``, ``layout_kernel`` (general form and float-atomic gradient), the grouped
gradient, inline arguments or uploaded pointer tables, one launch or several of up to 48 slices.  The
reference's own tests (tests/test_boundary_gpu.py) cover the general form; this module covers the forms the
training path takes under MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS and the launch splits of the general form.

Shapes.  The one-fid cases give every feature a matrix of its own with MORE rows than the batch; a batch
row's fid names a random permutation of those rows (a kernel that took the batch row for the row index
fails), slices start at column 0, 4 or 8 of a row that is wider than the slice (a kernel that ignored
``start`` or took the slice width for the row stride fails).  Batch is 19 or 33: two or three 16-row
workgroups of ``layout_rows_kernel``, the last one partial.

Every forward goes through ``raw_forward``: the C ABI on output buffers this module owns and fills with
NaN before the call, so a float the call does not write is seen.  ``raw_grad`` does the same with the
gradient buffers (the op zero-fills them: rows no fid names must come out exactly 0).

Bars.  In these shapes every forward value is a copy (or the reference's sequential fp32 sum) and every
gradient element has at most two addends, so every comparison is bit for bit: flag on against flag off,
against ``oracle.layout`` (``layout_model`` / ``layout_grad_model(acc_dtype=float32)`` /
``layout_model_slices``), and against a second identical call.  Only the float-atomic child process
compares at the tolerance of the test whose case it repeats.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import layout as OL  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd.distribution_ops import _layout_plan, _ptr_array, _stream, check, vp  # noqa: E402
from layout_cases import (CASES, CYCLE, HAND, _hand_case, _slice, build_case, concat_case, general_case,  # noqa: E402,F401
                          mixed_case, one_fid_case, overlap_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = _lib.MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS


# ===================================================================== helpers
def dev_inputs(c, embs=None):
  """The case's index arrays (and, unless given, its matrices) on the device."""
  return {"embs": [torch.from_numpy(e).cuda() for e in c["embs"]] if embs is None else embs,
          "fo": torch.from_numpy(c["fid_offset"].view(np.int64)).cuda(),
          "fe": torch.from_numpy(c["feature_offset"]).cuda(),
          "nf": torch.from_numpy(c["nfl_offset"].view(np.int32)).cuda(), "batch": int(c["batch"])}


def slice_array(slices):
  return slices if isinstance(slices, C.Array) else (_lib.LayoutSlice * len(slices))(*slices)


def _call(forward, d, mats, slices, bufs, flag):
  """mhte_embedding_to_layout(_grad) as it is: ``mats`` the matrices (forward: read; gradient: the gradient
  buffers, written), ``bufs`` the layouts' tensors (forward: written; gradient: their gradients, read)."""
  for t in list(mats) + list(bufs):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
  stride = (C.c_int32 * len(mats))(*[int(e.shape[1]) for e in mats])
  count = (C.c_int64 * len(mats))(*[e.numel() for e in mats])
  lens = (C.c_int64 * len(bufs))(*[b.numel() for b in bufs])
  sl = slice_array(slices)
  fn = _lib.lib().mhte_embedding_to_layout if forward else _lib.lib().mhte_embedding_to_layout_grad
  check(fn(_ptr_array(mats), stride, count, len(mats), vp(d["fo"]), d["fo"].numel(), vp(d["fe"]), d["fe"].numel(),
           vp(d["nf"]), d["nf"].numel(), d["batch"], sl, len(sl), _ptr_array(bufs), lens, len(bufs), int(flag),
           _stream()))


def nan_like(n_or_tensor):
  if isinstance(n_or_tensor, torch.Tensor):
    return torch.full_like(n_or_tensor, float("nan"))
  return torch.full((int(n_or_tensor),), float("nan"), dtype=torch.float32, device="cuda")


def raw_forward(d, slices, out_lens, flag, outs=None):
  """-> flat numpy outputs; the buffers (``outs``: the caller's own, e.g. misaligned ones) hold NaN before."""
  outs = [nan_like(n) for n in out_lens] if outs is None else outs
  for o, n in zip(outs, out_lens):
    assert o.numel() == n
    o.fill_(float("nan"))
  _call(True, d, d["embs"], slices, outs, flag)
  return [o.cpu().numpy().reshape(-1) for o in outs]


def raw_grad(d, slices, tensors_grad, flag, grads=None):
  """-> gradients of the matrices (numpy, the matrices' shapes); the buffers hold NaN before."""
  grads = [nan_like(e) for e in d["embs"]] if grads is None else grads
  for g in grads:
    g.fill_(float("nan"))
  _call(False, d, grads, slices, tensors_grad, flag)
  return [g.cpu().numpy() for g in grads]


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def same_bits(got, want, what=""):
  assert len(got) == len(want), what
  for k, (g, w) in enumerate(zip(got, want)):
    assert not np.isnan(g).any(), "%s: tensor %d keeps NaN in %d floats" % (what, k, int(np.isnan(g).sum()))
    np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s: tensor %d" % (what, k))


def planned(c):
  slices, shapes = _layout_plan(c["cfgs"], c["batch"])
  return slices, shapes, [int(np.prod(sh)) for sh in shapes]


def output_grads(shapes, seed):
  rng = np.random.default_rng(1000 + seed)
  return [rng.standard_normal(sh).astype(np.float32) for sh in shapes]


def unnamed_rows_are_zero(c, grads):
  """Rows of a matrix that no fid names (every matrix has some) hold exactly +0."""
  named = [set() for _ in c["embs"]]
  for v in c["fid_offset"].tolist():
    if (v >> 32) < len(named):
      named[v >> 32].add(v & 0xffffffff)
  seen = 0
  for m, g in enumerate(grads):
    rest = [r for r in range(g.shape[0]) if r not in named[m]]
    seen += len(rest)
    assert not bits(g[rest]).any(), "matrix %d: a row no fid names is not +0" % m
  assert seen > 0


def check_forward(c, d=None, flags=(FLAG, 0), what=""):
  d = dev_inputs(c) if d is None else d
  slices, _, lens = planned(c)
  want = OL.layout_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"], c["cfgs"])
  for flag in flags:
    for rep in range(2):
      same_bits(raw_forward(d, slices, lens, flag), want, "%s forward flag %d call %d" % (what, flag, rep))
  return want


def check_grad(c, d=None, flags=(FLAG, 0), seed=0, what=""):
  d = dev_inputs(c) if d is None else d
  slices, shapes, _ = planned(c)
  tg = output_grads(shapes, seed)
  dtg = [torch.from_numpy(t).cuda() for t in tg]
  want = OL.layout_grad_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"],
                              c["cfgs"], tg, acc_dtype=np.float32)
  assert sum(int((w != 0).sum()) for w in want) > 0
  for flag in flags:
    for rep in range(2):
      got = raw_grad(d, slices, dtg, flag)
      same_bits(got, want, "%s gradient flag %d call %d" % (what, flag, rep))
      unnamed_rows_are_zero(c, got)


# ===================================================================== the flagged cases (a) .. (k)
@pytest.mark.parametrize("cid", CASES)
def test_flagged_forms_forward_and_gradient(cid):
  """Cases (a) .. (k) of the module's table (``build_case``): forward and gradient with the flag, without it,
  each twice, bit for bit against the oracle; no NaN of the caller's fill survives the forward; the
  gradient's unnamed rows are +0."""
  c = build_case(cid)
  slices, _, _ = planned(c)
  cols = sum(s.dim // 4 for s in slices)
  expect = {"a": (32, 2048), "b": (33, 2049), "bh": (42, 2067), "c4": (32, 2044), "c8": (32, 2044), "d": (48, 870),
            "e": (48, 870), "f": (49, 874), "g": (53, 2084), "h": (9, 18), "i": (70, 140), "k": (7, 8)}[cid]
  assert (len(slices), cols) == expect       # (the shape is the one the case is named for)
  assert all(s.start in (0, 4, 8, 20) for s in slices) and any(s.start > 0 for s in slices)
  d = dev_inputs(c)
  check_forward(c, d, what=cid)
  check_grad(c, d, what=cid)


def test_shared_list_absent_list_and_a_matrix_index_past_the_list_forward():
  """(j), forward only: f000 ordinary, f001 SHARED (bit 31 of nfl_offset, one instance for the whole batch),
  f002 a list with no instances, f003 ordinary with one fid whose matrix index is n_emb.  One fid per
  instance still holds, so the flagged call writes whole rows: the absent list's columns and that fid's
  row are zeros over the NaN fill, the shared row repeats in every batch row; the general form agrees."""
  rng = np.random.default_rng(11)
  batch, w = 19, 16
  names = ["f%03d" % i for i in range(4)]
  feats = {n: OL.FeatureConfig("t", OL.SUM, [w + 8], 0) for n in names}
  cfgs = OL.FeatureConfigs(feats, {"vec": OL.infer_shape([OL.SliceConfig(n, 4, 4 + w) for n in names], OL.CONCAT)})
  embs = [rng.standard_normal((batch + 4, w + 8)).astype(np.float32) for _ in range(3)]   # (f002 has no matrix)
  mat = {0: 0, 1: 1, 3: 2}
  fid_offset, nfl_offset = [], []
  for i in range(4):
    shared = i == 1
    nfl_offset.append(len(fid_offset) | ((1 << 31) if shared else 0))
    if i == 2:
      continue
    perm = rng.permutation(batch + 4)
    for b in range(1 if shared else batch):
      m = len(embs) if (i == 3 and b == 5) else mat[i]
      fid_offset.append((m << 32) | int(perm[b]))
  c = {"cfgs": cfgs, "batch": batch, "embs": embs, "fid_offset": np.array(fid_offset, dtype=np.uint64),
       "feature_offset": np.arange(len(fid_offset), dtype=np.int32), "nfl_offset": np.array(nfl_offset, dtype=np.uint32)}
  want = check_forward(c, what="j")[0]
  assert not want[:, 2 * w:3 * w].any() and not want[5, 3 * w:].any() and want[4, 3 * w:].all()
  assert (want[:, w:2 * w] == want[0, w:2 * w]).all() and want[0, w:2 * w].all()


# ===================================================================== hand-written slices, forward
@pytest.mark.parametrize("hid", sorted(HAND))
def test_hand_written_slices_forward(hid):
  """The whole-rows decision on slices no configuration produces, through the raw caller: no NaN left anywhere
  and equality with ``layout_model_slices`` (later slices over earlier ones), with the flag, without, twice."""
  c = _hand_case()
  slices, lens = HAND[hid](c["batch"])
  d = dev_inputs(c)
  want = OL.layout_model_slices(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"],
                                slices, lens)
  assert all(w.any() for w in want) and any((w == 0).any() for w in want)
  if hid.startswith("overlap"):
    later = 1 if hid == "overlap" else 0     # (matrix of the later slice: its columns fill [8, 16))
    w0 = want[0].reshape(c["batch"], 32)
    row = c["embs"][later][int(c["fid_offset"][later * c["batch"]]) & 0xffffffff]
    np.testing.assert_array_equal(w0[0, 8:16], row[8:16] if later == 1 else row[12:20])
  for flag in (FLAG, 0):
    for rep in range(2):
      same_bits(raw_forward(d, slices, lens, flag), want, "%s flag %d call %d" % (hid, flag, rep))


@pytest.mark.parametrize("forward", [True, False])
def test_an_invalid_slice_is_refused_before_anything_is_written(forward):
  """Batch 19, the five slices of ``two_outputs`` and a sixth that does not fit its output ([16, 32) of a 24-float
  row): InvalidArgument, and every float of the written side (the outputs; the gradient buffers) is still the NaN
  it held — no zero fill, no launch of the slices in front of the bad one."""
  c = _hand_case()
  slices, lens = HAND["two_outputs"](c["batch"])
  slices = slices + [_slice(0, 0, 16, 0, 16, 24)]
  d = dev_inputs(c)
  outs = [nan_like(n) for n in lens]
  grads = [nan_like(e) for e in d["embs"]]
  for flag in (FLAG, 0):
    with pytest.raises(_lib.InvalidArgumentError, match="slice 5 does not fit its output"):
      if forward:
        _call(True, d, d["embs"], slices, outs, flag)
      else:
        _call(False, d, grads, slices, [torch.ones_like(o) for o in outs], flag)
    for t in outs if forward else grads:
      assert bool(torch.isnan(t).all())


# ===================================================================== the overlap rule (gradient)
def test_flagged_gradient_of_a_feature_fed_to_two_layouts_is_the_sum():
  """One fid per instance and distinct rows, but the same columns of a feature go to two layouts: the
  flagged gradient must be the sum (the form taken without the flag), not the last plain store."""
  c = overlap_case()
  d = dev_inputs(c)
  check_forward(c, d, what="overlap")
  check_grad(c, d, what="overlap")


# ===================================================================== the general form, more than 48 slices
def test_general_form_with_sixty_slices_per_layout():
  """No flag.  The ADDN layout's 60 slices take two launches with inline arguments (the second one continues
  from the stored sums), the CONCAT's 60 likewise; the grouped gradient walks 120 slices.  Forward against
  ``layout_model``, gradient against the sequential fp32 ``layout_grad_model``, bit for bit, twice."""
  c = general_case()
  d = dev_inputs(c)
  slices, shapes, lens = planned(c)
  assert len(slices) == 120 and len(c["embs"]) == 3 and shapes == [[9, 1], [9, 240]]
  want = OL.layout_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"], c["cfgs"])
  tg = output_grads(shapes, 2)
  dtg = [torch.from_numpy(t).cuda() for t in tg]
  gwant = OL.layout_grad_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"], c["cfgs"],
                               tg, acc_dtype=np.float32)
  for rep in range(2):
    got = raw_forward(d, slices, lens, 0)
    for g, w in zip(got, want):
      assert not np.isnan(g).any()
      np.testing.assert_array_equal(g, w.reshape(-1))
    for g, w in zip(raw_grad(d, slices, dtg, 0), gwant):
      np.testing.assert_array_equal(g, w)


# ===================================================================== MHTE_POOL_ATOMICS=1 (a child process)
def atomic_child_main():
  """Runs in the child: the layout gradient in its float-atomic form (``layout_kernel<false>``) on the mixed
  batch-7 case and on the 60-feature case, against the float64 sums at that test's tolerance."""
  assert os.environ.get("MHTE_POOL_ATOMICS") == "1"
  for what, c in (("mixed", mixed_case()), ("sixty", general_case())):
    d = dev_inputs(c)
    slices, shapes, _ = planned(c)
    tg = output_grads(shapes, 3)
    dtg = [torch.from_numpy(t).cuda() for t in tg]
    want = OL.layout_grad_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"],
                                c["cfgs"], tg)
    assert sum(int((w != 0).sum()) for w in want) > 100
    for g, w in zip(raw_grad(d, slices, dtg, 0), want):
      np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-5, err_msg=what)
  print("LAYOUT-ATOMIC-FORM-OK")


CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_layout_forms_gpu as T
T.atomic_child_main()
"""


def test_layout_gradient_in_the_float_atomic_form():
  """MHTE_POOL_ATOMICS is read once per process: a fresh child with its own time limit.  A child that ends
  with a fault status ends the session — nothing more is started on the GPU behind a fault."""
  env = dict(os.environ, MHTE_POOL_ATOMICS="1", MHTE_NO_REBUILD="1")
  try:
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=240)
  except subprocess.TimeoutExpired:
    pytest.exit("the float-atomic child ran into its time limit: nothing more is started on the GPU", returncode=3)
  if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
    pytest.exit("the float-atomic child ended with status %d: nothing more is started on the GPU\n%s" %
                (r.returncode, r.stderr[-2000:]), returncode=3)
  assert r.returncode == 0 and "LAYOUT-ATOMIC-FORM-OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
