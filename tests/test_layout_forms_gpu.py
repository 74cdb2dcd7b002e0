"""fused_embedding_to_layout: every kernel form ``layout_launch`` (csrc/mhte.hip) chooses on the host (-m gpu).

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = _lib.MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS
CYCLE = [4, 12, 260, 16, 64]      # slice widths of cases (d) .. (f): 1, 3, 65, 4, 16 float4 columns


# ===================================================================== helpers
def one_fid_case(seed, batch, strides, layouts, poolings=(OL.SUM, OL.MEAN)):
  """One fid per feature instance, distinct rows.  ``strides[i]``: floats per row of feature i's own matrix,
  which has batch + 3 + i % 4 rows; batch row b of feature i names row perm_i[b].  ``layouts``: name ->
  (out_type, [(feature, start, end), ...], row floats of a CONCAT output or None = exactly the slices).
  -> dict(cfgs, batch, embs, fid_offset, feature_offset, nfl_offset) as oracle.layout's cases."""
  rng = np.random.default_rng(seed)
  n = len(strides)
  names = ["f%03d" % i for i in range(n)]
  feats = {names[i]: OL.FeatureConfig("t%03d" % i, poolings[i % len(poolings)], [int(strides[i])], 0) for i in range(n)}
  outs = {}
  for ln, (out_type, slices, width) in layouts.items():
    scs = [OL.SliceConfig(names[f], s, e) for f, s, e in slices]
    oc = OL.infer_shape(scs, out_type)
    if width is not None:
      assert out_type == OL.CONCAT and width >= oc.shape[0][1]
      oc = OL.OutConfig(scs, out_type, [[-1, int(width)]])
    outs[ln] = oc
  embs, fid_offset = [], []
  for i in range(n):
    rows = batch + 3 + i % 4
    embs.append(rng.standard_normal((rows, int(strides[i]))).astype(np.float32))
    perm = rng.permutation(rows)[:batch]
    assert not np.array_equal(perm, np.arange(batch))
    fid_offset += [(i << 32) | int(r) for r in perm]
  return {"cfgs": OL.FeatureConfigs(feats, outs), "batch": batch, "embs": embs,
          "fid_offset": np.array(fid_offset, dtype=np.uint64),
          "feature_offset": np.arange(n * batch, dtype=np.int32),
          "nfl_offset": (np.arange(n, dtype=np.uint32) * np.uint32(batch)).astype(np.uint32)}


def concat_case(seed, batch, widths, pad=0):
  """One CONCAT layout of one slice per feature: feature i's slice is [4 * (i % 3), .. + widths[i]) of a row
  4 floats wider than that; ``pad``: floats of the output row behind the last slice."""
  starts = [4 * (i % 3) for i in range(len(widths))]
  strides = [s + w + 4 for s, w in zip(starts, widths)]
  slices = [(i, s, s + w) for i, (s, w) in enumerate(zip(starts, widths))]
  return one_fid_case(seed, batch, strides, {"vec": (OL.CONCAT, slices, sum(widths) + pad)})


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
def _case_h_parts(first, n=3):
  """Features ``first`` .. ``first + n - 1`` with rows 24 floats wide, slice_dims [4, 16, 4]: [0, 4) to a NONE
  tensor each, [4, 20) to a CONCAT, [20, 24) to a STACK."""
  ids = range(first, first + n)
  return ([24] * n, [(i, 0, 4) for i in ids], [(i, 4, 20) for i in ids], [(i, 20, 24) for i in ids])


def build_case(cid):
  if cid == "a":        # 32 x 256 floats = 2048 float4 columns, exact width: rows kernel, whole rows, no fill
    return concat_case(1, 19, [256] * 32)
  if cid == "b":        # 2049 columns: past the column table -> fill + layout_copy_kernel
    return concat_case(2, 19, [256] * 32 + [4])
  if cid == "bh":       # (b) with (h)'s three-way split features in the same launch: start 4 and 20, stride 24
    c = concat_case(2, 19, [256] * 32 + [4])
    strides, lead, mid, tail = _case_h_parts(33)
    vec = c["cfgs"].out_configs["vec"]
    base = [(i, sc.start, sc.end) for i, sc in enumerate(vec.slice_configs)]
    return one_fid_case(3, 19, [sum(fc.slice_dims) for _, fc in sorted(c["cfgs"].feature_configs.items())] + strides,
                        {"lead": (OL.NONE, lead, None), "stk": (OL.STACK, tail, None),
                         "vec": (OL.CONCAT, base + mid, None)})
  if cid in ("c4", "c8"):   # 2044 columns of slices + 4 (covered: 2048) or 8 (2052: the fill stays) of padding
    return concat_case(4, 19, [256] * 31 + [240], pad=16 if cid == "c4" else 32)
  if cid == "d":        # 48 slices, exact width: one launch, whole rows
    return concat_case(5, 33, [CYCLE[i % 5] for i in range(48)])
  if cid == "e":        # ... 4 floats wider: 48 slices + 1 zero run = 49 tasks -> fill + rows kernel
    return concat_case(5, 33, [CYCLE[i % 5] for i in range(48)], pad=4)
  if cid == "f":        # 49 slices: two rows launches behind the fill
    return concat_case(6, 33, [CYCLE[i % 5] for i in range(49)])
  if cid == "g":        # 48 x 172 floats = 2064 columns (copy launch), then 5 x 16 (rows launch), one call
    return concat_case(7, 19, [172] * 48 + [16] * 5)
  if cid == "h":        # one feature row to three layouts from starts 0, 4, 20: rows form, whole rows
    strides, lead, mid, tail = _case_h_parts(0)
    return one_fid_case(8, 33, strides, {"lead": (OL.NONE, lead, None), "stk": (OL.STACK, tail, None),
                                         "vec": (OL.CONCAT, mid, None)})
  if cid == "i":        # 70 matrices: pointer tables, and 70 slices: two rows launches
    return concat_case(9, 19, [8] * 70)
  if cid == "k":        # widths that are no float4s: layout_kernel<true> / <false> (float atomics, one addend)
    return concat_case(10, 33, [3, 5, 8, 5, 3, 8, 8])
  raise KeyError(cid)


CASES = ["a", "b", "bh", "c4", "c8", "d", "e", "f", "g", "h", "i", "k"]


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
def _slice(feature, start, dim, out_index, out_offset, row, pooling=OL.SUM, out_type=OL.NONE):
  s = _lib.LayoutSlice()
  s.feature_idx, s.start, s.dim, s.pooling, s.max_sequence_length = feature, start, dim, pooling, 0
  s.out_type, s.out_index, s.out_offset, s.out_row_floats = out_type, out_index, out_offset, row
  return s


def _hand_case(batch=19):
  """Three features with rows 28 floats wide, and a fourth named feature list without instances."""
  c = one_fid_case(12, batch, [28, 28, 28], {"x": (OL.NONE, [(0, 0, 4)], None)})
  c["nfl_offset"] = np.append(c["nfl_offset"], np.uint32(3 * batch)).astype(np.uint32)
  return c


HAND = {
    # zero runs in the middle ([16, 32)) and at the end ([48, 64)) of a 64-float row: whole rows, no fill
    "gaps": lambda B: ([_slice(0, 4, 16, 0, 0, 64), _slice(1, 8, 16, 0, 32, 64)], [B * 64]),
    # [0, 16) and [8, 24) of a 32-float row: the fill stays ([24, 32)), the later slice's values stay on [8, 16)
    "overlap": lambda B: ([_slice(0, 4, 16, 0, 0, 32), _slice(1, 8, 16, 0, 8, 32)], [B * 32]),
    # ... the same with the earlier slice listed later
    "overlap_reversed": lambda B: ([_slice(1, 8, 16, 0, 8, 32), _slice(0, 4, 16, 0, 0, 32)], [B * 32]),
    # an output of batch + 3 rows: the fill stays, the last three rows are zeros
    "rows_beyond_batch": lambda B: ([_slice(0, 4, 16, 0, 0, 16)], [(B + 3) * 16]),
    # output 0 tiled with a gap (left to the rows launch), output 1 overlapping (behind the fill); on output 1
    # an ABSENT list's slice lies over the first slice: it writes nothing, the first slice's values stay
    "two_outputs": lambda B: ([_slice(0, 0, 8, 0, 0, 24), _slice(1, 4, 16, 1, 0, 24), _slice(2, 12, 8, 0, 16, 24),
                               _slice(2, 0, 12, 1, 8, 24), _slice(3, 0, 8, 1, 4, 24)], [B * 24, B * 24]),
}


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


# ===================================================================== the overlap rule (gradient)
def overlap_case(batch=33):
  """``vec`` = CONCAT of f[4:20] and ``ffm`` = STACK of the same f[4:20] for three features, ``part`` = CONCAT
  of f[12:24]: elements [4, 12) of a row have two addends, [12, 20) three, [20, 24) one."""
  sl = lambda a, b: [(i, a, b) for i in range(3)]  # noqa: E731
  return one_fid_case(13, batch, [28, 28, 28], {"ffm": (OL.STACK, sl(4, 20), None), "part": (OL.CONCAT, sl(12, 24), None),
                                                "vec": (OL.CONCAT, sl(4, 20), None)})


def test_flagged_gradient_of_a_feature_fed_to_two_layouts_is_the_sum():
  """One fid per instance and distinct rows, but the same columns of a feature go to two layouts: the
  flagged gradient must be the sum (the form taken without the flag), not the last plain store."""
  c = overlap_case()
  d = dev_inputs(c)
  check_forward(c, d, what="overlap")
  check_grad(c, d, what="overlap")


# ===================================================================== the general form, more than 48 slices
def general_case(seed=14, batch=9, n=60):
  """60 features over 3 matrices (inline kernel arguments), SUM or MEAN with 0 .. 3 fids per instance: one
  ADDN layout of all 60 one-wide slices (continues over two launches), one CONCAT layout of all 60
  four-wide slices."""
  rng = np.random.default_rng(seed)
  names = ["f%03d" % i for i in range(n)]
  feats = {names[i]: OL.FeatureConfig("t%d" % (i % 3), OL.SUM if i % 2 else OL.MEAN, [1, 4, 1], 0) for i in range(n)}
  outs = {"bias": OL.infer_shape([OL.SliceConfig(nm, 0, 1) for nm in names], OL.ADDN),
          "vec": OL.infer_shape([OL.SliceConfig(nm, 1, 5) for nm in names], OL.CONCAT)}
  embs = [rng.standard_normal((40, 6)).astype(np.float32) for _ in range(3)]
  fid_offset, feature_offset, nfl_offset = [], [], []
  for i in range(n):
    nfl_offset.append(len(feature_offset))
    for _ in range(batch):
      feature_offset.append(len(fid_offset))
      for _ in range(int(rng.integers(0, 4))):
        fid_offset.append(((i % 3) << 32) | int(rng.integers(0, 40)))
  return {"cfgs": OL.FeatureConfigs(feats, outs), "batch": batch, "embs": embs,
          "fid_offset": np.array(fid_offset, dtype=np.uint64), "feature_offset": np.array(feature_offset, dtype=np.int32),
          "nfl_offset": np.array(nfl_offset, dtype=np.uint32)}


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
def mixed_case(batch=7, seed=1):
  """The configuration of test_fused_embedding_to_layout_forward_and_grad (tests/test_boundary_gpu.py): five
  features over three matrices, 0 .. 5 fids, a SHARED and an absent list, all four output types, FIRSTN."""
  rng = np.random.default_rng(seed)
  F, S_ = OL.FeatureConfig, OL.SliceConfig
  feats = {"f_a": F("t0", OL.SUM, [1, 8], 0), "f_b": F("t1", OL.MEAN, [1, 8], 0), "f_c": F("t2", OL.FIRSTN, [1, 4], 3),
           "f_d": F("t0", OL.SUM, [1, 8], 0), "f_e": F("t1", OL.SUM, [1, 8], 0)}
  outs = {
      "bias": OL.OutConfig([S_("f_a", 0, 1), S_("f_b", 0, 1), S_("f_d", 0, 1), S_("f_e", 0, 1)], OL.ADDN, [[-1, 1]]),
      "vec": OL.OutConfig([S_("f_a", 1, 9), S_("f_b", 1, 9), S_("f_d", 1, 9)], OL.CONCAT, [[-1, 24]]),
      "ffm": OL.OutConfig([S_("f_b", 1, 9), S_("f_a", 1, 9)], OL.STACK, [[-1, 2, 8]]),
      "seq": OL.OutConfig([S_("f_c", 1, 5)], OL.NONE, [[-1, 3, 4]]),
      "two": OL.OutConfig([S_("f_a", 1, 9), S_("f_b", 0, 1)], OL.NONE, [[-1, 8], [-1, 1]]),
  }
  embs = [rng.standard_normal((50, 9)).astype(np.float32), rng.standard_normal((40, 9)).astype(np.float32),
          rng.standard_normal((30, 5)).astype(np.float32)]
  mat_of = {"f_a": 0, "f_b": 1, "f_c": 2, "f_d": 0, "f_e": 1}
  fid_offset, feature_offset, nfl_offset = [], [], []
  for name in sorted(feats):
    shared, absent = name == "f_d", name == "f_e"
    nfl_offset.append(len(feature_offset) | ((1 << 31) if shared else 0))
    for _ in range(0 if absent else (1 if shared else batch)):
      feature_offset.append(len(fid_offset))
      for _ in range(int(rng.integers(0, 6))):
        m = mat_of[name]
        fid_offset.append((m << 32) | int(rng.integers(0, embs[m].shape[0])))
  return {"cfgs": OL.FeatureConfigs(feats, outs), "batch": batch, "embs": embs,
          "fid_offset": np.array(fid_offset, dtype=np.uint64), "feature_offset": np.array(feature_offset, dtype=np.int32),
          "nfl_offset": np.array(nfl_offset, dtype=np.uint32)}


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
