"""The cases of tests/test_layout_forms_gpu.py (run on the device, bit for bit against the oracle) and of
tests/test_layout_plan_cpu.py (the planned launch sequence of the same calls): pure numpy, no device."""
import numpy as np

from oracle import layout as OL
from monolith_amd import _lib

CYCLE = [4, 12, 260, 16, 64]      # slice widths of cases (d) .. (f): 1, 3, 65, 4, 16 float4 columns


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


def overlap_case(batch=33):
  """``vec`` = CONCAT of f[4:20] and ``ffm`` = STACK of the same f[4:20] for three features, ``part`` = CONCAT
  of f[12:24]: elements [4, 12) of a row have two addends, [12, 20) three, [20, 24) one."""
  sl = lambda a, b: [(i, a, b) for i in range(3)]  # noqa: E731
  return one_fid_case(13, batch, [28, 28, 28], {"ffm": (OL.STACK, sl(4, 20), None), "part": (OL.CONCAT, sl(12, 24), None),
                                                "vec": (OL.CONCAT, sl(4, 20), None)})


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
