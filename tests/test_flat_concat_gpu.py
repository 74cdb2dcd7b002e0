"""GPU suite of the aligned flat concat / split (monolith_amd/distribution_ops.py, csrc/mhte_flat_kernels.h).
Every comparison is on the raw bits against the numpy restatement (tests/flat_concat_truth.py): each output
element is one rounded float32 product and, on the fp16 wire, one IEEE conversion — no tolerance."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ops_truth as CT  # noqa: E402
import flat_concat_truth as T  # noqa: E402
from monolith_amd import clip_ops  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32 = np.float16, np.float32
TORCH_OF = {F32: torch.float32, F16: torch.float16}
FILL = 0x7fc12345   # a NaN pattern: what a buffer holds before the concat writes it


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unaligned(a):
  """The same values in a view that starts one float into its storage: a pointer that is not 16-byte aligned."""
  buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
  v = buf[1:1 + a.size]
  v.copy_(torch.from_numpy(a.ravel()))
  assert v.data_ptr() % 16 == 4
  return v.view(a.shape)


@functools.lru_cache(maxsize=None)
def host_set(name):
  if name == "edges":
    return T.set_edges()
  if name == "fp16":
    return T.set_fp16_edges()
  return T.set_seeded(int(name), seed=int(name))   # "129", "155"


def prefilled(total, wire):
  if wire is F32:
    return torch.full((total,), FILL, dtype=torch.int32, device=DEV).view(torch.float32)
  return torch.full((total,), 0x7e55, dtype=torch.int16, device=DEV).view(torch.float16)


def check_concat(hs, ts, scale, wire, align=16, scale_arg=None):
  """One concat into a NaN-filled ``out`` against the truth, padding included -> the device buffer."""
  exp = T.concat(hs, scale, wire, align)
  out = prefilled(exp.size, wire)
  got = D.aligned_flat_concat(ts, scale=scale if scale_arg is None else scale_arg, wire_dtype=TORCH_OF[wire],
                              align=align, out=out)
  assert got is out
  g = got.cpu().numpy()
  np.testing.assert_array_equal(T.raw(g), T.raw(exp))
  off = T.offsets([a.size for a in hs], align)
  pad = np.ones(exp.size, bool)
  for a, o in zip(hs, off):
    pad[o:o + a.size] = False
  assert not T.raw(g)[pad].any()   # every padding element is +0, also behind the last tensor
  return got


# ---- sizes, padding, alignments, the round trip -----------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "129", "155"])
@pytest.mark.parametrize("wire", [F32, F16], ids=["fp32", "fp16"])
def test_sizes_and_padding(name, wire):
  hs = host_set(name)
  assert name == "edges" or len(hs) == int(name)
  check_concat(hs, [dev(a) for a in hs], 0.37, wire)


def test_last_tensor_is_followed_by_padding():
  hs = host_set("edges")[:9]          # ends with 4097 elements: 15 elements of padding behind the last tensor
  assert hs[-1].size == 4097
  check_concat(hs, [dev(a) for a in hs], 1.0, F32)
  check_concat(hs, [dev(a) for a in hs], 1.0, F16)


@pytest.mark.parametrize("name", ["edges", "155"])
def test_round_trip_is_the_reference_s(name):
  """distribution_ops_test.py:520-531: split(like, concat(arrays)) == arrays, views of the flat buffer."""
  hs = host_set(name)
  ts = [dev(a) for a in hs]
  flat = D.aligned_flat_concat(ts)
  assert flat.dtype == torch.float32 and flat.numel() == T.offsets([a.size for a in hs])[-1]
  back = D.aligned_flat_split(ts, flat)
  off = T.offsets([a.size for a in hs])
  for b, a, o in zip(back, hs, off):
    assert b.shape == a.shape
    assert b.numel() == 0 or b.data_ptr() == flat.data_ptr() + 4 * o
    np.testing.assert_array_equal(T.raw(b.cpu().numpy()), T.raw(a))


@pytest.mark.parametrize("align", [4, 1024])
@pytest.mark.parametrize("wire", [F32, F16], ids=["fp32", "fp16"])
def test_alignments(align, wire):
  hs = host_set("edges")
  ts = [dev(a) for a in hs]
  flat = check_concat(hs, ts, 0.37, wire, align=align)
  if wire is F32:
    for b, a in zip(D.aligned_flat_split(ts, flat, align=align), T.split(hs, T.concat(hs, 0.37, F32, align), align)):
      np.testing.assert_array_equal(T.raw(b.cpu().numpy()), T.raw(a))


# ---- more chunks than workgroups ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_set():
  """2052 chunks in front of 130 small tensors: the launch has 2048 workgroups, so workgroups 0 .. 3 take a
  second chunk — workgroup 0's in the same tensor (its 5 tail elements and their padding), workgroup 1's in the
  next one, those of 2 and 3 in the one after."""
  rng = np.random.default_rng(23)
  return [rng.standard_normal(n).astype(F32) for n in (2048 * 4096 + 5, 7, 4097)] + T.set_seeded(130, seed=130)


@pytest.mark.parametrize("table", ["inline", "uploaded"])
@pytest.mark.parametrize("wire", [F32, F16], ids=["fp32", "fp16"])
def test_workgroups_take_a_second_chunk(wire, table):
  hs = long_set()[:3] if table == "inline" else long_set()
  assert sum((a.size + 4095) // 4096 for a in hs[:3]) == 2052 and (len(hs) > 128) == (table == "uploaded")
  scale = np.float32(0.37)
  assert np.isfinite(T.concat(hs[:3], scale, wire)).all()
  got = check_concat(hs, [dev(a) for a in hs], scale, wire, scale_arg=dev(np.array(scale)))
  tail = T.offsets([a.size for a in hs])[0] + hs[0].size
  assert not T.raw(got[tail:tail + 11].cpu().numpy()).any()   # the 11 zeros behind the first tensor's 5 tail elements


# ---- misaligned sources ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", [F32, F16], ids=["fp32", "fp16"])
def test_misaligned_sources_give_the_same_bits(wire):
  hs = host_set("edges")
  aligned = check_concat(hs, [dev(a) for a in hs], 0.37, wire)
  ts = [unaligned(a) if a.size else dev(a) for a in hs]
  got = check_concat(hs, ts, 0.37, wire)
  assert torch.equal(got.view(torch.int32 if wire is F32 else torch.int16),
                     aligned.view(torch.int32 if wire is F32 else torch.int16))


# ---- the scale ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.37, 0.0, float("nan")], ids=["1", "0.37", "0", "nan"])
@pytest.mark.parametrize("wire", [F32, F16], ids=["fp32", "fp16"])
def test_host_scales(scale, wire):
  hs = host_set("edges")
  check_concat(hs, [dev(a) for a in hs], scale, wire)   # (a NaN or zero scale leaves the padding +0)


@pytest.mark.parametrize("where", ["clipping", "not clipping"])
@pytest.mark.parametrize("wire", [F32, F16], ids=["fp32", "fp16"])
def test_device_scale_from_the_norm(where, wire):
  hs = host_set("edges")
  norm = np.sqrt(CT.tree_sumsq(hs)[0], dtype=np.float32)
  clip_norm = float(norm) * (0.37 if where == "clipping" else 2.0)
  _, _, scale_t = CT.norm_and_scale(hs, clip_norm)
  assert (scale_t != np.float32(1)) == (where == "clipping")
  ts = [dev(a) for a in hs]
  _, scale_dev = clip_ops.global_norm_and_scale(ts, clip_norm)
  got = check_concat(hs, ts, scale_t, wire, scale_arg=scale_dev)
  host = D.aligned_flat_concat(ts, scale=float(scale_t), wire_dtype=TORCH_OF[wire])
  view = torch.int32 if wire is F32 else torch.int16
  assert torch.equal(got.view(view), host.view(view))
  assert CT.bits(scale_dev.cpu().numpy()) == CT.bits(scale_t)


# ---- the fp16 wire --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5, 3.0])
def test_fp16_wire_edges(scale):
  hs = host_set("fp16")
  exp = T.concat(hs, scale, F16)
  if scale == 1.0:   # the set holds what it says
    e = exp[:hs[0].size]
    assert np.isinf(e).any() and np.isnan(e).any() and (T.raw(e) == 0x8000).any()
    assert ((T.raw(e) & 0x7c00) == 0).any() and ((T.raw(e) & 0x7fff) == 1).any()   # subnormals, the smallest one
    assert T.raw(np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], F32).astype(F16)).tolist() == [0x3c00, 0x3c02]
  check_concat(hs, [dev(a) for a in hs], scale, F16)
  check_concat(hs, [unaligned(a) for a in hs], scale, F16)


@pytest.mark.parametrize("scale", [0.37, 3.0])
def test_fp16_wire_is_a_float32_product_then_a_conversion(scale):
  """Products that land on an fp16 tie after their float32 rounding: a fused multiply-and-convert would round
  about half of them to the other neighbour."""
  x, one_step = T.set_two_roundings(scale)
  exp = T.concat([x], scale, F16)
  differ = int((T.raw(exp[:x.size]) != one_step).sum())
  print("scale %r: %d of %d values tell the two orders apart" % (scale, differ, x.size))
  assert differ >= x.size // 4
  check_concat([x], [dev(x)], scale, F16)
  check_concat([x], [unaligned(x)], scale, F16)


# ---- the decode -----------------------------------------------------------------------------------------
def test_decode_fp16_and_fp32_in_place():
  hs = host_set("edges") + host_set("fp16")
  ts = [dev(a) for a in hs]
  off = T.offsets([a.size for a in hs])
  # fp16 -> a new fp32 buffer, post_scale 0.5
  flat16 = D.aligned_flat_concat(ts, scale=0.37, wire_dtype=torch.float16)
  before = flat16.clone()
  got = D.aligned_flat_split(ts, flat16, post_scale=0.5)
  exp = T.decode(T.concat(hs, 0.37, F16), 0.5)
  base = got[1].data_ptr() - 4 * off[1]
  for g, a, o in zip(got, hs, off):
    assert g.dtype == torch.float32 and g.shape == a.shape
    assert g.numel() == 0 or g.data_ptr() == base + 4 * o           # views of ONE decoded buffer
    np.testing.assert_array_equal(T.raw(g.cpu().numpy().ravel()), T.raw(exp[o:o + a.size]))
  assert torch.equal(before.view(torch.int16), flat16.view(torch.int16))   # the wire buffer is left alone
  # fp16 without a post_scale: the conversion alone
  got = D.aligned_flat_split(ts, flat16)
  exp = T.decode(T.concat(hs, 0.37, F16), 1.0)
  for g, a, o in zip(got, hs, off):
    np.testing.assert_array_equal(T.raw(g.cpu().numpy().ravel()), T.raw(exp[o:o + a.size]))
  # fp32 in place
  flat32 = D.aligned_flat_concat(ts, scale=0.37)
  got = D.aligned_flat_split(ts, flat32, post_scale=0.5)
  exp = T.decode(T.concat(hs, 0.37, F32), 0.5)
  np.testing.assert_array_equal(T.raw(flat32.cpu().numpy()), T.raw(exp))
  for g, a, o in zip(got, hs, off):
    assert g.numel() == 0 or g.data_ptr() == flat32.data_ptr() + 4 * o
    np.testing.assert_array_equal(T.raw(g.cpu().numpy().ravel()), T.raw(exp[o:o + a.size]))


def test_decode_of_an_unaligned_and_ragged_buffer():
  """The C entry point takes any element count and any 4-byte-aligned pointer: the single-element form."""
  import ctypes as C
  from monolith_amd import _lib
  rng = np.random.default_rng(5)
  h = rng.standard_normal(3 * 4096 + 3).astype(F32)
  src = unaligned(h)
  out = torch.empty(h.size + 1, dtype=torch.float32, device=DEV)[1:]
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  _lib.check(_lib.lib().mhte_aligned_flat_decode(_lib.vp(src), 0, h.size, 0.5, _lib.vp(out), st))
  np.testing.assert_array_equal(T.raw(out.cpu().numpy()), T.raw(T.decode(h, 0.5)))
  al = dev(h)                           # aligned, but not a multiple of 4 elements: the tail
  _lib.check(_lib.lib().mhte_aligned_flat_decode(_lib.vp(al), 0, h.size, 0.25, _lib.vp(al), st))
  np.testing.assert_array_equal(T.raw(al.cpu().numpy()), T.raw(T.decode(h, 0.25)))


# ---- no host value in the path --------------------------------------------------------------------------
def test_norm_concat_and_decode_replay_in_one_graph():
  """global_norm_and_scale -> concat (device scale, fp16 wire) -> decode, captured on one stream and replayed
  after the gradients were overwritten: the output is the truth for the new contents."""
  shapes = [(5000,), (4097,), (3,), (33, 7), (16,)]
  rng = np.random.default_rng(41)
  first = [rng.standard_normal(s).astype(F32) for s in shapes]
  contents = {"clipped": [rng.standard_normal(s).astype(F32) for s in shapes],
              "not clipped": [(rng.standard_normal(s) * 1e-3).astype(F32) for s in shapes]}
  clip_norm, world = 1.0, 4
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    grads = [dev(a) for a in first]

    def run():
      _, scale = clip_ops.global_norm_and_scale(grads, clip_norm)
      flat = D.aligned_flat_concat(grads, scale=scale, wire_dtype=torch.float16)
      return D.aligned_flat_split(grads, flat, post_scale=1.0 / world)

    run()                # (the warm-up call: the workspace exists afterwards)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
      res = run()
    for k, hs in contents.items():
      for t, a in zip(grads, hs):
        t.copy_(torch.from_numpy(a))
      g.replay()
      s.synchronize()
      _, _, scale_t = CT.norm_and_scale(hs, clip_norm)
      assert (scale_t != np.float32(1)) == (k == "clipped")
      exp = T.split(hs, T.decode(T.concat(hs, scale_t, F16), 1.0 / world))
      for r, e in zip(res, exp):
        np.testing.assert_array_equal(T.raw(r.cpu().numpy()), T.raw(e), err_msg=k)
  torch.cuda.synchronize()
