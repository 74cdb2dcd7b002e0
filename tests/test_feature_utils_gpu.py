"""GPU suite of monolith_amd/feature_utils.py: allreduce_cond with an injected two-rank collective and None
entries, and the clip / allreduce order of clip_and_allreduce — bit for bit against the numpy restatements
(tests/flat_concat_truth.py, tests/clip_ops_truth.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ops_truth as CT  # noqa: E402
import flat_concat_truth as T  # noqa: E402
from monolith_amd import feature_utils as F  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32 = np.float16, np.float32
SHAPES = [(17,), (4097,), (3, 5), (1,), (64, 65)]


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_grads(seed, shapes=SHAPES, mul=1.0):
  rng = np.random.default_rng(seed)
  return [(rng.standard_normal(s) * mul).astype(F32) for s in shapes]


def with_nones(xs):
  """[None, x0, x1, None, x2, ...]: None entries at the front, inside and at the end."""
  out = [None, xs[0], xs[1], None] + list(xs[2:]) + [None]
  return out


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_allreduce_cond_with_two_injected_ranks(fp16):
  a = host_grads(1)
  wire = F16 if fp16 else F32
  s = np.float32(0.37)
  rng = np.random.default_rng(2)
  total = T.offsets([x.size for x in a])[-1]
  b = rng.standard_normal(total).astype(F32).astype(wire)   # the other rank's flat buffer, as the wire carries it
  b_dev = dev(b)
  seen = []

  def two_ranks(flat):
    seen.append((flat.dtype, flat.numel()))
    flat.add_(b_dev)   # the sum over the ranks, formed in the wire's format

  grads = with_nones([dev(x) for x in a])
  got = F.allreduce_cond(grads, scale=float(s), fp16=fp16, allreduce=two_ranks, world=2)
  assert seen == [(torch.float16 if fp16 else torch.float32, total)]
  assert len(got) == len(grads)
  with np.errstate(over="ignore"):
    summed = (T.concat(a, s, wire) + b).astype(wire)         # (a * s + b), one rounding in the wire's format
  exp = T.split(a, T.decode(summed, 0.5))
  it = iter(exp)
  for g, orig in zip(got, grads):
    if orig is None:
      assert g is None
      continue
    e = next(it)
    assert g.dtype == torch.float32 and g.shape == orig.shape
    np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(e))
  if not fp16:   # exactly (a * s + b) * 0.5 per element
    o = T.offsets([x.size for x in a])
    np.testing.assert_array_equal(T.raw(got[1].cpu().numpy()), T.raw((a[0] * s + b[o[0]:o[0] + a[0].size]) * F32(0.5)))
  # a returned buffer is taken instead of the one passed in
  got2 = F.allreduce_cond(grads, scale=float(s), fp16=fp16, allreduce=lambda flat: flat + b_dev, world=2)
  for g, h in zip(got, got2):
    assert (g is None) == (h is None)
    if g is not None:
      assert torch.equal(g.view(torch.int32), h.view(torch.int32))
  for x, orig in zip([t for t in grads if t is not None], a):   # the gradients themselves are left alone
    np.testing.assert_array_equal(T.raw(x.cpu().numpy()), T.raw(orig))


def test_allreduce_cond_single_rank_is_the_scaled_list():
  a = host_grads(3)
  grads = with_nones([dev(x) for x in a])
  nones = [None, None]
  assert F.allreduce_cond(nones) is nones
  got = F.allreduce_cond(grads, scale=0.37)   # torch.distributed is not initialised: one rank, no collective
  for g, e in zip([t for t in got if t is not None], a):
    np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(e * F32(0.37)))
  assert [t is None for t in got] == [t is None for t in grads]


@pytest.mark.parametrize("where", ["clipping", "not clipping"])
def test_clip_by_global_norm_deferred_into_the_concat(where):
  dense, sparse = host_grads(4), host_grads(5, [(300, 8), (77,)])
  clip_norm = 1.0 if where == "clipping" else 1e4
  _, norm_t, scale_t = CT.norm_and_scale(dense + sparse, clip_norm)   # ONE norm over dense + sparse
  assert (scale_t != F32(1)) == (where == "clipping")
  d_dev = with_nones([dev(x) for x in dense])
  out, sparse_scale = F.clip_and_allreduce(d_dev, [dev(x) for x in sparse], F.GradClipType.ClipByGlobalNorm,
                                           clip_norm, use_allreduce=True)
  assert sparse_scale.dim() == 0 and sparse_scale.is_cuda and sparse_scale.dtype == torch.float32
  assert CT.bits(sparse_scale.cpu().numpy()) == CT.bits(scale_t)
  assert [t is None for t in out] == [t is None for t in d_dev]
  for g, x in zip([t for t in out if t is not None], dense):
    np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(x * scale_t))
  # without the allreduce the dense gradients are clipped by clip_by_global_norm with the same norm
  out2, sparse_scale2 = F.clip_and_allreduce(d_dev, [dev(x) for x in sparse], F.GradClipType.ClipByGlobalNorm,
                                             clip_norm, use_allreduce=False)
  assert CT.bits(sparse_scale2.cpu().numpy()) == CT.bits(scale_t)
  exp, _ = CT.clip(dense, clip_norm, use_norm=norm_t)
  for g, e in zip([t for t in out2 if t is not None], exp):
    np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(e))
  # another bound for the sparse side: the same norm against it
  _, sparse_scale3 = F.clip_and_allreduce(d_dev, [dev(x) for x in sparse], F.GradClipType.ClipByGlobalNorm,
                                          clip_norm, sparse_clip_norm=0.25, use_allreduce=True)
  assert CT.bits(sparse_scale3.cpu().numpy()) == CT.bits(CT.norm_and_scale(dense + sparse, 0.25)[2])


def test_no_clip_returns_the_inputs_values():
  dense, sparse = host_grads(6), host_grads(7, [(50, 4)])
  d_dev = with_nones([dev(x) for x in dense])
  for use_allreduce in (False, True):
    for kw in ({"clip_type": F.GradClipType.NoClip, "clip_norm": 1e-3},
               {"clip_type": F.GradClipType.ClipByGlobalNorm, "clip_norm": None}):
      out, sparse_scale = F.clip_and_allreduce(d_dev, [dev(x) for x in sparse], use_allreduce=use_allreduce, **kw)
      assert sparse_scale.dim() == 0 and sparse_scale.is_cuda and CT.bits(sparse_scale.cpu().numpy()) == CT.bits(F32(1))
      assert [t is None for t in out] == [t is None for t in d_dev]
      for g, x in zip([t for t in out if t is not None], dense):
        np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(x))


def test_clip_by_dense_and_sparse_uses_two_norms():
  dense, sparse = host_grads(8), host_grads(9, [(300, 8), (77,)], mul=3.0)
  clip_norm, sparse_clip_norm = 2.0, 0.5
  _, _, dense_scale_t = CT.norm_and_scale(dense, clip_norm)
  _, _, sparse_scale_t = CT.norm_and_scale(sparse, sparse_clip_norm)
  assert dense_scale_t != F32(1) and sparse_scale_t != F32(1) and dense_scale_t != sparse_scale_t
  d_dev, s_dev = [dev(x) for x in dense], [dev(x) for x in sparse]
  out, sparse_scale = F.clip_and_allreduce(d_dev, s_dev, F.GradClipType.ClipByDenseAndSparse, clip_norm,
                                           sparse_clip_norm=sparse_clip_norm, use_allreduce=True)
  assert CT.bits(sparse_scale.cpu().numpy()) == CT.bits(sparse_scale_t)
  for g, x in zip(out, dense):
    np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(x * dense_scale_t))
  # no bound for the sparse side: no second norm, its scale is 1
  out, sparse_scale = F.clip_and_allreduce(d_dev, s_dev, F.GradClipType.ClipByDenseAndSparse, clip_norm,
                                           use_allreduce=True, fp16=True)
  assert CT.bits(sparse_scale.cpu().numpy()) == CT.bits(F32(1))
  exp = T.split(dense, T.decode(T.concat(dense, dense_scale_t, F16), 1.0))
  for g, e in zip(out, exp):
    np.testing.assert_array_equal(T.raw(g.cpu().numpy()), T.raw(e))
  with pytest.raises(NotImplementedError):
    F.clip_and_allreduce(d_dev, s_dev, F.GradClipType.ClipByValue, clip_norm)
