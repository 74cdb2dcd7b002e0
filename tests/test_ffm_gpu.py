"""GPU suite of the FFM feature cross (mhte_ffm / mhte_ffm_grad, monolith_amd/layer_ops.py,
monolith_amd/feature_cross.py).  Every comparison is with the numpy truth (tests/ffm_truth.py) on raw bits: no
tolerance, no element left out.  Outputs start as a NaN pattern with guard words on both sides; the upstream
gradient is random; the launch counters (mhte_ffm_launch_counts) must show the kernel form the shape and the
alignment call for, and test_every_form_is_reached_by_a_case shows that the cases below reach all sixteen."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffm_truth as FT  # noqa: E402
from monolith_amd import _lib, feature_cross, layer_ops  # noqa: E402
from monolith_amd._lib import check, vp  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 8                 # floats on each side of a buffer (32 bytes: the alignment of the payload is the storage's)
NAN_WORD = 0x7FC0BEEF     # a quiet NaN no computation produces
GUARD_WORD = 0x7FC0CAFE


class Buf:
  """[rows, cols] float32 at ``off`` floats into storage of its own: off 0 is 16-byte aligned, off 1 has
  data_ptr() % 16 == 4.  Payload and guards start as NaN patterns."""

  def __init__(self, rows, cols, off, data=None):
    n = rows * cols
    words = np.full(GUARD + off + n + GUARD, GUARD_WORD, np.uint32)
    words[GUARD + off:GUARD + off + n] = NAN_WORD if data is None else FT.bits(data).ravel()
    self.store = torch.from_numpy(words.view(np.int32)).cuda()
    self.lo, self.n = GUARD + off, n
    self.t = self.store.view(torch.float32)[self.lo:self.lo + n].view(rows, cols)
    assert self.store.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * off

  def read(self, what):
    """The payload; the guards must be untouched."""
    words = self.store.cpu().numpy().view(np.uint32)
    assert (words[:self.lo] == GUARD_WORD).all() and (words[self.lo + self.n:] == GUARD_WORD).all(), \
        "%s: a guard word was overwritten" % what
    return words[self.lo:self.lo + self.n].view(F).reshape(self.t.shape)


def stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_case(B, L, R, D, int_type, off, left_extra=0, right_extra=0, seed=1, zero_left=False):
  """Forward and gradient through the C ABI on buffers at ``off``; -> the names of the two forms that ran."""
  left, right, grad = FT.case(seed, B, L, R, D, int_type, left_extra, right_extra)
  if zero_left:
    left[:] = F(0.0)
  it = FT.INT_TYPES.index(int_type)
  want_out = FT.forward(left, right, D, int_type)
  want_lg, want_rg = FT.gradient(grad, left, right, D, int_type)
  dl, dr, dg = Buf(*left.shape, off, left), Buf(*right.shape, off, right), Buf(*grad.shape, off, grad)
  out, lg, rg = Buf(*want_out.shape, off), Buf(*left.shape, off), Buf(*right.shape, off)
  lib = _lib.lib()
  before = layer_ops.ffm_launch_counts()
  check(lib.mhte_ffm(vp(dl.t), left.shape[1], vp(dr.t), right.shape[1], B, D, it, vp(out.t), want_out.shape[1],
                     stream()))
  check(lib.mhte_ffm_grad(vp(dg.t), grad.shape[1], vp(dl.t), left.shape[1], vp(dr.t), right.shape[1], B, D, it,
                          vp(lg.t), vp(rg.t), stream()))
  torch.cuda.synchronize()
  after = layer_ops.ffm_launch_counts()
  what = "%s B=%d L=%d R=%d D=%d off=%d" % (int_type, B, L, R, D, off)
  FT.assert_same_bits(out.read(what), want_out, what + " out")
  FT.assert_same_bits(lg.read(what), want_lg, what + " left_grad")
  FT.assert_same_bits(rg.read(what), want_rg, what + " right_grad")
  for b, host in ((dl, left), (dr, right), (dg, grad)):   # the inputs are only read
    FT.assert_same_bits(b.read(what), host, what + " input")
  ran = sorted(k for k in after if after[k] != before[k])
  assert all(after[k] == before[k] + 1 for k in ran) and len(ran) == 2, (what, ran)
  return ran, expected_forms(L, R, D, int_type, off, left.shape[1], right.shape[1])


def expected_forms(L, R, D, int_type, off, left_cols, right_cols):
  """All buffers of a case share ``off``; the widths of out and grad are multiples of 4 whenever D is."""
  aligned = off == 0 and left_cols % 4 == 0 and right_cols % 4 == 0
  forms = FT.kernel_forms(L, R, D, aligned)
  dot = FT.INT_TYPES.index(int_type)
  return sorted([FT.COUNTERS[forms[dot][3]], FT.COUNTERS[forms[2 + dot][3]]])


OFFS = pytest.mark.parametrize("off", [0, 1], ids=["aligned", "one float in"])
TYPES = pytest.mark.parametrize("int_type", FT.INT_TYPES)

# lane shapes and edges: one element; fewer outputs than lanes; L or R of 1; D of 3, 4, 16, 17 and 64; several
# workgroups; a last tile that is partial
EDGE_SHAPES = [(1, 1, 1, 1), (67, 1, 5, 3), (67, 5, 1, 4), (300, 10, 12, 16), (33, 3, 7, 17), (5, 6, 6, 64)]
# operands beyond the LDS budgets (and the 32 KiB slab that fits): B, L, R, D
BIG_SHAPES = [(3, 48, 48, 32), (3, 16, 16, 32), (2, 1, 129, 64), (2, 128, 128, 4), (2, 130, 130, 1), (2, 1, 1, 8196)]


@OFFS
@TYPES
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "B%d-L%d-R%d-D%d" % s)
def test_lane_shapes_and_edges(shape, int_type, off):
  B, L, R, D = shape
  ran, want = run_case(B, L, R, D, int_type, off)
  assert ran == want
  vec = "vec4" if (off == 0 and D % 4 == 0) else "vec1"   # float4 for the aligned D % 4 == 0 cases, else one float
  assert all(("/%s/" % vec) in k and k.endswith("/lds") for k in ran), ran


@OFFS
@TYPES
@pytest.mark.parametrize("extra", [(1, 3), (4, 8)], ids=["odd widths", "whole float4s"])
def test_trailing_columns(extra, int_type, off):
  """left is L D + 1 wide and right R D + 3: the forward ignores the columns, the gradients are full width with +0
  bits there (the truth says so, the comparison is on bits).  Widths that stay multiples of 4 keep the float4 form
  and its whole-float4 zero stores."""
  B, L, R, D = 9, 3, 5, 16
  ran, want = run_case(B, L, R, D, int_type, off, left_extra=extra[0], right_extra=extra[1])
  assert ran == want
  assert all(("/vec4/" if (off == 0 and extra == (4, 8)) else "/vec1/") in k for k in ran), ran
  left, right, grad = FT.case(1, B, L, R, D, int_type, *extra)
  lg, rg = FT.gradient(grad, left, right, D, int_type)
  assert not FT.bits(lg[:, L * D:]).any() and not FT.bits(rg[:, R * D:]).any() and lg.shape == left.shape


@OFFS
@TYPES
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: "B%d-L%d-R%d-D%d" % s)
def test_operands_beyond_the_lds_budget(shape, int_type, off):
  """B = 3, L = R = 48, D = 32 has a 288 KiB multiply slab, more than a CU's LDS: the gradient takes the direct
  form; L = R = 16 (32 KiB) is staged.  The other shapes send the forward and the dot gradient past theirs."""
  B, L, R, D = shape
  ran, want = run_case(B, L, R, D, int_type, off)
  assert ran == want
  grad_form = [k for k in ran if k.startswith("gradient/")][0]
  if (L, R, D) == (48, 48, 32) and int_type == "multiply":
    assert grad_form.endswith("/direct")
  if (L, R, D) == (16, 16, 32):
    assert grad_form.endswith("/lds")


def test_every_form_is_reached_by_a_case():
  reached = set()
  for B, L, R, D in EDGE_SHAPES + BIG_SHAPES:
    for int_type in FT.INT_TYPES:
      for off in (0, 1):
        reached.update(expected_forms(L, R, D, int_type, off, L * D, R * D))
  assert reached == set(FT.COUNTERS)


@TYPES
def test_batch_past_one_grid_pass(int_type):
  """B = 70 000, L = R = 2, D = 4: tiles of 64 rows, 1 094 of them, the last with 48 rows.  The forward launches
  1 024 workgroups at most and the gradient 512: both grids stride here (70 resp. 582 tiles are second or third
  tiles of their workgroup)."""
  B, L, R, D = 70000, 2, 2, 4
  forms = FT.kernel_forms(L, R, D, True)
  assert all(f[2] == 64 for f in forms)
  tiles = -(-B // 64)
  assert tiles == 1094 and B % 64 == 48 and tiles > FT.FWD_MAX_GROUPS > FT.GRAD_MAX_GROUPS
  ran, want = run_case(B, L, R, D, int_type, 0)
  assert ran == want and all("/vec4/lds" in k for k in ran)


@TYPES
def test_reference_shape_through_the_python_ops(int_type):
  """layer_ops_test.py's shape, B = 8, L = 10, R = 12, D = 4, through layer_ops.ffm with backward() and through
  feature_cross.GroupInt on lists of [8, 4] tensors; a weighted sum makes the upstream gradient random."""
  B, L, R, D = 8, 10, 12, 4
  left, right, grad = FT.case(21, B, L, R, D, int_type)
  want = FT.forward(left, right, D, int_type)
  want_lg, want_rg = FT.gradient(grad, left, right, D, int_type)
  assert want.shape == ((8, 480) if int_type == "multiply" else (8, 120))
  w = torch.from_numpy(grad).cuda()
  tl = torch.from_numpy(left).cuda().requires_grad_()
  tr = torch.from_numpy(right).cuda().requires_grad_()
  out = layer_ops.ffm(tl, tr, D, int_type)
  (out * w).sum().backward()
  FT.assert_same_bits(out.detach().cpu().numpy(), want, "ffm")
  FT.assert_same_bits(tl.grad.cpu().numpy(), want_lg, "left.grad")
  FT.assert_same_bits(tr.grad.cpu().numpy(), want_rg, "right.grad")
  raw = layer_ops.ffm_grad(w, tl.detach(), tr.detach(), D, int_type)
  FT.assert_same_bits(raw[0].cpu().numpy(), want_lg, "ffm_grad left")
  FT.assert_same_bits(raw[1].cpu().numpy(), want_rg, "ffm_grad right")
  # the layer: lists of [8, 4] tensors that require gradients
  fl = [torch.from_numpy(np.ascontiguousarray(left[:, i * D:(i + 1) * D])).cuda().requires_grad_() for i in range(L)]
  fr = [torch.from_numpy(np.ascontiguousarray(right[:, i * D:(i + 1) * D])).cuda().requires_grad_() for i in range(R)]
  for keep_list in (False, True):
    layer = feature_cross.GroupInt(interaction_type=int_type, keep_list=keep_list)
    got = layer((fl, fr))
    assert isinstance(got, list) == keep_list
    got = got[0] if keep_list else got
    FT.assert_same_bits(got.detach().cpu().numpy(), want, "GroupInt")
  (got * w).sum().backward()
  FT.assert_same_bits(torch.cat([t.grad for t in fl], 1).cpu().numpy(), want_lg, "GroupInt left fields")
  FT.assert_same_bits(torch.cat([t.grad for t in fr], 1).cpu().numpy(), want_rg, "GroupInt right fields")
  # a non-contiguous operand is copied first
  wide = torch.from_numpy(np.concatenate([left, left], 1)).cuda()
  FT.assert_same_bits(layer_ops.ffm(wide[:, :L * D], tr.detach(), D, int_type).cpu().numpy(), want, "a column slice")
  with pytest.raises(_lib.InvalidArgumentError, match="ffm_grad: the in/out shape not match"):
    layer_ops.ffm_grad(w[:, :-1], tl.detach(), tr.detach(), D, int_type)


@TYPES
def test_empty_problems(int_type):
  """B = 0, and L = 0 (a [B, 0] left, and a left narrower than one feature): the shapes come back, nothing is
  launched, and the gradients of the empty cross are +0 in every bit."""
  D = 4
  before = layer_ops.ffm_launch_counts()
  e = lambda r, c: torch.full((r, c), float("nan"), device="cuda")  # noqa: E731
  out = layer_ops.ffm(e(0, 40), e(0, 48), D, int_type)
  assert out.shape == ((0, 480) if int_type == "multiply" else (0, 120))
  lg, rg = layer_ops.ffm_grad(e(0, out.shape[1]), e(0, 40), e(0, 48), D, int_type)
  assert lg.shape == (0, 40) and rg.shape == (0, 48)
  for left_cols in (0, 2):
    out = layer_ops.ffm(e(7, left_cols), e(7, 50), D, int_type)
    assert out.shape == (7, 0)
    lg, rg = layer_ops.ffm_grad(e(7, 0), e(7, left_cols), e(7, 50), D, int_type)
    assert lg.shape == (7, left_cols) and rg.shape == (7, 50)
    assert not FT.bits(lg.cpu().numpy()).any() and not FT.bits(rg.cpu().numpy()).any()
  lg, rg = layer_ops.ffm_grad(e(7, 0), e(7, 50), e(7, 0), D, int_type)   # R = 0
  assert lg.shape == (7, 50) and not FT.bits(lg.cpu().numpy()).any() and rg.shape == (7, 0)
  torch.cuda.synchronize()
  assert layer_ops.ffm_launch_counts() == before


@OFFS
def test_signed_zeros(off):
  """dot with an all-zero left: the products are zeros of both signs, every output is +0 + (+-0) ... = +0 in its
  sign bit too, and so is every right gradient; an accumulator started from the first product would give -0."""
  B, L, R, D = 6, 3, 4, 8
  left, right, _ = FT.case(1, B, L, R, D, "dot")
  prod = np.zeros_like(left).reshape(B, L, 1, D) * right.reshape(B, 1, R, D)
  assert np.signbit(prod[..., 0]).any()   # some FIRST products are -0
  want = FT.forward(np.zeros_like(left), right, D, "dot")
  assert not FT.bits(want).any()
  ran, wanted = run_case(B, L, R, D, "dot", off, zero_left=True)
  assert ran == wanted
  run_case(B, L, R, D, "multiply", off, zero_left=True)   # (here the zeros keep their signs: the truth has them)


@TYPES
def test_replays_in_a_graph(int_type):
  """Forward and gradient captured into one graph on a side stream (a single chain), replayed twice with the
  operands rewritten in place in between: each replay gives the truth for the values it saw."""
  B, L, R, D = 40, 5, 6, 8
  cases = [FT.case(seed, B, L, R, D, int_type) for seed in (31, 32, 33)]
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    tl, tr, tg = (torch.from_numpy(a).cuda() for a in cases[0])
    layer_ops.ffm(tl, tr, D, int_type)   # (the warm-up call)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
      out = layer_ops.ffm(tl, tr, D, int_type)
      lg, rg = layer_ops.ffm_grad(tg, tl, tr, D, int_type)
    for left, right, grad in cases[1:]:
      tl.copy_(torch.from_numpy(left))
      tr.copy_(torch.from_numpy(right))
      tg.copy_(torch.from_numpy(grad))
      g.replay()
      s.synchronize()
      FT.assert_same_bits(out.cpu().numpy(), FT.forward(left, right, D, int_type), "replayed out")
      want_lg, want_rg = FT.gradient(grad, left, right, D, int_type)
      FT.assert_same_bits(lg.cpu().numpy(), want_lg, "replayed left_grad")
      FT.assert_same_bits(rg.cpu().numpy(), want_rg, "replayed right_grad")
  torch.cuda.synchronize()


@TYPES
def test_the_same_call_twice_gives_the_same_bits(int_type):
  B, L, R, D = 300, 10, 12, 16
  left, right, grad = FT.case(51, B, L, R, D, int_type)
  tl, tr, tg = (torch.from_numpy(a).cuda() for a in (left, right, grad))
  runs = []
  for _ in range(2):
    out = layer_ops.ffm(tl, tr, D, int_type)
    lg, rg = layer_ops.ffm_grad(tg, tl, tr, D, int_type)
    runs.append([FT.bits(t.cpu().numpy()) for t in (out, lg, rg)])
  for a, b in zip(*runs):
    assert np.array_equal(a, b)
