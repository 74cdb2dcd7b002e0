"""GPU suite of FeatureInsight (csrc/mhte_fi_kernels.h, mhte_fi_host.h, monolith_amd/layer_ops.py) against the
float64 truth of tests/feature_insight_truth.py within its derived bounds, and against the truth's fp32 definition
bit for bit (it is implemented for every form).  Every case goes through the C ABI on guarded buffers, runs both
modes and both gradients and checks besides: a second call repeats the first one's bits, a single requested gradient
has the bits of the pair, the aggregate squares the very bits the plain op stores, no guard word or input changes,
every zero is +0.

Measured on an MI355X (the largest share of its bound any case of this file used): out 0.98, agg 0.22,
input_grad 0.87, weight_grad 0.84, composed agg 0.04; the largest shares come from chains of one to three terms."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import feature_insight_truth as FT  # noqa: E402
from monolith_amd import _lib, layer_ops  # noqa: E402
from monolith_amd._lib import check, vp  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 8                 # floats on each side of a buffer
NAN_WORD = 0x7FC0BEEF     # a quiet NaN no computation produces
GUARD_WORD = 0x7FC0CAFE
NAMES = ("out", "agg", "input_grad", "weight_grad")
USED = dict.fromkeys(NAMES + ("agg_composed",), 0.0)   # the largest share of a bound any case used (printed)
REACHED = layer_ops.feature_insight_launch_counts()    # the counters before this file's first launch


class Buf:
  """n float32 at ``off`` floats into storage of its own: off 0 is 16-byte aligned, off 1 has
  data_ptr() % 16 == 4.  Payload and guards start as NaN patterns."""

  def __init__(self, n, off, data=None):
    words = np.full(GUARD + off + n + GUARD, GUARD_WORD, np.uint32)
    words[GUARD + off:GUARD + off + n] = NAN_WORD if data is None else FT.bits(data).ravel()
    self.store = torch.from_numpy(words.view(np.int32)).cuda()
    self.lo, self.n = GUARD + off, n
    self.t = self.store.view(torch.float32)[self.lo:self.lo + n]
    assert self.store.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * off

  def read(self, what):
    """The payload; the guards must be untouched."""
    words = self.store.cpu().numpy().view(np.uint32)
    assert (words[:self.lo] == GUARD_WORD).all() and (words[self.lo + self.n:] == GUARD_WORD).all(), \
        "%s: a guard word was overwritten" % what
    return words[self.lo:self.lo + self.n].view(F).copy()


def stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same(a, b):
  return np.array_equal(FT.bits(a), FT.bits(b))


def c_sizes(sizes):
  return (C.c_int32 * len(sizes))(*sizes)


def run_abi(x, w, g, sizes, off=0, what=""):
  """Every form through the C ABI on buffers at ``off`` -> {name: array}, with the consistency checks every case
  must hold."""
  (B, E), K, nseg = x.shape, w.shape[1], len(sizes)
  ins = [Buf(a.size, off, a) for a in (x, w, g)]
  px, pw, pg = (vp(b.t) if b.n else None for b in ins)
  lib, cs = _lib.lib(), c_sizes(sizes)
  outs = {}

  def fwd(name, aggregate):
    cols = nseg if aggregate else nseg * K
    o = Buf(B * cols, off)
    check(lib.mhte_feature_insight(px, pw, B, E, K, cs, nseg, aggregate, vp(o.t) if o.n else None, cols, stream()))
    outs[name] = o

  def bwd(name, want_i, want_w):
    gi, gw = Buf(B * E, off) if want_i else None, Buf(E * K, off) if want_w else None
    check(lib.mhte_feature_insight_grad(pg, nseg * K, px, pw, B, E, K, cs, nseg, vp(gi.t) if gi else None,
                                        vp(gw.t) if gw else None, stream()))
    outs[name + "/i"], outs[name + "/w"] = gi, gw

  fwd("out", 0)
  fwd("agg", 1)
  bwd("both", True, True)
  fwd("out again", 0)
  fwd("agg again", 1)
  bwd("again", True, True)
  if E:
    bwd("only i", True, False)
    bwd("only w", False, True)
  torch.cuda.synchronize()
  got = {n: b.read(what + " " + n) for n, b in outs.items() if b is not None}
  for b, a in zip(ins, (x, w, g)):
    assert same(b.read(what), a.ravel()), what + ": an input changed"
  assert same(got["out"], got["out again"]) and same(got["agg"], got["agg again"]), what + ": two calls differ"
  assert same(got["both/i"], got["again/i"]) and same(got["both/w"], got["again/w"]), what + ": two calls differ"
  if E:
    assert same(got["both/i"], got["only i/i"]), what + ": input_grad alone"
    assert same(got["both/w"], got["only w/w"]), what + ": weight_grad alone"
  res = dict(out=got["out"].reshape(B, nseg * K), agg=got["agg"].reshape(B, nseg),
             input_grad=got["both/i"].reshape(B, E), weight_grad=got["both/w"].reshape(E, K))
  for n, a in res.items():
    assert not np.signbit(a[a == 0]).any(), what + ": a zero of %s must be +0" % n
  return res


def check_case(x, w, g, sizes, what, off=0, bitwise=True):
  t = FT.Truth(x, w, sizes, g)
  got = run_abi(x, w, g, sizes, off, what)
  bounds = t.bounds()
  for name in NAMES:
    want, bound = getattr(t, name), bounds[name]
    assert got[name].shape == want.shape, (what, name)
    err = np.abs(got[name].astype(np.float64) - want)
    assert np.isfinite(got[name]).all() and (err <= bound).all(), (what, name, float((err - bound).max()))
    share = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    USED[name] = max(USED[name], share)
    print("%s: %s uses %.3f of its bound" % (what, name, share))
  if bitwise:
    d = FT.Fp32(x, w, sizes)
    for name, want in (("out", d.out()), ("agg", d.agg()), ("input_grad", d.input_grad(g)),
                       ("weight_grad", d.weight_grad(g))):
      assert same(got[name], want), what + ": %s differs from the fp32 definition" % name
  return t, got


def case(seed, B, sizes, K, what, **kw):
  x, w, g = FT.inputs(seed, B, sizes, K)
  return check_case(x, w, g, sizes, what, **kw)


# ---- the block edges, read from the plan ------------------------------------------------------------------------
PLAN = layer_ops.feature_insight_plan(1, 9, 2, 3)
STAGE, TILE, ROWS, INLINE = PLAN["stage"], PLAN["column_tile"], PLAN["row_block"], PLAN["inline_segments"]


def _three(n):
  return [n - 1, n, n + 1]


def test_segment_sizes():
  sizes = [1] + _three(8) + _three(32) + [STAGE + 1] + _three(TILE) + [2 * STAGE + 1]
  case(1, 5, sizes, 3, "segment sizes")


@pytest.mark.parametrize("nseg", [1, 3, INLINE + 1, FT.MAX_SEGMENTS])
def test_numbers_of_segments(nseg):
  if nseg == 1:
    sizes = [2 * TILE + 6]   # one segment: a plain GEMM, several stages, several tiles of the gradients
  else:
    sizes = [(1, 0, 2, 3)[i % 4] for i in range(nseg)] if nseg > 3 else [3, 2, 4]
  assert layer_ops.feature_insight_plan(3, sum(sizes), 2, nseg)["groups"] == (nseg + INLINE - 1) // INLINE
  case(2, 3, sizes, 2, "F %d" % nseg)


@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, TILE + 1])
def test_output_widths(K):
  case(3, 5, [3, 2, 4], K, "K %d" % K)


def _slab_batch():
  """One above two slabs: three slabs are summed."""
  rows = layer_ops.feature_insight_plan(3 * TILE, 9, 2, 3)["slab_rows"]
  B = 2 * rows + 1
  assert layer_ops.feature_insight_plan(B, 9, 2, 3)["slabs"] == 3
  return B


@pytest.mark.parametrize("B", [1, 31, 32, 33, ROWS + 1, _slab_batch()])
def test_batch_sizes(B):
  case(4, B, [3, 2, 4], 2, "B %d" % B)


@pytest.mark.parametrize("sizes", [[0, 5, 3], [5, 0, 0, 3], [5, 3, 0], [0, 0], [0, 9, 0, 0, 7, 0]])
def test_zero_size_segments(sizes):
  t, got = case(5, 4, sizes, 3, "sizes %s" % sizes)
  for f, s in enumerate(sizes):
    if s == 0:
      assert not FT.bits(got["out"][:, 3 * f:3 * f + 3]).any() and not FT.bits(got["agg"][:, f]).any()   # +0


def test_several_row_blocks_column_tiles_and_slabs_at_once():
  B = 2 * ROWS + 7
  assert layer_ops.feature_insight_plan(B, 104, 70, 3)["slabs"] >= 3
  case(6, B, [TILE + 6, 0, STAGE + 2], TILE + 6, "all edges", bitwise=True)


# ---- the reference's example and exact inputs ---------------------------------------------------------------------
def test_the_reference_example_through_layer_ops_and_the_abi():
  with open(os.path.join(ROOT, "tests", "golden", "feature_insight_kat.json")) as f:
    k = json.load(f)
  sizes = k["segment_sizes"]
  x = np.array(k["input"], dtype=F).reshape(k["batch"], -1)
  w = np.array(k["weight"], dtype=F).reshape(-1, k["k"])
  g = np.ones((k["batch"], len(sizes) * k["k"]), dtype=F)
  t, got = check_case(x, w, g, sizes, "the reference's example")
  b = t.bounds()
  for name in NAMES:
    assert (np.abs(got[name] - np.array(k[name])) <= b[name] + 1e-15).all(), name
  tx, tw = torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(w).cuda().requires_grad_()
  out = layer_ops.feature_insight(tx, tw, sizes)
  out.sum().backward()
  assert same(out.detach().cpu().numpy(), got["out"])
  assert same(tx.grad.cpu().numpy(), got["input_grad"]) and same(tw.grad.cpu().numpy(), got["weight_grad"])
  agg = layer_ops.feature_insight(tx.detach(), tw.detach(), sizes, aggregate=True)
  assert same(agg.cpu().numpy(), got["agg"])
  np.testing.assert_allclose(agg.cpu().numpy()[0], [0.0968, 0.3098, 8.9896], rtol=1e-5)


def test_exact_inputs_equal_fp64_bit_for_bit():
  # small integers: every order gives the same value, so a dropped or doubled term shows
  sizes, K, B = [200, 1, 0, 37, 64], 35, 300
  x, w, g = FT.inputs(7, B, sizes, K, exact=8)
  t = FT.Truth(x, w, sizes, g)
  got = run_abi(x, w, g, sizes, what="exact")
  assert layer_ops.feature_insight_plan(B, sum(sizes), K, len(sizes))["slabs"] >= 3
  for name in ("out", "input_grad", "weight_grad"):
    assert np.abs(getattr(t, name)).max() < 2 ** 24
    assert np.array_equal(got[name].astype(np.float64), getattr(t, name)), name
  sizes, K, B = [1, 8, 7, 3, 0, 8], 33, 70
  x, w, g = FT.inputs(8, B, sizes, K, exact=3)
  t = FT.Truth(x, w, sizes, g)
  got = run_abi(x, w, g, sizes, what="exact aggregate")
  assert np.abs(t.agg).max() < 2 ** 24 and np.array_equal(got["agg"].astype(np.float64), t.agg)
  assert np.array_equal(got["out"].astype(np.float64), t.out)


# ---- alignment and layout ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,sizes,K", [(33, [3, 2, 4], 7), (70, [33, 0, 65], 66)])
def test_operands_that_are_only_4_byte_aligned(B, sizes, K):
  x, w, g = FT.inputs(9 + B, B, sizes, K)
  t, got = check_case(x, w, g, sizes, "off 1", off=1)
  aligned = run_abi(x, w, g, sizes, what="off 0")
  for name in NAMES:
    assert same(got[name], aligned[name]), name


def test_non_contiguous_inputs_are_copied():
  sizes, K, B = [3, 2, 4], 5, 12
  x, w, g = FT.inputs(10, B, sizes, K)
  tx, tw, tg = (torch.from_numpy(a).cuda() for a in (x, w, g))
  nx, nw, ng = (torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t() for a in (x, w, g))
  assert not nx.is_contiguous() and not nw.is_contiguous() and torch.equal(nx, tx)
  assert torch.equal(layer_ops.feature_insight(nx, nw, sizes), layer_ops.feature_insight(tx, tw, sizes))
  assert torch.equal(layer_ops.feature_insight(nx, nw, sizes, True), layer_ops.feature_insight(tx, tw, sizes, True))
  for a, b in zip(layer_ops.feature_insight_grad(ng, nx, nw, sizes), layer_ops.feature_insight_grad(tg, tx, tw, sizes)):
    assert torch.equal(a, b)
  wide = torch.from_numpy(np.concatenate([x, x], axis=1)).cuda()[:, :9]   # a view with a row stride of 18
  assert torch.equal(layer_ops.feature_insight(wide, tw, sizes), layer_ops.feature_insight(tx, tw, sizes))


# ---- autograd -------------------------------------------------------------------------------------------------------
def test_autograd_matches_the_grad_op_and_respects_requires_grad():
  sizes, K, B = [5, 0, 33, 2], 6, 70
  x, w, g = FT.inputs(11, B, sizes, K)
  tx, tw, tg = (torch.from_numpy(a).cuda() for a in (x, w, g))
  gi, gw = layer_ops.feature_insight_grad(tg, tx, tw, sizes)
  only_i = layer_ops.feature_insight_grad(tg, tx, tw, sizes, want_weight=False)
  only_w = layer_ops.feature_insight_grad(tg, tx, tw, sizes, want_input=False)
  assert only_i[1] is None and only_w[0] is None and torch.equal(only_i[0], gi) and torch.equal(only_w[1], gw)
  for want_i, want_w in ((True, True), (True, False), (False, True)):
    a, b = tx.clone().requires_grad_(want_i), tw.clone().requires_grad_(want_w)
    before = layer_ops.feature_insight_launch_counts()
    out = layer_ops.feature_insight(a, b, sizes)
    out.backward(tg)
    after = layer_ops.feature_insight_launch_counts()
    assert after["input_grad"] - before["input_grad"] == int(want_i)       # a gradient not needed is not computed
    assert after["weight_grad"] - before["weight_grad"] == int(want_w)
    for v, want, on in ((a, gi, want_i), (b, gw, want_w)):
      assert (torch.equal(v.grad, want) if on else v.grad is None)
  assert not layer_ops.feature_insight(tx, tw, sizes).requires_grad


def test_aggregate_with_requires_grad_takes_the_composed_route():
  sizes, K, B = [5, 0, 33, 2], 37, 40
  x, w, g = FT.inputs(12, B, sizes, K)
  t = FT.Truth(x, w, sizes)
  tx, tw = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
  before = layer_ops.feature_insight_launch_counts()
  fused = layer_ops.feature_insight(tx, tw, sizes, aggregate=True)
  mid = layer_ops.feature_insight_launch_counts()
  a, b = tx.clone().requires_grad_(), tw.clone().requires_grad_()
  composed = layer_ops.feature_insight(a, b, sizes, aggregate=True)
  after = layer_ops.feature_insight_launch_counts()
  assert (mid["aggregate"] - before["aggregate"], mid["forward"] - before["forward"]) == (1, 0)
  assert (after["aggregate"] - mid["aggregate"], after["forward"] - mid["forward"]) == (0, 1)
  with torch.no_grad():   # gradients disabled: the fused kernel again
    assert torch.equal(layer_ops.feature_insight(a, b, sizes, aggregate=True), fused)
  bounds = t.bounds()
  for name, got in (("agg", fused), ("agg_composed", composed)):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - t.agg)
    assert (err <= bounds[name]).all(), name
    USED[name] = max(USED[name], float(np.max(err / np.maximum(bounds[name], 1e-300))))
  # its gradient against an fp64 autograd composition: d agg / d out = 2 out, one more rounding of the product on
  # top of the grad op's chains, whose upstream gradient 2 c out carries the error of out
  c = torch.from_numpy(FT.inputs(13, B, [1] * len(sizes), 1)[0]).cuda()     # [B, F] upstream
  (composed * c).sum().backward()
  x64, w64 = (torch.from_numpy(v.astype(np.float64)).requires_grad_() for v in (x, w))
  off = FT.offsets(sizes)
  o64 = torch.cat([x64[:, off[f]:off[f + 1]] @ w64[off[f]:off[f + 1]] for f in range(len(sizes))], dim=1)
  ((o64 * o64).view(B, len(sizes), K).sum(dim=2) * c.cpu().double()).sum().backward()
  c64 = np.repeat(c.cpu().numpy().astype(np.float64), K, axis=1)
  up = 2 * c64 * t.out                                                              # the upstream gradient of out
  d_up = 2 * np.abs(c64) * (bounds["out"] + 2 * FT.U * np.abs(t.out))
  tg = FT.Truth(x, w, sizes, up.astype(F))
  td = FT.Truth(x, w, sizes, np.abs(d_up).astype(F) * (1 + 2.0 ** -20))
  bi = tg.bounds()["input_grad"] + td.input_grad_abs + FT.U * tg.input_grad_abs
  bw = tg.bounds()["weight_grad"] + td.weight_grad_abs + FT.U * tg.weight_grad_abs
  assert (np.abs(a.grad.cpu().numpy() - x64.grad.numpy()) <= bi).all()
  assert (np.abs(b.grad.cpu().numpy() - w64.grad.numpy()) <= bw).all()


# ---- stale tables, graph capture and the launch counts -------------------------------------------------------------
def _delta(fn):
  before = layer_ops.feature_insight_launch_counts()
  out = fn()
  after = layer_ops.feature_insight_launch_counts()
  return {n: after[n] - before[n] for n in after if after[n] != before[n]}, out


def _nonzero(d):
  return {n: v for n, v in d.items() if v}


@pytest.mark.parametrize("nseg", [4, INLINE + 2])
def test_two_calls_with_different_lists_each_get_their_own_result(nseg):
  K, B = 3, 9
  list_a = [2, 0, 1, 3] * (nseg // 4) + [3, 3][:nseg % 4]
  list_b = list(reversed(list_a))
  assert sum(list_a) == sum(list_b) and list_a != list_b
  x, w, g = FT.inputs(14, B, list_a, K)
  tx, tw, tg = (torch.from_numpy(a).cuda() for a in (x, w, g))
  got = []
  for sizes in (list_a, list_b, list_a):   # back to back, nothing waits in between
    got.append((sizes, layer_ops.feature_insight(tx, tw, sizes), layer_ops.feature_insight(tx, tw, sizes, True)) +
               layer_ops.feature_insight_grad(tg, tx, tw, sizes))
  torch.cuda.synchronize()
  for sizes, out, agg, gi, gw in got:
    d = FT.Fp32(x, w, sizes)
    assert same(out.cpu().numpy(), d.out()) and same(agg.cpu().numpy(), d.agg())
    assert same(gi.cpu().numpy(), d.input_grad(g)) and same(gw.cpu().numpy(), d.weight_grad(g))
  assert not same(got[0][1].cpu().numpy(), got[1][1].cpu().numpy())


@pytest.mark.parametrize("nseg", [4, INLINE + 2])
def test_a_replayed_graph_keeps_the_list_it_was_captured_with(nseg):
  K, B = 3, 2 * TILE + 1   # three slabs: the slab sum is part of the graph
  list_a = [2, 0, 1, 3] * (nseg // 4) + [3, 3][:nseg % 4]
  list_b = list(reversed(list_a))
  cases = [FT.inputs(s, B, list_a, K) for s in (15, 16)]
  groups = (nseg + INLINE - 1) // INLINE
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    ts = [torch.from_numpy(a).cuda() for a in cases[0]]
    layer_ops.feature_insight_grad(ts[2], ts[0], ts[1], list_a)   # (the warm-up call: the workspace is there)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()

    def capture():
      with torch.cuda.graph(graph, stream=s):
        out = layer_ops.feature_insight(ts[0], ts[1], list_a)
        agg = layer_ops.feature_insight(ts[0], ts[1], list_a, True)
        gi, gw = layer_ops.feature_insight_grad(ts[2], ts[0], ts[1], list_a)
      return out, agg, gi, gw
    counted, outs = _delta(capture)
    assert counted == {"forward": groups, "aggregate": groups, "input_grad": groups, "weight_grad": groups,
                       "slab_sum": 1}
    for x, w, g in reversed(cases):
      for t, a in zip(ts, (x, w, g)):
        t.copy_(torch.from_numpy(a))
      other = layer_ops.feature_insight(ts[0], ts[1], list_b)   # an eager call with another list in between
      layer_ops.feature_insight_grad(ts[2], ts[0], ts[1], list_b)
      graph.replay()
      s.synchronize()
      d = FT.Fp32(x, w, list_a)
      for got, want in zip(outs, (d.out(), d.agg(), d.input_grad(g), d.weight_grad(g))):
        assert same(got.cpu().numpy(), want)
      assert same(other.cpu().numpy(), FT.Fp32(x, w, list_b).out())
  torch.cuda.synchronize()


def test_launch_counts_of_every_form_and_an_empty_batch_launches_nothing():
  lib = _lib.lib()
  w9 = torch.ones(9, 6, device="cuda")
  for B, sizes, K in ((50, [3, 2, 4], 6), (2 * TILE + 1, [3, 2, 4], 6), (5, [0] * INLINE + [4, 1], 2),
                      (5, [1] * (2 * INLINE + 1), 2), (5, [0, 0], 2)):
    x, w, g = (torch.from_numpy(a).cuda() for a in FT.inputs(17, B, sizes, K))
    E = sum(sizes)
    for aggregate in (False, True):
      d, _ = _delta(lambda: layer_ops.feature_insight(x, w, sizes, aggregate))
      assert d == _nonzero(FT.launches(B, E, K, sizes, aggregate)[0]), (B, sizes, aggregate)
    for want_i, want_w in ((True, True), (True, False), (False, True)):
      d, _ = _delta(lambda: layer_ops.feature_insight_grad(g, x, w, sizes, want_i, want_w))
      assert d == _nonzero(FT.launches(B, E, K, sizes, False, want_i, want_w)[1]), (B, sizes, want_i, want_w)
  assert FT.launches(50, 9, 6, [3, 2, 4])[1] == dict(forward=0, aggregate=0, input_grad=1, weight_grad=1, slab_sum=0)
  assert FT.launches(129, 9, 6, [3, 2, 4])[1]["slab_sum"] == 1
  # batch == 0: the forward launches nothing; the gradient only clears weight_grad to +0
  cs = c_sizes([3, 2, 4])
  for aggregate in (0, 1):
    d, _ = _delta(lambda: check(lib.mhte_feature_insight(None, vp(w9), 0, 9, 6, cs, 3, aggregate, None,
                                                         3 if aggregate else 18, stream())))
    assert d == {}
  gw = Buf(54, 1)
  d, _ = _delta(lambda: check(lib.mhte_feature_insight_grad(None, 18, None, vp(w9), 0, 9, 6, cs, 3, None, vp(gw.t),
                                                            stream())))
  torch.cuda.synchronize()
  assert d == {} and not FT.bits(gw.read("empty batch")).any()
  empty = torch.zeros(0, 9, device="cuda", requires_grad=True)
  wr = w9.clone().requires_grad_()
  out = layer_ops.feature_insight(empty, wr, [3, 2, 4])
  assert out.shape == (0, 18) and layer_ops.feature_insight(empty.detach(), w9, [3, 2, 4], True).shape == (0, 3)
  out.sum().backward()
  assert empty.grad.shape == (0, 9) and not FT.bits(wr.grad.cpu().numpy()).any()


def test_the_plan_reaches_every_case():
  """Every kernel form ran in this file, in more than one launch per call where the list is long."""
  now = layer_ops.feature_insight_launch_counts()
  assert all(now[n] > REACHED[n] for n in FT.COUNTERS), (REACHED, now)
  assert layer_ops.feature_insight_plan(3, 6144, 2, FT.MAX_SEGMENTS)["groups"] == 32
  assert layer_ops.feature_insight_plan(3, 9, 2, 3) == FT.plan(3, 9, 2, 3)
  assert layer_ops.feature_insight_plan(65536, 416, 1024, 26)["forward_workspace_bytes"] == 0


def test_zz_report_the_share_of_the_bounds_used():
  print("largest share of a bound used: " + ", ".join("%s %.3f" % kv for kv in USED.items()))
  assert all(v <= 1.0 for v in USED.values())
