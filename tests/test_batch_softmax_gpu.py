"""GPU suite of the batch softmax loss (csrc/mhte_bsm_kernels.h, mhte_bsm_host.h, monolith_amd/losses.py) against
the float64 truth of tests/batch_softmax_truth.py and its derived bounds.  Every case goes through the C ABI on
guarded buffers and checks, besides the bounds: the loss has the same bits with and without gradients, the forward's
unit gradients have the bits of the grad entry with grad = 1, a single requested gradient has the bits of the pair,
a second call repeats the first one's bits, and no guard word or input changes.

Measured on an MI355X (the largest share of its bound any case of this file used): loss 0.11, dquery 0.10,
ditem 0.22."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import batch_softmax_truth as BT  # noqa: E402
from monolith_amd import _lib, entry, losses  # noqa: E402
from monolith_amd._lib import check, vp  # noqa: E402
from monolith_amd.multi_hash_table_ops import MultiHashTable  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 8                 # floats on each side of a buffer
NAN_WORD = 0x7FC0BEEF     # a quiet NaN no computation produces
GUARD_WORD = 0x7FC0CAFE
USED = {"loss": 0.0, "dquery": 0.0, "ditem": 0.0}   # the largest share of a bound any case used (printed)


class Buf:
  """n float32 at ``off`` floats into storage of its own: off 0 is 16-byte aligned, off 1 has
  data_ptr() % 16 == 4.  Payload and guards start as NaN patterns."""

  def __init__(self, n, off, data=None):
    words = np.full(GUARD + off + n + GUARD, GUARD_WORD, np.uint32)
    words[GUARD + off:GUARD + off + n] = NAN_WORD if data is None else BT.bits(data).ravel()
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
  return np.array_equal(BT.bits(a), BT.bits(b))


def run_abi(q, it, iv, r, normalize, T, grad=1.0, off=0, what=""):
  """Every form through the C ABI on buffers at ``off`` -> (loss, unit dquery, unit ditem, dquery and ditem for
  ``grad``), with the consistency checks every case must hold."""
  B, k = q.shape
  ins = [Buf(x.size, off, x) for x in (q, it, iv, r)]
  p = [vp(b.t) for b in ins]
  lib = _lib.lib()
  norm = int(normalize)
  outs = {}

  def fwd(name, want_q, want_i):
    loss, uq, ui = Buf(1, off), Buf(B * k, off) if want_q else None, Buf(B * k, off) if want_i else None
    check(lib.mhte_batch_softmax_loss(*p, B, k, norm, T, vp(loss.t), vp(uq.t) if uq else None,
                                      vp(ui.t) if ui else None, stream()))
    outs[name] = (loss, uq, ui)

  def bwd(name, want_q, want_i, g, word=None):
    dq, di = Buf(B * k, off) if want_q else None, Buf(B * k, off) if want_i else None
    check(lib.mhte_batch_softmax_loss_grad(*p, B, k, norm, T, g, vp(word), vp(dq.t) if dq else None,
                                           vp(di.t) if di else None, stream()))
    outs[name] = (None, dq, di)

  word = torch.tensor([grad], dtype=torch.float32, device="cuda")
  fwd("both", True, True)
  fwd("again", True, True)
  fwd("loss", False, False)
  fwd("q", True, False)
  bwd("unit", True, True, 1.0)
  bwd("i", False, True, 1.0)
  bwd("host", True, True, grad)
  bwd("word", True, True, 7.0, word)
  torch.cuda.synchronize()
  got = {n: tuple(None if b is None else b.read(what + " " + n) for b in v) for n, v in outs.items()}
  for b, x in zip(ins, (q, it, iv, r)):
    assert same(b.read(what), x.ravel()), what + ": an input changed"
  loss, uq, ui = got["both"]
  for a, b in zip(got["both"], got["again"]):
    assert same(a, b), what + ": two calls differ"
  assert same(loss, got["loss"][0]) and same(loss, got["q"][0]), what + ": the loss with and without gradients"
  assert same(uq, got["q"][1]) and same(uq, got["unit"][1]), what + ": dquery across the forms"
  assert same(ui, got["i"][2]) and same(ui, got["unit"][2]), what + ": ditem across the forms"
  assert same(got["host"][1], got["word"][1]) and same(got["host"][2], got["word"][2]), what + ": grad and grad_dev"
  return loss[0], uq.reshape(B, k), ui.reshape(B, k), got["host"][1].reshape(B, k), got["host"][2].reshape(B, k)


def check_case(q, it, iv, r, normalize, T, what, grad=1.0, off=0):
  t = BT.Truth(q, it, iv, r, normalize, T)
  loss, uq, ui, dq, di = run_abi(q, it, iv, r, normalize, T, grad, off, what)
  lb, qb, ib = t.bounds()
  for name, got, want, bound in (("loss", loss, t.loss, lb), ("dquery", uq, t.dquery, qb), ("ditem", ui, t.ditem, ib)):
    share = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(bound, 1e-300)))
    USED[name] = max(USED[name], share)
    print("%s: %s uses %.3f of its bound" % (what, name, share))
    assert np.isfinite(got).all() and share <= 1.0, (what, name, share)
  if grad != 1.0:
    _, qg, ig = t.bounds(grad)
    assert (np.abs(dq - grad * t.dquery) <= qg).all() and (np.abs(di - grad * t.ditem) <= ig).all(), what
  for g in (uq, ui, dq, di):
    assert not np.signbit(g[g == 0]).any(), what + ": a zero gradient must be +0"
  return t, loss, uq, ui


# ---- row blocks, tiles and chunks -----------------------------------------------------------------------------
def _shape_cases():
  cases = []
  for k in (16, 100):   # the two row-block heights
    p = losses.batch_softmax_plan(1000, k)
    rb, tile = p["row_block"], p["column_tile"]
    assert (rb, tile) == ((128, 32) if k == 16 else (64, 32))
    for B in sorted({1, 2, tile - 1, tile, tile + 1, rb - 1, rb, rb + 1}):
      cases.append((B, k))
  cases.append((544, 64))   # several row blocks, several chunks, the last chunk short
  cases.append((300, 64))
  return cases


def test_the_plan_reaches_every_case():
  assert losses.batch_softmax_plan(32, 16)["row_chunks"] == 1                 # one chunk
  p = losses.batch_softmax_plan(544, 64)
  tiles = (544 + p["column_tile"] - 1) // p["column_tile"]
  per = (tiles + p["row_chunks"] - 1) // p["row_chunks"]
  assert 544 > 4 * p["row_block"] and p["row_chunks"] > 1 and tiles % per != 0   # the last chunk holds fewer tiles
  assert per > 1                                                               # ... and a chunk several
  p = losses.batch_softmax_plan(300, 64)
  assert p["row_chunks"] == 10 and p["column_chunks"] == 10                    # one tile per chunk
  assert p == {n: BT.plan(300, 64)[n] for n in BT.PLAN_NAMES}


@pytest.mark.parametrize("B,k", _shape_cases())
@pytest.mark.parametrize("normalize", [True, False])
def test_shapes_within_the_bounds(B, k, normalize):
  q, it, iv, r = BT.inputs(B * 1000 + k, B, k, scale=1.0 if normalize else 0.5)
  check_case(q, it, iv, r, normalize, 0.5 if normalize else 0.7, "B %d k %d" % (B, k))


@pytest.mark.parametrize("k", [1, 2, 3, 16, 33, 64, 100, 256])
@pytest.mark.parametrize("normalize", [True, False])
def test_dims_within_the_bounds(k, normalize):
  B = 70
  q, it, iv, r = BT.inputs(k, B, k, scale=1.0 if normalize else 2.0 / np.sqrt(k))
  check_case(q, it, iv, r, normalize, 0.25 if normalize else 1.0, "k %d" % k, grad=-2.5)


# ---- value edges ------------------------------------------------------------------------------------------------
def test_intervals_are_clamped_at_one():
  B, k = 40, 8
  q, it, _, r = BT.inputs(21, B, k)
  ones = run_abi(q, it, np.ones(B, dtype=F), r, True, 0.5, what="ones")
  iv = np.resize(np.array([0, 0.5, -3, 1, -0.0, -1e30], dtype=F), B)
  clamped = run_abi(q, it, iv, r, True, 0.5, what="clamped")
  for a, b in zip(ones, clamped):
    assert same(a, b)
  iv = np.resize(np.array([1e6, 1, 37.5, 2], dtype=F), B)
  check_case(q, it, iv, r, True, 0.5, "interval 1e6")


def test_r_zero_negative_and_mixed():
  B, k = 45, 12
  q, it, iv, r = BT.inputs(22, B, k)
  loss, uq, ui, dq, di = run_abi(q, it, iv, np.zeros(B, dtype=F), True, 0.3, grad=-3.0, what="r = 0")
  assert BT.bits(loss) == 0
  for g in (uq, ui, dq, di):
    assert not BT.bits(g).any()   # +0 everywhere, also under a negative upstream gradient
  check_case(q, it, iv, -r, True, 0.3, "r negative")
  mixed = (r * np.resize(np.array([1, -1, 0, 2.5], dtype=F), B)).astype(F)
  check_case(q, it, iv, mixed, False, 0.9, "r mixed", grad=0.5)


def test_all_zero_rows_take_the_epsilon_branch():
  B, k = 37, 10
  q, it, iv, r = BT.inputs(23, B, k)
  q[3] = 0
  it[5] = 0
  q[36] = 1e-8   # a sum of squares below the epsilon that is not zero
  t, _, uq, ui = check_case(q, it, iv, r, True, 0.5, "zero rows")
  assert t.inv_q[3] == 1e6 and t.inv_i[5] == 1e6 and t.s_q[36] < BT.NORM_EPS
  assert np.abs(uq[3]).max() > 1e4 and np.abs(ui[5]).max() > 1e4   # g * 1e6


@pytest.mark.parametrize("T", [1.0, 0.05, 0.01])
def test_temperatures_with_normalised_inputs(T):
  B, k = 150, 24
  q, it, iv, r = BT.inputs(24, B, k)
  it[:10] = q[:10] * 2   # aligned pairs: q^ . i^ = 1
  t, loss, _, _ = check_case(q, it, iv, r, True, T, "T %g" % T)
  ref = BT.reference_fp32(q, it, iv, r, True, T)
  if T == 0.01:
    assert np.isnan(ref) and np.isfinite(loss)   # the one defined deviation: exp(100) overflows in the reference
  else:
    assert abs(float(ref) - t.loss) <= t.bounds()[0] + 2 * B * BT.U * np.abs(t.r * (t.zd - t.lse)).sum()


def test_unnormalised_rows_of_norm_thirty():
  B, k = 130, 36
  q, it, iv, r = BT.inputs(25, B, k, scale=5.0)   # |row| about 5 * 6 = 30
  t, _, _, _ = check_case(q, it, iv, r, False, 1.0, "norm 30")
  assert 20 < np.sqrt(t.s_q).mean() < 40 and (t.z.max(axis=1) - t.z.min(axis=1)).max() > 300


# ---- alignment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k", [(33, 7), (129, 64), (70, 100)])
def test_operands_that_are_only_4_byte_aligned(B, k):
  q, it, iv, r = BT.inputs(26 + B, B, k)
  t, loss, uq, ui = check_case(q, it, iv, r, True, 0.2, "off 1", off=1)
  aligned = run_abi(q, it, iv, r, True, 0.2, what="off 0")
  assert same(loss, aligned[0]) and same(uq, aligned[1]) and same(ui, aligned[2])


# ---- autograd -------------------------------------------------------------------------------------------------------
def test_autograd_scales_the_unit_gradients_and_respects_requires_grad():
  B, k = 90, 20
  q, it, iv, r = BT.inputs(27, B, k)
  t = BT.Truth(q, it, iv, r, True, 0.5)
  tq, ti, tv, tr = (torch.from_numpy(x).cuda() for x in (q, it, iv, r))
  unit_q, unit_i = losses.batch_softmax_loss_grad(tq, ti, tv, tr, 1.0, True, 0.5)
  for want_q, want_i in ((True, True), (True, False), (False, True)):
    a, b = tq.clone().requires_grad_(want_q), ti.clone().requires_grad_(want_i)
    loss = losses.batch_softmax_loss(a, b, tv, tr, True, 0.5)
    assert loss.shape == () and abs(loss.item() - t.loss) <= t.bounds()[0]
    (loss * -1.75).backward()
    for x, unit, want in ((a, unit_q, want_q), (b, unit_i, want_i)):
      if want:
        assert torch.equal(x.grad, unit * -1.75)   # (one exact fp32 product per element)
      else:
        assert x.grad is None
  plain = losses.batch_softmax_loss(tq, ti, tv, tr, True, 0.5)
  assert not plain.requires_grad
  word = torch.tensor(-1.75, device="cuda")
  dq, di = losses.batch_softmax_loss_grad(tq, ti, tv, tr, word, True, 0.5)
  hq, hi = losses.batch_softmax_loss_grad(tq, ti, tv, tr, -1.75, True, 0.5)
  assert torch.equal(dq, hq) and torch.equal(di, hi)
  only_i = losses.batch_softmax_loss_grad(tq, ti, tv, tr, -1.75, True, 0.5, want_query=False)
  assert only_i[0] is None and torch.equal(only_i[1], hi)


# ---- graph capture and the launch counts ------------------------------------------------------------------------
def _delta(fn):
  before = losses.batch_softmax_launch_counts()
  out = fn()
  after = losses.batch_softmax_launch_counts()
  return {n: after[n] - before[n] for n in after if after[n] != before[n]}, out


def _nonzero(d):
  return {n: v for n, v in d.items() if v}


def test_replays_in_a_graph_and_counts_its_launches():
  B, k = 200, 48
  cases = [BT.inputs(s, B, k) for s in (31, 32, 33)]
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    ts = [torch.from_numpy(a).cuda() for a in cases[0]]
    word = torch.tensor(1.0, device="cuda")
    losses._bsm_forward(*ts, True, 0.1, True, True)   # (the warm-up call: the workspace is there)
    s.synchronize()
    g = torch.cuda.CUDAGraph()

    def both():
      with torch.cuda.graph(g, stream=s):
        fw = losses._bsm_forward(*ts, True, 0.1, True, True)
        bw = losses.batch_softmax_loss_grad(*ts, word, True, 0.1)
      return fw + bw
    counted, outs = _delta(both)
    want = {n: BT.launches(True, True)[n] * 2 for n in BT.COUNTERS}
    assert counted == want and sum(want.values()) == 12   # six launches per form with both gradients
    for n, case in enumerate(cases[1:]):
      for t, a in zip(ts, case):
        t.copy_(torch.from_numpy(a))
      word.fill_(-1.5 - n)
      g.replay()
      s.synchronize()
      got = [t.cpu().numpy().copy() for t in outs]
      eager = losses._bsm_forward(*ts, True, 0.1, True, True) + \
          losses.batch_softmax_loss_grad(*ts, -1.5 - n, True, 0.1)
      for a, b in zip(got, eager):
        assert same(a, b.cpu().numpy())
      t64 = BT.Truth(*case, True, 0.1)
      assert abs(float(got[0]) - t64.loss) <= t64.bounds()[0]
      assert (np.abs(got[3] - (-1.5 - n) * t64.dquery) <= t64.bounds(-1.5 - n)[1]).all()
  torch.cuda.synchronize()


def test_launch_counts_of_every_form_and_an_empty_batch_launches_nothing():
  q, it, iv, r = (torch.from_numpy(a).cuda() for a in BT.inputs(34, 50, 6))
  for want_q, want_i in ((False, False), (True, False), (False, True), (True, True)):
    d, _ = _delta(lambda: losses._bsm_forward(q, it, iv, r, True, 1.0, want_q, want_i))
    assert d == _nonzero(BT.launches(want_q, want_i)), (want_q, want_i)
    if want_q or want_i:
      d, _ = _delta(lambda: losses.batch_softmax_loss_grad(q, it, iv, r, 2.0, True, 1.0, want_q, want_i))
      assert d == _nonzero(BT.launches(want_q, want_i)), (want_q, want_i)
  assert sum(BT.launches(False, False).values()) == 3 and sum(BT.launches(True, True).values()) == 6
  # batch == 0: no launch, the loss cleared to +0
  lib = _lib.lib()
  loss = torch.full((), 7.0, device="cuda")
  d, _ = _delta(lambda: check(lib.mhte_batch_softmax_loss(None, None, None, None, 0, 4, 1, 1.0, vp(loss), None, None,
                                                          stream())))
  assert d == {} and BT.bits(loss.cpu().numpy()) == 0
  out = torch.zeros(1, device="cuda")
  d, _ = _delta(lambda: check(lib.mhte_batch_softmax_loss_grad(None, None, None, None, 0, 4, 1, 1.0, 1.0, None,
                                                               vp(out), None, stream())))
  assert d == {}
  empty = torch.zeros(0, 4, device="cuda", requires_grad=True)
  z = torch.zeros(0, device="cuda")
  got = losses.batch_softmax_loss(empty, torch.zeros(0, 4, device="cuda"), z, z)
  assert got.item() == 0.0 and torch.autograd.grad(got, empty)[0].shape == (0, 4)


# ---- the loop closed with the table ---------------------------------------------------------------------------------
def test_intervals_of_a_batch_softmax_optimizer_table_feed_the_loss():
  B, k = 64, 16
  mt = MultiHashTable.from_configs({"t": entry.make_table_config(
      [entry.CombineAsSegment(1, entry.ZerosInitializer(), entry.BatchSoftmaxOptimizer(0.1))])},
      name_suffix="bsm_loop")
  ids = torch.arange(1, B + 1, dtype=torch.int64, device="cuda")
  ones = torch.ones(B, 1, device="cuda")
  mt.apply_gradients({"t": (ids, ones)}, global_step=100)
  mt.apply_gradients({"t": (ids[::2].contiguous(), ones[::2].contiguous())}, global_step=1500)
  mt.apply_gradients({"t": (ids, ones)}, global_step=4000)
  interval = mt.lookup({"t": ids})["t"]   # [B, 1] on the device, never read on the host by the loss
  iv = interval.cpu().numpy().reshape(B)
  assert len(np.unique(iv)) >= 2 and iv.max() > 100   # the two histories, some above the clamp
  q, it, _, r = BT.inputs(35, B, k)
  tq, ti, tr = (torch.from_numpy(x).cuda().requires_grad_(n < 2) for n, x in enumerate((q, it, r)))
  loss = losses.batch_softmax_loss(tq, ti, interval, tr, True, 0.05)
  loss.backward()
  t = BT.Truth(q, it, iv, r, True, 0.05)
  lb, qb, ib = t.bounds()
  assert abs(loss.item() - t.loss) <= lb
  assert (np.abs(tq.grad.cpu().numpy() - t.dquery) <= qb).all() and (np.abs(ti.grad.cpu().numpy() - t.ditem) <= ib).all()


def test_zz_report_the_share_of_the_bounds_used():
  print("largest share of a bound used: " + ", ".join("%s %.3f" % kv for kv in USED.items()))
  assert all(v <= 1.0 for v in USED.values())
