"""GPU suite of the in-batch AUC loss (csrc/mhte_auc_kernels.h, mhte_auc_host.h, monolith_amd/losses.py) against
the float64 truth of tests/inbatch_auc_truth.py and its derived bounds.  A lost or doubled pair is caught by the
gradient (for |logit| <= 1 every term of a row sum of N terms is >= 0.1, against a bound of 6 * 2^-23 * N), so every
shape case checks the loss and the gradient; every case also checks that the fused forward's unit gradient has
the bits of the gradient op with grad = 1 and that the loss has the same bits with and without it."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import inbatch_auc_truth as AT  # noqa: E402
from monolith_amd import _lib, losses  # noqa: E402
from monolith_amd._lib import check, vp  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 8                 # floats on each side of a buffer
NAN_WORD = 0x7FC0BEEF     # a quiet NaN no computation produces
GUARD_WORD = 0x7FC0CAFE


class Buf:
  """[n] float32 at ``off`` floats into storage of its own: off 0 is 16-byte aligned, off 1 has
  data_ptr() % 16 == 4.  Payload and guards start as NaN patterns."""

  def __init__(self, n, off, data=None):
    words = np.full(GUARD + off + n + GUARD, GUARD_WORD, np.uint32)
    words[GUARD + off:GUARD + off + n] = NAN_WORD if data is None else AT.bits(data).ravel()
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


def run_abi(label, logit, neg_weight=1.0, grad=1.0, off=0, grad_word=False, what=""):
  """The three forms through the C ABI on buffers at ``off`` -> (loss, gradient for `grad`).  Checks what every
  case must hold: untouched guards and inputs, the two forms' consistency."""
  label, logit = np.asarray(label, dtype=F).ravel(), np.asarray(logit, dtype=F).ravel()
  n = label.size
  dl, dg = Buf(n, off, label), Buf(n, off, logit)
  loss, loss_only = Buf(1, off), Buf(1, off)
  unit, g1, g = Buf(n, off), Buf(n, off), Buf(n, off)
  word = torch.tensor([grad], dtype=torch.float32, device="cuda") if grad_word else None
  lib = _lib.lib()
  check(lib.mhte_inbatch_auc_loss(vp(dl.t), vp(dg.t), n, neg_weight, vp(loss.t), vp(unit.t), stream()))
  check(lib.mhte_inbatch_auc_loss(vp(dl.t), vp(dg.t), n, neg_weight, vp(loss_only.t), None, stream()))
  check(lib.mhte_inbatch_auc_loss_grad(vp(dl.t), vp(dg.t), n, 1.0, None, neg_weight, vp(g1.t), stream()))
  check(lib.mhte_inbatch_auc_loss_grad(vp(dl.t), vp(dg.t), n, 7.0 if grad_word else grad, vp(word), neg_weight,
                                       vp(g.t), stream()))
  torch.cuda.synchronize()
  assert np.array_equal(AT.bits(dl.read(what)), AT.bits(label)) and np.array_equal(AT.bits(dg.read(what)), AT.bits(logit))
  got_loss, got_unit = loss.read(what), unit.read(what)
  assert np.array_equal(AT.bits(got_loss), AT.bits(loss_only.read(what))), what + ": the loss with and without the gradient"
  assert np.array_equal(AT.bits(got_unit), AT.bits(g1.read(what))), what + ": the fused unit gradient and the gradient op"
  return got_loss[0], got_unit, g.read(what)


def check_case(label, logit, what, neg_weight=1.0, grad=1.0, off=0, grad_word=False, truth=None):
  truth = truth or AT.Truth(label, logit)
  loss, unit, g = run_abi(label, logit, neg_weight, grad, off, grad_word, what)
  truth.check_loss(loss, what)
  truth.check_grad(unit, 1.0, neg_weight, what + " unit")
  truth.check_grad(g, grad, neg_weight, what + " grad=%g" % grad)
  return truth, loss, unit, g


# ---- tile and class edges -------------------------------------------------------------------------------------
EDGE_PN = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (255, 257), (256, 256)]
# tile - 1, tile, tile + 1 of each tile and chunk constant of the core header, in both roles
CONSTS = sorted({AT.TILE, AT.CHUNK, AT.STAGE, AT.SCAN_TILE})
EDGE_PN += [(c + d, 300) for c in CONSTS for d in (-1, 0, 1)] + [(300, c + d) for c in CONSTS for d in (-1, 0, 1)]


@pytest.mark.parametrize("pn", EDGE_PN, ids=lambda pn: "P%d-N%d" % pn)
def test_tile_and_class_edges(pn):
  P, N = pn
  for k, (layout, ignored) in enumerate((("random", 37), ("clustered", 5), ("ends", 70), ("random", 0))):
    if P + N + ignored == 0:
      continue
    label, logit = AT.layout_case(1000 * k + P * 7 + N, P, N, ignored, layout)
    t, *_ = check_case(label, logit, "P=%d N=%d %s" % (P, N, layout))
    assert (t.P, t.N) == (P, N)


def test_one_case_past_one_grid_pass():
  """The smallest n, taken from the plan, at which every workgroup of the pair kernel takes two work items or more
  in each sweep (half positives, half negatives)."""
  n = AT.smallest_two_pass_n()
  i0, i1 = AT.items(n // 2, n // 2, n)
  groups = AT.plan(n)["pair_groups"]
  assert i0 >= 2 * groups and i1 >= 2 * groups and groups < AT.MAX_GROUPS
  label, logit = AT.layout_case(77, n // 2, n // 2, 0, "random")
  check_case(label, logit, "n=%d, %d + %d items on %d workgroups" % (n, i0, i1, groups))


# ---- exact counts ---------------------------------------------------------------------------------------------
def _t0():
  loss, _, _ = run_abi([1, 0], [0.37, 0.37], what="t0")
  assert abs(float(loss) + math.log(2.0)) <= AT.LOSS_FACTOR * AT.EPS * math.log(2.0)
  return float(loss)


# the last one: chunks of 1 280 elements in both sweeps, longer than one LDS stage (the budget caps the chunk
# count); 5.28e8 pairs, which the closed form checks without a truth
EXACT_PN = [(1, 1), (1000, 3000), (4000, 5000), (5000, 5000), (8000, 9000), (33000, 16000)]


def test_exact_count_cases_straddle_two_to_the_24():
  e = [math.frexp(P * N * math.log(2.0))[1] - 1 for P, N in EXACT_PN]
  assert min(e) < 24 <= max(e) and 23 in e and 24 in e, e
  assert all(P * N < 2 ** 29 for P, N in EXACT_PN)   # P N t0 fits fp64's 53 bits
  P, N = EXACT_PN[-1]
  budget = AT.plan(P + N + 11)["budget"]
  assert AT.split(P, N, budget)[2] > AT.STAGE and AT.split(N, P, budget)[2] > AT.STAGE
  assert all(AT.split(p, n, AT.plan(p + n + 11)["budget"])[2] == AT.CHUNK for p, n in EXACT_PN[:-1])


@pytest.mark.parametrize("pn", EXACT_PN, ids=lambda pn: "P%d-N%d" % pn)
def test_exact_counts_with_all_logits_equal(pn):
  """Every s is exactly 0.5 and every t the same t0: the gradient is a closed form and the loss counts the pairs.
  P N t0 needs up to 53 bits: every fp64 partial sum is exact, an fp32 one is not."""
  P, N = pn
  t0 = _t0()
  label, _ = AT.layout_case(P + N, P, N, 11, "random")
  logit = np.full(label.size, 0.37, dtype=F)
  cls = AT.classify(label)
  for nw, grad in ((1.0, 1.0), (0.25, 2.0), (0.25, -0.5)):
    loss, unit, g = run_abi(label, logit, nw, grad, what="exact")
    assert AT.bits(loss) == AT.bits(F(P * N * t0)), (P, N, loss, F(P * N * t0))
    want = np.zeros(label.size, dtype=F)
    want[cls == AT.POSITIVE] = F(grad * N / 2)
    want[cls == AT.NEGATIVE] = F(-grad * nw * P / 2)
    assert np.array_equal(AT.bits(g), AT.bits(want)), (P, N, nw, grad)


# ---- the branches ---------------------------------------------------------------------------------------------
def test_exact_branches_on_the_device():
  """Diffs of the outer branches only (negative logit 0, so diff = the positive's logit; then the mirror): every
  term is exact, so loss and gradient have the truth's bits."""
  pos = np.array([-87, -200, 88, 200, np.nan, np.inf, -1000], dtype=F)
  for label, logit in ((np.r_[np.ones(7), 0, -10000, np.nan].astype(F), np.r_[pos, 0, 5, 5].astype(F)),
                       (np.r_[np.zeros(7), 1, -1e9].astype(F), np.r_[-pos, 0, 5].astype(F))):
    t = AT.Truth(label, logit)
    for nw, grad in ((1.0, 1.0), (0.5, 3.0)):
      loss, unit, g = run_abi(label, logit, nw, grad, what="branches")
      assert AT.bits(loss) == AT.bits(F(t.loss)), (loss, t.loss)
      assert np.array_equal(AT.bits(g), AT.bits(t.gradient(grad, nw).astype(F)))
      assert np.array_equal(AT.bits(unit), AT.bits(t.gradient(1.0, nw).astype(F)))
  loss, unit, _ = run_abi([1, 0], [-np.inf, 0.0], what="-inf")
  assert loss == -np.inf and list(unit) == [1.0, -1.0]


def test_branch_and_classification_edges_on_the_device():
  """Diffs at -87, 88, their inward neighbours, +-200, NaN and +-inf beside ordinary ones, labels at the
  classification edges: within the bounds, +0 where the truth is zero."""
  edge = np.array([-87, np.nextafter(F(-87), F(0)), 88, np.nextafter(F(88), F(0)), 200, -200, np.nan, np.inf, -60,
                   60, 0.25], dtype=F)
  pos_label = np.array([2, 1e-30], dtype=F)
  neg_label = np.array([0, -0.0, -9999.5], dtype=F)
  ign_label = np.array([-10000, -1e9, np.nan], dtype=F)
  # positives at the edge logits against negatives at 0 (diff = the edge) and at +-0.5; then the mirror image
  for mirror in (False, True):
    a = np.resize(pos_label if not mirror else neg_label, edge.size)
    b = np.resize(neg_label if not mirror else pos_label, 3)
    label = np.r_[ign_label[:1], a, ign_label[1:], b, ign_label].astype(F)
    logit = np.r_[9, -edge if mirror else edge, 9, 9, 0, 0.5, -0.5, 9, 9, 9].astype(F)
    t, loss, unit, g = check_case(label, logit, "edges mirror=%d" % mirror, neg_weight=0.5, grad=2.0)
    assert (t.P, t.N) == ((3, edge.size) if mirror else (edge.size, 3))
    ignored = t.cls == AT.IGNORED
    assert ignored.sum() == 6 and not AT.bits(g[ignored]).any() and not AT.bits(unit[ignored]).any()


# ---- moderate size, scaling -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_moderate_size(scale):
  n = 8192
  P = int(0.3 * n)
  label, logit = AT.layout_case(int(scale), P, n - P, 0, "random", scale)
  check_case(label, logit, "n=8192 scale=%g" % scale)


def test_neg_weight_and_grad_scaling():
  label, logit = AT.layout_case(9, 300, 500, 20, "random", 3.0)
  truth = AT.Truth(label, logit)
  for nw in (1.0, 0.25):
    for grad in (1.0, 2.0, -0.5):
      for word in (False, True):
        check_case(label, logit, "nw=%g grad=%g word=%d" % (nw, grad, word), nw, grad, 0, word, truth)


# ---- the Python layer -------------------------------------------------------------------------------------------
def test_reference_test_cases_through_the_python_ops():
  label = torch.tensor([1, 0, 0, 1], dtype=torch.float32, device="cuda")
  logit = torch.tensor([0.5, -0.2, -0.4, 0.8], dtype=torch.float32, device="cuda")
  loss = losses.inbatch_auc_loss(label, logit, neg_weight=1.0)
  assert loss.shape == () and loss.dtype == torch.float32 and abs(loss.item() - (-1.3208841)) <= 1e-6
  g = losses.inbatch_auc_loss_grad(label, logit, 2.0, 1.0)
  np.testing.assert_allclose(g.cpu().numpy(), [1.2417255, -1.2015073, -1.0410514, 1.0008333], rtol=1e-6, atol=1e-6)
  gw = losses.inbatch_auc_loss_grad(label, logit, torch.tensor(2.0, device="cuda"), 1.0)
  assert torch.equal(g, gw)


def test_autograd_shapes_and_refusals():
  n = 700
  label_h, logit_h = AT.layout_case(4, 250, 400, 50, "random", 2.0)
  truth = AT.Truth(label_h, logit_h)
  label = torch.from_numpy(label_h).cuda()
  logit = torch.from_numpy(logit_h).cuda().reshape(n, 1).requires_grad_(True)   # [n, 1] against a [n] label
  loss = losses.inbatch_auc_loss(label, logit, 0.5)
  truth.check_loss(loss.item(), "python")
  (g3,) = torch.autograd.grad(3.0 * loss, logit)
  assert g3.shape == (n, 1) and g3.dtype == torch.float32
  op3 = losses.inbatch_auc_loss_grad(label, logit.detach(), 3.0, 0.5)
  assert op3.shape == (n, 1)
  # the backward scales the rounded unit gradient, the op rounds once: half an ulp apart, both within the bound
  truth.check_grad(op3.cpu().numpy(), 3.0, 0.5, "grad op")
  truth.check_grad(g3.cpu().numpy(), 3.0, 0.5, "autograd")
  assert np.abs(g3.cpu().numpy() - op3.cpu().numpy()).max() <= 2 * AT.EPS * np.abs(op3.cpu().numpy()).max()
  (g1,) = torch.autograd.grad(losses.inbatch_auc_loss(label, logit, 0.5), logit)
  assert torch.equal(g1, losses.inbatch_auc_loss_grad(label, logit.detach(), 1.0, 0.5))
  assert losses.inbatch_auc_loss(label, logit).grad_fn is not None
  with pytest.raises(ValueError, match="the label and logit not match"):
    losses.inbatch_auc_loss(label[:-1], logit)
  with pytest.raises(ValueError, match="the label and logit not match"):
    losses.inbatch_auc_loss_grad(label, logit.detach()[:-1].contiguous(), 1.0, 1.0)
  with pytest.raises(ValueError, match="logit must be contiguous"):
    losses.inbatch_auc_loss(label, torch.zeros(n, 2, device="cuda")[:, 0])


# ---- house rules ------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits():
  label, logit = AT.layout_case(21, 700, 900, 30, "random", 5.0)
  runs = [run_abi(label, logit, 0.5, 2.0, what="twice") for _ in range(2)]
  for a, b in zip(*runs):
    assert np.array_equal(AT.bits(a), AT.bits(b))


def test_unaligned_operands_give_the_same_bits():
  label, logit = AT.layout_case(22, 300, 1025, 9, "ends")
  a = run_abi(label, logit, 0.5, 2.0, off=0, what="aligned")
  for off in (1, 3):
    b = run_abi(label, logit, 0.5, 2.0, off=off, what="off %d" % off)
    for x, y in zip(a, b):
      assert np.array_equal(AT.bits(x), AT.bits(y))


def test_replays_in_a_graph():
  """The forward with its unit gradient and the gradient op with a device grad word, captured into one graph on a
  side stream and replayed on rewritten inputs (other counts of positives and negatives included): each replay has
  the eager call's bits."""
  n = 1500
  cases = [AT.layout_case(s, P, n - P - 40, 40, "random", 2.0) for s, P in ((31, 500), (32, 70), (33, 1200))]
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    tl, tg = (torch.from_numpy(a).cuda() for a in cases[0])
    word = torch.tensor(1.0, device="cuda")
    losses.inbatch_auc_loss(tl, tg, 0.5)   # (the warm-up call: the workspace is there)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
      loss, unit = losses._forward(tl, tg, 0.5, want_grad=True)
      grad = losses.inbatch_auc_loss_grad(tl, tg, word, 0.5)
    for k, (label, logit) in enumerate(cases[1:]):
      tl.copy_(torch.from_numpy(label))
      tg.copy_(torch.from_numpy(logit))
      word.fill_(-1.5 - k)
      g.replay()
      s.synchronize()
      got = [t.cpu().numpy().copy() for t in (loss, unit, grad)]
      e_loss, e_unit = losses._forward(tl, tg, 0.5, want_grad=True)
      e_grad = losses.inbatch_auc_loss_grad(tl, tg, -1.5 - k, 0.5)
      for a, b in zip(got, (e_loss, e_unit, e_grad)):
        assert np.array_equal(AT.bits(a), AT.bits(b.cpu().numpy()))
      AT.Truth(label, logit).check_grad(got[2], -1.5 - k, 0.5, "replay %d" % k)
  torch.cuda.synchronize()


def test_launch_counts_name_every_form_and_an_empty_batch_launches_nothing():
  label, logit = (torch.from_numpy(a).cuda() for a in AT.layout_case(5, 40, 50, 3, "random"))
  loss = torch.full((), 7.0, device="cuda")
  lib = _lib.lib()

  def delta(fn):
    before = losses.inbatch_auc_launch_counts()
    fn()
    after = losses.inbatch_auc_launch_counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}

  common = {"count": 1, "scan": 1, "scatter": 1}
  assert delta(lambda: losses._forward(label, logit, 1.0, False)) == dict(common, **{"pair/loss": 1, "final/loss": 1})
  assert delta(lambda: losses._forward(label, logit, 1.0, True)) == dict(common, **{"pair/loss+grad": 1,
                                                                                       "final/loss+grad": 1})
  assert delta(lambda: losses.inbatch_auc_loss_grad(label, logit, 2.0)) == dict(common, **{"pair/grad": 1,
                                                                                            "final/grad": 1})
  # n == 0: no launch, the loss cleared to +0
  assert delta(lambda: check(lib.mhte_inbatch_auc_loss(None, None, 0, 1.0, vp(loss), None, stream()))) == {}
  assert delta(lambda: check(lib.mhte_inbatch_auc_loss_grad(None, None, 0, 1.0, None, 1.0, None, stream()))) == {}
  assert AT.bits(loss.cpu().numpy()) == 0
  empty = torch.zeros(0, device="cuda", requires_grad=True)
  out = losses.inbatch_auc_loss(torch.zeros(0, device="cuda"), empty)
  assert out.item() == 0.0 and torch.autograd.grad(out, empty)[0].shape == (0,)
  assert set(losses.inbatch_auc_launch_counts()) == set(AT.COUNTERS)
