"""GPU test (-m gpu) of the dense tower's GEMMs (mhte_dense_mlp_*, csrc/mhte_gemm_kernels.h) with
operands for which every sum is exact in fp32, so that every output bit is compared: no tolerance.

Inputs, weights, biases and dy are small integers and lr is a power of two.  Every bf16 operand and
every product is then exact, and every partial sum of every GEMM, row-dot, bias gradient and slab sum
is a multiple of one quantum q with magnitude below 2^24 q — representable in fp32, whatever the
summation order of the kernel (MFMA k-order, split-K slabs, trees).  The only roundings left are the
round-to-nearest-even casts to bf16 of stored activations, gradients and weight copies, which the
reference mirrors with torch's ``.to(torch.bfloat16)``; everything else it computes in float64.
The reference itself asserts the conditions this rests on (``RefExact``): operands are multiples of
their quantum, sum |a||b| / q < 2^24 for every output element, 20-80 % of the ReLU gates of every
hidden layer open, and at least 1 % of every layer's stored activations above 256 quanta (bf16 keeps
8 bits: those are rounded, odd ones are ties).  CASES holds the committed value ranges and seeds.

What a forward AFTER an SGD step can show exactly.  Updated weights w - lr g carry the ~12 bits of a
16 384-row gradient sum; two such layers in a row need 8 + 8 + 10 bits per 1024-term sum and more in
the next: no choice of ranges makes the whole refreshed tower exact.  The refreshed bf16 copies are
therefore read by a PROBE forward: the layers other than the probed one are re-seeded (set_params)
with 0 / 2^j selection matrices and the input has a few non-zeros per row, so the SGD-written copy
W_l of the probed layer is read with sums of a few terms and reaches the logits through exact sums;
the step is repeated from the same integers for every probed layer (which also shows that a step is
reproducible bit for bit).  The fp32 master weights of every layer are compared exactly after every
step in any case.

Which tile ran is asserted from the handle's launch counters (mhte_dense_mlp_launch_counts): the
256 x 256 instantiation is reached only through a host heuristic."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from monolith_amd.dense_mlp import DenseMlp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
LIMIT = float(2 ** 24)


def _bf16(t):
  """float64 -> the float64 value of its bf16 rounding (through fp32, which holds it exactly)."""
  f = t.to(torch.float32)
  assert torch.equal(f.to(F64), t), "the reference's value is not an fp32 number"
  return f.to(torch.bfloat16).to(F64)


def _quantum(*tensors):
  """The largest power of two that divides every element (1.0 for all-zero tensors)."""
  qe = None
  for t in tensors:
    t = t.to(F64).flatten()
    t = t[t != 0]
    if t.numel() == 0:
      continue
    assert bool(torch.isfinite(t).all())
    m, e = torch.frexp(t)                                   # t = m 2^e, 0.5 <= |m| < 1
    mi = (m.abs() * float(2 ** 53)).to(torch.int64)
    tz = torch.log2((mi & -mi).to(F64)).round()             # trailing zeros of the 53-bit significand
    lo = int((e.to(F64) - 53 + tz).min())
    qe = lo if qe is None else min(qe, lo)
  return 1.0 if qe is None else 2.0 ** qe


class RefExact:
  """float64 reference of the tower's arithmetic with the kernels' bf16 casts, asserting on the way
  that the fp32 arithmetic of the kernels is exact for these operands.  ``margin[what]`` keeps the
  largest sum |a||b| / q relative to 2^24 per kind of sum, ``gates`` / ``big`` the open-gate fraction
  and the share of stored activations above 256 quanta per hidden layer of the last forward."""

  def __init__(self, widths):
    self.widths = list(widths)
    self.nl = len(widths) - 2
    self.w = [None] * (self.nl + 1)
    self.b = [None] * (self.nl + 1)
    self.margin = {}

  def set_params(self, layer, w, b):
    self.w[layer] = w.to(F64).reshape(self.widths[layer + 1], self.widths[layer]).clone()
    self.b[layer] = b.to(F64).reshape(self.widths[layer + 1]).clone()

  def _bound(self, what, mag, q):
    m = float(mag.max()) / q / LIMIT
    self.margin[what] = max(self.margin.get(what, 0.0), m)
    assert m < 1.0, ("sum |a||b| / quantum reaches 2^24: fp32 sums are not exact", what, m)

  def _gemm(self, what, a, b, bias=None):
    """a [M][K] b[N][K]^T (+ bias[N]); every partial sum a multiple of q below 2^24 q."""
    q = _quantum(a) * _quantum(b)
    mag = a.abs() @ b.abs().t()
    out = a @ b.t()
    if bias is not None:
      q = min(q, _quantum(bias))
      mag = mag + bias.abs()
      out = out + bias
    self._bound(what, mag, q)
    return out

  def forward(self, x, stats=True):
    self.h = [_bf16(x.to(F64))]
    assert torch.equal(self.h[0], x.to(F64)), "x is not exact in bf16"
    self.gates, self.big = [], []
    for l in range(self.nl):
      z = self._gemm("forward", self.h[-1], _bf16(self.w[l]), self.b[l])
      h = _bf16(torch.relu(z))
      self.gates.append(float((h > 0).double().mean()))
      self.big.append(float((h.abs() > 256 * _quantum(h)).double().mean()))
      self.h.append(h)
    if stats:
      for l in range(self.nl):
        assert 0.2 <= self.gates[l] <= 0.8, ("open ReLU gates", l, self.gates[l])
        assert self.big[l] >= 0.01, ("stored activations above 256 quanta", l, self.big[l])
    return self.logits()

  def logits(self):
    """The last layer over the hidden activations of the last forward (fp32 weights, not rounded)."""
    y = self._gemm("rowdot", self.h[-1], self.w[-1], self.b[-1]).view(-1)
    return y.to(torch.float32)

  def backward(self, dy, lr, need_dx=True):
    """-> dx (fp32) or None; SGD on every layer."""
    dy = dy.to(F64)
    nl = self.nl
    gw, gb = [None] * (nl + 1), [None] * (nl + 1)
    top = self.h[-1]
    gw[nl] = self._gemm("dW_last", dy.view(1, -1), top.t().contiguous())
    gb[nl] = dy.sum().view(1)
    self._bound("db_last", dy.abs().sum(), _quantum(dy))
    wl = self.w[nl].view(1, -1)
    self._bound("dy*w_last", dy.abs().max() * wl.abs().max(), _quantum(dy) * _quantum(wl))
    dz = _bf16((top > 0).to(F64) * dy.view(-1, 1) * wl)
    dx = None
    for l in range(nl - 1, -1, -1):
      gw[l] = self._gemm("wgrad", dz.t().contiguous(), self.h[l].t().contiguous())
      gb[l] = dz.sum(0)
      self._bound("db", dz.abs().sum(0), _quantum(dz))
      if l > 0 or need_dx:
        d = self._gemm("dgrad", dz, _bf16(self.w[l]).t().contiguous())
        if l > 0:
          dz = _bf16(d * (self.h[l] > 0).to(F64))
        else:
          dx = d.to(torch.float32)
          assert torch.equal(dx.to(F64), d)
    for l in range(nl + 1):
      for p, g in ((self.w[l], gw[l].view_as(self.w[l])), (self.b[l], gb[l])):
        self._bound("sgd", p.abs() + lr * g.abs(), min(_quantum(p), lr * _quantum(g)))
      self.w[l] = self.w[l] - lr * gw[l].view_as(self.w[l])
      self.b[l] = self.b[l] - lr * gb[l]
    return dx


# ---- committed operand ranges (integers drawn uniformly from [-r, r]; see make_case) and seeds.
# Tuned with RefExact alone at the real shapes; its assertions hold the conditions.
#   x, w[l], b[l]: ranges of the input and of every GEMM layer; bal[l] > 0: the layer's weights are
#   bal[l] / 2 entries +1 and as many -1 per row instead (sparse and BALANCED: the mean of the ReLU
#   outputs below would otherwise shift whole columns of the next layer by the row sum of W, and the
#   16 384-row sums of the last layer's gradient over such a column reach 2^24);
#   last: magnitudes 1..last of the second draw of w_last (the first draw is +-1); dy: 1..dy, signed.
CASES = {
    "tile256": dict(widths=[1024, 1024, 1024, 1], batch=16384, x=2, w=[5, 1], bal=[0, 128], b=[8, 8],
                    last=1, dy=1, lr=2.0 ** -11, seed=101, slices=2),
    "tile256_shallow": dict(widths=[1024, 1024, 1], batch=16384, x=2, w=[5], bal=[0], b=[8], last=2, dy=1,
                            lr=2.0 ** -11, seed=102),
    "square4096": dict(widths=[256, 4096, 4096, 1], batch=4096, x=4, w=[8, 1], bal=[0, 128], b=[16, 16], last=2,
                       dy=1, lr=2.0 ** -9, seed=108, slices=8),
    "wgrad256_b128": dict(widths=[4096, 4096, 1], batch=128, x=2, w=[3], bal=[0], b=[8], last=3, dy=3,
                          lr=2.0 ** -6, seed=103),
    "wgrad256_b256": dict(widths=[4096, 4096, 1], batch=256, x=2, w=[3], bal=[0], b=[8], last=3, dy=3,
                          lr=2.0 ** -6, seed=104),
    "tile128_deep": dict(widths=[256, 384, 128, 1], batch=512, x=4, w=[8, 2], bal=[0, 0], b=[16, 16],
                         last=3, dy=3, lr=2.0 ** -8, seed=105),
    "one_workgroup": dict(widths=[128, 128, 1], batch=128, x=5, w=[10], bal=[0], b=[16], last=3, dy=3,
                          lr=2.0 ** -6, seed=106),
    "batches": dict(widths=[256, 256, 1], batch=2048, x=4, w=[8], bal=[0], b=[16], last=3, dy=3,
                    lr=2.0 ** -8, seed=107),
}


def _ints(gen, r, shape, nonzero=False):
  if nonzero:
    mag = torch.randint(1, r + 1, shape, generator=gen)
    return (mag * (2 * torch.randint(0, 2, shape, generator=gen) - 1)).to(torch.float32)
  return torch.randint(-r, r + 1, shape, generator=gen).to(torch.float32)


def make_case(name, batch=None, reseed=0, device="cuda"):
  """The integers of a case: x [B][w0], per GEMM layer (W, b), two draws of w_last without zeros
  (+-1, then magnitudes 1..last), b_last, dy [B] without zeros."""
  c = CASES[name]
  widths, B = c["widths"], batch or c["batch"]
  gen = torch.Generator().manual_seed(c["seed"] + 1000 * reseed)
  out = {"name": name, "widths": widths, "batch": B, "lr": c["lr"]}
  out["x"] = _ints(gen, c["x"], (B, widths[0])).to(device)
  out["w"], out["b"] = [], []
  for l in range(len(widths) - 2):
    shape = (widths[l + 1], widths[l])
    w = _ints(gen, c["w"][l], shape)
    if c["bal"][l]:
      half = c["bal"][l] // 2
      order = torch.rand(shape, generator=gen).argsort(1)
      w = torch.zeros(shape)
      w.scatter_(1, order[:, :half], 1.0)
      w.scatter_(1, order[:, half:2 * half], -1.0)
    out["w"].append(w.to(device))
    out["b"].append(_ints(gen, c["b"][l], (widths[l + 1],)).to(device))
  out["last"] = [_ints(gen, 1, (widths[-2],), nonzero=True).to(device),
                 _ints(gen, c["last"], (widths[-2],), nonzero=True).to(device)]
  if c["last"] == 1:   # (two DIFFERENT draws also where both are +-1)
    assert not torch.equal(out["last"][0], out["last"][1])
  out["b_last"] = _ints(gen, 4, (1,)).to(device)
  out["dy"] = _ints(gen, c["dy"], (B,), nonzero=True).to(device)
  return out


def _load(mlp, ref, case, draw):
  nl = len(case["widths"]) - 2
  for l in range(nl):
    mlp.set_params(l, case["w"][l], case["b"][l])
    ref.set_params(l, case["w"][l], case["b"][l])
  mlp.set_params(nl, case["last"][draw], case["b_last"])
  ref.set_params(nl, case["last"][draw], case["b_last"])


def _same(got, exp, what):
  """Bit-exact, all elements; the message names the first mismatching indices (tile, wave, part)."""
  assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
  if not torch.equal(got, exp):
    bad = (got != exp).nonzero()
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r; last at %s" % (
        what, bad.shape[0], got.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(exp[tuple(bad[0])]),
        bad[-1].tolist()))


def _counts_delta(mlp, before):
  now = mlp.launch_counts()
  return {r: (now[r][0] - before[r][0], now[r][1] - before[r][1]) for r in now}


def run_step(mlp, ref, case, need_dx=True, report=None):
  """Loads the case's integers, forward with both draws of w_last, backward + SGD with the second;
  y, dx and every layer's parameters bit-exact against the reference.  -> dx."""
  nl = len(case["widths"]) - 2
  x, dy, lr = case["x"], case["dy"], case["lr"]
  ref.margin = {}
  for draw in (0, 1):
    _load(mlp, ref, case, draw)
    y_ref = ref.forward(x)
    _same(mlp.forward(x), y_ref, "y (draw %d of w_last)" % draw)
  dx_ref = ref.backward(dy, lr, need_dx)
  dx = mlp.backward(dy, lr, need_dx=need_dx)
  if need_dx:
    _same(dx, dx_ref, "dx")
  for l in range(nl + 1):
    w, b = mlp.get_params(l)
    _same(w.to(F64), ref.w[l], "weights of layer %d after the step" % l)   # (fp32 -> fp64 is exact)
    _same(b.to(F64), ref.b[l], "bias of layer %d after the step" % l)
  if report is not None:
    report.append({"case": case["name"], "batch": case["batch"],
                   "margin_vs_2^24": {k: round(v, 4) for k, v in ref.margin.items()},
                   "gates_open": [round(g, 3) for g in ref.gates], "above_256_quanta": [round(g, 4) for g in ref.big]})
  return dx


def _selection(N, K, device):
  """W [N][K] that passes its input on: N <= K folds it, W[n][k] = 2^(k // N) where k % N == n (sums of
  K / N terms with distinct powers of two); N > K copies it into the first K outputs and leaves the
  rest zero (an input with one non-zero keeps one non-zero)."""
  n = torch.arange(N, device=device).view(N, 1)
  k = torch.arange(K, device=device).view(1, K)
  return ((k % N) == n).to(torch.float32) * (2.0 ** (k // N).to(torch.float32))


def probe_inputs(case, layer):
  """-> ([(layer index, W, b)] to re-seed, x2, [w_last of every probe forward]): selection matrices in
  the GEMM layers other than ``layer``; x2 with max(1, w0 / B) ones per row (every input column is
  used); the last layer without bias, the first draw (+-1) cut into CASES[..]["slices"] slices of the
  top layer's outputs, one forward each (every output is read by exactly one: a row-dot over all 4096
  outputs of updated weights would pass 2^24 quanta)."""
  widths, B = case["widths"], case["batch"]
  nl = len(widths) - 2
  dev = case["x"].device
  sets = [(j, _selection(widths[j + 1], widths[j], dev), torch.zeros(widths[j + 1], device=dev))
          for j in range(nl) if j != layer]
  x2 = torch.zeros(B, widths[0], device=dev)
  rows = torch.arange(B, device=dev)
  for i in range(max(1, widths[0] // B)):
    x2[rows, (rows + i * B) % widths[0]] = 1.0
  n_slices = CASES[case["name"]].get("slices", 1)
  idx = torch.arange(widths[-2], device=dev) * n_slices // widths[-2]
  lasts = [case["last"][0] * (idx == s).to(torch.float32) for s in range(n_slices)]
  return sets, x2, lasts


def run_probe(mlp, ref, case, layer):
  """After a step: the SGD-written bf16 copy W of ``layer`` (and its bias) read by forwards whose
  other layers are re-seeded (probe_inputs).  -> forwards run."""
  sets, x2, lasts = probe_inputs(case, layer)
  for j, w, b in sets:
    mlp.set_params(j, w, b)
    ref.set_params(j, w, b)
  zero = torch.zeros(1, device=x2.device)
  for s, w_last in enumerate(lasts):
    mlp.set_params(ref.nl, w_last, zero)
    ref.set_params(ref.nl, w_last, zero)
    y_ref = ref.forward(x2, stats=False) if s == 0 else ref.logits()
    _same(mlp.forward(x2), y_ref, "logits of the probe forward through layer %d, slice %d" % (layer, s))
  return len(lasts)


def run_case(name, report=None, probe=True):
  """One exact step of a case, then per GEMM layer the probe of its refreshed copy (the step repeated
  from the same integers for every layer after the first).  -> (launch counts, forwards run)."""
  case = make_case(name)
  nl = len(case["widths"]) - 2
  mlp = DenseMlp(case["widths"], max_batch=case["batch"])
  ref = RefExact(case["widths"])
  steps = probes = 0
  for layer in range(nl if probe else 1):
    run_step(mlp, ref, case, report=report if layer == 0 else None)
    steps += 1
    if probe:
      probes += run_probe(mlp, ref, case, layer)
  counts = mlp.launch_counts()
  mlp.close()
  return counts, steps, probes


def _expect(nl, steps, probes, big):
  """Launch counts of ``steps`` steps (two forwards each) and ``probes`` probe forwards of a tower
  with nl GEMM layers; ``big``: the roles that take the 256 x 256 tile."""
  per = {"forward": nl * (2 * steps + probes), "dgrad": (nl - 1) * steps, "dgrad_input": steps, "wgrad": nl * steps}
  return {r: ((0, n) if r in big else (n, 0)) for r, n in per.items()}


REPORT = []


def _print_report():
  for r in REPORT:
    print("EXACT-MARGINS " + json.dumps(r))
  del REPORT[:]


# ---- 1. the 256 x 256 tile in forward, dgrad and dgradF32

def test_tile256_forward_dgrad_exact():
  """[1024, 1024, 1024, 1] at B = 16384: forward and both input gradients are 64 x 4 = 256 workgroups
  of the 256 x 256 tile (asserted from the launch counters); ht of layer 0, dzt of both layers and
  xt are observed through the weight gradients that read them (128 tile: 4 x 4 x 8 slices)."""
  counts, steps, probes = run_case("tile256", REPORT)
  _print_report()
  assert counts == _expect(2, steps, probes, ("forward", "dgrad", "dgrad_input")), counts


def test_tile256_square_transposed_outputs_exact():
  """[256, 4096, 4096, 1] at B = 4096: both forwards (M = B = 4096, N = 4096), the gradient below the
  top GEMM layer and that layer's weight gradient (M = N = 4096, one slice) are 16 x 16 = 256
  workgroups of the 256 tile, and the transposed outputs ht / dzt of its epilogue are SQUARE: a
  transposed write with row and column block exchanged stays inside its buffer at this shape and
  shows as wrong values (ht of layer 0 through dW_1, dzt of layer 0 through dW_0 and db_0).  Layer
  0's weight gradient (16 x 1 tiles, 8 slices) and dx (16 x 1) take the 128 tile."""
  counts, steps, probes = run_case("square4096", REPORT)
  _print_report()
  nfwd = 2 * steps + probes
  assert counts == {"forward": (0, 2 * nfwd), "dgrad": (0, steps), "dgrad_input": (steps, 0),
                    "wgrad": (steps, steps)}, counts


# ---- 2. the 256 x 256 tile in wgrad

@pytest.mark.parametrize("name", ["wgrad256_b128", "wgrad256_b256"])
def test_tile256_wgrad_exact(name):
  """[4096, 4096, 1]: M = N = 4096, one slice: 16 x 16 = 256 workgroups of the 256 tile in the weight
  gradient; forward and dx take the 128 tile (B = 128: M not a multiple of 256)."""
  counts, steps, probes = run_case(name, REPORT)
  _print_report()
  assert counts == _expect(1, steps, probes, ("wgrad",)), counts


# ---- 3. the 128 x 128 tile at the shapes of test_dense_mlp_gpu.py

@pytest.mark.parametrize("name", ["tile128_deep", "one_workgroup"])
def test_tile128_exact(name):
  """[256, 384, 128, 1] at B = 512 (N = 384: 12 workgroups, not a multiple of 8: no XCD renumbering)
  and [128, 128, 1] at B = 128 (one workgroup)."""
  counts, steps, probes = run_case(name, REPORT)
  _print_report()
  assert counts == _expect(len(CASES[name]["widths"]) - 2, steps, probes, ()), counts


# ---- 4. batches below max_batch

def test_batches_below_max_batch_exact():
  """One DenseMlp([256, 256, 1], max_batch=2048) stepped at B = 2048, 384, 128, 1152, 2048: split_now
  16, 2, 2, 2, 16, ldct = B inside buffers sized for 2048, slabs and part_last with stale content of
  the larger step.  Variant: the weights are RE-SEEDED to fresh integers (set_params, another draw per
  step) before every step — after one step they are multiples of lr with the bits of a gradient sum,
  and a forward over them is not exact (module docstring); each step is compared exactly."""
  mlp = DenseMlp(CASES["batches"]["widths"], max_batch=2048)
  ref = RefExact(CASES["batches"]["widths"])
  steps = 0
  for i, B in enumerate((2048, 384, 128, 1152, 2048)):
    case = make_case("batches", batch=B, reseed=i)
    run_step(mlp, ref, case, report=REPORT)
    steps += 1
  _print_report()
  counts = mlp.launch_counts()
  mlp.close()
  assert counts == _expect(1, steps, 0, ()), counts


# ---- 5. need_dx=False

def test_need_dx_false_leaves_identical_parameters():
  """The same tower and data stepped with and without dx: bit-identical parameters; the dx of the
  first run equals the reference (run_step)."""
  case = make_case("tile128_deep")
  nl = len(case["widths"]) - 2
  params = []
  for need_dx in (True, False):
    mlp = DenseMlp(case["widths"], max_batch=case["batch"])
    ref = RefExact(case["widths"])
    dx = run_step(mlp, ref, case, need_dx=need_dx)
    assert (dx is not None) == need_dx
    params.append([mlp.get_params(l) for l in range(nl + 1)])
    counts = mlp.launch_counts()
    assert counts["dgrad_input"] == ((1, 0) if need_dx else (0, 0)), counts
    mlp.close()
  for l in range(nl + 1):
    _same(params[1][l][0], params[0][l][0], "weights of layer %d without dx" % l)
    _same(params[1][l][1], params[0][l][1], "bias of layer %d without dx" % l)


# ---- 6. non-finite inputs

NONFINITE = {"+inf": 0x7f800000, "-inf": 0xff800000, "quiet nan": 0x7fc00000, "nan 0x7fffffff": 0x7fffffff,
             "nan 0xffffffff": 0xffffffff}


@pytest.mark.parametrize("name", ["tile128_deep", "tile256_shallow"])
def test_nonfinite_input_reaches_its_row_only(name):
  """+-Inf, the quiet NaN and the full-mantissa NaN patterns in ONE element of x make exactly that row
  of y non-finite; every other row is bit-identical to the clean run.  (0x7fffffff / 0xffffffff
  used to carry through the rounding add of f32_to_bf16 into -0.0 / +0.0, and fmaxf in the ReLU
  returned 0 for a NaN pre-activation.)"""
  case = make_case(name)
  mlp = DenseMlp(case["widths"], max_batch=case["batch"])
  ref = RefExact(case["widths"])
  _load(mlp, ref, case, 1)
  x = case["x"]
  y_clean = mlp.forward(x).clone()
  _same(y_clean, ref.forward(x), "y of the clean run")
  B, K = x.shape
  for i, (what, bits) in enumerate(sorted(NONFINITE.items())):
    row, col = (37 + 131 * i) % B, (5 + 67 * i) % K
    xd = x.clone()
    xd.view(torch.int32)[row, col] = bits - (1 << 32) if bits >= (1 << 31) else bits
    y = mlp.forward(xd)
    assert not bool(torch.isfinite(y[row])), (what, row, col, float(y[row]))
    keep = torch.ones(B, dtype=torch.bool, device=x.device)
    keep[row] = False
    _same(y[keep].view(torch.int32), y_clean[keep].view(torch.int32), "rows beside the one with %s" % what)
  mlp.close()


# ---- the 128 x 128 tile forced at the large shape, in a fresh process

def _child_main():
  """(child of test_forced_tile128_in_a_child_process) MHTE_GEMM_TILE128 is read once per process."""
  counts, steps, probes = run_case("tile256_shallow")
  print("CHILD-COUNTS " + json.dumps({"counts": counts, "steps": steps, "probes": probes}))


def test_forced_tile128_in_a_child_process():
  """Case 1 at reduced depth ([1024, 1024, 1], B = 16384) with MHTE_GEMM_TILE128 set, in a fresh child
  process: the same exact outputs (the child runs the same comparisons) and no 256-tile launch; the
  parent runs the same case without the variable and sees the 256 tile."""
  counts, steps, probes = run_case("tile256_shallow", REPORT)
  _print_report()
  assert counts == _expect(1, steps, probes, ("forward", "dgrad_input")), counts
  env = dict(os.environ, MHTE_GEMM_TILE128="1")
  code = ("import sys; sys.path[:0] = [%r, %r]; import test_dense_mlp_exact_gpu as t; t._child_main()"
          % (ROOT, os.path.join(ROOT, "tests")))
  r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
  assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
  line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD-COUNTS ")]
  assert len(line) == 1, r.stdout[-2000:]
  got = json.loads(line[0][len("CHILD-COUNTS "):])
  exp = _expect(1, got["steps"], got["probes"], ())
  assert {k: tuple(v) for k, v in got["counts"].items()} == exp, got
  assert all(v[1] == 0 for v in got["counts"].values()), got
