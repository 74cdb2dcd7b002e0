"""FeatureInsight in numpy: the truth of tests/test_feature_insight_*.py.

The formulas (native_training/layers/kernels/feature_insight_kernels.cc:70-83, :148-160; layer_ops.py:49-85), with
segment f covering the columns o_f .. o_f + s_f - 1 of input [B, E] and the same rows of weight [E, K]:

    out[b, f K + k]   = sum_{j in seg f} input[b, j] weight[j, k]
    input_grad[b, j]  = sum_k grad[b, f(j) K + k] weight[j, k]
    weight_grad[j, k] = sum_b grad[b, f(j) K + k] input[b, j]
    agg[b, f]         = sum_k out[b, f K + k]^2

``Truth`` is the fp64 value from the fp32 inputs.  ``Fp32`` is the op's own fp32 definition (csrc/mhte_fi_core.h),
bit for bit: every sum is the chain ``acc = +0; acc = fmaf(a_t, b_t, acc)`` for t ascending — over the segment's
columns (out), over k (input_grad), over the rows of one batch slab (weight_grad; the slabs' partials are then added
in slab order, starting from the first).  agg squares the ROUNDED out values in LANES = 16 chains, lane l over
k = l, l + 16, ... ascending, and adds the 16 lane sums in lane order starting from lane 0.  ``fmaf`` is evaluated
here in float64 with a round-to-odd correction (the product of two fp32 values is exact in float64; the sum is
rounded to odd at 53 bits from the error term of a two-sum, which makes the second rounding to 24 bits the correct
single rounding).

THE ERROR BOUNDS (first order in u = 2^-24, the unit roundoff of fp32; ``Truth.bounds()``).  A chain of n terms
loses at most n u times the sum of the absolute values of its terms (each fmaf rounds once; a term passes through at
most n roundings).  Adding m partials one after another loses at most (m - 1) u times the same sum.

    out          s_f terms:                     |d out|  <= s_f u  A,      A = sum_j |input weight|
    input_grad   K terms:                       |d ig|   <= K u  sum_k |grad weight|
    weight_grad  slab_rows terms in a slab, then slabs - 1 additions:
                                                |d wg|   <= (min(B, slab_rows) + slabs - 1) u  sum_b |grad input|
    agg          K squares of rounded values o~ = out + d out: the square moves by 2 |out| |d out| + |d out|^2, the
                 chain of ceil(K / 16) terms and the 15 additions by (ceil(K / 16) + 15) u of the sum of squares:
                                                |d agg|  <= sum_k (2 |out| |d out| + |d out|^2)
                                                            + (ceil(K / 16) + 15) u sum_k (|out| + |d out|)^2
    composed     the torch square and sum over the stored out: every square rounds once (u) and the sum of K terms
                 loses at most (K - 1) u in any order:
                                                |d agg|  <= sum_k (2 |out| |d out| + |d out|^2)
                                                            + K u sum_k (|out| + |d out|)^2

The tests compare against these bounds, not against tolerances tuned on results.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24

# ---- the plan, restated (csrc/mhte_fi_core.h) -------------------------------------------------------------------
TILE, STAGE, LANES, INLINE, MAX_SEGMENTS, MAX_SLABS, TARGET_GROUPS = 64, 32, 16, 128, 4096, 64, 2048
MAX_COLS = 64 * 65535
MAX_BATCH = 2 ** 30 - 64
COUNTERS = ("forward", "aggregate", "input_grad", "weight_grad", "slab_sum")
PLAN_NAMES = ("row_block", "column_tile", "stage", "inline_segments", "groups", "slab_rows", "slabs",
              "forward_workspace_bytes", "grad_workspace_bytes")


def _ceil(a, b):
  return (a + b - 1) // b


def plan(B, E, K, nseg):
  tiles = max(nseg, _ceil(E, TILE)) * _ceil(K, TILE)
  wanted = max(1, min(MAX_SLABS, _ceil(TARGET_GROUPS, tiles)))
  slab_rows = max(TILE, _ceil(_ceil(B, wanted), TILE) * TILE)
  slabs = _ceil(B, slab_rows) if B > 0 else 1
  return dict(row_block=TILE, column_tile=TILE, stage=STAGE, inline_segments=INLINE, groups=_ceil(nseg, INLINE),
              slab_rows=slab_rows, slabs=slabs, forward_workspace_bytes=0,
              grad_workspace_bytes=4 * slabs * E * K if slabs > 1 else 0)


def launches(B, E, K, sizes, aggregate=False, want_input=True, want_weight=True):
  """-> ({counter: launches} of one forward call, the same of one gradient call)."""
  groups = [sizes[i:i + INLINE] for i in range(0, len(sizes), INLINE)]
  busy = sum(1 for g in groups if max(g) > 0)
  fwd = dict.fromkeys(COUNTERS, 0)
  grd = dict.fromkeys(COUNTERS, 0)
  if B > 0:
    fwd["aggregate" if aggregate else "forward"] = len(groups)
    if E > 0:
      grd["input_grad"] = busy if want_input else 0
      grd["weight_grad"] = busy if want_weight else 0
      grd["slab_sum"] = int(want_weight and plan(B, E, K, len(sizes))["slabs"] > 1)
  return fwd, grd


def bits(x):
  return np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32)


def offsets(sizes):
  return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


# ---- fmaf, exactly ------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
  """round_fp32(a * b + c) for fp32 arrays, with ONE rounding."""
  a64, b64, c64 = (np.asarray(x, dtype=F).astype(np.float64) for x in (a, b, c))
  p = a64 * b64                      # exact: 48 bits
  s = p + c64
  bb = s - p
  err = (p - (s - bb)) + (c64 - bb)  # two-sum: p + c = s + err exactly
  s, err = np.broadcast_arrays(s, err)
  s = s.copy()
  fix = (err != 0) & np.isfinite(s) & ((s.view(np.int64) & 1) == 0)
  toward = np.where(err > 0, np.inf, -np.inf)
  s[fix] = np.nextafter(s[fix], toward[fix])   # round to odd: the sticky bit of what the 53-bit sum dropped
  return s.astype(F)


def add32(a, b):
  return (np.asarray(a, dtype=F) + np.asarray(b, dtype=F)).astype(F)


class Fp32:
  """The op's fp32 definition, bit for bit."""

  def __init__(self, inp, weight, sizes):
    self.x, self.w = np.asarray(inp, dtype=F), np.asarray(weight, dtype=F)
    self.sizes, self.off = list(sizes), offsets(sizes)
    self.B, self.E = self.x.shape
    self.K = self.w.shape[1]
    self.nseg = len(self.sizes)

  def out(self):
    res = np.zeros((self.B, self.nseg * self.K), dtype=F)
    for f in range(self.nseg):
      acc = np.zeros((self.B, self.K), dtype=F)
      for j in range(self.off[f], self.off[f + 1]):
        acc = fmaf(self.x[:, j:j + 1], self.w[j:j + 1, :], acc)
      res[:, f * self.K:(f + 1) * self.K] = acc
    return res

  def agg(self):
    o = self.out().reshape(self.B, self.nseg, self.K)
    lane = np.zeros((self.B, self.nseg, LANES), dtype=F)
    for k in range(self.K):
      lane[:, :, k % LANES] = fmaf(o[:, :, k], o[:, :, k], lane[:, :, k % LANES])
    t = lane[:, :, 0]
    for l in range(1, LANES):
      t = add32(t, lane[:, :, l])
    return t

  def input_grad(self, grad):
    g = np.asarray(grad, dtype=F).reshape(self.B, self.nseg, self.K)
    res = np.zeros((self.B, self.E), dtype=F)
    for f in range(self.nseg):
      o, e = self.off[f], self.off[f + 1]
      acc = np.zeros((self.B, e - o), dtype=F)
      for k in range(self.K):
        acc = fmaf(g[:, f, k:k + 1], self.w[o:e, k][None, :], acc)
      res[:, o:e] = acc
    return res

  def weight_grad(self, grad):
    g = np.asarray(grad, dtype=F).reshape(self.B, self.nseg, self.K)
    p = plan(self.B, self.E, self.K, self.nseg)
    seg_of = np.repeat(np.arange(self.nseg), self.sizes)   # f(j)
    total = None
    for i in range(p["slabs"]):
      acc = np.zeros((self.E, self.K), dtype=F)
      for b in range(i * p["slab_rows"], min(self.B, (i + 1) * p["slab_rows"])):
        acc = fmaf(self.x[b, :, None], g[b][seg_of, :], acc)
      total = acc if total is None else add32(total, acc)
    return total


class Truth:
  """Everything in float64 from the fp32 inputs."""

  def __init__(self, inp, weight, sizes, grad=None):
    self.x = np.asarray(inp, dtype=F).astype(np.float64)
    self.w = np.asarray(weight, dtype=F).astype(np.float64)
    self.sizes, self.off = list(sizes), offsets(sizes)
    self.B, self.E = self.x.shape
    self.K = self.w.shape[1]
    self.nseg = len(self.sizes)
    assert self.off[-1] == self.E == self.w.shape[0]
    self.seg_of = np.repeat(np.arange(self.nseg), self.sizes)
    self.out, self.out_abs = self._forward(self.x, self.w), self._forward(np.abs(self.x), np.abs(self.w))
    self.agg = (self.out ** 2).reshape(self.B, self.nseg, self.K).sum(axis=2)
    if grad is not None:
      self.g = np.asarray(grad, dtype=F).astype(np.float64).reshape(self.B, self.nseg, self.K)
      self.input_grad, self.weight_grad = self._backward(self.g, self.x, self.w)
      self.input_grad_abs, self.weight_grad_abs = self._backward(np.abs(self.g), np.abs(self.x), np.abs(self.w))

  def _forward(self, x, w):
    res = np.zeros((self.B, self.nseg * self.K))
    for f in range(self.nseg):
      o, e = self.off[f], self.off[f + 1]
      res[:, f * self.K:(f + 1) * self.K] = x[:, o:e] @ w[o:e]
    return res

  def _backward(self, g, x, w):
    ig = np.einsum("bjk,jk->bj", g[:, self.seg_of, :], w) if self.E else np.zeros((self.B, 0))
    wg = np.einsum("bjk,bj->jk", g[:, self.seg_of, :], x) if self.E else np.zeros((0, self.K))
    return ig, wg

  def bounds(self):
    """-> dict of the bounds of out, agg (fused), agg_composed and, with a grad, input_grad and weight_grad."""
    u = U
    s_of = np.repeat(np.asarray(self.sizes, dtype=np.float64), self.K)[None, :]   # the chain length per out column
    d_out = s_of * u * self.out_abs
    o, d = np.abs(self.out), d_out
    moved = (2 * o * d + d * d).reshape(self.B, self.nseg, self.K).sum(axis=2)
    mass = ((o + d) ** 2).reshape(self.B, self.nseg, self.K).sum(axis=2)
    res = dict(out=d_out, agg=moved + (_ceil(self.K, LANES) + LANES - 1) * u * mass,
               agg_composed=moved + self.K * u * mass)
    if hasattr(self, "g"):
      p = plan(self.B, self.E, self.K, self.nseg)
      res["input_grad"] = self.K * u * self.input_grad_abs
      res["weight_grad"] = (min(self.B, p["slab_rows"]) + p["slabs"] - 1) * u * self.weight_grad_abs
    return res


def inputs(seed, B, sizes, K, exact=None):
  """-> input, weight, grad as fp32 arrays; ``exact``: integers in [-exact, exact]."""
  rng = np.random.default_rng(seed)
  E = int(sum(sizes))
  if exact:
    draw = lambda *shape: rng.integers(-exact, exact + 1, shape).astype(F)  # noqa: E731
  else:
    draw = lambda *shape: rng.standard_normal(shape).astype(F)  # noqa: E731
  return draw(B, E), draw(E, K), draw(B, len(sizes) * K)
