"""The truth of the in-batch AUC loss (csrc/mhte_auc_core.h), in numpy: the classification of the labels, the
fp32 ``diff``, float64 terms with the reference's three branches, float64 sums.  Shared by the CPU and the GPU suite,
together with the error bounds, and with a restatement of the launch plan (the CPU suite holds it against the core
header compiled for the host).

The middle branch is evaluated in float64 in the form that cancels nothing (``e = exp(-|diff|)``): the reference's
literal ``1 - 1 / (1 + exp(-diff))`` loses every digit for a large ``diff`` in float64 as well.

Error bounds, derived and not tuned (2^-23 is the spacing of fp32 relative to a value's binade):
  a term t costs one expf (<= 1 ulp), one log1p (<= 2 ulp: the core header's own, logf of the rounded 1 + e within
  1 ulp plus an exact correction and one addition; its condition number at e in (0, 1] is <= 1) and at most one
  addition whose result is not smaller than its parts (1/2 ulp): 4 when rounded up.  The fp64
  accumulation adds nothing visible at fp32; the sum is rounded once:
      |loss - truth| <= 4 * 2^-23 * sum |t_ij| + 2^-24 * |truth|
  a weight s costs expf 1 + the addition 1 + e 1/2 + the division <= 2 1/2, and the scaled sum's rounding 1/2:
  6 when rounded up.  An element's terms all have one sign, so the bound is relative:
      |g - truth| <= 6 * 2^-23 * |truth|
The installed ROCm ships no accuracy table for expf / logf / log1pf / fp32 division (none under its share/
directory or in its HIP headers), so the figures are the ones the HIP documentation gives (expf 1, logf 1, log1pf 2,
a correctly rounded division); the 2 1/2 allowed for the division covers a build without the correctly rounded one.
"""
import numpy as np

F = np.float32
LOSS_FACTOR = 4.0
GRAD_FACTOR = 6.0
TERM_FACTOR = 4.0      # per term t, relative
WEIGHT_FACTOR = 4.0    # per weight s, relative: expf 1 + addition 1/2 + division 2 1/2
EPS = 2.0 ** -23

IGNORED, POSITIVE, NEGATIVE = 0, 1, 2

# ---- the constants of csrc/mhte_auc_core.h (tests/test_inbatch_auc_cpu.py holds them against the header) --------
TILE = 256
CHUNK = 256
STAGE = 1024
SCAN_TILE = 1024
MAX_GROUPS = 2048
GROUP_ELEMS = 64
MIN_BUDGET = 1 << 19
COUNTERS = ("count", "scan", "scatter", "pair/loss", "pair/loss+grad", "pair/grad", "final/loss", "final/loss+grad",
            "final/grad")


def bits(x):
  return np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32)


def classify(label):
  label = np.asarray(label, dtype=F).ravel()
  with np.errstate(invalid="ignore"):
    pos = label > F(0)
    neg = ~pos & (label > F(-10000))
  return np.where(pos, POSITIVE, np.where(neg, NEGATIVE, IGNORED))


def terms64(diff):
  """fp32 diffs -> (t, s) in float64, the reference's branches."""
  diff = np.asarray(diff, dtype=F)
  d = diff.astype(np.float64)
  with np.errstate(invalid="ignore", over="ignore"):
    e = np.exp(-np.abs(d))
    l = np.log1p(e)
    up = d >= 0
    tm = np.where(up, -l, d - l)
    sm = np.where(up, e, 1.0) / (1.0 + e)
    mid = (diff > F(-87)) & (diff < F(88))
    low = diff <= F(-87)
  t = np.where(mid, tm, np.where(low, d, 0.0))
  s = np.where(mid, sm, np.where(low, 1.0, 0.0))
  return t, s


def terms32(diff):
  """The device's formula with numpy's float32 functions (every operation rounded to fp32)."""
  diff = np.asarray(diff, dtype=F)
  with np.errstate(invalid="ignore", over="ignore", under="ignore"):
    e = np.exp(-np.abs(diff)).astype(F)
    l = np.log1p(e).astype(F)
    up = diff >= F(0)
    tm = np.where(up, -l, (diff - l).astype(F))
    sm = (np.where(up, e, F(1)) / (F(1) + e).astype(F)).astype(F)
    mid = (diff > F(-87)) & (diff < F(88))
    low = diff <= F(-87)
  t = np.where(mid, tm, np.where(low, diff, F(0))).astype(F)
  s = np.where(mid, sm, np.where(low, F(1), F(0))).astype(F)
  return t, s


class Truth:
  """loss, sum |t|, the gradient for grad = neg_weight = 1 (float64), the classes."""

  def __init__(self, label, logit, rows=512):
    label = np.asarray(label, dtype=F).ravel()
    logit = np.asarray(logit, dtype=F).ravel()
    if label.size != logit.size:
      raise ValueError("the label and logit not match")
    self.n = label.size
    self.cls = classify(label)
    self.pos = np.flatnonzero(self.cls == POSITIVE)
    self.neg = np.flatnonzero(self.cls == NEGATIVE)
    self.P, self.N = self.pos.size, self.neg.size
    self.row = np.zeros(self.P)   # sum_j s_ij
    self.col = np.zeros(self.N)   # sum_i s_ij
    self.loss = 0.0
    self.abs_t = 0.0
    lp, ln = logit[self.pos], logit[self.neg]
    with np.errstate(invalid="ignore"):
      for a in range(0, self.P, rows):
        diff = (lp[a:a + rows, None] - ln[None, :]).astype(F)   # one fp32 subtraction
        t, s = terms64(diff)
        self.loss += t.sum()
        self.abs_t += np.abs(t).sum()
        self.row[a:a + rows] = s.sum(axis=1)
        self.col += s.sum(axis=0)

  def gradient(self, grad=1.0, neg_weight=1.0):
    """float64, shaped [n]; a zero of either sign is +0."""
    g = np.zeros(self.n)
    if self.P and self.N:
      g[self.pos] = float(grad) * self.row
      g[self.neg] = -(float(grad) * float(neg_weight)) * self.col
    g[g == 0] = 0.0
    return g

  def loss_bound(self):
    if not np.isfinite(self.loss):
      return 0.0
    return LOSS_FACTOR * EPS * self.abs_t + 2.0 ** -24 * abs(self.loss)

  def check_loss(self, got, what=""):
    got = float(np.asarray(got, dtype=F).reshape(()))
    if not np.isfinite(self.loss):
      assert got == self.loss, (what, got, self.loss)
      return
    err, bound = abs(got - self.loss), self.loss_bound()
    print("%s loss %.9g truth %.17g err %.3g bound %.3g" % (what, got, self.loss, err, bound))
    assert err <= bound, (what, got, self.loss, err, bound)

  def check_grad(self, got, grad=1.0, neg_weight=1.0, what="", factor=GRAD_FACTOR):
    got = np.asarray(got, dtype=F).ravel()
    want = self.gradient(grad, neg_weight)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bound = factor * EPS * np.abs(want)
    rel = (err[want != 0] / np.abs(want[want != 0])).max() / EPS if np.any(want != 0) else 0.0
    print("%s gradient: largest error %.3g * 2^-23 of the truth (bound %g)" % (what, rel, factor))
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), (what, worst, got[worst], want[worst])
    zero = want == 0
    assert not bits(got[zero]).any(), what   # +0 where the truth is zero: ignored elements, no pairs, s = 0


# ---- the launch plan, restated --------------------------------------------------------------------------------
def split(A, B, budget):
  """-> (a_tiles, chunks, chunk_len, stride) of a sweep with A elements in registers against B."""
  a_tiles = (A + TILE - 1) // TILE
  stride = a_tiles * TILE
  if A == 0 or B == 0:
    return a_tiles, 0, CHUNK, stride
  cmax = max(1, budget // stride)
  minis = (B + CHUNK - 1) // CHUNK
  c = min(cmax, minis)
  per = (minis + c - 1) // c
  return a_tiles, (minis + per - 1) // per, per * CHUNK, stride


def plan(n):
  """-> dict(scan_tiles, pair_groups, final_groups, budget, loss_slots, bytes)"""
  up = lambda x, a: (x + a - 1) // a * a  # noqa: E731
  scan_tiles = (n + SCAN_TILE - 1) // SCAN_TILE
  budget = max(MIN_BUDGET, up(n, TILE))
  loss_slots = budget // TILE
  sizes = [16, 8 * scan_tiles, 8 * scan_tiles, 4 * n, 4 * n, 4 * n, 8 * loss_slots, 8 * budget, 8 * budget]
  return dict(scan_tiles=scan_tiles, pair_groups=min(MAX_GROUPS, max(1, (n + GROUP_ELEMS - 1) // GROUP_ELEMS)),
              final_groups=min(MAX_GROUPS, (n + TILE - 1) // TILE), budget=budget, loss_slots=loss_slots,
              bytes=sum(up(s, 256) for s in sizes))


def items(P, N, n):
  """work items of the first (positives in registers) and the second sweep"""
  b = plan(n)["budget"]
  s0, s1 = split(P, N, b), split(N, P, b)
  return s0[0] * s0[1], s1[0] * s1[1]


def pairs_visited(A, B, budget):
  """[(a, b)] in the order the sweep's work items reach them — the enumeration the host driver prints."""
  a_tiles, chunks, chunk_len, _ = split(A, B, budget)
  out = []
  for k in range(a_tiles * chunks):
    c, at = divmod(k, a_tiles)
    for a in range(at * TILE, min(A, (at + 1) * TILE)):
      out.extend((a, b) for b in range(c * chunk_len, min(B, (c + 1) * chunk_len)))
  return out


def smallest_two_pass_n():
  """The smallest n (a multiple of 2 * TILE, half positives and half negatives) at which every workgroup of the
  pair kernel's grid takes at least two work items in each sweep."""
  n = 2 * TILE
  while True:
    i0, i1 = items(n // 2, n // 2, n)
    if min(i0, i1) >= 2 * plan(n)["pair_groups"]:
      return n
    n += 2 * TILE


# ---- cases ----------------------------------------------------------------------------------------------------
def layout_case(seed, P, N, ignored, layout, scale=1.0):
  """label, logit of P positives, N negatives and `ignored` ignored elements.  layout: 'random' (interleaved),
  'clustered' (positives, then negatives, then the ignored ones), 'ends' (ignored elements at both ends)."""
  rng = np.random.default_rng(seed)
  n = P + N + ignored
  cls = np.array([POSITIVE] * P + [NEGATIVE] * N + [IGNORED] * ignored)
  if layout == "random":
    rng.shuffle(cls)
  elif layout == "ends":
    head = ignored // 2 if ignored > 1 else ignored
    mid = cls[:P + N].copy()
    rng.shuffle(mid)
    cls = np.concatenate([[IGNORED] * head, mid, [IGNORED] * (ignored - head)]).astype(int)
  elif layout != "clustered":
    raise ValueError(layout)
  label = np.empty(n, dtype=F)
  label[cls == POSITIVE] = rng.choice(np.array([1.0, 0.5, 2.0, 1e-30], dtype=F), size=P)
  label[cls == NEGATIVE] = rng.choice(np.array([0.0, -0.0, -1.0, -9999.5], dtype=F), size=N)
  label[cls == IGNORED] = rng.choice(np.array([-10000.0, -1e9, np.nan], dtype=F), size=ignored)
  logit = (rng.uniform(-1.0, 1.0, size=n) * scale).astype(F)
  return label, logit
