"""The batch softmax loss in numpy float64, from the fp32 inputs: the truth of tests/test_batch_softmax_*.py.

The formula (native_training/losses/batch_softmax_loss.py:36-57, restated with the row maximum taken out):

    q^_i = q_i * rsqrt(max(sum q_i^2, 1e-12))    (likewise i^_j; the rows themselves if not normalize)
    c_j  = log(max(item_step_interval_j, 1))
    z_ij = (q^_i . i^_j) / temperature + c_j
    lse_i = m_i + log sum_j exp(z_ij - m_i),  m_i = max_j z_ij
    loss = -sum_i r_i (z_ii - lse_i)
    G_ij = r_i (exp(z_ij - lse_i) - [i == j]);  g_q^ = G I^ / T,  g_i^ = G^T Q^ / T
    through the normalisation of a row x, s = sum x^2, inv = rsqrt(max(s, 1e-12)), x^ = x inv:
        s >= 1e-12: dx = (g - x^ (x^ . g)) inv          s < 1e-12: dx = g inv

``reference_fp32`` follows the reference's own order of operations in fp32 (exp of the unshifted similarity, the
division, the log): it agrees with the truth where it is finite and is NaN where exp overflows.

THE ERROR BOUNDS (first order in u = 2^-24, the unit roundoff of fp32; ``Truth.bounds()``).  What the device does
(csrc/mhte_bsm_kernels.h) and what each step can lose:

  operands   sum of squares: an fmaf chain of at most 4 terms per lane and a tree of 6 additions, 11 u relative
             (all terms positive); inv = 1 / sqrt(max(s, eps)): half of that plus two correctly rounded operations,
             6.5 u; x * inv and, for the query, the division by T: one u each.  E_Q = 8.5 u, E_I = 7.5 u; without
             normalisation E_Q = u (the division), E_I = 0.
  s_ij       an fmaf chain of kp terms (the f32-input MFMA, kp = k padded to 8; the padding adds exact zeros):
             |ds_ij| <= ((kp + 1) u + E_Q + E_I) A_ij,  A_ij = sum_k |q^_ik i^_jk| / T
  c_j        logf within LOG_ULP = 2 ulp (the HIP math API documents 1): |dc_j| <= 2 LOG_ULP u |c_j|
  z_ij       one addition: |dz_ij| <= |ds_ij| + |dc_j| + u |z_ij|.  The diagonal z_ii of the loss is a separate row
             dot (chain and tree, at most 10 additions): the same bound holds for it.
  lse_i      lse is 1-Lipschitz in the maximum norm of its row: max_j |dz_ij| from the inputs.  From the running
             sum: a term exp(z - m) is formed against the running maximum and rescaled when that rises; the
             arguments' roundings add up to u |z_ij - m_i| (the running maxima rise monotonically to m_i), weighted
             by the term's share p_ij of the sum; every term passes at most n = tiles_per_chunk + chunks + 2
             rescalings and merges, each an expf (EXP_ULP = 2 ulp; documented 1), a multiplication and an addition,
             and 16 in-lane additions:  rel(l_i) <= u sum_j p_ij |z_ij - m_i| + n (2 EXP_ULP + 2) u + 16 u.
             Then logf and one addition:  |dlse_i| <= max_j |dz_ij| + rel(l_i) + 2 LOG_ULP u |log l_i| + u |lse_i|
  loss       the sum is fp64, rounded once:  |dloss| <= sum_i |r_i| (|dz_ii| + |dlse_i| + 2 u |z_ii - lse_i|)
             + u |loss|
  G_ij       e_ij = |dz_ij| + |dlse_i| + u |z_ij - lse_i| + 2 EXP_ULP u is the relative error of p_ij (expm1 of it,
             to keep the bound valid when it is not small);  |dG_ij| <= |r_i| (p_ij expm1(e_ij) + u |p_ij - d_ij|)
             + u |G_ij|
  g          the second product is an fmaf chain over the L = 32 tiles_per_chunk streamed rows of a chunk, then
             `chunks` additions:  |dg| <= sum |dG| |y| + (L + chunks + E_Y) u sum |G| |y|, y the other operand as
             the kernel holds it (Q^ / T, or I^ and then one division by T for the query: + u |g|).
  dx         dot = x^ . g: chain and tree, 10 u, and x^ is recomputed (E_X = 7.5 u):
             |ddot| <= sum_m |x^_m| |dg_m| + (10 u + E_X) sum_m |x^_m g_m|
             |ddx| <= inv (|dg| + |x^| |ddot| + (E_X + 2 u) |x^| |dot| + u |g - x^ dot|) + (1 + 6.5) u |dx|
             (the epsilon branch and the unnormalised form: |ddx| = |dg| inv + 7.5 u |dx|, resp. |dg|)
             and one more u |dx| for the upstream gradient.

The tests compare against these bounds, not against tolerances tuned on results.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
EXP_ULP = 2.0
LOG_ULP = 2.0
NORM_EPS = 1e-12

# ---- the plan, restated (csrc/mhte_bsm_core.h) ----------------------------------------------------------------
K_PAD, TILE, MAX_CHUNKS, TARGET_GROUPS, MAX_DIM = 8, 32, 16, 512, 256
COUNTERS = ("prep", "row/forward", "row/grad", "col", "final/lse", "final/grad")
PLAN_NAMES = ("row_block", "column_tile", "row_chunks", "column_chunks", "workspace_bytes")


def plan(B, k):
  kp = (k + K_PAD - 1) // K_PAD * K_PAD
  nb = 1 if kp <= 32 else 2 if kp <= 64 else 4 if kp <= 128 else 8
  row_block = 128 if nb <= 2 else 64
  bp = (B + row_block - 1) // row_block * row_block
  blocks = bp // row_block
  tiles = (B + TILE - 1) // TILE
  wanted = (TARGET_GROUPS + blocks - 1) // blocks if blocks else 1
  wanted = max(1, min(wanted, MAX_CHUNKS, tiles))
  tpc = max(1, (tiles + wanted - 1) // wanted)
  chunks = (tiles + tpc - 1) // tpc if tiles else 1
  up = lambda floats: (4 * floats + 255) // 256 * 256  # noqa: E731
  mat = bp * kp
  nbytes = 6 * up(bp) + 2 * up(mat) + 2 * up(chunks * bp) + up(bp) + 2 * up(chunks * mat)
  return dict(kp=kp, nb=nb, row_block=row_block, column_tile=TILE, bp=bp, blocks=blocks, tiles=tiles,
              tiles_per_chunk=tpc, chunks=chunks, row_chunks=chunks, column_chunks=chunks, workspace_bytes=nbytes)


def launches(want_query, want_item):
  """{counter: launches} of one call (either entry point)."""
  g = want_query or want_item
  return {"prep": 1, "row/forward": 1, "row/grad": int(want_query), "col": int(want_item), "final/lse": 1,
          "final/grad": int(g)}


def bits(x):
  return np.ascontiguousarray(np.asarray(x, dtype=F)).view(np.uint32)


def _normalise(x, normalize):
  s = (x * x).sum(axis=1)
  inv = 1.0 / np.sqrt(np.maximum(s, NORM_EPS)) if normalize else np.ones_like(s)
  return x * inv[:, None], inv, s


class Truth:
  """Everything in float64 from the fp32 inputs."""

  def __init__(self, query, item, interval, r, normalize=True, temperature=1.0):
    self.q = np.asarray(query, dtype=F).astype(np.float64)
    self.it = np.asarray(item, dtype=F).astype(np.float64)
    self.B, self.k = self.q.shape
    self.interval = np.asarray(interval, dtype=F).astype(np.float64).reshape(self.B)
    self.r = np.asarray(r, dtype=F).astype(np.float64).reshape(self.B)
    self.normalize, self.T = bool(normalize), float(F(temperature))
    self.qh, self.inv_q, self.s_q = _normalise(self.q, self.normalize)
    self.ih, self.inv_i, self.s_i = _normalise(self.it, self.normalize)
    self.c = np.log(np.maximum(self.interval, 1.0))
    self.z = self.qh @ self.ih.T / self.T + self.c[None, :]
    self.m = self.z.max(axis=1)
    self.l = np.exp(self.z - self.m[:, None]).sum(axis=1)
    self.lse = self.m + np.log(self.l)
    self.zd = np.diagonal(self.z).copy()
    self.loss = float(-(self.r * (self.zd - self.lse)).sum())
    self.p = np.exp(self.z - self.lse[:, None])
    self.G = self.r[:, None] * (self.p - np.eye(self.B))
    self.g_q = self.G @ self.ih / self.T
    self.g_i = self.G.T @ self.qh / self.T
    self.dquery = self._back(self.g_q, self.qh, self.inv_q, self.s_q)
    self.ditem = self._back(self.g_i, self.ih, self.inv_i, self.s_i)

  def _back(self, g, xh, inv, s):
    if not self.normalize:
      return g.copy()
    dot = (xh * g).sum(axis=1)
    full = (g - xh * dot[:, None]) * inv[:, None]
    return np.where((s >= NORM_EPS)[:, None], full, g * inv[:, None])

  def bounds(self, grad=1.0):
    """-> (loss bound, dquery bound [B, k], ditem bound [B, k]) for an upstream gradient ``grad``."""
    p = plan(self.B, self.k)
    u, T = U, self.T
    e_q, e_i = (8.5 * u, 7.5 * u) if self.normalize else (u, 0.0)
    A = np.abs(self.qh) @ np.abs(self.ih).T / T
    ds = ((p["kp"] + 1) * u + e_q + e_i) * A
    dc = 2 * LOG_ULP * u * np.abs(self.c)
    dz = ds + dc[None, :] + u * np.abs(self.z)
    n = p["tiles_per_chunk"] + p["chunks"] + 2
    share = self.p   # the share of a term in the row's sum
    rel_l = u * (share * np.abs(self.z - self.m[:, None])).sum(axis=1) + n * (2 * EXP_ULP + 2) * u + 16 * u
    dlse = dz.max(axis=1) + rel_l + 2 * LOG_ULP * u * np.abs(np.log(self.l)) + u * np.abs(self.lse)
    dzd = np.diagonal(dz)
    loss_b = (np.abs(self.r) * (dzd + dlse + 2 * u * np.abs(self.zd - self.lse))).sum() + u * abs(self.loss)
    e = dz + dlse[:, None] + u * np.abs(self.z - self.lse[:, None]) + 2 * EXP_ULP * u
    dG = np.abs(self.r)[:, None] * (self.p * np.expm1(e) + u * np.abs(self.p - np.eye(self.B))) + u * np.abs(self.G)
    L = TILE * p["tiles_per_chunk"]
    aG = np.abs(self.G)
    # the query side: y = I^, then one division by T;  the item side: y = Q^ / T
    dg_q = (dG @ np.abs(self.ih) + (L + p["chunks"]) * u * (aG @ np.abs(self.ih)) + e_i * (aG @ np.abs(self.ih))) / T
    dg_q += u * np.abs(self.g_q)
    yq = np.abs(self.qh) / T
    dg_i = dG.T @ yq + (L + p["chunks"]) * u * (aG.T @ yq) + e_q * (aG.T @ yq)
    out = []
    for g, dg, xh, inv, s, dx in ((self.g_q, dg_q, self.qh, self.inv_q, self.s_q, self.dquery),
                                  (self.g_i, dg_i, self.ih, self.inv_i, self.s_i, self.ditem)):
      if not self.normalize:
        b = dg.copy()
      else:
        e_x = 7.5 * u
        dot = (xh * g).sum(axis=1)
        ddot = (np.abs(xh) * dg).sum(axis=1) + (10 * u + e_x) * np.abs(xh * g).sum(axis=1)
        full = inv[:, None] * (dg + np.abs(xh) * ddot[:, None] + (e_x + 2 * u) * np.abs(xh) * np.abs(dot)[:, None] +
                               u * np.abs(g - xh * dot[:, None])) + 7.5 * u * np.abs(dx)
        eps = dg * inv[:, None] + 7.5 * u * np.abs(dx)
        b = np.where((s >= NORM_EPS)[:, None], full, eps)
      out.append(abs(grad) * (b + u * np.abs(dx)))
    return loss_b, out[0], out[1]


def reference_fp32(query, item, interval, r, normalize=True, temperature=1.0):
  """batch_softmax_loss.py's own order of operations, every step rounded to fp32 -> the loss as np.float32."""
  q, it = np.asarray(query, dtype=F), np.asarray(item, dtype=F)
  if normalize:
    q = (q * (F(1) / np.sqrt(np.maximum((q * q).sum(axis=1, dtype=F), F(NORM_EPS))))[:, None]).astype(F)
    it = (it * (F(1) / np.sqrt(np.maximum((it * it).sum(axis=1, dtype=F), F(NORM_EPS))))[:, None]).astype(F)
  with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
    sim = ((q @ it.T).astype(F) / F(temperature)).astype(F)
    freq = (F(1) / np.maximum(np.asarray(interval, dtype=F).reshape(-1), F(1))).astype(F)
    sim = np.exp((sim - np.log(freq).astype(F)[None, :]).astype(F)).astype(F)
    ratio = (np.diagonal(sim) / sim.sum(axis=1, dtype=F)).astype(F)
    return F(-(np.asarray(r, dtype=F).reshape(-1) * np.log(ratio).astype(F)).sum(dtype=F))


def central_differences(query, item, interval, r, normalize, temperature, h=1e-6):
  """d loss / d query and d item by central differences in float64 (small shapes only)."""
  q0, i0 = np.asarray(query, dtype=np.float64), np.asarray(item, dtype=np.float64)

  def loss(q, it):
    qh, ih = _normalise(q, normalize)[0], _normalise(it, normalize)[0]
    z = qh @ ih.T / temperature + np.log(np.maximum(np.asarray(interval, dtype=np.float64), 1.0))[None, :]
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    return -(np.asarray(r, dtype=np.float64) * (np.diagonal(z) - lse)).sum()

  dq, di = np.zeros_like(q0), np.zeros_like(i0)
  for a in range(q0.shape[0]):
    for b in range(q0.shape[1]):
      e = np.zeros_like(q0)
      e[a, b] = h
      dq[a, b] = (loss(q0 + e, i0) - loss(q0 - e, i0)) / (2 * h)
      di[a, b] = (loss(q0, i0 + e) - loss(q0, i0 - e)) / (2 * h)
  return dq, di


def inputs(seed, B, k, scale=1.0, zipf=True):
  """-> query, item, interval, r as fp32 arrays."""
  rng = np.random.default_rng(seed)
  q = (rng.standard_normal((B, k)) * scale).astype(F)
  it = (rng.standard_normal((B, k)) * scale).astype(F)
  interval = (1.0 + rng.zipf(1.5, B).clip(max=10 ** 6)).astype(F) if zipf else np.ones(B, dtype=F)
  r = rng.uniform(0.5, 1.5, B).astype(F)
  return q, it, interval, r
