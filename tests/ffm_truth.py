"""The truth of the FFM feature cross (mhte_ffm / mhte_ffm_grad), in numpy: a restatement of what the four loops
of the reference's CPU kernels (layers/kernels/ffm_kernels.cc:28-103) compute per element, float32 throughout.

Every product is rounded on its own and every sum adds ONE rounded product to the running float32 value, in the
order the loops reach an element: ascending k for a dot output, ascending r for a left gradient, ascending l for a
right gradient, each started from +0 (the loops clear their outputs first).  The feature counts come from integer
division of the widths; columns beyond the last whole feature are not read, and the gradients have the inputs'
full widths with +0 there.  numpy's float32 * and + are IEEE single operations, so the vectorised statements below
are those scalar loops, batched over everything but the summed index.
"""
import numpy as np

F = np.float32
INT_TYPES = ("multiply", "dot")


def shape(left_cols, right_cols, dim_size):
  return left_cols // dim_size, right_cols // dim_size


def forward(left, right, dim_size, int_type):
  assert left.dtype == F and right.dtype == F and int_type in INT_TYPES
  B, D = left.shape[0], dim_size
  L, R = shape(left.shape[1], right.shape[1], D)
  le = left[:, :L * D].reshape(B, L, 1, D)
  ri = right[:, :R * D].reshape(B, 1, R, D)
  prod = (le * ri).astype(F)                      # [B, L, R, D], each product rounded once
  if int_type == "multiply":
    return np.ascontiguousarray(prod.reshape(B, L * R * D))
  acc = np.zeros((B, L, R), F)                    # +0
  for k in range(D):
    acc = (acc + prod[:, :, :, k]).astype(F)
  return np.ascontiguousarray(acc.reshape(B, L * R))


def gradient(grad, left, right, dim_size, int_type):
  """-> (left_grad, right_grad).  Raises ValueError('the in/out shape not match') as FFMGradOp does."""
  assert grad.dtype == F and left.dtype == F and right.dtype == F and int_type in INT_TYPES
  B, D = left.shape[0], dim_size
  L, R = shape(left.shape[1], right.shape[1], D)
  feats = grad.shape[1] if int_type == "dot" else grad.shape[1] // D
  if feats != L * R:
    raise ValueError("the in/out shape not match")
  if int_type == "dot":
    g = np.broadcast_to(grad.reshape(B, L, R, 1), (B, L, R, D))
  else:
    g = grad[:, :L * R * D].reshape(B, L, R, D)
  le = left[:, :L * D].reshape(B, L, D)
  ri = right[:, :R * D].reshape(B, R, D)
  lg = np.zeros(left.shape, F)                    # full widths, +0 in the trailing columns
  rg = np.zeros(right.shape, F)
  acc = np.zeros((B, L, D), F)
  for r in range(R):
    acc = (acc + (g[:, :, r, :] * ri[:, None, r, :]).astype(F)).astype(F)
  lg[:, :L * D] = acc.reshape(B, L * D)
  acc = np.zeros((B, R, D), F)
  for l in range(L):
    acc = (acc + (g[:, l, :, :] * le[:, None, l, :]).astype(F)).astype(F)
  rg[:, :R * D] = acc.reshape(B, R * D)
  return lg, rg


# ---- the kernel forms -----------------------------------------------------------------------------------------
# mhte_ffm_launch_counts' order
COUNTERS = tuple("%s/%s/%s/%s" % (k, i, v, f) for k in ("forward", "gradient") for i in INT_TYPES
                 for v in ("vec4", "vec1") for f in ("lds", "direct"))
FWD_LDS_FLOATS, GRAD_LDS_FLOATS, TILE_ROWS_MAX = 8192, 16384, 64
FWD_MAX_GROUPS, GRAD_MAX_GROUPS = 1024, 512


def kernel_forms(L, R, D, aligned):
  """A restatement of the host's choice (mhte_ffm_core.h) -> [(vec, lds, tile_rows, counter)] for forward
  multiply, forward dot, gradient multiply, gradient dot.  vec 4 needs D % 4 == 0 and aligned operands; a tile's
  rows must fit 8192 floats of LDS forward ((L + R) D per row) and 16384 - 3 floats in the gradient (the slab,
  L R D or L R, plus (L + R) D), 64 rows at most; where not even one row fits: the direct form.
  Counter: 8 kernel + 4 dot + 2 (vec 1) + 1 (direct)."""
  vec = 4 if (D % 4 == 0 and aligned) else 1
  rows = []
  for kernel in (0, 1):
    for dot in (0, 1):
      if kernel == 0:
        fit = FWD_LDS_FLOATS // ((L + R) * D)
      else:
        fit = (GRAD_LDS_FLOATS - 3) // ((L * R if dot else L * R * D) + (L + R) * D)
      tile = min(fit, TILE_ROWS_MAX)
      lds = 1 if tile >= 1 else 0
      rows.append((vec, lds, tile, 8 * kernel + 4 * dot + (0 if vec == 4 else 2) + (0 if lds else 1)))
  return rows


# ---- inputs ---------------------------------------------------------------------------------------------------
def operand(rng, rows, cols, plant=True):
  """Seeded uniform values in [-10, 10], far from the subnormal range, with exact +0, -0 and a few sure negative
  values planted (an operand of fewer than 5 elements takes as many as fit)."""
  a = rng.uniform(-10.0, 10.0, size=(rows, cols)).astype(F)
  tiny = np.abs(a) < 1e-3
  a[tiny] = F(1.5)
  flat = a.reshape(-1)
  if plant and flat.size:
    spots = rng.permutation(flat.size)[:5]
    for s, v in zip(spots, (F(0.0), F(-0.0), F(-3.25), F(-7.0), F(-0.5))):
      flat[s] = v
  return a


def case(seed, B, L, R, D, int_type, left_extra=0, right_extra=0):
  """-> (left, right, upstream gradient): planted operands and a random (not all-ones) upstream gradient."""
  rng = np.random.default_rng(seed)
  left = operand(rng, B, L * D + left_extra)
  right = operand(rng, B, R * D + right_extra)
  gcols = L * R if int_type == "dot" else L * R * D
  grad = operand(rng, B, gcols)
  return left, right, grad


def bits(a):
  return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same_bits(got, want, what=""):
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  g, w = bits(got), bits(want)
  if not np.array_equal(g, w):
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r (%08x), want %r (%08x)" %
                         (what, len(bad), g.size, i, got[i], g[i], want[i], w[i]))
