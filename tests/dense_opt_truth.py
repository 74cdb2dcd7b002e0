"""The numpy truth of the dense optimizers (csrc/mhte_dense_opt_core.h): Adamom and RMSprop, V1 and V2, on
float32 arrays with every operation rounded on its own (numpy's float32 ``*``, ``+``, ``-``, ``/`` and ``sqrt``
are the correctly rounded IEEE ones; no FMA), ``rsqrt(x) := 1 / sqrt(x)``.  The expression trees are the
reference's, optimizers/cc/kernels/training_ops.cc:34-121.

The reference does not pin the bits (Eigen's packet rsqrt on the CPU, rsqrtf and contracted FMAs on the GPU);
its goldens (adamom_test.py:24-51, rmsprop_test.py:25-60, rmspropv2_test.py:22-58) hold for this restatement
within their own eps = 1e-8 (largest deviation 6.2e-9), which tests/test_dense_optimizers_cpu.py asserts.

How the device's division and square root treat float32 subnormals is not part of the contract: ``Tracker``
asserts that no intermediate of the suites' seeded sets is subnormal."""
import numpy as np

F = np.float32
TINY = np.finfo(np.float32).tiny
NAN_BITS = 0x7fc00000

KINDS = ("adamom", "adamom_v2", "rmsprop", "rmsprop_v2")
SLOTS = {"adamom": ("m", "v", "c"), "adamom_v2": ("m", "v", "c"), "rmsprop": ("m", "v"), "rmsprop_v2": ("m", "v")}

# the hyper-parameters of the suites: weight decay on, no value a power of two (every product rounds)
HYPER = {
    "adamom": dict(learning_rate=0.013, ada_decay=0.97, mom_decay=0.87, epsilon=1e-3, weight_decay=0.011),
    "adamom_v2": dict(learning_rate=0.013, ada_decay=0.97, mom_decay=0.87, epsilon=1e-3, weight_decay=0.011),
    "rmsprop": dict(learning_rate=0.017, beta1=0.83, beta2=0.93, epsilon=1e-3, weight_decay=0.013),
    "rmsprop_v2": dict(learning_rate=0.017, beta1=0.83, beta2=0.93, epsilon=1e-3, weight_decay=0.013),
}


class Tracker:
  """Watches the intermediates of the truth: ``seen_subnormal`` becomes True when a finite non-zero one lies
  below the smallest normal float32."""

  def __init__(self):
    self.seen_subnormal = False

  def __call__(self, x):
    a = np.abs(np.asarray(x))
    if np.any((a > 0) & (a < TINY)):
      self.seen_subnormal = True
    return x


def _noop(x):
  return x


def grad_after_decay(var, g0, grad_scale, wd, w=_noop):
  grad = w(np.asarray(g0).astype(F) * F(grad_scale))     # (an fp16 gradient converts exactly)
  return w(w(F(wd) * var) + grad)


def adamom(var, m, v, c, g0, learning_rate, ada_decay, mom_decay, epsilon, weight_decay, grad_scale=1.0,
           update_slots=True, use_v2=False, watch=None):
  """-> (var, m, v, c) after one step; the inputs stay."""
  w = watch or _noop
  lr, ada, mom, eps = F(learning_rate), F(ada_decay), F(mom_decay), F(epsilon)
  with np.errstate(all="ignore"):
    g = grad_after_decay(var, g0, grad_scale, weight_decay, w)
    if update_slots:
      m = w(w(mom * m) + w(w(F(1.0) - mom) * g))
      v = w(w(ada * v) + w(g * g))
      c = w(w(ada * c) + F(1.0))
    ml = w(m * lr)
    q = w(v / c)
    if use_v2:
      step = w(ml / w(w(np.sqrt(q)) + eps))
    else:
      step = w(ml * w(F(1.0) / w(np.sqrt(w(q + eps)))))
    return w(var - step), m, v, c


def rmsprop(var, m, v, g0, learning_rate, beta1, beta2, epsilon, weight_decay, grad_scale=1.0, update_slots=True,
            use_v2=False, watch=None):
  """-> (var, m, v) after one step; without update_slots nothing changes."""
  if not update_slots:
    return var, m, v
  w = watch or _noop
  lr, b1, b2, eps = F(learning_rate), F(beta1), F(beta2), F(epsilon)
  with np.errstate(all="ignore"):
    g = grad_after_decay(var, g0, grad_scale, weight_decay, w)
    gl = w(g * lr)
    if use_v2:
      v = w(w(b2 * v) + w(g * g))
      step = w(gl / w(w(np.sqrt(v)) + eps))
    else:
      v = w(v + w(w(w(g * g) - v) * w(F(1.0) - b2)))
      step = w(gl * w(F(1.0) / w(np.sqrt(w(v + eps)))))
    m = w(w(b1 * m) + step)
    return w(var - m), m, v


class Model:
  """A list of variables with zero slots, stepped by the truth.  ``kind``: one of KINDS."""

  def __init__(self, kind, variables, hyper=None, watch=None):
    self.kind = kind
    self.hyper = dict(HYPER[kind] if hyper is None else hyper)
    self.vars = [np.array(v, F, copy=True) for v in variables]
    self.slots = {s: [np.zeros(v.shape, F) for v in self.vars] for s in SLOTS[kind]}
    self.watch = watch

  def step(self, grads, grad_scale=1.0, update_slots=True, learning_rate=None):
    """``grads``: one float32 / float16 array or None per variable."""
    h = dict(self.hyper)
    if learning_rate is not None:
      h["learning_rate"] = learning_rate
    v2 = self.kind.endswith("_v2")
    for i, g in enumerate(grads):
      if g is None or self.vars[i].size == 0:
        continue
      g = np.asarray(g).reshape(self.vars[i].shape)
      s = self.slots
      if self.kind.startswith("adamom"):
        self.vars[i], s["m"][i], s["v"][i], s["c"][i] = adamom(
            self.vars[i], s["m"][i], s["v"][i], s["c"][i], g, grad_scale=grad_scale, update_slots=update_slots,
            use_v2=v2, watch=self.watch, **h)
      else:
        self.vars[i], s["m"][i], s["v"][i] = rmsprop(
            self.vars[i], s["m"][i], s["v"][i], g, grad_scale=grad_scale, update_slots=update_slots, use_v2=v2,
            watch=self.watch, **h)
    if isinstance(self.watch, Tracker):
      assert not self.watch.seen_subnormal, "a subnormal intermediate: outside the contract, choose other inputs"


def same_bits(got, want):
  """Raw bits equal, NaNs canonicalised: NaN where the truth is NaN (x86 and the device give 0 / 0 different
  signs), the same bits everywhere else."""
  got = np.ascontiguousarray(got, F).ravel()
  want = np.ascontiguousarray(want, F).ravel()
  if got.shape != want.shape:
    return False
  gn, wn = np.isnan(got), np.isnan(want)
  if not np.array_equal(gn, wn):
    return False
  return np.array_equal(got.view(np.uint32)[~wn], want.view(np.uint32)[~wn])


def assert_same_bits(got, want, what=""):
  got = np.ascontiguousarray(got, F).ravel()
  want = np.ascontiguousarray(want, F).ravel()
  assert got.shape == want.shape, (what, got.shape, want.shape)
  gn, wn = np.isnan(got), np.isnan(want)
  bad = (gn != wn) | (~wn & ~gn & (got.view(np.uint32) != want.view(np.uint32)))
  if bad.any():
    i = int(np.flatnonzero(bad)[0])
    raise AssertionError("%s: %d of %d elements differ, first at %d: got %r (0x%08x), want %r (0x%08x)" %
                         (what, int(bad.sum()), bad.size, i, got[i], got.view(np.uint32)[i], want[i],
                          want.view(np.uint32)[i]))


def seeded_grads(shapes, steps, seed, scale=0.3):
  """``steps`` lists of float32 gradients for the shapes."""
  rng = np.random.default_rng(seed)
  return [[(rng.standard_normal(s) * F(scale)).astype(F) for s in shapes] for _ in range(steps)]


# ---- the reference's goldens: (kind, hyper, var0, gradient, {name: expected}) -------------------------
GOLDENS = [
    ("adamom", dict(learning_rate=0.1, weight_decay=0.01, ada_decay=0.99, mom_decay=0.9, epsilon=1e-6), 0.1, 0.12,
     {"var": 0.090000336, "m": 0.0121, "v": 0.014641, "c": 1.0}),                       # adamom_test.py:24-51
    ("rmsprop", dict(learning_rate=0.1, weight_decay=1.0, beta1=0.9, beta2=0.9, epsilon=0.1), 0.1, 0.12,
     {"var": 0.03205473846225154, "m": 0.06794526153774846, "v": 0.00484}),             # rmsprop_test.py:25-60
    ("rmsprop_v2", dict(learning_rate=0.1, weight_decay=1.0, beta1=0.9, beta2=0.9, epsilon=0.1), 0.1, 0.12,
     {"var": 0.031250, "m": 0.068750, "v": 0.0484}),                                    # rmspropv2_test.py:22-58
]
GOLDEN_EPS = 1e-8
