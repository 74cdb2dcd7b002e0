"""GPU suite of clip by global norm (monolith_amd/clip_ops.py, csrc/mhte_clip_kernels.h): the norm's bits
against the numpy restatement of the fixed tree (tests/clip_ops_truth.py), the clip's bits in every form
(fused, host norm, device norm, device scale; out of place and in place), the reference's cases, the whole
path captured into a graph with no host value in it, and the gather gradient with the scale on the device."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ops_truth as T  # noqa: E402
from monolith_amd import _lib, clip_ops  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SNAN = 0x7fa00001   # a signalling NaN with a payload: x * 1 would set its quiet bit


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unaligned(a):
  """The same values in a view that starts one float into its storage: a pointer that is not 16-byte aligned."""
  buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
  v = buf[1:]
  v.copy_(torch.from_numpy(a))
  assert v.data_ptr() % 16 == 4
  return v


def result_block(tensors, clip_norm=float("inf")):
  """mhte_global_l2_reduce on a list of device tensors (any number, also none) -> the 4 result floats."""
  n = len(tensors)
  ptrs = (C.c_void_p * max(n, 1))(*[C.c_void_p(t.data_ptr()) for t in tensors])
  lens = (C.c_int64 * max(n, 1))(*[t.numel() for t in tensors])
  res = torch.full((4,), -7.0, dtype=torch.float32, device=DEV)
  _lib.check(_lib.lib().mhte_global_l2_reduce(ptrs, lens, n, clip_norm, _lib.vp(res),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
  return res.cpu().numpy()


@functools.lru_cache(maxsize=None)
def host_set(name):
  if name == "unaligned":
    return host_set("edges")
  if name == "none":
    return []
  return getattr(T, "set_" + name)()


@functools.lru_cache(maxsize=None)
def truth_sumsq(name):
  return T.tree_sumsq(host_set(name))[0]


# ---- 1. the bits of the norm --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "unaligned", "two_rounds", "many", "dense", "none"])
def test_norm_bits(name):
  hs = host_set(name)
  ts = [dev(a) for a in hs]
  if name == "unaligned":
    ts[-2] = unaligned(hs[-2])
  exp = truth_sumsq(name)
  runs = [result_block(ts) for _ in range(3)]
  got = runs[0]
  print("%s: sum %r truth %r" % (name, got[0], exp))
  assert T.bits(got[0]) == T.bits(exp)
  assert T.bits(got[1]) == T.bits(np.sqrt(exp, dtype=np.float32))
  assert T.bits(got[2]) == T.bits(np.float32(1)) and T.bits(got[3]) == 0   # clip_norm = +inf: the norm alone
  for r in runs[1:]:
    np.testing.assert_array_equal(T.bits(r), T.bits(got))
  if name != "none":
    n = clip_ops._global_norm(ts)
    assert n.dim() == 0 and n.is_cuda
    assert T.bits(n.cpu().numpy()) == T.bits(got[1])
  else:   # n = 0: sum 0, norm 0, scale 1
    np.testing.assert_array_equal(got, np.array([0, 0, 1, 0], np.float32))


def test_norm_order_of_the_list_matters_and_is_kept():
  hs = host_set("edges")
  rev = hs[::-1]
  got = result_block([dev(a) for a in rev])
  assert T.bits(got[0]) == T.bits(T.tree_sumsq(rev)[0])


# ---- 2. the clip's bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["below", "equal", "above"])
def test_clip_bits_in_every_form(where):
  hs = host_set("edges")
  norm = np.sqrt(truth_sumsq("edges"), dtype=np.float32)
  clip_norm = {"below": float(norm) * 0.37, "equal": float(norm), "above": float(norm) * 2.0}[where]
  _, norm_t, scale_t = T.norm_and_scale(hs, clip_norm)
  assert (scale_t != np.float32(1)) == (where == "below")
  ts = [dev(a) for a in hs]
  outs, gn = clip_ops.clip_by_global_norm(ts, clip_norm)
  assert T.bits(gn.cpu().numpy()) == T.bits(norm_t)
  exp, _ = T.clip(hs, clip_norm)
  for o, e, t, h in zip(outs, exp, ts, hs):
    assert o.data_ptr() != t.data_ptr() or o.numel() == 0
    np.testing.assert_array_equal(T.bits(o.cpu().numpy()), T.bits(e))
    if where != "below":
      np.testing.assert_array_equal(T.bits(o.cpu().numpy()), T.bits(h))   # not clipped: the inputs
    np.testing.assert_array_equal(T.bits(t.cpu().numpy()), T.bits(h))     # out of place: inputs unchanged
  # the other forms, given the fused form's norm and scale
  n_dev, s_dev = clip_ops.global_norm_and_scale(ts, clip_norm)
  assert n_dev.dim() == 0 and s_dev.dim() == 0
  assert n_dev.untyped_storage().data_ptr() == s_dev.untyped_storage().data_ptr()
  assert T.bits(n_dev.cpu().numpy()) == T.bits(norm_t) and T.bits(s_dev.cpu().numpy()) == T.bits(scale_t)
  forms = {"host norm": clip_ops.clip_by_global_norm(ts, clip_norm, use_norm=float(norm_t))[0],
           "device norm": clip_ops.clip_by_global_norm(ts, clip_norm, use_norm=gn)[0],
           "device scale": clip_ops.scale_tensors(ts, s_dev)}
  for form, got in forms.items():
    for o, f in zip(outs, got):
      np.testing.assert_array_equal(T.bits(f.cpu().numpy()), T.bits(o.cpu().numpy()), err_msg=form)
  for t, h in zip(ts, hs):
    np.testing.assert_array_equal(T.bits(t.cpu().numpy()), T.bits(h))


def test_clip_beyond_the_inline_table_and_unaligned():
  """150 tensors (the table is uploaded) and an unaligned tensor through the 4-byte form of the multiply."""
  hs = host_set("many")
  clip_norm = 3.0
  exp, norm_t = T.clip(hs, clip_norm)
  outs, gn = clip_ops.clip_by_global_norm([dev(a) for a in hs], clip_norm)
  assert T.bits(gn.cpu().numpy()) == T.bits(norm_t)
  for o, e in zip(outs, exp):
    np.testing.assert_array_equal(T.bits(o.cpu().numpy()), T.bits(e))
  he = host_set("edges")
  ts = [dev(a) for a in he]
  ts[-2] = unaligned(he[-2])
  exp, _ = T.clip(he, 1.0)
  outs, _ = clip_ops.clip_by_global_norm(ts, 1.0, inplace=True)
  for o, e in zip(outs, exp):
    np.testing.assert_array_equal(T.bits(o.cpu().numpy()), T.bits(e))


@pytest.mark.parametrize("count", [128, 129])
def test_clip_on_both_sides_of_the_inline_table_s_edge(count):
  """128 tensors are the last list that rides in the kernel arguments, 129 the first that is uploaded: the fused
  entry (norm and multiply) and the multiply alone with a host norm, 3000 elements each (one ragged chunk)."""
  rng = np.random.default_rng(1000 + count)
  hs = [rng.standard_normal(3000).astype(np.float32) for _ in range(count)]
  clip_norm = 3.0
  exp, norm_t = T.clip(hs, clip_norm)
  assert np.isfinite(norm_t) and norm_t > clip_norm and all(np.isfinite(e).all() for e in exp)
  ts = [dev(a) for a in hs]
  outs, gn = clip_ops.clip_by_global_norm(ts, clip_norm)
  assert T.bits(gn.cpu().numpy()) == T.bits(norm_t)
  alone = clip_ops.clip_by_global_norm(ts, clip_norm, use_norm=float(norm_t))[0]
  assert len(outs) == len(alone) == count
  for o, a, e, t, h in zip(outs, alone, exp, ts, hs):
    np.testing.assert_array_equal(T.bits(o.cpu().numpy()), T.bits(e))
    np.testing.assert_array_equal(T.bits(a.cpu().numpy()), T.bits(e))
    np.testing.assert_array_equal(T.bits(t.cpu().numpy()), T.bits(h))   # out of place: the inputs are left alone


# ---- 3. in place --------------------------------------------------------------------------------------
def test_in_place_same_bits_and_untouched_without_clipping():
  hs = host_set("edges")
  clip_norm = 1.0
  exp, _ = T.clip(hs, clip_norm)
  ts = [dev(a) for a in hs]
  ptrs = [t.data_ptr() for t in ts]
  outs, _ = clip_ops.clip_by_global_norm(ts, clip_norm, inplace=True)
  assert [o.data_ptr() for o in outs] == ptrs
  for o, e in zip(outs, exp):
    np.testing.assert_array_equal(T.bits(o.cpu().numpy()), T.bits(e))
  # no clipping: signalling NaNs written through an int32 view survive every in-place form (their norm is
  # NaN, which leaves the scale at 1; a stray x * 1 would quiet them)
  pat = [np.full(a.size, SNAN, np.int32) + np.arange(a.size, dtype=np.int32) % 1000 for a in hs]
  ts = [dev(p).view(torch.float32) for p in pat]

  def untouched(what):
    for t, p in zip(ts, pat):
      np.testing.assert_array_equal(t.view(torch.int32).cpu().numpy(), p, err_msg=what)

  _, gn = clip_ops.clip_by_global_norm(ts, clip_norm, inplace=True)
  assert np.isnan(gn.cpu().numpy())
  untouched("fused")
  clip_ops.clip_by_global_norm(ts, clip_norm, use_norm=0.5, inplace=True)
  untouched("host norm")
  clip_ops.clip_by_global_norm(ts, clip_norm, use_norm=dev(np.array(0.5, np.float32)), inplace=True)
  untouched("device norm")
  clip_ops.scale_tensors(ts, dev(np.array(1.0, np.float32)), inplace=True)
  untouched("device scale")
  # ... and out of place without clipping is a copy of the bits
  outs, _ = clip_ops.clip_by_global_norm(ts, clip_norm, use_norm=0.5)
  for o, p in zip(outs, pat):
    np.testing.assert_array_equal(o.view(torch.int32).cpu().numpy(), p)


# ---- 4. the reference's cases -------------------------------------------------------------------------
def test_reference_cases_on_the_device():
  for c in T.load_kat()["clip"]:
    ts = [dev(a) for a in c["inputs"]]
    outs, gn = clip_ops.clip_by_global_norm(ts, c["clip_norm"])
    for o, e, t, a in zip(outs, c["expected"], ts, c["inputs"]):
      got = o.cpu().numpy()
      if c["name"] == "exploded grad":
        assert np.isnan(got).all(), c["name"]
      else:
        np.testing.assert_array_equal(T.bits(got), T.bits(e), err_msg=c["name"])   # zero norm: zeros, not NaN
      np.testing.assert_array_equal(T.bits(t.cpu().numpy()), T.bits(a))
  for c in T.load_kat()["norm"]:
    assert float(clip_ops._global_norm([dev(a) for a in c["inputs"]]).cpu()) == c["expected"]


# ---- helpers of sections 5 and 6: a gather-gradient case and its sequential truth --------------------------
def gather_case(dims, n_rows, slots, seed):
  rng = np.random.default_rng(seed)
  base, offs, grads = 0, [], []
  for d, n, k in zip(dims, n_rows, slots):
    offs.append((base + rng.integers(0, k, n) * d).astype(np.int32))
    grads.append(rng.standard_normal((n, d)).astype(np.float32))
    base += k * d
  return base, offs, grads


def gather_sequential(base, offs, grads, dims, sc):
  """The loop of test_fused_gather_gradient_is_sequential_and_repeatable: addends scaled, added in row order."""
  exp = np.zeros(base, np.float32)
  sc = np.float32(sc)
  for o, g, d in zip(offs, grads, dims):
    acc = {}
    for j in range(o.size):
      a = acc.get(int(o[j]))
      t = g[j] * sc
      acc[int(o[j])] = t if a is None else a + t
    for off, v in acc.items():
      exp[off:off + d] = np.float32(0) + v
  return exp


# ---- 5. no host value in the path ---------------------------------------------------------------------
def test_norm_scale_and_gather_gradient_replay_in_one_graph():
  """global_norm_and_scale + scale_tensors(inplace) + the gather gradient with the scale tensor, captured on
  one stream and replayed with other contents: one replay clipped, one not, each bit-equal to eager."""
  dims, n_rows, slots = [8, 4], [500, 300], [40, 30]
  base, offs_h, grads_h = gather_case(dims, n_rows, slots, 33)
  rng = np.random.default_rng(34)
  layout_h = [rng.standard_normal(n).astype(np.float32) for n in (5000, 4097, 3)]
  contents = {"clipped": (layout_h, grads_h),
              "not clipped": ([a * np.float32(1e-3) for a in layout_h], [g * np.float32(1e-3) for g in grads_h])}
  clip_norm = 1.0
  for k, (lt, gr) in contents.items():
    assert (T.norm_and_scale(list(lt) + list(gr), clip_norm)[2] != np.float32(1)) == (k == "clipped")
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    offs = [dev(o) for o in offs_h]
    layout = [torch.empty(a.size, dtype=torch.float32, device=DEV) for a in layout_h]
    grads = [torch.empty(g.shape, dtype=torch.float32, device=DEV) for g in grads_h]

    def fill(k):
      for t, a in zip(layout + grads, list(contents[k][0]) + list(contents[k][1])):
        t.copy_(torch.from_numpy(a))

    def run():
      norm, scale = clip_ops.global_norm_and_scale(layout + grads, clip_norm)
      clip_ops.scale_tensors(layout, scale, inplace=True)
      out = D.fused_gather_embeddings_by_input_gradient(base, grads, offs, dims, scale=scale)
      return norm, scale, out

    def snapshot(res):
      s.synchronize()
      return [x.cpu().numpy().copy() for x in list(res) + layout]

    eager = {}
    for k in contents:   # (the first of these is the warm-up call: the workspace exists afterwards)
      fill(k)
      eager[k] = snapshot(run())
      hs = list(contents[k][0]) + list(contents[k][1])
      _, n_t, s_t = T.norm_and_scale(hs, clip_norm)
      assert T.bits(eager[k][0]) == T.bits(n_t) and T.bits(eager[k][1]) == T.bits(s_t)
      np.testing.assert_array_equal(T.bits(eager[k][2]), T.bits(gather_sequential(base, offs_h, contents[k][1], dims, s_t)))
    fill("clipped")
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
      res = run()
    for k in ("clipped", "not clipped"):
      fill(k)
      g.replay()
      got = snapshot(res)
      for a, b in zip(got, eager[k]):
        np.testing.assert_array_equal(T.bits(a), T.bits(b), err_msg=k)
  torch.cuda.synchronize()


# ---- 6. the gather gradient with the scale on the device ----------------------------------------------
@pytest.mark.parametrize("dims,n_rows,slots", [([8, 16, 4], [3000, 2000, 500], [40, 30, 5]),
                                               ([3, 2], [700, 900], [50, 11])])
def test_gather_gradient_with_a_device_scale(dims, n_rows, slots):
  base, offs_h, grads_h = gather_case(dims, n_rows, slots, 21)
  sc = np.float32(0.37)
  offs, grads = [dev(o) for o in offs_h], [dev(g) for g in grads_h]
  host = D.fused_gather_embeddings_by_input_gradient(base, grads, offs, dims, scale=float(sc)).cpu().numpy()
  got = D.fused_gather_embeddings_by_input_gradient(base, grads, offs, dims, scale=dev(np.array(sc))).cpu().numpy()
  np.testing.assert_array_equal(T.bits(got), T.bits(host))
  np.testing.assert_array_equal(T.bits(got), T.bits(gather_sequential(base, offs_h, grads_h, dims, sc)))


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from monolith_amd import distribution_ops as D
rng = np.random.default_rng(9)
dims, n_rows = [8, 3], [600, 500]
base, offs, grads = 0, [], []
for d, n in zip(dims, n_rows):
  offs.append((base + rng.permutation(n) * d).astype(np.int32))   # unique offsets: the atomic form is order-free
  grads.append(rng.standard_normal((n, d)).astype(np.float32))
  base += n * d
sc = np.float32(0.37)
exp = np.zeros(base, np.float32)
for o, g, d in zip(offs, grads, dims):
  for j in range(o.size):
    exp[o[j]:o[j] + d] = np.float32(0) + g[j] * sc
to = [torch.from_numpy(o).cuda() for o in offs]
tg = [torch.from_numpy(g).cuda() for g in grads]
host = D.fused_gather_embeddings_by_input_gradient(base, tg, to, dims, scale=float(sc)).cpu().numpy()
got = D.fused_gather_embeddings_by_input_gradient(base, tg, to, dims,
                                                  scale=torch.tensor(sc, device="cuda")).cpu().numpy()
assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), "device scale differs from the host float"
assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "differs from the loop"
print("ATOMIC-FORM-OK")
"""


def test_gather_gradient_with_a_device_scale_in_the_float_atomic_form():
  """MHTE_POOL_ATOMICS is read once per process: a fresh child with its own time limit.  A child that ends
  with a fault status ends the session — nothing more is started on the GPU behind a fault."""
  env = dict(os.environ, MHTE_POOL_ATOMICS="1", MHTE_NO_REBUILD="1")
  try:
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=240)
  except subprocess.TimeoutExpired:
    pytest.exit("the float-atomic child ran into its time limit: nothing more is started on the GPU", returncode=3)
  if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
    pytest.exit("the float-atomic child ended with status %d: nothing more is started on the GPU\n%s" %
                (r.returncode, r.stderr[-2000:]), returncode=3)
  assert r.returncode == 0 and "ATOMIC-FORM-OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
