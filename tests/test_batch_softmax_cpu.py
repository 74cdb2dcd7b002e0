"""CPU suite of the batch softmax loss (csrc/mhte_bsm_core.h, mhte_bsm_host.h, monolith_amd/losses.py): the numpy
truth (tests/batch_softmax_truth.py) is pinned on closed forms and on central differences; the reference's own
fp32 order of operations agrees with it where it is finite and is NaN where it overflows; the core header, compiled
for the host, plans a sweep that visits every (row, column) pair exactly once, lays the workspace out without
overlap, merges (m, l) partials like a two-pass evaluation and takes the normalisation backward like the truth; the
same driver runs once more under the address and undefined-behaviour sanitizers, as a program; every argument the
entry points can refuse on the host is refused there; a valid call without a device is refused loudly; the symbols
are on the surface and the ABI version stands; the Python functions check their arguments."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import batch_softmax_truth as BT  # noqa: E402
import monolith_amd  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import losses  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
FAKE = 0x10000   # a "device pointer" the host never follows
F = np.float32


# ---- the truth is pinned ------------------------------------------------------------------------------------
def test_truth_a_batch_of_one_has_no_loss():
  for seed, normalize, T in ((0, True, 1.0), (1, False, 0.3), (2, True, 0.01)):
    q, it, iv, r = BT.inputs(seed, 1, 7, scale=3.0)
    t = BT.Truth(q, it, iv, r, normalize, T)
    assert t.loss == 0.0 and not t.G.any()


def test_truth_equal_items_and_intervals_give_sum_r_log_b():
  B = 6
  q = BT.inputs(3, B, 5)[0]
  it = np.tile(np.array([[0.3, -1.0, 2.0, 0.5, 0.25]], dtype=F), (B, 1))
  r = np.array([1, 0.5, 2, 0.25, 0.7, 0.257], dtype=F)
  want = float(r.astype(np.float64).sum() * np.log(B))
  for normalize, T, interval in ((True, 1.0, 40.0), (False, 0.05, 1.0)):
    t = BT.Truth(q, it, np.full(B, interval, dtype=F), r, normalize, T)
    assert abs(t.loss - want) < 1e-12 * want
  assert abs(want - 4.707 * 1.791759469228055) < 1e-6   # sum r = 4.707 (as fp32 values), log 6


@pytest.mark.parametrize("normalize,T", [(True, 1.0), (True, 0.05), (False, 0.7)])
def test_truth_gradients_against_central_differences(normalize, T):
  q, it, iv, r = BT.inputs(4, 7, 5)
  t = BT.Truth(q, it, iv, r, normalize, T)
  dq, di = BT.central_differences(q, it, iv, r, normalize, t.T)
  for got, want in ((t.dquery, dq), (t.ditem, di)):
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max()


def test_truth_epsilon_branch_and_clamped_intervals():
  q, it, iv, r = BT.inputs(5, 4, 3)
  q[1] = 0
  it[2] = 0
  t = BT.Truth(q, it, iv, r, True, 1.0)
  assert t.inv_q[1] == 1e6 and t.inv_i[2] == 1e6
  np.testing.assert_allclose(t.dquery[1], t.g_q[1] * 1e6, rtol=1e-15)
  np.testing.assert_allclose(t.ditem[2], t.g_i[2] * 1e6, rtol=1e-15)
  a = BT.Truth(q, it, np.array([0, 0.5, -3, 1], dtype=F), r)
  b = BT.Truth(q, it, np.ones(4, dtype=F), r)
  assert a.loss == b.loss and np.array_equal(a.dquery, b.dquery)


def test_reference_fp32_agrees_where_finite_and_overflows_at_low_temperature():
  q, it, iv, r = BT.inputs(6, 64, 16)
  it[0] = 3 * q[0]   # one aligned pair, as a trained model has them: q^ . i^ = 1, exp(1 / 0.01) overflows
  t = BT.Truth(q, it, iv, r, True, 1.0)
  ref = BT.reference_fp32(q, it, iv, r, True, 1.0)
  # the reference's fp32 evaluation: the matmul and the sums in numpy's own order, a sum of B terms per row and
  # of B rows; within the bound of the device's order plus B u per sum
  bound = t.bounds()[0] + 2 * 64 * BT.U * np.abs(t.r * (t.zd - t.lse)).sum()
  assert np.isfinite(ref) and abs(float(ref) - t.loss) <= bound
  cold = BT.Truth(q, it, iv, r, True, 0.01)
  assert np.isnan(BT.reference_fp32(q, it, iv, r, True, 0.01)) and np.isfinite(cold.loss)
  assert all(np.isfinite(b).all() for b in cold.bounds())


# ---- the core header on the host ----------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
  exe = str(tmp_path_factory.mktemp(name) / "bsm_host")
  subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-DMHTE_HOST_ONLY", "-ffp-contract=off"] + extra +
                        ["-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         os.path.join(ROOT, "tests", "bsm_host_driver.cc"), "-o", exe])
  return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  return _build(tmp_path_factory, "bsm", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
  return _build(tmp_path_factory, "bsm_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, *args):
  return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout


PLAN_SHAPES = [(0, 5), (1, 1), (2, 3), (31, 8), (32, 9), (33, 16), (127, 64), (128, 64), (129, 65), (1000, 100),
               (2100, 64), (4096, 64), (4096, 256), (16384, 64), (65536, 64), (2 ** 24 - 1, 256)]
COVER_SHAPES = [(1, 1), (2, 3), (31, 8), (32, 8), (33, 16), (63, 100), (64, 100), (65, 100), (127, 64), (128, 64),
                (129, 64), (257, 33), (1000, 256), (2100, 64)]


def _check_plan(exe):
  for B, k in PLAN_SHAPES:
    lines = _run(exe, "plan", B, k).splitlines()
    got = [int(x) for x in lines[0].split()]
    want = BT.plan(B, k)
    assert got == [want[n] for n in ("kp", "nb", "row_block", "column_tile", "bp", "blocks", "tiles",
                                     "tiles_per_chunk", "chunks", "workspace_bytes")], (B, k)
    assert want["chunks"] >= 1 and want["chunks"] <= BT.MAX_CHUNKS
    assert (want["chunks"] - 1) * want["tiles_per_chunk"] < max(want["tiles"], 1) <= \
        want["chunks"] * want["tiles_per_chunk"]                      # no empty chunk, every tile in one
    assert want["tiles"] * BT.TILE <= want["bp"]                       # the streamed tiles end inside the padding
    spans = [tuple(int(x) for x in line.split()) for line in lines[1:]]
    assert len(spans) == 13
    end = 0
    for off, nbytes in spans:   # in order, 256-byte aligned, none overlapping
      assert off % 256 == 0 and off >= end, (B, k, spans)
      end = off + nbytes
    assert end <= want["workspace_bytes"]
    out = (C.c_int64 * 5)()
    assert _lib.lib().mhte_batch_softmax_plan(B, k, out, 5) == _lib.MHTE_OK
    assert list(out) == [want[n] for n in BT.PLAN_NAMES], (B, k)
    assert losses.batch_softmax_plan(B, k) == {n: want[n] for n in BT.PLAN_NAMES}


def _check_cover(exe, shapes):
  for B, k in shapes:
    visited, most, outside = (int(x) for x in _run(exe, "cover", B, k).split())
    assert (visited, most, outside) == (B * B, 1, 0), (B, k)


def _check_merge(exe, tmp_path):
  rng = np.random.default_rng(8)
  cases = [rng.standard_normal(1000) * 30, rng.standard_normal(37) * 0.1 + 95,
           np.concatenate([np.full(40, -np.inf), rng.standard_normal(50), np.full(16, -np.inf)]),
           np.sort(rng.standard_normal(300) * 50), -np.sort(rng.standard_normal(300) * 50)]
  for n, z in enumerate(cases):
    z = z.astype(F)
    path = str(tmp_path / ("z%d.bin" % n))
    z.tofile(path)
    z64 = z.astype(np.float64)
    m = z64.max()
    two_pass = m + np.log(np.exp(z64 - m).sum())
    for G in (16, 32, 1000):
      gm, gl, glse = (float(x) for x in _run(exe, "merge", path, G).split())
      assert F(gm) == F(m)
      steps = len(z) // G + 2
      # each term: its argument's rounding weighted by its share (at most |z - m| u, summed below as the mean
      # over the shares), `steps` rescalings of (2 ulp exp + multiply + add), G additions; logf 2 ulp, one addition
      share = np.exp(z64 - two_pass)
      bound = BT.U * (np.where(share > 0, share * np.abs(np.maximum(z64, -1e30) - m), 0).sum() + steps * 6 + min(G, len(z)) +
                      4 * abs(np.log(gl)) + abs(two_pass))
      assert abs(glse - two_pass) <= bound, (n, G, glse, two_pass, bound)
  path = str(tmp_path / "none.bin")
  np.full(5, -np.inf, dtype=F).tofile(path)
  assert _run(exe, "merge", path, 2).split()[:2] == ["-inf", "0"]


def _check_back(exe, tmp_path):
  rng = np.random.default_rng(9)
  for n, (k, normalize, scale) in enumerate(((5, 1, 1.0), (64, 1, 30.0), (256, 1, 1e-3), (3, 1, 1e-8), (7, 0, 2.0))):
    g = rng.standard_normal(k).astype(F)
    x = (rng.standard_normal(k) * scale).astype(F)
    path = str(tmp_path / ("b%d.bin" % n))
    np.concatenate([g, x]).tofile(path)
    lines = _run(exe, "back", path, k, normalize).splitlines()
    got = np.array([float(v) for v in lines[:k]])
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    s = (x64 * x64).sum()
    inv = 1 / np.sqrt(max(s, BT.NORM_EPS)) if normalize else 1.0
    xh = x64 * inv
    dot = (xh * g64).sum()
    want = g64 if not normalize else ((g64 - xh * dot) * inv if s >= BT.NORM_EPS else g64 * inv)
    if scale == 1e-8:
      assert s < BT.NORM_EPS and inv == 1e6   # the epsilon branch
    # the chain of k terms in s and in the dot, the recomputed x^, the last operations
    u = BT.U
    bound = inv * ((k + 10) * u * np.abs(xh) * np.abs(xh * g64).sum() + (k / 2 + 10) * u * np.abs(xh * dot) +
                   u * np.abs(g64 - xh * dot)) + (k / 2 + 8) * u * np.abs(want)
    assert (np.abs(got - want) <= bound).all(), (k, normalize, scale)
    inv_got, c_got = (float(v) for v in lines[k].split())
    assert abs(inv_got - inv) <= (k / 2 + 3) * u * inv
    assert abs(c_got - np.log(max(float(x[0]), 1.0))) <= 4 * u * abs(np.log(max(float(x[0]), 1.0)))


def test_constants_on_the_host(driver):
  consts = dict((k, int(v)) for k, v in (line.split() for line in _run(driver, "consts").splitlines()))
  assert consts == dict(max_dim=BT.MAX_DIM, k_pad=BT.K_PAD, tile=BT.TILE, max_chunks=BT.MAX_CHUNKS,
                        target_groups=BT.TARGET_GROUPS, final_threads=1024, counters=len(BT.COUNTERS))
  assert losses.BSM_COUNTER_NAMES == BT.COUNTERS and losses.BSM_PLAN_NAMES == BT.PLAN_NAMES


def test_plan_equals_its_restatement_and_the_entry_point(driver):
  _check_plan(driver)
  # the flagship shapes: the grid is of the order of the CU count, the workspace at 65536 x 64 is below 1 GB
  assert BT.plan(4096, 64)["blocks"] * BT.plan(4096, 64)["chunks"] == 512
  assert 256 <= BT.plan(16384, 64)["blocks"] * BT.plan(16384, 64)["chunks"] <= 1024
  assert BT.plan(65536, 64)["workspace_bytes"] < 1 << 30


def test_plan_covers_every_pair_exactly_once(driver):
  _check_cover(driver, COVER_SHAPES)


def test_online_merge_against_a_two_pass_evaluation(driver, tmp_path):
  _check_merge(driver, tmp_path)


def test_normalisation_backward_against_the_truth(driver, tmp_path):
  _check_back(driver, tmp_path)


def test_the_driver_under_the_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
  """The same program, built with -fsanitize=address,undefined and run as a program: a finding aborts it."""
  _check_plan(sanitized)
  _check_cover(sanitized, COVER_SHAPES[:9])
  _check_merge(sanitized, tmp_path)
  _check_back(sanitized, tmp_path)


# ---- the refusals, before any device call ---------------------------------------------------------------------
def _fwd(query=FAKE, item=2 * FAKE, interval=3 * FAKE, r=4 * FAKE, batch=8, dim=4, normalize=1, temperature=1.0,
         loss=5 * FAKE, unit_dquery=None, unit_ditem=None):
  L = _lib.lib()
  st = L.mhte_batch_softmax_loss(query, item, interval, r, batch, dim, normalize, temperature, loss, unit_dquery,
                                 unit_ditem, None)
  return st, L.mhte_last_error().decode()


def _grad(query=FAKE, item=2 * FAKE, interval=3 * FAKE, r=4 * FAKE, batch=8, dim=4, normalize=1, temperature=1.0,
          grad=1.0, grad_dev=None, dquery=6 * FAKE, ditem=7 * FAKE):
  L = _lib.lib()
  st = L.mhte_batch_softmax_loss_grad(query, item, interval, r, batch, dim, normalize, temperature, grad, grad_dev,
                                      dquery, ditem, None)
  return st, L.mhte_last_error().decode()


def _invalid(fn, name, needle, **kw):
  st, msg = fn(**kw)
  assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
  assert msg.startswith(name + ": "), msg
  assert needle in msg, msg


@pytest.mark.parametrize("fn,name", [(_fwd, "batch_softmax_loss"), (_grad, "batch_softmax_loss_grad")],
                         ids=["forward", "gradient"])
def test_entry_points_refuse_invalid_arguments_on_the_host(fn, name):
  bad = lambda needle, **kw: _invalid(fn, name, needle, **kw)  # noqa: E731
  for arg in ("query", "item", "interval", "r"):
    shown = "item_step_interval" if arg == "interval" else arg
    bad("null argument: " + shown, **{arg: None})
    bad(shown + " must be 4-byte aligned", **{arg: 9 * FAKE + 2})
  bad("batch must be >= 0, got -1", batch=-1)
  bad("batch must be below 2^24, got 16777216", batch=2 ** 24)
  bad("batch must be below 2^24", batch=2 ** 40)
  for d in (0, -1, 257, 2 ** 20):
    bad("dim must be in [1, 256], got %d" % d, dim=d)
  for t in (0.0, -0.5, float("nan"), float("-inf")):
    bad("temperature must be > 0, got", temperature=t)
  for n in (2, -1, 256):
    bad("normalize must be 0 or 1, got %d" % n, normalize=n)
  if fn is _fwd:
    bad("null argument: loss", loss=None)
    bad("null argument: loss", loss=None, batch=0, query=None, item=None, interval=None, r=None)
    bad("loss must be 4-byte aligned", loss=5 * FAKE + 2)
    bad("unit_dquery must be 4-byte aligned", unit_dquery=6 * FAKE + 1)
    bad("unit_ditem must be 4-byte aligned", unit_ditem=7 * FAKE + 3)
  else:
    bad("null argument: dquery and ditem", dquery=None, ditem=None)
    bad("dquery must be 4-byte aligned", dquery=6 * FAKE + 3)
    bad("ditem must be 4-byte aligned", ditem=7 * FAKE + 1)
    bad("grad_dev must be 4-byte aligned", grad_dev=8 * FAKE + 2)


def test_plan_and_launch_counts_refusals():
  L = _lib.lib()
  out = (C.c_int64 * 6)()
  for args, needle in (((8, 4, None, 5), "batch_softmax_plan: null argument: out"),
                       ((8, 4, out, 4), "batch_softmax_plan: n must be 5, got 4"),
                       ((-1, 4, out, 5), "batch_softmax_plan: batch must be >= 0"),
                       ((2 ** 24, 4, out, 5), "batch_softmax_plan: batch must be below 2^24"),
                       ((8, 0, out, 5), "batch_softmax_plan: dim must be in [1, 256]"),
                       ((8, 257, out, 5), "batch_softmax_plan: dim must be in [1, 256]")):
    assert L.mhte_batch_softmax_plan(*args) == _lib.MHTE_INVALID_ARGUMENT
    assert needle in L.mhte_last_error().decode()
  assert L.mhte_batch_softmax_launch_counts(None, 6) == _lib.MHTE_INVALID_ARGUMENT
  assert "batch_softmax_launch_counts: null argument: out" in L.mhte_last_error().decode()
  assert L.mhte_batch_softmax_launch_counts(out, 5) == _lib.MHTE_INVALID_ARGUMENT
  assert "n must be 6, got 5" in L.mhte_last_error().decode()
  assert L.mhte_batch_softmax_launch_counts(out, 6) == _lib.MHTE_OK   # needs no device
  assert tuple(losses.batch_softmax_launch_counts()) == BT.COUNTERS
  assert monolith_amd.batch_softmax_launch_counts is losses.batch_softmax_launch_counts


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_a_valid_call_without_a_device_is_unavailable():
  for kw in ({}, {"batch": 0, "query": None, "item": None, "interval": None, "r": None}, {"batch": 2 ** 24 - 1},
             {"dim": 256}, {"normalize": 0, "temperature": 0.01}, {"query": FAKE + 4, "item": 2 * FAKE + 12}):
    for fn in (_fwd, _grad):
      st, msg = fn(**kw)
      assert st == _lib.MHTE_UNAVAILABLE, (fn.__name__, kw, st, msg)
      assert "no CPU fallback" in msg
  st, msg = _fwd(unit_dquery=6 * FAKE, unit_ditem=7 * FAKE)
  assert st == _lib.MHTE_UNAVAILABLE, msg
  for kw in ({"dquery": None}, {"ditem": None}, {"grad_dev": 8 * FAKE}):
    st, msg = _grad(**kw)
    assert st == _lib.MHTE_UNAVAILABLE, msg
  assert not any(losses.batch_softmax_launch_counts().values())


# ---- the surface ----------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in ("mhte_batch_softmax_loss", "mhte_batch_softmax_loss_grad", "mhte_batch_softmax_plan",
            "mhte_batch_softmax_launch_counts"):
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  for word in ("batch_softmax_loss.py:18-57", "one defined deviation"):
    assert word in text, word
  p, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
  sig = _lib.signatures()
  assert sig["mhte_batch_softmax_loss"] == (i32, [p, p, p, p, i64, i32, i32, f32, p, p, p, p])
  assert sig["mhte_batch_softmax_loss_grad"] == (i32, [p, p, p, p, i64, i32, i32, f32, f32, p, p, p, p])
  assert sig["mhte_batch_softmax_plan"] == (i32, [i64, i32, p, i32])
  assert sig["mhte_batch_softmax_launch_counts"] == (i32, [p, i32])
  for name in ("losses", "batch_softmax_loss", "batch_softmax_loss_grad", "batch_softmax_plan",
               "batch_softmax_launch_counts"):
    assert name in monolith_amd.__all__ and getattr(monolith_amd, name) is not None


# ---- the Python mirror ----------------------------------------------------------------------------------------
def test_python_argument_contract():
  q, it, iv, r = torch.zeros(8, 4), torch.zeros(8, 4), torch.ones(8), torch.ones(8)
  fns = ((losses.batch_softmax_loss, "batch_softmax_loss"),
         (lambda a, b, c, d, n=True, t=1.0: losses.batch_softmax_loss_grad(a, b, c, d, 1.0, n, t),
          "batch_softmax_loss_grad"))
  for fn, name in fns:
    for t in (0.0, -1.0, float("nan")):
      with pytest.raises(ValueError, match="temperature should be positive, while got"):
        fn(q, it, iv, r, True, t)
    with pytest.raises(ValueError, match="%s: query and item must be \\[B, k\\] of one shape" % name):
      fn(q, torch.zeros(8, 5), iv, r)
    with pytest.raises(ValueError, match="query and item must be"):
      fn(torch.zeros(32), torch.zeros(32), iv, r)
    with pytest.raises(ValueError, match="item_step_interval must hold B = 8 elements, got 7"):
      fn(q, it, torch.ones(7), r)
    with pytest.raises(ValueError, match="r must hold B = 8 elements, got 9"):
      fn(q, it, iv, torch.ones(9))
    with pytest.raises(ValueError, match=r"k must be in \[1, 256\], got 257"):
      fn(torch.zeros(2, 257), torch.zeros(2, 257), torch.ones(2), torch.ones(2))
    with pytest.raises(TypeError, match="query must be float32"):
      fn(q.double(), it, iv, r)
    with pytest.raises(TypeError, match="item_step_interval must be float32"):
      fn(q, it, iv.long(), r)
    with pytest.raises(TypeError, match="item must be a torch tensor"):
      fn(q, it.numpy(), iv, r)
    with pytest.raises(ValueError, match="item must be contiguous"):
      fn(q, torch.zeros(4, 8).t(), iv, r)
    with pytest.raises(ValueError, match="r must be contiguous"):
      fn(q, it, iv, torch.ones(16)[::2])
    with pytest.raises(TypeError, match="normalize must be a bool"):
      fn(q, it, iv, r, 2)
    with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
      fn(q, it, iv, r)
  with pytest.raises(TypeError, match="grad must be a float or a 0-d float32 tensor on the GPU"):
    losses.batch_softmax_loss_grad(q, it, iv, r, torch.ones(()))
  with pytest.raises(ValueError, match="at least one of want_query and want_item"):
    losses.batch_softmax_loss_grad(q, it, iv, r, 1.0, want_query=False, want_item=False)
