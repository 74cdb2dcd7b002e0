"""CPU suite of the in-batch AUC loss (csrc/mhte_auc_core.h, mhte_auc_host.h, monolith_amd/losses.py): the numpy
truth (tests/inbatch_auc_truth.py) is pinned on the reference test's vectors and on the classification and branch
edges; the core header, compiled for the host, classifies as the truth does, keeps both term functions within
their per-term bounds and plans a sweep that visits every pair exactly once; the same driver runs once more under
the address and undefined-behaviour sanitizers, as a program; every argument the entry points can refuse on the
host is refused there, with the entry point's name and the argument; a valid call without a device is refused
loudly; the symbols are on the surface and the ABI version stands; the Python functions check their arguments."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import inbatch_auc_truth as AT  # noqa: E402
import monolith_amd  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import losses  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
FAKE = 0x10000   # a "device pointer" the host never follows
F = np.float32

EDGE_LABELS = np.array([2, 1e-30, 0, -0.0, -9999.5, -10000, -1e9, np.nan], dtype=F)
EDGE_CLASSES = [AT.POSITIVE, AT.POSITIVE, AT.NEGATIVE, AT.NEGATIVE, AT.NEGATIVE, AT.IGNORED, AT.IGNORED, AT.IGNORED]
EDGE_DIFFS = np.array([-87, np.nextafter(F(-87), F(0)), 88, np.nextafter(F(88), F(0)), 200, -200, np.nan, np.inf,
                       -np.inf], dtype=F)


# ---- the truth is pinned ------------------------------------------------------------------------------------
def test_truth_on_the_reference_test_s_vectors():
  """inbatch_auc_loss_test.py: the loss within its delta of 1e-6, the gradient within assertAllClose's defaults."""
  t = AT.Truth([1, 0, 0, 1], [0.5, -0.2, -0.4, 0.8])
  assert (t.P, t.N) == (2, 2)
  assert abs(t.loss - (-1.3208841)) <= 1e-6
  np.testing.assert_allclose(t.gradient(grad=2.0, neg_weight=1.0), [1.2417255, -1.2015073, -1.0410514, 1.0008333],
                             rtol=1e-6, atol=1e-6)
  half = t.gradient(grad=2.0, neg_weight=0.5)
  np.testing.assert_allclose(half[[1, 2]], np.array([-1.2015073, -1.0410514]) / 2, rtol=1e-6, atol=1e-6)


def test_truth_classification_edges():
  assert list(AT.classify(EDGE_LABELS)) == EDGE_CLASSES
  t = AT.Truth(EDGE_LABELS, np.zeros(8, dtype=F))
  assert (t.P, t.N) == (2, 3)
  g = t.gradient()
  assert np.array_equal(g, [1.5, 1.5, -1.0, -1.0, -1.0, 0, 0, 0]) and not np.signbit(g[5:]).any()
  assert abs(t.loss - 6 * -np.log(2.0)) < 1e-12
  for lab in ([1, 1, 2], [0, -1, 0], [np.nan, -10000, -1e9]):   # no positive, no negative, nothing
    t = AT.Truth(lab, [0.1, 0.2, 0.3])
    assert t.loss == 0.0 and not AT.bits(t.gradient(3.0, 0.5)).any()
  with pytest.raises(ValueError, match="the label and logit not match"):
    AT.Truth([1, 0], [0.0])


def test_truth_branch_edges():
  t, s = AT.terms64(EDGE_DIFFS)
  inner_lo, inner_hi = float(EDGE_DIFFS[1]), float(EDGE_DIFFS[3])
  assert t[0] == -87.0 and s[0] == 1.0                               # diff <= -87: the diff itself
  assert abs(t[1] - (inner_lo - np.log1p(np.exp(inner_lo)))) < 1e-12 and abs(s[1] - 1) < 1e-15
  assert t[2] == 0.0 and s[2] == 0.0                                 # diff >= 88: nothing
  assert -1e-38 < t[3] < 0 and 0 < s[3] < 1e-38 and abs(s[3] / np.exp(-inner_hi) - 1) < 1e-12
  assert (t[4], s[4]) == (0.0, 0.0) and (t[5], s[5]) == (-200.0, 1.0)
  assert (t[6], s[6]) == (0.0, 0.0)                                  # NaN: the reference's else branch
  assert (t[7], s[7]) == (0.0, 0.0) and (t[8], s[8]) == (-np.inf, 1.0)
  # the middle branch is the reference's formula where that one still has digits
  d = np.linspace(-30, 30, 241).astype(F)
  t, s = AT.terms64(d)
  d64 = d.astype(np.float64)
  np.testing.assert_allclose(t, d64 - np.log(1.0 + np.exp(d64)), rtol=0, atol=1e-13)
  np.testing.assert_allclose(s, 1.0 - 1.0 / (1.0 + np.exp(-d64)), rtol=0, atol=1e-15)


@pytest.mark.parametrize("scale", [1.0, 10.0, 40.0])
def test_the_fp32_formula_restated_in_numpy_is_within_the_per_term_bounds(scale):
  rng = np.random.default_rng(int(scale))
  logit = (rng.standard_normal(2048) * scale).astype(F)
  diff = (logit[:1024, None] - logit[None, 1024:]).astype(F)
  t64, s64 = AT.terms64(diff)
  t32, s32 = AT.terms32(diff)
  mid = (diff > F(-87)) & (diff < F(88))   # the outer branches are exact
  assert np.array_equal(t32[~mid], t64[~mid]) and np.array_equal(s32[~mid], s64[~mid])
  et = (np.abs(t32 - t64)[mid] / np.abs(t64[mid])).max() / AT.EPS
  es = (np.abs(s32 - s64)[mid] / np.abs(s64[mid])).max() / AT.EPS
  print("scale %g: t within %.2f, s within %.2f of 2^-23" % (scale, et, es))
  assert et <= AT.TERM_FACTOR and es <= AT.WEIGHT_FACTOR


# ---- the core header on the host ----------------------------------------------------------------------------
def _build(tmp_path_factory, name, extra):
  exe = str(tmp_path_factory.mktemp(name) / "auc_host")
  subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-DMHTE_HOST_ONLY", "-ffp-contract=off"] + extra +
                        ["-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         os.path.join(ROOT, "tests", "auc_host_driver.cc"), "-o", exe])
  return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  return _build(tmp_path_factory, "auc", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
  return _build(tmp_path_factory, "auc_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, *args):
  return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout


def _sweep():
  """diffs: every threshold and its neighbours on both sides, zeros, a dense sweep, powers of two, the edges."""
  out = [EDGE_DIFFS, np.array([0.0, -0.0, 1e-30, -1e-30, 1e-45, -1e-45], dtype=F)]
  for x in (F(-87), F(88), F(0)):
    lo = hi = x
    for _ in range(4):
      lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
      out.append(np.array([lo, hi], dtype=F))
  out.append(np.linspace(-90, 90, 7201).astype(F))
  out.append((2.0 ** np.arange(-40, 8)).astype(F))
  out.append((-(2.0 ** np.arange(-40, 8))).astype(F))
  out.append(np.random.default_rng(5).uniform(-88, 88, 4000).astype(F))
  return np.concatenate(out)


def _check_terms(exe, tmp_path):
  diffs = _sweep()
  path = str(tmp_path / "diffs.bin")
  diffs.tofile(path)
  words = np.array([[int(x, 16) for x in line.split()] for line in _run(exe, "terms", path).splitlines()],
                   dtype=np.uint32)
  t32, s32 = words[:, 0].copy().view(F), words[:, 1].copy().view(F)
  t64, s64 = AT.terms64(diffs)
  exact = ~((diffs > F(-87)) & (diffs < F(88)))   # the outer branches (NaN included): the truth's bits
  assert np.array_equal(AT.bits(t32[exact]), AT.bits(t64[exact].astype(F)))
  assert np.array_equal(AT.bits(s32[exact]), AT.bits(s64[exact].astype(F)))
  mid = ~exact
  et = np.abs(t32[mid] - t64[mid]) / np.abs(t64[mid])
  es = np.abs(s32[mid] - s64[mid]) / np.abs(s64[mid])
  print("host terms: t within %.2f, s within %.2f of 2^-23" % (et.max() / AT.EPS, es.max() / AT.EPS))
  assert et.max() <= AT.TERM_FACTOR * AT.EPS and es.max() <= AT.WEIGHT_FACTOR * AT.EPS


def test_constants_and_classification_on_the_host(driver, tmp_path):
  consts = dict((k, int(v)) for k, v in (line.split() for line in _run(driver, "consts").splitlines()))
  assert consts == dict(threads=256, tile=AT.TILE, chunk=AT.CHUNK, stage=AT.STAGE, scan_tile=AT.SCAN_TILE,
                        max_groups=AT.MAX_GROUPS, group_elems=AT.GROUP_ELEMS, min_budget=AT.MIN_BUDGET,
                        counters=len(AT.COUNTERS))
  assert losses.COUNTER_NAMES == AT.COUNTERS
  labels = np.concatenate([EDGE_LABELS, np.array([np.inf, -np.inf, -9999.999, np.nextafter(F(-10000), F(0)),
                                                  np.nextafter(F(0), F(1)), -np.nextafter(F(0), F(1))], dtype=F)])
  path = str(tmp_path / "labels.bin")
  labels.tofile(path)
  got = [int(x) for x in _run(driver, "classify", path).split()]
  assert got == list(AT.classify(labels)) and got[:8] == EDGE_CLASSES


def test_term_functions_on_the_host_are_within_the_per_term_bounds(driver, tmp_path):
  _check_terms(driver, tmp_path)


PLAN_NS = [1, 63, 64, 65, 1023, 1024, 1025, 8192, 65536, 131072, 131073, (1 << 19) + 1, 10 ** 6, 2 ** 31 - 1]


def test_plan_and_split_equal_their_restatement(driver):
  for n in PLAN_NS:
    lines = _run(driver, "plan", n).splitlines()
    got = [int(x) for x in lines[0].split()]
    want = AT.plan(n)
    assert got == [want[k] for k in ("scan_tiles", "pair_groups", "final_groups", "budget", "loss_slots", "bytes")], n
    offs = [int(x) for x in lines[1].split()]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[-1] + 8 * want["budget"] <= want["bytes"]
  assert AT.plan(65536)["bytes"] < 16 << 20   # (the workspace at the flagship batch: low tens of MB at most)
  t = AT.TILE
  for budget in (AT.MIN_BUDGET, 4 * t, 1024 * t):
    for A in (0, 1, t - 1, t, t + 1, 3 * t + 5, 65536):
      for B in (0, 1, t - 1, t, t + 1, 3 * t + 5, 65536, 2 ** 31 - 1):
        if budget < (A + t - 1) // t * t:
          continue   # (the plan's budget holds one chunk of every element)
        got = tuple(int(x) for x in _run(driver, "split", A, B, budget).split())
        assert got == AT.split(A, B, budget), (A, B, budget)
        a_tiles, chunks, chunk_len, stride = got
        assert chunks * stride <= budget or chunks == 1           # the partials fit
        assert a_tiles * chunks <= max(budget // t, a_tiles)      # ... and the loss slots
        if A and B:
          assert (chunks - 1) * chunk_len < B <= chunks * chunk_len and chunk_len % AT.CHUNK == 0
  n2 = AT.smallest_two_pass_n()
  assert n2 == 8192 and min(AT.items(n2 // 2, n2 // 2, n2)) >= 2 * AT.plan(n2)["pair_groups"]


def _pairs(exe, A, B, budget):
  text = _run(exe, "pairs", A, B, budget)
  return np.array(np.fromstring(text, dtype=np.int64, sep=" ") if text else [], dtype=np.int64).reshape(-1, 2)


def _check_cover(exe, sizes, budgets):
  for budget in budgets:
    for A in sizes:
      for B in sizes:
        if budget < (A + AT.TILE - 1) // AT.TILE * AT.TILE:
          continue
        got = _pairs(exe, A, B, budget)
        assert got.shape[0] == A * B, (A, B, budget, got.shape)
        if A * B:
          flat = got[:, 0] * B + got[:, 1]
          assert flat.min() >= 0 and got[:, 0].max() < A and got[:, 1].max() < B
          assert np.unique(flat).size == A * B, (A, B, budget)   # every pair once, none twice


def test_plan_covers_every_pair_exactly_once(driver):
  t = AT.TILE
  sizes = [0, 1, t - 1, t, t + 1, 3 * t + 5]
  _check_cover(driver, sizes, [AT.MIN_BUDGET, 4 * t])   # one chunk per 256, and chunks forced long by the budget
  # a chunk longer than one LDS stage, and the order of a small case
  _check_cover(driver, [1, 2 * AT.STAGE + 3], [2 * AT.STAGE + 256 + 3])
  got = _pairs(driver, t + 1, 2 * t + 3, AT.MIN_BUDGET)
  want = np.array(AT.pairs_visited(t + 1, 2 * t + 3, AT.MIN_BUDGET))
  assert np.array_equal(got, want)


def test_the_driver_under_the_address_and_undefined_behaviour_sanitizers(sanitized, tmp_path):
  """The same program, built with -fsanitize=address,undefined and run as a program: a finding aborts it."""
  _check_terms(sanitized, tmp_path)
  t = AT.TILE
  _check_cover(sanitized, [0, 1, t + 1], [AT.MIN_BUDGET, 4 * t])
  for n in PLAN_NS:
    _run(sanitized, "plan", n)
  for A, B in ((2 ** 31 - 1, 2 ** 31 - 1), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1)):
    b = AT.plan(2 ** 31 - 1)["budget"]
    assert tuple(int(x) for x in _run(sanitized, "split", A, B, b).split()) == AT.split(A, B, b)


# ---- the refusals, before any device call ---------------------------------------------------------------------
def _fwd(label=FAKE, logit=2 * FAKE, n=8, neg_weight=1.0, loss=3 * FAKE, unit_grad=None):
  L = _lib.lib()
  st = L.mhte_inbatch_auc_loss(label, logit, n, neg_weight, loss, unit_grad, None)
  return st, L.mhte_last_error().decode()


def _grad(label=FAKE, logit=2 * FAKE, n=8, grad=1.0, grad_dev=None, neg_weight=1.0, logit_grad=4 * FAKE):
  L = _lib.lib()
  st = L.mhte_inbatch_auc_loss_grad(label, logit, n, grad, grad_dev, neg_weight, logit_grad, None)
  return st, L.mhte_last_error().decode()


def _invalid(fn, name, needle, **kw):
  st, msg = fn(**kw)
  assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
  assert msg.startswith(name + ": "), msg
  assert needle in msg, msg


@pytest.mark.parametrize("fn,name", [(_fwd, "inbatch_auc_loss"), (_grad, "inbatch_auc_loss_grad")],
                         ids=["forward", "gradient"])
def test_entry_points_refuse_invalid_arguments_on_the_host(fn, name):
  bad = lambda needle, **kw: _invalid(fn, name, needle, **kw)  # noqa: E731
  bad("null argument: label", label=None)
  bad("null argument: logit", logit=None)
  bad("label must be 4-byte aligned", label=FAKE + 2)
  bad("logit must be 4-byte aligned", logit=2 * FAKE + 1)
  bad("n must be >= 0, got -1", n=-1)
  bad("n must be below 2^31, got 2147483648", n=2 ** 31)
  bad("n must be below 2^31", n=2 ** 40)
  for w in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
    bad("neg_weight must be in (0, 1], got", neg_weight=w)
  if fn is _fwd:
    bad("null argument: loss", loss=None)
    bad("null argument: loss", loss=None, n=0, label=None, logit=None)
    bad("loss must be 4-byte aligned", loss=3 * FAKE + 2)
    bad("unit_grad must be 4-byte aligned", unit_grad=5 * FAKE + 1)
  else:
    bad("null argument: logit_grad", logit_grad=None)
    bad("logit_grad must be 4-byte aligned", logit_grad=4 * FAKE + 3)
    bad("grad_dev must be 4-byte aligned", grad_dev=6 * FAKE + 2)


def test_launch_counts_refusals():
  L = _lib.lib()
  out = (C.c_int64 * 9)()
  assert L.mhte_inbatch_auc_launch_counts(None, 9) == _lib.MHTE_INVALID_ARGUMENT
  assert "inbatch_auc_launch_counts: null argument: out" in L.mhte_last_error().decode()
  assert L.mhte_inbatch_auc_launch_counts(out, 8) == _lib.MHTE_INVALID_ARGUMENT
  assert "n must be 9, got 8" in L.mhte_last_error().decode()
  assert L.mhte_inbatch_auc_launch_counts(out, 9) == _lib.MHTE_OK   # needs no device
  assert tuple(losses.inbatch_auc_launch_counts()) == AT.COUNTERS
  assert monolith_amd.inbatch_auc_launch_counts is losses.inbatch_auc_launch_counts


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_a_valid_call_without_a_device_is_unavailable():
  for kw in ({}, {"n": 0, "label": None, "logit": None}, {"n": 2 ** 31 - 1}, {"neg_weight": 0.25},
             {"label": FAKE + 4, "logit": 2 * FAKE + 12}):
    for fn in (_fwd, _grad):
      st, msg = fn(**kw)
      assert st == _lib.MHTE_UNAVAILABLE, (fn.__name__, kw, st, msg)
      assert "no CPU fallback" in msg
  st, msg = _fwd(unit_grad=5 * FAKE)
  assert st == _lib.MHTE_UNAVAILABLE, msg
  st, msg = _grad(grad_dev=6 * FAKE, n=0, label=None, logit=None, logit_grad=None)
  assert st == _lib.MHTE_UNAVAILABLE, msg
  assert not any(losses.inbatch_auc_launch_counts().values())


# ---- the surface ----------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in ("mhte_inbatch_auc_loss", "mhte_inbatch_auc_loss_grad", "mhte_inbatch_auc_launch_counts"):
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  for word in ("inbatch_auc_loss.cc:30-138", "inbatch_auc_loss_test.py", "neg_weight outside (0, 1]"):
    assert word in text, word
  p, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
  sig = _lib.signatures()
  assert sig["mhte_inbatch_auc_loss"] == (i32, [p, p, i64, f32, p, p, p])
  assert sig["mhte_inbatch_auc_loss_grad"] == (i32, [p, p, i64, f32, p, f32, p, p])
  assert sig["mhte_inbatch_auc_launch_counts"] == (i32, [p, i32])
  for name in ("losses", "inbatch_auc_loss", "inbatch_auc_loss_grad", "inbatch_auc_launch_counts"):
    assert name in monolith_amd.__all__ and getattr(monolith_amd, name) is not None


# ---- the Python mirror ----------------------------------------------------------------------------------------
def test_python_argument_contract():
  a, b = torch.zeros(8), torch.zeros(8)
  fns = ((losses.inbatch_auc_loss, "inbatch_auc_loss"),
         (lambda la, lo, nw=1.0: losses.inbatch_auc_loss_grad(la, lo, 1.0, nw), "inbatch_auc_loss_grad"))
  for fn, name in fns:
    with pytest.raises(ValueError, match="%s: the label and logit not match" % name):
      fn(a, torch.zeros(7))
    with pytest.raises(ValueError, match="the label and logit not match"):
      fn(torch.zeros(4, 2), torch.zeros(9, 1))
    with pytest.raises(TypeError, match="label must be float32"):
      fn(a.double(), b)
    with pytest.raises(TypeError, match="logit must be float32"):
      fn(a, b.half())
    with pytest.raises(TypeError, match="logit must be a torch tensor"):
      fn(a, b.numpy())
    with pytest.raises(ValueError, match="logit must be contiguous"):
      fn(a, torch.zeros(8, 2)[:, 0])
    with pytest.raises(ValueError, match="label must be contiguous"):
      fn(torch.zeros(16)[::2], b)
    for w in (0.0, -1.0, 1.5, float("nan")):
      with pytest.raises(ValueError, match=r"neg_weight must be in \(0, 1\]"):
        fn(a, b, w)
    with pytest.raises(TypeError, match="must be on the GPU"):   # checked last: there is no CPU path
      fn(a, b)
  with pytest.raises(TypeError, match="grad must be a float or a 0-d float32 tensor on the GPU"):
    losses.inbatch_auc_loss_grad(a, b, torch.ones(()), 1.0)
