"""CPU suite of the dense optimizers (csrc/mhte_dense_opt_core.h, mhte_dense_opt_host.h,
monolith_amd/optimizers.py): the numpy truth (tests/dense_opt_truth.py) holds the reference's goldens within
their own eps; the element functions of the core header, compiled for the host, equal the truth bit for bit
over 25 steps; the chunk table equals its numpy restatement; every argument the entry points can refuse on the
host is refused there, with the entry point's name and the argument; a valid call without a device is refused
loudly; the symbols are on the surface and the ABI version stands; the Python classes check their arguments."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_opt_truth as DT  # noqa: E402
import flat_concat_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
FAKE = 0x10000   # a "device pointer" the host never follows
LENS = [0, 1, 15, 16, 17, 0, 4096, 4097, 1000003, 5]
F = np.float32


# ---- the goldens of the reference, through the truth ----------------------------------------------------
@pytest.mark.parametrize("golden", DT.GOLDENS, ids=[g[0] for g in DT.GOLDENS])
def test_truth_holds_the_reference_s_goldens(golden):
  kind, hyper, var0, g0, want = golden
  model = DT.Model(kind, [np.array([var0], F)], hyper)
  model.step([np.array([g0], F)])
  got = {"var": model.vars[0][0]}
  got.update({s: model.slots[s][0][0] for s in DT.SLOTS[kind]})
  assert sorted(got) == sorted(want)
  for k, w in want.items():
    print("%s %s: %.10g (golden %.10g, off by %.2g)" % (kind, k, got[k], w, abs(float(got[k]) - w)))
    assert abs(float(got[k]) - w) <= DT.GOLDEN_EPS, (kind, k, got[k], w)


# ---- the element functions on the host --------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
  exe = str(tmp_path_factory.mktemp("dense_opt") / "dense_opt_host")
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMHTE_HOST_ONLY", "-ffp-contract=off",
                         "-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         os.path.join(ROOT, "tests", "dense_opt_host_driver.cc"), "-o", exe])
  return exe


@pytest.mark.parametrize("kind", DT.KINDS)
def test_core_arithmetic_on_the_host_equals_the_truth(kind, driver, tmp_path):
  dim, steps, scale = 24, 25, 0.37
  rng = np.random.default_rng(77 + DT.KINDS.index(kind))
  var0 = rng.standard_normal(dim).astype(F)
  grads = DT.seeded_grads([(dim,)], steps, seed=5 + DT.KINDS.index(kind))
  h = DT.HYPER[kind]
  assert h["weight_decay"] != 0
  ab = (h["ada_decay"], h["mom_decay"]) if kind.startswith("adamom") else (h["beta1"], h["beta2"])
  path = str(tmp_path / "case.bin")
  with open(path, "wb") as f:
    f.write(struct.pack("<3i", DT.KINDS.index(kind), dim, steps))
    f.write(struct.pack("<6f", scale, h["learning_rate"], ab[0], ab[1], h["epsilon"], h["weight_decay"]))
    f.write(var0.tobytes())
    for g in grads:
      f.write(g[0].tobytes())
  out = subprocess.run([driver, "steps", path], capture_output=True, text=True, check=True).stdout
  got = np.array([int(x, 16) for x in out.split()], dtype=np.uint32).view(F).reshape(-1, dim)
  watch = DT.Tracker()
  model = DT.Model(kind, [var0], watch=watch)
  for g in grads:
    model.step(g, grad_scale=scale)
  want = [model.vars[0]] + [model.slots[s][0] for s in DT.SLOTS[kind]]
  assert got.shape[0] == len(want)
  for name, a, b in zip(("var",) + DT.SLOTS[kind], got, want):
    DT.assert_same_bits(a, b, "%s %s" % (kind, name))
    assert np.isfinite(b).all() and np.any(b != 0)
  assert not np.array_equal(model.vars[0], var0)


def _table_truth(lens, align, null_at):
  """(index, len, off, chunk0) of the variables that take part, and the number of chunks."""
  off = T.offsets(lens, align)
  rows, chunks = [], 0
  for i, n in enumerate(lens):
    if n == 0 or i == null_at:
      continue
    rows.append((i, n, off[i], chunks))
    chunks += (n + 4095) // 4096
  return rows, chunks


@pytest.mark.parametrize("align", [4, 16, 1024])
@pytest.mark.parametrize("null_at", [7, -1, -2], ids=["null gradient", "all gradients", "flat source"])
def test_chunk_table_equals_numpy(align, null_at, driver):
  out = subprocess.run([driver, "table", str(align), str(null_at)] + [str(n) for n in LENS], capture_output=True,
                       text=True, check=True).stdout.split("\n")
  rows, chunks = _table_truth(LENS, align, null_at)
  assert out[0].split() == [str(len(rows)), str(chunks)]
  got = [tuple(int(x) for x in line.split()) for line in out[1:] if line]
  assert got == [r + (1,) for r in rows]   # (the last column: the entry carries its own gradient, or none)
  assert all(r[2] % align == 0 for r in rows)
  if null_at == 7:   # the skipped variable still occupies its span of the slots
    nxt = [r for r in rows if r[0] == 8][0]
    assert nxt[2] == T.offsets(LENS, align)[8] and all(r[0] != 7 for r in rows)
  big = subprocess.run([driver, "table", str(align), "-1", str(2 ** 43)], capture_output=True, text=True, check=True)
  assert big.stdout.strip() == "too many chunks"


# ---- the refusals, before any device call -----------------------------------------------------------------
ENTRY = {"adamom": "mhte_dense_apply_adamom", "rmsprop": "mhte_dense_apply_rmsprop"}


def _apply(which, lens=(8, 0, 5), n=None, align=16, null=(), null_var=(), null_grad=(), source="list", wire=0,
           slot=64 * FAKE, slot_elems=None, flat=128 * FAKE, update_slots=1, use_v2=0, scale_dev=None, lr_dev=None):
  L = _lib.lib()
  lens = list(lens)
  k = len(lens)
  pv = (C.c_void_p * max(k, 1))(*[None if i in null_var else FAKE + 65536 * i for i in range(k)])
  pg = (C.c_void_p * max(k, 1))(*[None if i in null_grad else 2 * FAKE + 65536 * i for i in range(k)])
  ln = (C.c_int64 * max(k, 1))(*lens)
  a = {"vars": pv, "lens": ln, "m": C.c_void_p(slot), "v": C.c_void_p(slot + 16 * FAKE), "c": C.c_void_p(slot + 32 * FAKE)}
  for name in null:
    a[name] = None
  if slot_elems is None:
    slot_elems = T.offsets([max(v, 0) for v in lens], align if align in (4, 16, 1024) else 16)[-1]
  grads = pg if source in ("list", "both") else None
  gflat = C.c_void_p(flat) if source in ("flat", "both") else None
  nn = k if n is None else n
  if which == "adamom":
    st = L.mhte_dense_apply_adamom(a["vars"], a["lens"], nn, align, a["m"], a["v"], a["c"], slot_elems, grads, gflat,
                                   wire, 0.5, scale_dev, 0.01, lr_dev, 0.99, 0.9, 1e-6, 0.01, update_slots, use_v2,
                                   None)
  else:
    st = L.mhte_dense_apply_rmsprop(a["vars"], a["lens"], nn, align, a["m"], a["v"], slot_elems, grads, gflat, wire,
                                    0.5, scale_dev, 0.01, lr_dev, 0.9, 0.9, 0.1, 0.01, update_slots, use_v2, None)
  return st, L.mhte_last_error().decode()


@pytest.mark.parametrize("which", ["adamom", "rmsprop"])
def test_refuses_invalid_arguments_on_the_host(which):
  def invalid(needle, **kw):
    st, msg = _apply(which, **kw)
    assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
    assert msg.startswith(ENTRY[which][len("mhte_"):] + ": "), msg
    assert needle in msg, msg

  invalid("null argument: vars", null=("vars",))
  invalid("null argument: lens", null=("lens",))
  invalid("null argument: m", null=("m",))
  invalid("null argument: v", null=("v",))
  if which == "adamom":
    invalid("null argument: c", null=("c",))
  invalid("n must be >= 0", n=-1)
  invalid("variable 2 has the negative length -5", lens=(8, 0, -5))
  invalid("null argument: vars[2]", null_var=(2,))
  invalid("exactly one of grads and grads_flat", source="both")
  invalid("exactly one of grads and grads_flat", source="neither")
  invalid("wire must be 0 (fp32) or 1 (fp16), got 2", wire=2)
  invalid("wire must be 0 (fp32) or 1 (fp16), got -1", wire=-1, source="flat")
  invalid("wire 1 needs grads_flat", wire=1)
  for al in (0, 1, 2, 3, 24, 2048, -4):
    invalid("align_elems must be a power of two in [4, 1024], got %d" % al, align=al)
  invalid("slot_elems must be the aligned total 32, got 31", slot_elems=31)
  invalid("slot_elems must be the aligned total 32, got 13", slot_elems=13)
  invalid("slot_elems must be the aligned total 2048, got 32", align=1024, slot_elems=32)
  invalid("slot buffers must be 16-byte aligned", slot=64 * FAKE + 4)
  invalid("grads_flat must be 16-byte aligned", source="flat", flat=128 * FAKE + 8)
  invalid("grads_flat must be 16-byte aligned", source="flat", flat=128 * FAKE + 8, wire=1)
  invalid("2^31 chunks", lens=(2 ** 43,))
  invalid("2^31 chunks", lens=(2 ** 42, 7, 2 ** 42), source="flat")
  invalid("update_slots must be 0 or 1, got 2", update_slots=2)
  invalid("use_v2 must be 0 or 1, got -1", use_v2=-1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
@pytest.mark.parametrize("which", ["adamom", "rmsprop"])
def test_a_valid_call_without_a_device_is_unavailable(which):
  for kw in ({}, {"lens": (), "n": 0}, {"null_grad": (0,)}, {"null_var": (1,)}, {"source": "flat"},
             {"source": "flat", "wire": 1}, {"align": 1024}, {"use_v2": 1}, {"update_slots": 0},
             {"scale_dev": C.c_void_p(FAKE - 64), "lr_dev": C.c_void_p(FAKE - 32)},
             {"lens": (0, 0), "null": ("m", "v", "c")}):   # (nothing to keep: the slots may be null)
    st, msg = _apply(which, **kw)
    assert st == _lib.MHTE_UNAVAILABLE, (kw, st, msg)
    assert "no CPU fallback" in msg


# ---- the surface ------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_listed():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in ENTRY.values():
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  for word in ("ResourceApplyAdamom", "ResourceApplyRmsprop", "training_ops"):
    assert word in text, word
  m = re.search(r"#define\s+MHTE_DENSE_OPT_INLINE\s+(\d+)", text)
  assert m and int(m.group(1)) == _lib.DENSE_OPT_INLINE
  assert 36 * _lib.DENSE_OPT_INLINE + 256 <= 4096   # the table's 36 bytes per variable: the arguments fit 4 KB
  p, i32, i64, f = C.c_void_p, C.c_int32, C.c_int64, C.c_float
  sig = _lib.signatures()
  assert sig["mhte_dense_apply_adamom"] == (i32, [p, p, i32, i32, p, p, p, i64, p, p, i32, f, p, f, p, f, f, f, f, i32,
                                                  i32, p])
  assert sig["mhte_dense_apply_rmsprop"] == (i32, [p, p, i32, i32, p, p, i64, p, p, i32, f, p, f, p, f, f, f, f, i32,
                                                   i32, p])


# ---- the Python mirror ------------------------------------------------------------------------------------
def test_python_argument_contract():
  from monolith_amd import optimizers as O
  assert O.AdamomOptimizer().get_slot_names() == ["m", "v", "c"]
  assert O.RmspropOptimizer().get_slot_names() == ["m", "v"]
  for cls in (O.AdamomOptimizer, O.RmspropOptimizer):
    opt = cls()
    assert opt.align == 16
    with pytest.raises(_lib.InvalidArgumentError, match="align_elems"):
      cls(align=24)
    v = torch.zeros(3)
    with pytest.raises(TypeError, match="contiguous float32 tensors on the GPU"):
      opt.apply_gradients([(torch.zeros(3), v)])                       # a host variable
    with pytest.raises(TypeError, match="contiguous float32 tensors on the GPU"):
      opt.apply_flat(torch.zeros(16), variables=[torch.zeros(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="empty variable list"):
      opt.apply_gradients([])
    with pytest.raises(ValueError, match="the first apply needs the variables"):
      opt.apply_flat(torch.zeros(16))
    with pytest.raises(ValueError, match="no slots before the first apply"):
      opt.state_dict()
    with pytest.raises(KeyError):
      opt.get_slot(v, "m")
    with pytest.raises(KeyError, match="has the slots"):
      opt.get_slot(v, "accumulator")
    with pytest.raises(ValueError, match="align"):
      opt.load_state_dict({"align": 4, "numels": [3], "m": torch.zeros(4), "v": torch.zeros(4), "c": torch.zeros(4)})
    with pytest.raises(ValueError, match="1-d tensor of 16 elements"):
      opt.load_state_dict({"align": 16, "numels": [3], "m": torch.zeros(4), "v": torch.zeros(4), "c": torch.zeros(4)})

