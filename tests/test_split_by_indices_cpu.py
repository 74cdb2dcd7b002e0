"""CPU suite of the split-by-indices ops (csrc/mhte_split_kernels.h, mhte_split_host.h,
monolith_amd/distribution_ops.py, monolith_amd/distributed_ps.py): the numpy truth
(tests/split_by_indices_truth.py) reproduces the reference's examples; the entry points are on the surface with
the ABI version unchanged; what the host can refuse it refuses with the entry point's name; a valid call
without a device is refused loudly; the Python functions exist and check their arguments before any device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import split_by_indices_truth as ST  # noqa: E402
from monolith_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
FAKE = 0x10000   # a "device pointer" the host never follows
ENTRY = ("mhte_split_plan", "mhte_split_rows", "mhte_split_rows_grad", "mhte_split_launch_counts")


# ---- the reference's examples, through the truth ----------------------------------------------------------
def test_truth_split_by_indices_example():
  ids = np.array([0, 1, 2, 2, 3], np.int64)
  got = ST.split(ids % 3, ids, 3)
  assert [g.tolist() for g in got] == [[0, 3], [1], [2, 2]]
  pos, sizes, n_bad = ST.plan(ids % 3, 3)
  assert pos.tolist() == [0, 4, 1, 2, 3] and sizes.tolist() == [2, 1, 2] and n_bad == 0


def test_truth_gradient_examples():
  indices = np.array([0, 1, 0], np.int64)
  tensor = np.array([[0, 0], [1, 1], [2, 2]], np.float32)
  splits = ST.split(indices, tensor, 3)
  assert [s.shape for s in splits] == [(2, 2), (1, 2), (0, 2)]
  grad = ST.gradient(indices, [np.ones_like(s) for s in splits], tensor.shape)
  assert grad.tolist() == [[1, 1], [1, 1], [1, 1]]
  # each row comes from the row of its split that it became
  grads = [np.array([[1, 2], [3, 4]], np.float32), np.array([[5, 6]], np.float32), np.zeros((0, 2), np.float32)]
  assert ST.gradient(indices, grads, tensor.shape).tolist() == [[1, 2], [5, 6], [3, 4]]
  empty = ST.split(np.zeros(0, np.int64), np.zeros(0, np.float32), 3)
  assert [e.shape for e in empty] == [(0,)] * 3
  assert ST.gradient(np.zeros(0, np.int64), empty, (0,)).tolist() == []


def test_truth_ragged_examples():
  indices = np.array([0, 1, 0, 1], np.int64)
  # six rows of which four are empty: [[], [], [4, 3, 2], [1], [], []]
  splits, pos = ST.ragged_split(indices, [4, 3, 2, 1], [0, 0, 0, 3, 4, 4, 4], 2)
  assert [ST.to_lists(*s) for s in splits] == [[[], [], [4, 2], [], [], []], [[], [], [3], [1], [], []]]
  assert [ST.to_lists(*p) for p in pos] == [[[], [], [0, 2], [], [], []], [[], [], [1], [3], [], []]]
  # the docstring's example
  splits, pos = ST.ragged_split(indices, [4, 3, 2, 1], [0, 3, 4], 2)
  assert [ST.to_lists(*s) for s in splits] == [[[4, 2], []], [[3], [1]]]
  assert [ST.to_lists(*p) for p in pos] == [[[0, 2], []], [[1], [3]]]
  with pytest.raises(AssertionError, match="The input ragged tensor is invalid"):
    ST.split_row_splits(indices, [0, 3, 5], 2)


def test_truth_row_splits_are_lower_bounds_of_the_positions():
  """What the device computes: entry [s][t] counts the positions of split s below row_splits[t]."""
  rng = np.random.RandomState(3)
  indices = rng.randint(0, 5, size=200).astype(np.int64)
  rs = np.array([0, 0, 17, 17, 90, 200, 200], np.int64)
  want = ST.split_row_splits(indices, rs, 5)
  pos = ST.split(indices, np.arange(200, dtype=np.int64), 5)
  got = np.array([[np.searchsorted(p, e, side="left") for e in rs] for p in pos], np.int64)
  assert np.array_equal(got, want)


# ---- the surface ------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
  text = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in ENTRY:
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", text) and _lib.ABI_VERSION == 19   # additive: no bump
  for word in ("MonolithSplitByIndices", "MonolithRaggedSplitByIndices", "split_by_indices_op.cc"):
    assert word in text, word
  p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
  sig = _lib.signatures()
  assert sig["mhte_split_plan"] == (i32, [p, i64, i32, p, i32, p, p, p, p, p, p])
  assert sig["mhte_split_rows"] == (i32, [p, i64, i64, i32, p, p, p])
  assert sig["mhte_split_rows_grad"] == (i32, [p, p, i32, i64, i64, i32, p, p, p])
  assert sig["mhte_split_launch_counts"] == (i32, [p, i32])


def _plan(n=8, num_splits=3, row_splits=None, null=(), **over):
  a = dict(indices=FAKE, pos=2 * FAKE, sizes=3 * FAKE, srs=4 * FAKE if row_splits is not None else None,
           n_bad=5 * FAKE)
  a.update(over)
  for k in null:
    a[k] = None
  rs = None if row_splits is None else np.ascontiguousarray(row_splits, np.int64)
  L = _lib.lib()
  st = L.mhte_split_plan(a["indices"], n, num_splits, None if rs is None else rs.ctypes.data_as(C.c_void_p),
                         over.get("n_row_splits", 0 if rs is None else rs.size), a["pos"], a["sizes"], a["srs"],
                         a["n_bad"], None, None)
  return st, L.mhte_last_error().decode()


def _rows(n=8, element_size=4, elem_bytes=4, inp=FAKE, pos=2 * FAKE, packed=3 * FAKE):
  L = _lib.lib()
  return L.mhte_split_rows(inp, n, element_size, elem_bytes, pos, packed, None), L.mhte_last_error().decode()


def _grad(n=8, num_splits=3, element_size=4, elem_bytes=4, table=(FAKE, 2 * FAKE, 3 * FAKE), sizes=4 * FAKE,
          pos=5 * FAKE, out=6 * FAKE, null_table=False):
  L = _lib.lib()
  tab = (C.c_void_p * max(len(table), 1))(*table)
  st = L.mhte_split_rows_grad(None if null_table else tab, sizes, num_splits, n, element_size, elem_bytes, pos, out,
                              None)
  return st, L.mhte_last_error().decode()


def test_refuses_invalid_arguments_on_the_host():
  def invalid(call, needle, **kw):
    st, msg = call(**kw)
    assert st == _lib.MHTE_INVALID_ARGUMENT, (kw, st, msg)
    assert msg.startswith({_plan: "split_plan", _rows: "split_rows", _grad: "split_rows_grad"}[call] + ": "), msg
    assert needle in msg, msg

  for bad in (0, -1, 1025):
    invalid(_plan, "num_splits must be in [1, 1024]", num_splits=bad)
  invalid(_plan, "n must be >= 0", n=-1)
  invalid(_plan, "n must be below 2^31 - 1", n=2 ** 31 - 1)
  for name in ("indices", "pos", "sizes", "n_bad"):
    invalid(_plan, "null argument: " + name, null=(name,))
  invalid(_plan, "null argument: split_row_splits", row_splits=[0, 8], null=("srs",))
  invalid(_plan, "null argument: row_splits", n_row_splits=2)
  invalid(_plan, "pos must be 8-byte aligned", pos=FAKE + 4)
  for rs in ([1, 8], [0, 7], [0, 5, 4, 8], [0, 9, 8]):
    invalid(_plan, "The input ragged tensor is invalid.", row_splits=rs)
  invalid(_rows, "element_size must be >= 1", element_size=0)
  invalid(_rows, "elem_bytes must be 4 (float32) or 8 (int64)", elem_bytes=2)
  invalid(_rows, "null argument: input", inp=None)
  invalid(_rows, "null argument: packed", packed=None)
  invalid(_rows, "null argument: pos", pos=None)
  invalid(_rows, "input must be 4-byte aligned", inp=FAKE + 2)
  invalid(_rows, "overflows the kernels' 32-bit word index", n=2 ** 30, element_size=4)
  invalid(_grad, "num_splits must be in [1, 1024]", num_splits=0, table=())
  invalid(_grad, "null argument: grads", null_table=True)
  invalid(_grad, "null argument: sizes", sizes=None)
  invalid(_grad, "null argument: input_grads", out=None)
  invalid(_grad, "grads[i] must be 4-byte aligned", table=(FAKE, FAKE + 1, FAKE))
  L = _lib.lib()
  out = (C.c_int64 * 6)()
  assert L.mhte_split_launch_counts(out, 5) == _lib.MHTE_INVALID_ARGUMENT
  assert "n must be 6" in L.mhte_last_error().decode()
  assert L.mhte_split_launch_counts(None, 6) == _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_split_launch_counts(out, 6) == _lib.MHTE_OK   # (reads the counters: needs no device)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_a_valid_call_without_a_device_is_unavailable():
  for call, kw in ((_plan, {}), (_plan, {"n": 0, "null": ("indices", "pos")}), (_plan, {"row_splits": [0, 3, 3, 8]}),
                   (_rows, {}), (_rows, {"elem_bytes": 8, "inp": FAKE + 4}), (_rows, {"n": 0}),
                   (_grad, {}), (_grad, {"table": (FAKE, 0, FAKE + 4)})):
    st, msg = call(**kw)
    assert st == _lib.MHTE_UNAVAILABLE, (call.__name__, kw, st, msg)
    assert "no CPU fallback" in msg


# ---- the Python mirror ------------------------------------------------------------------------------------
def test_python_functions_exist_and_check_their_arguments_before_any_device():
  from monolith_amd import distribution_ops as D
  from monolith_amd.multi_hash_table_ops import Ragged
  for f in ("split_by_indices", "ragged_split_by_indices", "split_plan", "finalize_shared_tensor",
            "split_launch_counts"):
    assert callable(getattr(D, f)), f
  assert D.SPLIT_COUNTER_NAMES == ST.COUNTERS
  assert D.split_launch_counts().keys() == set(ST.COUNTERS)
  idx = torch.zeros(3, dtype=torch.int64)
  with pytest.raises(TypeError, match="indices must be on the GPU"):
    D.split_by_indices(idx, torch.zeros(3), 2)
  with pytest.raises(TypeError, match="indices must be on the GPU"):
    D.split_plan(idx, 2)
  with pytest.raises(TypeError, match="indices must be on the GPU"):
    D.ragged_split_by_indices(idx, Ragged(idx, np.array([0, 3], np.int64)), 2)
  with pytest.raises(TypeError, match="indices must be int64"):
    D.split_by_indices(idx.to(torch.int32), torch.zeros(3), 2)
  with pytest.raises(TypeError, match="num_splits must be an int"):
    D.split_plan(idx, 2.0)
  # finalize_shared_tensor touches no device
  buf = torch.arange(6, dtype=torch.float32)
  assert D.finalize_shared_tensor([buf, buf, buf], torch.float32, [None]) is not None
  assert D.finalize_shared_tensor([buf, buf], shape=[2, 3]).shape == (2, 3)
  assert D.finalize_shared_tensor([buf]).data_ptr() == buf.data_ptr()
  with pytest.raises(_lib.InvalidArgumentError, match="not the same shared tensor"):
    D.finalize_shared_tensor([buf, buf.clone()])
  with pytest.raises(TypeError, match="not torch.float16"):
    D.finalize_shared_tensor([buf], torch.float16)
  with pytest.raises(ValueError, match="non-empty list"):
    D.finalize_shared_tensor([])


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_without_a_device_there_is_no_sharded_table():
  from monolith_amd import entry
  from monolith_amd.distributed_ps import DistributedMultiTypeHashTable
  cfgs = {"t": entry.make_table_config(
      [entry.CombineAsSegment(4, entry.ZerosInitializer(), entry.SgdOptimizer())])}
  with pytest.raises(ValueError, match="num_ps must be an int >= 1"):
    DistributedMultiTypeHashTable(0, cfgs)
  with pytest.raises(_lib.MhteError) as e:
    DistributedMultiTypeHashTable(2, cfgs)
  assert e.value.code == _lib.MHTE_UNAVAILABLE
