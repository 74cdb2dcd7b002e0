"""CPU suite of the touched-key set: the key-by-key truth model reproduces the reference's documented
cases (touched_key_set_ops_test.py; hopscotch_hash_set_test overflow, scaled), the new symbols are on the
whole surface, and what can be refused before the device is refused."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from touched_key_set_truth import TruthSet  # noqa: E402
from monolith_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
SYMBOLS = ["mhte_touched_key_set_create", "mhte_touched_key_set_destroy", "mhte_touched_key_set_insert",
           "mhte_touched_key_set_stats", "mhte_touched_key_set_steal", "mhte_multi_table_set_touched_key_set"]


def test_truth_reference_basic_case():
  t = TruthSet(1000)
  assert t.insert(range(1000)) == 0
  assert t.stats() == (1000, 0, 0, 1000)
  assert [k[0] for k in t.steal()] == list(range(1000))
  assert t.stats()[0] == 0


def test_truth_reference_overflow_case():
  t = TruthSet(1000)
  assert t.insert(range(1005)) == 1001
  assert [k[0] for k in t.steal()] == [1001, 1002, 1003, 1004]


def test_truth_overflow_scaled():
  C_ = 1000
  t = TruthSet(C_)
  t.insert(range(20 * C_ + 500))
  assert t.clears == 20 and t.dropped == 20 * (C_ + 1)


def test_truth_empty_call_never_clears_and_duplicates_trigger():
  t = TruthSet(2)
  t.insert([1, 2, 3])          # size C + 1, no clear yet
  assert t.stats() == (3, 0, 0, 2)
  t.insert([])
  assert t.stats() == (3, 0, 0, 2)
  t.insert([3])                # a duplicate still finds the set over capacity
  assert t.stats() == (1, 3, 1, 2)
  a = TruthSet(3)
  a.insert_segments([([7], 0), ([7], 1)])
  assert a.stats()[0] == 2     # one fid under two tags is two keys


def test_symbols_declared_exported_and_listed():
  src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
  declared = set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src))
  L = C.CDLL(_lib.build_library())
  for s in SYMBOLS:
    assert s in declared, s
    assert s in _lib.EXPORTS, s
    assert hasattr(L, s), s
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", open(HEADER).read())   # additive: no bump
  from monolith_amd.touched_key_set_ops import TouchedKeySet
  from monolith_amd.multi_hash_table_ops import MultiHashTable
  for m in ("insert", "steal", "steal_pairs", "capacity", "size", "handle"):
    assert hasattr(TouchedKeySet, m), m
  assert callable(MultiHashTable.set_touched_key_set) and callable(MultiHashTable.touched_entries)


def test_arguments_refused_before_the_device():
  L = _lib.lib()
  h = C.c_void_p()
  for cap in (0, -5):
    assert L.mhte_touched_key_set_create(C.c_int64(cap), C.c_int64(0), C.c_int32(0), C.byref(h)) == \
        _lib.MHTE_INVALID_ARGUMENT
    assert b"capacity" in L.mhte_last_error()
  assert L.mhte_touched_key_set_create(C.c_int64(8), C.c_int64(0), C.c_int32(0), None) == _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_touched_key_set_create(C.c_int64(8), C.c_int64(-1), C.c_int32(0), C.byref(h)) == \
      _lib.MHTE_INVALID_ARGUMENT
  fake = C.c_void_p(0x10000)   # handles and device pointers the host never follows on these paths
  assert L.mhte_touched_key_set_insert(fake, fake, C.c_int64(-1), None, C.c_int32(0), None) == \
      _lib.MHTE_INVALID_ARGUMENT
  assert b"n_max" in L.mhte_last_error()
  assert L.mhte_touched_key_set_insert(fake, fake, C.c_int64(4), None, C.c_int32(-1), None) == \
      _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_touched_key_set_insert(None, fake, C.c_int64(4), None, C.c_int32(0), None) == \
      _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_touched_key_set_stats(fake, None, None) == _lib.MHTE_INVALID_ARGUMENT
  n = C.c_int64(0)
  assert L.mhte_touched_key_set_steal(fake, fake, fake, C.c_int64(4), None, None) == _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_touched_key_set_steal(None, fake, fake, C.c_int64(4), C.byref(n), None) == \
      _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_touched_key_set_steal(fake, fake, fake, C.c_int64(-1), C.byref(n), None) == \
      _lib.MHTE_INVALID_ARGUMENT
  assert L.mhte_multi_table_set_touched_key_set(None, None) == _lib.MHTE_INVALID_ARGUMENT
  L.mhte_touched_key_set_destroy(None)   # a no-op


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_no_gpu_means_loud_failure():
  L = _lib.lib()
  h = C.c_void_p()
  assert L.mhte_touched_key_set_create(C.c_int64(64), C.c_int64(0), C.c_int32(0), C.byref(h)) == \
      _lib.MHTE_UNAVAILABLE
  assert b"no CPU fallback" in L.mhte_last_error()
  from monolith_amd.touched_key_set_ops import TouchedKeySet
  with pytest.raises(_lib.MhteError):
    TouchedKeySet(64)
