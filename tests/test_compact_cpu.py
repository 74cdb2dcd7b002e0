"""CPU suite: table compaction (mhte_table_compact / mhte_table_set_auto_compact) on the whole surface —
declared in the header as an additive change, bound by _lib, exported by the library, reachable from
MultiHashTable — and, without a GPU, a loud failure like everything else."""
import ctypes as C
import os
import re

import pytest
import torch

from monolith_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")


def test_header_declares_compaction_and_the_abi_version_stands():
  text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
  assert re.search(r"mhte_status\s+mhte_table_compact\s*\(\s*mhte_multi_table\s*\*\s*t,\s*int32_t\s+table,\s*"
                   r"int64_t\s+out\[4\],\s*void\s*\*\s*stream\s*\)\s*;", text)
  assert re.search(r"mhte_status\s+mhte_table_set_auto_compact\s*\(\s*mhte_multi_table\s*\*\s*t,\s*int32_t\s+table,\s*"
                   r"double\s+min_free_fraction\s*\)\s*;", text)
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", open(HEADER).read()) and _lib.ABI_VERSION == 19   # additive


def test_binding_and_library_have_both_functions():
  vp, i32, st = C.c_void_p, C.c_int32, C.c_int32
  sigs = _lib.signatures()
  assert sigs["mhte_table_compact"] == (st, [vp, i32, vp, vp])
  assert sigs["mhte_table_set_auto_compact"] == (st, [vp, i32, C.c_double])
  L = C.CDLL(_lib.build_library())
  for name in ("mhte_table_compact", "mhte_table_set_auto_compact"):
    assert name in _lib.EXPORTS and hasattr(L, name)


def test_python_methods_exist_and_a_null_handle_is_refused():
  from monolith_amd.multi_hash_table_ops import MultiHashTable
  assert callable(MultiHashTable.compact) and callable(MultiHashTable.set_auto_compact)
  L = _lib.lib()
  out = (C.c_int64 * 4)()
  assert L.mhte_table_compact(None, 0, out, None) == _lib.MHTE_INVALID_ARGUMENT
  assert b"null table handle" in L.mhte_last_error()
  assert L.mhte_table_set_auto_compact(None, 0, 0.25) == _lib.MHTE_INVALID_ARGUMENT


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_without_a_device_there_is_no_table_to_compact():
  """No CPU fallback: a table cannot be created without a GPU, so neither method can be reached."""
  from monolith_amd import entry
  from monolith_amd.multi_hash_table_ops import MultiHashTable
  cfgs = {"t": entry.make_table_config(
      [entry.CombineAsSegment(4, entry.ZerosInitializer(), entry.SgdOptimizer())])}
  with pytest.raises(_lib.MhteError) as e:
    MultiHashTable.from_configs(cfgs).compact("t")
  assert e.value.code == _lib.MHTE_UNAVAILABLE
