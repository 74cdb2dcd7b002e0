"""CPU suite: the C-ABI library builds for gfx950, loads, and exports every symbol the header
declares; without a GPU the product refuses to run (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from monolith_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")


def _declared_symbols():
  src = open(HEADER).read()
  src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
  return sorted(set(re.findall(r"\b(mhte_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_header_symbols():
  so = _lib.build_library()
  assert os.path.exists(so)
  L = C.CDLL(so)
  declared = _declared_symbols()
  assert len(declared) >= 30
  missing = [s for s in declared if not hasattr(L, s)]
  assert not missing, missing
  # ... and nothing beside them: the library's dynamic symbol table against the header
  out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r"\bmhte_\w+$", out, flags=re.M))
  assert exported == set(declared), exported ^ set(declared)
  assert L.mhte_abi_version() == _lib.ABI_VERSION


def test_signatures_known_answers():
  """One declaration of each kind against its hand-written ctypes signature."""
  vp, i32, i64, st = C.c_void_p, C.c_int32, C.c_int64, C.c_int32
  expected = {
      "mhte_lookup": (st, [vp, vp, vp, i64, vp, i64, vp]),
      "mhte_multi_table_create_from_proto":
          (st, [vp, i64, vp, C.c_uint64, C.c_float, i32, C.c_char_p, vp, i32, vp]),
      "mhte_advance_clock_for_testing": (None, [C.c_double]),
      "mhte_table_name": (C.c_char_p, [vp, i32]),
      "mhte_multi_table_find": (vp, [C.c_char_p]),
      "mhte_shard_step_info": (st, [vp, vp]),
      "mhte_multi_table_create": (st, [C.POINTER(_lib.TableConfig), i32, i32, C.c_char_p, vp]),
      "mhte_table_get_stats": (st, [vp, i32, C.POINTER(_lib.TableStats), vp]),
  }
  sigs = _lib.signatures()
  for name, sig in expected.items():
    assert sigs[name] == sig, (name, sigs[name])
  slices = [a for a in sigs["mhte_embedding_to_layout"][1] if a is C.POINTER(_lib.LayoutSlice)]
  assert len(slices) == 1


def test_signatures_cover_the_whole_header():
  declared = _declared_symbols()
  assert sorted(_lib.signatures()) == declared == _lib.EXPORTS and len(declared) >= 117
  L = _lib.lib()
  for name, (restype, argtypes) in _lib.signatures().items():
    f = getattr(L, name)
    assert f.restype == restype and list(f.argtypes) == argtypes, name


def test_unknown_declaration_is_an_error(monkeypatch):
  """A type or a declaration the binding does not know raises, naming it: never a guess, never a skip."""
  for bad in ("mhte_status mhte_new_thing(size_t n);", "mhte_status mhte_new_thing(int64_t);",
              "mhte_status mhte_new_thing(void (*cb)(int32_t));", "mhte_status mhte_new_thing(int32_t n, ...);",
              "struct x mhte_new_thing(void);"):
    monkeypatch.setattr(_lib, "_HEADER_TEXT", "const char* mhte_last_error(void);\n" + bad)
    _lib.signatures.cache_clear()
    try:
      with pytest.raises(_lib.MhteError, match="mhte_new_thing") as e:
        _lib.signatures()
      assert e.value.code == _lib.MHTE_INTERNAL
    finally:
      monkeypatch.undo()
      _lib.signatures.cache_clear()
  assert len(_lib.signatures()) == len(_lib.EXPORTS)


def test_wide_scalars_arrive_whole():
  """A bare Python int reaches an int64_t parameter as 64 bits (an untyped ctypes function passed the
  low 32: capacity 2^32 + 8 went past the range check as 8)."""
  L = _lib.lib()
  h = C.c_void_p()
  assert L.mhte_touched_key_set_create(2**32 + 8, 0, 0, C.byref(h)) == _lib.MHTE_INVALID_ARGUMENT
  assert b"capacity" in L.mhte_last_error()
  fake = C.c_void_p(0x10000)   # a handle and a device pointer the host never follows on this path
  assert L.mhte_touched_key_set_insert(fake, fake, 2**32, None, 0, None) == _lib.MHTE_INVALID_ARGUMENT
  assert b"n_max" in L.mhte_last_error()


def test_misuse_raises_at_the_call():
  L = _lib.lib()
  h = C.c_void_p()
  with pytest.raises(TypeError):
    L.mhte_touched_key_set_create(8, 0, 0)                               # one argument too few
  with pytest.raises(C.ArgumentError):
    L.mhte_touched_key_set_create(C.c_int32(8), 0, 0, C.byref(h))        # a wrapper of the wrong width
  with pytest.raises(C.ArgumentError):
    L.mhte_table_get_stats(None, 0, C.byref(_lib.TableConfig()), None)   # a pointer to the wrong struct


def _header_constants():
  """{name: value} of the header's enumerators and integer #defines."""
  src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
  consts = {k: int(v, 0) for k, v in re.findall(r"^#define\s+(MHTE_\w+)\s+(\w+)\s*$", src, flags=re.M)}
  for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S):
    for k, v in re.findall(r"(MHTE_\w+)\s*=\s*(\w+)", body):
      consts[k] = int(v, 0)
  return consts


def test_constants_match_the_header():
  consts = _header_constants()
  checked = 0
  for name, value in vars(_lib).items():
    if name.startswith(("OPT_", "INIT_")):
      assert consts["MHTE_" + name] == value, name
      checked += 1
    elif name.startswith("MHTE_") and isinstance(value, int):
      assert consts[name] == value, name
      checked += 1
  assert checked >= 12 + 13 + 4   # status codes and flags; OPT_* with its flag; INIT_*
  assert consts["MHTE_ABI_VERSION"] == _lib.ABI_VERSION


def test_struct_mirrors_have_the_c_size(tmp_path):
  names = ["segment_config", "table_config", "layout_slice", "table_stats"]
  src = tmp_path / "sizes.c"
  src.write_text('#include <stdio.h>\n#include "monolith_amd_hash_table.h"\nint main(void) {\n' +
                 "".join('  printf("%%zu\\n", sizeof(mhte_%s));\n' % n for n in names) + "  return 0;\n}\n")
  exe = str(tmp_path / "sizes")
  r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                      "-o", exe], capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  c_sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
  mirrors = [_lib.SegmentConfig, _lib.TableConfig, _lib.LayoutSlice, _lib.TableStats]
  assert [C.sizeof(m) for m in mirrors] == c_sizes == [52, 112, 36, 72]


def test_dense_mlp_launch_counts_on_the_whole_surface():
  """ABI 19: the read-only GEMM launch counters are declared in the header, listed in _lib.EXPORTS,
  exported by the library and reachable from the Python class."""
  name = "mhte_dense_mlp_launch_counts"
  assert name in _declared_symbols() and name in _lib.EXPORTS
  assert hasattr(C.CDLL(_lib.build_library()), name)
  assert re.search(r"#define\s+MHTE_ABI_VERSION\s+19\b", open(HEADER).read()) and _lib.ABI_VERSION == 19
  from monolith_amd.dense_mlp import DenseMlp
  assert callable(DenseMlp.launch_counts) and len(DenseMlp.GEMM_ROLES) == 4


def test_library_contains_gfx950_code_object():
  so = _lib.build_library()
  out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-S", so], capture_output=True,
                       text=True).stdout
  assert ".hip_fatbin" in out
  raw = open(so, "rb").read()
  assert b"gfx950" in raw


def test_header_is_plain_c():
  # the boundary must compile as C: no C++ / torch types in the signatures
  r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER], capture_output=True,
                     text=True)
  assert r.returncode == 0, r.stderr


def build_c_client(out_dir):
  """gcc (C99, no hipcc, no C++) compiles tests/c_client.c against the public header and links
  libmhte.so: the boundary is usable from plain C."""
  so = _lib.build_library()
  exe = os.path.join(str(out_dir), "mhte_c_client")
  r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                      "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                      os.path.join(ROOT, "tests", "c_client.c"), "-o", exe,
                      "-L" + os.path.dirname(so), "-lmhte", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
                      "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"],
                     capture_output=True, text=True)
  assert r.returncode == 0, r.stderr
  return exe


def test_c_client_compiles_and_links(tmp_path):
  exe = build_c_client(tmp_path)
  assert os.path.exists(exe)
  out = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
  for sym in ("mhte_multi_table_create", "mhte_lookup", "mhte_optimize", "mhte_multi_table_save",
              "mhte_multi_table_restore", "mhte_lookup_entry", "mhte_feature_stat"):
    assert sym in out, sym


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_no_gpu_means_loud_failure():
  L = _lib.lib()
  seg = _lib.SegmentConfig()
  seg.dim_size = 4
  cfg = _lib.TableConfig()
  cfg.name = b"t"
  cfg.n_segments = 1
  cfg.segments = C.pointer(seg)
  cfg.initial_capacity = 1
  h = C.c_void_p()
  st = L.mhte_multi_table_create(C.byref(cfg), 1, 0, b"x", C.byref(h))
  assert st == _lib.MHTE_UNAVAILABLE
  assert b"no CPU fallback" in L.mhte_last_error()
  from monolith_amd.multi_hash_table_ops import MultiHashTable
  from monolith_amd import entry
  cfgs = {"t": entry.make_table_config(
      [entry.CombineAsSegment(4, entry.ZerosInitializer(), entry.SgdOptimizer())])}
  with pytest.raises(_lib.MhteError):
    MultiHashTable.from_configs(cfgs)


def test_product_never_imports_oracle():
  pkg = os.path.join(ROOT, "monolith_amd")
  for dp, _, fns in os.walk(pkg):
    for fn in fns:
      if fn.endswith((".py", ".hip", ".h", ".cc")):
        txt = open(os.path.join(dp, fn)).read()
        assert "import oracle" not in txt and "from oracle" not in txt, fn
        assert "liboracle" not in txt and "libmonolith_ref" not in txt, fn
