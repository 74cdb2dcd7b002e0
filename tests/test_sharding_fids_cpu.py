"""CPU suite of the fused-layout packer (distribution_ops.sharding_sparse_fids, mhte_sharding_sparse_fids).

  * the plain-Python truth (tests/sharding_fids_truth.py) against the reference's own test procedure as
    oracle/layout.py restates it: the id generation of ``reference_forward_case`` replayed (the same
    ``random.Random`` sequence) must give that case's fid_offset and feature_offset exactly, and its nfl_offset
    apart from the final entry, which the op writes as parse_sparse_feature.cc:321 says (pinned here);
  * hand-written known answers in both ``unique`` modes;
  * the surface: header, binding, the checks the entry point makes on the host before it needs a device;
  * the plan arithmetic (csrc/mhte_sharding_plan.h) through tests/sharding_plan_host_driver.cc, once more under
    AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sharding_fids_truth as ST  # noqa: E402
from oracle import layout as OL  # noqa: E402
from monolith_amd import _lib  # noqa: E402

HEADER = os.path.join(ROOT, "include", "monolith_amd_hash_table.h")
DRIVER_SRC = os.path.join(ROOT, "tests", "sharding_plan_host_driver.cc")


def fo(*pairs):
  return np.array([(a << 32) | b for a, b in pairs], dtype=np.uint64)


def same(got, want):
  for k in ("fid_offset", "feature_offset", "nfl_offset"):
    assert got[k].dtype == want[k].dtype, k
    np.testing.assert_array_equal(got[k], want[k], err_msg=k)
  assert len(got["fid_list"]) == len(want["fid_list"])
  for i, (g, w) in enumerate(zip(got["fid_list"], want["fid_list"])):
    np.testing.assert_array_equal(g, np.array(w, dtype=np.int64), err_msg="fid_list %d" % i)
  for i, (g, w) in enumerate(zip(got["fid_list_row_splits"], want["fid_list_row_splits"])):
    np.testing.assert_array_equal(g, np.array(w, dtype=np.int64), err_msg="fid_list_row_splits %d" % i)


# ---- the truth against the reference's test procedure ------------------------------------------------------
def test_truth_reproduces_the_reference_forward_case():
  batch, num_ps, slot_count, seed, msl = 256, 5, 200, 0, 3
  case = OL.reference_forward_case(seed=seed, batch_size=batch, num_ps=num_ps, slot_count=slot_count)
  rnd = random.Random(seed)
  feature_to_table = {n: c.table for n, c in case["cfgs"].feature_configs.items()}
  features, shared = {}, set()
  for fn in sorted(feature_to_table):
    slot = int(fn.split("fc_slot_")[-1])
    if slot % 2 == 0:
      shared.add(fn)
    features[fn] = [list(set([(slot * 10000) + (i + 1) * 1000 + rnd.randint(1, 9) * 100
                              for i in range(rnd.randint(1, msl * 2))]))
                    for _ in range(1 if slot % 2 == 0 else batch)]
  got = ST.sharding_sparse_fids(feature_to_table, num_ps, False, features, shared)
  np.testing.assert_array_equal(got["fid_offset"], case["fid_offset"])
  np.testing.assert_array_equal(got["feature_offset"], case["feature_offset"])
  np.testing.assert_array_equal(got["nfl_offset"][:-1], case["nfl_offset"][:-1])
  assert got["fid_offset"].size >= 100 * batch and got["batch_size"] == batch   # (100 odd slots, a fid or more per row)
  # the final entry: the test's generator leaves the rows, the op writes the entries of feature_offset (:321)
  rows = got["feature_offset"].size - 1
  assert int(case["nfl_offset"][-1]) == rows and int(got["nfl_offset"][-1]) == rows + 1 == got["feature_offset"].size


# ---- known answers ---------------------------------------------------------------------------------------
TABLES_3 = {"a": "t0", "b": "t0", "c": "t1"}
ROWS_3 = {"a": [[2, 4, 2], [4, 3]], "b": [[2], [5, 5]], "c": [[], [7]]}


def test_known_answer_three_features_two_tables():
  common = {"feature_offset": np.array([0, 3, 5, 6, 8, 8, 9], dtype=np.int32),
            "nfl_offset": np.array([0, 2, 4, 7], dtype=np.uint32)}
  same(ST.sharding_sparse_fids(TABLES_3, 2, False, ROWS_3),
       dict(common, fid_offset=fo((0, 0), (0, 1), (0, 2), (0, 3), (2, 0), (1, 0), (3, 0), (3, 1), (5, 0)),
            fid_list=[[2, 4, 2, 4, 2], [3, 5, 5], [], [7]],
            fid_list_row_splits=[[0, 4, 5], [0, 1, 3], [0, 0], [0, 1]]))
  # unique: per feature — id 2 of feature b is not feature a's id 2, though they share a table and a shard
  same(ST.sharding_sparse_fids(TABLES_3, 2, True, ROWS_3),
       dict(common, fid_offset=fo((0, 0), (0, 1), (0, 0), (0, 1), (2, 0), (1, 0), (3, 0), (3, 0), (5, 0)),
            fid_list=[[2, 4, 2], [3, 5], [], [7]],
            fid_list_row_splits=[[0, 2, 3], [0, 1, 2], [0, 0], [0, 1]]))


def test_known_answer_shared_feature_sets_bit_31():
  for unique in (False, True):
    same(ST.sharding_sparse_fids({"u": "t0", "v": "t0"}, 2, unique, {"u": [[1, 2]], "v": [[3], [4]]}, {"u"}),
         {"fid_offset": fo((2, 0), (0, 0), (3, 0), (1, 0)), "feature_offset": np.array([0, 2, 3, 4], dtype=np.int32),
          "nfl_offset": np.array([0x80000000, 1, 4], dtype=np.uint32),
          "fid_list": [[2, 4], [1, 3]], "fid_list_row_splits": [[0, 1, 2], [0, 1, 2]]})


def test_known_answer_bit_63_takes_the_unsigned_remainder():
  # uint64(-1) % 3 == 0 and uint64(-2) % 3 == 2; floormod would say 2 and 1
  assert ((1 << 64) - 1) % 3 == 0 and ((1 << 64) - 2) % 3 == 2 and (-1) % 3 == 2 and (-2) % 3 == 1
  for unique in (False, True):
    same(ST.sharding_sparse_fids({"x": "t"}, 3, unique, {"x": [[-1, -2]]}),
         {"fid_offset": fo((0, 0), (2, 0)), "feature_offset": np.array([0, 2], dtype=np.int32),
          "nfl_offset": np.array([0, 2], dtype=np.uint32), "fid_list": [[-1], [], [-2]],
          "fid_list_row_splits": [[0, 1], [0, 0], [0, 1]]})


# ---- the surface -----------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
  name = "mhte_sharding_sparse_fids"
  assert name in open(HEADER).read() and name in _lib.EXPORTS
  assert hasattr(C.CDLL(_lib.build_library()), name)
  i32, i64, p = C.c_int32, C.c_int64, C.c_void_p
  assert _lib.signatures()[name] == (i32, [C.POINTER(_lib.ShardFeature), i32, p, i32, i32, i32, p, p, p, p, p, p, p,
                                           p, p])
  assert C.sizeof(_lib.ShardFeature) == 40
  from monolith_amd import distribution_ops as D
  import monolith_amd
  assert callable(D.sharding_sparse_fids) and callable(D.sharding_sparse_fids_plan)
  assert monolith_amd.PartitionedHashTable.__module__ == "monolith_amd.partitioned_hash_table"


def _raw(feats, tfc, ps_num):
  """The entry point on pointers the host never follows: every refusal here comes before a device is needed."""
  fake = C.c_void_p(0x10000)
  arr = (_lib.ShardFeature * len(feats))()
  for x, (n_ids, n_rows, shared, t, j) in zip(arr, feats):
    x.values, x.row_splits, x.n_ids, x.n_rows, x.shared = 0x10000, 0x20000, n_ids, n_rows, shared
    x.table_index, x.feature_in_table_index = t, j
  L = _lib.lib()
  st = L.mhte_sharding_sparse_fids(arr, len(feats), (C.c_int32 * len(tfc))(*tfc), len(tfc), ps_num, 1, fake, fake, fake,
                                   fake, fake, fake, fake, None, None)
  return st, L.mhte_last_error().decode()


def test_host_checks_refuse_before_any_device_call():
  ok = [(3, 2, 0, 0, 0), (1, 2, 0, 0, 1)]
  for ps in (0, -1, 1025):
    st, msg = _raw(ok, [2], ps)
    assert st == _lib.MHTE_INVALID_ARGUMENT and "ps_num must be in [1, 1024]" in msg
  st, msg = _raw([(2 ** 32, 2, 0, 0, 0), (1, 2, 0, 0, 1)], [2], 2)
  assert st == _lib.MHTE_INVALID_ARGUMENT and "more than 2^32 - 1 ids in a (feature, shard)" in msg
  st, msg = _raw([(2 ** 31, 2, 0, 0, 0), (1, 2, 0, 0, 1)], [2], 2)
  assert st == _lib.MHTE_INVALID_ARGUMENT and "below 2^31 - 1" in msg
  for feats, tfc, word in (([(3, 2, 0, 1, 0), (1, 2, 0, 0, 1)], [2], "table_index"),
                           ([(3, 2, 0, 0, 2), (1, 2, 0, 0, 1)], [2], "feature_in_table_index"),
                           ([(3, 2, 0, 0, 1), (1, 2, 0, 0, 1)], [2], "another feature"),
                           ([(3, 2, 1, 0, 0), (1, 2, 0, 0, 1)], [2], "a shared feature has one row"),
                           ([(3, 0, 0, 0, 0), (1, 2, 0, 0, 1)], [2], "ids without rows"),
                           (ok, [1], "add up"), (ok, [2, 0], "table 1")):
    st, msg = _raw(feats, tfc, 2)
    assert st == _lib.MHTE_INVALID_ARGUMENT and word in msg, (word, msg)


# ---- the plan arithmetic, stand-alone ----------------------------------------------------------------------
def _compile(exe, extra=()):
  subprocess.check_call(["g++", "-O2", "-std=c++17", *extra, "-I" + os.path.join(ROOT, "monolith_amd", "csrc"),
                         DRIVER_SRC, "-o", exe])
  return exe


# (ps_num, tables' feature counts, features as n_ids:n_rows:shared:table:index_in_table)
PLANS = [(2, [2, 1], ["5:2:0:0:0", "3:2:0:0:1", "1:2:0:1:0"]),
         (3, [1, 2], ["0:0:0:1:1", "4:1:1:0:0", "7:5:0:1:0"]),
         (1024, [1], ["9:3:0:0:0"])]


def _plan_truth(ps, tfc, feats):
  first = np.concatenate([[0], np.cumsum(tfc)])
  rows = [[int(v) for v in f.split(":")] for f in feats]
  lines = ["%d %d %d %d" % (sum(r[0] for r in rows), sum(r[1] for r in rows), len(rows) * ps, len(tfc) * ps)]
  ids = rws = 0
  for n_ids, n_rows, _, t, j in rows:
    lines.append("%d %d %d %d %d %d" % (ids, rws, first[t] + j, first[t] * ps, tfc[t], j))
    ids, rws = ids + n_ids, rws + n_rows
  return lines


def test_plan_driver_equals_the_restatement(tmp_path):
  exe = _compile(str(tmp_path / "sharding_plan_host"))
  for ps, tfc, feats in PLANS:
    out = subprocess.run([exe, str(ps), ",".join(map(str, tfc))] + feats, capture_output=True, text=True, check=True)
    assert out.stdout.strip().split("\n") == _plan_truth(ps, tfc, feats)
  out = subprocess.run([exe, "0", "1", "1:1:0:0:0"], capture_output=True, text=True, check=True).stdout
  assert out.startswith("refused: ps_num")
  out = subprocess.run([exe, "2", "1", "%d:1:0:0:0" % 2 ** 32], capture_output=True, text=True, check=True).stdout
  assert out.startswith("refused: feature 0: more than 2^32 - 1 ids")


def test_plan_driver_is_clean_under_asan_and_ubsan(tmp_path):
  flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
  probe = subprocess.run(["g++", "-x", "c++", "-", *flags, "-o", str(tmp_path / "probe")], input="int main() {}\n",
                         capture_output=True, text=True)
  if probe.returncode != 0:
    pytest.skip("the sanitizer runtimes are not installed: " + probe.stderr.strip().split("\n")[-1])
  exe = _compile(str(tmp_path / "sharding_plan_host_san"), flags)
  many = ["%d:4:0:%d:%d" % (i % 7, i % 3, i // 3) for i in range(69)]
  for args in ([(str(ps), ",".join(map(str, tfc))) + tuple(feats) for ps, tfc, feats in PLANS] +
               [("8", "23,23,23") + tuple(many), ("0", "1", "1:1:0:0:0"), ("2", "1", "1:1:0:0:5"),
                ("2", "2", "1:1:0:0:0", "1:1:0:0:0"), ("2", "1", "%d:1:0:0:0" % 2 ** 32)]):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args[:3], r.stderr[-2000:])
