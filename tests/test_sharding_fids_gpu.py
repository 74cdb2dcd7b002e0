"""GPU suite of the fused-layout packer (distribution_ops.sharding_sparse_fids, csrc/mhte_sharding_kernels.h)
against the plain-Python restatement of the reference op (tests/sharding_fids_truth.py): every output bit for
bit — fid_offset, feature_offset, nfl_offset, every (table, shard) fid list with its row_splits, the device
tables of the plan variant — at the shapes where the launch sequence takes another path: one row, one to eight
and 1024 shards, an empty feature, a one-feature table, an empty shard, a shared list, more features than a
wavefront has lanes, ranks that cross the tiles of the stable sort, buffers that are 8- but not 16-byte aligned,
and every refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sharding_fids_truth as ST  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402

pytestmark = pytest.mark.gpu

TABLES_3 = {"fa": "t0", "fb": "t0", "fc": "t1"}


def cfgs_of(feature_to_table):
  return D.FeatureConfigs({n: D.FeatureConfig(t, D.PoolingType.SUM, [4]) for n, t in feature_to_table.items()}, {})


def random_rows(rng, batch, pool, max_len=4):
  return [[int(x) for x in pool[rng.integers(0, pool.size, size=rng.integers(0, max_len + 1))]] for _ in range(batch)]


def pool_of(rng, n):
  """ids with the sign bit set among them: the shard is the UNSIGNED remainder"""
  return np.concatenate([rng.integers(-2 ** 63, -2 ** 62, size=max(n // 4, 1)),
                         rng.integers(0, 2 ** 62, size=n - max(n // 4, 1))]).astype(np.int64)


def to_device(rows, shared, device_splits=False, offset=False):
  """-> what sharding_sparse_fids takes for one feature; ``offset``: views 8 bytes into their buffers"""
  flat = np.array([x for r in rows for x in r], dtype=np.int64)
  splits = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
  if offset:
    v = torch.empty(flat.size + 1, dtype=torch.int64, device="cuda")[1:]
    v.copy_(torch.from_numpy(flat))
    s = torch.empty(splits.size + 1, dtype=torch.int64, device="cuda")[1:]
    s.copy_(torch.from_numpy(splits))
    assert v.data_ptr() % 16 == 8 and s.data_ptr() % 16 == 8
    return (v, s)
  v = torch.from_numpy(flat).cuda()
  if shared and not device_splits:
    return v
  return (v, torch.from_numpy(splits).cuda() if device_splits else splits)


def np_of(t):
  return t.cpu().numpy()


def check_against_truth(feature_to_table, ps, unique, feats, shared=(), **form):
  want = ST.sharding_sparse_fids(feature_to_table, ps, unique, feats, set(shared))
  dev = {n: to_device(rows, n in shared, **form) for n, rows in feats.items()}
  got = D.sharding_sparse_fids(dev, cfgs_of(feature_to_table), ps, unique=unique, shared_features=shared,
                               batch_size=want["batch_size"] if all(n in shared for n in feats) else None)
  what = "ps=%d unique=%s" % (ps, unique)
  assert got.fid_offset.dtype == torch.uint64 and got.nfl_offset.dtype == torch.uint32
  assert got.feature_offset.dtype == torch.int32
  np.testing.assert_array_equal(np_of(got.fid_offset), want["fid_offset"], err_msg=what)
  np.testing.assert_array_equal(np_of(got.feature_offset), want["feature_offset"], err_msg=what)
  np.testing.assert_array_equal(np_of(got.nfl_offset), want["nfl_offset"], err_msg=what)
  assert got.batch_size == want["batch_size"]
  assert len(got.fid_list) == len(want["fid_list"]) == len(got.fid_list_row_splits)
  for i, (ids, splits) in enumerate(zip(want["fid_list"], want["fid_list_row_splits"])):
    np.testing.assert_array_equal(np_of(got.fid_list[i]), ids, err_msg="%s fid_list %d" % (what, i))
    assert got.fid_list_row_splits[i].dtype == np.int64
    np.testing.assert_array_equal(got.fid_list_row_splits[i], splits, err_msg="%s row_splits %d" % (what, i))
  # the device tables of the plan variant say the same
  np.testing.assert_array_equal(np_of(got.row_splits_flat), np.concatenate(want["fid_list_row_splits"]))
  bounds, flat = np_of(got.list_bounds), np_of(got.fid_list_flat)
  for i, ids in enumerate(want["fid_list"]):
    np.testing.assert_array_equal(flat[bounds[i, 0]:bounds[i, 0] + bounds[i, 1]], ids)
  # a PS's ragged ids: its lists, table after table
  n_tables = len(want["fid_list"]) // ps
  for s in range(ps):
    r = got.ps_ragged(s)
    mine = [want["fid_list"][t * ps + s] for t in range(n_tables)]
    np.testing.assert_array_equal(np_of(r.values), np.concatenate(mine))
    np.testing.assert_array_equal(r.row_splits, np.concatenate([[0], np.cumsum([m.size for m in mine])]))
  sizes = got.pre_output_sizes()
  np.testing.assert_array_equal(sizes, np.concatenate([np.diff(s) for s in want["fid_list_row_splits"]]))
  assert int(np_of(got.key_start)[-1]) == 0 and int(np_of(got.key_start)[-2]) == sum(m.size for m in want["fid_list"])
  return got, want


def three_features(seed, batch, n_pool=12):
  rng = np.random.default_rng(seed)
  pool = pool_of(rng, n_pool)
  return {n: random_rows(rng, batch, pool) for n in TABLES_3}


@pytest.mark.parametrize("unique", [False, True])
def test_batch_of_one(unique):
  check_against_truth(TABLES_3, 2, unique, three_features(1, 1))


@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("ps", [1, 2, 3, 8])
def test_batch_5_three_features_two_tables(ps, unique):
  got, want = check_against_truth(TABLES_3, ps, unique, three_features(2, 5))
  if unique:   # the pool is smaller than the batch's ids: the dedup had something to do
    assert sum(m.size for m in want["fid_list"]) < want["fid_offset"].size


@pytest.mark.parametrize("unique", [False, True])
def test_empty_feature_single_feature_table_and_empty_shard(unique):
  feats = three_features(3, 5)
  feats["fb"] = [[] for _ in range(5)]                       # empty in every row
  check_against_truth(TABLES_3, 3, unique, feats)             # ("fc" is alone in its table)
  even = {n: [[x & ~1 for x in r] for r in rows] for n, rows in three_features(4, 5).items()}
  got, want = check_against_truth(TABLES_3, 2, unique, even)  # shard 1 receives nothing
  assert all(want["fid_list"][t * 2 + 1].size == 0 for t in range(2)) and want["fid_offset"].size > 0
  check_against_truth(TABLES_3, 2, unique, {n: [[] for _ in range(5)] for n in TABLES_3})   # no id at all
  only = dict(three_features(5, 5))
  del only["fa"]                                              # a configured feature the batch does not carry
  check_against_truth(TABLES_3, 2, unique, only)


@pytest.mark.parametrize("unique", [False, True])
def test_shared_feature(unique):
  feats = three_features(6, 5)
  feats["fb"] = [[7, 7, 9, 1 << 40, 7]]
  got, want = check_against_truth(TABLES_3, 3, unique, feats, shared=("fb",))
  assert int(want["nfl_offset"][1]) >> 31 == 1
  check_against_truth(TABLES_3, 3, unique, feats, shared=("fb",), device_splits=True)
  check_against_truth({"s": "t"}, 2, unique, {"s": [[4, 5, 4]]}, shared=("s",))   # every feature shared


@pytest.mark.parametrize("unique", [False, True])
def test_70_features(unique):
  rng = np.random.default_rng(7)
  tables = {"f%02d" % i: "t%d" % (i % 3) for i in range(70)}
  pool = pool_of(rng, 20)     # one pool for all: features of a table share ids, the dedup is per feature
  feats = {n: random_rows(rng, 3, pool, max_len=3) for n in tables}
  check_against_truth(tables, 4, unique, feats)


@pytest.mark.parametrize("unique", [False, True])
def test_ranks_cross_tiles_and_workgroups(unique):
  rng = np.random.default_rng(8)
  n = 3 * D.SHARDING_TILE + 1
  pool = pool_of(rng, 50)
  ids = pool[rng.integers(0, pool.size, size=n)]
  cuts = np.sort(rng.integers(0, n + 1, size=6))
  rows = [[int(x) for x in part] for part in np.split(ids, cuts)]
  got, want = check_against_truth({"big": "t0", "small": "t0"}, 2, unique, {"big": rows, "small": [[int(pool[0])]] * 7})
  ranks = want["fid_offset"] & np.uint64(0xffffffff)
  # (without dedup a shard's ranks run past a tile; with it the 50 ids of the pool are all that is placed)
  assert int(ranks.max()) >= (10 if unique else D.SHARDING_TILE)
  if unique:
    assert sum(m.size for m in want["fid_list"]) == 51


@pytest.mark.parametrize("unique", [False, True])
def test_ps_num_1024(unique):
  rng = np.random.default_rng(9)
  pool = pool_of(rng, 300)
  feats = {n: random_rows(rng, 5, pool, max_len=40) for n in TABLES_3}
  check_against_truth(TABLES_3, 1024, unique, feats)


@pytest.mark.parametrize("unique", [False, True])
def test_inputs_8_bytes_into_their_buffers(unique):
  check_against_truth(TABLES_3, 3, unique, three_features(10, 5), offset=True)


def _raw_outputs(feats_dev, ps, unique, offset):
  """mhte_sharding_sparse_fids on output buffers this test owns: ``offset`` puts every one of them 8 bytes into
  its allocation; a guard word behind each must keep its value."""
  names = sorted(TABLES_3)
  arr = (_lib.ShardFeature * 3)()
  n = rows = 0
  for x, name, (t, j) in zip(arr, names, [(0, 0), (0, 1), (1, 0)]):
    v, s = feats_dev[name]
    x.values, x.row_splits, x.n_ids, x.n_rows, x.shared = v.data_ptr(), s.data_ptr(), v.numel(), s.numel() - 1, 0
    x.table_index, x.feature_in_table_index = t, j
    n, rows = n + v.numel(), rows + s.numel() - 1
  n_pre, n_lists = 3 * ps, 2 * ps
  lens = {"fid_offset": (n, torch.int64), "feature_offset": (rows + 1, torch.int32), "nfl_offset": (4, torch.int32),
          "fid_list": (n, torch.int64), "key_start": (n_pre + 2, torch.int64),
          "row_splits_flat": (n_pre + n_lists, torch.int64), "list_bounds": (2 * n_lists, torch.int64)}
  bufs, outs = {}, {}
  for k, (m, dt) in lens.items():
    lead = (8 // torch.empty(0, dtype=dt).element_size()) if offset else 0
    bufs[k] = torch.full((lead + m + 2,), -77, dtype=dt, device="cuda")
    outs[k] = bufs[k][lead:lead + m]
    assert outs[k].data_ptr() % 16 == (8 if offset else 0)
  host = np.empty(n_pre + 2, dtype=np.int64)
  D.check(_lib.lib().mhte_sharding_sparse_fids(
      arr, 3, (C.c_int32 * 2)(2, 1), 2, ps, int(unique), *[D.vp(outs[k]) for k in lens],
      host.ctypes.data_as(C.c_void_p), D._stream()))
  for k, (m, dt) in lens.items():
    lead = bufs[k].numel() - m - 2
    assert (bufs[k][:lead] == -77).all() and (bufs[k][lead + m:] == -77).all(), k
  placed = int(host[n_pre])
  res = {k: np_of(v) for k, v in outs.items()}
  res["fid_list"] = res["fid_list"][:placed]
  return res, host


@pytest.mark.parametrize("unique", [False, True])
def test_outputs_8_bytes_into_their_buffers_and_two_runs(unique):
  feats = three_features(11, 5, n_pool=9)
  dev = {n: to_device(rows, False, offset=True) for n, rows in feats.items()}
  aligned, host_a = _raw_outputs(dev, 3, unique, offset=False)
  shifted, host_b = _raw_outputs(dev, 3, unique, offset=True)
  again, host_c = _raw_outputs(dev, 3, unique, offset=True)
  want = ST.sharding_sparse_fids(TABLES_3, 3, unique, feats)
  for res in (aligned, shifted, again):
    np.testing.assert_array_equal(res["fid_offset"].view(np.uint64), want["fid_offset"])
    np.testing.assert_array_equal(res["feature_offset"], want["feature_offset"])
    np.testing.assert_array_equal(res["nfl_offset"].view(np.uint32), want["nfl_offset"])
    np.testing.assert_array_equal(res["row_splits_flat"], np.concatenate(want["fid_list_row_splits"]))
  for k in aligned:
    np.testing.assert_array_equal(aligned[k], shifted[k], err_msg=k)
    np.testing.assert_array_equal(shifted[k], again[k], err_msg=k)
  np.testing.assert_array_equal(host_a, host_b)
  np.testing.assert_array_equal(host_b, host_c)


@pytest.mark.parametrize("unique", [False, True])
def test_two_runs_of_one_input_are_identical(unique):
  rng = np.random.default_rng(12)
  pool = pool_of(rng, 40)
  n = 2 * D.SHARDING_TILE + 77
  feats = {"fa": (torch.from_numpy(pool[rng.integers(0, 40, size=n)]).cuda(), np.array([0, 5, n], dtype=np.int64)),
           "fb": (torch.from_numpy(pool[rng.integers(0, 40, size=900)]).cuda(), np.array([0, 900, 900], dtype=np.int64))}
  cfgs = cfgs_of(TABLES_3)
  runs = [D.sharding_sparse_fids(feats, cfgs, 8, unique=unique) for _ in range(2)]
  plan = D.sharding_sparse_fids_plan(feats, cfgs, 8, unique=unique)
  assert plan.fid_list is None and plan.key_start_host is None and plan.fid_list_row_splits is None
  placed = int(runs[0].key_start_host[-2])
  for other in (runs[1], plan):
    for k in ("fid_offset", "feature_offset", "nfl_offset", "key_start", "row_splits_flat", "list_bounds"):
      np.testing.assert_array_equal(np_of(getattr(runs[0], k)), np_of(getattr(other, k)), err_msg=k)
    np.testing.assert_array_equal(np_of(runs[0].fid_list_flat)[:placed], np_of(other.fid_list_flat)[:placed])
  np.testing.assert_array_equal(runs[0].key_start_host, np_of(plan.key_start))


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals():
  cfgs = cfgs_of(TABLES_3)
  ids = torch.arange(6, dtype=torch.int64, device="cuda")
  good = {"fa": (ids, np.array([0, 2, 6]))}
  for ps in (0, -3, 1025):
    with pytest.raises(_lib.InvalidArgumentError, match=r"ps_num must be in \[1, 1024\]"):
      D.sharding_sparse_fids(good, cfgs, ps)
  with pytest.raises(TypeError, match="ps_num"):
    D.sharding_sparse_fids(good, cfgs, 2.0)
  with pytest.raises(TypeError, match="int64"):
    D.sharding_sparse_fids({"fa": (ids.to(torch.int32), np.array([0, 2, 6]))}, cfgs, 2)
  with pytest.raises(TypeError, match="on the GPU"):
    D.sharding_sparse_fids({"fa": (ids.cpu(), np.array([0, 2, 6]))}, cfgs, 2)
  with pytest.raises(ValueError, match="contiguous"):
    D.sharding_sparse_fids({"fa": (torch.arange(12, dtype=torch.int64, device="cuda")[::2], np.array([0, 2, 6]))},
                           cfgs, 2)
  for bad in ([0, 4, 2, 6], [0, 2, 5], [1, 2, 6], [0, 2, 7]):
    with pytest.raises(_lib.InvalidArgumentError, match="The input ragged tensor is invalid."):
      D.sharding_sparse_fids({"fa": (ids, np.array(bad))}, cfgs, 2)
    with pytest.raises(_lib.InvalidArgumentError, match="The input ragged tensor is invalid."):   # ... on the device
      D.sharding_sparse_fids({"fa": (ids, torch.tensor(bad, dtype=torch.int64, device="cuda"))}, cfgs, 2)
    plan = D.sharding_sparse_fids_plan({"fa": (ids, torch.tensor(bad, dtype=torch.int64, device="cuda"))}, cfgs, 2)
    assert int(np_of(plan.key_start)[-1]) == 1
  with pytest.raises(_lib.InvalidArgumentError, match="no feature config for zz"):
    D.sharding_sparse_fids({"fa": (ids, np.array([0, 2, 6])), "zz": (ids, np.array([0, 2, 6]))}, cfgs, 2)
  with pytest.raises(ValueError, match="rows"):
    D.sharding_sparse_fids({"fa": (ids, np.array([0, 2, 6])), "fb": (ids, np.array([0, 6]))}, cfgs, 2)
  with pytest.raises(ValueError, match="one row"):
    D.sharding_sparse_fids({"fa": (ids, np.array([0, 2, 6]))}, cfgs, 2, shared_features=("fa",))
  # more than 2^32 - 1 ids in a (feature, shard): refused on the host, from the sizes alone
  arr = (_lib.ShardFeature * 1)()
  arr[0].values, arr[0].row_splits, arr[0].n_ids, arr[0].n_rows = ids.data_ptr(), ids.data_ptr(), 2 ** 32, 1
  fake = D.vp(ids)
  st = _lib.lib().mhte_sharding_sparse_fids(arr, 1, (C.c_int32 * 1)(1), 1, 2, 1, fake, fake, fake, fake, fake, fake, fake,
                                            None, D._stream())
  assert st == _lib.MHTE_INVALID_ARGUMENT
  assert b"more than 2^32 - 1 ids in a (feature, shard)" in _lib.lib().mhte_last_error()
  # and the good call still works afterwards
  assert D.sharding_sparse_fids(good, cfgs, 2).batch_size == 2
