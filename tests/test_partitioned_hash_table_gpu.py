"""GPU suite of PartitionedHashTable (monolith_amd/partitioned_hash_table.py): batch 16, three parameter
servers, twelve feature slots in the shape of the reference's layout test (oracle.layout._test_configs: SUM, MEAN
and FIRSTN pooling; bias = ADDN, vec = CONCAT, ffm1 = STACK, ffm2 / firstN = NONE; the even slots shared lists)
over two tables, SGD (dim 13) and Adagrad (dim 21).  Ids carry the slot in the high bits; a slot draws from ten
ids, so rows repeat ids and batch rows share them.

  lookup            against oracle.layout.pooling applied to the ORIGINAL id lists over rows read from the CPU
                    oracle's tables (oracle.Table), preloaded with the same rows — bit for bit, the bar
                    tests/test_layout_forms_gpu.py sets for the forward.  (A MEAN list has 1, 2 or 4 ids: the op
                    scales every row by 1 / n before adding, pooling() divides the sum; with n a power of two the
                    two are the same floats.)
  apply_gradients   then lookup, against oracle.layout.layout_grad_model over the packer's truth
                    (tests/sharding_fids_truth.py) followed by the oracle tables' update, in both ``unique``
                    modes, at the layout gradient's tolerance (tests/test_boundary_gpu.py: rtol 1e-5, atol 1e-5).
  row placement     PS i holds exactly the ids with id % num_ps == i: by key set and as the sorted ids themselves."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle as O  # noqa: E402
import sharding_fids_truth as ST  # noqa: E402
from oracle import layout as OL  # noqa: E402
from monolith_amd import PartitionedHashTable, entry  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, NUM_PS, MSL = 16, 3, 3
SLOTS, SPLIT = range(1, 13), (4, 8)
DIMS = {"table_one": 13, "table_two": 21}
LR = {"table_one": 0.5, "table_two": 0.05}
INIT_ACC = 0.1
_seq = itertools.count()


def name_of(slot):
  return "fc_slot_%02d" % slot


def oracle_cfgs():
  """oracle.layout._test_configs with one dim per table: the FIRSTN slots live in table_two"""
  feats, bias, vec, ffm1, ffm2, firstn = {}, [], [], [], [], []
  for slot in SLOTS:
    fn = name_of(slot)
    if slot >= SPLIT[1]:
      feats[fn] = OL.FeatureConfig("table_two", OL.FIRSTN, [1, 4, 16], MSL)
      firstn.append(OL.SliceConfig(fn, 1, 21))
      continue
    if slot < SPLIT[0]:
      feats[fn] = OL.FeatureConfig("table_one", OL.SUM, [1, 4, 8], 0)
      ffm1.append(OL.SliceConfig(fn, 5, 13))
    else:
      feats[fn] = OL.FeatureConfig("table_two", OL.MEAN, [1, 4, 16], 0)
      ffm2.append(OL.SliceConfig(fn, 5, 21))
    bias.append(OL.SliceConfig(fn, 0, 1))
    vec.append(OL.SliceConfig(fn, 1, 5))
  outs = {"bias": OL.infer_shape(bias, OL.ADDN), "vec": OL.infer_shape(vec, OL.CONCAT),
          "ffm1": OL.infer_shape(ffm1, OL.STACK), "ffm2": OL.infer_shape(ffm2, OL.NONE),
          "firstN": OL.infer_shape(firstn, OL.NONE, MSL)}
  return OL.FeatureConfigs(feats, outs)


def product_cfgs(oc):
  feats = {n: D.FeatureConfig(f.table, f.pooling_type, f.slice_dims, f.max_sequence_length)
           for n, f in oc.feature_configs.items()}
  outs = {n: D.OutConfig([D.SliceConfig(s.feature_name, s.start, s.end) for s in o.slice_configs], o.out_type, o.shape)
          for n, o in oc.out_configs.items()}
  return D.FeatureConfigs(feats, outs)


def table_configs():
  seg = lambda dim, opt: entry.make_table_config(   # noqa: E731
      [entry.CombineAsSegment(dim, entry.ZerosInitializer(), opt)], entry.CuckooHashTableConfig())
  return {"table_one": seg(13, entry.SgdOptimizer(LR["table_one"])),
          "table_two": seg(21, entry.AdagradOptimizer(LR["table_two"], INIT_ACC))}


def oracle_tables():
  return {"table_one": O.Table(O.segment(13, O.OPT_SGD), 1),
          "table_two": O.Table(O.segment(21, O.OPT_ADAGRAD, p=(INIT_ACC, 0.0)), 1)}


def the_batch():
  """-> (cfgs, features {name: rows}, shared names, pools {table: ids})"""
  rng = np.random.default_rng(5)
  cfgs = oracle_cfgs()
  feats, shared, pools = {}, set(), {t: [] for t in DIMS}
  for slot in SLOTS:
    fn = name_of(slot)
    fc = cfgs.feature_configs[fn]
    pool = (slot << 48) + rng.choice(np.arange(1, 1000), size=10, replace=False).astype(np.int64)
    pools[fc.table].append(pool)
    lengths = [1, 2, 4] if fc.pooling_type == OL.MEAN else [0, 1, 2, 3, 5]
    rows = [[int(x) for x in pool[rng.integers(0, 10, size=rng.choice(lengths))]]
            for _ in range(1 if slot % 2 == 0 else BATCH)]
    if slot % 2 == 0:
      shared.add(fn)
      if not rows[0]:
        rows[0] = [int(pool[0]), int(pool[0])]
    feats[fn] = rows
  return cfgs, feats, shared, {t: np.concatenate(p) for t, p in pools.items()}


def device_features(feats, shared):
  out = {}
  for n, rows in feats.items():
    flat = torch.tensor([x for r in rows for x in r], dtype=torch.int64).cuda()
    out[n] = flat if n in shared else (flat, np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64))
  return out


def expected_layouts(cfgs, feats, tables):
  """The truth procedure of the reference's test (fused_embedding_to_layout_test.py:430-530) over the original
  id lists: per feature ``pooling()`` of the rows the oracle tables hold; a shared list serves every batch row."""
  outs = []
  for ln in sorted(cfgs.out_configs):
    oc = cfgs.out_configs[ln]
    tensors = [np.zeros([BATCH] + sh[1:], dtype=np.float32) for sh in oc.shape]
    off = 0
    for i, sc in enumerate(oc.slice_configs):
      fc = cfgs.feature_configs[sc.feature_name]
      dim = sc.end - sc.start
      ts = tensors[0] if len(oc.shape) == 1 else tensors[i]
      rows = feats[sc.feature_name]
      for b in range(BATCH):
        ids = rows[b] if b < len(rows) else rows[0]
        if not ids:
          continue
        emb = tables[fc.table].lookup(np.array(ids, dtype=np.int64))[0]
        val = OL.pooling(fc.pooling_type, [emb[q, sc.start:sc.end].copy() for q in range(len(ids))],
                         fc.max_sequence_length)
        if oc.out_type == OL.CONCAT:
          ts[b, off:off + dim] = val
        elif oc.out_type == OL.STACK:
          ts[b, i, :] = val
        elif oc.out_type == OL.ADDN:
          ts[b, :] += val
        else:
          ts[b] = val
      if oc.out_type == OL.CONCAT:
        off += dim
    outs += tensors
  return outs


def preload(pht, tables, pools):
  rng = np.random.default_rng(6)
  for t, ids in pools.items():
    rows = rng.standard_normal((ids.size, DIMS[t])).astype(np.float32)
    tables[t].assign(ids, rows)
    for i, ps in enumerate(pht.tables):
      m = ids % NUM_PS == i
      ps.assign({t: (torch.from_numpy(ids[m]).cuda(), torch.from_numpy(rows[m]).cuda())})


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def case():
  cfgs, feats, shared, pools = the_batch()
  return {"cfgs": cfgs, "feats": feats, "shared": shared, "pools": pools, "dev": device_features(feats, shared)}


def make(case, unique=True):
  return PartitionedHashTable(NUM_PS, table_configs(), product_cfgs(case["cfgs"]),
                              name_suffix="pht_test_%d" % next(_seq), unique=unique)


@pytest.mark.parametrize("unique", [True, False])
def test_lookup_equals_pooling_over_the_original_lists(case, unique):
  pht, tables = make(case, unique), oracle_tables()
  try:
    assert pht.unique == unique and pht.num_ps == NUM_PS and len(pht.tables) == NUM_PS
    preload(pht, tables, case["pools"])
    got = pht.lookup(case["dev"], shared_features=case["shared"])
    want = expected_layouts(case["cfgs"], case["feats"], tables)
    assert len(got) == len(want) == 3 + 4 + 5      # bias, vec, ffm1, 4 x ffm2, 5 x firstN
    for k, (g, w) in enumerate(zip(got, want)):
      assert tuple(g.shape) == w.shape and np.abs(w).max() > 0, k
      np.testing.assert_array_equal(bits(g.cpu().numpy()), bits(w), err_msg="tensor %d" % k)
  finally:
    pht.close()


@pytest.mark.parametrize("unique", [True, False])
def test_apply_gradients_then_lookup(case, unique):
  cfgs, feats, shared = case["cfgs"], case["feats"], case["shared"]
  pht, tables = make(case, unique), oracle_tables()
  try:
    preload(pht, tables, case["pools"])
    first = pht.lookup(case["dev"], shared_features=shared)
    rng = np.random.default_rng(7)
    tg = [rng.standard_normal(tuple(t.shape)).astype(np.float32) for t in first]
    assert pht.apply_gradients([torch.from_numpy(t).cuda() for t in tg], global_step=3, req_time=1000) is pht
    # ---- the model: the packer's truth, the layout gradient over it, the oracle tables' update
    f2t = {n: f.table for n, f in cfgs.feature_configs.items()}
    truth = ST.sharding_sparse_fids(f2t, NUM_PS, unique, feats, shared)
    _, table_names, conf, tinfo = ST.feature_index(f2t, NUM_PS)
    embs, ids_of = [], []
    for t, tn in enumerate(table_names):
      for s in range(NUM_PS):
        lst, rs = truth["fid_list"][t * NUM_PS + s], truth["fid_list_row_splits"][t * NUM_PS + s]
        for j in range(len(rs) - 1):
          ids = lst[rs[j]:rs[j + 1]]
          ids_of.append((tn, ids))
          embs.append(tables[tn].lookup(ids)[0].reshape(ids.size, DIMS[tn]))
    grads = OL.layout_grad_model(embs, truth["fid_offset"], truth["feature_offset"], truth["nfl_offset"], BATCH, cfgs,
                                 tg, acc_dtype=np.float32)
    if not unique:   # duplicates reach the table as separate rows
      assert any(np.unique(ids).size < ids.size for _, ids in ids_of)
    for (tn, ids), g in zip(ids_of, grads):
      if ids.size:
        tables[tn].optimize(ids, g, [LR[tn]], 1000, 3)
    want = expected_layouts(cfgs, feats, tables)
    got = pht.lookup(case["dev"], shared_features=shared)
    moved = 0
    for k, (g, w, f) in enumerate(zip(got, want, first)):
      g = g.cpu().numpy()
      print("tensor %d: max |got - want| = %.3g" % (k, float(np.abs(g - w).max())))
      np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-5, err_msg="tensor %d" % k)
      moved += int((g != f.cpu().numpy()).sum())
    assert moved > 1000   # the update changed the rows
  finally:
    pht.close()


@pytest.mark.parametrize("unique", [True, False])
def test_every_ps_holds_exactly_its_ids(case, unique):
  """A fresh table: the rows exist because apply_gradients put them there, on the PS the packer chose."""
  pht = make(case, unique)
  try:
    first = pht.lookup(case["dev"], shared_features=case["shared"])
    assert all(float(t.abs().max()) == 0.0 for t in first)     # nothing is there yet, and a lookup inserts nothing
    assert all(ps.size(t) == 0 for ps in pht.tables for t in DIMS)
    pht.apply_gradients([torch.ones_like(t) for t in first], global_step=0, req_time=0)
    for t in DIMS:
      used = np.unique(np.array([x for n, rows in case["feats"].items() for r in rows for x in r
                                 if case["cfgs"].feature_configs[n].table == t], dtype=np.int64))
      assert all((used % NUM_PS == i).any() for i in range(NUM_PS))   # every PS has ids to hold
      for i, ps in enumerate(pht.tables):
        mine = used[used % NUM_PS == i]
        held = ps.contains(t, torch.from_numpy(used).cuda()).cpu().numpy()
        np.testing.assert_array_equal(held, used % NUM_PS == i)
        assert ps.size(t) == mine.size
        np.testing.assert_array_equal(np.sort(ps.dump(t, with_rows=False)[0].cpu().numpy()), mine)
  finally:
    pht.close()


def test_constructor_and_plan_checks(case):
  with pytest.raises(ValueError, match="num_ps"):
    PartitionedHashTable(0, table_configs(), product_cfgs(case["cfgs"]))
  bad = product_cfgs(case["cfgs"])
  bad.feature_configs[name_of(1)].slice_dims = [1, 4]
  with pytest.raises(ValueError, match="slice_dims"):
    PartitionedHashTable(2, table_configs(), bad, name_suffix="pht_test_%d" % next(_seq))
  bad = product_cfgs(case["cfgs"])
  bad.feature_configs[name_of(1)].table = "table_nine"
  with pytest.raises(ValueError, match="not configured"):
    PartitionedHashTable(2, table_configs(), bad, name_suffix="pht_test_%d" % next(_seq))
  pht = make(case)
  try:
    with pytest.raises(RuntimeError, match="no lookup"):
      pht.apply_gradients([])
  finally:
    pht.close()
