"""GPU suite of the PS-sharded table (monolith_amd/distributed_ps.py): three tables of dims 4, 8 and 17 with SGD
and Adagrad, a few hundred ids with heavy duplication and some negative ids.  ``lookup`` after three
``apply_gradients`` equals, bit for bit, the same steps on ONE MultiHashTable driven through the same unique /
fill ops (so every unique id's duplicates are summed in the order fill_with_offset_map_gradient guarantees), and
PS i holds exactly the ids with floormod(id, num_ps) == i."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import split_by_indices_truth as ST  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd import entry  # noqa: E402
from monolith_amd.distributed_ps import DistributedMultiTypeHashTable  # noqa: E402
from monolith_amd.multi_hash_table_ops import MultiHashTable, Ragged  # noqa: E402

pytestmark = pytest.mark.gpu

_seq = itertools.count()
DIMS = {"a_sgd": 4, "b_adagrad": 8, "c_sgd17": 17}
STEPS = 3


def configs():
  seg = lambda dim, opt: entry.make_table_config(   # noqa: E731
      [entry.CombineAsSegment(dim, entry.ZerosInitializer(), opt)], entry.CuckooHashTableConfig())
  return {"a_sgd": seg(4, entry.SgdOptimizer(0.5)),
          "b_adagrad": seg(8, entry.AdagradOptimizer(0.05, 0.1)),
          "c_sgd17": seg(17, entry.SgdOptimizer(0.25))}


def batches():
  """Per step {slot: (ids, grads)}: ~300 ids per table from a pool of 40 (heavy duplication), negative ids among
  them; the last step leaves one table out."""
  rng = np.random.RandomState(11)
  pool = np.concatenate([rng.randint(-50, 0, size=8), rng.randint(0, 10 ** 12, size=32)]).astype(np.int64)
  out = []
  for step in range(STEPS):
    b = {}
    for k, (name, dim) in enumerate(DIMS.items()):
      if step == STEPS - 1 and k == 1:
        continue
      n = 280 + 17 * k + step
      b[name] = (pool[rng.randint(0, pool.size, size=n)], rng.standard_normal((n, dim)).astype(np.float32))
    out.append(b)
  return out, pool


def cuda(b):
  return {k: (torch.from_numpy(i).cuda(), torch.from_numpy(g).cuda()) for k, (i, g) in b.items()}


@pytest.fixture(scope="module")
def single_table_result():
  """The steps on ONE table through unique_key_with_value_and_offset / fill_with_offset_map(_gradient) with every
  unique id in one 'split', then the lookup of the whole pool: computed once, shared by the cases."""
  steps, pool = batches()
  table = MultiHashTable(configs(), name_suffix="dps_single_%d" % next(_seq))
  dims = list(table.get_table_dim_sizes())

  def everything(unique_key):
    return Ragged(torch.arange(unique_key.values.numel(), dtype=torch.int64, device="cuda"), unique_key.row_splits)

  for step, b in enumerate(steps):
    b = cuda(b)
    ragged_id = table.get_ragged_id({k: v[0] for k, v in b.items()})
    r = D.unique_key_with_value_and_offset(ragged_id, dims, generate_buffer=False)
    flat_grad = table.get_flat_value({k: v[1] for k, v in b.items()})
    g = D.fill_with_offset_map_gradient(everything(r.unique_key), flat_grad, r.value_offset, r.value_offset_split,
                                        dims)
    table.raw_apply_gradients(r.unique_key, g, global_step=step, req_time=0)
  query = {name: torch.from_numpy(np.concatenate([pool, pool[::3]])).cuda() for name in DIMS}
  ragged_id = table.get_ragged_id(query)
  r = D.unique_key_with_value_and_offset(ragged_id, dims)
  buf = D.fill_with_offset_map(everything(r.unique_key), table.raw_lookup(r.unique_key), r.value_offset,
                               r.value_offset_split, r.value_buffer, dims)
  emb = {k: v.cpu().numpy() for k, v in table.get_embeddings(ragged_id, buf).items()}
  table.close()
  assert all(np.abs(e).max() > 0 for e in emb.values())   # the steps moved every table
  return emb


@pytest.mark.parametrize("num_ps", [1, 2, 5])
def test_sharded_steps_equal_the_single_table(num_ps, single_table_result):
  steps, pool = batches()
  dps = DistributedMultiTypeHashTable(num_ps, configs(), name_suffix="dps_%d_%d" % (num_ps, next(_seq)))
  try:
    assert dps.num_ps == num_ps and len(dps.tables) == num_ps
    for step, b in enumerate(steps):
      assert dps.apply_gradients(cuda(b), global_step=step, req_time=0) is dps
    query = {name: torch.from_numpy(np.concatenate([pool, pool[::3]])).cuda() for name in DIMS}
    emb = dps.lookup(query)
    assert sorted(emb) == sorted(DIMS)
    for name, dim in DIMS.items():
      assert tuple(emb[name].shape) == (query[name].numel(), dim)
      ST.same_bits(emb[name].cpu().numpy(), single_table_result[name], "%s num_ps=%d" % (name, num_ps))
    # residency: PS i holds exactly the ids with floormod(id, num_ps) == i
    for name in DIMS:
      seen = np.unique(np.concatenate([b[name][0] for b in steps if name in b]))
      shard = np.mod(seen, num_ps)   # (numpy's mod is floormod: a negative id's shard is >= 0)
      assert (shard >= 0).all() and (seen < 0).any()
      for i, t in enumerate(dps.tables):
        held = t.contains(name, torch.from_numpy(seen).cuda()).cpu().numpy()
        assert np.array_equal(held, shard == i), (name, num_ps, i)
        assert t.size(name) == int((shard == i).sum()), (name, num_ps, i)
    # a slot that was not asked for is not returned
    assert sorted(dps.lookup({"a_sgd": query["a_sgd"][:5]})) == ["a_sgd"]
  finally:
    dps.close()
