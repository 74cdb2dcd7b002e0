"""GPU test (-m gpu): the checkpoint save and save_as_tensor walk a table through the same code
(csrc/mhte_ckpt_host.h, walk_slots + fetch_reserved_row), so a shard file of the single-table save holds, in
order, exactly the strings save_as_tensor hands out walking that shard."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from monolith_amd import entry  # noqa: E402
from monolith_amd.multi_hash_table_ops import MultiHashTable  # noqa: E402
from tests import ckpt_proto as P  # noqa: E402


def test_a_saved_shard_is_what_save_as_tensor_walks(tmp_path):
  """One table past a doubling, the reserved key INT64_MIN among its ids, nothing expired: for 1 and 3
  shards the records of shard file sh of mhte_table_save (uncompressed records, no .meta; parsed by the
  independent Python framing) are byte for byte the strings of save_as_tensor over shard sh, 7 at a time."""
  dim, n, limit = 4, 300, 7
  mt = MultiHashTable.from_configs({"t": entry.make_table_config(
      [entry.CombineAsSegment(dim, entry.ZerosInitializer(), entry.AdagradOptimizer(0.05, 0.1))],
      entry.CuckooHashTableConfig(initial_capacity=1 << 6))}, name_suffix="ckpt_walk")
  hp0 = int(mt.stats("t").hashpower)
  rng = np.random.default_rng(21)
  ids = rng.choice(1 << 40, n, replace=False).astype(np.int64)
  ids[5] = np.iinfo(np.int64).min
  vals = rng.standard_normal((n, dim)).astype(np.float32)
  mt.assign({"t": (torch.as_tensor(ids).cuda(), torch.as_tensor(vals).cuda())}, req_time=1000)
  assert mt.size("t") == n and int(mt.stats("t").hashpower) > hp0
  for nshards in (1, 3):
    base = str(tmp_path / ("one%d" % nshards))
    mt.save_table("t", base, nshards=nshards)
    records = 0
    for sh in range(nshards):
      saved = P.unframe(open("%s-%05d-of-%05d" % (base, sh, nshards), "rb").read())
      walked, offset = [], 0
      while True:
        offset, ents = mt.save_as_tensor("t", sh, nshards, limit, offset)
        walked += ents
        if len(ents) < limit:
          break
      assert saved == walked, (nshards, sh)
      records += len(saved)
    assert records == n, nshards
