"""GPU parity (-m gpu) of the id-sharded multi-table step (csrc/mhte_shard_host.h, C ABI
mhte_shard_step_* / mhte_shard_group_*):
  * world 1 (identity exchange) against the single-GPU multi-table step, bit for bit;
  * N ranks in one process on one GPU (device copies as links) against the CPU oracle: every
    rank's embeddings, and every owner's rows after the peers' gradient blocks were applied in
    rank order (the reference's one optimizer application per sender,
    native_training/distributed_ps_sync.py:357-479);
  * world 1 over a real RCCL communicator (send / recv to self): the dlopen'ed RCCL path;
  * a peer block that overflows is reported, its ids read zeros.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402,F401
from monolith_amd import _lib, synthetic as S  # noqa: E402
from monolith_amd.distributed_ps_sync import (ShardedMultiStep, ShardedStepGroup,  # noqa: E402
                                              shard_block_geometry)
from monolith_amd.fused_step import MultiSparseStep  # noqa: E402
from test_multi_step_gpu import (ATOL, RTOL, dlrm_specs, group_opt_specs, make, oracle_backward,  # noqa: E402
                                 ragged_of, val_t)


def batch_of(specs, seed, n, universe, dist="zipf", skip=()):
  out = {}
  for s in specs:
    if s.name in skip:
      continue
    out[s.name] = S.id_batch(seed * 131 + s.slot, n, universe, dist, feature_slot=s.slot)
  return out


def _info_of(grp):
  import ctypes as C
  out = (C.c_int64 * 4)()
  _lib.check(grp._lib.mhte_shard_step_info(grp._hs[0], out))  # pylint: disable=protected-access
  return list(out)


def grads_of(step, rank, spec, n):
  rng = np.random.default_rng(1000 * step + 17 * rank + spec.slot)
  return (rng.standard_normal((n, spec.dim)) * 0.1).astype(np.float32)


@pytest.mark.parametrize("overlap", [False, True])
def test_world1_identity_matches_multi_step(overlap):
  specs = dlrm_specs(7, initial_capacity=1 << 12)
  by_name = sorted(specs, key=lambda s: s.name)
  B, steps = 6000, 6
  batches = [batch_of(specs, s, B, 9000) for s in range(steps + 1)]
  mt_a, mt_b = make(specs), make(specs)
  ref = MultiSparseStep(mt_a, B)
  shd = ShardedMultiStep(mt_b, B)
  if overlap:     # the next batch prepared on the step's own stream beside a stand-in for the dense model
    shd.set_overlap(True)
    busy = torch.randn(2048, 2048, device="cuda")
  assert shd.info()["transport"] == "identity"
  geo = shard_block_geometry(mt_b.get_table_dim_sizes(), B, 1)
  assert (shd.info()["id_block_bytes"], shd.info()["row_block_bytes"]) == (8 * geo["ids_block"], 4 * geo["rows_block"])
  rag_a = [ragged_of(specs, mt_a, b) for b in batches]
  rag_b = [ragged_of(specs, mt_b, b) for b in batches]
  for s in range(steps):
    ea = ref.forward(rag_a[s], rag_a[s + 1])
    eb = shd.forward(rag_b[s], rag_b[s + 1] if s % 3 != 2 else None)   # (every third: not ahead)
    assert torch.equal(ea, eb), "forward step %d" % s
    g = val_t(np.concatenate([grads_of(s, 0, sp, B).ravel() for sp in by_name]))
    if overlap:
      busy = busy @ busy * 1e-3
    ref.backward(g, S.update_time(s))
    shd.backward(g, S.update_time(s))
  shd.check()
  allids = {sp.name: np.unique(np.concatenate([b[sp.name] for b in batches])) for sp in specs}
  ra, rb = ragged_of(specs, mt_a, allids), ragged_of(specs, mt_b, allids)
  assert torch.equal(mt_a.raw_lookup(ra), mt_b.raw_lookup(rb))
  ref.close()
  shd.close()


@pytest.mark.parametrize("dist,world", [("uniform", 3), ("zipf", 2), ("zipf", 5)])
def test_group_against_oracle(dist, world, grad_fp16=False):
  _group_against_oracle(dlrm_specs(8, initial_capacity=1 << 10), dist, world, grad_fp16)


@pytest.mark.parametrize("dist,world", [("uniform", 2), ("zipf", 3)])
def test_group_bias_slice_rows_against_oracle(dist, world):
  """The reference's own sharded test configuration (NT/distributed_ps_test.py:480-505: a dim-1 FTRL
  bias slice + an Adagrad vector; dims 17 and 33) through the id-sharded step — round 3 had no
  multi-GPU path for these rows at all: one float per lane in the owners' lookups / updates, in the
  senders' scatter / gradient sums and on the wire (row slots of 17 / 33 floats)."""
  from test_multi_step_gpu import bias_slice_specs
  _group_against_oracle(bias_slice_specs(), dist, world, False)


@pytest.mark.parametrize("world,n_tables,expect", [(2, 8, 8), (5, 8, 8), (8, 8, 8), (2, 3, 8)])
def test_group_launch_count_does_not_grow_with_the_world(world, n_tables, expect):
  """The owner applies EVERY peer's gradient block in one launch (shard_apply_kernel: the lane group of
  an id's lowest sender applies its entries in rank order — the reference's one optimizer application
  per sender, distributed_ps_sync.py:357-479, in the one-op-over-all-shards shape of
  multi_hash_table_update_op.cc:247-308), and the sender's scatter shares a launch with the next batch's
  run dedup: a steady-state step is the same number of launches + exchanges at N = 2, 5 and 8 — round
  4's step made 2 N + 6 owner launches.  8: lookup, rows, scatter | dedup; sums | numbering, gradients, ids,
  apply, displacement pass (with one rank the pass rides in the next lookup's launch: 7).  Checked against
  the oracle like every other group test."""
  counts = _group_against_oracle(dlrm_specs(n_tables, initial_capacity=1 << 10), "zipf", world, False, B=2000, steps=4,
                                 always_ahead=True)
  steady = counts[1:-1]          # (the first step also deduplicates, numbers and sends its own batch; the last
                                 # one owes its displacement pass to a lookup that never comes)
  assert all(c == steady[0] for c in steady), counts
  assert steady[0] == expect, counts


def _group_against_oracle(specs, dist, world, grad_fp16, B=3000, steps=5, always_ahead=False, exact_order=False,
                          universe=None, ids_per_peer_table=0, check_tables=None, rank_batch=None, check_group=None):
  """check_tables(mts): called with every rank's tables after the final comparison, before the group closes;
  check_group(grp): the same with the group.  rank_batch(step, rank) -> {table name: ids}: the caller's id
  streams instead of the seeded ones (with dist "uniform" the caller keeps every id's occurrences in a batch
  at or below 32; a table may be absent from a rank's batch)."""
  by_name = sorted(specs, key=lambda s: s.name)
  if universe is None:
    universe = 200000 if dist == "uniform" else 7000
  exact = dist == "uniform" or exact_order   # every id occurs <= 32 times in a batch: sums in occurrence order
  mts = [make(specs) for _ in range(world)]
  grp = ShardedStepGroup(mts, B, ids_per_peer_table=ids_per_peer_table)
  if exact_order:
    grp.set_exact_order(True)
  geo = shard_block_geometry(mts[0].get_table_dim_sizes(), B, world, ids_per_peer_table)
  info = _info_of(grp)
  assert (info[0], info[1], info[2]) == (geo["cap"], 8 * geo["ids_block"], 4 * geo["rows_block"])
  ots = {s.name: s.oracle_table() for s in specs}

  def seeded_batch(step, r):
    skip = (by_name[min(3, len(by_name) - 1)].name,) if (r == 1 and step % 2 == 0) else ()   # ragged: an empty table on one rank
    n = B if not (r == 0 and step == 2) else 1                 # and a one-id batch
    return batch_of(specs, 100 * step + r, n, universe, dist, skip)

  if rank_batch is None:
    rank_batch = seeded_batch
  batches = [[rank_batch(s, r) for r in range(world)] for s in range(steps + 1)]
  rag = [[ragged_of(specs, mts[r], batches[s][r]) for r in range(world)] for s in range(steps + 1)]
  pre = False
  launch_counts = []
  for s in range(steps):
    ahead = always_ahead or s % 2 == 0
    embs = grp.forward(rag[s], rag[s + 1] if ahead else None, prefetched=pre)
    pre = ahead
    flat = []
    for r in range(world):
      views = mts[r].get_embeddings(rag[s][r], embs[r])
      for sp in by_name:
        ids = batches[s][r].get(sp.name)
        if ids is None:
          continue
        exp = ots[sp.name].lookup(ids)[0]
        got = views[sp.name].cpu().numpy()
        if exact:
          np.testing.assert_array_equal(got, exp, err_msg="rank %d %s step %d" % (r, sp.name, s))
        else:
          np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL)
    # the owners apply the senders' blocks in rank order; owners hold disjoint ids, so one oracle
    # table per feature stands for all of them
    for r in range(world):
      fg = []
      for sp in by_name:
        ids = batches[s][r].get(sp.name)
        if ids is None:
          continue
        g = grads_of(s, r, sp, ids.size)
        fg.append(g.ravel())
        uk, gu = oracle_backward(ots[sp.name], sp, ids, g)
        if grad_fp16:   # the sender's sums cross the wire as fp16 (round to nearest even)
          gu = gu.astype(np.float16).astype(np.float32)
        ots[sp.name].optimize(uk, gu, sp.lrs(), S.update_time(s))
      flat.append(val_t(np.concatenate(fg)))
    grp.backward(flat, S.update_time(s))
    per_rank = [f + b for f, b in grp.launches()]
    assert all(c == per_rank[0] for c in per_rank) or not always_ahead, per_rank
    launch_counts.append(max(per_rank))
  grp.check()
  # every owner holds exactly its ids, with the oracle's rows
  for sp in by_name:
    seen = np.unique(np.concatenate([b[sp.name] for st in batches[:steps] for b in st if sp.name in b]))
    for r in range(world):
      mine = seen[seen % world == r]
      got = mts[r].lookup({sp.name: torch.as_tensor(mine).cuda()})[sp.name].cpu().numpy()
      exp = ots[sp.name].lookup(mine)[0]
      if exact:
        np.testing.assert_array_equal(got, exp, err_msg="owner %d %s" % (r, sp.name))
      else:
        np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL)
    sizes = [int(mts[r].size(sp.name)) for r in range(world)]
    assert sum(sizes) == seen.size, (sp.name, sizes, seen.size)
  if check_tables is not None:
    check_tables(mts)
  if check_group is not None:
    check_group(grp)
  grp.close()
  return launch_counts


def _displaced_not_doubled(specs, slots):
  """The three conditions of the other paths' high-load tests (test_multi_step_displacement_and_doubling),
  for every rank and table: nothing dropped, the table never doubled, and it is over half full — ids
  whose two buckets were full were placed by the displacement pass."""
  def check(mts):
    for r, mt in enumerate(mts):
      for sp in specs:
        st = mt.stats(sp.name)
        assert st.dropped == 0, (r, sp.name, st.dropped)
        assert st.hashpower == (slots // 4).bit_length() - 1, (r, sp.name, st.hashpower)
        assert st.size > 0.5 * slots, (r, sp.name, st.size)
  return check


@pytest.mark.parametrize("world,group_opt", [(1, False), (3, False), (2, True)])
def test_group_displacement_at_high_load(world, group_opt):
  """The owner's displacement pass, forced: tables of 8192 slots (hashpower 11) that may fill to 0.97,
  uniform ids, five steps that take every owner's tables to 5800-6700 ids (load 0.70-0.82; per-owner oracle
  tables of 8192 slots hold them without doubling), so that every update past the first defers ids whose two
  buckets are full.
    world 1: basic optimizers, the pass rides in the next owner lookup (shard_slow_all_role<true>);
    world 3: the pass as a launch of its own, deferred ids with entries of several senders in the
             cross-peer slots (shard_slow_all_role<false>);
    world 2, GroupAdaGrad tables: the whole-segment form of the 64-lane update (apply_row_wave's GROUP).
  The tables must not double, and an owner reserves key capacity for full blocks from every peer before each
  update (Table::ensure_capacity(cap * world)): live keys + cap * world has to stay under 0.97 * 8192 = 7946.
  Hence B = 1600 ids per rank and table from a universe of 30000 per rank, and peer blocks of B / world + 100
  ids (the largest block of these batches holds 578 of 636 at world 3, 834 of 900 at world 2): the bound peaks
  at 7340.  Uniform ids: bit-exact against the oracle like test_group_against_oracle[uniform-*]."""
  kw = dict(initial_capacity=1 << 13, max_load_factor=0.97)
  if group_opt:
    specs = group_opt_specs()
    for sp in specs:
      sp.kw = kw
  else:
    specs = dlrm_specs(3, **kw)
  B = 1600
  _group_against_oracle(specs, "uniform", world, False, B=B, steps=5, universe=30000 * world,
                        ids_per_peer_table=B if world == 1 else B // world + 100,
                        check_tables=_displaced_not_doubled(specs, 1 << 13))


@pytest.mark.parametrize("world", [1, 3])
def test_exact_order_makes_the_sharded_step_bit_exact_under_zipf(world):
  """mhte_shard_step_set_exact_order (round 6): Zipf batches hold lists of hundreds of occurrences, which the
  sender otherwise sums as a fixed tree (within 1e-6 of the sequential sum).  With exact order every sender's
  per-id sum is the reference's sequential sum (unique_mapping_ops.cc:284-329) and every owner's row — one
  optimizer application per sender, in rank order (distributed_ps_sync.py:357-479) — equals the oracle's bit for
  bit: embeddings of every step and the final rows are compared with assert_array_equal.  Eight tables of dims
  16 / 32 / 64 (Adagrad, SGD, and a two-segment FTRL + Adagrad row) in one model."""
  specs = dlrm_specs(8, initial_capacity=1 << 10)
  _group_against_oracle(specs, "zipf", world, False, B=4000, steps=4, exact_order=True)


@pytest.mark.parametrize("transport", ["auto", "ipc"])
def test_exact_order_one_rank_equals_the_exact_multi_table_step(transport):
  """One rank through the identity exchange and through the peer-store transport to itself (the sums then go
  straight into the window, gather_out_ptr's peer path): with exact order on both sides the sharded step and the
  multi-table step (MHTE_EXACT_ORDER, mstep_exact_sum_kernel) leave the same bits under Zipf — embeddings of
  every step and every row."""
  specs = dlrm_specs(7, initial_capacity=1 << 12)
  by_name = sorted(specs, key=lambda s: s.name)
  B, steps = 6000, 5
  batches = [batch_of(specs, 40 + s, B, 3000) for s in range(steps + 1)]   # (Zipf: lists of hundreds)
  mt_a, mt_b = make(specs), make(specs)
  ref = MultiSparseStep(mt_a, B, exact_order=True)
  shd = ShardedMultiStep(mt_b, B, transport=transport)
  shd.set_exact_order(True)
  assert shd.info()["transport"].startswith("ipc" if transport == "ipc" else "identity")
  rag_a = [ragged_of(specs, mt_a, b) for b in batches]
  rag_b = [ragged_of(specs, mt_b, b) for b in batches]
  for s in range(steps):
    ea = ref.forward(rag_a[s], rag_a[s + 1])
    eb = shd.forward(rag_b[s], rag_b[s + 1])
    assert torch.equal(ea, eb), "forward step %d" % s
    g = val_t(np.concatenate([grads_of(s, 0, sp, B).ravel() for sp in by_name]))
    ref.backward(g, S.update_time(s))
    shd.backward(g, S.update_time(s))
  shd.check()
  allids = {sp.name: np.unique(np.concatenate([b[sp.name] for b in batches])) for sp in specs}
  ra, rb = ragged_of(specs, mt_a, allids), ragged_of(specs, mt_b, allids)
  assert torch.equal(mt_a.raw_lookup(ra), mt_b.raw_lookup(rb))
  ref.close()
  shd.close()


def test_world1_over_rccl():
  specs = dlrm_specs(4, initial_capacity=1 << 10)
  by_name = sorted(specs, key=lambda s: s.name)
  B, steps = 2000, 4
  batches = [batch_of(specs, 7 + s, B, 5000) for s in range(steps + 1)]
  mt_a, mt_b = make(specs), make(specs)
  ref = ShardedMultiStep(mt_a, B)
  rc = ShardedMultiStep(mt_b, B, use_rccl=True)
  assert rc.info()["transport"] == "rccl"
  rag_a = [ragged_of(specs, mt_a, b) for b in batches]
  rag_b = [ragged_of(specs, mt_b, b) for b in batches]
  for s in range(steps):
    ea = ref.forward(rag_a[s], rag_a[s + 1])
    eb = rc.forward(rag_b[s], rag_b[s + 1])
    assert torch.equal(ea, eb), "forward step %d" % s
    g = val_t(np.concatenate([grads_of(s, 0, sp, B).ravel() for sp in by_name]))
    ref.backward(g, S.update_time(s))
    rc.backward(g, S.update_time(s))
  rc.check()
  ref.close()
  rc.close()


def test_exact_size_exchange(monkeypatch):
  """MHTE_SHARD_EXACT=1: rows and gradients cross only for the occupied part of every (peer, table)
  segment, the counts copied to the host behind the id exchange — same results, through the group
  transport and through RCCL send / recv to self."""
  monkeypatch.setenv("MHTE_SHARD_EXACT", "1")
  test_group_against_oracle("zipf", 3)
  test_group_against_oracle("uniform", 2)
  test_world1_over_rccl()


def test_exact_form_one_pair_per_peer_and_no_host_wait_when_prepared_ahead(monkeypatch):
  """VERDICT r5 next #4b.  The exact-size form used to issue world x T send / recv pairs per exchange and to
  block the host in every id exchange.  Now a peer's occupied table segments cross as ONE packed pair (the
  reference moves each tensor as one all-to-all-v, distributed_ps_sync.py:131-159,357-479) and the next
  batch's id headers ride in the gradient exchange's group, so a batch prepared a step ahead finds its
  counts on the host (when the device is not behind the host).  Checked on the in-process group (3 ranks, 6 tables: device copies stand for the pairs,
  the packing / unpacking / counting is the RCCL transport's code) against the oracle, and over a real
  communicator to self."""
  monkeypatch.setenv("MHTE_SHARD_EXACT", "1")
  world, n_tables, B, steps = 3, 6, 1500, 5
  specs = dlrm_specs(n_tables, initial_capacity=1 << 10)
  by_name = sorted(specs, key=lambda s: s.name)
  mts = [make(specs) for _ in range(world)]
  grp = ShardedStepGroup(mts, B)
  ots = {s.name: s.oracle_table() for s in specs}
  batches = [[batch_of(specs, 31 * s + r, B, 6000, "zipf") for r in range(world)] for s in range(steps + 1)]
  rag = [[ragged_of(specs, mts[r], batches[s][r]) for r in range(world)] for s in range(steps + 1)]
  for s in range(steps):
    embs = grp.forward(rag[s], rag[s + 1], prefetched=s > 0)
    flat = []
    for r in range(world):
      views = mts[r].get_embeddings(rag[s][r], embs[r])
      for sp in by_name:
        np.testing.assert_allclose(views[sp.name].cpu().numpy(), ots[sp.name].lookup(batches[s][r][sp.name])[0],
                                   rtol=RTOL, atol=ATOL)
    for r in range(world):
      fg = []
      for sp in by_name:
        ids = batches[s][r][sp.name]
        g = grads_of(s, r, sp, ids.size)
        fg.append(g.ravel())
        uk, gu = oracle_backward(ots[sp.name], sp, ids, g)
        ots[sp.name].optimize(uk, gu, sp.lrs(), S.update_time(s))
      flat.append(val_t(np.concatenate(fg)))
    grp.backward(flat, S.update_time(s))
    # (the device finishes the backward before the next forward is enqueued, so the counts fetched behind the
    # gradient exchange have landed.  A host that runs AHEAD of the device still waits at the next forward for
    # that exchange — with the owner update already enqueued behind it; round 5 blocked in front of it.)
    torch.cuda.synchronize()
    for w in grp.wire_stats():
      # ids, rows, gradients (+ the next batch's id headers in the gradient exchange's group): never a pair per
      # (peer, table)
      assert w["exchanges"] >= 3 and w["pairs_max"] <= 2 * world, w
      assert w["pairs"] <= w["exchanges"] * 2 * world, w
      if s > 0:
        assert w["host_waits"] == 0, (s, w)    # prepared ahead: nobody waited for a count
  grp.check()
  grp.close()
  # ... and through ncclSend / ncclRecv to self
  specs = dlrm_specs(4, initial_capacity=1 << 10)
  by_name = sorted(specs, key=lambda s: s.name)
  batches = [batch_of(specs, 7 + s, 2000, 5000) for s in range(5)]
  mt_a, mt_b = make(specs), make(specs)
  ref = ShardedMultiStep(mt_a, 2000)
  rc = ShardedMultiStep(mt_b, 2000, use_rccl=True)
  rag_a = [ragged_of(specs, mt_a, b) for b in batches]
  rag_b = [ragged_of(specs, mt_b, b) for b in batches]
  for s in range(4):
    ea = ref.forward(rag_a[s], rag_a[s + 1])
    eb = rc.forward(rag_b[s], rag_b[s + 1])
    assert torch.equal(ea, eb), "forward step %d" % s
    g = val_t(np.concatenate([grads_of(s, 0, sp, 2000).ravel() for sp in by_name]))
    ref.backward(g, S.update_time(s))
    rc.backward(g, S.update_time(s))
    torch.cuda.synchronize()
    w = rc.wire_stats()
    assert w["pairs_max"] <= 2 and (s == 0 or w["host_waits"] == 0), (s, w)
  rc.check()
  ref.close()
  rc.close()


def test_overlap_over_rccl(monkeypatch):
  """MHTE_SHARD_OVERLAP=1 with the RCCL transport: dedup and numbering run on the step's own stream,
  the id exchange stays on the communicator's stream (sent by the next forward)."""
  monkeypatch.setenv("MHTE_SHARD_OVERLAP", "1")
  test_world1_over_rccl()
  test_group_against_oracle("uniform", 2)      # (in-process groups ignore the mode)


@pytest.mark.parametrize("high_load", [False, True])
def test_sharded_step_with_occurrence_filters(high_load):
  """Tables with an occurrence filter through the sharded step (round 2 rejected them): every OWNER
  asks its own filter about the ids of a sender's block it does not hold, with count 1 per (sender,
  id) — the reference's fused optimize behind the all-to-all (tf_bridge.cc:300-321 per id of
  multi_hash_table_update_op.cc:270-306) — senders in rank order, the window moving between them.
  Checked against oracle tables + the filter restatement (oracle.SlidingFilter) per owner.
  high_load: tables of 1024 slots that may fill to 0.97 and never double, filled to 770-785 admitted ids per
  owner and table (the oracle tables' sizes), so that the per-peer displacement pass (shard_slow_role) must
  place ids.  An owner reserves key capacity for full blocks from every peer before each update
  (Table::ensure_capacity(cap * world)), so the load is reached in small steps: 40 steps of 120 ids per rank
  and table, peer blocks of 84 ids (the largest holds 73); live keys + 2 * 84 peaks at 940 of 0.97 * 1024 = 993."""
  from monolith_amd import entry
  from monolith_amd.multi_hash_table_ops import HashFilter, MultiHashTable
  world, thr = 2, 2
  B, steps, cap = (120, 40, 84) if high_load else (1500, 6, 0)
  dims = {"a": 16, "b": 32}
  mts, flts, ots, models = [], [], [], []
  for r in range(world):
    flt = HashFilter(capacity=4000, split_num=5)
    cfgs = {n: entry.make_table_config(
        [entry.CombineAsSegment(d, entry.ZerosInitializer(), entry.AdagradOptimizer(0.05, 0.1))],
        entry.CuckooHashTableConfig(**(dict(initial_capacity=1 << 10, max_load_factor=0.97) if high_load else {})),
        slot_occurrence_threshold_config=entry.SlotOccurrenceThresholdConfig(default_occurrence_threshold=thr))
            for n, d in dims.items()}
    mts.append(MultiHashTable.from_configs(cfgs, name_suffix="shflt%d" % r, hash_filter=flt))
    flts.append(flt)
    ots.append({n: O.Table(O.segment(d, O.OPT_ADAGRAD, p=(0.1, 0.0)), 1) for n, d in dims.items()})
    models.append(O.SlidingFilter(4000, 5, defer_advance=True))
  grp = ShardedStepGroup(mts, B, ids_per_peer_table=cap)
  names = sorted(dims)
  dropped = [0]

  def ids_of(s, r, k):
    # A small universe: ids come back, pass their threshold, get trained.  Every id has its own 12-bit
    # filter signature (fid bits 17..28, hash_filter.h:151), so no two ids share a count: which of two
    # aliasing ids of ONE launch crosses the threshold first is not defined (nor in the reference,
    # whose filter is not thread safe) and would make the expectation order-dependent.
    if high_load:
      # (the ids below reach 430-580 per owner and table — id_batch's fids collide modulo 1800 and the low
      # bits favour owner 0 — which no table size holds both over half full and under 0.97; here every
      # index comes and the owners get half each)
      idx = np.random.default_rng(50 * s + 7 * r + k).integers(0, 1700, B) + 1800 * k
      return ((idx + 1) << 17) | (idx % 2) | (np.int64(k + 1) << 48)
    idx = S.id_batch(50 * s + 7 * r + k, B, 1800, "uniform") % 1800 + 1800 * k
    return ((idx + 1) << 17) | (idx % 7) | (np.int64(k + 1) << 48)

  def rag_of(s, r):
    return mts[r].get_ragged_id({n: torch.as_tensor(ids_of(s, r, k)).cuda() for k, n in enumerate(names)})

  for s in range(steps):
    embs = grp.forward([rag_of(s, r) for r in range(world)], [rag_of(s + 1, r) for r in range(world)],
                       prefetched=s > 0)
    for r in range(world):
      views = mts[r].get_embeddings(rag_of(s, r), embs[r])
      for k, n in enumerate(names):
        ids = ids_of(s, r, k)
        exp = np.zeros((ids.size, dims[n]), np.float32)
        for o in range(world):
          m = np.mod(ids, world) == o
          exp[m] = ots[o][n].lookup(ids[m])[0]
        np.testing.assert_array_equal(views[n].cpu().numpy(), exp, err_msg="rank %d %s step %d" % (r, n, s))
    flat = []
    grads = {}
    for r in range(world):
      fg = []
      for k, n in enumerate(names):
        g = (np.random.default_rng(1000 * s + 10 * r + k).standard_normal((B, dims[n])) * 0.1).astype(np.float32)
        grads[(r, n)] = g
        fg.append(g.ravel())
      flat.append(val_t(np.concatenate(fg)))
    grp.backward(flat, S.update_time(s))
    # the owners' semantics: senders in rank order, one consultation per (sender, distinct id)
    for o in range(world):
      for r in range(world):
        for k, n in enumerate(names):
          ids = ids_of(s, r, k)
          uk, _, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, ids.size], [dims[n]])
          gu = O.fill_with_offset_map_gradient(np.arange(uk.size), [0, uk.size], grads[(r, n)].ravel(), vo, vos,
                                               [dims[n]]).reshape(-1, dims[n])
          mine = np.mod(uk, world) == o
          keep = []
          for i in np.nonzero(mine)[0]:
            fid = int(uk[i])
            if ots[o][n].contains(fid) or models[o].add(fid, 1) >= thr:
              keep.append(i)
            else:
              dropped[0] += 1
          if keep:
            ots[o][n].optimize(uk[keep], gu[keep], [0.05], S.update_time(s))
        models[o].advance_if_full()
  grp.check()
  assert dropped[0] > 1000            # the filters did filter
  for o in range(world):
    for k, n in enumerate(names):
      seen = np.unique(np.concatenate([ids_of(s, r, k) for s in range(steps) for r in range(world)]))
      mine = seen[np.mod(seen, world) == o]
      want = np.array([ots[o][n].contains(int(x)) for x in mine])
      got = mts[o].contains(n, torch.as_tensor(mine).cuda()).cpu().numpy().astype(bool)
      np.testing.assert_array_equal(got, want)
      assert want.sum() > 0
      held = mine[want]
      np.testing.assert_array_equal(mts[o].lookup({n: torch.as_tensor(held).cuda()})[n].cpu().numpy(),
                                    ots[o][n].lookup(held)[0])
    probe = np.unique(np.concatenate([ids_of(s, r, 0) for s in range(steps) for r in range(world)]))
    probe = probe[np.mod(probe, world) == o]
    absent = np.array([not ots[o][names[0]].contains(int(x)) for x in probe])
    if absent.any():
      np.testing.assert_array_equal(flts[o].get(torch.as_tensor(probe[absent]).cuda()).cpu().numpy(),
                                    [models[o].get(int(x)) for x in probe[absent]])
  if high_load:
    for o in range(world):
      for n in names:
        st = mts[o].stats(n)
        assert st.dropped == 0 and st.hashpower == 8 and st.size > 0.5 * (1 << 10), (o, n, st.size, st.hashpower)
  grp.close()


def test_fp16_gradient_wire(monkeypatch):
  """MHTE_SHARD_GRAD_FP16=1 (the reference's optional fp16 cast of the gradient all-to-all,
  distributed_ps_sync.py:47,334-337): the owners see every sender's per-id sums rounded to fp16 —
  bit-exact against the oracle fed the same rounding; through device copies, RCCL's exact-size form
  (send / recv to self) and the fixed-size form."""
  monkeypatch.setenv("MHTE_SHARD_GRAD_FP16", "1")
  test_group_against_oracle("uniform", 3, grad_fp16=True)
  monkeypatch.setenv("MHTE_SHARD_EXACT", "1")
  test_group_against_oracle("uniform", 2, grad_fp16=True)


def test_block_overflow_is_reported():
  specs = dlrm_specs(2, initial_capacity=1 << 10)
  B = 512
  mts = [make(specs) for _ in range(2)]
  grp = ShardedStepGroup(mts, B, ids_per_peer_table=16)
  b = [batch_of(specs, 3 + r, B, 100000, "uniform") for r in range(2)]
  rag = [ragged_of(specs, mts[r], b[r]) for r in range(2)]
  embs = grp.forward(rag)
  with pytest.raises(_lib.MhteError) as ei:
    grp.check()
  assert ei.value.code == _lib.MHTE_RESOURCE_EXHAUSTED
  assert all(float(e.abs().max()) == 0.0 for e in embs)   # (empty tables: zeros either way)
  grp.close()


def test_argument_errors():
  specs = dlrm_specs(2, initial_capacity=1 << 10)
  mt = make(specs)
  with pytest.raises(_lib.MhteError):
    ShardedStepGroup([mt], 0)
  grp = ShardedStepGroup([mt, make(specs)], 64)
  one = ShardedMultiStep.__new__(ShardedMultiStep)
  # a rank of a world > 1 without a communicator cannot step on its own
  one._libmod, one._lib, one.table, one._dims = _lib, mt._lib, mt, mt.get_table_dim_sizes()  # pylint: disable=protected-access
  one._h, one._ahead, one._keep = grp._hs[0], None, None  # pylint: disable=protected-access
  b = batch_of(specs, 1, 64, 1000)
  with pytest.raises(_lib.MhteError) as ei:
    one.forward(ragged_of(specs, mt, b))
  assert ei.value.code == _lib.MHTE_FAILED_PRECONDITION
  one._h = None  # pylint: disable=protected-access
  grp.close()


@pytest.mark.parametrize("dist,world", [("uniform", 2), ("zipf", 3)])
def test_group_whole_segment_optimizer_against_oracle(dist, world):
  """GroupAdaGrad tables through the id-sharded step (round 3 refused them): the sender side is
  optimizer-agnostic, the owner applies every peer's block with the whole-segment instance of its
  upsert (shard_upsert_kernel<VW, GROUP>)."""
  _group_against_oracle(group_opt_specs(), dist, world, False)


def many_table_specs(n=40):
  """More tables than one launch takes (kMaxStepTables = 32), with every kind of row on BOTH sides of
  the chunk boundary: float4 rows, a bias + vector row (one float per lane), a whole-segment
  optimizer."""
  from test_multi_step_gpu import Spec
  specs = []
  for i in range(n):
    if i in (3, 34):
      segs = [(1, "ftrl", 0.05), (16, "adagrad", 0.01)]
    elif i in (6, 37):
      segs = [(16, "group", 0.02)]
    elif i == 38:
      segs = [(1, "ftrl", 0.05), (16, "group", 0.02)]
    else:
      segs = [((16, 32, 64)[i % 3], "adagrad", 0.01)]
    specs.append(Spec("t%02d" % i, segs, i + 1))
  return specs


@pytest.mark.parametrize("dist,world", [("uniform", 2), ("zipf", 3)])
def test_group_more_than_32_tables_against_oracle(dist, world):
  """Round 3's sharded step refused a model of more than 32 tables.  The limit is a per-launch budget
  (kernel arguments): every stage launches per 32 tables (ShardOwnerArgs.t0 / tc), the exchanges
  carry all of them in one block per peer."""
  _group_against_oracle(many_table_specs(), dist, world, False, B=700, steps=4)


def test_world1_identity_more_than_32_tables():
  """40 tables, world 1 (identity exchange): bit for bit the single-GPU multi-table step."""
  specs = [s for s in many_table_specs() if not any(o == "group" for _, o, _ in s.segs)]
  assert len(specs) > 32
  by_name = sorted(specs, key=lambda s: s.name)
  B, steps = 900, 4
  batches = [batch_of(specs, 7 + s, B, 20000) for s in range(steps + 1)]
  mt_a, mt_b = make(specs), make(specs)
  ref = MultiSparseStep(mt_a, B)
  shd = ShardedMultiStep(mt_b, B)
  rag_a = [ragged_of(specs, mt_a, b) for b in batches]
  rag_b = [ragged_of(specs, mt_b, b) for b in batches]
  for s in range(steps):
    ea = ref.forward(rag_a[s], rag_a[s + 1])
    eb = shd.forward(rag_b[s], rag_b[s + 1] if s % 2 == 0 else None)
    assert torch.equal(ea, eb), "forward step %d" % s
    g = val_t(np.concatenate([grads_of(s, 0, sp, B).ravel() for sp in by_name]))
    ref.backward(g, S.update_time(s))
    shd.backward(g, S.update_time(s))
  shd.check()
  allids = {sp.name: np.unique(np.concatenate([b[sp.name] for b in batches])) for sp in specs}
  ra, rb = ragged_of(specs, mt_a, allids), ragged_of(specs, mt_b, allids)
  assert torch.equal(mt_a.raw_lookup(ra), mt_b.raw_lookup(rb))
  ref.close()
  shd.close()
