"""GPU tests (-m gpu) of the device-resident touched-key set: the stand-alone op against the key-by-key
truth model of tests/touched_key_set_truth.py (contents compared after sorting, stats after every call),
and the recording of the update entry points of a MultiHashTable it is attached to."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from touched_key_set_truth import TruthSet  # noqa: E402
from monolith_amd import _lib, entry  # noqa: E402
from monolith_amd.multi_hash_table_ops import HashFilter, MultiHashTable  # noqa: E402
from monolith_amd.touched_key_set_ops import TouchedKeySet  # noqa: E402

_counter = [0]
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def _name():
  _counter[0] += 1
  return "tks%d" % _counter[0]


def ids_t(x):
  return torch.as_tensor(np.asarray(x, dtype=np.int64)).cuda()


def _pairs(tks):
  ids, tags = tks.steal_pairs()
  return sorted(zip(ids.cpu().tolist(), tags.cpu().tolist()))


def _check(tks, truth, what=""):
  assert tks.stats() == truth.stats(), what


# ------------------------------------------------------------------------------------------ 1
def test_reference_cases():
  tks = TouchedKeySet(1000, name_suffix=_name())
  assert tks.capacity == 1000
  assert tks.insert(ids_t(np.arange(1000))) == 0
  assert tks.size == 1000
  got = tks.steal()
  assert got.dtype == torch.int64
  assert sorted(got.cpu().tolist()) == list(range(1000))
  assert tks.size == 0
  # 1 005 ids: the host cuts the input at C + 1 positions, the second call finds the set over capacity
  assert tks.insert(ids_t(np.arange(1005))) == 1001
  assert sorted(tks.steal().cpu().tolist()) == [1001, 1002, 1003, 1004]
  assert tks.stats() == (0, 1001, 1, 1000)


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("C", [1, 7, 64, 257])
def test_random_call_sequences_against_the_truth(C):
  rng = np.random.default_rng(100 + C)
  lengths = [0, 1, 63, 64, 65, C, C + 1, 4 * C + 3]
  for universe in (C // 2 + 1, 2 * C + 3, 2**62):
    tks = TouchedKeySet(C, name_suffix=_name())
    truth = TruthSet(C)
    for call in range(14):
      n = int(lengths[(call * 3 + int(rng.integers(0, 8))) % 8])
      ids = rng.integers(0, universe, n).astype(np.int64)
      exp = truth.insert(ids.tolist())
      assert tks.insert(ids_t(ids)) == exp, (universe, call, n)
      _check(tks, truth, (universe, call, n))
      if call % 5 == 4:
        assert _pairs(tks) == truth.steal(), (universe, call)
        _check(tks, truth)
    assert _pairs(tks) == truth.steal(), universe
    tks.close()


# ------------------------------------------------------------------------------------------ 3
def test_hand_made_cuts():
  C = 4
  tks, truth = TouchedKeySet(C, name_suffix=_name()), TruthSet(C)

  def both(ids):
    assert tks.insert(ids_t(ids)) == truth.insert(ids)
    _check(tks, truth, ids)

  both([10, 11])                      # size 2
  # new keys 12, 13, 14 fill the set to C + 1 at position 2; the clear sits before position 3:
  # 10 / 12 (seen only before the cut) are gone, 11 (before and after) and 15 stay
  both([12, 13, 14, 11, 15])
  assert truth.stats() == (2, 5, 1, C)
  assert _pairs(tks) == [(11, 0), (15, 0)] == truth.steal()
  both([1, 2, 3, 4])                  # size0 == C afterwards
  both([5])                           # fills to C + 1, nothing follows: no clear
  assert truth.stats()[:3] == (5, 5, 1)
  tks.insert_async(ids_t([6, 7]), n_dev=torch.zeros(1, dtype=torch.int32, device="cuda"))
  _check(tks, truth, "an empty call must not clear, even over capacity")
  both([])
  both([5])                           # size0 == C + 1: even a duplicate clears first
  assert truth.stats()[:3] == (1, 10, 2)
  both([1, 2, 3])                     # size C exactly
  both([3, 9, 3])                     # 9 fills to C + 1 at position 1, the duplicate behind it clears
  assert truth.stats()[:3] == (1, 15, 3)
  assert _pairs(tks) == [(3, 0)] == truth.steal()


# ------------------------------------------------------------------------------------------ 4
def test_tags_and_extreme_fids():
  tks, truth = TouchedKeySet(64, name_suffix=_name()), TruthSet(64)
  fids = [-1, 0, I64_MIN, I64_MAX, 5]
  for tag in (0, 1, 7):
    tks.insert_async(ids_t(fids + fids), tag=tag)
    truth.insert(fids + fids, tag)
    _check(tks, truth, tag)
  assert truth.stats()[0] == 15      # one fid under two tags is two keys
  assert _pairs(tks) == truth.steal()


# ------------------------------------------------------------------------------------------ 5
def test_n_dev_is_honoured():
  tks, truth = TouchedKeySet(64, name_suffix=_name()), TruthSet(64)
  ids = list(range(100, 140))
  n_dev = torch.tensor([17], dtype=torch.int32, device="cuda")
  tks.insert_async(ids_t(ids), n_dev=n_dev)
  truth.insert(ids[:17])
  _check(tks, truth)
  n_dev.zero_()
  tks.insert_async(ids_t(ids), n_dev=n_dev)
  _check(tks, truth)
  n_dev.fill_(1000)                   # more than n_max: n_max bounds it
  tks.insert_async(ids_t(ids), n_dev=n_dev)
  truth.insert(ids)
  _check(tks, truth)
  assert _pairs(tks) == truth.steal()


# ------------------------------------------------------------------------------------------ 6
def _tk_slot(fid, tag, mask):
  """tk_hash of csrc/mhte_touched_kernels.h: fmix64(fid ^ tag * golden) >> 17, masked"""
  M = (1 << 64) - 1
  h = (fid ^ (tag * 0x9E3779B97F4A7C15)) & M
  h ^= h >> 33
  h = (h * 0xff51afd7ed558ccd) & M
  h ^= h >> 33
  h = (h * 0xc4ceb9fe1a85ec53) & M
  h ^= h >> 33
  return ((h >> 17) & 0xffffffff) & mask


def test_physical_worst_case_wrap_and_steal():
  C = 64                              # call limit 65; 512 slots = 2 * (65 + 65) rounded up
  mask = 511
  tail = [f for f in range(1, 200000) if _tk_slot(f, 0, mask) >= 508][:24]   # a cluster over the array end
  assert len(tail) == 24
  rest = [10**9 + i for i in range(200)]
  tks, truth = TouchedKeySet(C, name_suffix=_name()), TruthSet(C)
  for round_ in range(2):             # the second round: a fill after the steal
    first = tail[:12] + rest[:C + 1 - 12]
    assert tks.insert(ids_t(first)) == truth.insert(first)
    assert truth.stats()[0] == C + 1
    # size0 = C + 1, then max_insert new keys: C + 1 + 65 keys are in the table before the cut is applied
    second = tail[12:] + rest[100:100 + C + 1 - 12]
    assert tks.insert(ids_t(second)) == truth.insert(second) == C + 1
    _check(tks, truth, round_)
    n = truth.stats()[0]
    dev = "cuda"
    out, tg, got = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), \
        _lib.C.c_int64(-1)
    L = _lib.lib()
    st = L.mhte_touched_key_set_steal(tks.handle, _lib.vp(out), _lib.vp(tg), _lib.C.c_int64(n - 1),
                                      _lib.C.byref(got), None)
    assert st == _lib.MHTE_INVALID_ARGUMENT
    _check(tks, truth, "a steal with too small a buffer leaves the set untouched")
    _lib.check(L.mhte_touched_key_set_steal(tks.handle, _lib.vp(out), _lib.vp(tg), _lib.C.c_int64(n),
                                            _lib.C.byref(got), None))
    torch.cuda.synchronize()
    assert got.value == n
    assert sorted(zip(out.cpu().tolist(), tg.cpu().tolist())) == truth.steal()
    _check(tks, truth)
    _lib.check(L.mhte_touched_key_set_steal(tks.handle, _lib.vp(out), None, _lib.C.c_int64(0),
                                            _lib.C.byref(got), None))
    assert got.value == 0              # empty
    assert tks.steal().numel() == 0


# ------------------------------------------------------------------------------------------ 7
def _two_tables(hash_filter=None, thr=0, opt=None):
  occ = entry.SlotOccurrenceThresholdConfig(default_occurrence_threshold=thr) if thr else None
  cfgs = {}
  for name, dim in (("a", 4), ("b", 8)):
    kw = {"slot_occurrence_threshold_config": occ} if occ is not None else {}
    cfgs[name] = entry.make_table_config(
        [entry.CombineAsSegment(dim, entry.ZerosInitializer(), opt or entry.SgdOptimizer(0.5))], **kw)
  return MultiHashTable.from_configs(cfgs, name_suffix=_name(), hash_filter=hash_filter)


def _grads(n, dim):
  return torch.full((n, dim), 0.25, dtype=torch.float32, device="cuda")


def test_classic_ops_record_and_reads_do_not():
  mt = _two_tables()
  tks = TouchedKeySet(4096, name_suffix=_name())
  mt.set_touched_key_set(tks)
  a = [5, 6, 5, -1, 7, 6]
  b = [5, 100, 100]
  mt.apply_gradients({"a": (ids_t(a), _grads(len(a), 4)), "b": (ids_t(b), _grads(len(b), 8))})
  assert _pairs(tks) == sorted({(x, 0) for x in a} | {(x, 1) for x in b})
  # reads and plain writes record nothing
  mt.lookup({"a": ids_t([5, 9]), "b": ids_t([100])})
  mt.assign({"a": (ids_t([40]), _grads(1, 4))})
  mt.assign_add({"b": (ids_t([41]), _grads(1, 8))})
  assert tks.stats()[0] == 0
  # the fused update: [shard][table] segments of distinct ids
  ids = ids_t([1, 2, 3, 11, 12])
  fss = np.array([3, 2], dtype=np.int32)
  ko = np.array([0, 3, 5], dtype=np.int32)
  go = np.array([0, 12, 28], dtype=np.int32)
  g = torch.full((28,), 0.5, dtype=torch.float32, device="cuda")
  for unique in (True, False):
    mt.fused_apply_gradient(ids, None, fss, g, ko, go, 0, 0, 1, ids_unique_per_segment=unique)
    assert _pairs(tks) == [(1, 0), (2, 0), (3, 0), (11, 1), (12, 1)], unique
  _, status = mt.reinitialize("b", ids_t([100, 777]))
  assert _pairs(tks) == [(100, 1), (777, 1)]
  # detached: nothing is recorded any more
  mt.set_touched_key_set(None)
  mt.apply_gradients({"a": (ids_t([5]), _grads(1, 4))})
  assert tks.stats()[:3] == (0, 0, 0)
  mt.close()


def test_filtered_table_records_what_it_holds_after_the_update():
  flt = HashFilter(capacity=1000, split_num=5)
  mt = _two_tables(hash_filter=flt, thr=2)
  tks = TouchedKeySet(4096, name_suffix=_name())
  mt.set_touched_key_set(tks)
  a, b = [21, 22, 23], [31, 32]
  # the filter drops an occurrence of an absent id while the count seen BEFORE it is below the threshold
  # (hash_filter.h ShouldBeFiltered): the two occurrences of the first pass raise the count to 2 and are
  # both dropped, the second pass finds 2 and is admitted
  first = {"a": (ids_t(a + a), _grads(6, 4)), "b": (ids_t(b + b), _grads(4, 8))}
  batch = {"a": (ids_t(a), _grads(3, 4)), "b": (ids_t(b), _grads(2, 8))}
  mt.apply_gradients(first)           # below the threshold: the tables hold nothing, nothing is recorded
  assert not mt.contains("a", ids_t(a)).any() and not mt.contains("b", ids_t(b)).any()
  assert tks.stats()[0] == 0
  mt.apply_gradients(batch)           # the second pass admits them
  assert mt.contains("a", ids_t(a)).all() and mt.contains("b", ids_t(b)).all()
  assert _pairs(tks) == sorted([(x, 0) for x in a] + [(x, 1) for x in b])
  mt.close()


# ------------------------------------------------------------------------------------------ 8
def _batches(seed, B, steps):
  rng = np.random.default_rng(seed)
  return [rng.integers(0, 700, B).astype(np.int64) | (1 << 40) for _ in range(steps + 1)]


def test_single_table_step_records_its_unique_ids():
  from monolith_amd.fused_step import SparseStep
  mt = _two_tables(opt=entry.AdagradOptimizer(0.01, 0.1))
  tks = TouchedKeySet(8192, name_suffix=_name())
  mt.set_touched_key_set(tks)
  B = 300
  bs = _batches(3, B, 3)
  dev = [ids_t(x) for x in bs]
  step = SparseStep(mt, "b", B)
  for s in range(3):
    step.forward(dev[s], next_ids=dev[s + 1])
    step.backward(_grads(B, 8), 1_700_000_000 + s)
  want = sorted((int(x), 1) for x in np.unique(np.concatenate(bs[:3])))
  assert _pairs(tks) == want
  mt.close()


def test_multi_step_records_and_touched_entries():
  from monolith_amd.fused_step import MultiSparseStep
  mt = _two_tables(opt=entry.AdagradOptimizer(0.01, 0.1))
  tks = TouchedKeySet(8192, name_suffix=_name())
  mt.set_touched_key_set(tks)
  B = 300
  ba, bb = _batches(5, B, 3), _batches(6, B, 3)
  rags = [mt.get_ragged_id({"a": ids_t(ba[s]), "b": ids_t(bb[s])}) for s in range(4)]
  step = MultiSparseStep(mt, B)
  for s in range(3):
    step.forward(rags[s], rags[s + 1])
    step.backward(torch.full((B * 12,), 0.125, dtype=torch.float32, device="cuda"), 1_700_000_000 + s)
  ua, ub = np.unique(np.concatenate(ba[:3])), np.unique(np.concatenate(bb[:3]))
  assert tks.stats()[:3] == (ua.size + ub.size, 0, 0)
  got = mt.touched_entries()
  assert tks.stats()[0] == 0
  assert sorted(got) == ["a", "b"]
  for name, u in (("a", ua), ("b", ub)):
    ids, dumps = got[name]
    order = np.argsort(ids.cpu().numpy())
    np.testing.assert_array_equal(ids.cpu().numpy()[order], u)
    ref = mt.lookup_entry({name: ids_t(u)})[name]
    assert [dumps[i] for i in order] == ref and all(len(d) > 0 for d in ref)
  # a table that holds no batch in a step contributes nothing (its unique count is stale)
  r1 = mt.get_ragged_id({"a": ids_t(ba[0][:10])})
  step.forward(r1)
  step.backward(torch.full((10 * 4,), 0.125, dtype=torch.float32, device="cuda"), 1_700_000_010)
  assert _pairs(tks) == sorted((int(x), 0) for x in np.unique(ba[0][:10]))
  # detached: a further step leaves the set's stats unchanged
  mt.set_touched_key_set(None)
  before = tks.stats()
  step.forward(rags[0])
  step.backward(torch.full((B * 12,), 0.125, dtype=torch.float32, device="cuda"), 1_700_000_011)
  assert tks.stats() == before
  step.close()
  mt.close()


def test_refusals():
  from monolith_amd.distributed_ps_sync import ShardedMultiStep
  from monolith_amd.fused_step import MultiSparseStep
  L = _lib.lib()
  # the id-sharded step refuses a table with a set
  mt = _two_tables(opt=entry.AdagradOptimizer(0.01, 0.1))
  tks = TouchedKeySet(256, name_suffix=_name())
  sharded = ShardedMultiStep(mt, 64)  # ... and a table with an id-sharded step refuses a set
  with pytest.raises(_lib.InvalidArgumentError):
    mt.set_touched_key_set(tks)
  sharded.close()
  mt.set_touched_key_set(tks)
  with pytest.raises(_lib.InvalidArgumentError):
    ShardedMultiStep(mt, 64)
  # one set serves one MultiHashTable
  other = _two_tables()
  with pytest.raises(_lib.InvalidArgumentError):
    other.set_touched_key_set(tks)
  other.close()
  mt.close()                          # destroying the table detaches: the set can serve another
  # filter + set: the multi step is refused at its creation ...
  flt = HashFilter(capacity=1000, split_num=5)
  mf = _two_tables(hash_filter=flt, thr=2)
  mf.set_touched_key_set(tks)
  with pytest.raises(_lib.InvalidArgumentError):
    MultiSparseStep(mf, 64)
  # ... the single-table step at the call (before it looks at the batch) ...
  C = _lib.C
  st = L.mhte_table_step_backward(mf.handle, C.c_int32(0), None, None, None, C.c_int64(0), None, None, C.c_int64(0),
                                  None, None, C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), None)
  assert st == _lib.MHTE_INVALID_ARGUMENT and b"touched-key set" in L.mhte_last_error()
  # ... and, with a multi step alive, at attach
  mf.set_touched_key_set(None)
  step = MultiSparseStep(mf, 64)
  with pytest.raises(_lib.InvalidArgumentError):
    mf.set_touched_key_set(tks)
  step.close()
  mf.set_touched_key_set(tks)         # no step any more: the op-level paths can record
  tks.close()                         # destroying the set detaches
  mf.apply_gradients({"a": (ids_t([1]), _grads(1, 4))})
  mf.close()


# ------------------------------------------------------------------------------------------ 9
def test_cut_inside_a_multi_segment_call():
  """One insert call over the device-resident descriptors of two tables (2 x 75 positions <= C + 1), with the
  clear falling between the segments: table a's single new id fills the set to C + 1, so the first id of table
  b finds it over capacity.  Whatever order the step's dedup gives the unique ids, the set afterwards is
  exactly table b's ids.  Then a step in which table a holds no batch (its skip bit)."""
  from monolith_amd.fused_step import MultiSparseStep
  B, C = 75, 150
  mt = _two_tables(opt=entry.AdagradOptimizer(0.01, 0.1))
  tks, truth = TouchedKeySet(C, name_suffix=_name()), TruthSet(C)
  mt.set_touched_key_set(tks)
  step = MultiSparseStep(mt, B)

  def run(a, b, s):
    batch = {}
    if len(a):
      batch["a"] = ids_t(a)
    if len(b):
      batch["b"] = ids_t(b)
    step.forward(mt.get_ragged_id(batch))
    step.backward(torch.full((len(a) * 4 + len(b) * 8,), 0.125, dtype=torch.float32, device="cuda"),
                  1_700_000_000 + s)
    truth.insert_segments([(sorted(set(a)), 0), (sorted(set(b)), 1)])
    _check(tks, truth, s)

  run(list(range(1000, 1075)), list(range(2000, 2075)), 0)     # 150 keys = C: no clear
  assert truth.stats() == (150, 0, 0, C)
  b2 = [3000 + (i % 40) for i in range(75)]                    # 40 distinct ids, with duplicates
  run([5000], b2, 1)                                           # 5000 fills to C + 1; b's first id clears
  assert truth.stats() == (40, 151, 1, C)
  assert _pairs(tks) == truth.steal() == [(3000 + i, 1) for i in range(40)]
  run(list(range(1000, 1075)), [], 2)
  run([], list(range(2000, 2060)), 3)                          # a's descriptor is skipped: its count is stale
  assert _pairs(tks) == truth.steal()
  step.close()
  mt.close()


# ----------------------------------------------------------------------------------------- 10
def test_max_insert_bounds_a_call():
  """max_insert = 16 at C = 64: the host cuts every input into calls of 16 positions (256 slots instead of
  512); the state is the key-by-key one all the same."""
  C = 64
  tks, truth = TouchedKeySet(C, name_suffix=_name(), max_insert=16), TruthSet(C)
  rng = np.random.default_rng(5)
  for call, n in enumerate([15, 16, 17, 100, 0, 65, 33, 259, 1, 64]):
    ids = rng.integers(0, 2 * C + 3, n).astype(np.int64)
    assert tks.insert(ids_t(ids)) == truth.insert(ids.tolist()), (call, n)
    _check(tks, truth, (call, n))
  assert truth.stats()[2] >= 2
  assert _pairs(tks) == truth.steal()
  # through a device-side count as well: the cut pieces each honour it
  ids = list(range(500, 540))
  tks.insert_async(ids_t(ids), n_dev=torch.tensor([21], dtype=torch.int32, device="cuda"))
  truth.insert(ids[:21])
  _check(tks, truth)
  assert _pairs(tks) == truth.steal()


# ----------------------------------------------------------------------------------------- 11
def test_consecutive_calls_on_different_streams_are_ordered():
  """Calls alternate between two streams with no host synchronisation in between; each depends on the state
  the one before left (the fill, then the call that finds the set over capacity), so the event the set
  records between them is what makes the result the sequential one."""
  C = 257
  tks, truth = TouchedKeySet(C, name_suffix=_name()), TruthSet(C)
  rng = np.random.default_rng(9)
  streams = [torch.cuda.Stream(), torch.cuda.Stream()]
  batches = [rng.integers(0, 3 * C, C + 1).astype(np.int64) for _ in range(12)]
  dev = [ids_t(b) for b in batches]
  torch.cuda.synchronize()
  for k, b in enumerate(batches):
    with torch.cuda.stream(streams[k % 2]):
      tks.insert_async(dev[k])
    truth.insert(b.tolist())
  torch.cuda.synchronize()
  assert truth.stats()[2] >= 3
  _check(tks, truth)
  assert _pairs(tks) == truth.steal()
