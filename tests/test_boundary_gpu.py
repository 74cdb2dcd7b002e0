"""GPU tests (-m gpu) of the boundary pieces a TF shim needs beyond the hot path: the serialized
config protos of the create ops, LookupEntry, FeatureStat, the resource registry, the RandomUniform
initializer, and the compiled plain-C client of tests/c_client.c."""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from monolith_amd import _lib, entry  # noqa: E402
from monolith_amd.multi_hash_table_ops import HashFilter, MultiHashTable  # noqa: E402
from tests import ckpt_proto as P  # noqa: E402
from tests.test_abi import build_c_client  # noqa: E402

_counter = [0]


def _name():
  _counter[0] += 1
  return "bd%d" % _counter[0]


def ids_t(x):
  return torch.as_tensor(np.asarray(x, dtype=np.int64)).cuda()


def val_t(x):
  return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda()


def _multi_config():
  m = P.MultiEmbeddingHashTableConfig()
  # given out of order on purpose: tables are kept sorted by name
  for name in ("vec", "bias", "emb"):
    m.names.append(name)
    c = m.configs.add()
    c.cuckoo.SetInParent()
    if name == "bias":        # SGD lr 1 (test_utils.generate_test_hash_table_config)
      s = c.entry_config.segments.add()
      s.dim_size = 2
      s.init_config.ones.dim_size = 2
      s.opt_config.sgd.learning_rate = 1.0
      c.initial_capacity = 64
    elif name == "emb":       # adagrad_optimizer_test.cc:32-60 KAT
      s = c.entry_config.segments.add()
      s.dim_size = 2
      s.init_config.zeros.dim_size = 2
      s.opt_config.adagrad.initial_accumulator_value = 1.0
      s.opt_config.adagrad.learning_rate = 0.1
      c.slot_expire_time_config.default_expire_time = 14
      e = c.slot_expire_time_config.slot_expire_times.add()
      e.slot, e.expire_time = 1, 5
      c.enable_feature_eviction = True
      c.feature_evict_every_n_hours = 2
    else:                     # FTRL bias + Adam vector, constants / random-uniform init
      s = c.entry_config.segments.add()
      s.dim_size = 4
      s.init_config.constants.constant = 0.25
      s.opt_config.ftrl.learning_rate = 0.05
      s.opt_config.ftrl.beta = 1.0
      s.opt_config.ftrl.l1_regularization_strength = 0.001
      s = c.entry_config.segments.add()
      s.dim_size = 8
      s.init_config.random_uniform.minval = -0.5
      s.init_config.random_uniform.maxval = 0.5
      s.opt_config.adam.learning_rate = 0.02
      s.opt_config.adam.use_nesterov = True
  return m


def test_create_from_serialized_config_and_kats():
  m = _multi_config()
  mt = MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name())
  assert mt.table_names == ("bias", "emb", "vec")
  assert mt.get_table_dim_sizes() == (2, 2, 12)
  np.testing.assert_allclose(mt.learning_rate, [1.0, 0.1, 0.05, 0.02])
  assert MultiHashTable.is_initialized(mt.shared_name) and not MultiHashTable.is_initialized("nope")
  # absent ids read as zeros whatever the initializer; SGD lr 1 on a ones-initialised row
  assert not mt.lookup({"bias": ids_t([5])})["bias"].any().item()
  mt.apply_gradients({"bias": (ids_t([5]), val_t([[0.5, 2.0]]))})
  np.testing.assert_array_equal(mt.lookup({"bias": ids_t([5])})["bias"].cpu().numpy(), [[0.5, -1.0]])
  # Adagrad KAT: init_acc 1, lr .1, g {1,2} -> {-0.07071068, -0.08944272}
  mt.apply_gradients({"emb": (ids_t([9]), val_t([[1.0, 2.0]]))})
  np.testing.assert_allclose(mt.lookup({"emb": ids_t([9])})["emb"].cpu().numpy(),
                             [[-0.07071068, -0.08944272]], rtol=0, atol=1e-7)
  # the two-segment table against the oracle (constants-initialised FTRL; the Adam part starts
  # from a random-uniform draw, so only its FTRL half is compared)
  ot = O.Table([O.segment(4, O.OPT_FTRL, p=(0.1, 1.0, 0.001, 0.0), init=O.INIT_CONSTANT, init_value=0.25),
                O.segment(8, O.OPT_ADAM, p=(0.9, 0.99, 0.01, 0.0, 1.0))], 1)
  g = np.linspace(-1, 1, 12, dtype=np.float32)[None, :]
  mt.apply_gradients({"vec": (ids_t([77]), val_t(g))})
  ot.optimize(np.array([77], np.int64), g, [0.05, 0.02], 0)
  got = mt.lookup({"vec": ids_t([77])})["vec"].cpu().numpy()
  np.testing.assert_array_equal(got[:, :4], ot.lookup(np.array([77], np.int64))[0][:, :4])
  # eviction config came through: ttl 5 days for slot 1
  st = mt.stats("emb")
  assert st.size == 1


def test_a_table_created_from_the_serialized_config_runs_adagrad_as_the_reference_is_built():
  """the reference's build dispatches AdagradOptimize to its AVX2 form (avx_utils.h:96-119:
  fused multiply-adds; with a weight decay the weight step uses the raw gradient inside each block of
  8).  A table created from the serialized config — the reference's own op input — defaults to that
  form: the same bits as entry.AdagradOptimizer(avx_semantics=True) (itself pinned to the reference's
  -mavx2 -mfma build, test_adagrad_avx_form_matches_the_reference_as_built), and NOT the scalar
  loop's when a weight decay is set."""
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("t")
  c = m.configs.add()
  c.cuckoo.SetInParent()
  s = c.entry_config.segments.add()
  s.dim_size = 20                       # two blocks of 8 + the scalar tail
  s.init_config.zeros.dim_size = 20
  s.opt_config.adagrad.learning_rate = 0.05
  s.opt_config.adagrad.initial_accumulator_value = 0.1
  s.opt_config.adagrad.weight_decay_factor = 0.1
  mt = MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name())
  mk = lambda avx: MultiHashTable.from_configs({"t": entry.make_table_config([entry.CombineAsSegment(  # noqa: E731
      20, entry.ZerosInitializer(), entry.AdagradOptimizer(0.05, 0.1, weight_decay_factor=0.1, avx_semantics=avx))])},
                                                name_suffix=_name())
  ref_avx, ref_scalar = mk(True), mk(False)
  rng = np.random.default_rng(11)
  ids = np.arange(1, 301, dtype=np.int64)
  for _ in range(3):
    g = val_t(rng.standard_normal((ids.size, 20)).astype(np.float32))
    for t in (mt, ref_avx, ref_scalar):
      t.apply_gradients({"t": (ids_t(ids), g)})
  w = mt.lookup({"t": ids_t(ids)})["t"]
  assert torch.equal(w, ref_avx.lookup({"t": ids_t(ids)})["t"])
  assert not torch.equal(w, ref_scalar.lookup({"t": ids_t(ids)})["t"])


def test_lookup_gradient_kat():
  """MonolithHashTableLookupGradient (hash_table_lookup_op.cc:110-147): ids pass through, the gradient
  row of entry i is input_grads[id_indices[i, 0]]; float4 and odd dims; a row outside the gradient
  matrix is InvalidArgument; the two inputs must agree in length (the op's own check)."""
  from monolith_amd.distribution_ops import lookup_gradient
  rng = np.random.default_rng(2)
  for dim in (1, 5, 16, 64):
    rows, n = 37, 1000
    idx = np.stack([rng.integers(0, rows, n), rng.integers(0, 9, n)], axis=1).astype(np.int64)
    ids = rng.integers(-2**62, 2**62, n).astype(np.int64)
    g = rng.standard_normal((rows, dim)).astype(np.float32)
    out_ids, out = lookup_gradient(ids_t(idx), ids_t(ids), val_t(g))
    np.testing.assert_array_equal(out_ids.cpu().numpy(), ids)
    np.testing.assert_array_equal(out.cpu().numpy(), g[idx[:, 0]])
  e_ids, e = lookup_gradient(ids_t(np.zeros((0, 2))), ids_t([]), val_t(np.zeros((3, 4))))
  assert e_ids.numel() == 0 and tuple(e.shape) == (0, 4)
  with pytest.raises(_lib.InvalidArgumentError, match="outside"):
    lookup_gradient(ids_t([[0, 0], [3, 0]]), ids_t([7, 8]), val_t(np.ones((3, 4))))
  with pytest.raises(_lib.InvalidArgumentError, match="should be same"):
    lookup_gradient(ids_t([[0, 0]]), ids_t([7, 8]), val_t(np.ones((3, 4))))


def test_save_as_tensor_hands_out_the_reserved_key_once():
  """The id INT64_MIN lives in the engine's side slot (its bucket-empty marker); the reference's map holds
  it in a bucket like any other key and partial_dump returns it.  The walk hands it out behind the last
  bucket of shard 0, once, whatever the limit — so a dump holds size() entries."""
  dim = 4
  mt = MultiHashTable.from_configs({"t": entry.make_table_config(
      [entry.CombineAsSegment(dim, entry.ZerosInitializer(), entry.SgdOptimizer(0.1))],
      entry.CuckooHashTableConfig(initial_capacity=1 << 6))}, name_suffix=_name())
  ids = np.array([np.iinfo(np.int64).min, 3, 17, 1 << 40, -5, 99], np.int64)
  vals = np.arange(ids.size * dim, dtype=np.float32).reshape(-1, dim)
  mt.assign({"t": (ids_t(ids), val_t(vals))}, req_time=77)
  assert mt.size("t") == ids.size
  strings = dict(zip(ids.tolist(), mt.lookup_entry({"t": ids_t(ids)})["t"]))
  for total, limit in ((1, 1000), (1, 2), (3, 1), (2, 0), (1, 6), (1, 5)):
    got = []
    for shard in range(total):
      offset = 0
      for _ in range(64):
        new_offset, ents = mt.save_as_tensor("t", shard, total, limit, offset)
        got += ents
        if len(ents) < max(limit, 1):
          break
        offset = new_offset
      # a walk that has run off the end stays there
      assert mt.save_as_tensor("t", shard, total, limit, new_offset)[1] == []
    assert sorted(got) == sorted(strings.values()), (total, limit)


def test_save_as_tensor_walks_the_table_like_partial_dump():
  """MonolithHashTableSaveAsTensor (ops/hash_table/misc_ops.cc:46-94) = cuckoohash_map::partial_dump
  (cuckoohash_map.hpp:740-773) `limit` entries at a time: ids inserted one by one sit where the
  reference map puts them (the oracle's dump gives (bucket * 4 + slot) of every key), so the sequence
  of (new_offset, ids) of every call is checked against that walk restated here — over 1 and 3 shards,
  limits that do and do not divide the counts, a limit of 0 (one entry, as the reference's count check
  comes after the entry) — and every string is the id's LookupEntry string.  The reference's own test
  (hash_table_ops_test.py:116-126): assign 3 ids, dump with limit 1000, every string parses."""
  dim, n = 4, 300
  mt = MultiHashTable.from_configs({"t": entry.make_table_config(
      [entry.CombineAsSegment(dim, entry.ZerosInitializer(), entry.AdagradOptimizer(0.05, 0.1))],
      entry.CuckooHashTableConfig(initial_capacity=1 << 10))}, name_suffix=_name())
  ot = O.Table(O.segment(dim, O.OPT_ADAGRAD, p=(0.1, 0.0)), 1 << 10)
  rng = np.random.default_rng(9)
  ids = rng.choice(1 << 40, n, replace=False).astype(np.int64)
  for k, i in enumerate(ids):      # one by one: placement is the reference's
    v = rng.standard_normal((1, dim)).astype(np.float32)
    mt.assign({"t": (ids_t([i]), val_t(v))}, req_time=1000 + k)
    ot.assign(np.array([i]), v, 1000 + k)
  o_ids, o_pos, _, _ = ot.dump()
  hp = ot.hashpower()
  assert int(mt.stats("t").hashpower) == hp
  order = np.argsort(o_pos)
  o_ids, o_pos = o_ids[order], o_pos[order]
  strings = dict(zip(ids.tolist(), mt.lookup_entry({"t": ids_t(ids)})["t"]))

  def walk(shard, total, limit, offset):   # partial_dump restated on the oracle's positions
    hs = 1 << hp
    Q, R = divmod(hs, total)
    begin = shard * Q + min(shard, R)
    end = begin + Q + (1 if shard < R else 0)
    lo, hi = begin * 4 + offset, end * 4
    got, count = [], 0
    for key, pos in zip(o_ids, o_pos):
      if pos < lo or pos >= hi:
        continue
      got.append(int(key))
      count += 1
      if count >= limit:
        return pos - begin * 4 + 1, got
    return (end - begin + 1) * 4, got

  seen = []
  for total, limit in ((1, 1000), (1, 7), (3, 16), (3, 0), (5, 1)):
    got_all = []
    for shard in range(total):
      offset, calls = 0, 0
      while True:
        new_offset, ents = mt.save_as_tensor("t", shard, total, limit, offset)
        exp_offset, exp_ids = walk(shard, total, limit, offset)
        assert new_offset == exp_offset, (total, limit, shard, offset)
        assert ents == [strings[i] for i in exp_ids], (total, limit, shard, offset)
        got_all += exp_ids
        calls += 1
        if len(ents) < max(limit, 1):
          break
        offset = new_offset
      assert calls >= 1
    assert sorted(got_all) == sorted(ids.tolist()), (total, limit)
    seen.append(len(got_all))
  assert seen == [n] * 5
  # the reference's own test: three ids, one call, strings that parse
  small = MultiHashTable.from_configs({"s": entry.make_table_config(
      [entry.CombineAsSegment(1, entry.ZerosInitializer(), entry.SgdOptimizer(1.0))])}, name_suffix=_name())
  small.assign({"s": (ids_t([0, 1, 2]), val_t([[0.1], [0.2], [0.3]]))})
  _, dump = small.save_as_tensor("s", 0, 1, 1000, 0)
  nums = []
  for d in dump:
    e = P.EntryDump()
    e.ParseFromString(d)
    nums.append((e.id, list(e.num)))
  assert sorted(nums) == [(0, [np.float32(0.1)]), (1, [np.float32(0.2)]), (2, [np.float32(0.3)])]
  with pytest.raises(_lib.InvalidArgumentError):
    small.save_as_tensor("s", 2, 2, 10, 0)


def test_serialized_config_stochastic_rounding_float16():
  """OptimizerConfig.stochastic_rounding_float16 (optimizer.proto:228) in the serialized config: the
  segment's weights are binary16 values after an update, the other segment's are not rounded; on a
  group_adagrad segment the flag is refused."""
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("t")
  c = m.configs.add()
  s = c.entry_config.segments.add()
  s.dim_size = 8
  s.opt_config.adagrad.learning_rate = 0.05
  s.opt_config.stochastic_rounding_float16 = True
  s = c.entry_config.segments.add()
  s.dim_size = 8
  s.opt_config.adagrad.learning_rate = 0.05
  mt = MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name())
  rng = np.random.default_rng(4)
  ids = np.arange(1, 257, dtype=np.int64)
  for _ in range(2):
    mt.apply_gradients({"t": (ids_t(ids), val_t(rng.standard_normal((ids.size, 16)).astype(np.float32)))})
  w = mt.lookup({"t": ids_t(ids)})["t"].cpu().numpy()
  assert (w[:, :8].astype(np.float16).astype(np.float32) == w[:, :8]).all() and w[:, :8].any()
  assert (w[:, 8:].astype(np.float16).astype(np.float32) != w[:, 8:]).mean() > 0.9
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("g")
  s = m.configs.add().entry_config.segments.add()
  s.dim_size = 4
  s.opt_config.group_adagrad.learning_rate = 0.05
  s.opt_config.stochastic_rounding_float16 = True
  with pytest.raises(_lib.InvalidArgumentError):
    MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name())


def test_serialized_config_errors():
  m = _multi_config()
  m.names.append("extra")                                # names / configs of different length
  with pytest.raises(_lib.InvalidArgumentError):
    MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name())
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("t")
  s = m.configs.add().entry_config.segments.add()
  s.dim_size = 4
  s.opt_config.dc.lambda_ = 0.1                          # not implemented (out of scope)
  with pytest.raises(_lib.InvalidArgumentError):
    MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name())
  with pytest.raises(_lib.InvalidArgumentError):
    MultiHashTable.from_serialized_config(b"\xff\xff\xff", name_suffix=_name())


def test_filter_config_proto_sets_occurrence_thresholds():
  oc = P.SlotOccurrenceThresholdConfig()
  oc.default_occurrence_threshold = 2
  e = oc.slot_occurrence_thresholds.add()
  e.slot, e.occurrence_threshold = 3, 0
  flt = HashFilter(capacity=1000, split_num=1, config=oc.SerializeToString())
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("t")
  s = m.configs.add().entry_config.segments.add()
  s.dim_size = 1
  s.opt_config.sgd.learning_rate = 1.0
  mt = MultiHashTable.from_serialized_config(m.SerializeToString(), name_suffix=_name(), hash_filter=flt)
  a, b = 11, (3 << 48) | 11
  g = val_t([[1.0], [1.0]])
  mt.apply_gradients({"t": (ids_t([a, b]), g)})          # a: first sighting, dropped; b: slot 3 -> thr 0
  assert mt.contains("t", ids_t([a, b])).cpu().tolist() == [False, True]
  mt.apply_gradients({"t": (ids_t([a, b]), g)})
  mt.apply_gradients({"t": (ids_t([a, b]), g)})          # third sighting of a: admitted
  assert mt.contains("t", ids_t([a, b])).cpu().tolist() == [True, True]


def test_random_uniform_initializer_distribution():
  cfg = entry.make_table_config([entry.CombineAsSegment(
      16, entry.RandomUniformInitializer(-0.05, 0.05), entry.SgdOptimizer(0.0))])
  mt = MultiHashTable.from_configs({"t": cfg}, name_suffix=_name())
  n = 20000
  ids = np.arange(1, n + 1, dtype=np.int64)
  assert not mt.lookup({"t": ids_t(ids)})["t"].any().item()      # lookups do not insert
  mt.apply_gradients({"t": (ids_t(ids), torch.zeros(n, 16).cuda())}, ids_unique=True)  # lr 0: w = init
  w = mt.lookup({"t": ids_t(ids)})["t"].cpu().numpy()
  assert w.min() >= -0.05 and w.max() < 0.05
  assert abs(w.mean()) < 2e-4 and abs(w.std() - 0.1 / np.sqrt(12)) < 3e-4
  assert np.unique(w).size > 0.98 * w.size                        # independent draws
  h, _ = np.histogram(w, bins=10, range=(-0.05, 0.05))
  assert h.min() > 0.09 * w.size and h.max() < 0.11 * w.size


def test_lookup_entry_and_feature_stat(tmp_path):
  cfgs = {"a": entry.make_table_config([entry.CombineAsSegment(
              3, entry.ZerosInitializer(), entry.AdagradOptimizer(0.1, 1.0))]),
          "b": entry.make_table_config([entry.CombineAsSegment(
              2, entry.ZerosInitializer(), entry.SgdOptimizer(1.0))])}
  mt = MultiHashTable.from_configs(cfgs, name_suffix=_name())
  mt.apply_gradients({"a": (ids_t([1, 2]), val_t([[1, 2, 3], [4, 5, 6]])),
                      "b": (ids_t([3]), val_t([[1, 1]]))}, req_time=1234)
  out = mt.lookup_entry({"a": ids_t([2, 99, 1]), "b": ids_t([3, 4])})
  assert [len(x) > 0 for x in out["a"]] == [True, False, True] and out["b"][1] == b""
  e = P.EntryDump.FromString(out["a"][0])
  rows = mt.lookup({"a": ids_t([2])})["a"].cpu().numpy()[0]
  assert e.id == 2 and e.last_update_ts_sec == 1234
  np.testing.assert_array_equal(np.array(e.num, np.float32), rows)
  np.testing.assert_allclose(list(e.opt.dump[0].adagrad.norm), [1 + 16, 1 + 25, 1 + 36])
  e = P.EntryDump.FromString(out["b"][0])
  assert e.id == 3 and list(e.num) == [-1.0, -1.0] and e.opt.dump[0].HasField("sgd")
  # what LookupEntry returns is what Save writes
  base = str(tmp_path / "fs" / "ck")
  mt.save(base, nshards=2)
  recs = []
  for sh in range(2):
    recs += P.unframe(P.read_tf_snappy(open("%s-%05d-of-00002" % (base, sh), "rb").read()))
  assert sorted(recs) == sorted([out["a"][0], out["a"][2], out["b"][0]])
  assert MultiHashTable.feature_stat(base) == {"a": 2, "b": 1}
  with pytest.raises(_lib.MhteError):
    MultiHashTable.feature_stat(str(tmp_path / "none"))


def test_plain_c_client_runs(tmp_path):
  exe = build_c_client(tmp_path)
  r = subprocess.run([exe, str(tmp_path / "c_ckpt")], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0 and "c_client ok" in r.stdout, r.stdout + r.stderr


# =============================================================================== sliding hash filter
# The checker is oracle.SlidingFilter (oracle/mhte_filter_oracle.c): the restatement of
# sliding_hash_filter.cc / hash_filter.h that tests/test_filter_oracle.py pins, add by add and word by
# word, to those very sources compiled in place.  defer_advance: the window moves between launches.
def SlidingModel(capacity, split_num):
  return O.SlidingFilter(capacity, split_num, defer_advance=True)


def _filter_table(flt, thr):
  cfg = entry.make_table_config(
      [entry.CombineAsSegment(1, entry.ZerosInitializer(), entry.SgdOptimizer(1.0))],
      slot_occurrence_threshold_config=entry.SlotOccurrenceThresholdConfig(default_occurrence_threshold=thr))
  return MultiHashTable.from_configs({"t": cfg}, name_suffix=_name(), hash_filter=flt)


def test_pipelined_step_consults_a_filter_with_many_splits_like_the_model():
  """The fused step's lane-group consultation (filter_consult_group) over a filter of 12 splits: it fetches the
  windows of 6 older splits at a time, so an id whose last count lies further back — or nowhere — takes the
  second pass; a single id per launch makes every add comparable with the restatement, add by add.  Counts and
  admissions against oracle.SlidingFilter while the window goes round more than once."""
  from monolith_amd.fused_step import SparseStep
  thr = 3
  flt = HashFilter(capacity=330, split_num=12)            # 12 splits of 30
  mt = _filter_table(flt, thr)
  model = SlidingModel(330, 12)
  rng = np.random.default_rng(11)
  universe = (rng.integers(1, 2**40, 1200).astype(np.int64) | (1 << 48))
  seq = []
  for k in range(900):
    # a drifting working set with a long memory: ids come back after the window has moved many splits on
    lo = k // 2
    back = int(rng.integers(0, 60)) if rng.random() < 0.7 else int(rng.integers(0, 400))
    seq.append(int(universe[max(0, lo + 30 - back)]))
  dev = [ids_t([f]) for f in seq] + [ids_t([seq[-1]])]
  step = SparseStep(mt, "t", 1, exact_order=True)
  g1 = val_t([[1.0]])
  admitted = set()
  for i, fid in enumerate(seq):
    step.forward(dev[i], next_ids=dev[i + 1])
    step.backward(g1, 1_700_000_000 + i)
    if fid not in admitted:
      if model.add(fid, 1) >= thr:
        admitted.add(fid)
      model.advance_if_full()
    if i % 150 == 149 or i == len(seq) - 1:
      probe = np.unique(np.array(seq[:i + 1], dtype=np.int64))
      got = flt.get(ids_t(probe)).cpu().numpy()
      np.testing.assert_array_equal(got, [model.get(int(x)) for x in probe], err_msg="step %d" % i)
      present = mt.contains("t", ids_t(probe)).cpu().numpy()
      np.testing.assert_array_equal(present, [int(x) in admitted for x in probe])
  st = model.state()
  assert st["head_increment"] > 12 and len(admitted) > 20


def test_sliding_hash_filter_window_against_model(tmp_path):
  """Ids seen again and again while the window moves on (capacity 300 -> 5 splits of 75): counts
  carry over from older splits, fall out of the window after nsplit - 2 moves, and the table admits
  an id exactly when the model's count reaches the threshold.  Then save -> restore into a fresh
  filter -> the same counts, and the two keep agreeing."""
  thr = 3
  flt = HashFilter(capacity=300, split_num=5)
  mt = _filter_table(flt, thr)
  model = SlidingModel(300, 5)
  rng = np.random.default_rng(9)
  universe = (rng.integers(1, 2**40, 900).astype(np.int64) | (1 << 48))
  admitted = set()
  g1 = val_t([[1.0]])

  def step(fid):
    mt.apply_gradients({"t": (ids_t([fid]), g1)})
    if fid not in admitted:                      # (tf_bridge.cc:315-321: the filter is asked only
      if model.add(fid, 1) >= thr:               #  about ids the table does not hold)
        admitted.add(fid)
      model.advance_if_full()

  seq = []
  for k in range(1000):
    # a slowly drifting working set: old ids return for a while, then never again
    lo = k // 2
    seq.append(int(universe[lo + int(rng.integers(0, 60))]))
  for i, fid in enumerate(seq):
    step(fid)
    if i % 100 == 99 or i == len(seq) - 1:
      probe = np.unique(np.array(seq[:i + 1], dtype=np.int64))
      got = flt.get(ids_t(probe)).cpu().numpy()
      np.testing.assert_array_equal(got, [model.get(int(x)) for x in probe], err_msg="step %d" % i)
      present = mt.contains("t", ids_t(probe)).cpu().numpy()
      np.testing.assert_array_equal(present, [int(x) in admitted for x in probe])
  st = model.state()
  assert st["head_increment"] > len(st["num_elements"])   # the window went round more than once
  base = str(tmp_path / "flt" / "filter")
  flt.save(base)
  assert sorted(os.listdir(tmp_path / "flt")) == ["filter-%05d-of-00005" % i for i in range(5)]
  # the files hold the reference's messages, and the device's words ARE the reference's uint16
  # words: every split, slot for slot, equals the restatement's (which test_filter_oracle.py pins to
  # the compiled reference) — independent TFRecord + protobuf-runtime reader
  ref = O.RefSlidingFilter(300, 5) if O.ref_filter_available() else None
  for sp in range(5):
    meta, words = P.read_filter_split("%s-%05d-of-00005" % (base, sp))
    np.testing.assert_array_equal(words, model.split_words(sp), err_msg="split %d" % sp)
    sl = meta.sliding_hash_filter_meta
    assert (meta.total_size, meta.num_elements, meta.fill_rate) == (90, st["num_elements"][sp], 1.2)
    assert (sl.split_num, sl.max_forward_step, sl.max_backward_step, sl.max_step, sl.head, sl.head_increment) == (
        5, 2, 3, 16, st["head"], st["head_increment"])
    if ref is not None:   # ... and the reference's own Restore takes them
      assert ref.restore_split(sp, {"failure_count": meta.failure_count, "total_size": meta.total_size,
                                    "num_elements": meta.num_elements, "fill_rate_e6": 1200000,
                                    "split_num": sl.split_num, "max_forward_step": sl.max_forward_step,
                                    "max_backward_step": sl.max_backward_step, "max_step": sl.max_step,
                                    "head": sl.head, "head_increment": sl.head_increment,
                                    "sliding_failure_count": sl.failure_count}, words)
  if ref is not None:
    probe = np.unique(np.array(seq, dtype=np.int64))
    np.testing.assert_array_equal(ref.get_many(probe.astype(np.uint64)), flt.get(ids_t(probe)).cpu().numpy())
  flt2 = HashFilter(capacity=300, split_num=5)
  flt2.restore(base)
  probe = np.unique(np.array(seq, dtype=np.int64))
  np.testing.assert_array_equal(flt2.get(ids_t(probe)).cpu().numpy(), flt.get(ids_t(probe)).cpu().numpy())
  mt2 = _filter_table(flt2, thr)
  for fid in seq[-50:] + [int(x) for x in universe[400:430]]:
    mt.apply_gradients({"t": (ids_t([fid]), g1)})
    if fid not in admitted:
      mt2.apply_gradients({"t": (ids_t([fid]), g1)})
  probe2 = np.unique(np.concatenate([probe, universe[400:430]]))
  mask = np.array([int(x) not in admitted for x in probe2])
  np.testing.assert_array_equal(flt2.get(ids_t(probe2)).cpu().numpy()[mask],
                                flt.get(ids_t(probe2)).cpu().numpy()[mask])
  with pytest.raises(_lib.MhteError):             # geometry is validated (RestoreMetaDump)
    HashFilter(capacity=300, split_num=7).restore(base)
  with pytest.raises(_lib.MhteError):
    HashFilter(capacity=300, split_num=5).restore(str(tmp_path / "flt" / "absent"))


def _device_add(mt, ids_with_multiplicity):
  """add(fid, k) for every distinct fid occurring k times: an update of a table whose threshold (100)
  no 4-bit count reaches, so every occurrence is dropped and counted (tf_bridge.cc:300-321)."""
  n = len(ids_with_multiplicity)
  mt.apply_gradients({"t": (ids_t(ids_with_multiplicity), torch.zeros((n, 1), device="cuda"))})


def test_sliding_hash_filter_reference_kats():
  """sliding_hash_filter_test.cc:27-41 (test_simple), :43-62 (test_count), :101-111
  (SkipZeroThresholdFeatures) on the device filter."""
  for key_num in (1, 3, 100):
    flt = HashFilter(capacity=key_num, split_num=10)
    mt = _filter_table(flt, 100)
    for i in range(17):
      assert int(flt.get(ids_t([1]))[0]) == min(i, 15)
      _device_add(mt, [1])
    assert int(flt.get(ids_t([1]))[0]) == 15
  flt = HashFilter(capacity=1000000, split_num=10)
  mt = _filter_table(flt, 100)
  big = 10000002961562801052 - (1 << 64)
  for c in (1, 20, 1):
    _device_add(mt, [big] * c)
  assert int(flt.get(ids_t([big]))[0]) == 15
  meta_total = sum(int(x) for x in flt.num_elements())
  assert meta_total == 1
  # threshold 0 never consults the filter, threshold 1 drops the first sighting
  flt = HashFilter(capacity=1000000, split_num=10)
  cfg0 = entry.make_table_config(
      [entry.CombineAsSegment(1, entry.ZerosInitializer(), entry.SgdOptimizer(1.0))],
      slot_occurrence_threshold_config=entry.SlotOccurrenceThresholdConfig(default_occurrence_threshold=0))
  mt0 = MultiHashTable.from_configs({"t": cfg0}, name_suffix=_name(), hash_filter=flt)
  mt1 = _filter_table(flt, 1)
  zero_thr = ids_t([0, 1, 2, 3, 4])
  normal = ids_t([0, 2, 4, 6, 8])
  g = torch.ones((5, 1), device="cuda")
  mt0.apply_gradients({"t": (zero_thr, g)})
  mt1.apply_gradients({"t": (normal, g)})
  assert mt0.contains("t", zero_thr).cpu().numpy().all()             # not filtered
  assert not mt1.contains("t", normal).cpu().numpy().any()           # filtered: seen 0 < 1 times before
  assert sum(int(x) for x in flt.num_elements()) == 5                # only the normal fids were counted


def test_sliding_hash_filter_conflict_rate_kat():
  """sliding_hash_filter_test.cc:64-99 compare_to_unordered_map(1 000 000 keys, capacity 1 000 000,
  10 splits): the reference expects 0.908 % (+- half) of the filter's counts to differ from an exact
  map — aliasing of 12-bit signatures over 16 probe positions — and fewer than keys / 10 000 probe
  failures.  The device filter must land in the same band, and agree with the restatement fed the
  same launches (the window moves between launches on both).  Launches of 5 000 ids: the one
  documented difference — the head split can overfill by one launch's new ids before the window
  moves — is then 4.5 % of a split (with 25 000 per launch the rate is 1.41 % on the device and on the
  deferred restatement alike, against 1.08 % for the reference's add-by-add window)."""
  cap, keys, per = 1000000, 1000000, 5000
  flt = HashFilter(capacity=cap, split_num=10)
  mt = _filter_table(flt, 100)
  model = O.SlidingFilter(cap, 10, defer_advance=True)
  rng = np.random.default_rng(cap)
  counter = {}
  for b in range(keys // per):
    draw = rng.integers(0, 2**31 - 1, per)
    uniq, mult = np.unique(draw, return_counts=True)
    ok = np.array([counter.get(int(u), 0) + 2 * int(m) <= 14 for u, m in zip(uniq, mult)])
    uniq, mult = uniq[ok], mult[ok]
    for u, m in zip(uniq.tolist(), mult.tolist()):
      counter[u] = counter.get(u, 0) + 2 * m
      model.add(u, 2 * m)
    model.advance_if_full()
    _device_add(mt, np.repeat(uniq, 2 * mult))
  keys_arr = np.fromiter(counter.keys(), dtype=np.int64, count=len(counter))
  want = np.fromiter(counter.values(), dtype=np.int64, count=len(counter))
  got = flt.get(ids_t(keys_arr)).cpu().numpy()
  rate = float((got != want).mean())
  assert abs(rate - 0.00908) <= 0.00908 / 2, rate
  mod = np.array([model.get(int(k)) for k in keys_arr.tolist()])
  # (within a launch the order in which aliasing or colliding ids reach a probe window is not
  # defined — nor is it in the reference, whose filter is documented as not thread safe,
  # hash_filter_op.cc:68-69; measured 7e-4 of the counts)
  assert float((got != mod).mean()) <= 2e-3, float((got != mod).mean())
  assert flt.failure_count() < len(counter) / 10000


def test_unpipelined_fused_backward_consults_the_filter():
  """mhte_table_sum_optimize_n (SparseStep without a next batch) on a table with an occurrence
  filter: the update must ask the filter with each id's occurrence count (tf_bridge.cc:300-310:
  ShouldBeFiltered(id, count) = add(id, count) < threshold, add returning the count BEFORE it) — round 2's
  sum_apply_kernel path updated such a table without asking."""
  from monolith_amd.fused_step import SparseStep
  flt = HashFilter(capacity=100000, split_num=5)
  mt = _filter_table(flt, 3)
  ids = np.unique(np.random.default_rng(2).integers(1, 2**40, 3000).astype(np.int64) | (1 << 48))
  batch = np.repeat(ids, 2)                       # every id twice per batch
  step = SparseStep(mt, "t", batch.size)
  g = torch.ones((batch.size, 1), device="cuda")
  seen_before = [0, 2, 4]
  for k, before in enumerate(seen_before):
    step.forward(ids_t(batch))
    step.backward(g, 1_700_000_000 + k)
    present = mt.contains("t", ids_t(ids)).cpu().numpy().astype(bool)
    assert present.all() == (before >= 3) and present.any() == (before >= 3), (k, present.mean())
  assert (flt.get(ids_t(ids)).cpu().numpy() == 6).all()      # three consultations of count 2; admitted ids are no longer counted
  rows = mt.lookup({"t": ids_t(ids[:50])})["t"].cpu().numpy()
  np.testing.assert_array_equal(rows, np.full((50, 1), -2.0, np.float32))   # one update: 2 gradients of 1, lr 1


def _prob_table(flt, thr):
  cfg = entry.make_table_config(
      [entry.CombineAsSegment(1, entry.ZerosInitializer(), entry.SgdOptimizer(1.0))],
      slot_occurrence_threshold_config=entry.SlotOccurrenceThresholdConfig(default_occurrence_threshold=thr))
  return MultiHashTable.from_configs({"t": cfg}, name_suffix=_name(), hash_filter=flt)


@pytest.mark.parametrize("equal", [False, True])
def test_probabilistic_filter_admission_rate(equal):
  """ProbabilisticFilter (probabilistic_filter.cc:24-52; the reference's RNG is seeded with the clock, so
  its own tests check RATES at threshold 7: probabilistic_filter_test.cc:28-50 unequal, :52-76 equal,
  :78-118 ShouldBeFiltered against a table): an absent id is admitted with probability
  count / threshold per consultation — or 1 - 0.05^(count / threshold) — ids the table holds are never
  filtered, a threshold of 0 admits everything, get() is max_count, the draws are a function of the
  seed."""
  from monolith_amd.multi_hash_table_ops import ProbabilisticFilter
  thr, n = 7, 40000
  flt = ProbabilisticFilter(equal_probability=equal, seed=1234)
  mt = _prob_table(flt, thr)
  rng = np.random.default_rng(5)
  ids = np.unique(rng.integers(1, 2**40, n).astype(np.int64) | (1 << 48))
  n = ids.size
  g = torch.ones((n, 1), device="cuda")
  p1 = (1.0 - 0.05 ** (1.0 / thr)) if equal else 1.0 / thr
  mt.apply_gradients({"t": (ids_t(ids), g)})
  in1 = mt.contains("t", ids_t(ids)).cpu().numpy().astype(bool)
  assert abs(in1.mean() - p1) < 4 * np.sqrt(p1 * (1 - p1) / n), (in1.mean(), p1)
  # a second sighting: the admitted ids are updated (never filtered), the others draw again
  mt.apply_gradients({"t": (ids_t(ids), g)})
  in2 = mt.contains("t", ids_t(ids)).cpu().numpy().astype(bool)
  assert in2[in1].all()
  p2 = 1 - (1 - p1) ** 2
  assert abs(in2.mean() - p2) < 4 * np.sqrt(p2 * (1 - p2) / n), (in2.mean(), p2)
  rows = mt.lookup({"t": ids_t(ids[in1][:100])})["t"].cpu().numpy()
  np.testing.assert_array_equal(rows, np.full((min(100, int(in1.sum())), 1), -2.0, np.float32))   # two SGD steps of lr 1
  assert (flt.get(ids_t(ids[:10])).cpu().numpy() == 15).all()
  # k occurrences in one deduplicated update: one consultation with count k (tf_bridge.cc:300-310)
  from monolith_amd.fused_step import SparseStep
  flt3 = ProbabilisticFilter(equal_probability=equal, seed=99)
  mt3 = _prob_table(flt3, thr)
  fresh = np.unique(rng.integers(1, 2**40, 20000).astype(np.int64) | (2 << 48))
  batch = np.repeat(fresh, 2)
  step = SparseStep(mt3, "t", batch.size)
  step.forward(ids_t(batch))
  step.backward(torch.ones((batch.size, 1), device="cuda"), 1_700_000_000)
  pk = (1.0 - 0.05 ** (2.0 / thr)) if equal else 2.0 / thr
  got = mt3.contains("t", ids_t(fresh)).cpu().numpy().mean()
  assert abs(got - pk) < 4 * np.sqrt(pk * (1 - pk) / fresh.size), (got, pk)
  # same seed, same launches -> same draws; another seed -> another set
  a, b, c = (ProbabilisticFilter(equal_probability=equal, seed=s_) for s_ in (7, 7, 8))
  sets = []
  for f in (a, b, c):
    t = _prob_table(f, thr)
    t.apply_gradients({"t": (ids_t(ids[:5000]), g[:5000])})
    sets.append(t.contains("t", ids_t(ids[:5000])).cpu().numpy())
  assert np.array_equal(sets[0], sets[1]) and not np.array_equal(sets[0], sets[2])
  # threshold 0: everything is admitted
  mt0 = _prob_table(ProbabilisticFilter(equal_probability=False, seed=3), 0)
  mt0.apply_gradients({"t": (ids_t(ids[:1000]), g[:1000])})
  assert mt0.contains("t", ids_t(ids[:1000])).cpu().numpy().all()


# =============================================================================== fused_embedding_to_layout
# The checkers live in oracle/layout.py: layout_model / layout_grad_model (the op's algorithm over
# its own offset encoding) and the reference test's input generation + truth procedure
# (fused_embedding_to_layout_test.py:176-530, :553-790); tests/test_layout_oracle.py pins the former
# to the latter on the CPU.
from oracle import layout as OL  # noqa: E402


def _to_oracle_cfgs(cfgs):
  return OL.FeatureConfigs(
      {n: OL.FeatureConfig(f.table, f.pooling_type, list(f.slice_dims), f.max_sequence_length)
       for n, f in cfgs.feature_configs.items()},
      {n: OL.OutConfig([OL.SliceConfig(s_.feature_name, s_.start, s_.end) for s_ in o.slice_configs], o.out_type,
                       [list(x) for x in o.shape]) for n, o in cfgs.out_configs.items()})


def _to_product_cfgs(ocfgs):
  from monolith_amd import distribution_ops as D
  return D.FeatureConfigs(
      {n: D.FeatureConfig(f.table, f.pooling_type, list(f.slice_dims), f.max_sequence_length)
       for n, f in ocfgs.feature_configs.items()},
      {n: D.OutConfig([D.SliceConfig(s_.feature_name, s_.start, s_.end) for s_ in o.slice_configs], o.out_type,
                      [list(x) for x in o.shape]) for n, o in ocfgs.out_configs.items()})


def _layout_model(embs, fid_offset, feature_offset, nfl_offset, batch, cfgs, tensors_grad=None,
                  acc_dtype=np.float64):
  oc = _to_oracle_cfgs(cfgs)
  if tensors_grad is None:
    return OL.layout_model(embs, fid_offset, feature_offset, nfl_offset, batch, oc)
  return OL.layout_grad_model(embs, fid_offset, feature_offset, nfl_offset, batch, oc, tensors_grad,
                              acc_dtype=acc_dtype)


# the gradient's general form adds without float atomics, in the op's traversal order, unless the
# process was started with MHTE_POOL_ATOMICS=1 (then: arrival order, tolerance only)
_LAYOUT_GRAD_EXACT = os.environ.get("MHTE_POOL_ATOMICS", "0") in ("", "0")


def _dev_case(c):
  fo = torch.tensor(c["fid_offset"].view(np.int64)).cuda()
  fe = torch.tensor(c["feature_offset"]).cuda()
  nf = torch.tensor(c["nfl_offset"].view(np.int32)).cuda()
  return [torch.tensor(e).cuda() for e in c["embs"]], fo, fe, nf


@pytest.mark.parametrize("seed", [0, 1])
def test_fused_embedding_to_layout_reference_test_forward(seed):
  """The reference's own forward test (fused_embedding_to_layout_test.py:176-530: 199 slots, 5 shards,
  batch 256, shared lists for even slots, SUM / MEAN / FIRSTN, ADDN / CONCAT / STACK / NONE): the
  device against the test's truth procedure at the test's tolerance, and bit for bit against the
  op's restatement."""
  from monolith_amd import distribution_ops as D
  c = OL.reference_forward_case(seed)
  embs, fo, fe, nf = _dev_case(c)
  got = D.fused_embedding_to_layout(embs, fo, fe, nf, c["batch"], _to_product_cfgs(c["cfgs"]))
  model = OL.layout_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"], c["cfgs"])
  assert len(got) == len(c["expected"]) == len(model)
  for g, e, m in zip(got, c["expected"], model):
    g = g.cpu().numpy()
    assert np.allclose(e, g, rtol=1e-4, atol=1e-7)          # (:523)
    np.testing.assert_array_equal(g, m)


def test_fused_embedding_to_layout_reference_test_grad():
  """The reference's gradient test (:553-790: 29 slots, 3 shards, batch 256, every output gradient 1):
  the gradient of a fid's row is how often it was pooled (1 / len for MEAN, first 3 for FIRSTN)."""
  from monolith_amd import distribution_ops as D
  c = OL.reference_grad_case(0)
  embs, fo, fe, nf = _dev_case(c)
  tg = [torch.tensor(t).cuda() for t in c["tensors_grad"]]
  got = D.fused_embedding_to_layout_grad(embs, fo, fe, nf, c["batch"], tg, _to_product_cfgs(c["cfgs"]))
  for g, e in zip(got, c["expected_grads"]):
    np.testing.assert_allclose(g.cpu().numpy(), e, rtol=1e-4, atol=1e-6)
  if _LAYOUT_GRAD_EXACT:   # ... and the op's own sequential fp32 sums bit for bit, on every run
    seq = OL.layout_grad_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"],
                               c["cfgs"], c["tensors_grad"], acc_dtype=np.float32)
    again = D.fused_embedding_to_layout_grad(embs, fo, fe, nf, c["batch"], tg, _to_product_cfgs(c["cfgs"]))
    for g, g2, m in zip(got, again, seq):
      np.testing.assert_array_equal(g.cpu().numpy(), m)
      np.testing.assert_array_equal(g.cpu().numpy(), g2.cpu().numpy())


@pytest.mark.parametrize("batch,seed", [(1, 0), (7, 1), (300, 2)])
def test_fused_embedding_to_layout_forward_and_grad(batch, seed):
  from monolith_amd import distribution_ops as D
  rng = np.random.default_rng(seed)
  P_, OT = D.PoolingType, D.OutType
  feats = {"f_a": D.FeatureConfig("t0", P_.SUM, [1, 8]), "f_b": D.FeatureConfig("t1", P_.MEAN, [1, 8]),
           "f_c": D.FeatureConfig("t2", P_.FIRSTN, [1, 4], max_sequence_length=3),
           "f_d": D.FeatureConfig("t0", P_.SUM, [1, 8]), "f_e": D.FeatureConfig("t1", P_.SUM, [1, 8])}
  S_ = D.SliceConfig
  outs = {
      "bias": D.OutConfig([S_("f_a", 0, 1), S_("f_b", 0, 1), S_("f_d", 0, 1), S_("f_e", 0, 1)], OT.ADDN, [[-1, 1]]),
      "vec": D.OutConfig([S_("f_a", 1, 9), S_("f_b", 1, 9), S_("f_d", 1, 9)], OT.CONCAT, [[-1, 24]]),
      "ffm": D.OutConfig([S_("f_b", 1, 9), S_("f_a", 1, 9)], OT.STACK, [[-1, 2, 8]]),
      "seq": D.OutConfig([S_("f_c", 1, 5)], OT.NONE, [[-1, 3, 4]]),
      "two": D.OutConfig([S_("f_a", 1, 9), S_("f_b", 0, 1)], OT.NONE, [[-1, 8], [-1, 1]]),
  }
  cfgs = D.FeatureConfigs(feats, outs)
  embs = [rng.standard_normal((50, 9)).astype(np.float32), rng.standard_normal((40, 9)).astype(np.float32),
          rng.standard_normal((30, 5)).astype(np.float32)]
  mat_of = {"f_a": 0, "f_b": 1, "f_c": 2, "f_d": 0, "f_e": 1}
  fid_offset, feature_offset, nfl_offset = [], [], []
  for name in sorted(feats):
    shared = name == "f_d"                       # one feature instance for the whole batch
    absent = name == "f_e"                       # a named feature list with no instances at all
    nfl_offset.append(len(feature_offset) | ((1 << 31) if shared else 0))
    for b in range(0 if absent else (1 if shared else batch)):
      feature_offset.append(len(fid_offset))
      for _ in range(int(rng.integers(0, 6))):   # 0..5 fids; 0: the row keeps zeros
        m = mat_of[name]
        fid_offset.append((m << 32) | int(rng.integers(0, embs[m].shape[0])))
  fo = torch.tensor(np.array(fid_offset, dtype=np.uint64).view(np.int64)).cuda()
  fe = torch.tensor(np.array(feature_offset, dtype=np.int32)).cuda()
  nf = torch.tensor(np.array(nfl_offset, dtype=np.uint32).view(np.int32)).cuda()
  dev_embs = [torch.tensor(e).cuda() for e in embs]
  got = D.fused_embedding_to_layout(dev_embs, fo, fe, nf, batch, cfgs)
  exp = _layout_model(embs, fid_offset, feature_offset, nfl_offset, batch, cfgs)
  assert len(got) == len(exp) == 6
  for g, e in zip(got, exp):
    np.testing.assert_array_equal(g.cpu().numpy(), e)      # sequential sums: bit for bit
  tg = [rng.standard_normal(e.shape).astype(np.float32) for e in exp]
  gg = D.fused_embedding_to_layout_grad(dev_embs, fo, fe, nf, batch, [torch.tensor(t).cuda() for t in tg], cfgs)
  ge = _layout_model(embs, fid_offset, feature_offset, nfl_offset, batch, cfgs, tensors_grad=tg)
  for g, e in zip(gg, ge):
    np.testing.assert_allclose(g.cpu().numpy(), e, rtol=1e-5, atol=1e-5)
  if _LAYOUT_GRAD_EXACT:
    # rows of matrix 0 are reached from f_a and from the SHARED list f_d, through overlapping slices
    # of four layouts: slices in configuration order, batch rows ascending, fids in list order
    # (at batch 300 the shared list's rows are heavy: the workgroup form, restated exactly too)
    oc = _to_oracle_cfgs(cfgs)
    gs, n_heavy = OL.layout_grad_model_grouped(embs, fid_offset, feature_offset, nfl_offset, batch, oc, tg)
    for g, e in zip(gg, gs):
      np.testing.assert_array_equal(g.cpu().numpy(), e)
    if n_heavy == 0:   # light rows only: the op's strictly sequential fp32 sums
      seq = OL.layout_grad_model(embs, fid_offset, feature_offset, nfl_offset, batch, oc, tg, acc_dtype=np.float32)
      for e, s_ in zip(gs, seq):
        np.testing.assert_array_equal(e, s_)
    else:
      assert batch == 300


def test_fused_embedding_to_layout_grad_heavy_rows():
  """Rows that receive more contributions than one lane group should walk (a hot row pooled into
  thousands of batch rows; every row of a SHARED list at batch > 1024): the workgroup form — a
  slice's sequence in 64 contiguous ranges, range sums added in range order — against its
  restatement bit for bit, the same bits on a second run, and the sequential sum within fp32
  re-association."""
  if not _LAYOUT_GRAD_EXACT:
    pytest.skip("MHTE_POOL_ATOMICS=1")
  from monolith_amd import distribution_ops as D
  rng = np.random.default_rng(11)
  batch = 1500
  P_, OT, S_ = D.PoolingType, D.OutType, D.SliceConfig
  feats = {"f_a": D.FeatureConfig("t0", P_.SUM, [1, 8]), "f_b": D.FeatureConfig("t0", P_.MEAN, [1, 8]),
           "f_s": D.FeatureConfig("t1", P_.SUM, [1, 8]),
           "f_n": D.FeatureConfig("t1", P_.FIRSTN, [1, 4], max_sequence_length=2)}
  outs = {"bias": D.OutConfig([S_("f_a", 0, 1), S_("f_b", 0, 1), S_("f_s", 0, 1)], OT.ADDN, [[-1, 1]]),
          "vec": D.OutConfig([S_("f_a", 1, 9), S_("f_b", 1, 9), S_("f_s", 1, 9)], OT.CONCAT, [[-1, 24]]),
          "seq": D.OutConfig([S_("f_n", 1, 5)], OT.NONE, [[-1, 2, 4]])}
  cfgs = D.FeatureConfigs(feats, outs)
  embs = [rng.standard_normal((64, 9)).astype(np.float32), rng.standard_normal((32, 9)).astype(np.float32)]
  mat_of = {"f_a": 0, "f_b": 0, "f_s": 1, "f_n": 1}
  fid_offset, feature_offset, nfl_offset = [], [], []
  for name in sorted(feats):
    shared = name == "f_s"
    nfl_offset.append(len(feature_offset) | ((1 << 31) if shared else 0))
    for b in range(1 if shared else batch):
      feature_offset.append(len(fid_offset))
      m = mat_of[name]
      for _ in range(3 if shared else int(rng.integers(0, 4))):
        # rows 0 and 1 of matrix 0 are hot (f_a AND f_b reach them: two features, overlapping slices)
        row = int(rng.integers(0, 2)) if (m == 0 and rng.random() < 0.7) else int(rng.integers(0, embs[m].shape[0]))
        fid_offset.append((m << 32) | row)
  fo = torch.tensor(np.array(fid_offset, dtype=np.uint64).view(np.int64)).cuda()
  fe = torch.tensor(np.array(feature_offset, dtype=np.int32)).cuda()
  nf = torch.tensor(np.array(nfl_offset, dtype=np.uint32).view(np.int32)).cuda()
  dev_embs = [torch.tensor(e).cuda() for e in embs]
  shapes = [[batch, 1], [batch, 2, 4], [batch, 24]]            # layouts in sorted-name order
  tg = [rng.standard_normal(sh).astype(np.float32) for sh in shapes]
  dev_tg = [torch.tensor(t).cuda() for t in tg]
  got = [g.cpu().numpy() for g in D.fused_embedding_to_layout_grad(dev_embs, fo, fe, nf, batch, dev_tg, cfgs)]
  again = [g.cpu().numpy() for g in D.fused_embedding_to_layout_grad(dev_embs, fo, fe, nf, batch, dev_tg, cfgs)]
  oc = _to_oracle_cfgs(cfgs)
  exp, n_heavy = OL.layout_grad_model_grouped(embs, fid_offset, feature_offset, nfl_offset, batch, oc, tg)
  assert n_heavy >= 5           # the two hot rows, and the shared list's rows (3 fids x 1500 batch rows)
  seq = OL.layout_grad_model(embs, fid_offset, feature_offset, nfl_offset, batch, oc, tg, acc_dtype=np.float32)
  for g, g2, e, s_ in zip(got, again, exp, seq):
    np.testing.assert_array_equal(g, e)
    np.testing.assert_array_equal(g, g2)
    np.testing.assert_allclose(g, s_, rtol=2e-5, atol=2e-4)
  assert any(not np.array_equal(e, s_) for e, s_ in zip(exp, seq))   # (the ranges do re-associate)


def test_fused_embedding_to_layout_copy_form():
  """MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS: one fid per feature instance, unique rows, float4-aligned
  slices — the vector copy form (plain stores in the gradient) equals the general form.  With 28 float4
  columns per batch row this runs ``layout_rows_kernel`` (forward: whole rows, no fill in front), not
  ``layout_copy_kernel``, which takes launches of more than 2048 columns: tests/test_layout_forms_gpu.py
  cases (b) and (g)."""
  from monolith_amd import distribution_ops as D
  rng = np.random.default_rng(4)
  B, dims = 257, [16, 32, 64]
  names = ["a", "b", "c"]
  feats = {n: D.FeatureConfig(n, D.PoolingType.SUM, [d]) for n, d in zip(names, dims)}
  cfgs = D.FeatureConfigs(feats, {"x": D.OutConfig([D.SliceConfig(n, 0, d) for n, d in zip(names, dims)],
                                                     D.OutType.CONCAT, [[-1, sum(dims)]])})
  embs = [torch.tensor(rng.standard_normal((B, d)).astype(np.float32)).cuda() for d in dims]
  T = len(dims)
  fo = (torch.arange(T, dtype=torch.int64).repeat_interleave(B) << 32 | torch.arange(B).repeat(T)).cuda()
  fe = torch.arange(T * B, dtype=torch.int32).cuda()
  nf = (torch.arange(T, dtype=torch.int32) * B).cuda()
  a = D.fused_embedding_to_layout(embs, fo, fe, nf, B, cfgs)[0]
  b = D.fused_embedding_to_layout(embs, fo, fe, nf, B, cfgs, one_fid_unique_rows=True)[0]
  assert torch.equal(a, b) and torch.equal(a, torch.cat(embs, dim=1))
  g = torch.tensor(rng.standard_normal((B, sum(dims))).astype(np.float32)).cuda()
  ga = D.fused_embedding_to_layout_grad(embs, fo, fe, nf, B, [g], cfgs)
  gb = D.fused_embedding_to_layout_grad(embs, fo, fe, nf, B, [g], cfgs, one_fid_unique_rows=True)
  for x, y, w in zip(ga, gb, torch.split(g, dims, dim=1)):
    assert torch.equal(x, y) and torch.equal(x, w)


def test_fused_embedding_to_layout_whole_rows_form_needs_no_zero_fill():
  """Round 5: with one fid per feature instance the forward writes whole output rows from one workgroup
  per 16 batch rows (layout_rows_kernel) — the padding columns behind the last slice included, so the
  zero fill in front of the launch is left out.  The output memory is poisoned first; a batch that is
  not a multiple of 16 rows; against the general form and against the concatenation itself."""
  from monolith_amd import distribution_ops as D
  rng = np.random.default_rng(5)
  B, dims, kin = 1003, [16, 32, 64, 16], 256
  names = ["a", "b", "c", "d"]
  feats = {n: D.FeatureConfig(n, D.PoolingType.SUM, [d]) for n, d in zip(names, dims)}
  cfgs = D.FeatureConfigs(feats, {"x": D.OutConfig([D.SliceConfig(n, 0, d) for n, d in zip(names, dims)],
                                                     D.OutType.CONCAT, [[-1, kin]])})
  embs = [torch.tensor(rng.standard_normal((B, d)).astype(np.float32)).cuda() for d in dims]
  T = len(dims)
  fo = (torch.arange(T, dtype=torch.int64).repeat_interleave(B) << 32 | torch.arange(B).repeat(T)).cuda()
  fe = torch.arange(T * B, dtype=torch.int32).cuda()
  nf = (torch.arange(T, dtype=torch.int32) * B).cuda()
  want = torch.cat(embs + [torch.zeros(B, kin - sum(dims), device="cuda")], dim=1)
  for _ in range(3):
    poison = torch.full((B, kin), float("nan"), device="cuda")   # (the allocator hands this block out again)
    del poison
    got = D.fused_embedding_to_layout(embs, fo, fe, nf, B, cfgs, one_fid_unique_rows=True)[0]
    assert torch.equal(got, want)
  assert torch.equal(D.fused_embedding_to_layout(embs, fo, fe, nf, B, cfgs)[0], want)
  g = torch.tensor(rng.standard_normal((B, kin)).astype(np.float32)).cuda()
  gb = D.fused_embedding_to_layout_grad(embs, fo, fe, nf, B, [g], cfgs, one_fid_unique_rows=True)
  for y, w in zip(gb, torch.split(g[:, :sum(dims)], dims, dim=1)):
    assert torch.equal(y, w)
