"""CPU suite: pins the C restatement (oracle/mhte_oracle.c) to
  (1) the known-answer values of the reference's own tests,
  (2) the committed golden fixtures generated from the reference's code (tests/golden/), and
  (3) where it exists (build container), the reference-built library oracle/_ref directly.
"""
import os

import numpy as np
import pytest

import oracle as O
from monolith_amd import synthetic as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built here")


# ------------------------------------------------------------------ reference KATs: optimizers
def test_adagrad_kat_reference_test():
  # adagrad_optimizer_test.cc:32-48: init_acc=1, lr=.1, g={1,2} -> {-0.07071067,-0.08944272}
  num, norm = O.adagrad([0, 0], [1, 1], [1, 2], 0.1, 0.0)
  np.testing.assert_allclose(num, [-0.07071067, -0.08944272], rtol=0, atol=1e-7)
  np.testing.assert_array_equal(norm, [2.0, 5.0])


def test_adagrad_weight_decay_kat():
  # adagrad_optimizer_test.cc:60-88 second step with wd=.1 (baseline semantics)
  num, norm = O.adagrad([0, 0], [1, 1], [1, 2], 0.1, 0.1)
  num, norm = O.adagrad(num, norm, [1, 2], 0.1, 0.1)
  np.testing.assert_allclose(num, [-0.128173, -0.155943], rtol=0, atol=1e-5)


def test_sgd_kat():
  # embedding_hash_table_test.h:60-66: Optimize(13, {1}, lr .01) -> -0.01
  np.testing.assert_array_equal(O.sgd([0.0], [1.0], 0.01), np.float32([-0.01]))


def test_adagrad_matches_reference_arithmetic_fixture():
  z = np.load(os.path.join(GOLD, "adagrad_kat.npz"))
  for wd in (0.0, 0.1):
    num, norm = O.adagrad(z["num"], z["norm"], z["grad"], float(z["lr"]), wd)
    # scalar reference path: bit-exact
    np.testing.assert_array_equal(num, z["num_wd%g_avx0" % wd])
    np.testing.assert_array_equal(norm, z["norm_wd%g_avx0" % wd])
    # AVX2/FMA reference path: avx_test.cc:29-62 allows 1e-6 (only when wd == 0 the two agree,
    # avx_utils.h:112 subtracts eff_lr*grad, not eff_lr*g)
    if wd == 0.0:
      np.testing.assert_allclose(num, z["num_wd0_avx1"], rtol=0, atol=1e-6)


# ------------------------------------------------------------------ reference KATs: table ops
def _table(dim=1, opt=O.OPT_SGD, **kw):
  return O.Table(O.segment(dim, opt, **kw), 1)


def test_lookup_miss_is_zero_and_does_not_insert():
  # embedding_hash_table_test.h:41-49
  t = _table(2)
  e, hits = t.lookup([1, 2, 3])
  assert hits == 0 and not e.any() and t.size() == 0


def test_assign_add_negative_id():
  # embedding_hash_table_test.h:51-58: AssignAdd(-10, 2.5)
  t = _table(1)
  t.assign_add([-10], [[2.5]])
  np.testing.assert_array_equal(t.lookup([-10])[0], [[2.5]])


def test_optimize_duplicates_apply_sequentially():
  # hash_table_ops_test.py:134-148: ids [0,0,1], grad -1, lr .1 -> [[.2],[.1]]
  t = _table(1)
  t.optimize([0, 0, 1], [[-1.0], [-1.0], [-1.0]], [0.1])
  np.testing.assert_allclose(t.lookup([0, 1])[0], [[0.2], [0.1]], atol=1e-7)


def test_multi_table_sgd_kat():
  # multi_hash_table_ops_test.py:101-127: SGD lr 1: grads 2;[[1,3],[2,4]] -> -2;[[-1,-3],[-2,-4]]
  t1, t2 = _table(1), _table(2)
  t1.optimize([0], [[2.0]], [1.0])
  t2.optimize([1, 2], [[1.0, 3.0], [2.0, 4.0]], [1.0])
  np.testing.assert_array_equal(t1.lookup([0])[0], [[-2.0]])
  np.testing.assert_array_equal(t2.lookup([1, 2])[0], [[-1.0, -3.0], [-2.0, -4.0]])


def test_reinitialize_status_codes():
  # multi_hash_table_ops_test.py:52-99: assign_add ids then reinitialize -> [0,1,1] style
  t = _table(1)
  t.assign_add([1, 2], [[1.0], [1.0]])
  st = t.reinitialize([0, 1, 2])
  np.testing.assert_array_equal(st, [0, 1, 1])
  assert not t.lookup([0, 1, 2])[0].any()


def test_evict_ttl_per_slot():
  # embedding_hash_table_test.h:282-326: slot 1 TTL 5 d evicted at +5 d 60 s; slot 2 TTL 6 d and
  # default 14 d kept.
  t = _table(1)
  day = 86400
  f1, f2, f3 = (1 << 48) | 123, (2 << 48) | 123, (3 << 48) | 123
  t.assign([f1, f2, f3], [[1.0], [2.0], [3.0]], update_time=1000)
  t.set_ttl(14, {1: 5, 2: 6})
  t.evict(1000 + 5 * day + 60)
  assert not t.contains(f1) and t.contains(f2) and t.contains(f3)
  assert t.size() == 2


def test_update_time_truncated_to_uint32():
  t = _table(1)
  t.assign([5], [[1.0]], update_time=(1 << 32) + 77)
  assert int(t.dump()[2][0]) == 77


def test_multi_segment_row_layout_and_lrs():
  # bias FTRL(dim 1) + vector Adagrad(dim 4) as in distributed_ps_test.py:480-505
  segs = [O.segment(1, O.OPT_FTRL, p=(0.1, 0.0, 0.0, 0.0)), O.segment(4, O.OPT_ADAGRAD, p=(0.1, 0.0))]
  t = O.Table(segs, 1)
  assert t.dim == 5 and t.row_floats == 5 + 2 + 4
  g = np.float32([[1, 1, 2, 3, 4]])
  t.optimize([9], g, [0.5, 0.1])
  row = t.dump()[3][0]
  # adagrad part: n = .1 + g^2 ; w = -lr/sqrt(n)*g
  gv = g[0, 1:]
  n = np.float32(0.1) + gv * gv
  np.testing.assert_allclose(row[7:11], n, rtol=1e-7)
  np.testing.assert_allclose(row[1:5], -np.float32(0.1) / np.sqrt(n) * gv, rtol=1e-6)
  # ftrl part (ftrl_optimizer.cc:56-75) with l1=0: z = g - sigma*0 = 1; w = lr*(signbit(z)*0 - z)/(sqrt(n)+beta)
  nf = np.float32(0.1) + np.float32(1.0)
  np.testing.assert_allclose(row[5], nf, rtol=1e-7)
  np.testing.assert_allclose(row[6], 1.0, rtol=1e-7)
  np.testing.assert_allclose(row[0], 0.5 * (-1.0) / np.sqrt(nf), rtol=1e-6)


# ------------------------------------------------------------------ dedup / packing KATs
def test_unique_key_with_value_and_offset_docstring_example():
  # reference distribution_ops.py:101-110
  uk, uks, vo, vos, blen = O.unique_key_with_value_and_offset([0, 1, 0, 0], [0, 3, 4], [2, 3])
  np.testing.assert_array_equal(uk, [0, 1, 0])
  np.testing.assert_array_equal(uks, [0, 2, 3])
  np.testing.assert_array_equal(vo, [0, 4, 2, 6])
  np.testing.assert_array_equal(vos, [0, 2, 3, 4])
  assert blen == 9


def test_fill_with_offset_map_docstring_example():
  # reference distribution_ops.py:133-140
  buf = O.fill_with_offset_map([0, 1, 2], [0, 2, 3], np.arange(7, dtype=np.float32), [0, 4, 2, 6],
                               [0, 2, 3, 4], [2, 3], 9)
  np.testing.assert_array_equal(buf, [0, 1, 2, 3, 0, 1, 4, 5, 6])


def test_fill_with_offset_map_gradient_sums_in_order():
  g = np.float32([1, 2, 10, 20, 100, 200, 7, 8, 9])
  out = O.fill_with_offset_map_gradient([0, 1, 2], [0, 2, 3], g, [0, 4, 2, 6], [0, 2, 3, 4], [2, 3])
  np.testing.assert_array_equal(out, [101, 202, 10, 20, 7, 8, 9])


def test_fused_lookup_offsets_kat():
  # hash_table_ops_test.py:1086-1107: splits [4,4], id_offsets 0..6, emb_offsets [0,1,2,4,5,6,8]
  ko, eo, kpt, es, tk, te = O.compute_fused_offsets([1, 1, 1, 1, 1, 1], [1, 1, 2], 3, 2)
  np.testing.assert_array_equal(ko, [0, 1, 2, 3, 4, 5, 6])
  np.testing.assert_array_equal(eo, [0, 1, 2, 4, 5, 6, 8])
  np.testing.assert_array_equal(es, [4, 4])
  assert (tk, te) == (6, 8)


def test_fused_reorder_by_indices_semantics():
  # fused_reorder_by_indices.cc:38-123: per-table dedup, shard-major table-minor packing
  out, shard_sizes, sss, eos, feo = O.fused_reorder_by_indices([[0, 1, 2, 1, 4], [3, 3, 6]], 2,
                                                               [2, 3])
  # shard 0: table0 {0,2,4}, table1 {6}; shard 1: table0 {1}, table1 {3}
  np.testing.assert_array_equal(out, [0, 2, 4, 6, 1, 3])
  np.testing.assert_array_equal(shard_sizes, [4, 2])
  np.testing.assert_array_equal(sss, [3, 1, 1, 1])
  np.testing.assert_array_equal(eos, [5, 3])
  # emb offsets: shard0 t0 at 0 (3 ids x2), shard0 t1 at 6 (1x3), shard1 t0 at 9 (1x2), shard1 t1 at 11
  np.testing.assert_array_equal(feo, [0, 9, 2, 9, 4, 11, 11, 6])


# ------------------------------------------------------------------ golden fixtures from the reference
@pytest.mark.parametrize("name", ["sgd_d8_uniform", "adagrad_d16_zipf", "adagrad_d64_zipf"])
def test_training_loop_matches_reference_fixture(name):
  z = np.load(os.path.join(GOLD, "table_%s.npz" % name))
  dim, opt = int(z["dim"]), int(z["opt"])
  t = O.Table(O.segment(dim, opt, p=(float(z["init_acc"]), float(z["wd"]))), 1)
  for s in range(int(z["steps"])):
    ids = S.id_batch(s, int(z["batch"]), int(z["universe"]), str(z["dist"]))
    g = S.grad_batch(s, int(z["batch"]), dim)
    uk, _, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, ids.size], [dim])
    assert uk.size == int(z["n_unique"][s])
    emb_u, _ = t.lookup(uk)
    emb = O.fill_with_offset_map(np.arange(uk.size), [0, uk.size], emb_u.ravel(), vo, vos, [dim],
                                 ids.size * dim).reshape(-1, dim)
    np.testing.assert_array_equal(emb[:64], z["step_emb_first"][s])
    np.testing.assert_allclose(emb.astype(np.float64).sum(0), z["step_emb_sum"][s], rtol=1e-12)
    gu = O.fill_with_offset_map_gradient(np.arange(uk.size), [0, uk.size], g.ravel(), vo, vos,
                                         [dim]).reshape(-1, dim)
    t.optimize(uk, gu, [float(z["lr"])], S.update_time(s))
  assert t.size() == int(z["size"])
  final, hits = t.lookup(z["probe_ids"])
  assert hits == z["probe_ids"].size
  np.testing.assert_array_equal(final, z["final_rows"])


def test_sequential_placement_matches_reference_fixture():
  z = np.load(os.path.join(GOLD, "placement_seq.npz"))
  t = O.Table(O.segment(4, O.OPT_SGD), int(z["cap"]))
  for i in range(z["ids"].size):
    t.assign(z["ids"][i:i + 1], z["vals"][i:i + 1], 100 + i)
  ids, pos, ts, rows = t.dump()
  np.testing.assert_array_equal(ids, z["dump_ids"])
  np.testing.assert_array_equal(pos, z["dump_pos"])
  np.testing.assert_array_equal(ts, z["dump_ts"])
  np.testing.assert_array_equal(rows, z["dump_rows"])


# ------------------------------------------------------------------ live cross-check with oracle/_ref
@needs_ref
@pytest.mark.parametrize("opt", [O.OPT_SGD, O.OPT_ADAGRAD])
def test_random_ops_match_reference_map(opt):
  rng = np.random.default_rng(11 + opt)
  t = O.Table(O.segment(6, opt, p=(0.1, 0.0)), 1)
  r = O.RefTable(6, opt, 0.1, 0.0, 0.0, 1)
  universe = rng.integers(-2**62, 2**62, 30000)
  for step in range(12):
    ids = rng.choice(universe, 5000)
    v = rng.standard_normal((ids.size, 6)).astype(np.float32)
    kind = step % 4
    if kind == 0:
      t.assign(ids, v, 100 + step); r.assign(ids, v, 100 + step)
    elif kind == 1:
      t.assign_add(ids, v, 100 + step); r.assign_add(ids, v, 100 + step)
    elif kind == 2:
      t.optimize(ids, v, [0.05], 100 + step); r.optimize(ids, v, 0.05, 100 + step)
    else:
      np.testing.assert_array_equal(t.reinitialize(ids[:500], 5), r.reinitialize(ids[:500], 5))
  assert t.size() == r.size() and t.hashpower() == r.hashpower()
  a, b = t.dump(), r.dump()
  for x, y in zip(a, b):
    np.testing.assert_array_equal(x, y)
  e1, h1 = t.lookup(universe[:4000])
  e2, h2 = r.lookup(universe[:4000])
  assert h1 == h2
  np.testing.assert_array_equal(e1, e2)


# ---- the remaining sparse optimizers: KATs of the reference's own *_optimizer_test.cc -------------
OPT_KATS = [
    # (name, opt, p, lr, grads, after first step, after second step, file:line)
    ("momentum", O.OPT_MOMENTUM, (0.9, 0.0, 0.0), 0.01, [10.0, 1.0], [-0.1, -0.01], [-0.29, -0.029],
     "momentum_optimizer_test.cc:32-75"),
    ("adadelta", O.OPT_ADADELTA, (0.9, 0.01, 0.0), 0.01, [10.0, 1.0], [-0.0031607, -0.0030151],
     [-0.0064035, None], "adadelta_optimizer_test.cc:32-64"),
    ("rmsprop", O.OPT_RMSPROP, (0.9, 0.0, 0.01), 0.01, [10.0], [-0.024025], [-0.042686],
     "rmsprop_optimizer_test.cc:32-51"),
    ("rmspropv2", O.OPT_RMSPROPV2, (0.9, 0.0, 0.01), 0.01, [10.0, 1.0], [-0.0090909, -0.005],
     [None, None], "rmsprop_optimizer_test.cc:53-62"),
    ("adam", O.OPT_ADAM, (0.9, 0.99, 0.01, 0.0, 0.0), 0.01, [10.0, 1.0], [-0.00990099, -0.00909091],
     [-0.01983060, -0.01842895], "adam_optimizer_test.cc:32-76"),
    ("amsgrad", O.OPT_AMSGRAD, (0.9, 0.99, 0.01, 0.0, 0.0), 0.01, [10.0], [-0.00990099],
     [-0.01983060], "amsgrad_optimizer_test.cc:32-51"),
    ("moving_average", O.OPT_MOVING_AVERAGE, (0.9,), 0.01, [10.0, 1.0], [1.0, 0.1], [1.9, 0.19],
     "moving_average_optimizer_test.cc:32-68"),
    ("group_adagrad", O.OPT_GROUP_ADAGRAD, (0.0, 1.0, 1.0, 0.0), 0.01, [10.0], [-0.008182], [-0.014125],
     "group_adagrad_optimizer_test.cc:32-56"),
]


@pytest.mark.parametrize("kat", OPT_KATS, ids=[k[0] for k in OPT_KATS])
def test_remaining_optimizer_kats(kat):
  _, opt, p, lr, grads, exp1, exp2, _ = kat
  dim = len(grads)
  t = O.Table([O.segment(dim, opt, p=p)], 1)
  g = np.array([grads], np.float32)
  t.optimize(np.array([7], np.int64), g, [lr], 0)
  got1 = t.lookup(np.array([7], np.int64))[0][0]
  np.testing.assert_allclose(got1, exp1, rtol=0, atol=1e-6)
  t.optimize(np.array([7], np.int64), g, [lr], 0)
  got2 = t.lookup(np.array([7], np.int64))[0][0]
  for a, b in zip(got2, exp2):
    if b is not None:
      assert abs(a - b) < 1e-6


def test_batch_softmax_kat():
  """batch_softmax_optimizer_test.cc:32-42: alpha 0.1, global_step 1 -> B = 0.1; then the
  recurrence B = (1 - alpha) B + alpha (step - last step) by hand."""
  t = O.Table([O.segment(1, O.OPT_BATCH_SOFTMAX)], 1)
  one = np.array([7], np.int64)
  g = np.array([[2.0]], np.float32)
  t.optimize(one, g, [0.1], 0, global_step=1)
  assert t.lookup(one)[0][0][0] == np.float32(0.1)
  t.optimize(one, g, [0.1], 0, global_step=5)
  exp = np.float32(np.float32(np.float32(0.9) * np.float32(0.1)) + np.float32(np.float32(0.1) * np.float32(4.0)))
  assert t.lookup(one)[0][0][0] == exp
  # a second occurrence in the same call sees step - last step = 0
  t.optimize(np.array([9, 9], np.int64), np.zeros((2, 1), np.float32), [0.1], 0, global_step=3)
  first = np.float32(np.float32(0.1) * np.float32(3.0))
  assert t.lookup(np.array([9], np.int64))[0][0][0] == np.float32(np.float32(0.9) * first)


def test_group_adagrad_list_kat():
  """group_adagrad_optimizer_test.cc:58-84: dim 2, l2 0.5, beta 1, accumulator 0."""
  t = O.Table([O.segment(2, O.OPT_GROUP_ADAGRAD, p=(0.0, 1.0, 0.5, 0.0))], 1)
  one = np.array([7], np.int64)
  t.optimize(one, np.array([[10.0, 1.0]], np.float32), [0.01], 0)
  np.testing.assert_allclose(t.lookup(one)[0][0], [-0.008639, -0.000864], rtol=0, atol=1e-6)
  t.optimize(one, np.array([[1.0, 5.0]], np.float32), [0.01], 0)
  np.testing.assert_allclose(t.lookup(one)[0][0], [-0.009096, -0.004778], rtol=0, atol=1e-6)


@needs_ref
def test_eviction_interleaved_with_inserts_matches_reference_map():
  """TTL eviction (cuckoohash_map.hpp:775-799 through cuckoo_embedding_hash_table.cc:251-264) between
  rounds of inserts: the slots an eviction frees are the ones later inserts take (last empty slot of
  the first bucket, :1398-1418), so physical placement after several evict / refill rounds pins the
  restatement's erase and its interaction with doubling."""
  rng = np.random.default_rng(4242)
  dim = 4
  t = O.Table(O.segment(dim, O.OPT_SGD), 1)
  r = O.RefTable(dim, O.OPT_SGD, 0.1, 0.0, 0.0, 1)
  day = 86400
  ttl = {1: 1, 2: 3}                      # feature slot -> days; everything else: 7 days
  t.set_ttl(7, ttl)
  r.set_ttl(7, ttl)
  now = 1_700_000_000
  sig = rng.integers(0, 2**40, 40000)
  slots = rng.integers(1, 5, sig.size)    # feature slots 1..4 (bit 63 clear)
  universe = (slots.astype(np.int64) << 48) | sig.astype(np.int64)
  for rnd in range(6):
    ids = rng.choice(universe, 6000)
    v = rng.standard_normal((ids.size, dim)).astype(np.float32)
    t.optimize(ids, v, [0.05], now)
    r.optimize(ids, v, 0.05, now)
    now += day * (1 + rnd % 3)            # 1, 2, 3 days later: slot-1 rows always expire, slot-2 sometimes
    t.evict(now)
    r.evict(now)
    assert t.size() == r.size() and t.hashpower() == r.hashpower(), rnd
    a, b = t.dump(), r.dump()
    for x, y in zip(a, b):
      np.testing.assert_array_equal(x, y)
  assert 0 < t.size() < 24000             # (something was evicted, something stayed)


# ---- every per-row optimizer against the reference's OWN sources compiled in place ----------------
# (oracle/ref_opt_driver.cc #includes runtime/hash_table/optimizer/*_optimizer.cc; the factory
# functions, Init() and Optimize() that run are the reference's.)  25 random Optimize() calls per
# configuration; weights AND optimizer context compared bit for bit after every call.
needs_ref_opt = pytest.mark.skipif(not O.ref_opt_available(), reason="oracle/_ref (optimizers) not built here")
REF_OPT_CASES = [
    ("sgd", O.OPT_SGD, ()),
    ("adagrad", O.OPT_ADAGRAD, (0.1, 0.0)),
    ("adagrad_wd", O.OPT_ADAGRAD, (1.0, 0.1)),
    ("ftrl", O.OPT_FTRL, (0.1, 0.0, 0.0, 0.0)),
    ("ftrl_l1_l2_beta", O.OPT_FTRL, (0.1, 1.0, 0.001, 0.01)),
    ("momentum", O.OPT_MOMENTUM, (0.9, 0.0, 0.0)),
    ("momentum_nesterov_wd", O.OPT_MOMENTUM, (0.9, 0.01, 1.0)),
    ("adadelta", O.OPT_ADADELTA, (0.9, 0.01, 0.0)),
    ("adadelta_wd", O.OPT_ADADELTA, (0.95, 1e-6, 0.02)),
    ("rmsprop", O.OPT_RMSPROP, (0.9, 0.0, 0.01)),
    ("rmsprop_wd", O.OPT_RMSPROP, (0.8, 0.05, 0.003)),
    ("rmspropv2", O.OPT_RMSPROPV2, (0.9, 0.0, 0.01)),
    ("rmspropv2_wd", O.OPT_RMSPROPV2, (0.8, 0.05, 0.003)),
    ("adam", O.OPT_ADAM, (0.9, 0.99, 0.01, 0.0, 0.0)),
    ("adam_nesterov_wd", O.OPT_ADAM, (0.9, 0.999, 1e-8, 0.01, 1.0)),
    ("amsgrad", O.OPT_AMSGRAD, (0.9, 0.99, 0.01, 0.0, 0.0)),
    ("amsgrad_nesterov_wd", O.OPT_AMSGRAD, (0.9, 0.999, 1e-8, 0.01, 1.0)),
    ("moving_average", O.OPT_MOVING_AVERAGE, (0.9,)),
    ("group_adagrad", O.OPT_GROUP_ADAGRAD, (0.1, 1.0, 0.001, 0.0)),
    ("group_adagrad_wd_l2", O.OPT_GROUP_ADAGRAD, (0.0, 1.0, 1.0, 0.05)),
    ("batch_softmax", O.OPT_BATCH_SOFTMAX, ()),
]


def _oracle_row(t, dim):
  _, _, _, rows = t.dump()
  return rows[0, :dim].copy(), rows[0, dim:].copy()


@needs_ref_opt
@pytest.mark.parametrize("case", REF_OPT_CASES, ids=[c[0] for c in REF_OPT_CASES])
def test_optimizer_restatement_bit_exact_vs_compiled_reference(case):
  name, opt, p = case
  for seed, dim in ((1, 1), (2, 8), (3, 19)):
    if opt == O.OPT_BATCH_SOFTMAX and dim != 1:
      continue   # (dim_size 1 by definition, batch_softmax_optimizer.cc:28)
    rng = np.random.Generator(np.random.PCG64(seed))
    t = O.Table([O.segment(dim, opt, p=p)], 1)
    r = O.RefOptimizer(opt, dim, p)
    one = np.array([7], np.int64)
    for step in range(25):
      g = (rng.standard_normal(dim) * (10.0 ** rng.integers(-3, 2))).astype(np.float32)
      lr = float(np.float32(10.0 ** rng.uniform(-3, -0.5)))
      gs = 3 * step + 1
      t.optimize(one, g[None, :], [lr], 0, global_step=gs)
      num_ref, ctx_ref = r.optimize(g, lr, global_step=gs)
      num, ctx = _oracle_row(t, dim)
      assert np.array_equal(num.view(np.uint32), num_ref.view(np.uint32)), (name, dim, step, num, num_ref)
      assert np.array_equal(ctx.view(np.uint32)[:ctx_ref.size], ctx_ref.view(np.uint32)), (name, dim, step)


@needs_ref_opt
@pytest.mark.parametrize("dim", [64, 100, 260])
@pytest.mark.parametrize("case", [c for c in REF_OPT_CASES if c[1] == O.OPT_GROUP_ADAGRAD], ids=lambda c: c[0])
def test_group_adagrad_restatement_vs_compiled_reference_at_wide_segments(case, dim):
  """GroupAdaGrad is the one optimizer whose step reads the whole segment (the largest squared gradient, the
  norm of the intermediate vector as ONE chain in element order): the oracle's restatement against the
  reference's own object at the segment widths the GPU tests of tests/test_optimizer_shapes_gpu.py use —
  64, 100 and 260 floats, where the device walks more than one trip of its lane group.  The first call's
  gradient is small enough for ||z|| < l2 (the branch that zeroes the segment: weights exactly zero although
  the gradient is not); the later ones take the shrinking branch."""
  name, opt, p = case
  rng = np.random.Generator(np.random.PCG64(dim))
  t = O.Table([O.segment(dim, opt, p=p)], 1)
  r = O.RefOptimizer(opt, dim, p)
  one = np.array([7], np.int64)
  shrunk = 0
  for step in range(25):
    scale = 1e-5 if step == 0 else 10.0 ** rng.integers(-3, 2)
    g = (rng.standard_normal(dim) * scale).astype(np.float32)
    lr = float(np.float32(10.0 ** rng.uniform(-3, -0.5)))
    t.optimize(one, g[None, :], [lr], 0)
    num_ref, ctx_ref = r.optimize(g, lr)
    num, ctx = _oracle_row(t, dim)
    assert np.array_equal(num.view(np.uint32), num_ref.view(np.uint32)), (name, dim, step)
    assert np.array_equal(ctx.view(np.uint32)[:ctx_ref.size], ctx_ref.view(np.uint32)), (name, dim, step)
    if step == 0:
      assert g.any() and not num_ref.any(), (name, dim)
    shrunk += int(num_ref.all())
  assert shrunk > 0, (name, dim)


@needs_ref_opt
def test_reference_as_built_avx_fma_flavour_stays_within_the_parity_bar():
  """The reference as its .bazelrc builds it (-mavx2 -mfma: avx_utils.h's vector Adagrad, contracted
  multiply-adds elsewhere) against the scalar arithmetic the engine follows: within north_star's
  1e-5 on the weights after 25 steps for every optimizer at wd = 0 (Adagrad with wd != 0 is a
  different FORMULA on the AVX path, avx_utils.h:112 — opt-in in the engine, tested on its own)."""
  if not O.ref_opt_available(avx=True):
    pytest.skip("avx flavour not built")
  for name, opt, p in REF_OPT_CASES:
    if name in ("adagrad_wd",):
      continue
    dim = 1 if opt == O.OPT_BATCH_SOFTMAX else 16
    rng = np.random.Generator(np.random.PCG64(11))
    a, b = O.RefOptimizer(opt, dim, p), O.RefOptimizer(opt, dim, p, avx=True)
    for step in range(25):
      g = (rng.standard_normal(dim) * 0.01).astype(np.float32)
      na, _ = a.optimize(g, 0.01, global_step=step + 1)
      nb, _ = b.optimize(g, 0.01, global_step=step + 1)
    np.testing.assert_allclose(na, nb, rtol=1e-5, atol=1e-5, err_msg=name)


@needs_ref_opt
def test_adagrad_avx_semantics_differ_with_weight_decay():
  """avx_utils.h:96-119 subtracts eff_lr * grad (not eff_lr * (grad + wd w)) — what the reference
  ships (.bazelrc:63-68); the oracle's opt-in restatement of THAT formula against the AVX build."""
  dim = 64
  rng = np.random.Generator(np.random.PCG64(5))
  a = O.RefOptimizer(O.OPT_ADAGRAD, dim, (0.1, 0.1))
  b = O.RefOptimizer(O.OPT_ADAGRAD, dim, (0.1, 0.1), avx=True)
  num = np.zeros(dim, np.float32)
  norm = np.full(dim, 0.1, np.float32)
  for step in range(10):
    g = rng.standard_normal(dim).astype(np.float32)
    na, _ = a.optimize(g, 0.05)
    nb, cb = b.optimize(g, 0.05)
    num, norm = O.adagrad_avx(num, norm, g, 0.05, 0.1)
    np.testing.assert_array_equal(num, nb)      # bit for bit: the restatement fuses where the AVX code does
    np.testing.assert_array_equal(norm, cb)
  assert np.abs(na - nb).max() > 1e-3   # the two formulas really are different updates
  # through the table (segment p[2] != 0), dim 19 = two fused blocks of 8 + a baseline tail of 3
  t = O.Table([O.segment(19, O.OPT_ADAGRAD, p=(0.1, 0.1, 1.0))], 1)
  r = O.RefOptimizer(O.OPT_ADAGRAD, 19, (0.1, 0.1), avx=True)
  one = np.array([3], np.int64)
  for step in range(10):
    g = rng.standard_normal(19).astype(np.float32)
    t.optimize(one, g[None, :], [0.05], 0)
    nr, cr = r.optimize(g, 0.05)
    num, ctx = _oracle_row(t, 19)
    np.testing.assert_array_equal(num, nr)
    np.testing.assert_array_equal(ctx, cr)


@needs_ref_opt
def test_dc_decorator_compiled_reference_matches_closed_form():
  """dc_optimizer.cc:28-43: g' = g + lambda g^2 (w - w_latest), then the base optimizer."""
  rng = np.random.Generator(np.random.PCG64(9))
  w = rng.standard_normal(8).astype(np.float32)
  g = rng.standard_normal(8).astype(np.float32)
  lv = rng.standard_normal(8).astype(np.float32)
  got = O.ref_dc_sgd(w, g, lv, 0.1, 0.5)
  lam, lr = np.float32(0.5), np.float32(0.1)
  gc = g + lam * g * g * (w - lv)
  np.testing.assert_array_equal(got, w - lr * gc)


def test_adagrad_avx_restatement_matches_the_committed_as_built_fixture():
  """tests/golden/adagrad_avx_kat.npz (the reference's NewAdagradOptimizer compiled -mavx2 -mfma,
  make_golden.py adagrad_avx_fixture): pins mo_adagrad_avx where oracle/_ref is absent."""
  z = np.load(os.path.join(GOLD, "adagrad_avx_kat.npz"))
  for dim in (64, 27):
    num = np.zeros(dim, np.float32)
    norm = np.full(dim, z["init_acc"], np.float32)
    for s in range(z["grad_d%d" % dim].shape[0]):
      num, norm = O.adagrad_avx(num, norm, z["grad_d%d" % dim][s], float(z["lr"]), float(z["wd"]))
      np.testing.assert_array_equal(num, z["num_d%d" % dim][s])
      np.testing.assert_array_equal(norm, z["norm_d%d" % dim][s])


def test_shared_reference_map_64_threads_through_two_doublings():
  """Variant (ii) of the CPU baseline (bench.py --cpu-child ii): ONE reference cuckoohash_map upserted
  by 64 threads while it doubles twice, from the capacity the baseline starts it at (2^18 slots = the
  map's kMaxNumLocks buckets: the locks array is never replaced, so the reference's
  `old_buckets_.swap(buckets_)` window — round 4's rc -11 of the 256-thread baseline, root-caused with
  oracle/stress/shared_map_stress.cc — cannot open).  Every id inserted is found afterwards, the rows
  are what a single-threaded replay of the same steps gives."""
  if not O.ref_available(True):
    pytest.skip("oracle/_ref not built")
  rng = np.random.default_rng(5)
  D, B, steps = 8, 65536, 11
  ps = O.RefPs(64, D, O.OPT_ADAGRAD, 0.1, 0.0, 0.0, 1 << 18, avx=True, shared=True)
  one = O.RefPs(1, D, O.OPT_ADAGRAD, 0.1, 0.0, 0.0, 1 << 18, avx=True, shared=True)
  hp0 = ps.hashpower()
  g = (rng.standard_normal((B, D)) * 0.01).astype(np.float32)
  ids = None
  for s in range(steps):
    ids = rng.integers(1, 1 << 40, size=B, dtype=np.int64)
    ps.step(ids, g, 0.001, 1_700_000_000 + s, want_emb=False)
    one.step(ids, g, 0.001, 1_700_000_000 + s, want_emb=False)
  assert ps.hashpower() >= hp0 + 2, (hp0, ps.hashpower())
  assert ps.size() == one.size()
  rows, hits = ps.lookup(ids)
  assert hits == B
  np.testing.assert_array_equal(rows, one.lookup(ids)[0])
