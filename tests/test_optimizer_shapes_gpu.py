"""The fused step's optimizer instances on every lane shape (-m gpu).

``Table::step_bwd_instance`` picks the pipelined step's backward kernel from BASIC / FULL, one segment or
several, admission filter or none, an optimizer fixed at compile time (``OPTK``: Momentum, Adadelta, RMSProp
v1 / v2, Adam, AMSGrad on a one-segment float4 table) and the lane shape ``for_shape`` gives (G in 8 / 16 /
32 / 64, VEC in 1 / 4).  The rest of the suite drives FULL tables through two-segment rows of dim 32 and 17
only; this module drives

  1. the 24 ``OPTK`` instances, on one-segment tables of dims 8 / 64 / 100 / 256 (G = 8 / 16 / 32 / 64) and the
     ragged dims 36 / 132 (a last lane group only partly filled);
  2. the generic one-segment FULL instance (MovingAverage, VEC = 1 rows, an fp16-rounded table);
  3. FULL tables with an admission filter;
  4. FULL updates in the displacement pass that rides in the next forward launch, and the forward launch's
     three-ids-per-group form at the maximum batch;
  5. the multi-table step's FULL families, with and without a filter in the launch;
  6. GroupAdaGrad (the whole-segment optimizer, op-level kernels) on segments of more than one trip of
     ``G * VEC`` floats, segments that start inside a trip, and G = 32 / 64.

Every comparison is against the CPU oracle (``oracle.Table`` after ``unique_key_with_value_and_offset`` +
``fill_with_offset_map_gradient``: duplicate gradients summed in occurrence order, one optimizer step per
distinct id), forward outputs at every step, all rows and ``size()`` at the end.

Bars.  With ``exact_order=True`` everything is bit for bit.  Without it, rows of ids that never had more than
32 occurrences in a step are bit for bit (their lists are summed in order), the others within the suite's
RTOL_TREE / ATOL_TREE.  Adam, RMSProp and Adadelta divide by a root of their state, so a re-associated sum
could have moved a heavy row by more than that bar; it does not — measured on the MI355X, max over every
heavy row and forward output of this module of |engine - oracle|: Momentum 1.8e-7, Adadelta 6.0e-8, RMSProp
v1 / v2 6.0e-8, Adam / AMSGrad 7.5e-8 (1.8e-7 at dim 256 in the multi-table step), MovingAverage 4.2e-7, the
closest any element comes to the bar being 3.5e-7 below it — so the bar stays the project's, for every
optimizer.

The id stream of sections 1 and 2 (``_stream``; 4096 ids per step, five steps, a table that starts at
capacity 1) holds, and the tests assert that it holds: ids that recur from the previous step (the row hint
probed a step ahead is hit, the prefetched row is used), ids new in every step (``is_new``: the prefetch is
discarded), lists of 33, 40 and 300 occurrences (item workgroups, and with exact order the pre-summed
apply), a list of exactly 32 (the last light one), and two doublings of the table after the first step (hints
probed a step ahead are stale when used).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from monolith_amd import _lib, entry  # noqa: E402
from monolith_amd.fused_step import MultiSparseStep, SparseStep  # noqa: E402
from monolith_amd.multi_hash_table_ops import HashFilter, MultiHashTable  # noqa: E402
import test_multi_step_gpu as M  # noqa: E402
from test_alignment_forms_gpu import _must_defer  # noqa: E402
from test_oracle import OPT_KATS  # noqa: E402
from test_parity_gpu import (ATOL_TREE, RTOL_TREE, _OPT_ENTRY, _half_neighbours, _name, ids_t,  # noqa: E402
                             val_t)

B, STEPS = 4096, 5
LIGHT_MAX = 32          # kStepLightMax: longer lists go to the item workgroups
GSTEP = 1000
OPTK = ["momentum", "adadelta", "rmsprop", "rmspropv2", "adam", "amsgrad"]
_KAT = {k[0]: k for k in OPT_KATS}


# =============================================================================== tables
def _opt(name):
  """(oracle optimizer, its parameters, learning rate, entry-config factory)"""
  if name == "adagrad":
    return O.OPT_ADAGRAD, (0.1, 0.0), 0.05, lambda: entry.AdagradOptimizer(0.05, 0.1)
  if name == "ftrl":
    return (O.OPT_FTRL, (0.1, 1.0, 0.001, 0.001), 0.05,
            lambda: entry.FtrlOptimizer(0.05, 0.1, 1.0, l1_regularization=0.001, l2_regularization=0.001))
  _, oopt, p, lr, _, _, _, _ = _KAT[name]
  return oopt, p, lr, _OPT_ENTRY[name]


class Tab:
  """One table: segments [(dim, optimizer name)], every segment initialised to 0.25 (a new row that skipped
  its initializer shows), for the engine and for the oracle."""

  def __init__(self, segs, sr16=False, thr=None, **kw):
    self.segs, self.sr16, self.thr, self.kw = tuple(segs), sr16, thr, dict(kw)
    self.dim = sum(d for d, _ in segs)
    self.lrs = [_opt(o)[2] for _, o in segs]

  def key(self):
    return (self.segs, self.sr16, self.thr, tuple(sorted(self.kw.items())))

  def entry_cfg(self):
    parts = []
    for i, (d, o) in enumerate(self.segs):
      opt = _opt(o)[3]()
      if self.sr16 and i == 0:
        opt = entry.StochasticRoundingFloat16OptimizerWrapper(opt)
      parts.append(entry.CombineAsSegment(d, entry.ConstantsInitializer(0.25), opt))
    thr = None if self.thr is None else entry.SlotOccurrenceThresholdConfig(self.thr, {})
    return entry.make_table_config(parts, entry.CuckooHashTableConfig(**self.kw), learning_rates=self.lrs,
                                   slot_occurrence_threshold_config=thr)

  def oracle_table(self):
    segs = [O.segment(d, _opt(o)[0], p=_opt(o)[1], init=O.INIT_CONSTANT, init_value=0.25) for d, o in self.segs]
    return O.Table(segs, int(self.kw.get("initial_capacity", 1)))


def _make(tabs, flt=None):
  return MultiHashTable.from_configs({n: t.entry_cfg() for n, t in tabs.items()}, name_suffix=_name(),
                                     hash_filter=flt)


# =============================================================================== id streams, gradients
@functools.lru_cache(maxsize=8)
def _stream(seed, slot=1, kind="growing"):
  """STEPS + 1 batches of B ids with feature slot ``slot``.

  growing: per step 2000 ids never seen before, 1000 distinct ids of the previous batch, one id 40 times and
  one 300 times in EVERY step, a new id 33 times and a new id 32 times, and draws from a pool of 200 ids for
  the rest (short lists).  zipf: Zipf(1.3) over 1500 ids (what the filter cases use: most ids come back).
  The 1500 ids are spread over 47 bits, as hashed feature ids are: the counting filter tells two ids that
  land in one probe window apart by a 12-bit signature taken from bits 17 .. 28 of the id (hash_filter.h),
  so ids that are all below 2^17 share one signature and are counted together wherever their windows meet
  — the reference's behaviour, which the dict of the host model (``_admit``) does not restate."""
  rng = np.random.default_rng(seed)
  tag = np.int64(slot) << 48
  if kind == "zipf":
    universe = np.unique(rng.integers(1, 1 << 47, 1600))[:1500].astype(np.int64)
    rng.shuffle(universe)
    return tuple((universe[rng.zipf(1.3, B) % 1500] | tag) for _ in range(STEPS + 1))
  uniq = (rng.permutation(1 << 22)[:(STEPS + 1) * 3100 + 300].astype(np.int64) + 1) | tag
  pool, h40, h300, rest = uniq[:200], uniq[200], uniq[201], uniq[300:]
  out = []
  for s in range(STEPS + 1):
    mine = rest[s * 3100:(s + 1) * 3100]
    parts = [mine[:2000], np.full(40, h40), np.full(300, h300), np.full(33, mine[2000]), np.full(32, mine[2001])]
    again = np.setdiff1d(out[-1], [h40, h300]) if out else None   # (the two fixed lists keep their lengths)
    parts.append(rng.choice(again, 1000, replace=False) if out else mine[2002:3002])
    parts.append(rng.choice(pool, B - sum(p.size for p in parts)))
    b = np.concatenate(parts).astype(np.int64)
    rng.shuffle(b)
    assert b.size == B
    out.append(b)
  return tuple(out)


def _assert_stream_shape(batches):
  """what the module docstring promises of the ``growing`` stream"""
  seen = set()
  for s, b in enumerate(batches[:STEPS]):
    u, c = np.unique(b, return_counts=True)
    assert {32, 33, 40}.issubset(set(c.tolist())) and c.max() >= 300, s
    new = [k for k in u.tolist() if k not in seen]
    assert len(new) >= 2000, s                                         # is_new rows, every step
    if s:
      assert np.intersect1d(u, np.unique(batches[s - 1])).size >= 1000, s   # rows the last step wrote
      assert any(k not in seen for k in u[c > LIGHT_MAX].tolist()), s  # a heavy list of a NEW id
    seen.update(u.tolist())


def _grads(seed, s, dim):
  return (np.random.default_rng(1000 * seed + s).standard_normal((B, dim)) * 0.1).astype(np.float32)


# =============================================================================== the oracle's side
def _sum_lists(ids, g):
  """(distinct ids in first-occurrence order, their gradient sums in occurrence order, occurrence counts)"""
  n, dim = ids.size, g.shape[1]
  uk, _, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, n], [dim])
  gu = O.fill_with_offset_map_gradient(np.arange(uk.size), [0, uk.size], g.ravel(), vo, vos, [dim]).reshape(-1, dim)
  return uk, gu, np.diff(vos)


def _admit(seen, present, uk, cnt, thr):
  """The host model of test_pipelined_step_with_hash_filter_matches_model: the step asks the filter once per
  distinct id that is not in the table, with its occurrence count; counts saturate at 15; an id whose count
  BEFORE the call reached the threshold is admitted."""
  keep = []
  for k_, (i, c) in enumerate(zip(uk.tolist(), cnt.tolist())):
    if i in present:
      keep.append(k_)
      continue
    c0 = seen.get(i, 0)
    seen[i] = min(15, c0 + min(15, int(c)))
    if c0 >= thr:
      keep.append(k_)
      present.add(i)
  return keep


class Expected:
  """What the oracle computes for one table over a stream: forward rows per step (``fwd``), final rows of
  every id seen (``rows`` of ``probe``), the rows a heavy list has been applied to (``heavy``, per step
  ``fwd_heavy``), the key count, a dump with the optimizer state and, with a filter, the host model's
  counts (``seen_f``) and admitted ids (``present``)."""


def _oracle_run(tab, batches, seed, order=None):
  e = Expected()
  e.fwd, e.fwd_heavy, e.seen_f, e.present = [], [], {}, set()
  ot = tab.oracle_table()
  heavy = set()
  order = list(range(STEPS)) if order is None else order
  for t, s in enumerate(order):
    ids, g = batches[s], _grads(seed, t, tab.dim)
    e.fwd.append(ot.lookup(ids)[0])
    e.fwd_heavy.append(np.array([k in heavy for k in ids.tolist()]))
    uk, gu, cnt = _sum_lists(ids, g)
    keep = np.arange(uk.size)
    if tab.thr is not None:
      keep = np.array(_admit(e.seen_f, e.present, uk, cnt, tab.thr), dtype=np.int64)
    if keep.size:
      ot.optimize(uk[keep], gu[keep], tab.lrs, 100 + t, global_step=GSTEP + 3 * t)
      heavy.update(uk[keep][cnt[keep] > LIGHT_MAX].tolist())
  e.probe = np.unique(np.concatenate([batches[s] for s in order]))
  e.rows = ot.lookup(e.probe)[0]
  e.heavy = np.array([k in heavy for k in e.probe.tolist()])
  e.size = ot.size()
  e.dump = ot.dump()
  return e


@functools.lru_cache(maxsize=1)
def _expected_cached(tab_key, seed, slot, kind):
  segs, sr16, thr, kw = tab_key
  return _oracle_run(Tab(segs, sr16=sr16, thr=thr, **dict(kw)), _stream(seed, slot, kind), seed)


def _expected(tab, seed, slot=1, kind="growing"):
  """one oracle run per (table, stream), shared by the exact and the tree case that follow each other"""
  return _expected_cached(tab.key(), seed, slot, kind)


# =============================================================================== comparisons
def _compare(got, want, heavy, exact, what):
  """bit for bit; without exact order only on the rows no heavy list was applied to, the others within
  RTOL_TREE / ATOL_TREE (printed first: run with -s to see the margin)"""
  if exact:
    np.testing.assert_array_equal(got, want, err_msg=what)
    return
  np.testing.assert_array_equal(got[~heavy], want[~heavy], err_msg=what + " (light rows)")
  if heavy.any():
    diff = np.abs(got[heavy].astype(np.float64) - want[heavy])
    print("%s: %d heavy rows, max |engine - oracle| %.3g, closest to the bar %.3g"
          % (what, int(heavy.sum()), diff.max(), (diff - ATOL_TREE - RTOL_TREE * np.abs(want[heavy])).max()))
  np.testing.assert_allclose(got[heavy], want[heavy], rtol=RTOL_TREE, atol=ATOL_TREE, err_msg=what + " (heavy rows)")


def _check_rows(got, exp, exact, what=""):
  _compare(got, exp.rows, exp.heavy, exact, what + " final rows")


def _check_fwd(got, exp, s, exact, what=""):
  _compare(got, exp.fwd[s], exp.fwd_heavy[s], exact, "%s forward %d" % (what, s))


def _check_state(mt, name, exp):
  """weights AND optimizer state (the state vectors; Adam's two running powers) through a key-sorted dump.
  Rows are float num[dim] | state(seg 0) | state(seg 1) ... in the engine and in the oracle; the engine pads
  Adam's pair of powers to a float4, which the tables here have in their LAST segment only: the oracle's row
  is a prefix of the engine's."""
  ids, _, _, rows = mt.dump(name)
  o_ids, _, _, o_rows = exp.dump
  a, b = np.argsort(ids.cpu().numpy()), np.argsort(o_ids)
  np.testing.assert_array_equal(ids.cpu().numpy()[a], o_ids[b])
  w = o_rows.shape[1]
  assert rows.shape[1] >= w
  np.testing.assert_array_equal(rows.cpu().numpy()[a][:, :w], o_rows[b], err_msg=name + ": rows with state")


# =============================================================================== single-table driver
def _run_single(tab, seed, exact, kind="growing", check_growth=False, flt=False):
  batches = _stream(seed, 1, kind)
  exp = _expected(tab, seed, 1, kind)
  f = HashFilter(capacity=200000) if flt else None
  mt = _make({"emb": tab}, f)
  assert mt._lib.mhte_table_fused_backward_ok(mt.handle, 0) == 2    # pylint: disable=protected-access
  step = SparseStep(mt, "emb", B, exact_order=exact)
  dev = [ids_t(b) for b in batches]
  hps = []
  for s in range(STEPS):
    emb = step.forward(dev[s], next_ids=dev[s + 1])
    _check_fwd(emb.cpu().numpy(), exp, s, exact)
    step.backward(val_t(_grads(seed, s, tab.dim)), 100 + s, global_step=GSTEP + 3 * s)
    assert step.n_unique() == np.unique(batches[s]).size
    hps.append(mt.stats("emb").hashpower)   # (reads counters: no op on the table, the pipeline goes on)
  if check_growth:
    # the first update sizes the empty table; the later ones double it while hints probed a step ahead wait
    assert hps[-1] - hps[0] >= 2, hps
  got = mt.lookup({"emb": ids_t(exp.probe)})["emb"].cpu().numpy()
  _check_rows(got, exp, exact, "dim %d %s" % (tab.dim, "+".join(o for _, o in tab.segs)))
  assert mt.size("emb") == exp.size
  if exact:
    _check_state(mt, "emb", exp)
  st = mt.stats("emb")
  assert st.dropped == 0
  return mt, exp, f


# =============================================================================== 1. the OPTK instances
def test_the_growing_stream_holds_what_the_cases_need():
  _assert_stream_shape(_stream(7))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dim", [8, 64, 100, 256])
@pytest.mark.parametrize("name", OPTK)
def test_one_segment_full_tables_on_every_lane_shape(name, dim, exact):
  """``step_bwd_kernel<G, 4, true, true, OPTK>``: six optimizers x G = 8 / 16 / 32 / 64 float4 lanes.  Their
  own code is ``row_prefetch_full``, the ``RowRegsF`` hand-over into ``optimize_row_reg_full`` and the
  ``if constexpr (PF)`` branches of ``rd_apply_role`` (AMSGrad: an OPTK instance without the prefetch)."""
  _assert_stream_shape(_stream(7))
  _run_single(Tab([(dim, name)]), 7, exact, check_growth=True)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dim", [36, 132])
@pytest.mark.parametrize("name", ["adam", "momentum"])
def test_one_segment_full_tables_with_a_partly_filled_lane_group(name, dim, exact):
  """dim 36: G = 16 with 9 live lanes; dim 132: G = 64 with 33 — ``e >= tv.dim`` lanes prefetch and store
  nothing, and still take part in the group's probe and shuffles."""
  _run_single(Tab([(dim, name)]), 7, exact, check_growth=True)


@pytest.mark.parametrize("name", OPTK)
def test_one_segment_full_tables_restart_the_pipeline(name):
  """The sequence of test_pipelined_step_restart_flushes_deferred_ids on a one-segment FULL table (no
  ``clear`` in between): a pipeline that ends, one that restarts into the same slot, a batch deduplicated
  ahead whose buffer is refilled in place and trained unpipelined."""
  tab, seed = Tab([(64, name)]), 11
  b = _stream(seed)
  order = [0, 1, 2, 4, 5]
  exp = _oracle_run(tab, b, seed, order)
  mt = _make({"emb": tab})
  step = SparseStep(mt, "emb", B, exact_order=True)
  d = [ids_t(x) for x in b]
  t = [0]

  def train(dev_ids, nxt):
    emb = step.forward(dev_ids, next_ids=nxt)
    np.testing.assert_array_equal(emb.cpu().numpy(), exp.fwd[t[0]], err_msg="forward %d" % t[0])
    step.backward(val_t(_grads(seed, t[0], tab.dim)), 100 + t[0], global_step=GSTEP + 3 * t[0])
    t[0] += 1

  train(d[0], d[1])
  train(d[1], None)            # the pipeline ends
  train(d[2], d[3])            # ... and starts again
  buf = d[3]                   # deduplicated ahead ...
  buf.copy_(d[4])              # ... then refilled in place with another batch
  train(buf, None)
  train(d[5], None)
  _check_rows(mt.lookup({"emb": ids_t(exp.probe)})["emb"].cpu().numpy(), exp, True)
  assert mt.size("emb") == exp.size
  _check_state(mt, "emb", exp)


# =============================================================================== 2. the generic instance
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name,dim", [("moving_average", 64), ("moving_average", 132), ("adam", 13),
                                      ("adam", 50), ("momentum", 13), ("momentum", 50)])
def test_generic_one_segment_full_instance(name, dim, exact):
  """``step_bwd_kernel<G, V, true, true>``: MovingAverage (no OPTK instance) on float4 rows; Adam and
  Momentum on rows that are not whole float4s — dim 13: G = 16, dim 50: G = 64, one float per lane."""
  _run_single(Tab([(dim, name)]), 7, exact, check_growth=True)


def test_generic_one_segment_full_instance_with_fp16_rounding():
  """One-segment Adam, dim 64, weights stochastically rounded to binary16 (sr16 tables take the generic
  instance), checked as test_stochastic_rounding_float16 checks its two-segment one: after every update each
  weight is one of the two binary16 neighbours of what the oracle computes from the device's weights before
  it, and the upper neighbour is taken with probability (w - down) / (up - down)."""
  dim, seed = 64, 13
  tab = Tab([(dim, "adam")], sr16=True)
  batches = _stream(seed, 1, "zipf")
  mt, ot = _make({"emb": tab}), tab.oracle_table()
  step = SparseStep(mt, "emb", B, exact_order=True)
  dev = [ids_t(b) for b in batches]
  num = den = 0.0
  n_inexact = 0
  for s in range(STEPS):
    ids, g = batches[s], _grads(seed, s, dim)
    uk = np.unique(ids)
    have = uk[np.array([ot.contains(int(k)) for k in uk], bool)] if ot.size() else uk[:0]
    if have.size:   # the oracle continues from the device's (rounded) weights: Assign overwrites weights only
      ot.assign(have, mt.lookup({"emb": ids_t(have)})["emb"].cpu().numpy(), 50)
    uo, gu, _ = _sum_lists(ids, g)
    ot.optimize(uo, gu, tab.lrs, 100 + s)
    step.forward(dev[s], next_ids=dev[s + 1])
    step.backward(val_t(g), 100 + s)
    w = mt.lookup({"emb": ids_t(uk)})["emb"].cpu().numpy()
    exp = ot.lookup(uk)[0]
    dn, up = _half_neighbours(exp)
    assert ((w == dn) | (w == up)).all(), "step %d" % s
    assert (w.astype(np.float16).astype(np.float32) == w).all()
    inexact = up > dn
    frac = (exp - dn)[inexact] / (up - dn)[inexact]
    num += float(((w == up)[inexact].astype(np.float64) - frac).sum())
    den += float((frac * (1 - frac)).sum())
    n_inexact += int(inexact.sum())
  assert mt.size("emb") == ot.size()
  # (Adam's state is checked through the steps: a state that had drifted would take the next step's
  # weights off the neighbour pair)
  assert n_inexact > 30000 and abs(num) / np.sqrt(den) < 5.0, (num, den, n_inexact)


# =============================================================================== 3. FULL + filter
@pytest.mark.parametrize("segs", [((64, "adam"),), ((4, "ftrl"), (28, "adam")), ((13, "momentum"),)],
                         ids=["adam64", "ftrl4_adam28", "momentum13"])
def test_full_tables_with_an_admission_filter(segs):
  """``step_bwd_kernel<G, V, *, true, -1, true>``: the FULL instances that consult the filter, one segment
  (float4 and one float per lane) and two segments, against the host model (saturating counts; the oracle
  sees admitted ids only)."""
  tab = Tab(segs, thr=3)
  mt, exp, flt = _run_single(tab, 17, True, kind="zipf", flt=True)
  assert mt.size("emb") == len(exp.present) and 0 < len(exp.present) < exp.probe.size
  np.testing.assert_array_equal(flt.get(ids_t(exp.probe)).cpu().numpy(),
                                [exp.seen_f.get(int(i), 0) for i in exp.probe])


# =============================================================================== 4. displacement pass
@pytest.mark.parametrize("segs", [((64, "adam"),), ((8, "momentum"),), ((4, "ftrl"), (28, "amsgrad"))],
                         ids=["adam64", "momentum8", "ftrl4_amsgrad28"])
def test_full_updates_in_the_displacement_pass_at_high_load(segs):
  """The recipe of test_pipelined_step_slow_path_at_high_load (2^13 slots at load 0.97, every id twice, a
  quarter of the previous batch again) on FULL tables: the pass that rides in the next forward launch
  (``step_fwd_kernel<G, V, unr, false>``) applies Adam / Momentum / AMSGrad updates to the ids it places."""
  cap, n, steps = 1 << 13, 3000, 4
  tab = Tab(segs, initial_capacity=cap, max_load_factor=0.97)
  mt, ot = _make({"emb": tab}), tab.oracle_table()
  step = SparseStep(mt, "emb", n, exact_order=True)
  rng = np.random.default_rng(12)
  batches = []
  for s in range(steps + 1):
    ids = rng.integers(1, 2**60, n)
    ids[n // 2:] = ids[:n - n // 2]
    if s > 0:
      ids[:n // 4] = batches[-1][:n // 4]
    batches.append(ids)
  dev = [ids_t(b) for b in batches]
  deferred = 0
  for s in range(steps):
    g = (np.random.default_rng(s).standard_normal((n, tab.dim)) * 0.1).astype(np.float32)
    emb = step.forward(dev[s], next_ids=dev[s + 1])
    np.testing.assert_array_equal(emb.cpu().numpy(), ot.lookup(batches[s])[0], err_msg="forward %d" % s)
    # (between forward and backward nothing is queued: the dump disturbs no pass)
    deferred += _must_defer(mt, batches[s], 11)
    step.backward(val_t(g), 100 + s, global_step=GSTEP + 3 * s)
    uk, gu, _ = _sum_lists(batches[s], g)
    ot.optimize(uk, gu, tab.lrs, 100 + s, global_step=GSTEP + 3 * s)
  st = mt.stats("emb")
  assert st.dropped == 0 and st.hashpower == 11 and st.size > 0.5 * cap
  assert deferred > 0          # (updates really queued ids for the pass)
  allids = np.unique(np.concatenate(batches[:steps]))
  np.testing.assert_array_equal(mt.lookup({"emb": ids_t(allids)})["emb"].cpu().numpy(), ot.lookup(allids)[0])
  assert mt.size("emb") == ot.size()


@pytest.mark.parametrize("name", ["adam", "adagrad"])
def test_full_batch_forward_with_three_ids_per_lane_group(name):
  """``step_fwd_kernel<G, V, 3, *>``: the forward launch gives a lane group three ids instead of two once two
  per group would need more than two trips of its resident workgroups — 65 536 ids on rows of G >= 32 lanes.
  Dim 100 (G = 32), the maximum batch, two pipelined steps, a FULL and a BASIC table."""
  n, dim, steps, seed = 65536, 100, 2, 29
  tab = Tab([(dim, name)], initial_capacity=1 << 18)
  mt, ot = _make({"emb": tab}), tab.oracle_table()
  step = SparseStep(mt, "emb", n, exact_order=True)
  rng = np.random.default_rng(seed)
  batches = [rng.integers(1, 150000, n).astype(np.int64) | (np.int64(1) << 48) for _ in range(steps + 1)]
  dev = [ids_t(b) for b in batches]
  for s in range(steps):
    g = (np.random.default_rng(seed + s).standard_normal((n, dim)) * 0.1).astype(np.float32)
    emb = step.forward(dev[s], next_ids=dev[s + 1])
    np.testing.assert_array_equal(emb.cpu().numpy(), ot.lookup(batches[s])[0], err_msg="forward %d" % s)
    step.backward(val_t(g), 100 + s, global_step=GSTEP + 3 * s)
    uk, gu, _ = _sum_lists(batches[s], g)
    ot.optimize(uk, gu, tab.lrs, 100 + s, global_step=GSTEP + 3 * s)
  probe = np.unique(np.concatenate(batches[:steps]))
  np.testing.assert_array_equal(mt.lookup({"emb": ids_t(probe)})["emb"].cpu().numpy(), ot.lookup(probe)[0])
  assert mt.size("emb") == ot.size()


# =============================================================================== 5. multi-table step
_MULTI = {   # sorted-name order = order in the flat buffers: the wide table in front of the odd dims
    "a_adam64": ((64, "adam"),),
    "b_adam256": ((256, "adam"),),
    "c_momentum13": ((13, "momentum"),),
    "d_bias_adam": ((1, "ftrl"), (16, "adam")),
    "e_adagrad32": ((32, "adagrad"),),
    # (not in the list the FULL families need: the BASIC families the filtered launches have not run yet —
    # one float per lane with one segment and with two, float4 lanes with two segments)
    "f_adagrad13": ((13, "adagrad"),),
    "g_bias_adagrad": ((1, "ftrl"), (16, "adagrad")),
    "h_ftrl4_adagrad28": ((4, "ftrl"), (28, "adagrad")),
}


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("filtered", [False, True])
def test_multi_table_step_full_families(filtered, exact):
  """``mstep_bwd_kernel<full, width, oneseg, filt>`` beyond the dims-16 / 32 / 17 two-segment rows of the rest
  of the suite: one-segment FULL float4 tables of dims 64 and 256, a one-segment FULL table with one float
  per lane, a bias FTRL + Adam row and BASIC tables of every family in ONE model — all sixteen instances;
  with a HashFilter attached every launch takes its ``filt`` instance and each table follows the host model
  of section 3."""
  seed = 23
  kind = "zipf" if filtered else "growing"
  tabs = {n: Tab(segs, thr=3 if filtered else None) for n, segs in _MULTI.items()}
  names = sorted(tabs)
  flt = HashFilter(capacity=600000) if filtered else None
  mt = _make(tabs, flt)
  step = MultiSparseStep(mt, B, exact_order=exact)
  streams = {n: _stream(seed + k, k + 1, kind) for k, n in enumerate(names)}
  exps = {n: _oracle_run(tabs[n], streams[n], seed + k) for k, n in enumerate(names)}
  rag = [mt.get_ragged_id({n: ids_t(streams[n][s]) for n in names}) for s in range(STEPS + 1)]
  for s in range(STEPS):
    emb = step.forward(rag[s], rag[s + 1])
    views = mt.get_embeddings(rag[s], emb)
    for n in names:
      _check_fwd(views[n].cpu().numpy(), exps[n], s, exact, n)
    flat = np.concatenate([_grads(seed + k, s, tabs[n].dim).ravel() for k, n in enumerate(names)])
    step.backward(val_t(flat), 100 + s, global_step=GSTEP + 3 * s)
  for n in names:
    exp = exps[n]
    got = mt.lookup({n: ids_t(exp.probe)})[n].cpu().numpy()
    _check_rows(got, exp, exact, n)
    assert mt.size(n) == exp.size, n
    if filtered:
      assert 0 < len(exp.present) < exp.probe.size and exp.size == len(exp.present), n
      np.testing.assert_array_equal(flt.get(ids_t(exp.probe)).cpu().numpy(),
                                    [exp.seen_f.get(int(i), 0) for i in exp.probe], err_msg=n)
    elif exact:
      _check_state(mt, n, exp)
  step.close()


# =============================================================================== 6. GroupAdaGrad
def _group_specs(which):
  """Rows whose GroupAdaGrad segment takes more than one trip of G * VEC floats, starts inside a trip, or
  needs G = 32 / 64 lanes.  ``all``: dims 260 and 81 do not fit the one-launch segment kernels, so the
  fused ops take the per-table op-level kernels (``upsert_kernel<G, V, kOpOptimize, true>``); ``seg``: the
  rows that do fit them (``seg_upsert_kernel<VW, true>``)."""
  specs = [M.Spec("a_group64", [(64, "group", 0.02)], 1),                     # G = 16
           M.Spec("b_group100", [(100, "group", 0.02)], 2),                   # G = 32
           M.Spec("d_mixed136", [(24, "adagrad", 0.01), (40, "group", 0.02), (72, "group", 0.01)], 4)]
  if which != "seg":
    specs += [M.Spec("c_group260", [(260, "group", 0.02)], 3),               # G = 64, float4: two trips
              # one float per lane, G = 64: the segment covers floats 1 .. 80 — two trips, the first from float 1
              M.Spec("e_bias_group80", [(1, "ftrl", 0.05), (80, "group", 0.02)], 5)]
  if which == "all+odd":   # G = 16 and 32 with one float per lane (last in the flat buffers: odd dims)
    specs += [M.Spec("f_bias_group12", [(1, "ftrl", 0.05), (12, "group", 0.02)], 6),
              M.Spec("g_bias_group24", [(1, "ftrl", 0.05), (24, "group", 0.02)], 7)]
  return sorted(specs, key=lambda s: s.name)


def _group_grads(rng, n, dim):
  """a tenth of the rows get gradients so small that ||z|| < l2: the group-lasso branch that zeroes the
  segment"""
  g = (rng.standard_normal((n, dim)) * 0.05).astype(np.float32)
  g[rng.random(n) < 0.1] *= np.float32(1e-4)
  return g


def _check_group_tables(mt, ots, specs):
  for sp in specs:
    ids_, _, _, rows_ = mt.dump(sp.name)
    probe = np.sort(ids_.cpu().numpy())
    assert probe.size == ots[sp.name].size(), sp.name
    np.testing.assert_array_equal(mt.lookup({sp.name: ids_t(probe)})[sp.name].cpu().numpy(),
                                  ots[sp.name].lookup(probe)[0], err_msg=sp.name)
    o_ids, _, _, o_rows = ots[sp.name].dump()
    if rows_.shape[1] == o_rows.shape[1]:     # (the accumulators too)
      a, b = np.argsort(ids_.cpu().numpy()), np.argsort(o_ids)
      np.testing.assert_array_equal(rows_.cpu().numpy()[a], o_rows[b], err_msg=sp.name + " (rows with state)")
    assert mt.stats(sp.name).dropped == 0


@pytest.mark.parametrize("which,shards", [("all", 1), ("all", 2), ("seg", 1)])
def test_group_adagrad_beyond_one_trip_fused_ops(which, shards):
  """FusedLookup / FusedOptimize over [shard][table] segments, ids distinct inside a segment — the entry point
  test_fused_optimize_with_whole_segment_optimizer uses — on the rows of ``_group_specs``, bit for bit.  With
  two shards the second shard's segments follow the 81-float table in the flat buffers: the float4 tables run
  with one float per lane there (group(260): five trips)."""
  specs = _group_specs(which)
  mt = M.make(specs)
  T = len(specs)
  ots = {s.name: s.oracle_table() for s in specs}
  rng = np.random.default_rng(31 + shards)
  mt.set_learning_rate([lr for sp in specs for lr in sp.lrs()])
  for it in range(3):
    per = {sp.name: np.unique(rng.integers(1, 3000, 700).astype(np.int64) | (sp.slot << 48)) for sp in specs}
    segs, fss = [], []
    for sh in range(shards):
      for sp in specs:
        seg = per[sp.name][per[sp.name] % shards == sh]
        segs.append(seg)
        fss.append(seg.size)
    ids = np.concatenate(segs)
    emb, _, id_off, emb_off, idx = mt.fused_lookup(ids_t(ids), fss, shards)
    emb = emb.cpu().numpy()
    for y, seg in enumerate(segs):
      np.testing.assert_array_equal(emb[emb_off[y]:emb_off[y + 1]], ots[specs[y % T].name].lookup(seg)[0].ravel())
    grads = np.concatenate([_group_grads(rng, seg.size, specs[y % T].dim).ravel() for y, seg in enumerate(segs)])
    mt.fused_apply_gradient(ids_t(ids), idx, fss, val_t(grads), id_off[:-1], emb_off[:-1], global_step=it,
                            req_time=100 + it, num_of_shards=shards, ids_unique_per_segment=True)
    for y, seg in enumerate(segs):
      sp = specs[y % T]
      if seg.size:
        ots[sp.name].optimize(seg, grads[emb_off[y]:emb_off[y + 1]].reshape(-1, sp.dim), sp.lrs(), 100 + it)
  _check_group_tables(mt, ots, specs)


@pytest.mark.parametrize("summed", [False, True])
def test_group_adagrad_beyond_one_trip_with_duplicates(summed):
  """``apply_gradients`` with duplicate ids: ONE Optimize() per occurrence, in order
  (cuckoo_embedding_hash_table.cc:229-236); and ``mhte_table_optimize_n`` with MHTE_SUM_DUPLICATES: the
  occurrences added in order, one Optimize() per id (tf_bridge.cc:270-310) — the two forms of
  ``group_adagrad_segment``'s ``grad_of``."""
  specs = _group_specs("all+odd")
  mt = M.make(specs)
  ots = {s.name: s.oracle_table() for s in specs}
  rng = np.random.default_rng(41 + int(summed))
  n = 1500
  for it in range(3):
    batch = {}
    for sp in specs:
      ids = (rng.zipf(1.5, n) % 400).astype(np.int64) | (sp.slot << 48)
      g = _group_grads(rng, n, sp.dim)
      batch[sp.name] = (ids, g)
      if summed:
        uk, gu, _ = _sum_lists(ids, g)
        ots[sp.name].optimize(uk, gu, sp.lrs(), 100 + it)
        mt.table_optimize_n(sp.name, ids_t(ids), None, val_t(g), np.array(sp.lrs(), np.float32), 100 + it,
                            flags=_lib.MHTE_SUM_DUPLICATES)
      else:
        ots[sp.name].optimize(ids, g, sp.lrs(), 100 + it)
    if not summed:
      mt.apply_gradients({nm: (ids_t(i), val_t(g)) for nm, (i, g) in batch.items()}, req_time=100 + it)
    torch.cuda.synchronize()
  _check_group_tables(mt, ots, specs)
