"""The multi-table step (``MultiSparseStep``: csrc/mhte_mstep_kernels.h, csrc/mhte_mstep_host.h) at every size edge
of the run dedup, through every forward form and restart (-m gpu).

The batches are those of tests/multi_step_truth.py: all of ``run_dedup_truth.CASES`` plus the ``cut`` family, dealt
one case per table of a model (tests/test_multi_step_truth_cpu.py asserts what the cases and the deal reach).  A
group is a pipeline of 4 steps (6 batches per table, consecutive seeds).

Models (table order = sorted name = order in the flat buffers; zeros initializer everywhere):
  small    a dim 4, b dim 5, c dim 8; SGD, lr 1.  ``item_target`` 256, ``item_split`` 1.  b moves one float per
           lane and pushes c off its 16-byte boundary whenever n_a * 4 + n_b * 5 is no multiple of 4.
  wide     small + d dim 16 + e dim 4.  ``item_target`` 1024, ``item_split`` 4.
  chunked  f00 .. f31 (dim 4, a few ids each) + y dim 5 + z dim 8: 34 tables, the case tables y and z are the
           second chunk of every launch (``ids + split[t0]``, ``id_off`` relative to the chunk).
  order    a dim 16, b dim 17, c dim 32; Adagrad, normal gradients, ``exact_order=True``.

Bars.  Before a pipeline starts every id of every batch is ASSIGNED a row that names it (a number unique to the id,
below 2^22, plus the column index), in the engine and in the oracle, so every element of every forward output says
whose row it is.  Gradients are integers in [-8, 8] and lr is 1: every row and every partial sum is an integer
below 2^24 (asserted), every association of a sum has the same bits, and every comparison is bit for bit in
every form.  The ``order`` model has real gradients: its naming rows are scaled by 2^-40 (exact, and far below the
rounding of an update) and it runs with ``exact_order`` only, bit for bit — that is what sees a list summed in the
wrong order; the bar without ``exact_order`` is held by test_multi_step_gpu.py and test_optimizer_shapes_gpu.py.

Forms, and the launches a step takes in them (lookup1 = ``mstep_fwd_kernel<256, 1>`` for the tables that move one
float per lane, which get no lookup blocks in the fused launch: ``fwd_start[t] == fwd_start[t + 1]`` for table b
in every group, and for c wherever b misaligns it; bwd = ``mstep_bwd_kernel`` instances + ``mstep_slow_kernel``):
  fused      forward(b[s], b[s+1]): lookup1, ``mstep_fwd_dedup_kernel`` (lookup of s | dedup of s + 1);
             backward: bwd (apply of s | numbering of s + 1).  Step 0 first runs ``dedup_now``.
  fused-1wg  the same with MHTE_MSTEP_FUSE_DEDUP_WGS=1, MHTE_MSTEP_FUSE_LOOKUP_WGS=2: ONE dedup workgroup walks
             every item of every table in turn, two lookup workgroups per table take several trips.
  two        MHTE_MSTEP_FUSE_FWD=0: ``launch_fwd`` (``mstep_fwd_kernel<256, 4>`` and lookup1), then
             ``launch_dedup`` (``mstep_dedup_kernel``, one workgroup per item); backward as above.
  side       MHTE_MSTEP_SIDE=1: ``mstep_dedup_kernel`` on the side stream with up to 128 persistent workgroups,
             ``launch_fwd`` on the main stream; backward joins the side stream, then as above.
  side-1wg   the same with MHTE_MSTEP_DEDUP_WGS=1: one persistent workgroup for every item of every table.
  no-ahead   forward(b[s], None) every step: ``dedup_now`` (``mstep_dedup_kernel`` + the build-only backward
             launch), ``launch_fwd``; backward applies only.
  ffb        forward(old batch, b[s]); forward(b[s], b[s+1]); backward: the second forward picks b[s] up
             deduplicated but un-numbered (``stage == 1``: the build-only launch inside ``forward``), and every
             step restarts the pipeline over a slot that still holds a numbered batch.  (The ``stage == 1``
             branch of ``backward`` cannot be reached through ``forward``, which always leaves the current slot
             numbered.)
  chunked    the 34-table model: more than kMaxStepTables tables, so ``launch_fwd`` + ``launch_dedup`` in two
             chunks each and two chunks of the backward launch.
MHTE_MSTEP_FUSE_INTERLEAVE is a function-local static read once per process: it cannot be switched per test and is
left out.

Coverage.  Every case runs in ``fused`` and ``two`` on ``small`` and in ``fused`` on ``wide``; the families
edge, reserved, long and cut, the runs of 32, 33 and 1024 and the sizes 1, 255, 257, 1023, 1024, 1025 (groups
"f..") run in every other form on ``small`` and in ``chunked``; the three cases of 64 513 to 65 536 ids run in
``fused`` and ``two`` only.  The final rows of all forms of a model that ran a group are compared bit for bit
with each other as well as with the oracle.

Which case and form reaches what:
  item-to-table mapping (``blk_start``, ``id_off``), persistent loop    every group (tables of different sizes side by
    over items of DIFFERENT tables with one ``RdLds``                   side) in fused-1wg and side-1wg: one workgroup
                                                                        walks all items (no group has more blocks than
                                                                        the 128 default workgroups of fused / side)
  a table with zero blocks in the middle of ``blk_start``               group f00 / o00 of every model: the middle table
                                                                        has no ids in batches 1 and 3; filler f16 of ``chunked``
  a last block of 1, 255, 1023 positions, table not the last            size-*-1 / 1025, size-*-255, size-*-1023 (the deal
                                                                        keeps them off the last table)
  relative ``id_off`` in the second chunk                               ``chunked``
  ``fwd_start[t] == fwd_start[t + 1]``                                  table b (and a misaligned c) of every fused group
  list of exactly 32 | 33 through ``hlist`` | items                     run-32-*, run-33-*, edge-32=*, edge-33=*,
                                                                        reserved-run32 / run33
  a run of exactly 1024                                                 run-1024-*, reserved-workgroup, size-equal-1024
  64 runs of one occurrence in one item                                 edge-64=1x64 (33 of them: reserved-33-singles)
  E not a multiple of 64; item_split 4 with fewer than four passes      the heavy lists of 33 .. 257 on ``wide``
  the item cut 512 | 513, 1024 | 1025 (target 256)                      cut-t256-* on ``small`` (cut-t1024-* lie on its
                                                                        next edges, 8 | 4 and 4 | 2 workgroups per item)
  the item cut 2048 | 2049, 4096 | 4097 (target 1024)                   cut-t1024-* on ``wide``
  the order inside a list                                               ``order`` model, exact order
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multi_step_truth as M  # noqa: E402
import run_dedup_truth as R  # noqa: E402
from monolith_amd import synthetic as S  # noqa: E402
from monolith_amd.fused_step import MultiSparseStep  # noqa: E402
from test_multi_step_gpu import Spec, ids_t, make, oracle_backward, val_t  # noqa: E402

STEPS = 4
ENV_VARS = ("MHTE_MSTEP_FUSE_DEDUP_WGS", "MHTE_MSTEP_FUSE_LOOKUP_WGS", "MHTE_MSTEP_FUSE_FWD", "MHTE_MSTEP_SIDE",
            "MHTE_MSTEP_DEDUP_WGS", "MHTE_MSTEP_ITEM_TARGET", "MHTE_MSTEP_OVERSUB", "MHTE_MSTEP_SCATTER_OVS")
FORMS = {
    "fused": {},
    "fused-1wg": {"MHTE_MSTEP_FUSE_DEDUP_WGS": "1", "MHTE_MSTEP_FUSE_LOOKUP_WGS": "2"},
    "two": {"MHTE_MSTEP_FUSE_FWD": "0"},
    "side": {"MHTE_MSTEP_SIDE": "1"},
    "side-1wg": {"MHTE_MSTEP_SIDE": "1", "MHTE_MSTEP_DEDUP_WGS": "1"},
    "no-ahead": {},
    "ffb": {},
}
EVERY_CASE_FORMS = ("fused", "two")
OTHER_FORMS = ("fused-1wg", "side", "side-1wg", "no-ahead", "ffb")

INT_DIMS = {"small": (("a", 4), ("b", 5), ("c", 8)),
            "wide": (("a", 4), ("b", 5), ("c", 8), ("d", 16), ("e", 4))}
ORDER_DIMS = (("a", 16), ("b", 17), ("c", 32))
N_FILLERS = 32
CHUNKED_DIMS = tuple(("f%02d" % i, 4) for i in range(N_FILLERS)) + (("y", 5), ("z", 8))
FILLER_HOLE = 16
ORDER_LR = 0.05


def _np(t):
  return t.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pow2(n):
  return 1 << max(4, int(n - 1).bit_length())


# ---------------------------------------------------------------------------------------------- a pipeline
class Pipeline:
  """The batches of every table of a model, their gradients, and what the oracle makes of them: the rows
  ``forward`` must return for every table at every step, the distinct ids, the final rows of every id."""

  def __init__(self, dims, batches, kind):
    # batches[s][t]: ids of table t (sorted-name order) in batch s
    assert len(batches) == STEPS + 2 and all(len(b) == len(dims) for b in batches)
    self.kind, self.batches = kind, batches
    self.T = len(dims)
    self.max_batch = max(1, max(ids.size for b in batches for ids in b))
    self.named = []
    self.specs = []
    for t, (name, dim) in enumerate(dims):
      every = np.concatenate([b[t] for b in batches])
      self.named.append(R.naming_rows(every, dim, 77 + t, 1.0 if kind == "int" else R.NAME_TINY))
      opt = ("sgd", 1.0) if kind == "int" else ("adagrad", ORDER_LR)
      self.specs.append(Spec(name, [(dim, opt[0], opt[1])], t + 1,
                             initial_capacity=_pow2(2 * self.named[t][0].size)))
    assert [s.name for s in self.specs] == sorted(s.name for s in self.specs)
    self.grads = [[self._grad(s, t, batches[s][t].size) for t in range(self.T)] for s in range(STEPS)]
    ots = [sp.oracle_table() for sp in self.specs]
    for ot, (ids, rows) in zip(ots, self.named):
      ot.assign(ids, rows, S.update_time(0))
    self.emb, self.uniq, self.old_emb = [], [], []
    for s in range(STEPS):
      old = batches[STEPS + 1] if s == 0 else batches[s - 1]     # (the forward-only batch of the ffb form)
      self.old_emb.append([self._lookup(ots[t], old[t], t) for t in range(self.T)])
      self.emb.append([self._lookup(ots[t], batches[s][t], t) for t in range(self.T)])
      self.uniq.append([np.unique(batches[s][t]).size for t in range(self.T)])
      for t, sp in enumerate(self.specs):
        if batches[s][t].size:
          uk, gu = oracle_backward(ots[t], sp, batches[s][t], self.grads[s][t])
          ots[t].optimize(uk, gu, sp.lrs(), S.update_time(s))
    self.rows = [ots[t].lookup(self.named[t][0])[0].copy() for t in range(self.T)]
    self.sizes = [ots[t].size() for t in range(self.T)]
    assert self.sizes == [ids.size for ids, _ in self.named]
    if kind == "int":   # the premise of the exact bar
      for rows in self.rows:
        assert np.abs(rows).max() < 2 ** 24 and (rows == np.round(rows)).all()
    self.grads_dev = [val_t(np.concatenate([g.ravel() for g in gs])) for gs in self.grads]

  def _grad(self, s, t, n):
    dim = self.specs[t].dim
    if self.kind == "int":
      return np.random.default_rng(900 + 10 * s + t).integers(-8, 9, size=(n, dim)).astype(np.float32)
    return (S.grad_batch(10 * s + t, n, dim) * 10).astype(np.float32) if n else np.zeros((0, dim), np.float32)

  def _lookup(self, ot, ids, t):
    return ot.lookup(ids)[0].copy() if ids.size else np.zeros((0, self.specs[t].dim), np.float32)

  def table(self):
    mt = make(self.specs)
    mt.assign({sp.name: (ids_t(ids), val_t(rows)) for sp, (ids, rows) in zip(self.specs, self.named)},
              req_time=S.update_time(0))
    return mt

  def check_forward(self, mt, step, rag, emb, expected, uniq, what):
    views = mt.get_embeddings(rag, emb)
    for t, sp in enumerate(self.specs):
      np.testing.assert_array_equal(_np(views[sp.name]), expected[t], err_msg="%s: rows of forward, table %s" %
                                    (what, sp.name))
    if uniq is not None:
      np.testing.assert_array_equal(step.unique_counts(), uniq, err_msg="%s: unique counts" % what)

  def run(self, form, exact=False):
    """The pipeline in one form, checked against the oracle step by step; the final rows per table."""
    mt = self.table()
    step = MultiSparseStep(mt, self.max_batch, exact_order=exact)
    rag = [mt.get_ragged_id({sp.name: ids_t(b[t]) for t, sp in enumerate(self.specs)}) for b in self.batches]
    for s in range(STEPS):
      what = "form %s, step %d" % (form, s)
      if form == "ffb":
        old = STEPS + 1 if s == 0 else s - 1
        emb = step.forward(rag[old], rag[s])
        self.check_forward(mt, step, rag[old], emb, self.old_emb[s], None, what + " (forward only)")
      emb = step.forward(rag[s], None if form == "no-ahead" else rag[s + 1])
      self.check_forward(mt, step, rag[s], emb, self.emb[s], self.uniq[s], what)
      step.backward(self.grads_dev[s], S.update_time(s))
    got = []
    for t, sp in enumerate(self.specs):
      rows = _np(mt.lookup({sp.name: ids_t(self.named[t][0])})[sp.name])
      np.testing.assert_array_equal(rows, self.rows[t], err_msg="form %s: final rows of table %s" % (form, sp.name))
      assert mt.size(sp.name) == self.sizes[t], (form, sp.name)
      got.append(_bits(rows))
    step.close()
    mt.close()
    return got


def _filler_batches():
  """[batch][filler] -> a few ids with repeats; filler FILLER_HOLE has none in batches 1 and 3."""
  rng = np.random.default_rng(31)
  out = []
  for s in range(STEPS + 2):
    row = []
    for i in range(N_FILLERS):
      n = 0 if (i == FILLER_HOLE and s in M.EMPTY_STEPS) else 1 + (i + s) % 5
      row.append(rng.integers(1, 40, n).astype(np.int64) | ((i + 1) << 48))
    out.append(row)
  return out


GROUPS = {"small": M.model_groups(3), "wide": M.model_groups(5),
          "chunked": [g for g in M.model_groups(2) if g[3]],
          "order": [("r%02d" % g, group, M.emptied_table(g, 3), True)
                    for g, group in enumerate(M.deal(M.order_cases(), 3))]}


@functools.lru_cache(maxsize=2)
def _pipeline(model, label):
  """(groups run in one form after the other: the oracle's pass is made once per group)"""
  _, group, hole, _ = [g for g in GROUPS[model] if g[0] == label][0]
  batches = M.deal_batches(group, hole)
  if model == "chunked":
    batches = [f + b for f, b in zip(_filler_batches(), batches)]
    return Pipeline(CHUNKED_DIMS, batches, "int")
  if model == "order":
    return Pipeline(ORDER_DIMS, batches, "normal")
  return Pipeline(INT_DIMS[model], batches, "int")


_FINAL = {}   # (model, label) -> (form, final rows per table) of the first form that ran the group


def _run(monkeypatch, model, label, form, exact=False):
  for k in ENV_VARS:
    monkeypatch.delenv(k, raising=False)
  for k, v in FORMS.get(form, {}).items():
    monkeypatch.setenv(k, v)
  got = _pipeline(model, label).run(form, exact)
  first = _FINAL.setdefault((model, label), (form, got))
  for t, (a, b) in enumerate(zip(got, first[1])):
    np.testing.assert_array_equal(a, b, err_msg="final rows of table %d, form %s | %s" % (t, form, first[0]))
  torch.cuda.synchronize()


def _params(model, plan):
  """Group-major: [(label, form)] with ``plan(every_form) -> forms`` for a group."""
  return [pytest.param(label, form, id="%s-%s" % (label, form))
          for label, _, _, every in GROUPS[model] for form in plan(every)]


# ============================================================ a. small: target 256, every form and restart
@pytest.mark.parametrize("label,form", _params("small", lambda e: EVERY_CASE_FORMS + (OTHER_FORMS if e else ())))
def test_small_model_every_form_equals_oracle(monkeypatch, label, form):
  _run(monkeypatch, "small", label, form)


# ================================================================ b. wide: target 1024, item_split 4, fused
@pytest.mark.parametrize("label,form", _params("wide", lambda e: ("fused",)))
def test_wide_model_fused_equals_oracle(monkeypatch, label, form):
  _run(monkeypatch, "wide", label, form)


# =========================================================== c. 34 tables: the case tables in the second chunk
@pytest.mark.parametrize("label,form", _params("chunked", lambda e: ("chunked",)))
def test_chunked_model_equals_oracle(monkeypatch, label, form):
  _run(monkeypatch, "chunked", label, form)


# ============================================================= d. normal gradients: the order inside a list
@pytest.mark.parametrize("label,form", _params("order", lambda e: ("fused",)))
def test_order_inside_lists_exact_order_equals_oracle(monkeypatch, label, form):
  _run(monkeypatch, "order", label, form, exact=True)
