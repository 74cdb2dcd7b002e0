"""Every entry point with caller buffers that are only 4-byte aligned (-m gpu).

Almost every launch of the engine picks its lane shape from the alignment of the caller's pointers
(``pick_shape(dim, vec_ok && aligned16(ptr))``): a table whose rows are whole float4s runs VEC = 4 on
16-byte aligned buffers and another template instantiation, VEC = 1 and usually another G, on anything
else.  Fresh torch allocations are always 16-byte aligned, so this module hands in contiguous views one
float into a larger allocation (``_mis``) and compares with the CPU oracle (``oracle.Table``,
``O.unique_key_with_value_and_offset``, ``O.fill_with_offset_map*``) or a sequential fp32 numpy loop.

Bars: bit for bit wherever the summation order is the reference's (every op-level call, the steps with
``exact_order=True``); sums taken as a fixed tree (``exact_order=False``) use the suite's RTOL_TREE /
ATOL_TREE.  The aligned and the misaligned run are never compared bit for bit in tree mode: the chunk
sum has 256 / G groups and G changes with VEC.  Every row of every id touched is compared.

Shapes: batch 4099 (odd; above 4096, where the aligned lookup takes ``lookup_kernel_u`` and the
misaligned one ``lookup_kernel``; five 1024-position dedup workgroups), ids Zipf over 600 with every
third one the same id (one list of ~1367 occurrences: heavy, six 256-entry chunks), three steps.
Dims of float4-capable tables 4 (G 8), 64 (G 16), 68 / 128 (G 32), 132 / 256 (G 64), and one table
that can never be float4: bias FTRL(1) + Adagrad(16), dim 17.

The layout op (section g) has no table: six one-fid slices of widths 4 .. 260 at batch 33, the shapes and the
raw caller of tests/test_layout_forms_gpu.py.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from monolith_amd import _lib, entry, synthetic as S  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd.fused_step import SparseStep  # noqa: E402
from monolith_amd.multi_hash_table_ops import Ragged, _i64p, _stream  # noqa: E402
from test_parity_gpu import (ATOL_TREE, RTOL_TREE, _oracle_step, adagrad_cfg, ids_t, make,  # noqa: E402
                             val_t)

N = 4099
STEPS = 3
LR = 0.05
VEC_DIMS = [4, 64, 68, 128, 132, 256]
ALL_DIMS = VEC_DIMS + [17]       # 17: the control table (never float4)
WIDE_DIMS = [68, 128, 132, 256]  # float4 tables whose row one VEC = 1 lane group cannot cover


def _mis(t):
  """A contiguous copy of ``t`` one float into a larger allocation: 4-byte aligned, not 16."""
  if not isinstance(t, torch.Tensor):
    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
  assert t.dtype == torch.float32
  flat = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
  v = flat[1:].view(t.shape)
  v.copy_(t)
  assert v.is_contiguous() and v.data_ptr() % 16 == 4
  return v


def _mis_empty(*shape):
  return _mis(torch.zeros(shape, dtype=torch.float32))


def _al(t):
  """The aligned counterpart of ``_mis``."""
  if not isinstance(t, torch.Tensor):
    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
  v = t.cuda().contiguous()
  assert v.numel() == 0 or v.data_ptr() % 16 == 0
  return v


def _buf(t, mis):
  return _mis(t) if mis else _al(t)


def _table(dim, **kw):
  """(GPU table, oracle table, learning rates) of the module's shape list."""
  if dim == 17:
    segs_o = [O.segment(1, O.OPT_FTRL, p=(0.1, 1.0, 0.0, 0.0)), O.segment(16, O.OPT_ADAGRAD, p=(0.1, 0.0))]
    segs_e = [entry.CombineAsSegment(1, entry.ZerosInitializer(), entry.FtrlOptimizer(0.03, 0.1, 1.0)),
              entry.CombineAsSegment(16, entry.ZerosInitializer(), entry.AdagradOptimizer(LR, 0.1))]
    lrs = [0.03, LR]
    cfg = entry.make_table_config(segs_e, entry.CuckooHashTableConfig(**kw), learning_rates=lrs)
  else:
    segs_o = [O.segment(dim, O.OPT_ADAGRAD, p=(0.1, 0.0))]
    lrs = [LR]
    cfg = adagrad_cfg(dim, LR, 0.1, **kw)
  return make({"emb": cfg}), O.Table(segs_o, kw.get("initial_capacity", 1)), lrs


def _replay(ot, ids, g, dim, lrs, t):
  """``_oracle_step`` of test_parity_gpu (dedup, occurrence-order gradient sum, one optimizer apply per
  id), with one learning rate per segment for the two-segment control table."""
  if len(lrs) == 1:
    return _oracle_step(ot, ids, g, dim, lrs[0], t)
  n = ids.size
  uk, _, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, n], [dim])
  gu = O.fill_with_offset_map_gradient(np.arange(uk.size), [0, uk.size], g.ravel(), vo, vos,
                                       [dim]).reshape(-1, dim)
  ot.optimize(uk, gu, lrs, t)
  return uk


def _batch(seed):
  ids = S.id_batch(seed, N, 600, "zipf")
  ids[::3] = ids[0]
  return ids


def _same_rows(got, exp, exact, what=""):
  if exact:
    np.testing.assert_array_equal(got, exp, err_msg=what)
  else:
    np.testing.assert_allclose(got, exp, rtol=RTOL_TREE, atol=ATOL_TREE, err_msg=what)


def _check_table(mt, ot, seen, exact, what=""):
  """All rows of all ids touched (weights through lookup, weights + optimizer state through a
  key-sorted dump) and the key count."""
  allids = np.unique(np.concatenate(seen))
  got = mt.lookup({"emb": ids_t(allids)})["emb"].cpu().numpy()
  _same_rows(got, ot.lookup(allids)[0], exact, what + " (weights)")
  assert mt.size("emb") == allids.size == ot.size(), what
  ids, _, ts, rows = mt.dump("emb")
  o_ids, _, o_ts, o_rows = ot.dump()
  a, b = np.argsort(ids.cpu().numpy()), np.argsort(o_ids)
  np.testing.assert_array_equal(ids.cpu().numpy()[a], o_ids[b], err_msg=what)
  np.testing.assert_array_equal(ts.cpu().numpy().astype(np.uint32)[a], o_ts[b], err_msg=what)
  _same_rows(rows.cpu().numpy()[a], o_rows[b], exact, what + " (rows with state)")


def _must_defer(mt, ids, hp):
  """How many of ``ids`` are new to the table and find both of their buckets full already: a lower
  bound of what the update of ``ids`` leaves to the displacement pass."""
  have, pos, _, _ = mt.dump("emb", with_rows=False)
  occ = np.bincount(pos.cpu().numpy() >> 2, minlength=1 << hp)
  known = set(have.cpu().numpy().tolist())
  L = O.lib()
  cnt = 0
  for k in np.unique(ids).tolist():
    if k not in known:
      hv = L.mo_hash(k)
      i1 = hv & ((1 << hp) - 1)
      i2 = L.mo_alt_index(hp, L.mo_partial(hv), i1)
      cnt += int(occ[i1] == 4 and occ[i2] == 4)
  return cnt


# ===================================================================== a. op-level calls
def _raw_assign_add(mt, rag, flat, t):
  _lib.check(mt._lib.mhte_assign_add(mt.handle, _lib.vp(rag.values), _i64p(rag.row_splits),  # pylint: disable=protected-access
                                     rag.row_splits.size, _lib.vp(flat), flat.numel(), int(t), 0, _stream()))


@pytest.mark.parametrize("dim", [64, 132, 256, 17])
def test_op_level_calls_with_misaligned_buffers(dim):
  """``table_lookup_n(out=misaligned)``, ``raw_assign`` / ``mhte_assign_add`` / ``raw_apply_gradients``
  with misaligned values and ``table_optimize_n`` with misaligned gradients (ids unique, and with
  duplicates grouped inside the op), as a random op sequence: after every op 1000 probes and the
  op's own 4099 ids are looked up into a misaligned and into an aligned buffer, at the end the
  key-sorted dump (rows with optimizer state, time stamps) — all bit for bit against the oracle."""
  rng = np.random.default_rng(dim)
  mt, ot, lrs = _table(dim)
  universe = np.unique(rng.integers(-2**62, 2**62, 6000))
  seen = []
  for step in range(10):
    k = step % 5
    ids = rng.choice(universe, N)            # with duplicates
    if k == 3:
      ids = rng.choice(universe, 3001, replace=False)
    v = (rng.standard_normal((ids.size, dim)) * 0.5).astype(np.float32)
    t = 100 + step
    rag = Ragged(ids_t(ids), np.array([0, ids.size], dtype=np.int64))
    vm = _mis(v)
    if k == 0:
      ot.assign(ids, v, t)
      mt.raw_assign(rag, vm.reshape(-1), req_time=t)
    elif k == 1:
      ot.assign_add(ids, v, t)
      _raw_assign_add(mt, rag, vm.reshape(-1), t)
    elif k == 2:
      ot.optimize(ids, v, lrs, t)
      mt.raw_apply_gradients(rag, vm.reshape(-1), req_time=t)
    elif k == 3:
      ot.optimize(ids, v, lrs, t)
      mt.table_optimize_n("emb", rag.values, None, vm, np.asarray(lrs), t, flags=_lib.MHTE_IDS_UNIQUE)
    else:
      ot.optimize(ids, v, lrs, t)
      mt.table_optimize_n("emb", rag.values, None, vm, np.asarray(lrs), t, flags=0)
    seen.append(ids)
    assert mt.size("emb") == ot.size(), step
    for probe in (rng.choice(universe, 1000), ids):
      exp = ot.lookup(probe)[0]
      for mis in (True, False):
        out = _mis_empty(probe.size, dim) if mis else torch.empty((probe.size, dim), device="cuda")
        mt.table_lookup_n("emb", ids_t(probe), None, out)
        np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg="step %d mis %s" % (step, mis))
  _check_table(mt, ot, seen, True)


def test_displacement_pass_with_one_float_per_lane_on_a_float4_table():
  """A float4-capable table (dim 8) at load 0.88 of a pre-sized table: ids that find both buckets full
  go to the displacement pass, which runs as ``slowpath_kernel<1, ..>`` because the values are
  misaligned.  Nothing dropped, rows equal to the oracle's."""
  cap, dim, n = 1 << 12, 8, 3600
  mt, ot, _ = _table(dim, initial_capacity=cap, max_load_factor=0.95)
  rng = np.random.default_rng(3)
  ids = np.unique(rng.integers(1, 2**60, n + 50))[:n]
  rng.shuffle(ids)
  v = rng.standard_normal((n, dim)).astype(np.float32)
  deferred = 0
  for lo in range(0, n, 512):
    part = ids[lo:lo + 512]
    deferred += _must_defer(mt, part, 10)
    mt.raw_assign(Ragged(ids_t(part), np.array([0, part.size], dtype=np.int64)),
                  _mis(v[lo:lo + 512]).reshape(-1), req_time=7)
    ot.assign(part, v[lo:lo + 512], 7)
  st = mt.stats("emb")
  assert st.dropped == 0 and st.hashpower == 10 and st.size == n
  assert deferred > 0   # (the pass had work)
  _check_table(mt, ot, [ids], True)


# ===================================================================== b. mhte_table_sum_optimize_n
@pytest.mark.parametrize("which", ["grads", "grad_unique", "both"])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dim", ALL_DIMS)
def test_sum_optimize_n_with_misaligned_buffers(dim, exact, which):
  """``table_sum_optimize_n`` on the CSR lists of the ordered dedup with misaligned ``grads``,
  misaligned ``grad_unique`` or both: all rows after three steps equal the oracle's replay.  Rows of
  more than 64 floats are right too, not refused: the launch shape for these pointers does not cover
  the row, so the entry point takes its segment-sum + upsert route."""
  mt, ot, lrs = _table(dim)
  ws = D.DedupWorkspace()
  seen = []
  for s_ in range(STEPS):
    ids, g = _batch(10 + s_), S.grad_batch(s_, N, dim)
    u = ws.unique(ids_t(ids), want_host_count=False)
    grads = _buf(g, which in ("grads", "both"))
    grad_u = _mis_empty(N, dim) if which in ("grad_unique", "both") else torch.empty((N, dim), device="cuda")
    mt.table_sum_optimize_n("emb", ws, u, grads, grad_u, np.asarray(lrs), S.update_time(s_),
                            exact_order=exact, n_max=N)
    _replay(ot, ids, g, dim, lrs, S.update_time(s_))
    seen.append(ids)
  _check_table(mt, ot, seen, exact)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dim", ALL_DIMS)
def test_unpipelined_sparse_step_with_misaligned_grads(dim, exact):
  """``SparseStep(fused_backward=True)`` without ``next_ids`` (unordered dedup + one fused launch)
  given a gradient view one float off alignment."""
  mt, ot, lrs = _table(dim)
  step = SparseStep(mt, "emb", N, exact_order=exact)
  seen = []
  for s_ in range(STEPS):
    ids, g = _batch(20 + s_), S.grad_batch(s_, N, dim)
    emb = step.forward(ids_t(ids))
    _same_rows(emb.cpu().numpy(), ot.lookup(ids)[0], exact, "forward %d" % s_)
    step.backward(_mis(g), S.update_time(s_))
    _replay(ot, ids, g, dim, lrs, S.update_time(s_))
    seen.append(ids)
  _check_table(mt, ot, seen, exact)


# ===================================================================== c. the pipelined step
class _Pipe:
  """The two-launch step over the C ABI (``table_step_forward`` / ``table_step_backward``) with the
  caller's own embedding, gradient and summed-gradient buffers; two workspaces alternate."""

  def __init__(self, mt, dim, lrs, exact, n=N):
    self.mt, self.dim, self.lrs, self.exact, self.n = mt, dim, np.asarray(lrs, dtype=np.float32), exact, n
    self.ws = [D.DedupWorkspace(), D.DedupWorkspace()]
    self.uids = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2)]
    self.nu = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    self.grad_u = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    self.cur = 0
    self.has_next = False

  def start(self, ids):
    self.mt.table_finish_pending("emb")
    self.ws[self.cur].step_dedup(ids, self.uids[self.cur], self.nu[self.cur])

  def forward(self, ids, out, next_ids=None):
    nxt = 1 - self.cur
    if next_ids is None:
      self.mt.table_step_forward("emb", ids, out)
    else:
      self.mt.table_step_forward("emb", ids, out, self.ws[nxt], next_ids, self.uids[nxt], self.nu[nxt])
    self.has_next = next_ids is not None
    return out

  def backward(self, grads, t, grad_u=None):
    cur, nxt = self.cur, 1 - self.cur
    self.mt.table_step_backward("emb", self.ws[cur], self.ws[nxt] if self.has_next else None, self.uids[cur],
                                self.nu[cur], grads, self.grad_u if grad_u is None else grad_u, self.lrs, t,
                                exact_order=self.exact)
    self.cur = nxt


@pytest.mark.parametrize("which", ["out", "grads", "grad_unique"])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dim", [4, 64, 17])
def test_pipelined_step_rows_of_at_most_64_floats(dim, exact, which):
  """Rows one VEC = 1 lane group covers: a misaligned ``out``, ``grads`` or ``grad_unique`` runs the
  other instantiation of ``step_fwd_kernel`` / ``step_bwd_kernel`` and gives the oracle's rows; the
  embeddings returned are the oracle's lookup."""
  mt, ot, lrs = _table(dim)
  pipe = _Pipe(mt, dim, lrs, exact)
  batches = [_batch(30 + s_) for s_ in range(STEPS + 1)]
  dev = [ids_t(b) for b in batches]
  pipe.start(dev[0])
  grad_u = _mis_empty(N, dim) if which == "grad_unique" else None
  for s_ in range(STEPS):
    g = S.grad_batch(s_, N, dim)
    out = _mis_empty(N, dim) if which == "out" else torch.empty((N, dim), device="cuda")
    pipe.forward(dev[s_], out, dev[s_ + 1])
    _same_rows(out.cpu().numpy(), ot.lookup(batches[s_])[0], exact, "forward %d" % s_)
    pipe.backward(_buf(g, which == "grads"), S.update_time(s_), grad_u)
    _replay(ot, batches[s_], g, dim, lrs, S.update_time(s_))
  _check_table(mt, ot, batches[:STEPS], exact)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("dim", ALL_DIMS)
def test_pipelined_sparse_step_with_misaligned_grads(dim, exact):
  """``SparseStep.forward(ids, next_ids)`` / ``backward(view one float off alignment)``: no exception
  at any width (rows of more than 64 floats are staged through an aligned buffer of the step's), rows
  equal to the oracle's."""
  mt, ot, lrs = _table(dim)
  step = SparseStep(mt, "emb", N, exact_order=exact)
  batches = [_batch(40 + s_) for s_ in range(STEPS + 1)]
  dev = [ids_t(b) for b in batches]
  for s_ in range(STEPS):
    g = S.grad_batch(s_, N, dim)
    emb = step.forward(dev[s_], next_ids=dev[s_ + 1])
    _same_rows(emb.cpu().numpy(), ot.lookup(batches[s_])[0], exact, "forward %d" % s_)
    step.backward(_mis(g), S.update_time(s_))
    _replay(ot, batches[s_], g, dim, lrs, S.update_time(s_))
    assert step.n_unique() == np.unique(batches[s_]).size
  _check_table(mt, ot, batches[:STEPS], exact)


def test_pipelined_step_changes_lane_width_between_backward_and_forward_at_high_load():
  """Dim 8 at loads 0.56 .. 0.85 of a pre-sized table, so every update leaves ids for the displacement pass that
  rides in the next forward.  A backward with misaligned grads (VEC = 1) followed by a forward with an
  aligned ``out`` (VEC = 4), and the other way round: the forward's lane width differs from the one the
  queued gradients were stored for, and it runs the pass on its own first.  Embeddings and rows equal
  the oracle's bit for bit, nothing dropped."""
  cap, dim, n, steps, total = 1 << 12, 8, 600, 4, 3500
  mt, ot, lrs = _table(dim, initial_capacity=cap, max_load_factor=0.95)
  rng = np.random.default_rng(13)
  fresh = np.unique(rng.integers(1, 2**60, 3700))[:total]
  rng.shuffle(fresh)
  # 2300 rows to begin with: the four updates insert 300 ids each at loads 0.56 .. 0.85 (the table
  # doubles once keys + batch size pass 0.95 of its 4096 slots)
  first, fresh = fresh[:total - 1200], fresh[total - 1200:]
  v0 = rng.standard_normal((first.size, dim)).astype(np.float32)
  mt.raw_assign(Ragged(ids_t(first), np.array([0, first.size], dtype=np.int64)), val_t(v0).reshape(-1), req_time=5)
  ot.assign(first, v0, 5)
  batches = []
  for s_ in range(steps + 1):
    b = fresh[300 * (s_ % 4):300 * (s_ % 4) + 300]
    again = batches[-1][-300:] if batches else first[:300]   # what the previous update just inserted
    batches.append(np.concatenate([again, b]))
  dev = [ids_t(b) for b in batches]
  out_mis = [False, False, True, False, True]
  grad_mis = [True, False, True, False]
  pipe = _Pipe(mt, dim, lrs, True, n=n)
  pipe.start(dev[0])
  deferred = {True: 0, False: 0}
  for s_ in range(steps + 1):
    out = _mis_empty(n, dim) if out_mis[s_] else torch.empty((n, dim), device="cuda")
    pipe.forward(dev[s_], out, dev[s_ + 1] if s_ < steps else None)
    np.testing.assert_array_equal(out.cpu().numpy(), ot.lookup(batches[s_])[0], err_msg="forward %d" % s_)
    if s_ == steps:
      break
    g = S.grad_batch(s_, n, dim)
    # (between forward and backward nothing is queued: the dump disturbs no pass)
    deferred[grad_mis[s_]] += _must_defer(mt, batches[s_], 10)
    pipe.backward(_buf(g, grad_mis[s_]), S.update_time(s_))
    _replay(ot, batches[s_], g, dim, lrs, S.update_time(s_))
  st = mt.stats("emb")
  assert st.dropped == 0 and st.hashpower == 10 and st.size == total
  assert deferred[True] > 0 and deferred[False] > 0   # (both kinds of update queued ids for the pass)
  _check_table(mt, ot, [first] + batches[:steps], True)


@pytest.mark.parametrize("which", ["out", "grads", "grad_unique"])
@pytest.mark.parametrize("dim", WIDE_DIMS)
def test_pipelined_step_refuses_misaligned_buffers_for_rows_of_more_than_64_floats(dim, which):
  """At the C ABI a float4 table of more than 64 floats per row needs 16-byte aligned ``embedding`` /
  ``grads`` / ``grad_unique``: a VEC = 1 lane group would cover columns 0..63 only.  The call is refused
  with InvalidArgument before anything changes: the same step repeated with aligned buffers and two
  more steps end with the rows of an oracle that never saw the refused call."""
  mt, ot, lrs = _table(dim)
  pipe = _Pipe(mt, dim, lrs, True)
  batches = [_batch(50 + s_) for s_ in range(STEPS + 1)]
  dev = [ids_t(b) for b in batches]
  pipe.start(dev[0])
  for s_ in range(STEPS):
    g = S.grad_batch(s_, N, dim)
    out = torch.empty((N, dim), device="cuda")
    size0 = mt.size("emb") if s_ == 1 else None    # (size: an op on the table — asked once, mid-pipeline)
    if s_ == 0 and which == "out":
      with pytest.raises(_lib.InvalidArgumentError, match="16-byte aligned"):
        pipe.forward(dev[s_], _mis_empty(N, dim), dev[s_ + 1])
      assert mt.size("emb") == 0
    pipe.forward(dev[s_], out, dev[s_ + 1])
    np.testing.assert_array_equal(out.cpu().numpy(), ot.lookup(batches[s_])[0], err_msg="forward %d" % s_)
    if s_ <= 1 and which != "out":
      with pytest.raises(_lib.InvalidArgumentError, match="16-byte aligned"):
        if which == "grads":
          pipe.backward(_mis(g), S.update_time(s_) + 1000)
        else:
          pipe.backward(val_t(g), S.update_time(s_) + 1000, _mis_empty(N, dim))
      if s_ == 1:
        assert mt.size("emb") == size0
    pipe.backward(val_t(g), S.update_time(s_))
    _replay(ot, batches[s_], g, dim, lrs, S.update_time(s_))
  _check_table(mt, ot, batches[:STEPS], True)


# ===================================================================== d. workspace ops
@pytest.mark.parametrize("dim", [8, 64, 100, 260])
def test_workspace_segment_sum_and_gather_rows_with_misaligned_buffers(dim):
  """``segment_sum(grads=misaligned)`` in both orders and ``gather_rows`` with a misaligned source or
  destination, against ``O.fill_with_offset_map_gradient`` and numpy indexing.  Dim 260 takes the
  ``e += G * VEC`` loop with VEC = 4 (aligned) and again with VEC = 1."""
  ids, g = _batch(60), S.grad_batch(60, N, dim)
  ws = D.DedupWorkspace()
  r = ws.unique(ids_t(ids))
  U = r.n_unique
  uk, _, vo, vos, _ = O.unique_key_with_value_and_offset(ids, [0, N], [dim])
  assert U == uk.size
  exp = O.fill_with_offset_map_gradient(np.arange(U), [0, U], g.ravel(), vo, vos, [dim]).reshape(U, dim)
  for mis in (True, False):
    got = ws.segment_sum(_buf(g, mis), r, dim, exact_order=True)[:U].cpu().numpy()
    np.testing.assert_array_equal(got, exp, err_msg="mis %s" % mis)
    got = ws.segment_sum(_buf(g, mis), r, dim, exact_order=False)[:U].cpu().numpy()
    np.testing.assert_allclose(got, exp, rtol=RTOL_TREE, atol=ATOL_TREE, err_msg="mis %s" % mis)
  got = ws.segment_sum(val_t(g), r, dim, out=_mis_empty(N, dim), exact_order=True)[:U].cpu().numpy()
  np.testing.assert_array_equal(got, exp)
  src = np.random.default_rng(dim).standard_normal((U, dim)).astype(np.float32)
  inv = r.inverse.cpu().numpy()
  for src_mis, out_mis in ((True, False), (False, True), (True, True), (False, False)):
    out = _mis_empty(N, dim) if out_mis else torch.empty((N, dim), device="cuda")
    ws.gather_rows(_buf(src, src_mis), r.inverse, N, dim, out=out)
    np.testing.assert_array_equal(out.cpu().numpy(), src[inv], err_msg="src %s out %s" % (src_mis, out_mis))


# ===================================================================== e. the public dedup trio
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("dims", [[8, 4, 260], [2, 3, 5]])
def test_dedup_trio_on_a_three_table_ragged_key(dims, mis):
  """``unique_key_with_value_and_offset`` / ``fill_with_offset_map`` / ``.._gradient`` on a ragged key of
  lengths 1500, 0, 2599 with one id repeated 500 times: all four outputs and the buffer length bit for
  bit against the oracle, with ``pos`` every unique key and then a permutation of a strict subset per
  table; dims [8, 4, 260] is the all-float4 path (an empty table in it), [2, 3, 5] the other; ``mis``:
  ``value`` / ``grad`` one float off alignment."""
  rng = np.random.default_rng(sum(dims))
  lens = [1500, 0, 2599]
  split = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  key = rng.integers(1, 900, split[-1]).astype(np.int64)
  key[1500 + 3:1500 + 3 + 5 * 500:5] = 123456789
  r = D.unique_key_with_value_and_offset(Ragged(ids_t(key), split), dims)
  uk, uks, vo, vos, blen = O.unique_key_with_value_and_offset(key, split, dims)
  np.testing.assert_array_equal(r.unique_key.values.cpu().numpy(), uk)
  np.testing.assert_array_equal(r.unique_key.row_splits, uks)
  np.testing.assert_array_equal(r.value_offset.cpu().numpy(), vo)
  np.testing.assert_array_equal(r.value_offset_split.cpu().numpy(), vos)
  assert r.value_buffer.numel() == blen == int(np.dot(lens, dims))
  full = (np.arange(uk.size, dtype=np.int64), uks.copy())
  parts = [uks[t] + rng.permutation(int(uks[t + 1] - uks[t]))[:int(uks[t + 1] - uks[t]) * 2 // 3]
           for t in range(3)]
  subset = (np.concatenate(parts).astype(np.int64),
            np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64))
  grad = rng.standard_normal(blen).astype(np.float32)
  for pos, pos_split in (full, subset):
    assert pos_split[-1] == pos.size and (pos is full[0] or pos.size < uk.size)
    nval = int(sum(int(pos_split[t + 1] - pos_split[t]) * dims[t] for t in range(3)))
    value = rng.standard_normal(nval).astype(np.float32)
    pr = Ragged(ids_t(pos), pos_split)
    buf = D.fill_with_offset_map(pr, _buf(value, mis), r.value_offset, r.value_offset_split,
                                 torch.zeros(blen, dtype=torch.float32, device="cuda"), dims)
    np.testing.assert_array_equal(buf.cpu().numpy(),
                                  O.fill_with_offset_map(pos, pos_split, value, vo, vos, dims, blen))
    bg = D.fill_with_offset_map_gradient(pr, _buf(grad, mis), r.value_offset, r.value_offset_split, dims)
    np.testing.assert_array_equal(bg.cpu().numpy(),
                                  O.fill_with_offset_map_gradient(pos, pos_split, grad, vo, vos, dims))


# ===================================================================== f. post-exchange ops
@pytest.mark.parametrize("sorted_", [True, False])
def test_reduce_ops_with_misaligned_values(sorted_):
  """``reduce_sum`` / ``reduce_mean`` / ``reduce_sqrtn`` (batch 500, dim 24, 0..8 rows per output, one
  empty): the misaligned run gives the bits of the aligned run and of the sequential fp32 loop."""
  rng = np.random.default_rng(9)
  batch, dim = 500, 24
  lens = rng.integers(0, 9, batch)
  lens[7] = 0
  ind = np.repeat(np.arange(batch), lens)
  vals = rng.standard_normal((ind.size, dim)).astype(np.float32)
  if not sorted_:
    perm = rng.permutation(ind.size)
    ind, vals = ind[perm], vals[perm]
  idx = torch.from_numpy(ind[:, None]).cuda()
  for mode, fn in ((0, D.reduce_sum), (1, D.reduce_mean), (2, D.reduce_sqrtn)):
    exp = np.zeros((batch, dim), np.float32)
    cnt = np.zeros(batch, np.int64)
    for i, b in enumerate(ind):
      exp[b] = exp[b] + (vals[i] * vals[i] if mode == 2 else vals[i])
      cnt[b] += 1
    with np.errstate(divide="ignore", invalid="ignore"):
      if mode == 1:
        exp = exp * (np.float32(1.0) / cnt.astype(np.float32))[:, None]
      if mode == 2:
        exp = np.sqrt(exp)
    got_m = fn(idx, _mis(vals), [batch], sorted_).cpu().numpy()
    got_a = fn(idx, _al(vals), [batch], sorted_).cpu().numpy()
    np.testing.assert_array_equal(got_m, exp)      # incl. the NaN row of an empty mean
    np.testing.assert_array_equal(got_m.view(np.uint32), got_a.view(np.uint32))


def test_lookup_gradient_with_misaligned_input_grads():
  rng = np.random.default_rng(2)
  for dim in (16, 64, 260):
    rows, n = 37, N
    idx = np.stack([rng.integers(0, rows, n), rng.integers(0, 9, n)], axis=1).astype(np.int64)
    ids = rng.integers(-2**62, 2**62, n).astype(np.int64)
    g = rng.standard_normal((rows, dim)).astype(np.float32)
    for mis in (True, False):
      out_ids, out = D.lookup_gradient(ids_t(idx), ids_t(ids), _buf(g, mis))
      np.testing.assert_array_equal(out_ids.cpu().numpy(), ids)
      np.testing.assert_array_equal(out.cpu().numpy(), g[idx[:, 0]], err_msg="dim %d mis %s" % (dim, mis))


def test_fused_gather_embeddings_by_input_with_misaligned_buffers():
  """Forward and gradient, dims [8, 16, 4], 3000 / 2000 / 500 rows over 40 / 30 / 5 slots: first the
  fused buffer misaligned, then one of the row tensors; the same bits as the aligned run and as numpy
  indexing / the sequential fp32 loop."""
  rng = np.random.default_rng(21)
  dims, n_rows, slots = [8, 16, 4], [3000, 2000, 500], [40, 30, 5]
  base, offs_h, grads_h = 0, [], []
  for d, n, k in zip(dims, n_rows, slots):
    offs_h.append((base + rng.integers(0, k, n) * d).astype(np.int32))
    grads_h.append(rng.standard_normal((n, d)).astype(np.float32))
    base += k * d
  fused = rng.standard_normal(base).astype(np.float32)
  offs = [torch.from_numpy(o).cuda() for o in offs_h]
  exp_f = [fused[o[:, None] + np.arange(d)[None, :]] for o, d in zip(offs_h, dims)]
  for mis in (True, False):
    outs = D.fused_gather_embeddings_by_input(_buf(fused, mis), offs, dims)
    for o, e in zip(outs, exp_f):
      np.testing.assert_array_equal(o.cpu().numpy(), e, err_msg="mis %s" % mis)
  sc = np.float32(0.37)
  exp = np.zeros(base, np.float32)
  for o, g, d in zip(offs_h, grads_h, dims):
    acc = {}
    for j in range(o.size):
      a = acc.get(int(o[j]))
      t = g[j] * sc
      acc[int(o[j])] = t if a is None else a + t
    for off, v in acc.items():
      exp[off:off + d] = np.float32(0) + v
  for mis_at in (None, 0, 1, 2):
    grads = [_buf(g, k == mis_at) for k, g in enumerate(grads_h)]
    out = D.fused_gather_embeddings_by_input_gradient(base, grads, offs, dims, scale=float(sc)).cpu().numpy()
    np.testing.assert_array_equal(out, exp, err_msg="misaligned input %s" % mis_at)


@pytest.mark.parametrize("unique", [True, False])
def test_fused_apply_gradient_with_misaligned_id_grads(unique):
  """Two tables (dims 8 and 132) x two shards.  ``fused_apply_gradient(id_grads=misaligned)`` takes the
  per-table updates instead of the one launch over the segments: the rows are those of the same call
  with an aligned buffer and of the oracle, bit for bit.  ``fused_lookup`` allocates its flat embedding
  buffer itself, always 16-byte aligned (checked here); no wrapper can hand ``mhte_fused_lookup`` a
  misaligned one, so its per-table fallback is reached through the C ABI only and has no case here."""
  rng = np.random.default_rng(5)
  dims, T, shards = [8, 132], 2, 2
  fss = [700, 300, 451, 649]                      # [shard][table]
  uni = np.unique(rng.integers(1, 2**60, 3000))
  rng.shuffle(uni)
  segs, lo = [], 0
  for n in fss:                                   # distinct inside a segment and across shards
    seg = uni[lo:lo + n].copy()
    if not unique:
      seg[n // 2:] = seg[:n - n // 2]             # duplicates inside the segment, applied in order
    segs.append(seg)
    lo += n
  ids = np.concatenate(segs)
  grads = [rng.standard_normal((n, dims[i % T])).astype(np.float32) * np.float32(0.1)
           for i, n in enumerate(fss)]
  flat = np.concatenate([g.ravel() for g in grads])
  ots = [O.Table([O.segment(d, O.OPT_ADAGRAD, p=(0.1, 0.0))], 1) for d in dims]
  rows = {}
  for mis in (True, False):
    mt = make({"t0": adagrad_cfg(dims[0], LR, 0.1), "t1": adagrad_cfg(dims[1], LR, 0.1)})
    for rep in range(2):
      emb, _, id_off, emb_off, idx = mt.fused_lookup(ids_t(ids), fss, num_of_shards=shards)
      assert emb.data_ptr() % 16 == 0
      if mis:   # the oracle sees every update once
        exp = np.concatenate([ots[i % T].lookup(s)[0].ravel() for i, s in enumerate(segs)])
        np.testing.assert_array_equal(emb.cpu().numpy(), exp)
        for i, s in enumerate(segs):
          ots[i % T].optimize(s, grads[i], [LR], 500 + rep)
      mt.fused_apply_gradient(ids_t(ids), idx, fss, _buf(flat, mis), id_off, emb_off, global_step=0,
                              req_time=500 + rep, num_of_shards=shards, ids_unique_per_segment=unique)
    rows[mis] = [mt.lookup({n: ids_t(np.unique(ids))})[n].cpu().numpy() for n in ("t0", "t1")]
    for n, ot in zip(("t0", "t1"), ots):
      ids_d, _, ts, r = mt.dump(n)
      o_ids, _, o_ts, o_rows = ot.dump()
      a, b = np.argsort(ids_d.cpu().numpy()), np.argsort(o_ids)
      np.testing.assert_array_equal(ids_d.cpu().numpy()[a], o_ids[b])
      np.testing.assert_array_equal(ts.cpu().numpy().astype(np.uint32)[a], o_ts[b])
      np.testing.assert_array_equal(r.cpu().numpy()[a], o_rows[b], err_msg="%s mis %s" % (n, mis))
  for a, b in zip(rows[True], rows[False]):
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ===================================================================== g. fused_embedding_to_layout
from oracle import layout as OL  # noqa: E402
from test_layout_forms_gpu import (CYCLE, FLAG, dev_inputs, one_fid_case, output_grads, planned,  # noqa: E402
                                   raw_forward, raw_grad, same_bits)


def _layout_case(with_bias):
  """Six one-fid features, slice widths 4, 12, 260, 16, 64, 4 from columns 0, 4, 8 of rows 4 floats wider,
  one CONCAT layout; ``with_bias``: an ADDN layout of every row's last float too — an output of ``batch`` =
  33 floats, so the zero fill has a tail behind its float4s when the buffer is aligned and takes its scalar
  branch when it is not (a one-wide slice also sends the whole launch to the general kernels)."""
  widths = CYCLE + [4]
  starts = [4 * (i % 3) for i in range(6)]
  strides = [s + w + 4 for s, w in zip(starts, widths)]
  layouts = {"vec": (OL.CONCAT, [(i, s, s + w) for i, (s, w) in enumerate(zip(starts, widths))], None)}
  if with_bias:
    layouts["bias"] = (OL.ADDN, [(i, strides[i] - 1, strides[i]) for i in range(6)], None)
  return one_fid_case(31, 33, strides, layouts)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("which", ["emb", "out", "tensors_grad", "grad_out", "all"])
def test_layout_entry_points_with_misaligned_buffers(which, with_bias):
  """``mhte_embedding_to_layout`` / ``_grad`` with one embedding matrix, one output, the output gradients, the
  gradient buffers or all of them one float off alignment, with MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS (the
  float4 forms must give way to ``layout_kernel``) and without: the bits of the all-aligned run and of
  the oracle; outputs and gradient buffers hold NaN before the call."""
  c = _layout_case(with_bias)
  slices, shapes, lens = planned(c)
  every = which == "all"
  embs = [_buf(e, every or (which == "emb" and i == 2)) for i, e in enumerate(c["embs"])]
  d, d_al = dev_inputs(c, embs), dev_inputs(c)
  assert all(e.data_ptr() % 16 == 0 for e in d_al["embs"])
  tg = output_grads(shapes, 4)
  want = OL.layout_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"], c["cfgs"])
  gwant = OL.layout_grad_model(c["embs"], c["fid_offset"], c["feature_offset"], c["nfl_offset"], c["batch"], c["cfgs"],
                               tg, acc_dtype=np.float32)
  for flag in (FLAG, 0):
    outs = [_mis_empty(n) if (every or (which == "out" and k == 0)) else torch.empty(n, device="cuda")
            for k, n in enumerate(lens)]
    got = raw_forward(d, slices, lens, flag, outs=outs)
    same_bits(got, want, "forward flag %d" % flag)
    same_bits(got, raw_forward(d_al, slices, lens, flag), "forward flag %d against the aligned run" % flag)
    dtg = [_buf(t, every or which == "tensors_grad") for t in tg]
    grads = [_mis_empty(*e.shape) if (every or which == "grad_out") else torch.empty(e.shape, device="cuda")
             for e in c["embs"]]
    gg = raw_grad(d, slices, dtg, flag, grads=grads)
    same_bits(gg, gwant, "gradient flag %d" % flag)
    same_bits(gg, raw_grad(d_al, slices, [_al(t) for t in tg], flag), "gradient flag %d against the aligned run" % flag)
