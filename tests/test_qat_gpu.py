"""GPU suite of the segment retrievers (quantization-aware training): fixed_r8 ->
fake-quant lookups, one_bit -> HashNet lookups and the gradient scaling in front of the optimizer,
against the NumPy truth of tests/qat_truth.py (itself checked against the reference in
tests/test_qat_truth_cpu.py) and the restated table of oracle/.

Shapes: dims {1, 3, 4, 8, 68, 260} (scalar lanes, float4 lanes, the column loop past one lane group,
past 256 floats) x id counts {1, 63, 65, 257} (one lane group, either side of one wavefront's worth of
8-lane groups, more than one workgroup); every batch of more than one id has duplicates, misses and the
id INT64_MIN, which the engine keeps in a side slot (kEmptyKey)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from monolith_amd import _lib, entry  # noqa: E402
from monolith_amd.multi_hash_table_ops import HashFilter, MultiHashTable  # noqa: E402
from tests import ckpt_proto as P  # noqa: E402
from tests import qat_truth as Q  # noqa: E402

DIMS = [1, 3, 4, 8, 68, 260]
COUNTS = [1, 63, 65, 257]
EMPTY = -2**63
MISS0 = 10**12           # ids from here on are never inserted
# HashNet forward values against the float64 truth: the product scale * w is rounded once (half an ulp
# of the argument, and |x tanh'(x) / tanh(x)| <= 1), the device tanhf is within the 5 ulp OpenCL allows
# it, the product with the amplitude is rounded once: 6 ulp = 3.6e-7 relative; the bound below is 1e-6.
HN_RTOL = 1e-6

_counter = [0]


def _name():
  _counter[0] += 1
  return "qat%d" % _counter[0]


def ids_t(x):
  return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()


def val_t(x):
  return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def bits(x):
  return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def make(cfgs, **kw):
  return MultiHashTable.from_configs(cfgs, name_suffix=_name(), **kw)


def cfg_of(segments, **kw):
  return entry.make_table_config(segments, **kw)


def seg(dim, opt=None, comp=None, init=None):
  return entry.CombineAsSegment(dim, init or entry.ZerosInitializer(), opt or entry.SgdOptimizer(0.1), comp)


def batches(rng, resident, n):
  """id batches of ``n`` ids over the resident ids: duplicates, misses and INT64_MIN (n = 1: one batch each
  of a resident id, a miss and INT64_MIN)"""
  if n == 1:
    return [np.array([resident[1]], np.int64), np.array([MISS0 + 5], np.int64), np.array([EMPTY], np.int64)]
  b = rng.choice(resident, size=n, replace=True)
  b[: n // 8 + 1] = b[-(n // 8 + 1):]                      # duplicates for certain
  b[rng.choice(n, size=max(1, n // 10), replace=False)] = MISS0 + rng.integers(0, 50, size=max(1, n // 10))
  b[n // 2] = EMPTY
  b[0] = EMPTY
  return [b.astype(np.int64)]


def lookup_forms(mt, name, ids):
  """the four lookup entry points -> {form: [n, dim] float32}"""
  dim = mt.get_table_dim_sizes()[0]
  t = ids_t(ids)
  n = ids.size
  out = {}
  out["lookup"] = mt.lookup({name: t})[name].cpu().numpy().reshape(n, dim)
  out["raw_lookup"] = mt.raw_lookup(mt.get_ragged_id({name: t})).cpu().numpy().reshape(n, dim)
  n0 = n // 2
  emb = mt.fused_lookup(t, np.array([n0, n - n0], np.int32), 2)[0]
  out["fused_lookup"] = emb.cpu().numpy().reshape(n, dim)
  buf = torch.full((n, dim), 7.0, dtype=torch.float32, device="cuda")
  out["table_lookup_n"] = mt.table_lookup_n(name, t, None, buf).cpu().numpy()
  return out


def expect_rows(ids, resident_ids, rows, transform):
  """the truth of a lookup: transform(row) of a resident id, zeros of a miss"""
  pos = {int(i): k for k, i in enumerate(resident_ids)}
  out = np.zeros((ids.size, rows.shape[1]), np.float32)
  for k, i in enumerate(ids):
    if int(i) in pos:
      out[k] = transform(rows[pos[int(i)]])
  return out


def stored_weights(mt, name, ids):
  """the raw weights of resident ``ids`` through lookup_entry (which serves INT64_MIN's side slot too;
  dump walks the buckets only)"""
  out = []
  for d in mt.lookup_entry({name: ids_t(ids)})[name]:
    e = P.EntryDump()
    e.ParseFromString(d)
    out.append(np.array(e.num, np.float32))
  return np.stack(out)


def sweep_rows(r, dim):
  """the fake-quant sweep of range r as raw rows of ``dim`` floats (padded with its first values); row 0
  belongs to INT64_MIN"""
  x = Q.fake_quant_sweep(r)
  n = -(-x.size // dim)
  x = np.concatenate([x, x[: n * dim - x.size]]).reshape(n, dim)
  ids = np.arange(n, dtype=np.int64)
  ids[0] = EMPTY
  return ids, x


# =========================================================================== 1. fixed_r8 lookups
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("r", [1.0, 5.0, 0.3])
def test_fixed_r8_lookups_return_the_quantized_weight(r, dim):
  """Every lookup entry point returns FakeQuantizer(r).Quantize of the stored weight, bit for bit, over the
  whole sweep (every rounding boundary and its neighbours, the grid, +-0, NaN, +-1e6, 200 000 draws).
  Fails on a build without the retrievers: lookups are raw there."""
  mt = make({"t": cfg_of([seg(dim, comp=entry.FixedR8Compressor(r))])})
  assert mt.retrievers("t") == [(_lib.MHTE_RETRIEVER_FAKE_QUANT_R8, (float(np.float32(r)),))]
  ids, rows = sweep_rows(r, dim)
  mt.assign({"t": (ids_t(ids), val_t(rows))})
  truth = Q.fake_quant(rows, r)
  got = mt.lookup({"t": ids_t(ids)})["t"].cpu().numpy()
  np.testing.assert_array_equal(bits(got), bits(truth))
  rng = np.random.default_rng(dim)
  for n in COUNTS:
    for b in batches(rng, ids, n):
      exp = expect_rows(b, ids, rows, lambda w: Q.fake_quant(w, r))
      for form, emb in lookup_forms(mt, "t", b).items():
        np.testing.assert_array_equal(bits(emb), bits(exp), err_msg="%s n=%d" % (form, n))
  mt.close()


# =========================================================================== 2. raw readers
@pytest.mark.parametrize("dim", [3, 68])
def test_raw_readers_return_the_assigned_bits(dim, tmp_path):
  from monolith_amd.touched_key_set_ops import TouchedKeySet
  r = 0.3
  cfgs = lambda: {"t": cfg_of([seg(dim, opt=entry.SgdOptimizer(0.1), comp=entry.FixedR8Compressor(r))])}   # noqa: E731
  mt = make(cfgs())
  ids, rows = sweep_rows(r, dim)
  ids, rows = ids[:600], rows[:600]
  mt.assign({"t": (ids_t(ids), val_t(rows))})
  by_id = {int(i): rows[k] for k, i in enumerate(ids)}

  def check_entries(eids, dumps):
    for i, d in zip(eids, dumps):
      e = P.EntryDump()
      e.ParseFromString(d)
      assert e.id == int(i)
      np.testing.assert_array_equal(bits(np.array(e.num, np.float32)), bits(by_id[int(i)]))

  # lookup_entry
  check_entries(ids, mt.lookup_entry({"t": ids_t(ids)})["t"])
  # dump
  d_ids, _, _, d_rows = mt.dump("t")
  for i, row in zip(d_ids.cpu().numpy(), d_rows.cpu().numpy()):
    np.testing.assert_array_equal(bits(row[:dim]), bits(by_id[int(i)]))
  # save_as_tensor
  _, ents = mt.save_as_tensor("t", 0, 1, 10**6, 0)
  assert len(ents) == ids.size
  parsed = []
  for d in ents:
    e = P.EntryDump()
    e.ParseFromString(d)
    parsed.append(e.id)
  check_entries(parsed, ents)
  # touched_entries: an update with a zero gradient touches the ids and leaves the weights as they are
  tks = TouchedKeySet(4096, name_suffix=_name())
  mt.set_touched_key_set(tks)
  sub = ids[5:70]
  mt.apply_gradients({"t": (ids_t(sub), val_t(np.zeros((sub.size, dim), np.float32)))})
  tids, dumps = mt.touched_entries()["t"]
  assert sorted(tids.cpu().tolist()) == sorted(sub.tolist())
  check_entries(tids.cpu().numpy(), dumps)
  mt.set_touched_key_set(None)
  # save -> restore into a fresh table: raw rows, quantized lookups
  base = str(tmp_path / "ckpt")
  mt.save(base)
  mt2 = make(cfgs()).restore(base)
  a, b = mt.dump("t"), mt2.dump("t")
  oa, ob = np.argsort(a[0].cpu().numpy()), np.argsort(b[0].cpu().numpy())
  np.testing.assert_array_equal(bits(a[3].cpu().numpy()[oa]), bits(b[3].cpu().numpy()[ob]))
  np.testing.assert_array_equal(bits(mt2.lookup({"t": ids_t(ids)})["t"].cpu().numpy()), bits(Q.fake_quant(rows, r)))
  mt.close()
  mt2.close()


# =========================================================================== 3. mixed rows
def _mixed_layouts():
  a = [seg(1, opt=entry.FtrlOptimizer(0.1)), seg(16, opt=entry.AdagradOptimizer(0.1, 0.1), comp=entry.FixedR8Compressor(0.3))]
  b = [seg(4, comp=entry.OneBitCompressor(step_size=4, amplitude=0.1)), seg(8, comp=entry.FixedR8Compressor()),
       seg(5)]
  return {"ftrl1_r8x16": (a, [("raw", 1), ("r8", 16, 0.3)]),
          "onebit4_r8x8_raw5": (b, [("hn", 4, 0.1), ("r8", 8, 1.0), ("raw", 5)])}


@pytest.mark.parametrize("layout", sorted(_mixed_layouts()))
def test_mixed_rows_transform_each_segment_alone(layout):
  """Retrievers combine per segment: each segment's columns get their own transform (segment edges fall
  inside a float4 of the 17-float row), the raw columns beside them are bit-identical to the stored row."""
  segs, kinds = _mixed_layouts()[layout]
  mt = make({"t": cfg_of(segs)})
  rng = np.random.default_rng(3)
  ids = np.arange(400, dtype=np.int64)
  ids[0] = EMPTY
  rows = rng.normal(0, 0.5, size=(400, 17)).astype(np.float32)
  rows[:, ::5] *= np.float32(-1)
  rows[7, :] = np.float32(-0.0)
  mt.assign({"t": (ids_t(ids), val_t(rows))})
  for n in COUNTS:
    for b in batches(rng, ids, n):
      exp = expect_rows(b, ids, rows, lambda w: w)
      for form, emb in lookup_forms(mt, "t", b).items():
        c = 0
        for kind in kinds:
          w, e = exp[:, c:c + kind[1]], emb[:, c:c + kind[1]]
          if kind[0] == "raw":
            np.testing.assert_array_equal(bits(e), bits(w), err_msg="%s raw cols %d" % (form, c))
          elif kind[0] == "r8":
            np.testing.assert_array_equal(bits(e), bits(Q.fake_quant(w, kind[2])), err_msg="%s r8 cols %d" % (form, c))
          else:
            truth = Q.HashNet(step_size=4, amplitude=kind[2]).forward(w)
            np.testing.assert_allclose(e, truth, rtol=HN_RTOL, atol=1e-12, err_msg="%s hash net cols %d" % (form, c))
          c += kind[1]
  mt.close()


# =========================================================================== 4. the scale schedule
def test_hash_net_scale_follows_global_step_and_only_real_updates_move_it():
  dim, amp = 4, 0.1
  comp = lambda: entry.OneBitCompressor(step_size=4, amplitude=amp)   # noqa: E731
  mt = make({"t": cfg_of([seg(dim, comp=comp(), init=entry.ConstantsInitializer(0.5))])})
  assert mt.retrievers("t") == [(_lib.MHTE_RETRIEVER_HASH_NET, (4.0, 1.0, 10000.0, float(np.float32(amp))))]
  assert mt.hash_net_scale("t", 0) == 1.0
  truth = Q.HashNet(step_size=4, amplitude=amp)
  rng = np.random.default_rng(0)
  ids = np.arange(1, 40, dtype=np.int64)
  for gs in range(10):
    g = rng.uniform(-1, 1, size=(ids.size, dim)).astype(np.float32)
    mt.apply_gradients({"t": (ids_t(ids), val_t(g))}, global_step=gs)
    if gs % 4 == 0:
      truth.scale = Q.hash_net_scale(gs)
    assert mt.hash_net_scale("t", 0) == pytest.approx(truth.scale, rel=1e-6), gs
    # the next lookup reads the live value
    d_ids, _, _, d_rows = mt.dump("t")
    raw = d_rows.cpu().numpy()[:, :dim]
    got = mt.lookup({"t": d_ids})["t"].cpu().numpy()
    np.testing.assert_allclose(got, truth.forward(raw), rtol=HN_RTOL, atol=1e-12)
  at8 = mt.hash_net_scale("t", 0)
  assert at8 == pytest.approx(Q.hash_net_scale(8), rel=1e-6)
  # n = 0 on a multiple of step_size: no Backward ran
  mt.apply_gradients({"t": (ids_t(np.zeros(0, np.int64)), val_t(np.zeros((0, dim), np.float32)))}, global_step=12)
  assert mt.hash_net_scale("t", 0) == at8
  mt.close()
  # every id dropped by the admission filter (threshold 3: the first three sightings), on multiples of step_size
  flt = HashFilter(capacity=1000)
  cfg = cfg_of([seg(dim, comp=comp(), init=entry.ConstantsInitializer(0.5))],
               slot_occurrence_threshold_config=entry.SlotOccurrenceThresholdConfig(3, {}))
  mt = make({"t": cfg}, hash_filter=flt)
  new = np.arange(1, 21, dtype=np.int64) << 17    # (distinct 12-bit filter signatures: no two ids share a count)
  g = val_t(np.ones((new.size, dim), np.float32))
  for gs in (4, 8, 12):
    mt.apply_gradients({"t": (ids_t(new), g)}, global_step=gs)
    assert mt.size("t") == 0 and mt.hash_net_scale("t", 0) == 1.0, gs
  mt.apply_gradients({"t": (ids_t(new), g)}, global_step=16)
  assert mt.size("t") == new.size
  assert mt.hash_net_scale("t", 0) == pytest.approx(Q.hash_net_scale(16), rel=1e-6)
  mt.close()


# =========================================================================== 5, 6. update parity
OPTS = {"sgd": lambda: entry.SgdOptimizer(0.1), "adagrad": lambda: entry.AdagradOptimizer(0.05, 0.1),
        "adam": lambda: entry.AdamOptimizer(0.01)}
STEPS = [0, 200, 400, 401, 1000, 1001]      # step_size 200: the scale moves at 0, 200, 400, 1000 (<= 2.45)
max_parity_diff = [0.0]


def _parity_calls(dim, seed):
  """six calls mixing new ids, resident ids and duplicates (and INT64_MIN): [(ids, grads, global_step)]"""
  rng = np.random.default_rng(seed)
  calls, pool = [], np.concatenate([[EMPTY], np.arange(1, 150)]).astype(np.int64)
  for k, n in enumerate([1, 63, 65, 257, 63, 65]):
    hi = min(pool.size, 40 + 30 * k)                 # the id range grows: new ids in every call
    b = rng.choice(pool[:hi], size=n, replace=True)
    if n > 1:
      b[0] = EMPTY
      b[-1] = b[1]
    g = rng.uniform(-1, 1, size=(n, dim)).astype(np.float32)
    calls.append((b.astype(np.int64), g, STEPS[k]))
  return calls


def _parity_truth(opt, dim, calls, amp):
  """oracle.Table stepped one occurrence at a time, each gradient scaled first from the oracle's current raw
  row (a new id's: the initializer's 0.5)"""
  ot = O.Table(O.segment(dim, opt.opt_type, p=opt.params(), init=O.INIT_CONSTANT, init_value=0.5), 1)
  hn = Q.HashNet(step_size=200, amplitude=amp)
  for s, (b, g, gs) in enumerate(calls):
    for i, gi in zip(b, g):
      w = ot.lookup([i])[0][0] if ot.contains(i) else np.full(dim, 0.5, np.float32)
      ot.optimize([i], hn.backward(w, gi, gs).astype(np.float32)[None, :], [opt.learning_rate], 100 + s, gs)
  return ot, hn


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("opt_name", sorted(OPTS))
def test_hash_net_update_matches_the_oracle_on_every_route(opt_name, dim):
  """apply_gradients, fused_apply_gradient and table_optimize_n (one optimizer step per occurrence, in
  order) against the truth, absolute tolerance 1e-5 (the project's parity bar for rows not summed in the
  reference's order).  |grad| <= 1, lr <= 0.1, scale <= 2.45, amplitude 0.1: a device tanhf off by k = 4 ulp
  moves the factor by at most amplitude * scale * 2k * 2^-24 ~ 1.2e-7 and a weight by ~1e-8 per application.
  After every call the caller's gradient tensor is what it was."""
  amp = 0.1
  opt = OPTS[opt_name]()
  calls = _parity_calls(dim, 11 * dim + len(opt_name))
  ot, hn = _parity_truth(opt, dim, calls, amp)
  o_ids, _, _, o_rows = ot.dump()
  order = np.argsort(o_ids)
  lrs = np.array([opt.learning_rate], np.float32)
  for route in ("apply_gradients", "fused_apply_gradient", "table_optimize_n"):
    mt = make({"t": cfg_of([seg(dim, opt=OPTS[opt_name](), comp=entry.OneBitCompressor(step_size=200, amplitude=amp),
                                init=entry.ConstantsInitializer(0.5))])})
    for s, (b, g, gs) in enumerate(calls):
      gt = val_t(g)
      keep = gt.clone()
      if route == "apply_gradients":
        mt.apply_gradients({"t": (ids_t(b), gt)}, global_step=gs, req_time=100 + s)
      elif route == "fused_apply_gradient":
        n0 = b.size // 2
        fss = np.array([n0, b.size - n0], np.int32)
        mt.fused_apply_gradient(ids_t(b), None, fss, gt.reshape(-1), np.array([0, n0, b.size], np.int32),
                                np.array([0, n0 * dim, b.size * dim], np.int32), gs, 100 + s, 2)
      else:
        mt.table_optimize_n("t", ids_t(b), None, gt, lrs, 100 + s, global_step=gs, flags=0)
      assert torch.equal(gt, keep), (route, s)
    assert mt.hash_net_scale("t", 0) == pytest.approx(hn.scale, rel=1e-6)
    d_ids, _, _, d_rows = mt.dump("t")       # (the buckets' rows, optimizer state included; INT64_MIN below)
    # (the oracle's row = weights | optimizer state; the engine pads Adam's two powers to four floats)
    d_ids, d_rows = d_ids.cpu().numpy(), d_rows.cpu().numpy()[:, :o_rows.shape[1]]
    do = np.argsort(d_ids)
    assert o_ids[order][0] == EMPTY and mt.size("t") == o_ids.size
    np.testing.assert_array_equal(d_ids[do], o_ids[order][1:])
    w_empty = stored_weights(mt, "t", np.array([EMPTY], np.int64))[0]
    np.testing.assert_allclose(w_empty, o_rows[order][0][:dim], rtol=0, atol=1e-5, err_msg=route + " INT64_MIN")
    o_rows_b = o_rows[order][1:]
    diff = float(np.abs(d_rows[do].astype(np.float64) - o_rows_b.astype(np.float64)).max())
    diff = max(diff, float(np.abs(w_empty.astype(np.float64) - o_rows[order][0][:dim]).max()))
    max_parity_diff[0] = max(max_parity_diff[0], diff)
    print("hash net parity %s dim %d %s: max |row - truth| = %.3e (running max %.3e)" %
          (opt_name, dim, route, diff, max_parity_diff[0]))
    np.testing.assert_allclose(d_rows[do], o_rows_b, rtol=0, atol=1e-5, err_msg=route)
    mt.close()


def test_summed_duplicates_get_one_backward_on_the_sum():
  """MHTE_SUM_DUPLICATES: the occurrences' gradients are added first, Backward runs once on the sum"""
  dim, amp = 8, 0.1
  mt = make({"t": cfg_of([seg(dim, comp=entry.OneBitCompressor(step_size=200, amplitude=amp),
                              init=entry.ConstantsInitializer(0.5))])})
  rng = np.random.default_rng(5)
  b = np.array([3, 4, 3, EMPTY, 3, 4, EMPTY, 9], np.int64)
  g = rng.uniform(-1, 1, size=(b.size, dim)).astype(np.float32)
  gt = val_t(g)
  keep = gt.clone()
  mt.table_optimize_n("t", ids_t(b), None, gt, np.array([0.1], np.float32), 7, global_step=200,
                      flags=_lib.MHTE_SUM_DUPLICATES)
  assert torch.equal(gt, keep)
  hn = Q.HashNet(step_size=200, amplitude=amp)
  u = np.unique(b)
  for i, row in zip(u, stored_weights(mt, "t", u)):
    s = np.zeros(dim, np.float32)
    for k in np.flatnonzero(b == i):
      s = (s + g[k]).astype(np.float32)
    exp = 0.5 - 0.1 * hn.backward(np.full(dim, 0.5, np.float32), s, 200)
    np.testing.assert_allclose(row[:dim], exp, rtol=0, atol=1e-6)
  mt.close()


# =========================================================================== 7. the fused-step boundary
def test_fused_step_boundary():
  from monolith_amd.distributed_ps_sync import ShardedStepGroup
  from monolith_amd.fused_step import MultiSparseStep, SparseStep
  dim, amp, B = 8, 0.1, 257
  mk = lambda: make({"t": cfg_of([seg(dim, comp=entry.OneBitCompressor(step_size=2, amplitude=amp),   # noqa: E731
                                      init=entry.ConstantsInitializer(0.5))])})
  mt, twin = mk(), mk()
  assert mt._lib.mhte_table_fused_backward_ok(mt.handle, 0) == 0   # pylint: disable=protected-access
  plain = make({"t": cfg_of([seg(dim)])})
  assert plain._lib.mhte_table_fused_backward_ok(plain.handle, 0) == 1   # pylint: disable=protected-access
  plain.close()
  # SparseStep takes the unfused route: the retriever's embeddings, the op-level update's rows
  step = SparseStep(mt, "t", B, exact_order=True)
  rng = np.random.default_rng(9)
  for s in range(3):
    b = rng.integers(1, 60, size=B).astype(np.int64)
    b[0] = EMPTY
    g = val_t(rng.uniform(-1, 1, size=(B, dim)).astype(np.float32))
    keep = g.clone()
    emb = step.forward(ids_t(b))
    assert torch.equal(emb, mt.lookup({"t": ids_t(b)})["t"])
    assert torch.equal(emb, twin.lookup({"t": ids_t(b)})["t"])
    step.backward(g, 50 + s, global_step=2 * s)
    assert torch.equal(g, keep)
    twin.table_optimize_n("t", ids_t(b), None, g, np.array([0.1], np.float32), 50 + s, global_step=2 * s,
                          flags=_lib.MHTE_SUM_DUPLICATES)
    assert mt.hash_net_scale("t", 0) == twin.hash_net_scale("t", 0)
  a, c = mt.dump("t"), twin.dump("t")
  oa, oc = torch.argsort(a[0]), torch.argsort(c[0])
  assert torch.equal(a[0][oa], c[0][oc]) and torch.equal(a[3][oa], c[3][oc])
  # the step kernels and the step objects refuse the table, naming the retriever
  out = torch.empty((B, dim), dtype=torch.float32, device="cuda")
  with pytest.raises(_lib.InvalidArgumentError, match="hash_net retriever"):
    mt.table_step_forward("t", ids_t(np.arange(B)), out)
  with pytest.raises(_lib.InvalidArgumentError, match="hash_net retriever"):
    MultiSparseStep(mt, B)
  with pytest.raises(_lib.InvalidArgumentError, match="hash_net retriever"):
    ShardedStepGroup([mt, twin], B)
  r8 = make({"t": cfg_of([seg(dim, comp=entry.FixedR8Compressor())])})
  assert r8._lib.mhte_table_fused_backward_ok(r8.handle, 0) == 0   # pylint: disable=protected-access
  with pytest.raises(_lib.InvalidArgumentError, match="fake_quant_r8 retriever"):
    MultiSparseStep(r8, B)
  # HashNet on a whole-segment optimizer is refused; fake quant on one is fine
  ga = lambda c: make({"t": cfg_of([seg(dim, opt=entry.AdaGradWithGroupLassoOptimizer(0.1), comp=c)])})   # noqa: E731
  with pytest.raises(_lib.InvalidArgumentError, match="group_adagrad"):
    ga(entry.OneBitCompressor())
  ga(entry.FixedR8Compressor()).close()
  for t in (mt, twin, r8):
    t.close()


# =========================================================================== 8. no change elsewhere
def test_no_compressor_fp32_and_fp16_are_the_same_table():
  dim = 12
  tabs = [make({"t": cfg_of([seg(dim, opt=entry.AdagradOptimizer(0.1, 0.1), comp=c)])})
          for c in (None, entry.Fp32Compressor(), entry.Fp16Compressor())]
  rng = np.random.default_rng(2)
  ids = np.concatenate([[EMPTY], rng.integers(1, 200, size=256)]).astype(np.int64)
  vals = rng.normal(size=(ids.size, dim)).astype(np.float32)
  g = rng.uniform(-1, 1, size=(ids.size, dim)).astype(np.float32)
  res = []
  for mt in tabs:
    assert mt.retrievers("t") == [(_lib.MHTE_RETRIEVER_RAW, ())]
    assert mt._lib.mhte_table_fused_backward_ok(mt.handle, 0) == 1   # pylint: disable=protected-access
    mt.assign({"t": (ids_t(ids[:100]), val_t(vals[:100]))})
    mt.apply_gradients({"t": (ids_t(ids), val_t(g))}, global_step=4, req_time=9)
    mt.assign_add({"t": (ids_t(ids[50:90]), val_t(vals[50:90]))})
    probe = ids_t(np.concatenate([ids, [MISS0]]))
    d = mt.dump("t")
    o = torch.argsort(d[0])
    res.append((mt.lookup({"t": probe})["t"], d[0][o], d[3][o]))
  for r in res[1:]:
    for x, y in zip(res[0], r):
      assert torch.equal(x, y)
  for mt in tabs:
    mt.close()


# =========================================================================== 9. the serialized config
def _varint(n):
  out = bytearray()
  while n >= 0x80:
    out.append((n & 0x7f) | 0x80)
    n >>= 7
  out.append(n)
  return bytes(out)


def _ld(field, payload):
  return _varint((field << 3) | 2) + _varint(len(payload)) + payload


def _serialized(dim, comp_arm, comp_body, constant=None):
  """MultiEmbeddingHashTableConfig{t: one SGD(0.1) segment of ``dim`` with comp_config{<arm>: body}}"""
  m = P.MultiEmbeddingHashTableConfig()
  m.names.append("t")
  c = m.configs.add()
  c.cuckoo.SetInParent()
  s = c.entry_config.segments.add()
  s.dim_size = dim
  if constant is None:
    s.init_config.zeros.dim_size = dim
  else:
    s.init_config.constants.constant = constant
  s.opt_config.sgd.learning_rate = 0.1
  s.MergeFromString(_ld(3, _ld(comp_arm, comp_body)))
  return m.SerializeToString()


def test_serialized_config_builds_the_retrievers():
  """from_serialized_config reads Segment.comp_config: the table behaves as the Python-configured one
  (it came up raw, silently, before)."""
  f32 = lambda field, v: _varint((field << 3) | 5) + np.float32(v).tobytes()   # noqa: E731
  dim, r = 8, 0.3
  a = MultiHashTable.from_serialized_config(_serialized(dim, 3, f32(2, r)), name_suffix=_name())
  b = make({"t": cfg_of([seg(dim, comp=entry.FixedR8Compressor(r))])})
  assert a.retrievers("t") == b.retrievers("t") == [(_lib.MHTE_RETRIEVER_FAKE_QUANT_R8, (float(np.float32(r)),))]
  ids, rows = sweep_rows(r, dim)
  ids, rows = ids[:2000], rows[:2000]
  for mt in (a, b):
    mt.assign({"t": (ids_t(ids), val_t(rows))})
  got = a.lookup({"t": ids_t(ids)})["t"]
  assert torch.equal(got.view(torch.int32), b.lookup({"t": ids_t(ids)})["t"].view(torch.int32))
  np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(Q.fake_quant(rows, r)))
  a.close()
  b.close()
  # one_bit: defaults (step_size 200, init_scale 1, max_scale 10000, amplitude 0.1), then explicit fields
  d = MultiHashTable.from_serialized_config(_serialized(dim, 4, b""), name_suffix=_name())
  assert d.retrievers("t") == [(_lib.MHTE_RETRIEVER_HASH_NET, (200.0, 1.0, 10000.0, float(np.float32(0.1))))]
  d.close()
  body = _varint((2 << 3) | 0) + _varint(4) + f32(5, 0.05)
  a = MultiHashTable.from_serialized_config(_serialized(dim, 4, body, constant=0.5), name_suffix=_name())
  b = make({"t": cfg_of([seg(dim, comp=entry.OneBitCompressor(step_size=4, amplitude=0.05),
                             init=entry.ConstantsInitializer(0.5))])})
  assert a.retrievers("t") == b.retrievers("t")
  rng = np.random.default_rng(4)
  for gs in (0, 3, 4, 8):
    bt = rng.integers(1, 50, size=65).astype(np.int64)
    g = rng.uniform(-1, 1, size=(65, dim)).astype(np.float32)
    for mt in (a, b):
      mt.apply_gradients({"t": (ids_t(bt), val_t(g))}, global_step=gs)
    assert a.hash_net_scale("t", 0) == b.hash_net_scale("t", 0)
    probe = ids_t(np.arange(0, 60))
    assert torch.equal(a.lookup({"t": probe})["t"], b.lookup({"t": probe})["t"])
  assert a.hash_net_scale("t", 0) == pytest.approx(Q.hash_net_scale(8), rel=1e-6)
  a.close()
  b.close()


# =========================================================================== 10. updates of multi-segment rows
def _mixed_update_layouts():
  """name -> [(dim, optimizer factory, compressor factory or None)]; every segment starts at 0.5"""
  sgd = lambda: entry.SgdOptimizer(0.1)   # noqa: E731
  one = lambda step, amp: (lambda: entry.OneBitCompressor(step_size=step, amplitude=amp))   # noqa: E731
  return {
      "onebit4_r8x8_raw5": [(4, sgd, one(200, 0.1)), (8, sgd, lambda: entry.FixedR8Compressor()), (5, sgd, None)],
      "ftrl1_onebit16": [(1, lambda: entry.FtrlOptimizer(0.1), None),
                         (16, lambda: entry.AdagradOptimizer(0.05, 0.1), one(200, 0.1))],
      "onebit4_onebit4": [(4, sgd, one(200, 0.1)), (4, lambda: entry.AdagradOptimizer(0.05, 0.1), one(400, 0.05))],
      "onebit8_groupadagrad8": [(8, sgd, one(200, 0.1)), (8, lambda: entry.AdaGradWithGroupLassoOptimizer(0.1), None)],
  }


def _mixed_truth(layout, calls):
  """the oracle stepped one occurrence at a time; the columns of every one_bit segment scaled first by that
  segment's own quantizer at the oracle's raw row, every other column's gradient as it is"""
  opts = [o() for _, o, _ in layout]
  comps = [c() if c else None for _, _, c in layout]
  dims = [d for d, _, _ in layout]
  dim = sum(dims)
  ot = O.Table([O.segment(d, o.opt_type, p=o.params(), init=O.INIT_CONSTANT, init_value=0.5)
                for d, o in zip(dims, opts)], 1)
  hns = [Q.HashNet(step_size=c.step_size, amplitude=c.amplitude) if isinstance(c, entry.OneBitCompressor) else None
         for c in comps]
  lrs = [o.learning_rate for o in opts]
  for s, (b, g, gs) in enumerate(calls):
    for i, gi in zip(b, g):
      w = ot.lookup([i])[0][0] if ot.contains(i) else np.full(dim, 0.5, np.float32)
      gg, c0 = gi.astype(np.float32).copy(), 0
      for d, hn in zip(dims, hns):
        if hn is not None:
          gg[c0:c0 + d] = hn.backward(w[c0:c0 + d], gi[c0:c0 + d], gs).astype(np.float32)
        c0 += d
      ot.optimize([i], gg[None, :], lrs, 100 + s, gs)
  return ot, hns


def _unique_calls(dim, seed):
  """calls whose ids are pairwise distinct (new and resident ids, INT64_MIN): what the one-launch fused
  optimize takes"""
  rng = np.random.default_rng(seed)
  pool = np.concatenate([[EMPTY], np.arange(1, 400)]).astype(np.int64)
  calls = []
  for k, n in enumerate([1, 63, 65, 257, 63, 65]):
    b = rng.choice(pool[: 100 + 60 * k], size=n, replace=False)
    if n > 1:
      b[0] = EMPTY if EMPTY not in b[1:] else b[0]
    calls.append((b.astype(np.int64), rng.uniform(-1, 1, size=(n, dim)).astype(np.float32), STEPS[k]))
  return calls


@pytest.mark.parametrize("name", sorted(_mixed_update_layouts()))
def test_multi_segment_rows_update_like_the_oracle(name):
  """The per-column instance of the update (kRtMixed): one_bit columns take the scaled gradient, the raw and
  fixed_r8 columns beside them the gradient as it is, each one_bit segment moves its own scale at its own
  step_size, and a GroupAdaGrad segment beside a one_bit one takes the whole-segment instance.  Sequential
  duplicates through apply_gradients and table_optimize_n, distinct ids through the one-launch fused optimize
  (the segment kernels) and table_optimize_n; stored weights against the oracle to 1e-5 as above."""
  layout = _mixed_update_layouts()[name]
  dim = sum(d for d, _, _ in layout)
  mk = lambda: make({"t": cfg_of([seg(d, opt=o(), comp=c() if c else None, init=entry.ConstantsInitializer(0.5))   # noqa: E731
                                  for d, o, c in layout])})
  lrs = np.array([o().learning_rate for _, o, _ in layout], np.float32)
  seed = 7 * dim + len(name)
  for calls, routes in ((_parity_calls(dim, seed), ("apply_gradients", "table_optimize_n")),
                        (_unique_calls(dim, seed), ("fused_unique", "table_optimize_n_unique"))):
    ot, hns = _mixed_truth(layout, calls)
    o_ids, _, _, o_rows = ot.dump()
    for route in routes:
      mt = mk()
      for s, (b, g, gs) in enumerate(calls):
        gt = val_t(g)
        keep = gt.clone()
        if route == "apply_gradients":
          mt.apply_gradients({"t": (ids_t(b), gt)}, global_step=gs, req_time=100 + s)
        elif route == "fused_unique":
          n0 = b.size // 2
          mt.fused_apply_gradient(ids_t(b), None, np.array([n0, b.size - n0], np.int32), gt.reshape(-1),
                                  np.array([0, n0, b.size], np.int32), np.array([0, n0 * dim, b.size * dim], np.int32),
                                  gs, 100 + s, 2, ids_unique_per_segment=True)
        else:
          mt.table_optimize_n("t", ids_t(b), None, gt, lrs, 100 + s, global_step=gs,
                              flags=_lib.MHTE_IDS_UNIQUE if route.endswith("unique") else 0)
        assert torch.equal(gt, keep), (route, s)
      for k, hn in enumerate(hns):
        if hn is not None:
          assert mt.hash_net_scale("t", k) == pytest.approx(hn.scale, rel=1e-6), (route, k)
      assert mt.size("t") == o_ids.size
      got = stored_weights(mt, "t", o_ids)
      diff = float(np.abs(got.astype(np.float64) - o_rows[:, :dim]).max())
      max_parity_diff[0] = max(max_parity_diff[0], diff)
      print("hash net parity %s %s: max |weight - truth| = %.3e (running max %.3e)" %
            (name, route, diff, max_parity_diff[0]))
      np.testing.assert_allclose(got, o_rows[:, :dim], rtol=0, atol=1e-5, err_msg=route)
      mt.close()
  if name == "onebit4_onebit4":   # the two scales differ after step 1000: 200 divides it, 400 does not
    assert hns[0].scale == pytest.approx(Q.hash_net_scale(1000)) and hns[1].scale == pytest.approx(Q.hash_net_scale(400))


# =========================================================================== 11. the two-ids-per-group lookup
@pytest.mark.parametrize("kind", ["one_bit8", "onebit4_r8x8_raw4"])
def test_large_lookups_of_retriever_tables(kind):
  """4096 ids and more of a float4 table take the two-ids-per-lane-group launch (lookup_role_u); fixed_r8's is
  covered by the whole-sweep lookup of test 1 at dims 4 and 8"""
  if kind == "one_bit8":
    segs, kinds = [seg(8, comp=entry.OneBitCompressor(step_size=4, amplitude=0.1))], [("hn", 8)]
  else:
    segs = [seg(4, comp=entry.OneBitCompressor(step_size=4, amplitude=0.1)), seg(8, comp=entry.FixedR8Compressor()), seg(4)]
    kinds = [("hn", 4), ("r8", 8), ("raw", 4)]
  dim = sum(k[1] for k in kinds)
  mt = make({"t": cfg_of(segs)})
  rng = np.random.default_rng(12)
  ids = np.arange(5001, dtype=np.int64)
  ids[0] = EMPTY
  rows = rng.normal(0, 0.5, size=(ids.size, dim)).astype(np.float32)
  mt.assign({"t": (ids_t(ids), val_t(rows))})
  probe = np.concatenate([ids, MISS0 + np.arange(40), ids[:300]]).astype(np.int64)
  exp = expect_rows(probe, ids, rows, lambda w: w)
  for form in ("lookup", "table_lookup_n"):
    if form == "lookup":
      emb = mt.lookup({"t": ids_t(probe)})["t"].cpu().numpy()
    else:
      emb = mt.table_lookup_n("t", ids_t(probe), None, torch.empty((probe.size, dim), dtype=torch.float32,
                                                                   device="cuda")).cpu().numpy()
    c = 0
    for k in kinds:
      w, e = exp[:, c:c + k[1]], emb[:, c:c + k[1]]
      if k[0] == "raw":
        np.testing.assert_array_equal(bits(e), bits(w))
      elif k[0] == "r8":
        np.testing.assert_array_equal(bits(e), bits(Q.fake_quant(w, 1.0)))
      else:
        np.testing.assert_allclose(e, Q.HashNet(step_size=4, amplitude=0.1).forward(w), rtol=HN_RTOL, atol=1e-12)
      c += k[1]
  mt.close()


# =========================================================================== 12. Adam's powers on wide raw rows
@pytest.mark.parametrize("dim", [65, 260])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_raw_adam_rows_wider_than_one_pass_of_the_lane_group(amsgrad, dim):
  """A raw table (no retriever): a lane group walks a row of more than G x VEC floats in several rounds (65
  floats with one float per lane, 260 with float4 lanes), and every column of a RESIDENT id must see the same
  beta powers — the first chunk's lane used to write them back before the later rounds read them.  Against the
  oracle, sequential duplicates included; weights stay below 0.1, so 1e-6 is hundreds of ulps of slack for the
  device's sqrt and division and a thousand times below what the stale powers cost (2e-3)."""
  opt = lambda: entry.AdamOptimizer(0.01, amsgrad=amsgrad)   # noqa: E731
  mt = make({"t": cfg_of([seg(dim, opt=opt())])})
  o = opt()
  ot = O.Table(O.segment(dim, o.opt_type, p=o.params()), 1)
  rng = np.random.default_rng(dim)
  for s in range(5):
    b = rng.integers(1, 40, size=65).astype(np.int64)
    b[0] = EMPTY
    g = rng.uniform(-1, 1, size=(65, dim)).astype(np.float32)
    mt.apply_gradients({"t": (ids_t(b), val_t(g))}, global_step=s, req_time=10 + s)
    for i, gi in zip(b, g):
      ot.optimize([i], gi[None, :], [o.learning_rate], 10 + s, s)
  o_ids, _, _, o_rows = ot.dump()
  got = stored_weights(mt, "t", o_ids)
  np.testing.assert_allclose(got, o_rows[:, :dim], rtol=0, atol=1e-6)
  mt.close()


# =========================================================================== 13. the config's fields, read back
def test_serialized_comp_config_fields_reach_the_retriever():
  f32 = lambda field, v: _varint((field << 3) | 5) + np.float32(v).tobytes()   # noqa: E731
  a = MultiHashTable.from_serialized_config(_serialized(4, 3, b""), name_suffix=_name())
  assert a.retrievers("t") == [(_lib.MHTE_RETRIEVER_FAKE_QUANT_R8, (1.0,))]          # r's default
  a.close()
  body = _varint((2 << 3) | 0) + _varint(6) + f32(3, 2.0) + f32(4, 9.0) + f32(5, 0.25)
  a = MultiHashTable.from_serialized_config(_serialized(4, 4, body, constant=0.5), name_suffix=_name())
  assert a.retrievers("t") == [(_lib.MHTE_RETRIEVER_HASH_NET, (6.0, 2.0, 9.0, 0.25))]   # step_size, init, max, amplitude
  assert a.hash_net_scale("t", 0) == 2.0
  g = val_t(np.ones((3, 4), np.float32))
  a.apply_gradients({"t": (ids_t([1, 2, 3]), g)}, global_step=6)
  assert a.hash_net_scale("t", 0) == pytest.approx(2.0 * np.sqrt(1.03), rel=1e-6)
  a.apply_gradients({"t": (ids_t([1, 2, 3]), g)}, global_step=6 * 10**6)               # the cap
  assert a.hash_net_scale("t", 0) == 9.0
  a.close()
  for bad in (2.5, 0.0, 2.0**25):      # the setter: a whole step_size in 1..2^24
    with pytest.raises(_lib.InvalidArgumentError, match="step_size"):
      t = make({"t": cfg_of([seg(4)])})
      try:
        arr = (_lib.C.c_float * 4)(bad, 1.0, 10.0, 0.1)
        _lib.check(t._lib.mhte_table_set_retriever(t.handle, 0, 0, _lib.MHTE_RETRIEVER_HASH_NET, arr, 4))   # pylint: disable=protected-access
      finally:
        t.close()


# =========================================================================== 14. HashNet rows behind the displacement pass
DISP_CAP, DISP_HP, DISP_N, DISP_SEED = 1 << 10, 8, 920, 3


def _ids_with_full_home_buckets(ids, cap, hp):
  """positions of the ids that find both home buckets full when they arrive one by one: the oracle's table of
  the same capacity, its bucket occupancy read before every insert (a condition on the inputs)"""
  L = O.lib()
  ot = O.Table(O.segment(1, O.OPT_SGD), cap)
  full = []
  for k, i in enumerate(ids):
    _, pos, _, _ = ot.dump(with_rows=False)
    occ = np.bincount(pos >> 2, minlength=1 << hp)
    hv = L.mo_hash(int(i))
    i1 = hv & ((1 << hp) - 1)
    i2 = L.mo_alt_index(hp, L.mo_partial(hv), i1)
    if occ[i1] == 4 and occ[i2] == 4:
      full.append(k)
    ot.assign([i], np.zeros((1, 1), np.float32))
  assert ot.hashpower() == hp and ot.size() == len(ids)
  return full


def test_hash_net_rows_placed_by_the_displacement_pass():
  """920 distinct new ids into a table pre-sized to 1024 slots (max_load_factor 0.95, the recipe of
  test_slow_path_displacement_at_high_load), 128 per call: ids whose two buckets are full go through the
  displacement pass of the retriever tables (slowpath_backward_kernel; seg_slow_backward_kernel on the
  one-launch fused optimize), which applies the same first update as the fast path: every id is new and seen
  once, so its row is 0.5 - lr * Backward(0.5, g, global_step).  Tolerance and its reasoning: as in
  test_hash_net_update_matches_the_oracle_on_every_route (|grad| <= 1, lr 0.1, scale <= 2.45).  The routes are
  that test's three and the fused optimize with ids_unique_per_segment, the only one that reaches the segment
  kernels."""
  from tests.test_parity_gpu import _check_placement_valid
  dim, amp, lr = 8, 0.1, 0.1
  rng = np.random.default_rng(DISP_SEED)
  ids = rng.integers(1, 2**60, DISP_N)
  assert np.unique(ids).size == DISP_N
  g = rng.uniform(-1, 1, size=(DISP_N, dim)).astype(np.float32)
  full = _ids_with_full_home_buckets(ids, DISP_CAP, DISP_HP)
  print("ids with both home buckets full at their insertion: %d of %d" % (len(full), DISP_N))
  assert len(full) >= 8          # (every route runs all the ids, so each has them all)
  calls = [(lo, min(lo + 128, DISP_N), STEPS[min(k, len(STEPS) - 1)]) for k, lo in enumerate(range(0, DISP_N, 128))]
  hn = Q.HashNet(step_size=200, amplitude=amp)
  exp = np.empty((DISP_N, dim), np.float64)
  for lo, hi, gs in calls:
    exp[lo:hi] = 0.5 - lr * hn.backward(np.full((hi - lo, dim), 0.5, np.float32), g[lo:hi], gs)
  lrs = np.array([lr], np.float32)
  for route in ("apply_gradients", "fused_apply_gradient", "fused_unique", "table_optimize_n"):
    mt = make({"t": entry.make_table_config(
        [seg(dim, opt=entry.SgdOptimizer(lr), comp=entry.OneBitCompressor(step_size=200, amplitude=amp),
             init=entry.ConstantsInitializer(0.5))],
        entry.CuckooHashTableConfig(initial_capacity=DISP_CAP, max_load_factor=0.95))})
    for s, (lo, hi, gs) in enumerate(calls):
      b, gt = ids_t(ids[lo:hi]), val_t(g[lo:hi])
      n, n0 = hi - lo, (hi - lo) // 2
      if route == "apply_gradients":
        mt.apply_gradients({"t": (b, gt)}, global_step=gs, req_time=100 + s)
      elif route.startswith("fused"):
        mt.fused_apply_gradient(b, None, np.array([n0, n - n0], np.int32), gt.reshape(-1),
                                np.array([0, n0, n], np.int32), np.array([0, n0 * dim, n * dim], np.int32),
                                gs, 100 + s, 2, ids_unique_per_segment=route == "fused_unique")
      else:
        mt.table_optimize_n("t", b, None, gt, lrs, 100 + s, global_step=gs, flags=0)
    st = mt.stats("t")
    assert st.dropped == 0 and st.hashpower == DISP_HP, route
    assert mt.size("t") == DISP_N, route
    assert mt.hash_net_scale("t", 0) == pytest.approx(hn.scale, rel=1e-6)
    got = stored_weights(mt, "t", ids)[:, :dim]
    diff = np.abs(got.astype(np.float64) - exp)
    print("displacement %s: max |row - truth| = %.3e, over the ids with full home buckets %.3e" %
          (route, diff.max(), diff[full].max()))
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-5, err_msg=route)
    _check_placement_valid(mt, "t", DISP_HP)
    mt.close()


# =========================================================================== 15. partial admission
def test_hash_net_table_admits_part_of_an_ids_occurrences():
  """Occurrence threshold 3 on a HashNet table, one optimizer step per occurrence (flags = 0): of a new id's five
  occurrences in one call the filter drops the first three and the update applies the last two; an id seen
  twice stays out, and the next call drops its third sighting and applies its fourth.  Which occurrences pass:
  oracle.SlidingFilter asked once per occurrence of an id the table does not hold (the checker of
  tests/test_boundary_gpu.py); those, in order, as Backward + SGD from 0.5 are the truth, to 1e-5 as above.
  Then the same occurrences as five segments of distinct ids through fused_apply_gradient (one consultation
  with count 1 per segment and id)."""
  dim, amp, lr, thr = 8, 0.1, 0.1, 3
  new = np.arange(1, 5, dtype=np.int64) << 17    # (distinct 12-bit filter signatures: no two ids share a count)
  segs = [list(new[:3]) + ([new[3]] if s in (1, 3) else []) for s in range(5)]
  b = np.array([i for sg in segs for i in sg], np.int64)       # a, b, c five times; d twice
  rng = np.random.default_rng(15)
  calls = [(b, rng.uniform(-1, 1, size=(b.size, dim)).astype(np.float32), gs) for gs in (200, 400)]
  model = O.SlidingFilter(1000, 7, defer_advance=True)         # (HashFilter's default split_num)
  hn = Q.HashNet(step_size=200, amplitude=amp)
  rows, applied, after = {}, [], []
  for ids, g, gs in calls:
    n_app = 0
    for i, gi in zip(ids, g):
      i = int(i)
      if i not in rows:
        if model.should_be_filtered(i, 1, thr):
          continue
        rows[i] = np.full(dim, 0.5, np.float64)
      w32 = rows[i].astype(np.float32)
      rows[i] = (w32 - np.float32(lr) * hn.backward(w32, gi, gs).astype(np.float32)).astype(np.float64)
      n_app += 1
    model.advance_if_full()
    applied.append(n_app)
    after.append(({k: v.copy() for k, v in rows.items()}, [model.get(int(i)) for i in new], float(hn.scale)))
  # the case is the one meant: 3 x 2 of 17 occurrences in the first call (d absent), 3 x 5 + 1 in the second
  assert applied == [6, 16] and sorted(after[0][0]) == [int(i) for i in new[:3]]
  lrs = np.array([lr], np.float32)
  offs = np.concatenate([[0], np.cumsum([len(sg) for sg in segs])]).astype(np.int32)
  for route in ("table_optimize_n", "fused_apply_gradient"):
    flt = HashFilter(capacity=1000)
    cfg = cfg_of([seg(dim, opt=entry.SgdOptimizer(lr), comp=entry.OneBitCompressor(step_size=200, amplitude=amp),
                      init=entry.ConstantsInitializer(0.5))],
                 slot_occurrence_threshold_config=entry.SlotOccurrenceThresholdConfig(thr, {}))
    mt = make({"t": cfg}, hash_filter=flt)
    for s, (ids, g, gs) in enumerate(calls):
      gt = val_t(g)
      keep = gt.clone()
      if route == "table_optimize_n":
        mt.table_optimize_n("t", ids_t(ids), None, gt, lrs, 100 + s, global_step=gs, flags=0)
      else:
        mt.fused_apply_gradient(ids_t(ids), None, np.diff(offs).astype(np.int32), gt.reshape(-1), offs,
                                (offs * dim).astype(np.int32), gs, 100 + s, 5, ids_unique_per_segment=True)
      assert torch.equal(gt, keep), (route, s)
      exp_rows, exp_counts, exp_scale = after[s]
      present = mt.contains("t", ids_t(new)).cpu().tolist()
      assert present == [int(i) in exp_rows for i in new], (route, s)
      assert mt.size("t") == len(exp_rows), (route, s)
      np.testing.assert_array_equal(flt.get(ids_t(new)).cpu().numpy(), exp_counts, err_msg="%s call %d" % (route, s))
      assert mt.hash_net_scale("t", 0) == pytest.approx(exp_scale, rel=1e-6), (route, s)
      held = np.array(sorted(exp_rows), np.int64)
      got = stored_weights(mt, "t", held)[:, :dim]
      want = np.stack([exp_rows[int(i)] for i in held])
      print("partial admission %s call %d: max |row - truth| = %.3e" %
            (route, s, float(np.abs(got.astype(np.float64) - want).max())))
      np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, err_msg="%s call %d" % (route, s))
    mt.close()
