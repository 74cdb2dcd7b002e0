"""GPU suite of the dense optimizers (monolith_amd/optimizers.py, csrc/mhte_dense_opt_kernels.h).  Every
comparison with the numpy truth (tests/dense_opt_truth.py) is on the raw bits, NaNs canonicalised: NaN where the
truth is NaN (x86 and the device give 0 / 0 different signs), the same bits everywhere else — each element is a
fixed tree of individually rounded float32 operations, so there is no tolerance.  Only the reference's goldens
carry the reference's own eps."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_ops_truth as CT  # noqa: E402
import dense_opt_truth as DT  # noqa: E402
import flat_concat_truth as T  # noqa: E402
from monolith_amd import _lib  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd import feature_utils as FU  # noqa: E402
from monolith_amd import optimizers as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, F32 = np.float16, np.float32
FILL = 0x7fc12345   # a NaN pattern planted into the slots' padding
STEPS = 3
SOURCES = ("list", "flat32", "flat16")


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unaligned(a):
  """The same values in a view that starts one float into its storage: a pointer that is not 16-byte aligned."""
  buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
  v = buf[1:1 + a.size]
  v.copy_(torch.from_numpy(a.ravel()))
  assert v.data_ptr() % 16 == 4
  return v.view(a.shape)


def word(x):
  return torch.tensor(float(x), dtype=torch.float32, device=DEV)


def make_opt(kind, align=16, hyper=None, **over):
  h = dict(DT.HYPER[kind] if hyper is None else hyper)
  h.update(over)
  cls = O.AdamomOptimizer if kind.startswith("adamom") else O.RmspropOptimizer
  return cls(use_v2=kind.endswith("_v2"), align=align, **h)


def wire_of(source):
  return F16 if source == "flat16" else F32


def as_seen(grads, source):
  """The gradients as the kernel reads them: an fp16 wire has rounded them."""
  with np.errstate(over="ignore"):
    return [None if g is None else g.astype(wire_of(source)) for g in grads]


def apply(opt, tvars, grads, source, scale=1.0, align=16, update_slots=True):
  """One apply of host gradients through ``source``."""
  if source == "list":
    opt.apply_gradients([(None if g is None else dev(g), v) for g, v in zip(grads, tvars)], grad_scale=scale,
                        update_slots=update_slots)
  else:
    flat = dev(T.concat(grads, 1.0, wire_of(source), align))
    opt.apply_flat(flat, variables=tvars, post_scale=scale, update_slots=update_slots)


def check_state(opt, tvars, model, what=""):
  for i, (tv, hv) in enumerate(zip(tvars, model.vars)):
    DT.assert_same_bits(tv.cpu().numpy(), hv, "%s var %d" % (what, i))
    for s in DT.SLOTS[model.kind]:
      got = opt.get_slot(tv, s)
      assert got.shape == tv.shape
      DT.assert_same_bits(got.cpu().numpy(), model.slots[s][i], "%s slot %s of var %d" % (what, s, i))


@functools.lru_cache(maxsize=None)
def edge_vars():
  return tuple(T.set_edges(seed=21))


@functools.lru_cache(maxsize=None)
def edge_grads():
  return DT.seeded_grads(T.EDGE_SHAPES, STEPS, seed=22)


@functools.lru_cache(maxsize=None)
def edge_truth(kind, fp16, scale):
  """The truth after 1 .. STEPS steps on the edge set (shared by the sources that see the same gradients);
  asserts on the way that no intermediate is subnormal."""
  model = DT.Model(kind, edge_vars(), watch=DT.Tracker())
  after = []
  for grads in edge_grads():
    model.step(as_seen(grads, "flat16" if fp16 else "list"), grad_scale=scale)
    after.append(([v.copy() for v in model.vars], {s: [x.copy() for x in model.slots[s]] for s in model.slots}))
  return after


class Snapshot:
  def __init__(self, kind, state):
    self.kind, (self.vars, self.slots) = kind, state


# ---- the reference's goldens on the device ----------------------------------------------------------------
@pytest.mark.parametrize("golden", DT.GOLDENS, ids=[g[0] for g in DT.GOLDENS])
def test_goldens_of_the_reference(golden):
  kind, hyper, var0, g0, want = golden
  opt = make_opt(kind, hyper=hyper)
  var = dev(np.array([var0], F32))
  opt.apply_gradients([(dev(np.array([g0], F32)), var)])
  got = {"var": var.cpu().numpy()[0]}
  got.update({s: opt.get_slot(var, s).cpu().numpy()[0] for s in opt.get_slot_names()})
  assert sorted(got) == sorted(want)
  for k, w in want.items():
    assert abs(float(got[k]) - w) <= DT.GOLDEN_EPS, (kind, k, got[k], w)


# ---- the full matrix --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["one", "host", "device"])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind", DT.KINDS)
def test_three_steps_equal_the_truth(kind, source, scale):
  value = 1.0 if scale == "one" else 0.37
  truth = edge_truth(kind, source == "flat16", value)
  opt = make_opt(kind)
  tvars = [dev(v) for v in edge_vars()]
  for step, grads in enumerate(edge_grads()):
    apply(opt, tvars, grads, source, scale=word(value) if scale == "device" else value)
    check_state(opt, tvars, Snapshot(kind, truth[step]), "%s %s step %d" % (kind, source, step))
  last = truth[-1]
  assert all(np.isfinite(v).all() for v in last[0]) and any(np.any(m != 0) for m in last[1]["m"])


@pytest.mark.parametrize("align", [4, 1024])
@pytest.mark.parametrize("source", ["flat32", "flat16"])
@pytest.mark.parametrize("kind", ["adamom", "rmsprop_v2"])
def test_flat_source_at_other_alignments(kind, source, align):
  truth = edge_truth(kind, source == "flat16", 0.37)
  opt = make_opt(kind, align=align)
  tvars = [dev(v) for v in edge_vars()]
  for step, grads in enumerate(edge_grads()):
    apply(opt, tvars, grads, source, scale=0.37, align=align)
  check_state(opt, tvars, Snapshot(kind, truth[-1]), "%s %s align %d" % (kind, source, align))
  sd = opt.state_dict()
  assert sd["m"].numel() == T.offsets([v.size for v in edge_vars()], align)[-1] and sd["align"] == align


@pytest.mark.parametrize("wire", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind", DT.KINDS)
def test_apply_flat_equals_split_then_apply_gradients(kind, wire):
  a, b = make_opt(kind), make_opt(kind)
  va, vb = [dev(v) for v in edge_vars()], [dev(v) for v in edge_vars()]
  for grads in edge_grads():
    flat = D.aligned_flat_concat([dev(g) for g in grads], scale=1.7, wire_dtype=wire)
    a.apply_flat(flat, variables=va, post_scale=0.5)
    b.apply_gradients(list(zip(D.aligned_flat_split(vb, flat.clone(), post_scale=0.5), vb)))
  for x, y in zip(va, vb):
    assert torch.equal(x.view(torch.int32), y.view(torch.int32))
  for s in a.get_slot_names():   # the whole buffers, padding included (it is +0 in both)
    assert torch.equal(a.state_dict()[s].view(torch.int32), b.state_dict()[s].view(torch.int32))
    assert a.state_dict()[s].abs().sum().item() > 0


@pytest.mark.parametrize("kind", DT.KINDS)
def test_pointers_four_bytes_into_their_storage(kind):
  """A var and a list gradient that are not 16-byte aligned take the 4-byte accesses: the same bits."""
  truth = edge_truth(kind, False, 0.37)
  opt = make_opt(kind)
  tvars = [unaligned(v) if v.size else dev(v) for v in edge_vars()]
  for grads in edge_grads():
    opt.apply_gradients([(unaligned(g) if g.size else dev(g), v) for g, v in zip(grads, tvars)], grad_scale=0.37)
  check_state(opt, tvars, Snapshot(kind, truth[-1]), kind + " unaligned")


# ---- the table on both sides of the upload ----------------------------------------------------------------
@pytest.mark.parametrize("source", ["list", "flat16"])
@pytest.mark.parametrize("kind", ["adamom_v2", "rmsprop"])
@pytest.mark.parametrize("count", [_lib.DENSE_OPT_INLINE, _lib.DENSE_OPT_INLINE + 1, 155])
def test_many_variables(count, kind, source):
  hs = T.set_seeded(count, seed=count)
  assert len(hs) == count
  steps = DT.seeded_grads([h.shape for h in hs], 2, seed=count + 1)
  model = DT.Model(kind, hs, watch=DT.Tracker())
  opt = make_opt(kind)
  tvars = [dev(h) for h in hs]
  for grads in steps:
    apply(opt, tvars, grads, source, scale=0.37)
    model.step(as_seen(grads, source), grad_scale=0.37)
  check_state(opt, tvars, model, "%d variables" % count)


# ---- more chunks than workgroups --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_vars():
  """2052 chunks in front of 130 small variables: the launch has 2048 workgroups, so the first of them take a
  second chunk — in the same variable, in the next one and in the one after."""
  rng = np.random.default_rng(31)
  return tuple([rng.standard_normal(n).astype(F32) for n in (2048 * 4096 + 5, 7, 4097)] + T.set_seeded(130, seed=130))


@pytest.mark.parametrize("table", ["inline", "uploaded"])
@pytest.mark.parametrize("kind,source", [("adamom", "list"), ("rmsprop_v2", "flat16")])
def test_workgroups_take_a_second_chunk(kind, source, table):
  hs = long_vars()[:3] if table == "inline" else long_vars()
  missing = 1 if source == "list" else None   # a gradient missing in the middle: the variable behind keeps its offset
  taking_part = len(hs) - (missing is not None)
  assert (taking_part > _lib.DENSE_OPT_INLINE) == (table == "uploaded")
  off = T.offsets([v.size for v in hs])
  pad = np.ones(off[-1], bool)
  for v, o in zip(hs, off):
    pad[o:o + v.size] = False
  opt = make_opt(kind)
  planted = torch.full((off[-1],), FILL, dtype=torch.int32, device=DEV).view(torch.float32)
  planted[dev(~pad)] = 0.0
  state = {s: planted.clone() for s in opt.get_slot_names()}
  state.update(numels=[v.size for v in hs], align=16)
  opt.load_state_dict(state)
  model = DT.Model(kind, hs)
  tvars = [dev(v) for v in hs]
  for grads in DT.seeded_grads([v.shape for v in hs], 2, seed=32):
    grads = [None if i == missing else g for i, g in enumerate(grads)]
    apply(opt, tvars, grads, source, scale=0.37)
    model.step(as_seen(grads, source), grad_scale=0.37)
  assert all(np.isfinite(v).all() for v in model.vars)
  assert all(np.isfinite(x).all() for s in model.slots for x in model.slots[s])
  check_state(opt, tvars, model, "%s %s, %s table" % (kind, source, table))
  if missing is not None:
    DT.assert_same_bits(tvars[missing].cpu().numpy(), hs[missing], "the variable without a gradient")
  for s in opt.get_slot_names():
    bits = opt.state_dict()[s].view(torch.int32).cpu().numpy()
    assert (bits[pad] == FILL).all(), s


# ---- None gradients, update_slots -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DT.KINDS)
def test_none_gradients_leave_variable_and_slots_alone(kind):
  opt = make_opt(kind)
  model = DT.Model(kind, edge_vars())
  tvars = [dev(v) for v in edge_vars()]
  steps = edge_grads()
  apply(opt, tvars, steps[0], "list", scale=0.37)
  model.step(steps[0], grad_scale=0.37)
  skipped = (1, 4, 7, 9, 12)   # lengths 1, 16, 4096, 8193 and (64, 65)
  before = {s: opt.state_dict()[s].clone() for s in opt.get_slot_names()}
  vars_before = [v.clone() for v in tvars]
  for grads in steps[1:]:
    grads = [None if i in skipped else g for i, g in enumerate(grads)]
    apply(opt, tvars, grads, "list", scale=0.37)
    model.step(grads, grad_scale=0.37)
  check_state(opt, tvars, model, kind + " with None gradients")
  off = T.offsets([v.size for v in edge_vars()])
  for i in skipped:
    assert torch.equal(tvars[i].view(torch.int32), vars_before[i].view(torch.int32))
    for s in opt.get_slot_names():   # the variable's whole span, padding included
      now = opt.state_dict()[s][off[i]:off[i + 1]]
      assert torch.equal(now.view(torch.int32), before[s][off[i]:off[i + 1]].view(torch.int32))
      assert now.abs().sum().item() > 0
  assert not torch.equal(tvars[2], vars_before[2])


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind", DT.KINDS)
def test_update_slots_false(kind, source):
  steps = edge_grads()
  opt = make_opt(kind)
  model = DT.Model(kind, edge_vars())
  tvars = [dev(v) for v in edge_vars()]
  apply(opt, tvars, steps[0], source, scale=0.37)
  model.step(as_seen(steps[0], source), grad_scale=0.37)
  slots_before = {s: opt.state_dict()[s].clone() for s in opt.get_slot_names()}
  vars_before = [v.clone() for v in tvars]
  apply(opt, tvars, steps[1], source, scale=0.37, update_slots=False)
  model.step(as_seen(steps[1], source), grad_scale=0.37, update_slots=False)
  check_state(opt, tvars, model, kind + " update_slots=False")
  for s in opt.get_slot_names():
    assert torch.equal(opt.state_dict()[s].view(torch.int32), slots_before[s].view(torch.int32))
  moved = not torch.equal(tvars[-2], vars_before[-2])
  assert moved == kind.startswith("adamom")   # Adamom still moves var; RMSprop changes nothing at all


@pytest.mark.parametrize("kind", ["adamom", "adamom_v2"])
def test_adamom_update_slots_false_on_fresh_slots_is_nan(kind):
  """0 / 0 with fresh slots: NaN, as IEEE has it and the reference's kernel computes it."""
  opt = make_opt(kind)
  model = DT.Model(kind, edge_vars())
  tvars = [dev(v) for v in edge_vars()]
  apply(opt, tvars, edge_grads()[0], "list", update_slots=False)
  model.step(edge_grads()[0], update_slots=False)
  assert all(np.isnan(v).all() for v in model.vars)
  check_state(opt, tvars, model, kind)


# ---- the padding of the slots ------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [16, 1024])
@pytest.mark.parametrize("kind", DT.KINDS)
def test_slot_padding_is_never_written(kind, align):
  hs = edge_vars()
  off = T.offsets([v.size for v in hs], align)
  pad = np.ones(off[-1], bool)
  for v, o in zip(hs, off):
    pad[o:o + v.size] = False
  assert pad.any()
  opt = make_opt(kind, align=align)
  planted = torch.full((off[-1],), FILL, dtype=torch.int32, device=DEV).view(torch.float32)
  state = {s: planted.clone() for s in opt.get_slot_names()}
  for s in state:
    state[s][dev(~pad)] = 0.0
  state.update(numels=[v.size for v in hs], align=align)
  opt.load_state_dict(state)   # (before the first apply: adopted when the variables are known)
  model = DT.Model(kind, hs)
  tvars = [dev(v) for v in hs]
  for grads, source in zip(edge_grads(), SOURCES):
    apply(opt, tvars, grads, source, scale=0.37, align=align)
    model.step(as_seen(grads, source), grad_scale=0.37)
  check_state(opt, tvars, model, kind + " planted padding")
  for s in opt.get_slot_names():
    bits = opt.state_dict()[s].view(torch.int32).cpu().numpy()
    assert (bits[pad] == FILL).all(), s
  # ... and a state loaded after the first apply replaces the buffers' contents
  again = make_opt(kind, align=align)
  others = [dev(v) for v in model.vars]
  apply(again, others, edge_grads()[0], "list", align=align)
  again.load_state_dict(opt.state_dict())
  for s in opt.get_slot_names():
    assert torch.equal(again.state_dict()[s].view(torch.int32), opt.state_dict()[s].view(torch.int32))
    assert again.state_dict()[s].data_ptr() != opt.state_dict()[s].data_ptr()


# ---- special values ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("kind", DT.KINDS)
def test_special_values(kind, source):
  special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0], F32)
  rng = np.random.default_rng(31)
  n = 4099
  var = rng.standard_normal(n).astype(F32)
  g = (rng.standard_normal(n) * 0.3).astype(F32)
  k = special.size
  var[:k * k] = np.repeat(special, k)      # every pair (variable, gradient) of the special values
  g[:k * k] = np.tile(special, k)
  var[-3:] = special[[2, 4, 1]]            # ... and some in the ragged last group
  g[-2:] = special[[5, 3]]
  hs = [var, special.copy()]
  grads = [g, special[::-1].copy()]
  opt = make_opt(kind)
  model = DT.Model(kind, hs)
  tvars = [dev(v) for v in hs]
  for _ in range(2):
    apply(opt, tvars, grads, source, scale=0.37)
    model.step(as_seen(grads, source), grad_scale=0.37)
  assert np.isnan(model.vars[0]).any() and not np.isfinite(model.slots["v"][0][:k * k]).all()
  assert np.isfinite(model.vars[0][k * k:-3]).all()
  check_state(opt, tvars, model, "%s %s special values" % (kind, source))


# ---- the device words -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DT.KINDS)
def test_device_learning_rate_and_scale_equal_their_host_forms(kind):
  lr = DT.HYPER[kind]["learning_rate"]
  truth = edge_truth(kind, False, 0.37)
  calls = []

  def schedule():
    calls.append(1)
    return lr

  forms = {"host": (make_opt(kind), 0.37), "device lr": (make_opt(kind, learning_rate=word(lr)), 0.37),
           "both device": (make_opt(kind, learning_rate=word(lr)), word(0.37)),
           "callable": (make_opt(kind, learning_rate=schedule), 0.37),
           "callable -> device": (make_opt(kind, learning_rate=lambda: word(lr)), word(0.37))}
  for name, (opt, scale) in forms.items():
    tvars = [dev(v) for v in edge_vars()]
    for grads in edge_grads():
      apply(opt, tvars, grads, "list", scale=scale)
    check_state(opt, tvars, Snapshot(kind, truth[-1]), "%s %s" % (kind, name))
  assert len(calls) == STEPS   # evaluated per apply


def test_apply_flat_replays_in_a_graph():
  """apply_flat with a device scale and a device learning rate, captured once and replayed after both words and
  the flat buffer were overwritten in place: every replay is the truth's step with the contents of then."""
  kind = "adamom"
  shapes = [(5000,), (4097,), (3,), (33, 7), (16,)]
  assert len(shapes) <= _lib.DENSE_OPT_INLINE
  rng = np.random.default_rng(43)
  hs = [rng.standard_normal(s).astype(F32) for s in shapes]
  contents = [([(rng.standard_normal(s) * 0.3).astype(F32) for s in shapes], sc, lr)
              for sc, lr in ((0.37, 0.013), (0.61, 0.029), (1.0, 0.0071))]
  model = DT.Model(kind, hs, watch=DT.Tracker())
  s = torch.cuda.Stream()
  torch.cuda.synchronize()
  with torch.cuda.stream(s):
    tvars = [dev(v) for v in hs]
    scale_w, lr_w = word(contents[0][1]), word(contents[0][2])
    flat = dev(T.concat(contents[0][0], 1.0, F16))
    opt = make_opt(kind, learning_rate=lr_w)
    opt.apply_flat(flat, variables=tvars, post_scale=scale_w)   # (the warm-up call: the slots exist afterwards)
    model.step(as_seen(contents[0][0], "flat16"), grad_scale=contents[0][1], learning_rate=contents[0][2])
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
      opt.apply_flat(flat, post_scale=scale_w)
    check_state(opt, tvars, model, "after the capture (nothing ran)")
    for grads, sc, lr in contents[1:]:
      flat.copy_(torch.from_numpy(T.concat(grads, 1.0, F16)))
      scale_w.fill_(sc)
      lr_w.fill_(lr)
      g.replay()
      s.synchronize()
      model.step(as_seen(grads, "flat16"), grad_scale=sc, learning_rate=lr)
      check_state(opt, tvars, model, "replay with scale %r" % sc)
  torch.cuda.synchronize()


# ---- clip, allreduce and apply ----------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32 wire", "fp16 wire"])
@pytest.mark.parametrize("kind", ["adamom", "rmsprop"])
def test_clip_allreduce_and_apply(kind, fp16):
  hs = list(edge_vars())
  grads = edge_grads()[0]
  sparse = [np.random.default_rng(51).standard_normal((37, 8)).astype(F32)]
  norm = np.sqrt(CT.tree_sumsq(list(grads) + sparse)[0], dtype=np.float32)
  clip_norm = float(norm) * 0.37
  _, _, scale_t = CT.norm_and_scale(list(grads) + sparse, clip_norm)
  assert scale_t != np.float32(1)
  wire = F16 if fp16 else F32

  def doubled(flat):   # the sum over two ranks that hold the same gradients
    flat.mul_(2)

  # with the allreduce: concat (scale, wire) -> the collective -> apply_flat(post_scale = 1 / world)
  opt = make_opt(kind)
  tvars = [dev(v) for v in hs]
  sparse_scale = FU.clip_allreduce_and_apply(opt, [(dev(g), v) for g, v in zip(grads, tvars)], [dev(x) for x in sparse],
                                             clip_norm=clip_norm, use_allreduce=True, fp16=fp16, allreduce=doubled,
                                             world=2)
  assert CT.bits(sparse_scale.cpu().numpy()) == CT.bits(scale_t)
  model = DT.Model(kind, hs, watch=DT.Tracker())
  with np.errstate(over="ignore"):
    reduced = T.concat(grads, scale_t, wire) * wire(2)
  model.step(T.split(hs, reduced), grad_scale=0.5)
  check_state(opt, tvars, model, kind + " with allreduce")
  # without: the scale goes into the optimizer, None gradients are skipped
  opt = make_opt(kind)
  tvars = [dev(v) for v in hs]
  some = [None if i in (2, 8) else g for i, g in enumerate(grads)]
  kept = [g for g in some if g is not None]
  _, _, scale_n = CT.norm_and_scale(kept + sparse, clip_norm)
  FU.clip_allreduce_and_apply(opt, [(None if g is None else dev(g), v) for g, v in zip(some, tvars)],
                              [dev(x) for x in sparse], clip_norm=clip_norm)
  model = DT.Model(kind, hs, watch=DT.Tracker())
  model.step(some, grad_scale=scale_n)
  check_state(opt, tvars, model, kind + " without allreduce")
  with pytest.raises(ValueError, match="every variable needs a gradient"):
    FU.clip_allreduce_and_apply(opt, [(None if g is None else dev(g), v) for g, v in zip(some, tvars)], [],
                                clip_norm=clip_norm, use_allreduce=True, world=2)


# ---- the argument contract that needs variables on the GPU -------------------------------------------------
@pytest.mark.parametrize("cls", [O.AdamomOptimizer, O.RmspropOptimizer])
def test_python_argument_contract_with_variables(cls):
  opt = cls(learning_rate=0.01)
  a, b = torch.ones(5, device=DEV), torch.ones(3, 7, device=DEV)
  ga, gb = torch.ones(5, device=DEV), torch.ones(3, 7, device=DEV)
  opt.apply_gradients([(ga, a), (gb, b)])
  with pytest.raises(ValueError, match="fixed by the first apply"):
    opt.apply_gradients([(gb, b), (ga, a)])                          # another order
  with pytest.raises(ValueError, match="fixed by the first apply"):
    opt.apply_gradients([(ga, a.clone()), (gb, b)])                  # another identity
  with pytest.raises(ValueError, match="fixed by the first apply"):
    opt.apply_flat(torch.zeros(48, device=DEV), variables=[a])
  with pytest.raises(TypeError, match="gradients must be float32 tensors on the GPU"):
    opt.apply_gradients([(ga.double(), a), (gb, b)])
  with pytest.raises(TypeError, match="gradients must be float32 tensors on the GPU"):
    opt.apply_gradients([(ga.cpu(), a), (gb, b)])
  with pytest.raises(ValueError, match="a gradient of 3 elements for a variable of 5"):
    opt.apply_gradients([(ga[:3], a), (gb, b)])
  with pytest.raises(ValueError, match="flat has 47 elements, the variables need 48"):
    opt.apply_flat(torch.zeros(47, device=DEV))
  with pytest.raises(TypeError, match="flat must be"):
    opt.apply_flat(torch.zeros(48, device=DEV, dtype=torch.bfloat16))
  with pytest.raises(TypeError, match="flat must be"):
    opt.apply_flat(torch.zeros(48))
  with pytest.raises(TypeError, match="gradient scale must be a float or a 0-d float32 tensor on the GPU"):
    opt.apply_gradients([(ga, a), (gb, b)], grad_scale=torch.ones(()))
  assert opt.get_slot(b, "m").shape == b.shape
  assert opt.get_slot(b, "v").data_ptr() == opt.state_dict()["v"].data_ptr() + 4 * 16
  assert opt.state_dict()["numels"] == [5, 21] and opt.state_dict()["align"] == 16
