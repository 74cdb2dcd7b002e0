"""Every owner instance and wire form of the id-sharded multi-table step at small shapes (-m gpu).

``csrc/mhte_shard_kernels.h`` / ``mhte_shard_host.h``: the rest of the suite drives the sharded step through SGD /
Adagrad / FTRL / GroupAdaGrad tables of dims 16 / 32 / 64 / 17 / 33 with peer blocks far larger than what they hold.
This module drives the forms it leaves out.  Every case is one ``Case`` of the table ``CASES``; ``plan_of`` derives
from its optimizers, dims, world and wire settings — with the predicates of the host code — which kernel instances
and copy paths it reaches, ``test_the_plan_reaches_every_case`` (section G) checks the union against the list of
everything there is, and every run checks the owner's apply instances it launched against its plan
(``mhte_shard_step_apply_launches``: host-side counters).

  A. The generic apply instance ``shard_apply_kernel<W, false, MULTI, false>`` (``shard_apply_loop``: one
     ``apply_row`` per sender in rank order, ``is_new`` only for the first): one-segment Momentum, Adadelta, RMSProp
     v1 / v2, Adam, AMSGrad and MovingAverage tables and a basic + non-basic row (FTRL(4) + Adam(28); FTRL(1) +
     Adam(16)), dims 8, 64 (float4 lanes) and 17 (one float per lane), worlds 1, 2, 3, three steps of ~110 ids per
     rank and table.  The stream (``_a_batches``) holds, asserted: ids sent by one rank, by two, by every rank, ids
     new to their owner that every rank sends in the same step, ids that recur from the previous step.
  B. Its displacement pass (``shard_slow_all_role<false>``, ``apply_row_wave`` once per sender) on Adam and Momentum
     tables with the recipe of test_group_displacement_at_high_load (8192 slots, load 0.97, B = 1600, five steps),
     worlds 1 and 2.  With one rank the pass of such tables is a launch of its own as well: it rides in the next
     lookup only when every table is SGD / Adagrad / FTRL (``ShardStep::can_fold``) — the folded form with one
     float per lane is reached by the all-Adagrad world-1 run of section C.
  C. Lane shapes, for fast (Adagrad), generic (Adam) and GroupAdaGrad tables: float4 dims 4, 8, 36, 100, 132, 256
     (G = 8, 8, 16 ragged, 32, 64 ragged, 64 full), one-float dims 1, 3, 5, 33, 63 in front of a dim-64 table whose
     slice of the flat buffers they push off its 16-byte boundary (B = 509: 105 * 509 floats in front of it),
     GroupAdaGrad rows of two group segments behind an Adagrad one (136 floats) and bias + group; world 2 with
     uniform ids, world 3 with Zipf ids and exact order (``shard_exact_sum_kernel`` at those widths), and world 1
     against ``MultiSparseStep`` with ``torch.equal``.  A group segment longer than one trip of G * VEC floats
     cannot reach the sharded step (rows of more than 256 floats, or of more than 64 that are not whole float4s,
     are refused at creation: asserted).
  D. The fp16 gradient wire: fixed-size copies and the exact-size form (pack / unpack) x worlds 2 and 3 x two
     models (dims 132, 36, 4, 3 — Adagrad, Adam, GroupAdaGrad — and dims 16, 17, 33, 1 — GroupAdaGrad, Adam, bias +
     group, SGD) with B = 500: cap / 4 and the dims' sum are odd, so an odd peer's block starts 8 mod 16, and some
     (peer, table) segment holds an odd number of 16-bit words (asserted: the byte tail of ``pack_copy``, the
     partial quad of ``shard_cvt_kernel``); exact order under Zipf; 40 tables; one rank over the peer-store
     transport to itself (``shard_push_kernel``'s 16-bit branch) and over RCCL to itself with the exact form.
  E. Segment fill: ids_per_peer_table 16 and 12 (cap / 4 even and odd), last table of dim 17 and 1, fp32 and fp16,
     fixed and exact form, world 3: deterministic batches (``fill_batches``) in which (sender, peer, table)
     segments hold exactly cap, cap - 1, 1 and 0 ids (asserted), the full one in the last table; and one rank over
     the peer-store transport with fp16.
  F. tests/test_shard_ipc_gpu.py: processes with the fp16 wire on the bias rows, and three processes on the
     fill model of E (``MHTE_TEST_SPECS=fill``).
  G. ``test_the_plan_reaches_every_case``.

Every comparison is bit for bit against the CPU oracle (test_shard_step_gpu._group_against_oracle: forward rows of
every rank and step, every owner's rows, the owners' sizes) or, world 1, against the multi-table step: ids occur at
most 32 times in a batch or exact order is on; with the fp16 wire the oracle's per-sender sums are rounded through
``np.float16``.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from monolith_amd import _lib, entry, synthetic as S  # noqa: E402
from monolith_amd.distributed_ps_sync import ShardedMultiStep, ShardedStepGroup, shard_block_geometry  # noqa: E402
from monolith_amd.fused_step import MultiSparseStep  # noqa: E402
from test_multi_step_gpu import Spec, make, oracle_backward, ragged_of, val_t  # noqa: E402
from test_optimizer_shapes_gpu import _opt  # noqa: E402
from test_shard_step_gpu import (_displaced_not_doubled, _group_against_oracle, batch_of, grads_of,  # noqa: E402
                                 many_table_specs)

BASIC = ("sgd", "adagrad", "ftrl")     # Table::basic_opts
LIGHT_MAX = 32                         # kStepLightMax: longer lists are summed as a tree without exact order


# =============================================================================== tables
def _optdef(name):
  """(oracle optimizer, its parameters, learning rate, entry-config factory)"""
  if name == "sgd":
    return O.OPT_SGD, (), 0.01, lambda: entry.SgdOptimizer(0.01)
  if name == "group":
    return (O.OPT_GROUP_ADAGRAD, (0.1, 1.0, 0.001, 0.0), 0.02,
            lambda: entry.AdaGradWithGroupLassoOptimizer(0.02, beta=1.0, initial_accumulator_value=0.1,
                                                         l2_regularization=0.001))
  return _opt(name)


class FSpec(Spec):
  """``Spec`` with every optimizer of test_optimizer_shapes_gpu's table: segs [(dim, optimizer name)], rows
  initialised to 0.25 (a row that was initialised twice, or not at all, shows)."""

  def __init__(self, name, segs, slot, **kw):
    super().__init__(name, [(d, o, _optdef(o)[2]) for d, o in segs], slot, **kw)

  def entry_cfg(self):
    parts = [entry.CombineAsSegment(d, entry.ConstantsInitializer(0.25), _optdef(o)[3]()) for d, o, _ in self.segs]
    return entry.make_table_config(parts, entry.CuckooHashTableConfig(**self.kw), learning_rates=self.lrs())

  def oracle_table(self):
    segs = [O.segment(d, _optdef(o)[0], p=_optdef(o)[1], init=O.INIT_CONSTANT, init_value=0.25)
            for d, o, _ in self.segs]
    return O.Table(segs, int(self.kw.get("initial_capacity", 1)))


def _tables(*rows, **kw):
  """rows: (name, [(dim, optimizer)]) in any order; slots by position"""
  return [FSpec(n, segs, i + 1, **kw) for i, (n, segs) in enumerate(rows)]


# =============================================================================== the cases and their plans
class Case:
  """One run.  transport: group (N ranks in one process) | identity | ipc | rccl (one rank to itself);
  stream: seeded (test_shard_step_gpu's batches) | a (_a_batches) | fill (fill_batches)."""

  def __init__(self, cid, section, specs, world, B, steps=3, dist="uniform", cap=0, fp16=False, exact_form=False,
               exact_order=False, transport="group", stream="seeded", universe=None, displace=False):
    self.id, self.section, self.specs, self.world, self.B, self.steps = cid, section, specs, world, B, steps
    self.dist, self.cap, self.fp16, self.exact_form, self.exact_order = dist, cap, fp16, exact_form, exact_order
    self.transport, self.stream, self.universe, self.displace = transport, stream, universe, displace


def _vec_ok(sp):        # Table::vec_ok for the optimizers here: every segment is whole float4s
  return all(d % 4 == 0 for d, _, _ in sp.segs)


def _kind(sp):          # ShardStep::owner_args: A.fast / kShapeGroupBit
  opts = [o for _, o, _ in sp.segs]
  return "group" if "group" in opts else "fast" if all(o in BASIC for o in opts) else "generic"


def plan_of(c):
  """The instances and copy paths the case reaches, as the host code selects them."""
  specs = sorted(c.specs(), key=lambda s: s.name)
  world, multi = c.world, c.world > 1
  geo = shard_block_geometry([s.dim for s in specs], c.B, world, c.cap)
  fold = world == 1 and all(_kind(s) == "fast" for s in specs)          # ShardStep::can_fold
  wire = c.transport != "identity"
  half = c.fp16 and wire
  out, off = set(), 0
  if fold:
    out.add(("lookup", 4, True))                                        # (the float4 instance runs the owed pass)
  for t, sp in enumerate(specs):
    vw = 4 if _vec_ok(sp) else 1                                        # seg_shape_code(tb): block rows are aligned
    out.add(("lookup", vw, fold))
    out.add(("apply", vw, _kind(sp), multi))
    out.add(("apply segments", _kind(sp), "one" if len(sp.segs) == 1 else "several"))
    svw = 4 if vw == 4 and off % 4 == 0 else 1                          # shape_code(tb, io_off): gather_tabs
    off += c.B * sp.dim
    out.add(("scatter", svw))
    out.add(("build", svw))
    if c.exact_order:
      out.add(("exact sum", svw))
    if c.displace:
      out.add(("displacement pass", _kind(sp), "folded" if fold else "own launch", multi))
    es = 2 if half else 4
    for p in range(world):
      a16 = ((p * geo["rows_block"] + geo["row_off"][t]) * es) % 16 == 0
      if c.exact_form and wire and c.transport != "ipc":
        out.add(("pack", "16-byte" if a16 else "4-byte"))
        out.add(("unpack", "16-byte" if a16 else "4-byte"))
      if c.transport == "ipc" and half:                                 # (direct stores are off for 16-bit gradients)
        out.add(("push half", "16-byte" if a16 else "8-byte"))
    if half:
      out.add(("cvt", "narrow"))
      out.add(("cvt", "widen"))
      if sp.dim % 2:
        out.add(("cvt", "odd dim"))
  return out


EVERYTHING = (
    [("lookup", vw, f) for vw in (4, 1) for f in (False, True)] +
    [("apply", vw, k, m) for vw in (4, 1) for k in ("fast", "generic", "group") for m in (False, True)] +
    [("apply segments", k, n) for k in ("fast", "generic", "group") for n in ("one", "several")] +
    [(w, vw) for w in ("scatter", "build", "exact sum") for vw in (4, 1)] +
    [("displacement pass", k, "own launch", m) for k in ("generic",) for m in (False, True)] +
    [("cvt", w) for w in ("narrow", "widen", "odd dim")] +
    [(w, b) for w in ("pack", "unpack") for b in ("16-byte", "4-byte")] +
    [("push half", b) for b in ("16-byte", "8-byte")])
# not in the list: shard_upsert_kernel / shard_slow_kernel, the per-peer owner form of tables with an occurrence
# filter (test_sharded_step_with_occurrence_filters), which nothing here touches


# ---- the models
_A_OPTS = (("momentum", "adadelta", "rmsprop"), ("rmspropv2", "adam", "amsgrad", "moving_average"))


def _a_specs(dim, half):
  rows = [("%s_%s%d" % ("abcd"[i], o, dim), [(dim, o)]) for i, o in enumerate(_A_OPTS[half])]
  if half == 0:   # the basic + non-basic row: not FAST
    rows.append(("e_ftrl_adam", [(1, "ftrl"), (16, "adam")] if dim % 4 else [(4, "ftrl"), (28, "adam")]))
  return _tables(*rows, initial_capacity=1 << 8)


def _b_specs():
  kw = dict(initial_capacity=1 << 13, max_load_factor=0.97)
  return _tables(("a_adam16", [(16, "adam")]), ("b_momentum32", [(32, "momentum")]), ("c_adam64", [(64, "adam")]), **kw)


_C_VEC = (256, 132, 100, 36, 8, 4)
_C_ODD = (1, 3, 5, 33, 63)


def _c_specs(kind, odd):
  o = {"fast": "adagrad", "generic": "adam", "group": "group"}[kind]
  if not odd:
    rows = [("%s_%s%d" % ("abcdef"[i], o, d), [(d, o)]) for i, d in enumerate(_C_VEC)]
  elif kind == "group":
    rows = [("a_mixed136", [(24, "adagrad"), (40, "group"), (72, "group")])]
    rows += [("%s_group%d" % ("bcd"[i], d), [(d, "group")]) for i, d in enumerate((1, 3, 5))]
    rows += [("e_bias_group32", [(1, "ftrl"), (32, "group")]), ("f_group63", [(63, "group")])]
  else:
    rows = [("%s_%s%d" % ("abcde"[i], o, d), [(d, o)]) for i, d in enumerate(_C_ODD)]
    rows.append(("f_plain64", [(64, o)]))      # float4 rows, off their boundary in the flat buffers
  return _tables(*rows, initial_capacity=1 << 10)


def _c_identity_specs(which):
  if which == "wide":
    opts = ("adam", "adagrad", "adam", "adagrad", "momentum", "adagrad")
    return _tables(*[("%s_%s%d" % ("abcdef"[i], o, d), [(d, o)]) for i, (d, o) in enumerate(zip(_C_VEC, opts))],
                   initial_capacity=1 << 10)
  return _c_specs("fast", True)


def _d_specs(which):
  if which == 0:    # dims 132 + 36 + 4 + 3 = 175
    return _tables(("a_adagrad132", [(132, "adagrad")]), ("b_adam36", [(36, "adam")]), ("c_group4", [(4, "group")]),
                   ("d_adagrad3", [(3, "adagrad")]), initial_capacity=1 << 10)
  return _tables(("a_group16", [(16, "group")]), ("b_adam17", [(17, "adam")]),      # dims 16 + 17 + 33 + 1 = 67
                 ("c_bias_group32", [(1, "ftrl"), (32, "group")]), ("d_sgd1", [(1, "sgd")]), initial_capacity=1 << 10)


def fill_specs(last_dim):
  """the model of section E (and of the three-process case of tests/test_shard_ipc_gpu.py): the last table in
  name order has an odd dim"""
  return _tables(("a_adagrad16", [(16, "adagrad")]), ("b_adam8", [(8, "adam")]),
                 ("c_last%d" % last_dim, [(last_dim, "adagrad")]), initial_capacity=1 << 8)


FILL_B = 64


def _cases():
  P = functools.partial
  out = []
  for dim in (8, 64, 17):
    for half in (0, 1):
      for world in (1, 2, 3):
        out.append(Case("A-dim%d-%s-world%d" % (dim, "mix" if half == 0 else "adam", world), "A",
                        P(_a_specs, dim, half), world, 128, stream="a"))
  for world in (1, 2):
    out.append(Case("B-world%d" % world, "B", _b_specs, world, 1600, steps=5, universe=30000 * world,
                    cap=1600 if world == 1 else 1600 // world + 100, displace=True))
  for kind in ("fast", "generic", "group"):
    for odd in (False, True):
      B = 509 if odd else 512
      out.append(Case("C-%s-%s-world2" % (kind, "odd" if odd else "vec"), "C", P(_c_specs, kind, odd), 2, B))
      out.append(Case("C-%s-%s-world3-zipf" % (kind, "odd" if odd else "vec"), "C", P(_c_specs, kind, odd), 3, B,
                      dist="zipf", exact_order=True))
  for which in ("wide", "odd"):
    out.append(Case("C-identity-%s" % which, "Ci", P(_c_identity_specs, which), 1, 512 if which == "wide" else 509,
                    steps=4, dist="zipf", transport="identity"))
  for which in (0, 1):
    for form in (False, True):
      for world in (2, 3):
        out.append(Case("D-model%d-%s-world%d" % (which, "exact" if form else "fixed", world), "D",
                        P(_d_specs, which), world, 500, fp16=True, exact_form=form))
  out.append(Case("D-zipf-exact-order", "D", P(_d_specs, 1), 3, 500, dist="zipf", fp16=True, exact_order=True))
  out.append(Case("D-40-tables", "D", many_table_specs, 2, 200, fp16=True))
  out.append(Case("D-ipc-to-self", "D1", P(_d_specs, 1), 1, 500, fp16=True, transport="ipc"))
  out.append(Case("D-rccl-to-self-exact", "D1", P(_d_specs, 1), 1, 500, fp16=True, exact_form=True, transport="rccl"))
  for cap in (16, 12):
    for last in (17, 1):
      for fp16 in (False, True):
        for form in (False, True):
          out.append(Case("E-cap%d-last%d-%s-%s" % (cap, last, "fp16" if fp16 else "fp32", "exact" if form else "fixed"),
                          "E", P(fill_specs, last), 3, FILL_B, cap=cap, fp16=fp16, exact_form=form, stream="fill"))
  for last in (17, 1):
    out.append(Case("E-ipc-to-self-last%d" % last, "E1", P(fill_specs, last), 1, FILL_B, cap=12, fp16=True,
                    transport="ipc", stream="fill"))
  return out


CASES = _cases()


def _section(*names):
  return pytest.mark.parametrize("case", [c for c in CASES if c.section in names], ids=lambda c: c.id)


# =============================================================================== G. the plan
def test_the_plan_reaches_every_case():
  reached = set()
  for c in CASES:
    reached |= plan_of(c)
  missing = [x for x in EVERYTHING if x not in reached]
  assert not missing, missing
  by_id = {c.id: plan_of(c) for c in CASES}
  # the basic + non-basic row is served by the generic loop, in its several-segments form
  assert ("apply segments", "generic", "several") in by_id["A-dim64-mix-world2"]
  assert _kind(_a_specs(64, 0)[-1]) == "generic" and _kind(_a_specs(17, 0)[-1]) == "generic"
  assert not any(x[0] == "apply" and x[2] == "fast" for c in CASES if c.section == "A" for x in plan_of(c))
  # one float per lane in the lookup that carries the owed pass: the all-Adagrad world-1 run
  assert ("lookup", 1, True) in by_id["C-identity-odd"]
  # the dim-64 table behind the odd dims: float4 lanes at its owner, one float per lane at its sender
  sp = sorted(_c_specs("fast", True), key=lambda s: s.name)
  assert sp[-1].dim == 64 and (509 * sum(s.dim for s in sp[:-1])) % 4 != 0
  assert ("apply", 4, "fast", True) in by_id["C-fast-odd-world2"] and ("scatter", 4) not in by_id["C-fast-odd-world2"]
  # an odd peer's block of 16-bit gradients starts 8 mod 16 (sections D and E)
  for c in CASES:
    if c.section == "D" and c.id != "D-40-tables":
      geo = shard_block_geometry([s.dim for s in c.specs()], c.B, c.world, c.cap)
      assert (geo["rows_block"] * 2) % 16 == 8, c.id


def _check_apply_launches(c):
  """every rank launched exactly the apply instances of the case's plan"""
  want = {x[1:] for x in plan_of(c) if x[0] == "apply"}

  def check(counts_per_rank):
    for r, counts in enumerate(counts_per_rank):
      for key, n in counts.items():
        k = (key[0], key[2], key[1])
        assert (n > 0) == (k in want), (c.id, r, key, n, sorted(want))
  return check


# =============================================================================== id streams
def _fid(slot, k):
  return (np.int64(slot) << np.int64(48)) | np.asarray(k, dtype=np.int64)


@functools.lru_cache(maxsize=4)
def _a_ids(world, steps):
  """Section A's stream, the same for every table up to its slot: per step and rank 12 ids every rank sends for
  the first time, 12 ids ranks 0 and 1 send, 40 ids only this rank sends, and of the previous step the 12 of
  every rank, 15 of this rank's own and 10 of the next rank's; the first ten twice or three times."""
  out = []
  for s in range(steps + 1):
    per_rank = []
    for r in range(world):
      b = 1000 * s
      parts = [np.arange(b + 1, b + 13), np.arange(b + 200 + 60 * r, b + 240 + 60 * r)]
      if r < 2:
        parts.append(np.arange(b + 101, b + 113))
      if s > 0:
        pb = b - 1000
        parts += [np.arange(pb + 1, pb + 13), np.arange(pb + 200 + 60 * r, pb + 215 + 60 * r),
                  np.arange(pb + 200 + 60 * ((r + 1) % world), pb + 210 + 60 * ((r + 1) % world))]
      k = np.concatenate(parts)
      k = np.concatenate([k, k[:10], k[:5]])
      np.random.default_rng(10 * s + r).shuffle(k)
      per_rank.append(k)
    out.append(per_rank)
  return out


def _a_batches(specs, world, steps):
  ks = _a_ids(world, steps)
  return [[{sp.name: _fid(sp.slot, ks[s][r]) for sp in specs} for r in range(world)] for s in range(steps + 1)]


def _assert_a_stream(batches, specs, world, steps):
  """what section A of the module docstring promises, per table"""
  for sp in specs:
    seen = set()
    for s in range(steps):
      senders = {}
      for r in range(world):
        u, cnt = np.unique(batches[s][r][sp.name], return_counts=True)
        assert cnt.max() <= LIGHT_MAX and cnt.max() >= 2
        for i in u.tolist():
          senders.setdefault(i, set()).add(r)
      n_senders = {i: len(v) for i, v in senders.items()}
      assert 1 in n_senders.values(), (sp.name, s)
      assert min(2, world) in n_senders.values() and world in n_senders.values(), (sp.name, s)
      # new to its owner and sent by every rank: the first sender inserts, the others must not — for every owner
      fresh_all = [i for i, n in n_senders.items() if n == world and i not in seen]
      assert {i % world for i in fresh_all} == set(range(world)), (sp.name, s)
      if s:     # the lookup's record of a resident row is used; resident ids from several senders
        again = [i for i in n_senders if i in prev]
        assert again and any(n_senders[i] == world for i in again), (sp.name, s)
        assert world == 1 or any(n_senders[i] == 2 and senders[i] != prev_senders.get(i) for i in again)
      prev, prev_senders = set(n_senders), senders
      seen |= prev


def _owned(slot, p, k, world):
  """the k-th id (k >= 1) of feature slot `slot` that rank p owns"""
  hi = int(slot) << 48
  return np.int64(hi) + np.asarray(k, dtype=np.int64) * world + (p - hi) % world


def fill_count(cap, T, r, p, t):
  """distinct ids sender r has for peer p in table t: cap, cap - 1, 1 and 0 in turn — the last table (t = T - 1)
  is full from every sender to itself, and in every table some segment is empty and some holds one id"""
  return (cap, cap - 1, 1, 0)[(p + 3 * r + (T - 1 - t)) % 4]


def fill_batches(specs, world, steps, cap):
  """Section E's stream: distinct ids chosen by id % world, ``fill_count`` of them per (sender, peer, table),
  seven further on every step (most recur, every segment has new ones, senders of one peer share ids), the first
  id of a segment three times."""
  by_name = sorted(specs, key=lambda s: s.name)
  out = []
  for s in range(steps + 1):
    per_rank = []
    for r in range(world):
      b = {}
      for t, sp in enumerate(by_name):
        parts = []
        for p in range(world):
          n = fill_count(cap, len(by_name), r, p, t)
          ids = _owned(sp.slot, p, 7 * s + 1 + np.arange(n), world)
          parts += [ids, ids[:1], ids[:1]]
        ids = np.concatenate(parts)
        np.random.default_rng(100 * s + 10 * r + t).shuffle(ids)
        b[sp.name] = ids
      per_rank.append(b)
    out.append(per_rank)
  return out


def segment_counts(batches, specs, world, steps):
  """{(step, sender, peer, table index in name order): distinct ids} of the batches"""
  by_name = sorted(specs, key=lambda s: s.name)
  out = {}
  for s in range(steps):
    for r in range(world):
      for t, sp in enumerate(by_name):
        ids = batches[s][r].get(sp.name)
        for p in range(world):
          out[(s, r, p, t)] = 0 if ids is None else int(np.unique(ids[ids % world == p]).size)
  return out


def _assert_fill(batches, specs, world, steps, cap, B):
  by_name = sorted(specs, key=lambda s: s.name)
  T = len(by_name)
  geo = shard_block_geometry([s.dim for s in by_name], B, world, cap)
  assert geo["cap"] == cap and by_name[-1].dim % 2 == 1
  counts = segment_counts(batches, specs, world, steps)
  assert max(counts.values()) == cap                                   # nothing overflows
  for s in range(steps):
    here = {k[1:]: v for k, v in counts.items() if k[0] == s}
    assert {cap, cap - 1, 1, 0} <= set(here.values()) if world > 1 else {cap, cap - 1, 1} <= set(here.values())
    assert all(here[(r, r, T - 1)] == cap for r in range(world))        # the full segment: the last table
    for r in range(world):
      assert all(b.size <= B for b in batches[s][r].values())


def _seeded_batches(specs, world, steps, B, universe, dist):
  """test_shard_step_gpu._group_against_oracle's own batches (an empty table on rank 1 at even steps, a one-id
  batch on rank 0 at step 2), made here so that a test can look at them first"""
  by_name = sorted(specs, key=lambda s: s.name)
  if universe is None:
    universe = 200000 if dist == "uniform" else 7000

  def one(step, r):
    skip = (by_name[min(3, len(by_name) - 1)].name,) if (r == 1 and step % 2 == 0) else ()
    n = B if not (r == 0 and step == 2) else 1
    return batch_of(specs, 100 * step + r, n, universe, dist, skip)
  return [[one(s, r) for r in range(world)] for s in range(steps + 1)]


def _assert_light(batches, steps):
  for st in batches[:steps]:
    for b in st:
      for ids in b.values():
        assert np.unique(ids, return_counts=True)[1].max() <= LIGHT_MAX


def _batches_of(c, specs):
  if c.stream == "a":
    b = _a_batches(specs, c.world, c.steps)
    _assert_a_stream(b, specs, c.world, c.steps)
  elif c.stream == "fill":
    b = fill_batches(specs, c.world, c.steps, c.cap)
    _assert_fill(b, specs, c.world, c.steps, c.cap, c.B)
  else:
    b = _seeded_batches(specs, c.world, c.steps, c.B, c.universe, c.dist)
  if not c.exact_order and c.transport != "identity":
    _assert_light(b, c.steps)
  return b


def _assert_odd_segment(c, specs, batches):
  """some (sender, peer, table) segment holds an odd number of gradients: its 16-bit words end inside a 4-byte
  word (pack_copy's byte tail) and inside a quad (shard_cvt_kernel)"""
  by_name = sorted(specs, key=lambda s: s.name)
  counts = segment_counts(batches, specs, c.world, c.steps)
  assert any((n * by_name[k[3]].dim) % 2 == 1 for k, n in counts.items()), c.id


# =============================================================================== drivers
def _run_group(c, monkeypatch, check_tables=None):
  if c.fp16:
    monkeypatch.setenv("MHTE_SHARD_GRAD_FP16", "1")
  if c.exact_form:
    monkeypatch.setenv("MHTE_SHARD_EXACT", "1")
  specs = c.specs()
  batches = _batches_of(c, specs)
  if c.fp16:
    _assert_odd_segment(c, specs, batches)
  check = _check_apply_launches(c)
  _group_against_oracle(specs, c.dist, c.world, c.fp16, B=c.B, steps=c.steps, exact_order=c.exact_order,
                        universe=c.universe, ids_per_peer_table=c.cap, check_tables=check_tables,
                        rank_batch=lambda s, r: batches[s][r], check_group=lambda grp: check(grp.apply_launches()))


def _run_one_rank(c, monkeypatch):
  """One rank over a transport to itself against the oracle fed the wire's rounding (the identity exchange
  ignores the wire settings; these do not)."""
  if c.exact_form:
    monkeypatch.setenv("MHTE_SHARD_EXACT", "1")
  specs = c.specs()
  by_name = sorted(specs, key=lambda s: s.name)
  batches = [st[0] for st in _batches_of(c, specs)]
  if c.fp16 and c.section != "E1":    # (one rank's fill model holds 12, 11 and 1 ids of dims 17 | 1, 8 and 16: all even)
    _assert_odd_segment(c, specs, [[b] for b in batches])
  mt = make(specs)
  step = ShardedMultiStep(mt, c.B, ids_per_peer_table=c.cap, transport="ipc" if c.transport == "ipc" else "auto",
                          use_rccl=c.transport == "rccl", grad_fp16=c.fp16)
  info = step.info()
  assert info["transport"].startswith(c.transport), info
  geo = shard_block_geometry(mt.get_table_dim_sizes(), c.B, 1, c.cap)
  assert (info["ids_per_peer_table"], info["row_block_bytes"]) == (geo["cap"], 4 * geo["rows_block"])
  ots = {s.name: s.oracle_table() for s in specs}
  rag = [ragged_of(specs, mt, b) for b in batches]
  for s in range(c.steps):
    emb = step.forward(rag[s], rag[s + 1] if s % 2 == 0 else None)
    views = mt.get_embeddings(rag[s], emb)
    fg = []
    for sp in by_name:
      ids = batches[s][sp.name]
      np.testing.assert_array_equal(views[sp.name].cpu().numpy(), ots[sp.name].lookup(ids)[0],
                                    err_msg="%s step %d" % (sp.name, s))
      g = grads_of(s, 0, sp, ids.size)
      fg.append(g.ravel())
      uk, gu = oracle_backward(ots[sp.name], sp, ids, g)
      if c.fp16:
        gu = gu.astype(np.float16).astype(np.float32)
      ots[sp.name].optimize(uk, gu, sp.lrs(), S.update_time(s))
    step.backward(val_t(np.concatenate(fg)), S.update_time(s))
  step.check()
  for sp in by_name:
    seen = np.unique(np.concatenate([b[sp.name] for b in batches[:c.steps]]))
    got = mt.lookup({sp.name: torch.as_tensor(seen).cuda()})[sp.name].cpu().numpy()
    np.testing.assert_array_equal(got, ots[sp.name].lookup(seen)[0], err_msg=sp.name)
    assert int(mt.size(sp.name)) == seen.size, sp.name
  _check_apply_launches(c)([step.apply_launches()])
  step.close()


# =============================================================================== A. the generic apply instance
@_section("A")
def test_generic_apply_instance(case, monkeypatch):
  _run_group(case, monkeypatch)


# =============================================================================== B. its displacement pass
@_section("B")
def test_generic_displacement_pass_at_high_load(case, monkeypatch):
  """test_group_displacement_at_high_load's tables, batches (the same slots and seeds: the same ids), peer blocks
  and bound — live keys + cap * world stays under 0.97 * 8192 — with Adam and Momentum rows."""
  specs = case.specs()
  _run_group(case, monkeypatch, check_tables=_displaced_not_doubled(specs, 1 << 13))


# =============================================================================== C. lane shapes
@_section("C")
def test_lane_shapes(case, monkeypatch):
  _run_group(case, monkeypatch)


@_section("Ci")
def test_lane_shapes_world1_identity_matches_multi_step(case):
  specs = case.specs()
  by_name = sorted(specs, key=lambda s: s.name)
  B, steps = case.B, case.steps
  batches = [batch_of(specs, 60 + s, B, 3000) for s in range(steps + 1)]
  mt_a, mt_b = make(specs), make(specs)
  ref = MultiSparseStep(mt_a, B)
  shd = ShardedMultiStep(mt_b, B)
  assert shd.info()["transport"] == "identity"
  rag_a = [ragged_of(specs, mt_a, b) for b in batches]
  rag_b = [ragged_of(specs, mt_b, b) for b in batches]
  for s in range(steps):
    ea = ref.forward(rag_a[s], rag_a[s + 1])
    eb = shd.forward(rag_b[s], rag_b[s + 1] if s % 3 != 2 else None)
    assert torch.equal(ea, eb), "forward step %d" % s
    g = val_t(np.concatenate([grads_of(s, 0, sp, B).ravel() for sp in by_name]))
    ref.backward(g, S.update_time(s))
    shd.backward(g, S.update_time(s))
  shd.check()
  allids = {sp.name: np.unique(np.concatenate([b[sp.name] for b in batches])) for sp in specs}
  ra, rb = ragged_of(specs, mt_a, allids), ragged_of(specs, mt_b, allids)
  assert torch.equal(mt_a.raw_lookup(ra), mt_b.raw_lookup(rb))
  _check_apply_launches(case)([shd.apply_launches()])
  ref.close()
  shd.close()


def test_rows_of_more_than_one_trip_are_refused_at_creation():
  """260 floats, and 81 that are not whole float4s: the rows test_optimizer_shapes_gpu gives the op-level
  GroupAdaGrad kernels for their second trip do not get as far as the sharded step's launches"""
  for segs in ([(260, "group", 0.02)], [(1, "ftrl", 0.05), (80, "group", 0.02)]):
    mt = make([Spec("a_group", segs, 1)])
    with pytest.raises(_lib.MhteError) as ei:
      ShardedStepGroup([mt], 64)
    assert ei.value.code == _lib.MHTE_INVALID_ARGUMENT


# =============================================================================== D. the fp16 gradient wire
@_section("D")
def test_fp16_wire(case, monkeypatch):
  _run_group(case, monkeypatch)


@_section("D1")
def test_fp16_wire_one_rank_over_a_transport(case, monkeypatch):
  _run_one_rank(case, monkeypatch)


# =============================================================================== E. segment fill
@_section("E")
def test_segment_fill(case, monkeypatch):
  _run_group(case, monkeypatch)


@_section("E1")
def test_segment_fill_one_rank_over_peer_stores(case, monkeypatch):
  _run_one_rank(case, monkeypatch)
