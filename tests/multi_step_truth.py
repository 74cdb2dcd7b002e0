"""The shared inputs of the multi-table step's run-dedup edge suite (csrc/mhte_mstep_kernels.h,
csrc/mhte_mstep_host.h): the cases of tests/run_dedup_truth.py, a ``cut`` family that puts a list spread over
many dedup workgroups on each side of every edge of ``rd_item_blocks``, and the deal of cases to the tables of a
model.  Numpy only: no GPU, no import of the engine, nothing taken from oracle/.
tests/test_multi_step_truth_cpu.py asserts that every case and every deal has the property it is named for;
tests/test_multi_step_forms_gpu.py runs them.  ``run_dedup_truth.CASES`` is left as it is (its order fixes the
seeds and the parametrisation of the single-table suite); the ``cut`` cases live in a registry of their own.

The item cut mirrored here (csrc/mhte_step_kernels.h, ``rd_item_blocks(c, target)``; ``MultiStep::init`` sets
``target`` to 256 for fewer than four tables and to 1024 from four on):

  a list of c <= 2 * target occurrences stays whole: as many of the 64 dedup workgroups per item as keep
  c * workgroups <= 128 * target (64, then halved); a longer list is cut into power-of-two ranges of workgroups
  with c * workgroups <= 64 * target, and its items are followed by a hand-off.

    target   256:   c = 512 -> 64 workgroups per item | 513 -> 16      1024 -> 16 | 1025 -> 8
    target  1024:   c = 2048 -> 64 | 2049 -> 16                        4096 -> 16 | 4097 -> 8
"""
import itertools

import numpy as np

import run_dedup_truth as R

ITEM_TARGETS = (256, 1024)
MAX_ITEM_BLOCKS = 64         # run descriptors per item = kRdMaxBlocks
HEAVY_ITEM_SPLIT_PASS = 64   # occurrences a wavefront of the forward's heavy scatter stores per pass


def item_target(n_tables):
  """``MultiStep::init``: expected occurrences per heavy work item."""
  return 4 * R.ITEM_TARGET if n_tables >= 4 else R.ITEM_TARGET


def item_split(target):
  """Wavefronts of the forward's scatter that share a heavy item (``launch_fwd``)."""
  return max(1, target // R.ITEM_TARGET)


def item_blocks(c, target):
  """``rd_item_blocks(c, target)``: dedup workgroups per work item of a list of ``c`` occurrences."""
  nbk = MAX_ITEM_BLOCKS
  lim = target * 64 * (1 if c > 2 * target else 2)
  while nbk > 1 and c * nbk > lim:
    nbk >>= 1
  return nbk


def items_of(split, target):
  """A heavy list with ``split[b]`` occurrences in dedup workgroup b -> (workgroups per item, the occurrences
  of every NON-EMPTY item in workgroup order) as ``rd_emit_items`` cuts it: aligned ranges of
  ``item_blocks`` workgroups, a range without a run of the list gets no item."""
  nbk = item_blocks(int(sum(split)), target)
  per_item = [int(sum(split[b0:b0 + nbk])) for b0 in range(0, len(split), nbk)]
  return nbk, [e for e in per_item if e]


def heavy_items(ids, target):
  """{id: (workgroups per item, occurrences per non-empty item)} of every heavy list (> 32) of a batch."""
  runs = R.workgroup_runs(ids)
  return {k: items_of(R.split_of(k, runs), target) for k, c in R.totals(ids, runs).items() if c > R.LIGHT_MAX}


# ------------------------------------------------------------------------------------------- the cut family
CUT_WGS = 32                                  # whole workgroups the list is spread evenly over
CUT_N = CUT_WGS * R.RD_BLOCK + 232            # 33 000: a 33rd, partial workgroup holds the odd occurrence
CUT_LENGTHS = tuple((target, c) for target in ITEM_TARGETS
                    for c in (2 * target, 2 * target + 1, 4 * target, 4 * target + 1))


def cut_name(target, c):
  return "cut-t%d-%d" % (target, c)


def cut_split(c):
  """``c`` occurrences evenly over 32 whole workgroups, the odd one in workgroup 33."""
  assert (c - c % 2) % CUT_WGS == 0
  return [c // CUT_WGS] * CUT_WGS + ([1] if c % 2 else [])


def cut_batch(c, seed):
  """n = 33 000: ONE id with ``cut_split(c)``, every other position a distinct singleton."""
  return R.split_batch([cut_split(c)], CUT_N, seed)


def cut_key(ids, c):
  hit = [k for k, v in R.totals(ids).items() if v == c]
  assert len(hit) == 1, (c, hit)
  return hit[0]


CUT = {cut_name(t, c): ("cut", lambda seed, c=c: cut_batch(c, seed)) for t, c in CUT_LENGTHS}

# every case the multi-table suite knows: the single-table suite's, then the cut family
ALL = dict(R.CASES)
ALL.update(CUT)
assert len(ALL) == len(R.CASES) + len(CUT)


def family(name):
  return ALL[name][0]


def build(name, seed):
  return ALL[name][1](seed)


def pipeline_seeds(name):
  """Consecutive seeds of a case's pipeline: the single-table suite's for its cases, a range behind them for
  the cut family."""
  if name in R.CASES:
    return R.pipeline_seeds(name)
  base = 1000 * (len(R.CASES) + list(CUT).index(name)) + 17
  return list(range(base, base + R.PIPELINE))


def names(*families):
  return [k for k, (f, _) in ALL.items() if f in families]


_SIZE = {}


def size_of(name):
  if name not in _SIZE:
    _SIZE[name] = int(build(name, pipeline_seeds(name)[0]).size)
  return _SIZE[name]


# the cases every forward form runs (the others run in the fused and the two-launch form only)
FORM_RUN_LENGTHS = (32, 33, 1024)
FORM_SIZES = (1, 255, 257, 1023, 1024, 1025)


def form_cases():
  out = names("edge", "reserved", "long", "cut")
  out += ["run-%d-%s" % (l, y) for l in FORM_RUN_LENGTHS for y in R.LAYOUTS]
  out += ["size-%s-%d" % (p, n) for n in FORM_SIZES for p in R.PATTERNS]
  return [k for k in ALL if k in set(out)]       # registry order


def other_cases():
  chosen = set(form_cases())
  return [k for k in ALL if k not in chosen]


def order_cases():
  """The cases of the Adagrad model (the order inside a list)."""
  return names("run", "long", "reserved", "edge", "cut")


# --------------------------------------------------------------------------------------------------- the deal
TAIL_EDGES = (1, 255, 1023)     # positions in the last dedup workgroup of a table
EMPTY_STEPS = (1, 3)            # the batches in which the emptied table of a deal has no ids


def tail(n):
  """Positions in the last 1024-position block of a table with ``n`` ids."""
  return n - R.RD_BLOCK * (R.n_workgroups(n) - 1) if n else 0


def deal(case_names, n_tables):
  """Partition ``case_names`` into groups of ``n_tables``, one case per table of a model (in table order).
  Cases are sorted by batch size and dealt round-robin, so a group holds small and large batches; inside a
  group the order is the first permutation in which neighbouring tables differ in size, preferring one that
  keeps a case whose last block has 1, 255 or 1023 positions off the last table.  The last group is filled up
  with the first cases again (those then run twice)."""
  by_size = sorted(case_names, key=lambda k: (size_of(k), list(ALL).index(k)))
  n_groups = -(-len(by_size) // n_tables)
  padded = by_size + by_size[:n_groups * n_tables - len(by_size)]
  groups = []
  for g in range(n_groups):
    members = padded[g::n_groups]
    assert len(members) == n_tables

    def score(perm):
      sizes = [size_of(k) for k in perm]
      clash = sum(a == b for a, b in zip(sizes, sizes[1:]))
      edge_last = tail(sizes[-1]) in TAIL_EDGES and len(perm) > 1
      return (clash, edge_last)

    groups.append(tuple(min(itertools.permutations(members), key=score)))
  return groups


def emptied_table(group_index, n_tables):
  """The table that has no ids at all in the batches EMPTY_STEPS of a group, or None: a middle table of the
  first group of every deal (the first of two)."""
  if group_index != 0:
    return None
  return n_tables // 2 if n_tables >= 3 else 0


def model_groups(n_tables):
  """The groups a model of ``n_tables`` case tables runs: [(label, group, emptied table or None, every_form)].
  The cases of every form are dealt first ("f.."), the others on their own ("o.."), so that a group is the same
  set of batches in every form that runs it."""
  out = []
  for prefix, cases, every in (("f", form_cases(), True), ("o", other_cases(), False)):
    for g, group in enumerate(deal(cases, n_tables)):
      out.append(("%s%02d" % (prefix, g), group, emptied_table(g, n_tables), every))
  return out


def deal_batches(group, hole):
  """[batch][table] -> ids of a dealt group: every case's pipeline, the batches EMPTY_STEPS of table ``hole``
  (None: no such table) cut to zero ids."""
  per_table = [[build(k, seed) for seed in pipeline_seeds(k)] for k in group]
  out = []
  for s in range(R.PIPELINE):
    row = [per_table[t][s] for t in range(len(group))]
    if hole is not None and s in EMPTY_STEPS:
      row[hole] = np.zeros(0, np.int64)
    out.append(row)
  return out


def block_starts(sizes):
  """``blk_start[]`` of a dedup launch over tables of ``sizes`` ids."""
  out = [0]
  for n in sizes:
    out.append(out[-1] + R.n_workgroups(n))
  return out
