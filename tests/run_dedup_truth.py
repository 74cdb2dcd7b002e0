"""A plain numpy model and the shared inputs of the RUN dedup of the pipelined single-table step
(csrc/mhte_step_kernels.h): ``rd_dedup_role`` (1024 threads, one position each: ``mhte_step_dedup`` and the
forward launch) and ``rd_dedup4_role`` (256 threads, four positions each — thread t owns local positions t,
t + 256, t + 512, t + 768 — in ``step_bwd_kernel`` when a batch two steps on is handed over).  No GPU, no
import of the engine, nothing taken from oracle/.  tests/test_run_dedup_truth_cpu.py asserts that every case
below has the property it is named for; tests/test_run_dedup_forms_gpu.py runs them.

The constants mirrored here, and the cases that put a batch on each side of them:

  kRdBlock       1024  positions per dedup workgroup                n = 1023, 1024, 1025, 2048, 2049
  kRd4Threads    256   threads of the four-position form            n = 255 .. 257; a last workgroup of 255, 257 and
                                                                    769 positions (valid in 1, 2 and 4 quarters)
  kRdLds         2048  LDS set entries (+ 1 side entry)             1024 distinct ids in every workgroup
  kLongRun       32    bitmap rank | counting rank of a run         runs of 31, 32, 33, 34
   = kLightMax = kStepLightMax   list in ``hlist`` | work items     totals 32 | 33 | 40 over several workgroups
  kMaxLongRuns   16    bitmaps per workgroup                        16, 17 and 31 runs of 33 in one workgroup
  kItemTarget    256   EXPECTED entries per heavy work item: no     lists of 255, 256, 257 in one workgroup and over 8
                       edge at 256.  ``rd_item_blocks`` keeps a     are all ONE item of up to 64 workgroups; the edges
                       list of <= 512 whole and cuts a longer one   512 | 513 and 1024 | 1025 (and 2048 | 2049, 4096 |
                       into power-of-two ranges of workgroups       4097 of the multi-table step's target of 1024) are
                       (513: 16 per item, 1025: 8)                  the ``cut`` family of tests/multi_step_truth.py
  kRdMaxBlocks   64    workgroups per batch                         n = 64 513, 65 535, 65 536
  (count field)  11 bits of the packed LDS word of the 256 form     a run of exactly 1024
  kEmptyKey      INT64_MIN, kept in the side entry / side slot      ``reserved_batch``

Every builder takes a seed — a pipeline of several batches has the same structure with other ids — and
returns int64 ids."""
import numpy as np

import dedup_truth as T
from dedup_truth import INT64_MAX, INT64_MIN  # noqa: F401  (re-exported)

RD_BLOCK = 1024        # kRdBlock
RD4_THREADS = 256      # kRd4Threads
RD_LDS = 2048          # kRdLds
LONG_RUN = 32          # kLongRun = kLightMax = kStepLightMax
LIGHT_MAX = 32
MAX_LONG_RUNS = 16     # kMaxLongRuns
ITEM_TARGET = 256      # kItemTarget
RD_MAX_BLOCKS = 64     # kRdMaxBlocks
QUARTERS = RD_BLOCK // RD4_THREADS

SIZE_EDGES = (1, 255, 256, 257, 1023, 1024, 1025, 1279, 1281, 1793, 2048, 2049)
PATTERNS = ("equal", "distinct", "alternating")
RUN_LENGTHS = (1, 2, 31, 32, 33, 34, 255, 256, 257, 1023, 1024)
LAYOUTS = ("runs", "shuffled", "strided")
SPECIAL = ((0, INT64_MIN), (1, 0), (2, INT64_MAX))
AVOID = (INT64_MIN, 0, INT64_MAX)


# -------------------------------------------------------------------------------------------------- model
def n_workgroups(n):
  return (n + RD_BLOCK - 1) // RD_BLOCK


def workgroup_runs(ids):
  """For each 1024-position workgroup: {id: its local positions in the workgroup, ascending} — what the run
  dedup leaves in ``seg`` and the workgroup's run directory."""
  ids = np.asarray(ids, np.int64)
  out = []
  for b in range(n_workgroups(ids.size)):
    blk = ids[b * RD_BLOCK:(b + 1) * RD_BLOCK]
    keys, inv, counts = np.unique(blk, return_inverse=True, return_counts=True)
    order = np.argsort(inv.reshape(-1), kind="stable")
    out.append(dict(zip(keys.tolist(), np.split(order, np.cumsum(counts)[:-1]))))
  return out


def totals(ids, runs=None):
  """{id: occurrences in the whole batch}, summed over the workgroups' runs."""
  tot = {}
  for wg in (runs if runs is not None else workgroup_runs(ids)):
    for k, pos in wg.items():
      tot[k] = tot.get(k, 0) + pos.size
  return tot


def light(ids, runs=None):
  """{id: True when its gradient list is summed by one lane group (<= 32 occurrences in the batch)}."""
  return {k: c <= LIGHT_MAX for k, c in totals(ids, runs).items()}


def split_of(key, runs):
  """Occurrences of ``key`` per workgroup."""
  return [wg[key].size if key in wg else 0 for wg in runs]


def unique_first_occurrence(ids, runs=None):
  """(uids, inverse, seg_off, seg_pos) as dedup_truth.unique_first_occurrence, derived from the runs alone:
  workgroups are position ranges, so an id's runs in workgroup order are its occurrence list, and its first
  occurrence is the first position of its first run."""
  ids = np.asarray(ids, np.int64)
  runs = runs if runs is not None else workgroup_runs(ids)
  lists, first = {}, {}
  for b, wg in enumerate(runs):
    for k, pos in wg.items():
      lists.setdefault(k, []).append(pos + b * RD_BLOCK)
      first.setdefault(k, int(pos[0]) + b * RD_BLOCK)
  keys = sorted(first, key=first.get)
  uids = np.array(keys, np.int64)
  inverse = np.empty(ids.size, np.int64)
  seg_pos, seg_off = [], [0]
  for u, k in enumerate(keys):
    p = np.concatenate(lists[k])
    inverse[p] = u
    seg_pos.append(p)
    seg_off.append(seg_off[-1] + p.size)
  seg_pos = np.concatenate(seg_pos).astype(np.int64) if seg_pos else np.zeros(0, np.int64)
  return uids, inverse, np.asarray(seg_off, np.int64), seg_pos


def quarters_of(pos):
  """The quarters (local position // 256: which of a thread's four positions) a run's positions fall in."""
  return sorted(set((np.asarray(pos) // RD4_THREADS).tolist()))


def last_workgroup_quarters(n):
  """How many quarters of the last workgroup hold a valid position."""
  last = n - RD_BLOCK * (n_workgroups(n) - 1)
  return (last + RD4_THREADS - 1) // RD4_THREADS


# ----------------------------------------------------------------------------------------------- builders
def _place(n, members, rng):
  """ids [n]: ``members`` is a list of (key, positions); every other position gets a distinct singleton."""
  out = np.empty(n, np.int64)
  taken = np.zeros(n, bool)
  for key, pos in members:
    pos = np.asarray(pos, np.int64)
    assert pos.size == np.unique(pos).size and not taken[pos].any() and pos.max() < n
    out[pos] = key
    taken[pos] = True
  free = np.flatnonzero(~taken)
  out[free] = T._distinct_keys(rng, free.size, avoid=[k for k, _ in members] + list(AVOID))
  return out


def _spread(rng, count, lo, hi, quarters=True):
  """``count`` distinct positions of [lo, hi), in seeded random order; with ``quarters`` (and a range that is
  one whole workgroup) the first min(count, 4) of them fall in different quarters."""
  if not quarters or hi - lo != RD_BLOCK or count < 2:
    return lo + rng.permutation(hi - lo)[:count]
  qs = rng.permutation(QUARTERS)[:min(count, QUARTERS)]
  head = lo + qs * RD4_THREADS + rng.integers(0, RD4_THREADS, size=qs.size)
  rest = np.setdiff1d(np.arange(lo, hi), head)
  return np.concatenate([head, rest[rng.permutation(rest.size)][:count - head.size]])


def size_batch(n, pattern, seed):
  """A size edge with the pattern "equal", "distinct" or "alternating" (dedup_truth.tiny_batch)."""
  return T.tiny_batch(n, pattern, seed=seed)


def one_id_and_a_single_batch(n, seed):
  """One id everywhere plus one single occurrence at the very end: runs of 1024 in every full workgroup."""
  a, b = T._distinct_keys(np.random.default_rng(seed), 2, AVOID)
  out = np.full(n, a, np.int64)
  out[-1] = b
  return out


RUN_N, RUN_WG = 2 * RD_BLOCK, 1        # the run-length and long-run cases: the run lies in workgroup 1 of 2


def run_length_batch(length, layout, seed):
  """n = 2048: ONE id with a run of ``length`` in workgroup 1, every other position a distinct singleton.
    "runs"      the run's positions adjacent, centred in the workgroup
    "shuffled"  seeded random positions, in all four quarters (of min(length, 4) of them)
    "strided"   positions floor(i * 1024 / length): evenly spread, in all four quarters"""
  rng = np.random.default_rng(seed)
  lo = RUN_WG * RD_BLOCK
  if layout == "runs":
    pos = lo + (RD_BLOCK - length) // 2 + np.arange(length)
  elif layout == "shuffled":
    pos = _spread(rng, length, lo, lo + RD_BLOCK)
  elif layout == "strided":
    pos = lo + (np.arange(length) * RD_BLOCK) // length
  else:
    raise ValueError(layout)
  key = T._distinct_keys(rng, 1, AVOID)[0]
  return _place(RUN_N, [(key, pos)], rng)


def long_runs_batch(n_runs, seed, length=LONG_RUN + 1):
  """n = 2048: ``n_runs`` ids with a run of 33 each in workgroup 1, shuffled over the whole workgroup; every
  other position a distinct singleton (31 runs of 33 leave exactly one)."""
  rng = np.random.default_rng(seed)
  lo = RUN_WG * RD_BLOCK
  pos = lo + rng.permutation(RD_BLOCK)[:n_runs * length].reshape(n_runs, length)
  keys = T._distinct_keys(rng, n_runs, AVOID)
  return _place(RUN_N, list(zip(keys.tolist(), pos)), rng)


LDS_WGS = 3


def lds_fill_batch(with_reserved, seed):
  """1024 distinct ids in every one of 3 workgroups, no id twice in the batch: the LDS set at half load.
  ``with_reserved``: 1023 distinct ids plus INT64_MIN in every workgroup."""
  rng = np.random.default_rng(seed)
  n = LDS_WGS * RD_BLOCK
  members = []
  if with_reserved:
    members = [(INT64_MIN, np.arange(LDS_WGS) * RD_BLOCK + rng.integers(0, RD_BLOCK, size=LDS_WGS))]
  return _place(n, members, rng)


def split_batch(splits, n, seed, keys=()):
  """ids [n] in which key k has ``splits[k][b]`` occurrences in workgroup b, at seeded random positions of
  it (in different quarters where the workgroup is whole); every other position a distinct singleton.
  ``keys``: literal ids of the first keys (INT64_MIN, 0, INT64_MAX), the others are seeded draws."""
  rng = np.random.default_rng(seed)
  nb = n_workgroups(n)
  names = list(keys) + T._distinct_keys(rng, len(splits) - len(keys), AVOID).tolist()
  free = [list(range(b * RD_BLOCK, min(n, (b + 1) * RD_BLOCK))) for b in range(nb)]
  pos = [[] for _ in splits]
  for k, split in enumerate(splits):
    assert len(split) <= nb
    for b, c in enumerate(split):
      if c == 0:
        continue
      lo = b * RD_BLOCK
      if len(free[b]) == RD_BLOCK:
        take = _spread(rng, c, lo, lo + RD_BLOCK)
      else:
        f = np.asarray(free[b], np.int64)
        take = f[rng.permutation(f.size)[:c]]
      assert take.size == c
      pos[k].extend(take.tolist())
      gone = set(take.tolist())
      free[b] = [p for p in free[b] if p not in gone]
  return _place(n, [(names[k], pos[k]) for k in range(len(splits))], rng)


# the reserved key INT64_MIN (kEmptyKey): LDS side entry, side slot of the global scratch
RESERVED = {
    "once": ([[0, 1]], 1300),                              # one occurrence, in the partial workgroup
    "run32": ([[0, 32]], 2048),                            # a light list of exactly 32, one run
    "run33": ([[0, 33]], 2048),                            # one run of 33: a long run, a heavy list
    "workgroup": ([[0, 1024, 0]], 2049),                   # a whole workgroup: the 11-bit count on the side entry
    "33-singles": ([[1] * 33], 32 * RD_BLOCK + 7),         # heavy, 33 runs of one through the side slot
    "with-0-and-max": ([[20, 13], [3, 2], [17, 23]], 1500),  # heavy MIN (33), light 0 (5), heavy MAX (40)
}
RESERVED_KEYS = (INT64_MIN, 0, INT64_MAX)


def reserved_batch(kind, seed):
  splits, n = RESERVED[kind]
  return split_batch(splits, n, seed, keys=RESERVED_KEYS[:len(splits)])


# lists across workgroups at the light / heavy edge: name -> (splits of the FIRST key(s), n)
EDGE = {
    "32=16+16": ([[16, 16]], 1500),
    "32=31+1": ([[31, 1]], 1500),
    "32=1x32": ([[1] * 32], 31 * RD_BLOCK + 7),
    "33=32+1": ([[32, 1]], 1500),
    "33=17+16": ([[17, 16]], 1500),
    "40=20+20": ([[20, 20]], 1500),                        # ``hlist`` written by one run, outgrown by the other
    "256-in-one": ([[0, 256]], 2048),
    "257-in-one": ([[0, 257]], 2048),
    "256-over-8": ([[32] * 8], 7 * RD_BLOCK + 500),
    "257-over-8": ([[32] * 7 + [33]], 7 * RD_BLOCK + 500),
    "64=1x64": ([[1] * 64], 63 * RD_BLOCK + 300),
}


def edge_batch(kind, seed):
  if kind == "300x33":                                     # dedup_truth's HEAVY_KEYS x HEAVY_LEN
    return T.ladder_batch([T.HEAVY_LEN] * T.HEAVY_KEYS, T.HEAVY_N, "strided", seed)
  splits, n = EDGE[kind]
  return split_batch(splits, n, seed)


def edge_key(ids, kind):
  """The id of an EDGE case's key: the only id with that many occurrences."""
  splits, _ = EDGE[kind]
  want = sum(splits[0])
  hit = [k for k, c in totals(ids).items() if c == want]
  assert len(hit) == 1, (kind, hit)
  return hit[0]


# ------------------------------------------------------------------------------- rows that name their id
NAME_LIMIT = 2 ** 22          # every element of a naming row is an integer below this
NAME_TINY = 2.0 ** -40        # scale of the naming rows of a table with real-valued updates: exact in fp32, and
                              # far below the rounding of an update of ~1e-2, which it therefore does not blunt


def naming_rows(ids, dim, seed, scale=1.0):
  """(the distinct ids, sorted; rows [k, dim]): row of an id = (a number unique to the id + the column index)
  * scale — assigned to a table before a pipeline starts, every element of every forward output then says
  whose row it is (a pipeline's ids are new in every batch: without it every forward returns the initializer's
  zeros, and a row scattered to the wrong occurrence is not seen)."""
  u = np.unique(np.asarray(ids, np.int64))
  base = 1 + np.random.default_rng(seed).permutation(u.size)
  rows = base[:, None] + np.arange(dim)[None, :]
  assert rows.max() < NAME_LIMIT
  return u, (rows.astype(np.float64) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ registry
def _cases():
  """name -> (family, builder(seed))."""
  c = {}
  for n in SIZE_EDGES:
    for pattern in PATTERNS:
      c["size-%s-%d" % (pattern, n)] = ("size", lambda seed, n=n, p=pattern: size_batch(n, p, seed))
  for n in (RD_MAX_BLOCKS * RD_BLOCK - 1, RD_MAX_BLOCKS * RD_BLOCK):
    c["size-one-id-and-a-single-%d" % n] = ("size", lambda seed, n=n: one_id_and_a_single_batch(n, seed))
  c["size-distinct-64513"] = ("size", lambda seed: size_batch(63 * RD_BLOCK + 1, "distinct", seed))
  for length in RUN_LENGTHS:
    for layout in LAYOUTS:
      c["run-%d-%s" % (length, layout)] = ("run", lambda seed, l=length, y=layout: run_length_batch(l, y, seed))
  for k in (MAX_LONG_RUNS, MAX_LONG_RUNS + 1, 31):
    c["long-%dx33" % k] = ("long", lambda seed, k=k: long_runs_batch(k, seed))
  c["lds-1024-distinct"] = ("lds", lambda seed: lds_fill_batch(False, seed))
  c["lds-1023-distinct-and-min"] = ("lds", lambda seed: lds_fill_batch(True, seed))
  for kind in RESERVED:
    c["reserved-%s" % kind] = ("reserved", lambda seed, k=kind: reserved_batch(k, seed))
  for kind in list(EDGE) + ["300x33"]:
    c["edge-%s" % kind] = ("edge", lambda seed, k=kind: edge_batch(k, seed))
  return c


CASES = _cases()


PIPELINE = 6           # batches of a pipeline: 4 steps and the two batches of look-ahead behind the last


def build(name, seed):
  return CASES[name][1](seed)


def pipeline_seeds(name):
  """The consecutive seeds of a case's pipeline (the same in the CPU and the GPU suite)."""
  base = 1000 * list(CASES).index(name) + 17
  return list(range(base, base + PIPELINE))


def names(*families):
  return [k for k, (f, _) in CASES.items() if f in families]
