"""Plain numpy models and the shared inputs of the list-building dedup (``mhte_unique``,
``mhte_unique_unordered``) and of the ops that read its lists (``mhte_segment_sum``, ``mhte_gather_rows``, the
chunk role of ``sum_apply_kernel``): csrc/mhte_kernels.h ``dd_*`` / ``segsum_*``.  No GPU, no import of the
engine, nothing taken from oracle/ (tests/test_dedup_truth_cpu.py checks these models AGAINST the oracle).

The batches are built so that every size constant of those kernels has a case on each side of it, by design
and not by the luck of a Zipf draw:

  kDdBlock / kDdTile 1024  positions per workgroup and per tile     n = 1023, 1024, 1025; 8192 and 8193
  kDdLds             2048  LDS hash set (2 x the positions)         all-distinct blocks: 1024 keys in the set
  kLightMax          32    rank sort in registers | bitmap ordering list lengths 31, 32, 33, 34
  kChunk             256   work items of the fused backward         255, 256, 257, 511, 512, 513, ... 2049
  kBmBits            262144 bitmap ordering in chunks               ``chunk_straddle_batch``
  hgrid              256   heavy workgroups loop                    300 lists of 33 (``HEAVY_KEYS``)
  C                  max(1024, pow2 >= 2n)                          n = 512 | 513
  pick_shape         (G, VEC)                                       ``SEG_LADDER`` x ``classify_windows``
"""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min   # the reserved key of the engine's hash sets: a legal id all the same
INT64_MAX = np.iinfo(np.int64).max
BLOCK = 1024                         # kDdBlock
LIGHT_MAX = 32                       # kLightMax
BM_BITS = 262144                     # kBmBits

# list lengths around kLightMax, kChunk and its multiples, kDdBlock and 2 * kDdBlock
LADDER = [1, 2, 31, 32, 33, 34, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049]
LADDER_SUM = 7558
LADDER_TOTALS = (7558, 8192, 8193)   # no padding | whole 1024-blocks | one position in a ninth block

# The segment-sum ladder ("runs" layout: CSR order == batch order, list bounds == prefix sums).  With
# WIN = min(G, 16): 16, 32, 5, 16, 3, 40 put lists on and off the window bounds of WIN = 16, the 3, 9 that
# follow give WIN = 8 a list from mid-window to mid-window of the next; 2049 entries are 257 or more windows
# of 8 (per > 8 at G = 8, NG = 32) and 129 or more of 16 (per > 8 at G = 16, > 16 at G = 32 and 64); 4100
# make per > 16 at G = 8 and 16 as well (see classify_windows).
SEG_LADDER = [16, 32, 5, 16, 3, 40, 3, 9, 1, 2, 31, 33, 255, 256, 257, 513, 1025, 2049, 4100]
SEG_LADDER_SUM = 8646
SEG_TOTALS = (8656, 8661)            # n % 16 == 0: the last window is full; n % 16 == 5 (and % 8 == 5): partial

HEAVY_KEYS, HEAVY_LEN = 300, 33      # more heavy lists than the 256 heavy workgroups; n = 9900 = 300 * 33
HEAVY_N = HEAVY_KEYS * HEAVY_LEN

CHUNK_N = BM_BITS + 1000             # two bitmap chunks
CHUNK_KEYS, CHUNK_LEN = 300, 40

assert sum(LADDER) == LADDER_SUM and sum(SEG_LADDER) == SEG_LADDER_SUM


# ------------------------------------------------------------------------------------------------ batches
def _distinct_keys(rng, count, avoid):
  """``count`` distinct int64 keys over the full range (negative values included), none of ``avoid``."""
  out = np.zeros(0, np.int64)
  while out.size < count:
    draw = rng.integers(INT64_MIN, INT64_MAX, size=count - out.size + 16, dtype=np.int64, endpoint=True)
    draw = draw[~np.isin(draw, np.asarray(list(avoid), dtype=np.int64))]
    both = np.concatenate([out, draw])
    _, first = np.unique(both, return_index=True)
    out = both[np.sort(first)]
  return out[:count]


def _deal_strided(lens, n, rng):
  """The key at every batch position of the "strided" layout.  Keys by descending length; first every key of
  two or more occurrences gets one position in each of min(len, nblocks) consecutive 1024-blocks that still
  have room (the last block may be short: its positions go to the longest keys), then the occurrences that
  are left are dealt round-robin over the blocks with room.  Every block takes exactly its capacity."""
  nb = (n + BLOCK - 1) // BLOCK
  cap = np.full(nb, BLOCK, np.int64)
  cap[-1] = n - BLOCK * (nb - 1)
  members = [[] for _ in range(nb)]
  order = np.argsort(-np.asarray(lens), kind="stable")
  left = np.array(lens, np.int64)
  c = 0
  for k in order:
    if lens[k] < 2:
      break
    want = min(int(lens[k]), nb)
    for _ in range(nb):                      # one trip round the blocks at most
      if lens[k] - left[k] == want:
        break
      if len(members[c]) < cap[c]:
        members[c].append(k)
        left[k] -= 1
      c = (c + 1) % nb
  for k in order:
    for _ in range(int(left[k])):
      while len(members[c]) == cap[c]:
        c = (c + 1) % nb
      members[c].append(k)
      c = (c + 1) % nb
  key_at = np.empty(n, np.int64)
  for b in range(nb):
    m = np.asarray(members[b], np.int64)
    key_at[b * BLOCK:b * BLOCK + m.size] = m[rng.permutation(m.size)]   # no order inside a block either
  return key_at


def ladder_batch(lengths, n, layout, seed, special=()):
  """int64 ids [n] in which key k occurs exactly ``lengths[k]`` times, padded to ``n`` with distinct
  singleton keys.  Keys are seeded draws over the full int64 range; ``special`` is a sequence of
  (k, literal id) that pins key k (INT64_MIN, 0, INT64_MAX).  ``layout``:
    "runs"      the occurrences of a key adjacent, keys in ladder order, the singletons last
    "shuffled"  a seeded permutation of "runs"
    "strided"   every key spread as evenly as possible over all 1024-position blocks"""
  lengths = [int(x) for x in lengths]
  pad = n - sum(lengths)
  assert pad >= 0 and min(lengths + [1]) >= 1
  lens = np.asarray(lengths + [1] * pad, np.int64)
  rng = np.random.default_rng(seed)
  pinned = dict(special)
  keys = _distinct_keys(rng, lens.size, avoid=[INT64_MIN, 0, INT64_MAX])
  for k, lit in pinned.items():
    keys[k] = lit
  assert np.unique(keys).size == keys.size
  if layout == "runs":
    return np.repeat(keys, lens)
  if layout == "shuffled":
    return np.repeat(keys, lens)[rng.permutation(n)]
  if layout == "strided":
    return keys[_deal_strided(lens, n, rng)]
  raise ValueError(layout)


def tiny_batch(n, pattern, seed=11):
  """``pattern``: "equal" (one key), "distinct" (n keys), "alternating" (two keys, a b a b ...)."""
  rng = np.random.default_rng(seed)
  if pattern == "equal":
    return np.repeat(_distinct_keys(rng, 1, ()), n)
  if pattern == "distinct":
    return _distinct_keys(rng, n, ())
  if pattern == "alternating":
    return _distinct_keys(rng, 2, ())[np.arange(n) % 2]
  raise ValueError(pattern)


def chunk_straddle_batch(seed=5):
  """n = 262 144 + 1000: 300 keys of 40 occurrences, every other id a singleton.  Key 0 has positions on
  both sides of the bitmap chunk bound, 262 143 and 262 144 among them; key 1 lies wholly in the second
  chunk, key 2 wholly in the first; the other keys lie anywhere.  Returns (ids, keys[:3])."""
  n = CHUNK_N
  rng = np.random.default_rng(seed)
  keys = _distinct_keys(rng, CHUNK_KEYS + n - CHUNK_KEYS * CHUNK_LEN, avoid=[INT64_MIN, 0, INT64_MAX])
  key_at = np.full(n, -1, np.int64)
  lo = rng.permutation(BM_BITS - 1)                          # positions below 262 143
  hi = BM_BITS + 1 + rng.permutation(n - BM_BITS - 1)        # positions above 262 144
  half = (CHUNK_LEN - 2) // 2
  key_at[[BM_BITS - 1, BM_BITS]] = 0
  key_at[lo[:half]] = 0
  key_at[hi[:CHUNK_LEN - 2 - half]] = 0
  key_at[hi[CHUNK_LEN:2 * CHUNK_LEN]] = 1
  key_at[lo[CHUNK_LEN:2 * CHUNK_LEN]] = 2
  free = np.flatnonzero(key_at < 0)
  free = free[rng.permutation(free.size)]
  rest = np.concatenate([np.repeat(np.arange(3, CHUNK_KEYS), CHUNK_LEN), np.arange(CHUNK_KEYS, keys.size)])
  assert rest.size == free.size
  key_at[free] = rest
  return keys[key_at], keys[:3]


# ------------------------------------------------------------------------------------------------ models
def unique_first_occurrence(ids):
  """(uids, inverse, seg_off, seg_pos): the distinct ids numbered by first occurrence, the number of every
  position, and the positions grouped by number, ascending inside every list (CSR)."""
  ids = np.asarray(ids, np.int64)
  if ids.size == 0:
    return ids.copy(), np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
  sorted_keys, first, inv_sorted = np.unique(ids, return_index=True, return_inverse=True)
  by_first = np.argsort(first, kind="stable")
  number = np.empty(sorted_keys.size, np.int64)
  number[by_first] = np.arange(sorted_keys.size)
  inverse = number[inv_sorted.reshape(-1)]
  seg_pos = np.argsort(inverse, kind="stable")
  seg_off = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=sorted_keys.size))])
  return sorted_keys[by_first], inverse, seg_off.astype(np.int64), seg_pos.astype(np.int64)


def segment_sum_seq32(g, seg_off, seg_pos):
  """out[u] = 0 + g[p0] + g[p1] + ... over list u, one float32 addition after the other."""
  g = np.ascontiguousarray(g, np.float32)
  seg_off, seg_pos = np.asarray(seg_off, np.int64), np.asarray(seg_pos, np.int64)
  lens = np.diff(seg_off)
  out = np.zeros((lens.size, g.shape[1]), np.float32)
  by_len = np.argsort(-lens, kind="stable")       # the lists that are still running are a prefix of by_len
  sorted_lens = lens[by_len]
  for r in range(int(lens.max()) if lens.size else 0):
    live = by_len[:np.searchsorted(-sorted_lens, -r, side="left")]   # lens > r
    out[live] = out[live] + g[seg_pos[seg_off[live] + r]]
  return out


def segment_sum_f64(g, seg_off, seg_pos):
  """The same sum in float64."""
  g = np.asarray(g, np.float64)
  seg_off, seg_pos = np.asarray(seg_off, np.int64), np.asarray(seg_pos, np.int64)
  if seg_off.size <= 1:
    return np.zeros((0, g.shape[1]), np.float64)
  return np.add.reduceat(g[seg_pos], seg_off[:-1], axis=0)   # (every list has at least one position)


def classify_windows(seg_off, n, G):
  """The list classes of segsum_window_kernel / segsum_combine_kernel that occur, for WIN = min(G, 16)
  entries per window and NG = 256 // G lane groups in the combine.  A list [s0, s1) touches the windows
  w0 = s0 // WIN .. w1 = (s1 - 1) // WIN; a list that crosses a bound is combined from items = w1 - w0 + 1
  partial rows, per = ceil(items / NG) of them per lane group.
    a  lies inside one window                     b  crosses a bound and ends exactly on one
    c  starts on a bound, spans exactly two       d  from mid-window to mid-window of the next
    e  covers a whole interior window             f  items > NG (per > 1)
    g  per > 8 (a second trip of `i += 8`)        h  per > 16
    i  the last window is partial                 j  the last window is full"""
  seg_off = np.asarray(seg_off, np.int64)
  win, ng = min(G, 16), 256 // G
  s0, s1 = seg_off[:-1], seg_off[1:]
  w0, w1 = s0 // win, (s1 - 1) // win
  cross = w1 > w0
  per = -(-(w1 - w0 + 1) // ng)
  has = {
      "a": bool(np.any(~cross)),
      "b": bool(np.any(cross & (s1 % win == 0))),
      "c": bool(np.any((s0 % win == 0) & (s1 - s0 == 2 * win))),
      "d": bool(np.any((s0 % win != 0) & (s1 % win != 0) & (w1 == w0 + 1))),
      "e": bool(np.any(w1 - w0 >= 2)),
      "f": bool(np.any(cross & (per > 1))),
      "g": bool(np.any(cross & (per > 8))),
      "h": bool(np.any(cross & (per > 16))),
      "i": n % win != 0,
      "j": n % win == 0,
  }
  return {c for c, v in has.items() if v}
