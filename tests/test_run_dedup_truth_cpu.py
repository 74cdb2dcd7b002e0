"""The coverage conditions of the batches tests/test_run_dedup_forms_gpu.py runs (tests/run_dedup_truth.py):
every case has the property it is named for, through the plain model ``workgroup_runs``, on every seed of
its pipeline.  A failure here means the INPUTS no longer reach an edge of the run dedup, not that a kernel
is wrong.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dedup_truth as T  # noqa: E402
import run_dedup_truth as R  # noqa: E402

ALL_QUARTERS = [0, 1, 2, 3]


def _pipeline(name):
  """(ids, runs) of every batch of the case's pipeline."""
  out = []
  for seed in R.pipeline_seeds(name):
    ids = R.build(name, seed)
    assert ids.dtype == np.int64 and ids.ndim == 1
    out.append((ids, R.workgroup_runs(ids)))
  return out


def _run_lengths(wg):
  return sorted(p.size for p in wg.values())


def _pad(split, nb):
  return list(split) + [0] * (nb - len(split))


# ---------------------------------------------------------------------------------------------- the model
def test_workgroup_runs_by_hand():
  ids = np.array([7, -3, 7] + [5] * 1021 + [7, R.INT64_MIN, 7, -3], np.int64)
  runs = R.workgroup_runs(ids)
  assert len(runs) == 2 and sorted(runs[0]) == [-3, 5, 7] and sorted(runs[1]) == [R.INT64_MIN, -3, 7]
  assert runs[0][7].tolist() == [0, 2] and runs[0][-3].tolist() == [1]
  assert runs[0][5].tolist() == list(range(3, 1024))
  assert runs[1][7].tolist() == [0, 2] and runs[1][R.INT64_MIN].tolist() == [1] and runs[1][-3].tolist() == [3]
  assert R.totals(ids) == {7: 4, -3: 2, 5: 1021, R.INT64_MIN: 1}
  assert R.light(ids) == {7: True, -3: True, 5: False, R.INT64_MIN: True}
  assert R.split_of(7, runs) == [2, 2] and R.split_of(5, runs) == [1021, 0]
  uids, inverse, seg_off, seg_pos = R.unique_first_occurrence(ids)
  assert uids.tolist() == [7, -3, 5, R.INT64_MIN]
  assert seg_off.tolist() == [0, 4, 6, 1027, 1028]
  assert seg_pos[:6].tolist() == [0, 2, 1024, 1026, 1, 1027] and seg_pos[-1] == 1025
  assert inverse[[0, 1, 3, 1025]].tolist() == [0, 1, 2, 3]
  assert R.quarters_of([0, 255, 256, 1023]) == [0, 1, 3]
  assert [R.last_workgroup_quarters(n) for n in (1, 256, 257, 1024, 1025, 1279, 1281, 1793, 2048)] == \
      [1, 1, 2, 4, 1, 1, 2, 4, 4]


def test_the_constants_are_the_kernels():
  """The table at the top of run_dedup_truth.py against csrc/mhte_step_kernels.h and mhte_kernels.h."""
  import re
  csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "monolith_amd", "csrc")
  text = ""
  for f in ("mhte_step_kernels.h", "mhte_kernels.h"):
    with open(os.path.join(csrc, f)) as fh:
      text += fh.read()
  def const(name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return m.group(1).strip()
  assert int(const("kRdBlock")) == R.RD_BLOCK
  assert int(const("kRd4Threads")) == R.RD4_THREADS
  assert int(const("kRdLds")) == R.RD_LDS
  assert int(const("kStepLightMax")) == R.LIGHT_MAX and int(const("kLightMax")) == R.LIGHT_MAX
  assert const("kLongRun") == "kLightMax"
  assert int(const("kMaxLongRuns")) == R.MAX_LONG_RUNS
  assert int(const("kItemTarget")) == R.ITEM_TARGET
  assert int(const("kRdMaxBlocks")) == R.RD_MAX_BLOCKS


def test_the_registry_holds_every_case_of_the_families():
  assert len(R.names("size")) == len(R.SIZE_EDGES) * len(R.PATTERNS) + 3
  assert len(R.names("run")) == len(R.RUN_LENGTHS) * len(R.LAYOUTS) == 33
  assert R.names("long") == ["long-16x33", "long-17x33", "long-31x33"]
  assert len(R.names("lds")) == 2 and len(R.names("reserved")) == 6 and len(R.names("edge")) == 12
  assert len(R.CASES) == sum(len(R.names(f)) for f in ("size", "run", "long", "lds", "reserved", "edge"))
  # only the 64-workgroup shapes and the lists of one occurrence in each of 32 / 33 / 64 workgroups (which
  # need that many workgroups) are larger than dedup_truth's 300 x 33
  big = {k for k in R.CASES if R.build(k, 1).size > T.HEAVY_N}
  assert big == {"size-one-id-and-a-single-65535", "size-one-id-and-a-single-65536", "size-distinct-64513",
                 "reserved-33-singles", "edge-32=1x32", "edge-64=1x64"}


# ----------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", list(R.CASES))
def test_first_occurrence_model_agrees_and_seeds_differ(name):
  pipe = _pipeline(name)
  assert len(pipe) == R.PIPELINE and len({ids.size for ids, _ in pipe}) == 1
  for ids, runs in pipe:
    for got, exp in zip(R.unique_first_occurrence(ids, runs), T.unique_first_occurrence(ids)):
      np.testing.assert_array_equal(got, exp)
  # (other ids in every batch — the reserved literals apart)
  first = [ids[~np.isin(ids, R.RESERVED_KEYS)] for ids, _ in pipe]
  for a, b in zip(first, first[1:]):
    assert a.size == 0 or not np.isin(a, b).any()


# -------------------------------------------------------------------------------------------------- size edges
@pytest.mark.parametrize("n", R.SIZE_EDGES)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_size_edges(pattern, n):
  for ids, runs in _pipeline("size-%s-%d" % (pattern, n)):
    nb = (n + 1023) // 1024
    assert ids.size == n and len(runs) == nb
    sizes = [min(1024, n - 1024 * b) for b in range(nb)]
    for wg, sz in zip(runs, sizes):
      if pattern == "equal":
        assert _run_lengths(wg) == [sz]
      elif pattern == "distinct":
        assert _run_lengths(wg) == [1] * sz
      else:
        assert _run_lengths(wg) == ([sz // 2, sz - sz // 2] if sz > 1 else [1])
    # the quarters of the 256-thread form that hold a valid position in the last workgroup
    last = np.concatenate(list(runs[-1].values()))
    assert len(R.quarters_of(last)) == R.last_workgroup_quarters(n)
  assert [R.last_workgroup_quarters(n) for n in (1279, 1281, 1793)] == [1, 2, 4]
  assert 1793 - 1024 == 3 * 256 + 1      # ... exactly four: one position in the fourth


@pytest.mark.parametrize("n", [65535, 65536])
def test_size_edge_of_64_workgroups_one_id_everywhere(n):
  for ids, runs in _pipeline("size-one-id-and-a-single-%d" % n):
    assert ids.size == n and len(runs) == R.RD_MAX_BLOCKS
    assert all(_run_lengths(wg) == [1024] for wg in runs[:-1])        # the 11-bit count field, 63 times
    assert _run_lengths(runs[-1]) == [1, n - 63 * 1024 - 1]
    single = [k for k, p in runs[-1].items() if p.size == 1][0]
    assert runs[-1][single].tolist() == [n - 63 * 1024 - 1]           # the very last position
    assert sorted(R.totals(ids, runs).values()) == [1, n - 1]


def test_size_edge_of_63_workgroups_and_one_position():
  for ids, runs in _pipeline("size-distinct-64513"):
    assert ids.size == 63 * 1024 + 1 and len(runs) == R.RD_MAX_BLOCKS
    assert [len(wg) for wg in runs] == [1024] * 63 + [1]
    assert np.unique(ids).size == ids.size


# ------------------------------------------------------------------------------------- run length in a workgroup
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("length", R.RUN_LENGTHS)
def test_run_length_in_one_workgroup(length, layout):
  for ids, runs in _pipeline("run-%d-%s" % (length, layout)):
    assert ids.size == R.RUN_N and len(runs) == 2
    assert _run_lengths(runs[0]) == [1] * 1024
    wg = runs[R.RUN_WG]
    assert _run_lengths(wg) == [1] * (1024 - length) + [length]
    if length == 1:
      continue
    key, pos = [(k, p) for k, p in wg.items() if p.size == length][0]
    assert R.split_of(key, runs) == [0, length]
    assert R.light(ids, runs)[key] == (length <= 32)
    if layout == "runs":
      np.testing.assert_array_equal(np.diff(pos), 1)
    else:   # in all four quarters: every one of a thread's four positions takes part in the run
      assert R.quarters_of(pos) == (ALL_QUARTERS if length >= 4 else R.quarters_of(pos)[:2])
      assert len(R.quarters_of(pos)) == min(length, 4)
      assert (np.diff(pos) > 1).any() or length >= 1023    # (not adjacent, where there is room not to be)


# -------------------------------------------------------------------------------------------- long-run slots
@pytest.mark.parametrize("k", [16, 17, 31])
def test_long_run_slots(k):
  for ids, runs in _pipeline("long-%dx33" % k):
    assert ids.size == R.RUN_N and _run_lengths(runs[0]) == [1] * 1024
    wg = runs[R.RUN_WG]
    long_runs = [p for p in wg.values() if p.size > R.LONG_RUN]
    assert len(long_runs) == k and all(p.size == 33 for p in long_runs)
    assert _run_lengths(wg) == [1] * (1024 - 33 * k) + [33] * k
    assert all(len(R.quarters_of(p)) > 1 and (np.diff(p) > 1).any() for p in long_runs)   # shuffled
  assert (16 <= R.MAX_LONG_RUNS) and (17 > R.MAX_LONG_RUNS) and 1024 - 33 * 31 == 1


# ---------------------------------------------------------------------------------------------- LDS set fill
@pytest.mark.parametrize("with_reserved", [False, True])
def test_lds_set_at_half_load(with_reserved):
  name = "lds-1023-distinct-and-min" if with_reserved else "lds-1024-distinct"
  for ids, runs in _pipeline(name):
    assert len(runs) == 3 and [len(wg) for wg in runs] == [1024] * 3 and 2 * 1024 == R.RD_LDS
    if with_reserved:
      assert R.split_of(R.INT64_MIN, runs) == [1, 1, 1]
      assert np.unique(ids).size == 3 * 1023 + 1
    else:
      assert np.unique(ids).size == 3 * 1024 and R.INT64_MIN not in R.totals(ids, runs)


# --------------------------------------------------------------------------------------------- reserved key
@pytest.mark.parametrize("kind", list(R.RESERVED))
def test_reserved_key(kind):
  splits, n = R.RESERVED[kind]
  for ids, runs in _pipeline("reserved-%s" % kind):
    assert ids.size == n
    tot = R.totals(ids, runs)
    for key, split in zip(R.RESERVED_KEYS, splits):
      assert R.split_of(key, runs) == _pad(split, len(runs))
    assert sorted(c for c in tot.values() if c > 1) == sorted(sum(s) for s in splits if sum(s) > 1)
    assert tot[R.INT64_MIN] == {"once": 1, "run32": 32, "run33": 33, "workgroup": 1024, "33-singles": 33,
                                "with-0-and-max": 33}[kind]
    if kind == "33-singles":
      assert len(runs) == 33 and not R.light(ids, runs)[R.INT64_MIN]
    if kind == "workgroup":
      assert list(runs[1]) == [R.INT64_MIN]
    if kind == "with-0-and-max":
      assert tot[0] == 5 and tot[R.INT64_MAX] == 40
      assert R.light(ids, runs)[0] and not R.light(ids, runs)[R.INT64_MIN] and not R.light(ids, runs)[R.INT64_MAX]


# -------------------------------------------------------------------------- lists at the light / heavy edge
@pytest.mark.parametrize("kind", list(R.EDGE))
def test_lists_across_workgroups(kind):
  splits, n = R.EDGE[kind]
  want = {"32=16+16": (32, [16, 16]), "32=31+1": (32, [31, 1]), "32=1x32": (32, [1] * 32),
          "33=32+1": (33, [32, 1]), "33=17+16": (33, [17, 16]), "40=20+20": (40, [20, 20]),
          "256-in-one": (256, [0, 256]), "257-in-one": (257, [0, 257]), "256-over-8": (256, [32] * 8),
          "257-over-8": (257, [32] * 7 + [33]), "64=1x64": (64, [1] * 64)}[kind]
  assert (sum(splits[0]), splits[0]) == want
  for ids, runs in _pipeline("edge-%s" % kind):
    assert ids.size == n and len(runs) == len(splits[0])
    key = R.edge_key(ids, kind)
    assert R.split_of(key, runs) == want[1]
    assert R.light(ids, runs)[key] == (want[0] <= 32)
    assert sorted(R.totals(ids, runs).values())[-2:] == [1, want[0]]     # every other id occurs once
    for b, c in enumerate(want[1]):      # a run of four or more in a whole workgroup: in all four quarters
      if c >= 4 and len(runs[b]) + c - 1 == 1024:
        assert R.quarters_of(runs[b][key]) == ALL_QUARTERS


def test_300_heavy_lists_of_33():
  for ids, runs in _pipeline("edge-300x33"):
    assert ids.size == T.HEAVY_N == 9900
    assert sorted(R.totals(ids, runs).values()) == [33] * 300
    assert max(p.size for wg in runs for p in wg.values()) <= R.LONG_RUN   # short runs of heavy lists
    assert all(min(R.split_of(k, runs)) >= 1 for k in runs[0])              # every list in every workgroup
