"""The coverage conditions of the batches tests/test_multi_step_forms_gpu.py runs (tests/multi_step_truth.py):
every ``cut`` case has the list length and the per-workgroup split it is named for and lies on the side of its
edge of ``rd_item_blocks`` that its name says, and the deal of cases to tables has the properties the item-to-table
mapping of the dedup launches is tested through.  A failure here means the INPUTS no longer reach an edge, not
that a kernel is wrong.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multi_step_truth as M  # noqa: E402
import run_dedup_truth as R  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "monolith_amd", "csrc")


def _text(name):
  with open(os.path.join(CSRC, name)) as fh:
    return fh.read()


# --------------------------------------------------------------------------------------------- the mirror
def test_item_blocks_by_hand():
  """``rd_item_blocks`` worked out from its text (csrc/mhte_step_kernels.h) for both targets."""
  for target in M.ITEM_TARGETS:
    t = target
    assert [M.item_blocks(c, t) for c in (33, t, 2 * t)] == [64, 64, 64]
    assert [M.item_blocks(c, t) for c in (2 * t + 1, 4 * t)] == [16, 16]
    assert [M.item_blocks(c, t) for c in (4 * t + 1, 8 * t)] == [8, 8]
    assert [M.item_blocks(c, t) for c in (8 * t + 1, 16 * t, 16 * t + 1, 32 * t + 1, 64 * t, 64 * t + 1)] == \
        [4, 4, 2, 1, 1, 1]
  # a list in 33 workgroups: whole, cut in three, cut in five (the ranges are aligned to their size)
  assert M.items_of([16] * 32, 256) == (64, [512])
  assert M.items_of([16] * 32 + [1], 256) == (16, [256, 256, 1])
  assert M.items_of([32] * 32, 256) == (16, [512, 512])
  assert M.items_of([32] * 32 + [1], 256) == (8, [256] * 4 + [1])
  assert M.items_of([0, 5, 0, 0, 0, 0, 0, 0, 0] + [0] * 8 + [600], 256) == (16, [5, 600])   # an empty range: no item
  # the rows 255 | 256 | 257 of the single-table suite are no edge of the cut
  assert {M.item_blocks(c, 256) for c in (255, 256, 257)} == {64}


def test_the_mirror_is_the_kernel_and_the_host_plan():
  text = _text("mhte_step_kernels.h")
  m = re.search(r"uint32_t rd_item_blocks\(uint32_t c, uint32_t target\) \{(.*?)\n\}", text, re.S)
  assert m, "rd_item_blocks"
  body = " ".join(m.group(1).split())
  assert "uint32_t nbk = 64;" in body
  assert "uint64_t(target) * 64 * (c > 2 * target ? 1 : 2)" in body
  assert "while (nbk > 1 && uint64_t(c) * nbk > lim) nbk >>= 1;" in body
  host = _text("mhte_mstep_host.h")
  assert "item_target = T >= 4 ? 4 * kItemTarget : kItemTarget;" in host
  assert "A.item_split = std::max<uint32_t>(1, item_target / kItemTarget);" in host
  assert [M.item_target(t) for t in (1, 3, 4, 5, 34)] == [256, 256, 1024, 1024, 1024]
  assert [M.item_split(t) for t in M.ITEM_TARGETS] == [1, 4]
  assert int(re.search(r"constexpr int kMaxStepTables = (\d+);", _text("mhte_mstep_kernels.h")).group(1)) == 32


# ------------------------------------------------------------------------------------------- the cut family
def test_the_registry():
  assert list(M.CUT) == ["cut-t256-512", "cut-t256-513", "cut-t256-1024", "cut-t256-1025",
                         "cut-t1024-2048", "cut-t1024-2049", "cut-t1024-4096", "cut-t1024-4097"]
  assert list(M.ALL)[:len(R.CASES)] == list(R.CASES) and len(M.ALL) == len(R.CASES) + 8
  assert not set(M.CUT) & set(R.CASES)
  seeds = [s for k in M.ALL for s in M.pipeline_seeds(k)]
  assert len(seeds) == len(set(seeds)) == R.PIPELINE * len(M.ALL)
  for k in R.CASES:
    assert M.pipeline_seeds(k) == R.pipeline_seeds(k)
  assert sorted(M.form_cases() + M.other_cases()) == sorted(M.ALL)
  assert len(M.form_cases()) == 12 + 6 + 3 + 8 + 9 + 18
  big = {"size-one-id-and-a-single-65535", "size-one-id-and-a-single-65536", "size-distinct-64513"}
  assert big <= set(M.other_cases())
  assert max(M.size_of(k) for k in M.ALL) == R.RD_MAX_BLOCKS * R.RD_BLOCK


@pytest.mark.parametrize("target,c", M.CUT_LENGTHS)
def test_cut_case_lies_on_its_side_of_the_edge(target, c):
  name = M.cut_name(target, c)
  whole = c % 2 == 0
  per_wg = (c - c % 2) // M.CUT_WGS
  assert c in (2 * target, 2 * target + 1, 4 * target, 4 * target + 1)
  for seed in M.pipeline_seeds(name):
    ids = M.build(name, seed)
    runs = R.workgroup_runs(ids)
    assert ids.size == M.CUT_N == 33000 and len(runs) == M.CUT_WGS + 1
    key = M.cut_key(ids, c)
    split = R.split_of(key, runs)
    assert sum(split) == c                                                    # the length it is named for
    assert split == [per_wg] * M.CUT_WGS + [0 if whole else 1]               # ... and the split
    assert sorted(R.totals(ids, runs).values())[-2:] == [1, c]               # every other id occurs once
    # the mirrored cut of exactly this split, for the target the case is named for
    nbk, items = M.items_of(split, target)
    assert M.heavy_items(ids, target) == {key: (nbk, items)}
    if c == 2 * target:
      assert (nbk, items) == (64, [c])                                       # whole: a single item
    elif c == 2 * target + 1:
      assert (nbk, items) == (16, [target, target, 1])                       # cut: three non-empty items
    elif c == 4 * target:
      assert (nbk, items) == (16, [2 * target, 2 * target])
    else:
      assert (nbk, items) == (8, [target] * 4 + [1])
    assert len(items) <= 64 and max(items) <= 2 * target
    # moved one occurrence across its edge the case would be another one
    other = c + 1 if whole else c - 1
    assert M.item_blocks(other, target) != nbk
    assert M.items_of(M.cut_split(other), target) != (nbk, items)
    # runs of 16 and 32 positions (counting rank) and of 64 and 128 (bitmap rank) in every whole workgroup
    assert per_wg in (16, 32, 64, 128) and (per_wg > R.LONG_RUN) == (target == 1024)


@pytest.mark.parametrize("target", M.ITEM_TARGETS)
def test_the_two_sides_of_every_edge_differ(target):
  for lo in (2 * target, 4 * target):
    a = M.items_of(M.cut_split(lo), target)
    b = M.items_of(M.cut_split(lo + 1), target)
    assert a[0] > b[0] and len(a[1]) < len(b[1])
  # under the target of 1024 the lists cut for 256 are ordinary ones (no edge between them); under the target
  # of 256 those cut for 1024 lie on the next two edges, 8 | 4 and 4 | 2 workgroups per item
  if target == 256:
    assert {M.item_blocks(c, 1024) for c in (512, 513, 1024, 1025)} == {64}
  else:
    assert [M.item_blocks(c, 256) for c in (2048, 2049, 4096, 4097)] == [8, 4, 4, 2]


def test_heavy_lists_of_the_wide_model_take_fewer_than_four_passes():
  """``item_split`` = 4 wavefronts share an item, each taking every fourth pass of 64 occurrences: items of
  33 .. 255 occurrences leave one to three of the four without a pass, and E is no multiple of 64."""
  split4 = M.item_split(M.item_target(5))
  assert split4 == 4
  seen = set()
  for name in ("edge-33=32+1", "edge-40=20+20", "edge-64=1x64", "edge-257-in-one", "reserved-33-singles",
               "run-33-runs", "run-255-shuffled", "run-1024-strided"):
    ids = M.build(name, M.pipeline_seeds(name)[0])
    for nbk, items in M.heavy_items(ids, 1024).values():
      for e in items:
        seen.add(-(-e // M.HEAVY_ITEM_SPLIT_PASS))
  assert {1, 4, 5, 16} <= seen
  e64 = M.heavy_items(M.build("edge-64=1x64", 1), 1024)
  assert list(e64.values()) == [(64, [64])]            # 64 runs of one occurrence in ONE item
  e33 = M.heavy_items(M.build("reserved-33-singles", 1), 256)
  assert list(e33.values()) == [(64, [33])]


# --------------------------------------------------------------------------------------------------- the deal
DEALS = [(3, "form"), (3, "other"), (5, "form"), (5, "other"), (2, "form"), (3, "order")]


def _cases(which):
  return {"form": M.form_cases, "other": M.other_cases, "order": M.order_cases}[which]()


@pytest.mark.parametrize("n_tables,which", DEALS)
def test_deal_is_a_partition_with_different_sizes_side_by_side(n_tables, which):
  cases = _cases(which)
  groups = M.deal(cases, n_tables)
  assert all(len(g) == n_tables for g in groups)
  dealt = [k for g in groups for k in g]
  assert set(dealt) == set(cases)
  extra = len(dealt) - len(cases)
  assert 0 <= extra < n_tables                                        # (the last group filled up)
  assert sorted(dealt) == sorted(cases + sorted(cases, key=lambda k: (M.size_of(k), list(M.ALL).index(k)))[:extra])
  for g in groups:
    sizes = [M.size_of(k) for k in g]
    assert all(a != b for a, b in zip(sizes, sizes[1:])), g
  assert M.deal(cases, n_tables) == groups                              # deterministic


@pytest.mark.parametrize("n_tables,which", [(3, "form"), (5, "form"), (2, "form"), (3, "other"), (5, "other")])
def test_deal_reaches_the_item_to_table_mapping(n_tables, which):
  groups = M.deal(_cases(which), n_tables)
  # a table other than the last with a last block of 1, 255 and 1023 positions
  tails = {M.tail(M.size_of(k)) for g in groups for k in g[:-1]}
  if which == "form":
    assert set(M.TAIL_EDGES) <= tails
  # the emptied table: in the middle of ``blk_start`` (the first of the two case tables of the 34-table model,
  # which has 32 tables in front of it and one behind)
  hole = M.emptied_table(0, n_tables)
  assert hole == (n_tables // 2 if n_tables >= 3 else 0)
  assert n_tables < 3 or 0 < hole < n_tables - 1
  assert all(M.emptied_table(g, n_tables) is None for g in range(1, len(groups)))
  batches = M.deal_batches(groups[0], hole)
  assert len(batches) == R.PIPELINE
  for s, row in enumerate(batches):
    sizes = [ids.size for ids in row]
    starts = M.block_starts(sizes)
    if s in M.EMPTY_STEPS:
      assert sizes[hole] == 0 and starts[hole] == starts[hole + 1]      # zero blocks
      assert n_tables < 3 or (starts[hole] > 0 and starts[-1] > starts[hole + 1])   # ... in the middle
    else:
      assert sizes == [M.size_of(k) for k in groups[0]]
  assert M.EMPTY_STEPS == (1, 3)
  # a persistent workgroup walks items of different tables in turn: every group has more than one table with ids
  for g in groups:
    assert sum(M.size_of(k) > 0 for k in g) == n_tables


def test_model_groups_cover_every_case_once_per_model():
  for n_tables in (3, 5):
    groups = M.model_groups(n_tables)
    labels = [label for label, _, _, _ in groups]
    assert len(labels) == len(set(labels))
    every = {k for _, g, _, e in groups if e for k in g}
    rest = {k for _, g, _, e in groups if not e for k in g}
    assert every == set(M.form_cases()) and every | rest == set(M.ALL)
    assert [hole for _, _, hole, _ in groups].count(None) == len(groups) - 2
