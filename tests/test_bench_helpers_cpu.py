"""CPU suite: the host-side helpers of bench.py that decide something about the measured run."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
  spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
  m = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(m)
  return m


def test_peer_unique_max_counts_distinct_ids_per_owner():
  b = _bench()
  ids = np.array([[8, 8, 16, 1, 9, 9, 9, 3],      # owner 0: {8, 16}; owner 1: {1, 9}; owner 3: {3}
                  [5, 5, 5, 5, 13, 21, 29, 2]],   # owner 1: {5, 13, 21, 29}; owner 2: {2}
                 dtype=np.int64)
  assert b.peer_unique_max(ids, 4) == 4
  assert b.peer_unique_max(ids[:1], 4) == 2
  assert b.peer_unique_max(ids, 1) == 5            # one owner: distinct ids of the larger batch


def test_algorithmic_bytes_follow_the_survey_formula():
  """bytes_lookup + bytes_update with P = 72, checked on the closed form at U = B."""
  b = _bench()
  B, D = 65536, 32
  step, per_kernel = b.algorithmic_bytes(B, B, D, 0)   # SGD: no optimizer state
  assert step == B * (16 + 20 * D + 2 * 72 + 4)        # 804 B per id pair at D = 32
  assert per_kernel["sum_apply_kernel"] == B * (8 + 4 * D + 72 + 8 * D + 4)
  assert per_kernel["lookup_kernel"] + per_kernel["sum_apply_kernel"] == step
  step, _ = b.algorithmic_bytes(B, B, 64, 64)          # Adagrad, D = 64: 1 956 B per id pair
  assert step == B * 1956


def test_a_plain_run_leaves_everything_beyond_the_headline_to_full(monkeypatch):
  b = _bench()
  monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
  a = b.parse()
  assert (a.steps, a.warmup, a.full, a.dump_outputs) == (20, 5, False, "")
  assert a.no_cpu_baseline and a.no_extra_windows and a.no_parity_check and a.no_stage_timing
  monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
  a = b.parse()
  assert not (a.no_cpu_baseline or a.no_extra_windows or a.no_parity_check or a.no_stage_timing)


def test_dumped_outputs_are_float32_whole_rows_of_a_fixed_sample_within_the_limit():
  import torch
  b = _bench()
  arrays = {"a": torch.arange(4096 * 16, dtype=torch.float32).view(4096, 16), "b": torch.ones(1024, 8)}
  limit = 64 << 10
  o1, o2 = b.take_outputs(arrays, limit), b.take_outputs(arrays, limit)
  assert sum(x.nbytes for x in o1.values()) <= limit
  assert all(x.dtype == np.float32 for x in o1.values())
  assert all(np.array_equal(o1[k], o2[k]) for k in arrays)
  rows = o1["a"][:, 0] // 16                        # whole rows, in their original order
  assert np.array_equal(o1["a"], arrays["a"].numpy()[rows.astype(np.int64)]) and np.all(np.diff(rows) > 0)
  assert b.take_outputs({"x": torch.ones(3, 4)})["x"].shape == (3, 4)   # under the limit: everything


def test_full_keeps_every_batch_fresh_unless_the_steps_alone_pass_the_ring():
  b = _bench()
  assert b.RING % 60 == 0                                      # whole graph chunks and dedup-slot turns
  # --full at the defaults (200 steps, 20 warm-up): every window and pass on batches of its own
  assert b.ring_size(1339, 200, True, b.RING) == 1339
  assert b.ring_size(7000, b.RING, True, b.RING) == 7000
  assert b.ring_size(9000, b.RING + 10, True, b.RING) == b.RING
  # a plain run: its own steps, at most the ring
  assert b.ring_size(244, 200, False, b.RING) == 244
  assert b.ring_size(20244, 20000, False, b.RING) == b.RING
  assert b.ring_size(275, 200, True, b.RING_DLRM) == 275     # dlrm26 --full at its defaults
  assert b.repeated_steps(221, 241, 1339) == 0
  assert b.repeated_steps(1000, 3000, 1440) == 1560
  assert b.repeated_steps(2000, 2100, 1440) == 100


def test_c_loop_stretches_cover_the_steps_in_order_and_never_read_past_the_ring():
  b = _bench()
  for P in (7, 60, 1440):
    for lo, hi in ((0, 5), (0, P - 1), (0, P), (3, 3 * P + 2), (P - 1, P + 1), (2 * P - 2, 5 * P)):
      seq = []
      for first, n in b.ring_stretches(lo, hi, P):
        if n is None:                         # one step enqueued by itself: the ring's last batch
          assert first == P - 1
          seq.append(first)
        else:                                 # the C loop reads batch first + n ahead: inside the ring
          assert n > 0 and first + n <= P - 1
          seq.extend(range(first, first + n))
      assert seq == [s % P for s in range(lo, hi)], (P, lo, hi)


def _slot_turn(lookahead, steps):
  """The dedup slots of fused_step.SparseStep's pipeline: the lowest slot free of the batches in flight takes
  the next one (lookahead 1: current + next; 2: + the one after).  -> the (cur, next) slots of every step."""
  free = lambda *busy: min(i for i in range(3) if i not in busy)   # noqa: E731
  cur, nxt = 0, None
  seen = []
  for _ in range(steps):
    if lookahead == 1:
      nxt = free(cur)
    elif nxt is None:
      nxt = free(cur)
    seen.append((cur, nxt))
    if lookahead == 2:
      ahead = free(cur, nxt)
      cur, nxt = nxt, ahead
    else:
      cur, nxt = nxt, None
  return seen


def test_a_lap_of_graphs_returns_to_the_dedup_slots_it_was_captured_from():
  """capture() replays one lap of RING steps over and over: the slot rotation must have come round."""
  b = _bench()
  for la in (1, 2):
    seen = _slot_turn(la, 2 * b.RING + 5)
    assert seen[b.RING:2 * b.RING] == seen[:b.RING], la
