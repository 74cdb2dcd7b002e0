"""Measurements of table compaction, one JSON object per line and a markdown table under
profiles/compact/ (or --out DIR): one table, dim 64 Adagrad (512-byte rows), 2^22 rows whose ids alternate
between two feature slots with TTLs of 5 and 6 days, so that one eviction scan drops every other row:

  * the compaction itself, by events around the call (it contains two host waits: the tile counts come
    back for the scans, and the stream drains before the slabs are freed), with its algorithmic bytes —
    the bucket array twice + the bitmap + 2 x moved rows x 512 B — and the fraction of the 8 TB/s HBM peak;
  * the pipelined step (SparseStep, 65 536 ids per batch, ids drawn from the rows that survive) on one
    fixed batch stream: before the eviction, after it, and after the compaction — the last shows whether
    rows that came back into slab 0 (addressed without the slab-table load) are visible.

A compaction can be timed once per table state, so every round builds its table again; figures are
medians over the rounds.
    python scripts/compact_bench.py [--out DIR] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monolith_amd import entry, synthetic as S  # noqa: E402
from monolith_amd.fused_step import SparseStep  # noqa: E402
from monolith_amd.multi_hash_table_ops import MultiHashTable  # noqa: E402

PEAK = 8e12
DIM, ROW_BYTES, B = 64, 512, 65536
DAY, T0 = 86400, 1_600_000_000


def build(rows, tag):
  cfg = entry.make_table_config(
      [entry.CombineAsSegment(DIM, entry.ZerosInitializer(), entry.AdagradOptimizer(0.01, 0.1))],
      entry.CuckooHashTableConfig(initial_capacity=2 * rows),
      slot_expire_time_config=entry.SlotExpireTimeConfig(14, {1: 5, 2: 6}))
  mt = MultiHashTable.from_configs({"emb": cfg}, name_suffix="compact_bench_%s" % tag)
  k = np.arange(rows, dtype=np.int64)
  ids = ((1 + (k & 1)) << 48) | (1000 + k)
  chunk = 1 << 18
  g = torch.full((chunk, DIM), 0.01, dtype=torch.float32, device="cuda")
  for lo in range(0, rows, chunk):
    part = torch.from_numpy(ids[lo:lo + chunk]).cuda()
    mt.apply_gradients({"emb": (part, g[:part.numel()])}, req_time=T0, ids_unique=True)
  return mt, ids


def step_time(mt, batches, grads, steps, warmup):
  """Mean time of one pipelined step (forward | next batch's dedup, backward) by events, in seconds."""
  step = SparseStep(mt, "emb", B)
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  n = len(batches) - 1
  for s_ in range(warmup + steps):
    if s_ == warmup:
      ev[0].record()
    step.forward(batches[s_ % n], next_ids=batches[s_ % n + 1])
    step.backward(grads, T0 + 1 + s_)
  ev[1].record()
  torch.cuda.synchronize()
  step.quiesce()
  return ev[0].elapsed_time(ev[1]) * 1e-3 / steps


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "profiles", "compact"))
  p.add_argument("--quick", action="store_true")
  a = p.parse_args()
  torch.cuda.set_device(0)
  rows = 1 << (20 if a.quick else 22)
  rounds, steps, warmup = (2, 20, 5) if a.quick else (3, 100, 10)
  runs = {"compact": [], "step before eviction": [], "step after eviction": [], "step after compaction": []}
  info = {}
  grads = torch.from_numpy(S.grad_batch(0, B, DIM)).cuda()
  for r in range(rounds):
    mt, ids = build(rows, r)
    rng = np.random.default_rng(r)
    keep = ids[1::2]       # slot 2: survives the scan
    batches = [torch.from_numpy(rng.choice(keep, B)).cuda() for _ in range(9)]
    runs["step before eviction"].append(step_time(mt, batches, grads, steps, warmup))
    mt.evict("emb", T0 + 5 * DAY + 60)
    st0 = mt.stats("emb")
    assert st0.size == keep.size, (st0.size, keep.size)
    runs["step after eviction"].append(step_time(mt, batches, grads, steps, warmup))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    res = mt.compact("emb")
    ev[1].record()
    torch.cuda.synchronize()
    runs["compact"].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    st1 = mt.stats("emb")
    assert st1.rows_allocated == st1.size == keep.size
    runs["step after compaction"].append(step_time(mt, batches, grads, steps, warmup))
    info = dict(res, buckets=1 << st1.hashpower, bytes_rows_before=st0.bytes_rows, bytes_rows_after=st1.bytes_rows)
    mt.close()
  alg = 2 * 64 * info["buckets"] + info["rows_after"] // 8 + 2 * info["rows_moved"] * ROW_BYTES
  lines = []
  for name, xs in runs.items():
    med = statistics.median(xs)
    rec = {"name": name, "us": round(med * 1e6, 1), "us_rounds": [round(x * 1e6, 1) for x in xs]}
    if name == "compact":
      rec.update(alg_bytes=alg, GBps=round(alg / med / 1e9, 1), peak_fraction=round(alg / med / PEAK, 4), **info)
    lines.append(rec)
    print(json.dumps(rec), flush=True)
  os.makedirs(a.out, exist_ok=True)
  with open(os.path.join(a.out, "compact.jsonl"), "w") as f:
    for rec in lines:
      f.write(json.dumps(rec) + "\n")
  with open(os.path.join(a.out, "compact.md"), "w") as f:
    f.write("# Table compaction (one MI355X)\n\n"
            "One table, dim 64 Adagrad (512-byte rows), %d rows, every other one evicted; %d rounds, each on a "
            "table built anew; medians.  The compaction is timed by events around the call and contains its two "
            "host waits.  Steps: SparseStep, %d ids per batch drawn from the surviving rows, %d steps after %d "
            "of warm-up.\n\n" % (rows, rounds, B, steps, warmup))
    c = lines[0]
    f.write("Compaction: %d handles in use -> %d, %d rows moved, %d bytes of slabs released (%d -> %d), %d buckets.  "
            "Algorithmic bytes %d (bucket array twice + bitmap + 2 x moved rows x 512 B).\n\n"
            % (c["rows_before"], c["rows_after"], c["rows_moved"], c["bytes_released"], c["bytes_rows_before"],
               c["bytes_rows_after"], c["buckets"], c["alg_bytes"]))
    f.write("| case | µs | GB/s | of 8 TB/s | rounds (µs) |\n|---|---|---|---|---|\n")
    for rec in lines:
      f.write("| %s | %s | %s | %s | %s |\n" % (
          rec["name"], rec["us"], rec.get("GBps", ""),
          ("%.2f %%" % (100 * rec["peak_fraction"])) if "peak_fraction" in rec else "", rec["us_rounds"]))


if __name__ == "__main__":
  main()
