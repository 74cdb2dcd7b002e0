"""Measurements of the fused-layout packer: distribution_ops.sharding_sparse_fids against the
composition a caller had to write before the op existed, and one PartitionedHashTable step; one JSON object per
line (sharding_fids.jsonl) and a markdown table (sharding_fids_table.md) under profiles/sharding_fids/ (or --out).

Shape: 26 features of 65 536 rows, one Zipf id per row (1 703 936 ids), 13 features per table, num_ps 8 and 64,
both ``unique`` modes.  Both sides end with fid_offset on the device and one id list per (table, shard); the op
also leaves feature_offset, nfl_offset and every list's row_splits, which the composition does not build.

The composition, per feature: ``unique_key_with_value_and_offset`` (unique mode: the distinct ids in
first-occurrence order and every occurrence's place), ``ragged_split_by_indices`` of the shard ``id % num_ps`` (the
per-shard lists and the original positions), then torch indexing: the ranks scattered back through the positions,
``(pre_output_index + shard * table_feature_count + feature_in_table_index) << 32 | rank``, gathered through the
inverse; at the end ``torch.cat`` of fid_offset over the features and of every (table, shard)'s lists.

Timing: device events around a window of back-to-back calls that lasts at least 0.5 s (--window), after warm-up;
the op and the composition take turns, case by case, and the whole round is repeated three times: a figure is the
median of the three windows, the spread their (max - min) / median.  There is no fallback: without a GPU the script
fails.
    python scripts/sharding_fids_bench.py [--out DIR] [--rows N] [--window S]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F, TABLES, DIM = 26, 2, 16


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                "profiles", "sharding_fids"))
  ap.add_argument("--rows", type=int, default=65536)
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  args = ap.parse_args()

  import numpy as np
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("sharding_fids_bench.py needs the MI355X: there is no fallback")
  from monolith_amd import PartitionedHashTable, entry, synthetic
  from monolith_amd import distribution_ops as D
  from monolith_amd.multi_hash_table_ops import Ragged

  B = args.rows
  names = ["f%02d" % i for i in range(F)]
  per = F // TABLES
  table_of = {n: "t%d" % (i // per) for i, n in enumerate(names)}
  cfgs = D.FeatureConfigs(
      {n: D.FeatureConfig(table_of[n], D.PoolingType.SUM, [DIM]) for n in names},
      {"vec": D.OutConfig([D.SliceConfig(n, 0, DIM) for n in names], D.OutType.CONCAT, [[-1, F * DIM]])})
  rs = np.arange(B + 1, dtype=np.int64)
  rs_dev = torch.from_numpy(rs).cuda()
  ids = {n: torch.from_numpy(synthetic.id_batch(40 + i, B, 10 ** 6, "zipf", feature_slot=i + 1)).cuda()
         for i, n in enumerate(names)}
  feats = {n: (ids[n], rs_dev) for n in names}
  one = np.array([0, B], dtype=np.int64)

  def compose(num_ps, unique):
    fid_offset, lists = [], [[] for _ in range(TABLES * num_ps)]
    for i, n in enumerate(names):
      t, j = i // per, i % per
      x = ids[n]
      if unique:
        r = D.unique_key_with_value_and_offset(Ragged(x, one), [1], generate_buffer=False)
        keys = r.unique_key.values
        counts = r.value_offset_split[1:] - r.value_offset_split[:-1]
        inverse = torch.empty(B, dtype=torch.int64, device="cuda")
        inverse[r.value_offset] = torch.repeat_interleave(torch.arange(keys.numel(), device="cuda"), counts)
      else:
        keys, inverse = x, None
      shard = torch.remainder(keys, num_ps)
      split, pos = D.ragged_split_by_indices(shard, Ragged(keys, np.array([0, keys.numel()], dtype=np.int64)), num_ps)
      rank = torch.empty(keys.numel(), dtype=torch.int64, device="cuda")
      rank[torch.cat([p.values for p in pos])] = torch.cat(
          [torch.arange(p.values.numel(), device="cuda") for p in pos])
      fo = ((t * per * num_ps + j + shard * per) << 32) | rank
      fid_offset.append(fo if inverse is None else fo[inverse])
      for s in range(num_ps):
        lists[t * num_ps + s].append(split[s].values)
    return torch.cat(fid_offset), [torch.cat(x) for x in lists]

  def window(fn):
    """seconds per call over a window of at least args.window seconds"""
    for _ in range(3):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def span(k):
      e0.record()
      for _ in range(k):
        fn()
      e1.record()
      e1.synchronize()
      return e0.elapsed_time(e1) * 1e-3

    per_call = span(3) / 3
    k = max(3, int(math.ceil(args.window / max(per_call, 1e-7))))
    return span(k) / k, k

  cases = []
  for num_ps in (8, 64):
    for unique in (True, False):
      cases.append((num_ps, unique,
                    lambda num_ps=num_ps, unique=unique: D.sharding_sparse_fids(feats, cfgs, num_ps, unique=unique),
                    lambda num_ps=num_ps, unique=unique: compose(num_ps, unique)))
  # both sides compute the same thing
  for num_ps, unique, ours, theirs in cases:
    a, (fo, lists) = ours(), theirs()
    assert torch.equal(a.fid_offset.view(torch.int64), fo), (num_ps, unique)
    assert all(torch.equal(x, y) for x, y in zip(a.fid_list, lists)), (num_ps, unique)
  del a, fo, lists

  times = {}
  for _ in range(args.repeats):
    for num_ps, unique, ours, theirs in cases:
      for who, fn in (("op", ours), ("composition", theirs)):
        times.setdefault((num_ps, unique, who), []).append(window(fn))

  def figure(ts):
    med = statistics.median(t for t, _ in ts)
    return {"us": med * 1e6, "windows_us": [t * 1e6 for t, _ in ts], "calls_per_window": ts[0][1],
            "spread": (max(t for t, _ in ts) - min(t for t, _ in ts)) / med}

  os.makedirs(args.out, exist_ok=True)
  recs = []
  for num_ps, unique, _, _ in cases:
    rec = {"case": "sharding_sparse_fids", "num_ps": num_ps, "unique": unique, "features": F, "rows": B, "ids": F * B}
    for who in ("op", "composition"):
      rec[who] = figure(times[(num_ps, unique, who)])
    rec["composition_over_op"] = rec["composition"]["us"] / rec["op"]["us"]
    recs.append(rec)

  # ---- one PartitionedHashTable step: lookup + apply_gradients
  seg = lambda: entry.make_table_config(   # noqa: E731
      [entry.CombineAsSegment(DIM, entry.ZerosInitializer(), entry.AdagradOptimizer(0.01, 0.1))],
      entry.CuckooHashTableConfig())
  for num_ps in (8, 64):
    for unique in (True, False):
      pht = PartitionedHashTable(num_ps, {"t0": seg(), "t1": seg()}, cfgs, name_suffix="bench_%d_%d" % (num_ps, unique),
                                 unique=unique)
      grad = [torch.full((B, F * DIM), 0.01, dtype=torch.float32, device="cuda")]
      step = [0]

      def one_step(pht=pht, grad=grad, step=step):
        pht.lookup(feats)
        pht.apply_gradients(grad, global_step=step[0], req_time=1_700_000_000 + step[0])
        step[0] += 1

      ts = [window(one_step) for _ in range(args.repeats)]
      rec = {"case": "PartitionedHashTable.lookup + apply_gradients", "num_ps": num_ps, "unique": unique, "features": F,
             "rows": B, "ids": F * B, "dim": DIM, "op": figure(ts)}
      recs.append(rec)
      pht.close()

  with open(os.path.join(args.out, "sharding_fids.jsonl"), "w") as f:
    for rec in recs:
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
  with open(os.path.join(args.out, "sharding_fids_table.md"), "w") as f:
    f.write("| call | num_ps | unique | ids | op µs | spread | composition µs | spread | composition / op |\n")
    f.write("|---|---|---|---|---|---|---|---|---|\n")
    for r in recs:
      c = r.get("composition")
      f.write("| %s | %d | %s | %d | %.1f | %.1f %% | %s | %s | %s |\n" %
              (r["case"], r["num_ps"], r["unique"], r["ids"], r["op"]["us"], 100 * r["op"]["spread"],
               "%.1f" % c["us"] if c else "-", "%.1f %%" % (100 * c["spread"]) if c else "-",
               "%.2fx" % r["composition_over_op"] if c else "-"))


if __name__ == "__main__":
  main()
