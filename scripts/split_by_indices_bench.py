"""Measurements of the split-by-indices ops: distribution_ops.ragged_split_by_indices and
distribution_ops.split_by_indices (float32 rows of 16) against the torch composition a caller had to write before
the ops existed, one JSON object per line (split_by_indices.jsonl) and a markdown table
(split_by_indices_table.md) under profiles/split_by_indices/ (or --out DIR).

Shape: T = 26 tables of 65 536 ids each (1 703 936 ids), num_ps 8 and 64, the shard floormod(id, num_ps) of
random ids.  Both sides end where the reference's ops end: every split's values (and positions) on the device,
the sizes and the per-split row_splits on the host — so both sides wait for the device once per call.

The composition: a stable ``torch.sort`` of the shard indices (the permutation), ``bincount`` (the sizes),
``index_select`` (the rows), and for the ragged form one ``searchsorted`` of ``split * n + row_splits[t]`` in the
sorted ``shard * n + position`` keys (the boundaries of all splits at once), then ``.cpu()`` of sizes and table.

Timing: device events around a window of back-to-back calls that lasts at least 0.5 s (--window), after warm-up;
the op and the composition take turns, case by case, and the whole round is repeated three times: a figure is the
median of the three windows, the spread their (max - min) / median.  There is no fallback: without a GPU the
script fails.
    python scripts/split_by_indices_bench.py [--out DIR] [--per-table N] [--window S]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, DIM = 26, 16


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                "profiles", "split_by_indices"))
  ap.add_argument("--per-table", type=int, default=65536)
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  args = ap.parse_args()

  import numpy as np
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("split_by_indices_bench.py needs the MI355X: there is no fallback")
  from monolith_amd import distribution_ops as D
  from monolith_amd.multi_hash_table_ops import Ragged

  n = T * args.per_table
  g = torch.Generator(device="cuda").manual_seed(13)
  ids = torch.randint(0, 2 ** 62, (n,), device="cuda", generator=g, dtype=torch.int64)
  rows = torch.rand(n, DIM, device="cuda", generator=g)
  rs = np.arange(T + 1, dtype=np.int64) * args.per_table
  rs_dev = torch.from_numpy(rs).cuda()

  def compose_plan(index, num_ps):
    order = torch.sort(index, stable=True).indices
    sizes = torch.bincount(index, minlength=num_ps)
    return order, sizes

  def compose_ragged(index, num_ps):
    order, sizes = compose_plan(index, num_ps)
    vals = ids.index_select(0, order)
    off = torch.cumsum(sizes, 0) - sizes
    keys = index.index_select(0, order) * n + order
    queries = (torch.arange(num_ps, device="cuda").view(-1, 1) * n + rs_dev.view(1, -1)).reshape(-1)
    table = (torch.searchsorted(keys, queries).view(num_ps, -1) - off.view(-1, 1)).cpu().numpy()
    cuts = sizes.cpu().tolist()
    return ([Ragged(v, table[s]) for s, v in enumerate(torch.split(vals, cuts))],
            [Ragged(p, table[s]) for s, p in enumerate(torch.split(order, cuts))])

  def compose_split(index, num_ps):
    order, sizes = compose_plan(index, num_ps)
    return list(torch.split(rows.index_select(0, order), sizes.cpu().tolist()))

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

    per = span(3) / 3
    k = max(3, int(math.ceil(args.window / max(per, 1e-7))))
    return span(k) / k, k

  cases = []
  for num_ps in (8, 64):
    index = torch.remainder(ids, num_ps)
    cases.append(("ragged_split_by_indices", num_ps,
                  lambda index=index, num_ps=num_ps: D.ragged_split_by_indices(index, Ragged(ids, rs), num_ps),
                  lambda index=index, num_ps=num_ps: compose_ragged(index, num_ps)))
    cases.append(("split_by_indices", num_ps,
                  lambda index=index, num_ps=num_ps: D.split_by_indices(index, rows, num_ps),
                  lambda index=index, num_ps=num_ps: compose_split(index, num_ps)))

  # the op and the composition compute the same thing, bit for bit; the launches of one call of the op
  launches = {}
  for name, num_ps, ours, theirs in cases:
    before = D.split_launch_counts()
    a, b = ours(), theirs()
    after = D.split_launch_counts()
    launches[(name, num_ps)] = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if name == "split_by_indices":
      assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, num_ps)
    else:
      for xs, ys in zip(a, b):
        assert all(torch.equal(x.values, y.values) and np.array_equal(x.row_splits, y.row_splits)
                   for x, y in zip(xs, ys)), (name, num_ps)
  del a, b

  times = {}
  for _ in range(args.repeats):
    for name, num_ps, ours, theirs in cases:
      for who, fn in (("op", ours), ("composition", theirs)):
        t, k = window(fn)
        times.setdefault((name, num_ps, who), []).append((t, k))

  os.makedirs(args.out, exist_ok=True)
  recs = []
  with open(os.path.join(args.out, "split_by_indices.jsonl"), "w") as f:
    for name, num_ps, _, _ in cases:
      rec = {"case": name, "num_ps": num_ps, "tables": T, "ids": n, "row_floats": DIM if name == "split_by_indices" else 0,
             "op_launches": launches[(name, num_ps)]}
      for who in ("op", "composition"):
        ts = [t for t, _ in times[(name, num_ps, who)]]
        med = statistics.median(ts)
        rec[who] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts],
                    "calls_per_window": times[(name, num_ps, who)][0][1], "spread": (max(ts) - min(ts)) / med}
      rec["composition_over_op"] = rec["composition"]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      recs.append(rec)
  with open(os.path.join(args.out, "split_by_indices_table.md"), "w") as f:
    f.write("| call | num_ps | ids | op µs | spread | composition µs | spread | composition / op | op launches |\n")
    f.write("|---|---|---|---|---|---|---|---|---|\n")
    for r in recs:
      f.write("| %s | %d | %d | %.1f | %.1f %% | %.1f | %.1f %% | %.2fx | %s |\n" %
              (r["case"], r["num_ps"], r["ids"], r["op"]["us"], 100 * r["op"]["spread"], r["composition"]["us"],
               100 * r["composition"]["spread"], r["composition_over_op"],
               ", ".join("%s %d" % kv for kv in sorted(r["op_launches"].items()))))


if __name__ == "__main__":
  main()
