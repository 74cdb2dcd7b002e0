"""Measurements of the device-resident touched-key set, one JSON object per line and a
markdown table under profiles/touched_key_set/ (or --out DIR):

  * insert of 65 536 unique ids into an empty set and into a set holding 1 M keys, at the default capacity;
  * the same with a Zipf(1.2) batch (duplicates);
  * steal of 1 M keys;
  * SparseStep (dim 64, batch 65 536) and MultiSparseStep (26 tables of dims 16 / 32 / 64, 65 536 ids each,
    configs[4]'s shape) with and without a set attached.

There is no reference GPU figure for this op: each line states the per-call time and the achieved bytes/s
beside the kernels' algorithmic bytes (8 n for the ids + 2 x 16 n for the slots of an insert without a cut;
16 B x slots read and written + 12 B per key for a steal), nothing more.
    python scripts/touched_key_set_bench.py [--out DIR] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monolith_amd import entry, synthetic as S  # noqa: E402
from monolith_amd.fused_step import MultiSparseStep, SparseStep  # noqa: E402
from monolith_amd.multi_hash_table_ops import MultiHashTable  # noqa: E402
from monolith_amd.touched_key_set_ops import TouchedKeySet  # noqa: E402

LINES = []
B = 65536


def emit(name, seconds, alg_bytes=None, **kw):
  rec = {"name": name, "us": round(seconds * 1e6, 2)}
  if alg_bytes is not None:
    rec.update(alg_bytes=int(alg_bytes), GBps=round(alg_bytes / seconds / 1e9, 1))
  rec.update(kw)
  LINES.append(rec)
  print(json.dumps(rec), flush=True)


def timed(fn, reps):
  torch.cuda.synchronize()
  t = time.perf_counter()
  for _ in range(reps):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) / reps


def bench_set(quick):
  reps = 5 if quick else 20
  tks = TouchedKeySet(name_suffix="bench")   # default capacity: 16 M slots
  rng = np.random.default_rng(7)
  uniq = [torch.from_numpy((rng.permutation(1 << 22)[:B].astype(np.int64) + (k << 32)) | (1 << 48)).cuda()
          for k in range(reps + 2)]
  zipf = [torch.from_numpy(S.id_batch(k, B, 10**9, "zipf")).cuda() for k in range(reps + 2)]
  fill = torch.from_numpy((np.arange(1 << 20, dtype=np.int64) * 7919) | (1 << 50)).cuda()
  for label, batches in (("unique", uniq), ("zipf1.2", zipf)):
    for pre in (0, 1 << 20):
      tks.steal()
      if pre:
        tks.insert_async(fill)
      tks.insert_async(batches[-1])          # warm
      k = [0]

      def one():
        tks.insert_async(batches[k[0]])
        k[0] += 1
      dt = timed(one, reps)
      emit("insert_%s_into_%d" % (label, pre), dt, alg_bytes=B * (8 + 32), ids=B, set_size_after=tks.size)
  tks.steal()
  tks.insert_async(fill)
  n = tks.size
  slots = 1 << 24
  t = time.perf_counter()
  got = tks.steal()
  torch.cuda.synchronize()
  dt = time.perf_counter() - t
  emit("steal_%d_keys" % n, dt, alg_bytes=2 * 16 * slots + 12 * n, keys=int(got.numel()),
       note="includes the size read-back and the output allocation")
  tks.close()


def bench_single(quick):
  steps = 20 if quick else 100
  D = 64
  for attach in (False, True):
    cfg = entry.make_table_config([entry.CombineAsSegment(D, entry.ZerosInitializer(),
                                                          entry.AdagradOptimizer(0.001, 0.1))])
    mt = MultiHashTable.from_configs({"emb": cfg}, name_suffix="tkb_s%d" % attach)
    tks = TouchedKeySet(name_suffix="tkb_s%d" % attach, max_insert=B + 1) if attach else None
    if tks is not None:
      mt.set_touched_key_set(tks)
    step = SparseStep(mt, "emb", B)
    ring = [torch.from_numpy(S.id_batch(s, B, 10**7, "zipf")).cuda() for s in range(16)]
    g = torch.from_numpy(S.grad_batch(0, B, D)).cuda()
    k = [0]

    def one():
      s = k[0]
      step.forward(ring[s % 16], next_ids=ring[(s + 1) % 16])
      step.backward(g, S.update_time(s))
      k[0] += 1
    timed(one, 10)
    dt = timed(one, steps)
    emit("sparse_step_dim64_b65536_%s" % ("set" if attach else "no_set"), dt,
         touched=(tks.stats()[:3] if tks else None))
    mt.close()
    if tks is not None:
      tks.close()


def bench_multi(quick):
  steps = 10 if quick else 50
  dims = [16, 32, 64]
  T = 26
  names = ["f%02d" % i for i in range(T)]
  for attach in (False, True):
    cfgs = {n: entry.make_table_config([entry.CombineAsSegment(dims[i % 3], entry.ZerosInitializer(),
                                                               entry.AdagradOptimizer(0.001, 0.1))])
            for i, n in enumerate(names)}
    mt = MultiHashTable.from_configs(cfgs, name_suffix="tkb_m%d" % attach)
    tks = TouchedKeySet(name_suffix="tkb_m%d" % attach) if attach else None
    if tks is not None:
      mt.set_touched_key_set(tks)
    step = MultiSparseStep(mt, B)
    ring = [mt.get_ragged_id({n: torch.from_numpy(S.id_batch(100 * s + i, B, 10**6, "zipf", feature_slot=i + 1)).cuda()
                              for i, n in enumerate(names)}) for s in range(4)]
    total = sum(B * dims[i % 3] for i in range(T))
    g = torch.full((total,), 0.001, dtype=torch.float32, device="cuda")
    k = [0]

    def one():
      s = k[0]
      step.forward(ring[s % 4], ring[(s + 1) % 4])
      step.backward(g, S.update_time(s))
      k[0] += 1
    timed(one, 4)
    dt = timed(one, steps)
    emit("multi_step_dlrm26_%s" % ("set" if attach else "no_set"), dt, ids_per_step=T * B,
         touched=(tks.stats()[:3] if tks else None))
    step.close()
    mt.close()
    if tks is not None:
      tks.close()


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "profiles", "touched_key_set"))
  p.add_argument("--quick", action="store_true")
  a = p.parse_args()
  torch.cuda.set_device(0)
  bench_set(a.quick)
  bench_single(a.quick)
  bench_multi(a.quick)
  os.makedirs(a.out, exist_ok=True)
  with open(os.path.join(a.out, "touched_key_set.jsonl"), "w") as f:
    for rec in LINES:
      f.write(json.dumps(rec) + "\n")
  with open(os.path.join(a.out, "touched_key_set.md"), "w") as f:
    f.write("# Touched-key set: per-call times (one MI355X)\n\n| case | µs | algorithmic bytes | GB/s | notes |\n|---|---|---|---|---|\n")
    for rec in LINES:
      extra = {k: v for k, v in rec.items() if k not in ("name", "us", "alg_bytes", "GBps")}
      f.write("| %s | %s | %s | %s | %s |\n" % (rec["name"], rec["us"], rec.get("alg_bytes", ""), rec.get("GBps", ""),
                                              json.dumps(extra) if extra else ""))


if __name__ == "__main__":
  main()
