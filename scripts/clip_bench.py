"""Measurements of clip by global norm, one JSON object per line and a markdown table under
profiles/clip/ (or --out DIR), on the dlrm26 gradient set: 26 tensors [65 536, dim] with dims 16 / 32 / 64 plus
the weight and bias gradients of the 1024-1024-512-256-1 dense tower:

  * global_l2_reduce (norm and deferred scale; 4 algorithmic bytes per element);
  * the fused clip out of place, clipped and not clipped (12 B per element: read for the norm, read and
    write for the multiply or the copy);
  * the fused clip in place, clipped (12 B) and not clipped (4 B: nothing is loaded or stored a second time);
  * what a user has without it: torch._foreach_norm + the norm of the stacked norms + .item() +
    torch._foreach_mul_ when the norm is above clip_norm (in place).

All cases take turns in every round of one process (interleaved); a case's figure is the median of its
rounds, each round the wall time of `reps` back-to-back calls and one synchronisation, divided by reps.
In-place cases that clip use clip_norm = 0.99^k x the set's first norm at their k-th call, so that every call
really clips.  Fractions are of the 8 TB/s HBM peak.
    python scripts/clip_bench.py [--out DIR] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monolith_amd import clip_ops  # noqa: E402

PEAK = 8e12
B = 65536


def gradient_set():
  g = torch.Generator(device="cuda").manual_seed(5)
  dims = [16, 32, 64]
  ts = [torch.randn(B, dims[i % 3], device="cuda", generator=g) for i in range(26)]
  widths = [1024, 1024, 512, 256, 1]
  for a, b in zip(widths[:-1], widths[1:]):
    ts.append(torch.randn(b, a, device="cuda", generator=g))
    ts.append(torch.randn(b, device="cuda", generator=g))
  return ts


def timed(fn, reps):
  torch.cuda.synchronize()
  t = time.perf_counter()
  for _ in range(reps):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) / reps


def torch_clip_(ts, clip_norm):
  norm = float(torch.linalg.vector_norm(torch.stack(torch._foreach_norm(ts))).item())
  if norm > clip_norm:
    torch._foreach_mul_(ts, clip_norm / norm)
  return norm


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "profiles", "clip"))
  p.add_argument("--quick", action="store_true")
  a = p.parse_args()
  torch.cuda.set_device(0)
  rounds, reps = (3, 5) if a.quick else (7, 20)
  ts = gradient_set()        # read-only cases and out-of-place cases
  ti = [t.clone() for t in ts]   # the in-place cases' own copy
  n = sum(t.numel() for t in ts)
  norm0 = float(clip_ops._global_norm(ts).item())
  big = 4.0 * norm0
  k = [0]

  def next_clip():
    k[0] += 1
    return norm0 * 0.99 ** k[0]

  cases = [
      ("global_l2_reduce", 4 * n, lambda: clip_ops.global_norm_and_scale(ts, 1.0)),
      ("fused clip, out of place, clipped", 12 * n, lambda: clip_ops.clip_by_global_norm(ts, 1.0)),
      ("fused clip, out of place, not clipped (copy)", 12 * n, lambda: clip_ops.clip_by_global_norm(ts, big)),
      ("fused clip, in place, clipped", 12 * n, lambda: clip_ops.clip_by_global_norm(ti, next_clip(), inplace=True)),
      ("fused clip, in place, not clipped", 4 * n, lambda: clip_ops.clip_by_global_norm(ti, big, inplace=True)),
      ("torch: _foreach_norm + stack norm + .item() + _foreach_mul_, clipped", 12 * n,
       lambda: torch_clip_(ti, next_clip())),
      ("torch: _foreach_norm + stack norm + .item(), not clipped", 4 * n, lambda: torch_clip_(ti, big)),
      ("torch: _foreach_norm + stack norm, no read-back (norm launches alone)", 4 * n,
       lambda: torch.linalg.vector_norm(torch.stack(torch._foreach_norm(ts)))),
  ]
  runs = {name: [] for name, _, _ in cases}
  for name, _, fn in cases:   # warm-up: workspace, allocator, code objects
    timed(fn, 2)
  for _ in range(rounds):
    for name, _, fn in cases:
      runs[name].append(timed(fn, reps))
  lines = []
  for name, alg, _ in cases:
    med = statistics.median(runs[name])
    rec = {"name": name, "us": round(med * 1e6, 1), "alg_bytes": alg, "GBps": round(alg / med / 1e9, 1),
           "peak_fraction": round(alg / med / PEAK, 3), "us_rounds": [round(x * 1e6, 1) for x in runs[name]]}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
  os.makedirs(a.out, exist_ok=True)
  with open(os.path.join(a.out, "clip.jsonl"), "w") as f:
    for rec in lines:
      f.write(json.dumps(rec) + "\n")
  with open(os.path.join(a.out, "clip.md"), "w") as f:
    f.write("# Clip by global norm: per-call times (one MI355X)\n\n"
            "%d tensors, %d floats (dlrm26 gradient set + the dense tower's gradients); %d rounds of %d calls, "
            "all cases interleaved; median of the rounds.\n\n"
            "| case | µs | algorithmic bytes | GB/s | of 8 TB/s | rounds (µs) |\n|---|---|---|---|---|---|\n"
            % (len(ts), n, rounds, reps))
    for rec in lines:
      f.write("| %s | %s | %s | %s | %.1f %% | %s |\n" % (rec["name"], rec["us"], rec["alg_bytes"], rec["GBps"],
                                                        100 * rec["peak_fraction"], rec["us_rounds"]))


if __name__ == "__main__":
  main()
