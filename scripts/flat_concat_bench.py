"""Measurements of the aligned flat concat / split, one JSON object per line and a markdown
table under profiles/flat_concat/ (or --out DIR), on the gradient set of scripts/clip_bench.py (26 tensors
[65 536, dim] with dims 16 / 32 / 64 plus the weight and bias gradients of the dense tower):

  * the concat with an fp32 wire (8 algorithmic bytes per element: read 4, write 4) and an fp16 wire (6 B),
    each with the scale in the arguments and in a device word;
  * the decode in place (fp32, 8 B) and from fp16 (6 B);
  * the pair global_l2_reduce + concat with the device scale (4 B more per element for the norm);
  * two baselines: (1) torch.cat of the flattened gradients times the scale (no padding; 16 B: the cat's
    read and write, then the multiply's), (2) mhte_scale_tensors_dev into hand-made views of a flat buffer at
    the aligned offsets, which moves the same 8 B (and leaves the padding alone).

All cases take turns in every round of one process (interleaved); a case's figure is the median of its
rounds, each round the wall time of `reps` back-to-back calls and one synchronisation, divided by reps.
Fractions are of the 8 TB/s HBM peak.
    python scripts/flat_concat_bench.py [--out DIR] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_bench import PEAK, gradient_set, timed  # noqa: E402
from monolith_amd import _lib, clip_ops  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "profiles", "flat_concat"))
  p.add_argument("--quick", action="store_true")
  a = p.parse_args()
  torch.cuda.set_device(0)
  rounds, reps = (3, 5) if a.quick else (7, 20)
  ts = gradient_set()
  n = sum(t.numel() for t in ts)
  offs = D.aligned_flat_offsets([t.numel() for t in ts])
  total = offs[-1]
  out32 = torch.empty(total, dtype=torch.float32, device="cuda")
  out16 = torch.empty(total, dtype=torch.float16, device="cuda")
  dec = torch.randn(total, device="cuda")
  wire16 = dec.to(torch.float16)
  _, scale_dev = clip_ops.global_norm_and_scale(ts, 1.0)
  scale_host = float(scale_dev.item())
  # baseline (2): the multiply of clip_ops.scale_tensors, its outputs hand-made views of one flat buffer
  views = [out32[o:o + t.numel()] for t, o in zip(ts, offs)]
  m = len(ts)
  pin = (C.c_void_p * m)(*[C.c_void_p(t.data_ptr()) for t in ts])
  pout = (C.c_void_p * m)(*[C.c_void_p(v.data_ptr()) for v in views])
  lens = (C.c_int64 * m)(*[t.numel() for t in ts])
  L = _lib.lib()

  def scale_into_views():
    _lib.check(L.mhte_scale_tensors_dev(pin, pout, lens, m, _lib.vp(scale_dev),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))

  def norm_and_concat():
    _, s = clip_ops.global_norm_and_scale(ts, 1.0)
    D.aligned_flat_concat(ts, scale=s, out=out32)

  cases = [
      ("concat fp32, host scale", 8 * n, lambda: D.aligned_flat_concat(ts, scale=scale_host, out=out32)),
      ("concat fp32, device scale", 8 * n, lambda: D.aligned_flat_concat(ts, scale=scale_dev, out=out32)),
      ("concat fp16, host scale", 6 * n,
       lambda: D.aligned_flat_concat(ts, scale=scale_host, wire_dtype=torch.float16, out=out16)),
      ("concat fp16, device scale", 6 * n,
       lambda: D.aligned_flat_concat(ts, scale=scale_dev, wire_dtype=torch.float16, out=out16)),
      ("decode fp32 in place (x 1.0)", 8 * n, lambda: D.aligned_flat_split(ts, dec, post_scale=1.0)),
      ("decode fp16 -> fp32 (new buffer)", 6 * n, lambda: D.aligned_flat_split(ts, wire16, post_scale=0.5)),
      ("global_l2_reduce + concat fp32, device scale", 12 * n, norm_and_concat),
      ("baseline 1: torch.cat(flattened) * scale", 16 * n,
       lambda: torch.cat([t.reshape(-1) for t in ts]) * scale_host),
      ("baseline 2: mhte_scale_tensors_dev into views of a flat buffer", 8 * n, scale_into_views),
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
  with open(os.path.join(a.out, "flat_concat.jsonl"), "w") as f:
    for rec in lines:
      f.write(json.dumps(rec) + "\n")
  with open(os.path.join(a.out, "flat_concat.md"), "w") as f:
    f.write("# Aligned flat concat / split: per-call times (one MI355X)\n\n"
            "%d tensors, %d floats (%d with the padding to 16 elements); %d rounds of %d calls, all cases "
            "interleaved; median of the rounds.  Algorithmic bytes count the tensors' elements, not the padding.\n\n"
            "| case | µs | algorithmic bytes | GB/s | of 8 TB/s | rounds (µs) |\n|---|---|---|---|---|---|\n"
            % (len(ts), n, total, rounds, reps))
    for rec in lines:
      f.write("| %s | %s | %s | %s | %.1f %% | %s |\n" % (rec["name"], rec["us"], rec["alg_bytes"], rec["GBps"],
                                                        100 * rec["peak_fraction"], rec["us_rounds"]))


if __name__ == "__main__":
  main()
