#!/usr/bin/env python
"""The dense tower's gradient export and parameter load against the SGD inside backward, on the tower of
``bench.py --config dlrm26 --dense`` (1024-1024-512-256-1 at batch 65 536), by device events:
  (a) backward(dy, lr)        the chain + the per-layer SGD launches (lr = 0: the weights keep their values)
  (b) backward_grads(dy)      the chain + mlp_export_grads_kernel
  (c) load_params(variables)  mlp_load_params_kernel
  (d) set_params per layer    what load_params replaces (copies + refresh launch + stream synchronise per layer)
All cases interleaved in every round; one JSON line per round and case, then the medians with the spread of
the rounds.  Needs a GPU: there is no fallback."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from monolith_amd.dense_mlp import DenseMlp  # noqa: E402

ROUNDS, CALLS = 7, 20


def timed(fn, reps):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) * 1e3 / reps


def main():
  widths = [int(w) for w in (sys.argv[1] if len(sys.argv) > 1 else "1024,1024,512,256,1").split(",")]
  B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
  dev = torch.device("cuda", 0)
  torch.manual_seed(0)
  mlp = DenseMlp(widths, max_batch=B)
  for i, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
    lin = torch.nn.Linear(a, b).to(dev)
    mlp.set_params(i, lin.weight, lin.bias)
  x = torch.randn(B, widths[0], device=dev)
  dy = torch.full((B,), 1.0 / B, device=dev)
  dx = torch.empty(B, widths[0], device=dev)
  mlp.forward(x)
  variables = mlp.variables()
  grads = [torch.empty_like(v) for v in variables]
  n_params = sum(v.numel() for v in variables)

  def set_all():
    for l in range(mlp.n_layers):
      mlp.set_params(l, variables[2 * l], variables[2 * l + 1])

  cases = [("backward (SGD inside)", lambda: mlp.backward(dy, 0.0, out=dx)),
           ("backward_grads", lambda: mlp.backward_grads(dy, out=dx, grads=grads)),
           ("load_params", lambda: mlp.load_params(variables)),
           ("set_params per layer", set_all)]
  for _, fn in cases:   # every shape warm
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  # the export computes what the SGD would apply: the same bits on these operands too
  before = [v.clone() for v in variables]
  mlp.backward_grads(dy, out=dx, grads=grads)
  mlp.backward(dy, 2.0 ** -10, out=dx)
  same = all(torch.equal(a, b - 2.0 ** -10 * g) for a, b, g in zip(mlp.variables(), before, grads))
  mlp.load_params(before)
  print(json.dumps({"what": "backward(lr) == p - lr * exported g, all bits", "ok": bool(same), "widths": widths,
                    "batch": B, "parameters": n_params}))
  us = {name: [] for name, _ in cases}
  for r in range(ROUNDS):
    for name, fn in cases:
      t = timed(fn, CALLS)
      us[name].append(t)
      print(json.dumps({"round": r, "what": name, "us_per_call": round(t, 2), "calls": CALLS}))
  for name, _ in cases:
    v = us[name]
    print(json.dumps({"what": name, "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                      "max_us": round(max(v), 2), "rounds": ROUNDS}))
  a, b = statistics.median(us["backward (SGD inside)"]), statistics.median(us["backward_grads"])
  print(json.dumps({"what": "backward_grads - backward, medians", "us": round(b - a, 2),
                    "spread_of_backward_us": round(max(us["backward (SGD inside)"]) - min(us["backward (SGD inside)"]), 2),
                    "load_params_bytes_per_weight": 12,
                    "load_params_TBps": round(12.0 * n_params / statistics.median(us["load_params"]) / 1e6, 3)}))
  mlp.close()
  return 0 if same else 1


if __name__ == "__main__":
  sys.exit(main())
