"""Measurements of the FFM feature cross: layer_ops.ffm and layer_ops.ffm_grad, both interaction
types, against the torch composition a user had to write before the op existed, one JSON object per line
(ffm.jsonl) and a markdown table (ffm_table.md) under profiles/ffm/ (or --out DIR).

Shape: B = 65 536, L = R = 13, D = 16 — dlrm26's 26 features as two groups; the multiply output is 709 MB.
Algorithmic bytes per call, from the shapes (fp32):
  forward   reads (L + R) D per row, writes L R D (multiply) or L R (dot)
  gradient  reads the upstream gradient, L R D (multiply) or L R (dot), and (L + R) D; writes (L + R) D
Fractions are of the 8 TB/s HBM peak.

The composition: ``left.view(B, L, 1, D) * right.view(B, 1, R, D)`` reshaped (multiply) or summed over the last
axis (dot); its gradients through autograd (the backward of that graph, the graph kept).  It materialises the
[B, L, R, D] products also for dot and for both gradients.

Timing: device events around a window of back-to-back calls that lasts at least 0.5 s (--window), after warm-up;
the op and the composition take turns, case by case, and the whole round is repeated three times: a figure is the
median of the three windows, the spread their (max - min) / median.  There is no fallback: without a GPU the
script fails after printing the byte counts.
    python scripts/ffm_bench.py [--out DIR] [--batch B] [--window S]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12   # B/s
L, R, D = 13, 13, 16


def algorithmic_bytes(B, int_type):
  """-> {"ffm": bytes, "ffm_grad": bytes} of one call."""
  ins = B * (L + R) * D * 4
  cross = B * L * R * (D if int_type == "multiply" else 1) * 4
  return {"ffm": ins + cross, "ffm_grad": cross + ins + ins}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                "profiles", "ffm"))
  ap.add_argument("--batch", type=int, default=65536)
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  args = ap.parse_args()
  B = args.batch
  for it in ("multiply", "dot"):
    print("algorithmic bytes", it, algorithmic_bytes(B, it))

  import torch
  if not torch.cuda.is_available():
    raise SystemExit("ffm_bench.py needs the MI355X: there is no fallback")
  from monolith_amd import layer_ops

  g = torch.Generator(device="cuda").manual_seed(13)
  left = (torch.rand(B, L * D, device="cuda", generator=g) * 20 - 10)
  right = (torch.rand(B, R * D, device="cuda", generator=g) * 20 - 10)
  ups = {"multiply": torch.rand(B, L * R * D, device="cuda", generator=g) * 2 - 1,
         "dot": torch.rand(B, L * R, device="cuda", generator=g) * 2 - 1}

  def compose(tl, tr, it):
    prod = tl.view(B, L, 1, D) * tr.view(B, 1, R, D)
    return prod.reshape(B, -1) if it == "multiply" else prod.sum(-1).reshape(B, -1)

  def window(fn):
    """seconds per call over a window of at least args.window seconds"""
    for _ in range(3):
      fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def span(n):
      e0.record()
      for _ in range(n):
        fn()
      e1.record()
      e1.synchronize()
      return e0.elapsed_time(e1) * 1e-3

    per = span(3) / 3
    n = max(3, int(math.ceil(args.window / max(per, 1e-7))))
    return span(n) / n, n

  cases = []
  for it in ("multiply", "dot"):
    tl, tr = left.clone().requires_grad_(), right.clone().requires_grad_()
    graph_out = compose(tl, tr, it)
    up = ups[it]
    cases.append(("ffm", it, lambda it=it: layer_ops.ffm(left, right, D, it),
                  lambda it=it: compose(left, right, it)))
    cases.append(("ffm_grad", it, lambda it=it, up=up: layer_ops.ffm_grad(up, left, right, D, it),
                  lambda o=graph_out, a=tl, b=tr, up=up: torch.autograd.grad(o, (a, b), up, retain_graph=True)))

  # the op and the composition compute the same thing (a tolerance: the composition's dot is another summation tree)
  for name, it, ours, theirs in cases:
    a, b = ours(), theirs()
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for x, y in zip(a, b):
      assert x.shape == y.shape and torch.allclose(x, y, rtol=1e-4, atol=1e-3), (name, it)
  del a, b, x, y

  times = {}
  for _ in range(args.repeats):
    for name, it, ours, theirs in cases:
      for who, fn in (("op", ours), ("composition", theirs)):
        t, n = window(fn)
        times.setdefault((name, it, who), []).append((t, n))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "ffm.jsonl"), "w") as f:
    for name, it, _, _ in cases:
      nbytes = algorithmic_bytes(B, it)[name]
      rec = {"case": name, "int_type": it, "batch": B, "L": L, "R": R, "D": D, "bytes": nbytes}
      for who in ("op", "composition"):
        ts = [t for t, _ in times[(name, it, who)]]
        med = statistics.median(ts)
        rec[who] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts], "calls_per_window": times[(name, it, who)][0][1],
                    "spread": (max(ts) - min(ts)) / med, "fraction_of_8TBps": nbytes / med / PEAK}
      rec["composition_over_op"] = rec["composition"]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "ffm_table.md"), "w") as f:
    f.write("| call | type | bytes | op µs | of 8 TB/s | spread | composition µs | spread | composition / op |\n")
    f.write("|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      f.write("| %s | %s | %.1f MB | %.1f | %.0f %% | %.1f %% | %.1f | %.1f %% | %.2fx |\n" %
              (r["case"], r["int_type"], r["bytes"] / 1e6, r["op"]["us"], 100 * r["op"]["fraction_of_8TBps"],
               100 * r["op"]["spread"], r["composition"]["us"], 100 * r["composition"]["spread"],
               r["composition_over_op"]))


if __name__ == "__main__":
  main()
