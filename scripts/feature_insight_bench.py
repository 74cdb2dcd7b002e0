"""Measurements of FeatureInsight: the plain forward, the forward plus both gradients and the
fused aggregate, against the torch composition on the same device, one JSON object per line
(feature_insight.jsonl) and a markdown table (feature_insight_table.md) under profiles/feature_insight/ (or
--out DIR).

Shapes: B = 65 536, 26 segments of 16 (E = 416) and 26 segments of mixed sizes 4 .. 64, K = 64: forward, and forward
plus both gradients; the aggregate at K = 64 and K = 1 024 (uniform segments).

The composition is the faster of ``split`` + per-feature ``matmul`` + ``cat`` (the reference test's own
construction) and, where the sizes are uniform, a batched ``einsum``; its gradients are the same two constructions
applied to grad (no autograd graph is kept, which favours the composition); the aggregate is the composition followed
by the square and the sum over K.  Where it cannot allocate its [B, F K] intermediate the line says so and the
comparison is repeated at the largest K (halving) where it can.

Beside the time a line holds the algorithmic bytes (every operand read once, every result written once) as a share
of 8 TB/s, and the flops (2 B E K per product: one for the forward and the aggregate, three with gradients) as a
share of the 157 TFLOPS fp32 peak.

Both sides are checked first: the op against the composition, with a tolerance that is NOT derived (1e-4 of the
largest element; the composition's own order of summation is not known) — a guard against a gross mismatch; the
derived bounds are the test suite's business (tests/feature_insight_truth.py).

Timing: device events around a window of back-to-back calls that lasts at least 0.5 s (--window), after warm-up;
the op and the composition take turns, case by case, and the whole round is repeated three times: a figure is the
median of the three windows, the spread their (max - min) / median.  There is no fallback: without a GPU the
script fails after printing the plans.
    python scripts/feature_insight_bench.py [--out DIR] [--window S] [--batch 65536]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FLOPS = 157.3e12
PEAK_BYTES = 8e12
UNIFORM = [16] * 26
MIXED = [4, 8, 16, 32, 64, 4, 8, 16, 32, 64, 4, 8, 16, 32, 64, 4, 8, 16, 32, 64, 4, 8, 16, 32, 64, 12]   # E = 632


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_insight"))
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--batch", type=int, default=65536)
  args = ap.parse_args()
  B = args.batch

  import torch
  from monolith_amd import layer_ops
  for sizes, K in ((UNIFORM, 64), (MIXED, 64), (UNIFORM, 1024)):
    print("plan B=%d E=%d K=%d F=%d" % (B, sum(sizes), K, len(sizes)),
          layer_ops.feature_insight_plan(B, sum(sizes), K, len(sizes)))
  if not torch.cuda.is_available():
    raise SystemExit("feature_insight_bench.py needs the MI355X: there is no fallback")

  def split_forward(x, w, sizes):
    return torch.cat([a @ b for a, b in zip(x.split(sizes, dim=1), w.split(sizes, dim=0))], dim=1)

  def split_grads(g, x, w, sizes):
    K = w.shape[1]
    gs = g.split(K, dim=1)
    gi = torch.cat([a @ b.t() for a, b in zip(gs, w.split(sizes, dim=0))], dim=1)
    gw = torch.cat([a.t() @ b for a, b in zip(x.split(sizes, dim=1), gs)], dim=0)
    return gi, gw

  def einsum_forward(x, w, sizes):
    F, s = len(sizes), sizes[0]
    return torch.einsum("bfs,fsk->bfk", x.view(x.shape[0], F, s), w.view(F, s, -1)).reshape(x.shape[0], -1)

  def einsum_grads(g, x, w, sizes):
    F, s = len(sizes), sizes[0]
    g3, x3, w3 = g.view(g.shape[0], F, -1), x.view(x.shape[0], F, s), w.view(F, s, -1)
    return (torch.einsum("bfk,fsk->bfs", g3, w3).reshape(x.shape),
            torch.einsum("bfk,bfs->fsk", g3, x3).reshape(w.shape))

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

  def close(a, b):
    assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-4 * b.abs().max().item(), (a - b).abs().max()

  gen = torch.Generator(device="cuda").manual_seed(1)
  cases = []   # (name, sizes, K, form, op fn, {composition name: fn}, note)

  def add(name, sizes, K, form):
    E, F = sum(sizes), len(sizes)
    uniform = len(set(sizes)) == 1
    x = torch.randn(B, E, device="cuda", generator=gen)
    w = torch.randn(E, K, device="cuda", generator=gen)
    note, comps = None, {}
    fwds = {"split+matmul+cat": split_forward}
    grads = {"split+matmul+cat": split_grads}
    if uniform:
      fwds["einsum"], grads["einsum"] = einsum_forward, einsum_grads
    if form == "aggregate":
      op = lambda: layer_ops.feature_insight(x, w, sizes, True)  # noqa: E731
      for n, f in fwds.items():
        comps[n] = lambda f=f: (f(x, w, sizes) ** 2).view(B, F, K).sum(dim=2)
    elif form == "forward":
      op = lambda: layer_ops.feature_insight(x, w, sizes)  # noqa: E731
      for n, f in fwds.items():
        comps[n] = lambda f=f: f(x, w, sizes)
    else:
      g = torch.randn(B, F * K, device="cuda", generator=gen)
      op = lambda: ((layer_ops.feature_insight(x, w, sizes),) +  # noqa: E731
                    layer_ops.feature_insight_grad(g, x, w, sizes))
      for n in fwds:
        comps[n] = lambda f=fwds[n], b=grads[n]: (f(x, w, sizes),) + b(g, x, w, sizes)
    try:
      for n, c in comps.items():
        got, want = op(), c()
        for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
          close(a, b)
        del got, want
    except torch.OutOfMemoryError as e:
      comps, note = {}, "the composition failed to allocate: " + str(e).splitlines()[0]
      print("%s: %s" % (name, note))
    torch.cuda.empty_cache()
    cases.append((name, sizes, K, form, op, comps, note))
    return bool(comps)

  add("uniform", UNIFORM, 64, "forward")
  add("uniform", UNIFORM, 64, "forward+grads")
  add("mixed", MIXED, 64, "forward")
  add("mixed", MIXED, 64, "forward+grads")
  add("uniform", UNIFORM, 64, "aggregate")
  K = 1024
  while not add("uniform", UNIFORM, K, "aggregate") and K > 64:
    K //= 2

  times = {}
  for _ in range(args.repeats):
    for name, sizes, K, form, op, comps, _ in cases:
      times.setdefault((name, K, form, "op"), []).append(window(op))
      for n, c in comps.items():
        times.setdefault((name, K, form, n), []).append(window(c))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "feature_insight.jsonl"), "w") as f:
    for name, sizes, K, form, _, comps, note in cases:
      E, F = sum(sizes), len(sizes)
      products = 3 if form == "forward+grads" else 1
      flops = products * 2.0 * B * E * K
      nbytes = 4.0 * (B * E + E * K + (B * F if form == "aggregate" else B * F * K))
      if form == "forward+grads":   # the gradient: grad, input and weight read, both gradients written
        nbytes += 4.0 * (B * F * K + 2 * B * E + 2 * E * K)
      rec = {"case": name, "form": form, "B": B, "E": E, "K": K, "F": F, "flops": flops, "algorithmic_bytes": nbytes,
             "plan": layer_ops.feature_insight_plan(B, E, K, F)}
      if note:
        rec["note"] = note

      def summary(key):
        ts = [t for t, _ in times[key]]
        med = statistics.median(ts)
        return {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts], "calls_per_window": times[key][0][1],
                "spread": (max(ts) - min(ts)) / med}
      rec["op"] = summary((name, K, form, "op"))
      rec["op"]["share_of_8_TB_s"] = nbytes / (rec["op"]["us"] * 1e-6) / PEAK_BYTES
      rec["op"]["share_of_fp32_peak"] = flops / (rec["op"]["us"] * 1e-6) / PEAK_FLOPS
      rec["compositions"] = {n: summary((name, K, form, n)) for n in comps}
      if comps:
        best = min(rec["compositions"], key=lambda n: rec["compositions"][n]["us"])
        rec["best_composition"] = best
        rec["composition_over_op"] = rec["compositions"][best]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "feature_insight_table.md"), "w") as f:
    f.write("| case | form | E | K | op µs | spread | of 8 TB/s | of 157 TFLOPS | best composition | µs | spread | "
            "composition / op |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      if "best_composition" in r:
        c = r["compositions"][r["best_composition"]]
        tail = "%s | %.1f | %.1f %% | %.2fx" % (r["best_composition"], c["us"], 100 * c["spread"],
                                                 r["composition_over_op"])
      else:
        tail = "failed to allocate | | | "
      f.write("| %s | %s | %d | %d | %.1f | %.1f %% | %.1f %% | %.1f %% | %s |\n" %
              (r["case"], r["form"], r["E"], r["K"], r["op"]["us"], 100 * r["op"]["spread"],
               100 * r["op"]["share_of_8_TB_s"], 100 * r["op"]["share_of_fp32_peak"], tail))


if __name__ == "__main__":
  main()
