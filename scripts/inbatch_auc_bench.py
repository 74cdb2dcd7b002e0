"""Measurements of the in-batch AUC loss: the forward alone, the forward with its fused unit
gradient and the separate gradient op, against a torch composition of the same math on the same device, one JSON
object per line (inbatch_auc.jsonl) and a markdown table (inbatch_auc_table.md) under profiles/inbatch_auc/ (or
--out DIR).

Shapes: n = 65 536 with 5 % and with 50 % positives, and n = 4 096 with 50 %; logits uniform in [-4, 4].
Work per call, from the shapes: P N pairs for the forward alone, 2 P N for the two with a gradient (the second
sweep repeats the terms for the negatives' sums).  Beside the time a line holds
  pairs_per_s        evaluated pairs per second
  valu_slots         vector-instruction issue slots the chip had per evaluated pair in that time: 1024 SIMDs at
                     2.4 GHz, one wavefront instruction (64 pairs) per 4 cycles
  hbm_fraction       the bytes a call must move (label, logit, the gradient, the partial sums written and read once)
                     over the time, as a fraction of the 8 TB/s peak
The kernels' inner loops hold about 65 (loss and weight), 45 (loss alone) and 42 (weight alone) vector
instructions per pair (the build's assembly); valu_slots over those figures is the share of the time the arithmetic
accounts for.

The composition: for a block of positives, ``d = pos[:, None] - neg[None, :]``, ``logsigmoid(d).sum()`` and the row
and column sums of ``sigmoid(-d)``; blocks of at most 2^25 pairs, so that the intermediates fit in memory.

Timing: device events around a window of back-to-back calls that lasts at least 0.5 s (--window), after warm-up;
the op and the composition take turns, case by case, and the whole round is repeated three times: a figure is the
median of the three windows, the spread their (max - min) / median.  There is no fallback: without a GPU the
script fails after printing the pair counts.
    python scripts/inbatch_auc_bench.py [--out DIR] [--window S]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12                          # B/s
SLOTS_PER_S = 1024 * 2.4e9 / 4 * 64    # pair-wide instruction slots per second
SHAPES = [(65536, 0.05), (65536, 0.5), (4096, 0.5)]
BLOCK_PAIRS = 1 << 25


def work(n, P, form):
  """-> (evaluated pairs, bytes a call must move)"""
  N = n - P
  sweeps = 1 if form == "forward" else 2
  moved = 8 * n + (4 * n if sweeps == 2 else 0)
  # partial sums: one double per element and chunk, written and read; at least one chunk (mhte_auc_core.h)
  budget = max(1 << 19, n)
  for A, B in ((P, N), (N, P))[:sweeps]:
    stride = (A + 255) // 256 * 256
    chunks = min(max(1, budget // max(stride, 1)), (B + 255) // 256)
    if sweeps == 2:
      moved += 16 * chunks * A
  return sweeps * P * N, moved


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                "profiles", "inbatch_auc"))
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  args = ap.parse_args()
  for n, frac in SHAPES:
    print("pairs n=%d positives=%g" % (n, frac), {f: work(n, int(n * frac), f)[0] for f in ("forward", "fused", "grad")})

  import torch
  if not torch.cuda.is_available():
    raise SystemExit("inbatch_auc_bench.py needs the MI355X: there is no fallback")
  from monolith_amd import losses

  def compose(label, logit, want_grad):
    pos, neg = logit[label > 0], logit[(label <= 0) & (label > -10000)]
    rows = max(1, BLOCK_PAIRS // max(1, neg.numel()))
    loss = torch.zeros((), device=logit.device, dtype=torch.float64)
    row = torch.empty_like(pos)
    col = torch.zeros_like(neg)
    for a in range(0, pos.numel(), rows):
      d = pos[a:a + rows, None] - neg[None, :]
      loss += torch.nn.functional.logsigmoid(d).sum(dtype=torch.float64)
      if want_grad:
        s = torch.sigmoid(-d)
        row[a:a + rows] = s.sum(1)
        col += s.sum(0)
    return loss.float(), row, col

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

  g = torch.Generator(device="cuda").manual_seed(17)
  cases = []
  for n, frac in SHAPES:
    P = int(n * frac)
    label = torch.zeros(n, device="cuda")
    label[torch.randperm(n, device="cuda", generator=g)[:P]] = 1.0
    logit = torch.rand(n, device="cuda", generator=g) * 8 - 4
    # the op and the composition compute the same thing (a tolerance: the composition sums in fp32 trees)
    loss, unit = losses._forward(label, logit, 1.0, True)
    closs, crow, ccol = compose(label, logit, True)
    assert torch.allclose(loss, closs, rtol=1e-5), (loss, closs)
    assert torch.allclose(unit[label > 0], crow, rtol=1e-4) and torch.allclose(unit[label <= 0], -ccol, rtol=1e-4)
    cases.append((n, P, "forward", lambda la=label, lo=logit: losses._forward(la, lo, 1.0, False),
                  lambda la=label, lo=logit: compose(la, lo, False)))
    cases.append((n, P, "fused", lambda la=label, lo=logit: losses._forward(la, lo, 1.0, True),
                  lambda la=label, lo=logit: compose(la, lo, True)))
    cases.append((n, P, "grad", lambda la=label, lo=logit: losses.inbatch_auc_loss_grad(la, lo, 2.0, 1.0),
                  lambda la=label, lo=logit: compose(la, lo, True)))

  times = {}
  for _ in range(args.repeats):
    for n, P, form, ours, theirs in cases:
      for who, fn in (("op", ours), ("composition", theirs)):
        times.setdefault((n, P, form, who), []).append(window(fn))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "inbatch_auc.jsonl"), "w") as f:
    for n, P, form, _, _ in cases:
      pairs, moved = work(n, P, form)
      rec = {"case": form, "n": n, "positives": P, "negatives": n - P, "pairs": pairs, "bytes": moved}
      for who in ("op", "composition"):
        ts = [t for t, _ in times[(n, P, form, who)]]
        med = statistics.median(ts)
        rec[who] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts],
                    "calls_per_window": times[(n, P, form, who)][0][1], "spread": (max(ts) - min(ts)) / med}
      op = rec["op"]["us"] * 1e-6
      rec["op"].update(pairs_per_s=pairs / op, valu_slots=SLOTS_PER_S * op / pairs, hbm_fraction=moved / op / PEAK)
      rec["composition_over_op"] = rec["composition"]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "inbatch_auc_table.md"), "w") as f:
    f.write("| call | n | positives | pairs | op µs | spread | pairs / s | issue slots per pair | of 8 TB/s | "
            "composition µs | spread | composition / op |\n")
    f.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      f.write("| %s | %d | %d | %.3g | %.1f | %.1f %% | %.3g | %.0f | %.2f %% | %.1f | %.1f %% | %.1fx |\n" %
              (r["case"], r["n"], r["positives"], r["pairs"], r["op"]["us"], 100 * r["op"]["spread"],
               r["op"]["pairs_per_s"], r["op"]["valu_slots"], 100 * r["op"]["hbm_fraction"],
               r["composition"]["us"], 100 * r["composition"]["spread"], r["composition_over_op"]))


if __name__ == "__main__":
  main()
