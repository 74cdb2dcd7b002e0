"""Measurements of the batch softmax loss: the loss alone, the loss with both unit gradients and
the grad entry, against the torch composition of the reference's lines with autograd (normalize, matmul,
logsumexp) on the same device, one JSON object per line (batch_softmax.jsonl) and a markdown table
(batch_softmax_table.md) under profiles/batch_softmax/ (or --out DIR).

Shapes: B = 4 096, 16 384 and 65 536 at k = 64, temperature 0.05, normalised, Zipf-like intervals.  Work per call:
a product is 2 B^2 k' flops (k' = k padded to 8); the loss alone takes one tile product, the two forms with
gradients three tile products (forward, once per gradient) and two second products (G . I^, G^T . Q^): five.
Beside the time a line holds the fraction of the 157 TFLOPS fp32 matrix peak those flops amount to, and the
workspace bytes of the plan.

The composition is not tuned: ``F.normalize``, ``q @ i.T / T + log(max(interval, 1))``, ``logsumexp``, the weighted
sum, ``torch.autograd.grad``.  It materialises B x B matrices; where it cannot allocate them, the line says so.

Both sides are checked first.  At B = 4 096 the op is checked against the float64 truth and its derived bounds
(tests/batch_softmax_truth.py); beyond that the truth's B x B float64 matrices are not affordable.  At every shape
the op is checked against the composition, with tolerances that are NOT derived (2e-5 relative on the loss, 1e-3 of
the largest gradient element): the composition's own error depends on the library's matmul and reduction orders,
which are not known; that check guards against a gross mismatch between the two sides, nothing finer.

Timing: device events around a window of back-to-back calls that lasts at least 0.5 s (--window), after warm-up;
the op and the composition take turns, case by case, and the whole round is repeated three times: a figure is the
median of the three windows, the spread their (max - min) / median.  There is no fallback: without a GPU the
script fails after printing the plans.
    python scripts/batch_softmax_bench.py [--out DIR] [--window S] [--shapes 4096,16384,65536]
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
K, TEMPERATURE = 64, 0.05
PRODUCTS = {"loss": 1, "loss+grads": 5, "grad": 5}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_softmax"))
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--shapes", default="4096,16384,65536")
  args = ap.parse_args()
  shapes = [int(x) for x in args.shapes.split(",")]

  import numpy as np
  import torch
  import batch_softmax_truth as BT
  from monolith_amd import losses
  for B in shapes:
    print("plan B=%d k=%d" % (B, K), losses.batch_softmax_plan(B, K))
  if not torch.cuda.is_available():
    raise SystemExit("batch_softmax_bench.py needs the MI355X: there is no fallback")

  def compose(q, it, iv, r, want_grad):
    if want_grad:
      q, it = q.detach().requires_grad_(True), it.detach().requires_grad_(True)
    qh = torch.nn.functional.normalize(q, dim=1, eps=1e-6)
    ih = torch.nn.functional.normalize(it, dim=1, eps=1e-6)
    z = qh @ ih.T / TEMPERATURE + torch.log(torch.clamp(iv, min=1.0))[None, :]
    loss = -(r * (z.diagonal() - torch.logsumexp(z, dim=1))).sum()
    if not want_grad:
      return loss, None, None
    dq, di = torch.autograd.grad(loss, (q, it))
    return loss, dq, di

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

  cases, notes = [], {}
  for B in shapes:
    q, it, iv, r = (torch.from_numpy(a).cuda() for a in BT.inputs(B, B, K))
    loss, uq, ui = losses._bsm_forward(q, it, iv, r, True, TEMPERATURE, True, True)
    if B <= 4096:   # the op against the truth
      t = BT.Truth(q.cpu().numpy(), it.cpu().numpy(), iv.cpu().numpy(), r.cpu().numpy(), True, TEMPERATURE)
      lb, qb, ib = t.bounds()
      used = (abs(loss.item() - t.loss) / lb, float((np.abs(uq.cpu().numpy() - t.dquery) / qb).max()),
              float((np.abs(ui.cpu().numpy() - t.ditem) / ib).max()))
      print("B=%d: share of the truth's bounds used: loss %.3f dquery %.3f ditem %.3f" % ((B,) + used))
      assert max(used) <= 1.0, used
      notes[B] = {"bounds_used": used}
    try:   # the op against the composition: tolerances not derived (the docstring), a guard against gross mismatch
      closs, cq, ci = compose(q, it, iv, r, True)
      assert abs(loss.item() - closs.item()) <= 2e-5 * abs(closs.item()), (loss, closs)
      for a, b in ((uq, cq), (ui, ci)):
        assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item(), (a - b).abs().max()
      del closs, cq, ci
      composed = True
    except torch.OutOfMemoryError as e:
      composed = False
      notes.setdefault(B, {})["composition_note"] = "failed to allocate: " + str(e).splitlines()[0]
      print("B=%d: the composition failed to allocate" % B)
    torch.cuda.empty_cache()
    T = TEMPERATURE
    forms = (("loss", lambda a=(q, it, iv, r): losses._bsm_forward(*a, True, T, False, False),
              lambda a=(q, it, iv, r): compose(*a, False)),
             ("loss+grads", lambda a=(q, it, iv, r): losses._bsm_forward(*a, True, T, True, True),
              lambda a=(q, it, iv, r): compose(*a, True)),
             ("grad", lambda a=(q, it, iv, r): losses.batch_softmax_loss_grad(*a, 2.0, True, T),
              lambda a=(q, it, iv, r): compose(*a, True)))
    for form, ours, theirs in forms:
      cases.append((B, form, ours, theirs if composed else None))

  times = {}
  for _ in range(args.repeats):
    for B, form, ours, theirs in cases:
      for who, fn in (("op", ours), ("composition", theirs)):
        if fn is not None:
          times.setdefault((B, form, who), []).append(window(fn))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "batch_softmax.jsonl"), "w") as f:
    for B, form, _, theirs in cases:
      plan = losses.batch_softmax_plan(B, K)
      flops = PRODUCTS[form] * 2.0 * B * B * BT.plan(B, K)["kp"]
      rec = {"case": form, "B": B, "k": K, "temperature": TEMPERATURE, "products": PRODUCTS[form], "flops": flops,
             "workspace_bytes": plan["workspace_bytes"], "chunks": plan["row_chunks"]}
      rec.update(notes.get(B, {}))
      for who in ("op", "composition"):
        if (B, form, who) not in times:
          continue
        ts = [t for t, _ in times[(B, form, who)]]
        med = statistics.median(ts)
        rec[who] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts],
                    "calls_per_window": times[(B, form, who)][0][1], "spread": (max(ts) - min(ts)) / med}
      rec["op"]["fraction_of_fp32_matrix_peak"] = flops / (rec["op"]["us"] * 1e-6) / PEAK_FLOPS
      if "composition" in rec and isinstance(rec["composition"], dict):
        rec["composition_over_op"] = rec["composition"]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "batch_softmax_table.md"), "w") as f:
    f.write("| call | B | k | chunks | workspace MiB | op µs | spread | of 157 TFLOPS | composition µs | spread | "
            "composition / op |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      comp = r.get("composition")
      tail = ("%.1f | %.1f %% | %.2fx" % (comp["us"], 100 * comp["spread"], r["composition_over_op"])
              if isinstance(comp, dict) else "failed to allocate | | ")
      f.write("| %s | %d | %d | %d | %.1f | %.1f | %.1f %% | %.1f %% | %s |\n" %
              (r["case"], r["B"], r["k"], r["chunks"], r["workspace_bytes"] / 2 ** 20, r["op"]["us"],
               100 * r["op"]["spread"], 100 * r["op"]["fraction_of_fp32_matrix_peak"], tail))


if __name__ == "__main__":
  main()
