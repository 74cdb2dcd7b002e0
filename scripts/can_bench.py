"""Measurements of the CAN co-action unit against the fp32 torch composition on the same device:
one JSON object per line (can.jsonl) and a markdown table (can_table.md) under profiles/can/ (or --out DIR).

Shapes (B = 65 536): stacked sequence F = 10, T = 12, d = 10, L = 2 (the reference test's); stacked sequence F = 4,
T = 50, d = 16, L = 2; stacked F = 26, d = 16, L = 2; stacked sequence F = 4, T = 50, d = 4, L = 8 (deep and narrow).
Forms: the forward; the forward plus both gradients.  The composition is the reference's own lines (split, reshape,
``relu(matmul(user, weight) + bias)`` per layer, ``sum`` over T) and its autograd backward; it is not tuned.

Beside the time a line holds the op's bound: the bytes that must move (user, item and out; dout, duser and ditem
more with the gradients) over 8 TB/s; and the peak allocation of either side.

Timing: device events around a window of back-to-back calls that lasts at least --window seconds, after warm-up;
the op and the composition take turns and the round is repeated three times: a figure is the median of the three
windows, the spread their (max - min) / median.  There is no fallback: without a GPU the script fails after
printing the plans.
    python scripts/can_bench.py [--out DIR] [--window S] [--batch 65536]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8e12
SHAPES = ((10, 12, 10, 2), (4, 50, 16, 2), (26, 1, 16, 2), (4, 50, 4, 8))   # F, T (1: no sequence axis), d, L


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "can"))
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--batch", type=int, default=65536)
  args = ap.parse_args()
  B = args.batch

  import torch
  from monolith_amd import layer_ops
  for shape in SHAPES:
    print("plan F=%d T=%d d=%d L=%d" % shape, layer_ops.can_plan(B, *shape))
  if not torch.cuda.is_available():
    raise SystemExit("can_bench.py needs the MI355X: there is no fallback")

  def composed(user, item, L, is_seq):
    """CAN.call, stacked"""
    d = user.shape[-1]
    params = torch.split(item, [d * d, d] * L, dim=1)
    lead = (B, 1) if is_seq else (B,)
    for i in range(L):
      user = torch.relu(torch.matmul(user, params[2 * i].reshape(lead + (d, d))) +
                        params[2 * i + 1].reshape(lead + (1, d)))
    return user.sum(2) if is_seq else user

  def window(fn):
    for _ in range(2):
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

    per = span(2) / 2
    k = max(2, int(math.ceil(args.window / max(per, 1e-7))))
    return span(k) / k

  def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base

  gen = torch.Generator(device="cuda").manual_seed(1)
  rnd = lambda *s: torch.rand(*s, device="cuda", generator=gen) * 2 - 1   # noqa: E731
  cases = []   # (shape, form, bytes, op fn, composition fn)

  def add(F, T, d, L):   # (a function: every closure below keeps this shape's own tensors)
    is_seq = T > 1
    user = rnd(*((B, F, T, d) if is_seq else (B, F, d)))
    item, g = rnd(B, L * d * (d + 1)) / math.sqrt(d), rnd(B, F, d)
    fwd_bytes = 4.0 * (user.numel() + item.numel() + g.numel())

    def op_fwd():
      return layer_ops.can_forward(user, item, L, "relu", is_seq, True)

    def op_all():
      return (op_fwd(),) + layer_ops.can_grad(g, user, item, L, "relu", is_seq, True)

    def comp_fwd():
      with torch.no_grad():
        return composed(user, item, L, is_seq)

    def comp_all():
      ops = [t.detach().requires_grad_() for t in (user, item)]
      out = composed(*ops, L, is_seq)
      return (out,) + torch.autograd.grad(out, ops, g)

    # a guard, not a derived bound (the test suite has those)
    for a, b in zip(op_all(), comp_all()):
      assert (a - b).norm().item() <= 1e-3 * b.norm().item()
    cases.extend([((F, T, d, L), "forward", fwd_bytes, op_fwd, comp_fwd),
                  ((F, T, d, L), "forward + gradients", 2 * fwd_bytes, op_all, comp_all)])

  for shape in SHAPES:
    add(*shape)

  times = {}
  for _ in range(args.repeats):
    for i, case in enumerate(cases):
      times.setdefault((i, "op"), []).append(window(case[3]))
      times.setdefault((i, "torch"), []).append(window(case[4]))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "can.jsonl"), "w") as f:
    for i, ((F, T, d, L), form, nbytes, op, comp) in enumerate(cases):
      rec = {"form": form, "B": B, "F": F, "T": T, "d": d, "layer_num": L, "min_bytes": nbytes,
             "plan": layer_ops.can_plan(B, F, T, d, L)}
      for side, fn in (("op", op), ("torch", comp)):
        ts = times[(i, side)]
        med = statistics.median(ts)
        rec[side] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts], "spread": (max(ts) - min(ts)) / med,
                     "time_over_bound": med / (nbytes / PEAK_BYTES), "peak_allocation_bytes": peak(fn)}
      rec["torch_over_op"] = rec["torch"]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "can_table.md"), "w") as f:
    f.write("| F | T | d | L | form | op ms | spread | over its bound | op peak MB | torch ms | spread | torch peak MB | "
            "torch / op |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      f.write("| %d | %d | %d | %d | %s | %.3f | %.1f %% | %.1fx | %.0f | %.3f | %.1f %% | %.0f | %.2fx |\n" %
              (r["F"], r["T"], r["d"], r["layer_num"], r["form"], r["op"]["us"] / 1e3, 100 * r["op"]["spread"],
               r["op"]["time_over_bound"], r["op"]["peak_allocation_bytes"] / 2 ** 20, r["torch"]["us"] / 1e3,
               100 * r["torch"]["spread"], r["torch"]["peak_allocation_bytes"] / 2 ** 20, r["torch_over_op"]))


if __name__ == "__main__":
  main()
