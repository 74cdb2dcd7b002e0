"""Measurements of the CIN layer against the fp32 torch composition on the same device: one JSON
object per line (cin.jsonl) and a markdown table (cin_table.md) under profiles/cin/ (or --out DIR).

Shapes: the workload's (m = 26, D = 16, H = U = 128) and xDeepFM's (m = 39, D = 10, H = U = 200), B = 65 536.
Forms: the layer forward; the layer forward plus all four gradients; a three-layer ``CIN`` module, forward and
backward through autograd.  The composition is the reference's own: ``einsum('bdh,bdm->bdhm')``, reshape,
``matmul``, bias, relu, ``sum(1)``, and its autograd backward; it is not tuned.

Beside the time a line holds the flops of the GEMMs (2 B D H m U per product: one forward, three with gradients)
as a share of the 157 TFLOPS fp32 matrix peak, and the peak allocation of either side (the composition's holds the
[B, D, H m] outer product, the op's must not).

Timing: device events around a window of back-to-back calls that lasts at least --window seconds, after warm-up;
the op and the composition take turns and the round is repeated three times: a figure is the median of the three
windows, the spread their (max - min) / median.  There is no fallback: without a GPU the script fails after
printing the plans.
    python scripts/cin_bench.py [--out DIR] [--window S] [--batch 65536]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 157.3e12
SHAPES = {"workload": (26, 16, 128), "xdeepfm": (39, 10, 200)}   # m, D, H = U


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cin"))
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--batch", type=int, default=65536)
  args = ap.parse_args()
  B = args.batch

  import torch
  from monolith_amd import layer_ops
  from monolith_amd.feature_cross import CIN
  for name, (m, D, U) in SHAPES.items():
    print("plan %s" % name, layer_ops.cin_plan(B, m, D, U, U))
  if not torch.cuda.is_available():
    raise SystemExit("cin_bench.py needs the MI355X: there is no fallback")

  def composed(x0, xl, w, bias, relu):
    """CIN.call's loop body on [B, D, m] / [B, D, H] operands -> (out [B, D, U], pooled)"""
    z = torch.einsum("bdh,bdm->bdhm", xl, x0).reshape(x0.shape[0], x0.shape[1], -1)
    out = z @ w + bias
    if relu:
      out = torch.relu(out)
    return out, out.sum(1)

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
  cases = []   # (shape name, form, flops, op fn, composition fn)

  def add(name, m, D, U):   # (a function: every closure below keeps this shape's own tensors)
    H = U
    x0, xl, w, bias = rnd(B, m, D), rnd(B, H, D), rnd(H * m, U) / math.sqrt(H * m), rnd(U)
    dxn, dp = rnd(B, U, D), rnd(B, U)
    x0t, xlt, dxnt = (t.transpose(1, 2).contiguous() for t in (x0, xl, dxn))
    gemm = 2.0 * B * D * H * m * U

    def op_fwd():
      return layer_ops.cin_layer(x0, xl, w, bias, "relu")

    def op_all():
      xn, _ = layer_ops.cin_layer(x0, xl, w, bias, "relu")
      return layer_ops.cin_layer_grad(dxn, dp, x0, xl, w, xn, "relu")

    def comp_fwd():
      with torch.no_grad():
        return composed(x0t, xlt, w, bias, True)

    def comp_all():
      ops = [t.detach().requires_grad_() for t in (x0t, xlt, w, bias)]
      out, pooled = composed(*ops, True)
      return torch.autograd.grad([out, pooled], ops, [dxnt, dp])

    got, want = op_fwd(), comp_fwd()
    assert (got[1] - want[1]).abs().max().item() <= 1e-4 * want[1].abs().max().item()
    gg, gw = op_all(), comp_all()
    # a guard, not a derived bound; in the norm, because a pre-activation that the two sides round to either side of
    # 0 flips relu's mask and moves a gradient element by a whole term (the test suite keeps such inputs out)
    for a, b in zip(gg, (gw[0].transpose(1, 2), gw[1].transpose(1, 2), gw[2], gw[3])):
      assert (a - b).norm().item() <= 1e-3 * b.norm().item()
    del got, want, gg, gw

    units = [U, U, U]
    layer = CIN(units, "relu")
    xin = x0.clone().requires_grad_()
    up = rnd(B, sum(units))
    layer(xin)
    params = [getattr(layer, "%s_%d" % (k, i)) for i in range(3) for k in ("kernel", "bias")]

    def op_module():
      return torch.autograd.grad(layer(xin), [xin] + params, up)

    def comp_module():
      xt = xin.transpose(1, 2)
      state, pooled = xt, []
      for i in range(3):
        state, p = composed(xt, state, params[2 * i], params[2 * i + 1], i < 2)
        pooled.append(p)
      return torch.autograd.grad(torch.cat(pooled, 1), [xin] + params, up)

    hs = [m, U, U]
    cases.extend([(name, "layer forward", gemm, op_fwd, comp_fwd),
                  (name, "layer forward + gradients", 3 * gemm, op_all, comp_all),
                  (name, "3-layer module, forward + backward", 3 * sum(2.0 * B * D * h * m * U for h in hs),
                   op_module, comp_module)])

  for name, (m, D, U) in SHAPES.items():
    add(name, m, D, U)

  times = {}
  for _ in range(args.repeats):
    for i, (_, _, _, op, comp) in enumerate(cases):
      times.setdefault((i, "op"), []).append(window(op))
      times.setdefault((i, "torch"), []).append(window(comp))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "cin.jsonl"), "w") as f:
    for i, (name, form, flops, op, comp) in enumerate(cases):
      m, D, U = SHAPES[name]
      rec = {"shape": name, "form": form, "B": B, "m": m, "D": D, "H": U, "U": U, "flops": flops,
             "outer_product_bytes": 4 * B * D * U * m, "plan": layer_ops.cin_plan(B, m, D, U, U)}
      for side, fn in (("op", op), ("torch", comp)):
        ts = times[(i, side)]
        med = statistics.median(ts)
        rec[side] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts], "spread": (max(ts) - min(ts)) / med,
                     "share_of_fp32_matrix_peak": flops / med / PEAK_FLOPS, "peak_allocation_bytes": peak(fn)}
      rec["torch_over_op"] = rec["torch"]["us"] / rec["op"]["us"]
      rec["op_holds_no_outer_product"] = rec["op"]["peak_allocation_bytes"] < rec["outer_product_bytes"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "cin_table.md"), "w") as f:
    f.write("| shape | form | op ms | spread | of 157 TFLOPS | op peak MB | torch ms | spread | torch peak MB | "
            "torch / op |\n|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      f.write("| %s | %s | %.2f | %.1f %% | %.1f %% | %.0f | %.2f | %.1f %% | %.0f | %.2fx |\n" %
              (r["shape"], r["form"], r["op"]["us"] / 1e3, 100 * r["op"]["spread"],
               100 * r["op"]["share_of_fp32_matrix_peak"], r["op"]["peak_allocation_bytes"] / 2 ** 20,
               r["torch"]["us"] / 1e3, 100 * r["torch"]["spread"], r["torch"]["peak_allocation_bytes"] / 2 ** 20,
               r["torch_over_op"]))


if __name__ == "__main__":
  main()
