"""Measurements of the DCN cross layer against the fp32 torch composition on the same device: one
JSON object per line (dcn.jsonl) and a markdown table (dcn_table.md) under profiles/dcn/ (or --out DIR).

Shapes: B = 65 536, d in {512, 1024}, the vector and the matrix form.  Forms: the layer forward; the layer forward
plus all four gradients; a three-layer ``DCN`` module, forward and backward through autograd.  The composition is the
reference's own line (``x0 * matmul(xl, w) + bias + xl`` / ``x0 * (matmul(xl, w) + bias) + xl``) and its autograd
backward; it is not tuned.

Beside the time a line holds what bounds the form: for the matrix form the flops of the GEMMs (2 B d d per product:
one forward, three with gradients) as a share of the 157 TFLOPS fp32 matrix peak, for the vector form the bytes that
must move (4 B d per pass over [B, d]: xl, x0, xnext forward; g, x0, xl, dxl, dx0 more with gradients) as a share of
8 TB/s; and the peak allocation of either side.

Timing: device events around a window of back-to-back calls that lasts at least --window seconds, after warm-up;
the op and the composition take turns and the round is repeated three times: a figure is the median of the three
windows, the spread their (max - min) / median.  There is no fallback: without a GPU the script fails after
printing the plans.
    python scripts/dcn_bench.py [--out DIR] [--window S] [--batch 65536]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8e12
DIMS = (512, 1024)
LAYERS = 3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcn"))
  ap.add_argument("--window", type=float, default=0.5)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--batch", type=int, default=65536)
  args = ap.parse_args()
  B = args.batch

  import torch
  from monolith_amd import layer_ops
  from monolith_amd.feature_cross import DCN
  for typ in layer_ops.DCN_TYPES:
    for d in DIMS:
      print("plan %s d=%d" % (typ, d), layer_ops.dcn_plan(B, d, typ))
  if not torch.cuda.is_available():
    raise SystemExit("dcn_bench.py needs the MI355X: there is no fallback")

  def composed(x0, xl, w, bias, typ):
    """DCN.call's loop body"""
    if typ == "matrix":
      return x0 * (torch.matmul(xl, w) + bias) + xl
    return x0 * torch.matmul(xl, w) + bias + xl

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
  cases = []   # (type, d, form, flops, bytes, op fn, composition fn)

  def add(typ, d):   # (a function: every closure below keeps this shape's own tensors)
    cols = d if typ == "matrix" else 1
    x0, xl, g = rnd(B, d), rnd(B, d), rnd(B, d)
    w, bias = rnd(d, cols) / math.sqrt(d), rnd(1, d)
    gemm = 2.0 * B * d * d if typ == "matrix" else 0.0
    sweep = 4.0 * B * d

    def op_fwd():
      return layer_ops.dcn_layer(x0, xl, w, bias, typ, want_aux=False)[0]

    def op_all():
      _, aux = layer_ops.dcn_layer(x0, xl, w, bias, typ)
      return layer_ops.dcn_layer_grad(g, x0, xl, w, aux, typ)

    def comp_fwd():
      with torch.no_grad():
        return composed(x0, xl, w, bias, typ)

    def comp_all():
      ops = [t.detach().requires_grad_() for t in (x0, xl, w, bias)]
      return torch.autograd.grad(composed(*ops, typ), ops, g)

    # a guard, not a derived bound (the test suite has those)
    got, want = op_fwd(), comp_fwd()
    assert (got - want).norm().item() <= 1e-4 * want.norm().item()
    for a, b in zip(op_all(), comp_all()):
      assert (a - b).norm().item() <= 1e-3 * b.norm().item()
    del got, want

    layer = DCN(LAYERS, typ)
    xin = x0.clone().requires_grad_()
    layer(xin)
    params = [getattr(layer, "%s_%d" % (k, i)) for i in range(LAYERS) for k in ("kernel", "bias")]

    def op_module():
      return torch.autograd.grad(layer(xin), [xin] + params, g)

    def comp_module():
      state = xin
      for i in range(LAYERS):
        state = composed(xin, state, params[2 * i], params[2 * i + 1], typ)
      return torch.autograd.grad(state, [xin] + params, g)

    cases.extend([(typ, d, "layer forward", gemm, 3 * sweep, op_fwd, comp_fwd),
                  (typ, d, "layer forward + gradients", 3 * gemm, 9 * sweep, op_all, comp_all),
                  (typ, d, "%d-layer module, forward + backward" % LAYERS, 3 * LAYERS * gemm, 9 * LAYERS * sweep,
                   op_module, comp_module)])

  for typ in layer_ops.DCN_TYPES:
    for d in DIMS:
      add(typ, d)

  times = {}
  for _ in range(args.repeats):
    for i, case in enumerate(cases):
      times.setdefault((i, "op"), []).append(window(case[5]))
      times.setdefault((i, "torch"), []).append(window(case[6]))

  os.makedirs(args.out, exist_ok=True)
  rows = []
  with open(os.path.join(args.out, "dcn.jsonl"), "w") as f:
    for i, (typ, d, form, flops, nbytes, op, comp) in enumerate(cases):
      rec = {"type": typ, "form": form, "B": B, "d": d, "flops": flops, "min_bytes": nbytes,
             "plan": layer_ops.dcn_plan(B, d, typ)}
      for side, fn in (("op", op), ("torch", comp)):
        ts = times[(i, side)]
        med = statistics.median(ts)
        least = max(flops / PEAK_FLOPS, nbytes / PEAK_BYTES)
        rec[side] = {"us": med * 1e6, "windows_us": [t * 1e6 for t in ts], "spread": (max(ts) - min(ts)) / med,
                     "share_of_bound": least / med, "bound": "matrix pipe" if flops / PEAK_FLOPS > nbytes / PEAK_BYTES
                     else "bandwidth", "peak_allocation_bytes": peak(fn)}
      rec["torch_over_op"] = rec["torch"]["us"] / rec["op"]["us"]
      f.write(json.dumps(rec) + "\n")
      print(json.dumps(rec))
      rows.append(rec)
  with open(os.path.join(args.out, "dcn_table.md"), "w") as f:
    f.write("| type | d | form | op ms | spread | of its bound | op peak MB | torch ms | spread | torch peak MB | "
            "torch / op |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in rows:
      f.write("| %s | %d | %s | %.3f | %.1f %% | %.1f %% (%s) | %.0f | %.3f | %.1f %% | %.0f | %.2fx |\n" %
              (r["type"], r["d"], r["form"], r["op"]["us"] / 1e3, 100 * r["op"]["spread"],
               100 * r["op"]["share_of_bound"], r["op"]["bound"], r["op"]["peak_allocation_bytes"] / 2 ** 20,
               r["torch"]["us"] / 1e3, 100 * r["torch"]["spread"], r["torch"]["peak_allocation_bytes"] / 2 ** 20,
               r["torch_over_op"]))


if __name__ == "__main__":
  main()
