"""Measurements of the dense optimizers, one JSON object per line and a markdown table under
profiles/dense_optimizers/ (or --out DIR), on two variable sets:

  * "dlrm26": the shapes of scripts/clip_bench.py's gradient set (26 tensors [65 536, dim] with dims 16 / 32 / 64
    plus the dense tower's weights and biases, about 64 M floats) — bandwidth;
  * "mlp": the eight tensors of DenseMlp([1024, 1024, 512, 256, 1]) (1.8 M floats) — where the launch count matters.

Each optimizer (Adamom, Adamom V2, RMSprop, RMSprop V2) runs with each gradient source: the list of fp32
tensors, the flat fp32 buffer and the flat fp16 buffer.  Algorithmic bytes per element: Adamom reads var, m, v,
c and the gradient and writes var, m, v, c — 36 B with an fp32 gradient, 34 B with an fp16 one; RMSprop 28 B and
26 B.  Fractions are of the 8 TB/s HBM peak.

Baselines, measured in the same run — what a user of the library had to do before these entry points existed,
starting from the fp16 flat buffer of the allreduce: aligned_flat_split's decode (one launch, a new fp32
buffer), then the update restated with torch ops (a) variable by variable and (b) with torch._foreach_* over
the lists, where the installed torch has them.  Their algorithmic bytes are counted as the fused kernel's
(34 B / 26 B): the figure says how far the same work is from the peak, not what they really move.

All cases take turns in every round of one process (interleaved); a case's figure is the median of its
rounds, each round the wall time of `reps` back-to-back calls and one synchronisation, divided by reps.
    python scripts/dense_opt_bench.py [--out DIR] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_bench import PEAK, gradient_set, timed  # noqa: E402
from monolith_amd import distribution_ops as D  # noqa: E402
from monolith_amd import optimizers as O  # noqa: E402

LR, WD = 5e-6, 0.01
ADA, MOM, EPS_A = 0.9999, 0.99, 1e-6
B1, B2, EPS_R = 0.99, 0.999, 1e-8
KINDS = {"adamom": (O.AdamomOptimizer, False, 36, 34), "adamom v2": (O.AdamomOptimizer, True, 36, 34),
         "rmsprop": (O.RmspropOptimizer, False, 28, 26), "rmsprop v2": (O.RmspropOptimizer, True, 28, 26)}


def mlp_set():
  g = torch.Generator(device="cuda").manual_seed(6)
  widths = [1024, 1024, 512, 256, 1]
  ts = []
  for a, b in zip(widths[:-1], widths[1:]):
    ts.append(torch.randn(b, a, device="cuda", generator=g))
    ts.append(torch.randn(b, device="cuda", generator=g))
  return ts


class TorchBaseline:
  """The update restated with torch ops on per-variable slots, from the fp16 flat buffer: the decode of
  aligned_flat_split, then elementwise ops — variable by variable, or torch._foreach_* over the lists."""

  def __init__(self, kind, shapes, flat16, foreach):
    self.kind, self.flat16, self.foreach = kind, flat16, foreach
    self.vars = [torch.randn(s, device="cuda") for s in shapes]
    self.m = [torch.zeros_like(v) for v in self.vars]
    self.v = [torch.zeros_like(v) for v in self.vars]
    self.c = [torch.zeros_like(v) for v in self.vars]

  def __call__(self):
    grads = D.aligned_flat_split(self.vars, self.flat16, post_scale=0.5)
    if self.foreach:
      return self._adamom_foreach(grads) if self.kind == "adamom" else self._rmsprop_foreach(grads)
    for var, m, v, c, g in zip(self.vars, self.m, self.v, self.c, grads):
      g = torch.add(g, var, alpha=WD)
      if self.kind == "adamom":
        m.mul_(MOM).add_(g, alpha=1 - MOM)
        v.mul_(ADA).addcmul_(g, g)
        c.mul_(ADA).add_(1.0)
        var.addcmul_(m, torch.div(v, c).add_(EPS_A).rsqrt_(), value=-LR)
      else:
        v.mul_(B2).addcmul_(g, g, value=1 - B2)
        m.mul_(B1).addcmul_(g, torch.add(v, EPS_R).rsqrt_(), value=LR)
        var.sub_(m)

  def _adamom_foreach(self, grads):
    gs = torch._foreach_add(grads, self.vars, alpha=WD)
    torch._foreach_mul_(self.m, MOM)
    torch._foreach_add_(self.m, gs, alpha=1 - MOM)
    torch._foreach_mul_(self.v, ADA)
    torch._foreach_addcmul_(self.v, gs, gs)
    torch._foreach_mul_(self.c, ADA)
    torch._foreach_add_(self.c, 1.0)
    d = torch._foreach_div(self.v, self.c)
    torch._foreach_add_(d, EPS_A)
    torch._foreach_sqrt_(d)
    torch._foreach_reciprocal_(d)
    torch._foreach_addcmul_(self.vars, self.m, d, value=-LR)

  def _rmsprop_foreach(self, grads):
    gs = torch._foreach_add(grads, self.vars, alpha=WD)
    torch._foreach_mul_(self.v, B2)
    torch._foreach_addcmul_(self.v, gs, gs, value=1 - B2)
    d = torch._foreach_add(self.v, EPS_R)
    torch._foreach_sqrt_(d)
    torch._foreach_reciprocal_(d)
    torch._foreach_mul_(self.m, B1)
    torch._foreach_addcmul_(self.m, gs, d, value=LR)
    torch._foreach_sub_(self.vars, self.m)


def cases_of(set_name, templates):
  shapes = [tuple(t.shape) for t in templates]
  n = sum(t.numel() for t in templates)
  grads = [torch.randn(s, device="cuda") * 0.1 for s in shapes]
  flat32 = D.aligned_flat_concat(grads)
  flat16 = D.aligned_flat_concat(grads, wire_dtype=torch.float16)
  scale = torch.tensor(0.5, device="cuda")
  cases = []
  for kind, (cls, v2, b32, b16) in KINDS.items():
    hyper = (dict(ada_decay=ADA, mom_decay=MOM, epsilon=EPS_A) if cls is O.AdamomOptimizer else
             dict(beta1=B1, beta2=B2, epsilon=EPS_R))
    for source in ("list", "flat fp32", "flat fp16"):
      opt = cls(learning_rate=LR, weight_decay=WD, use_v2=v2, **hyper)
      tvars = [torch.randn(s, device="cuda") for s in shapes]
      if source == "list":
        pairs = list(zip(grads, tvars))
        fn = (lambda opt=opt, pairs=pairs: opt.apply_gradients(pairs, grad_scale=scale))
      else:
        flat = flat32 if source == "flat fp32" else flat16
        fn = (lambda opt=opt, flat=flat, tvars=tvars: opt.apply_flat(flat, variables=tvars, post_scale=0.5))
      cases.append(dict(set=set_name, name="%s, %s" % (kind, source), kind=kind, source=source, fn=fn,
                        alg=(b16 if source == "flat fp16" else b32) * n, n=n, tensors=len(shapes)))
    # the fp16 flat buffer without the fused source: aligned_flat_split's decode, then the list form
    opt = cls(learning_rate=LR, weight_decay=WD, use_v2=v2, **hyper)
    tvars = [torch.randn(s, device="cuda") for s in shapes]
    fn = (lambda opt=opt, tvars=tvars: opt.apply_gradients(
        list(zip(D.aligned_flat_split(tvars, flat16, post_scale=0.5), tvars))))
    cases.append(dict(set=set_name, name="%s, decode then list" % kind, kind=kind, source="decode then list", fn=fn,
                      alg=b16 * n, n=n, tensors=len(shapes)))
  forms = [("per variable", False)]
  if all(hasattr(torch, f) for f in ("_foreach_add", "_foreach_addcmul_", "_foreach_div", "_foreach_sqrt_",
                                     "_foreach_reciprocal_", "_foreach_sub_")):
    forms.append(("torch._foreach", True))
  for kind in ("adamom", "rmsprop"):
    for label, foreach in forms:
      cases.append(dict(set=set_name, name="baseline: decode + torch ops %s, %s" % (label, kind), kind=kind,
                        source="baseline " + label, fn=TorchBaseline(kind, shapes, flat16, foreach),
                        alg=KINDS[kind][3] * n, n=n, tensors=len(shapes)))
  return cases


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "profiles", "dense_optimizers"))
  p.add_argument("--quick", action="store_true")
  a = p.parse_args()
  torch.cuda.set_device(0)
  rounds, reps = (3, 3) if a.quick else (7, 10)
  cases = cases_of("dlrm26", gradient_set()) + cases_of("mlp", mlp_set())
  for c in cases:   # warm-up: slots, workspace, allocator, code objects
    timed(c["fn"], 2)
    c["runs"] = []
  for _ in range(rounds):
    for c in cases:
      c["runs"].append(timed(c["fn"], reps))
  lines = []
  med = {(c["set"], c["name"]): statistics.median(c["runs"]) for c in cases}
  for c in cases:
    m = med[(c["set"], c["name"])]
    rec = {"set": c["set"], "name": c["name"], "tensors": c["tensors"], "floats": c["n"], "us": round(m * 1e6, 1),
           "alg_bytes": c["alg"], "GBps": round(c["alg"] / m / 1e9, 1), "peak_fraction": round(c["alg"] / m / PEAK, 3),
           "us_min": round(min(c["runs"]) * 1e6, 1), "us_max": round(max(c["runs"]) * 1e6, 1),
           "us_rounds": [round(x * 1e6, 1) for x in c["runs"]]}
    if not c["source"].startswith("baseline"):
      for other in cases:   # how many times longer the baselines of this optimizer take
        if other["set"] == c["set"] and other["kind"] == c["kind"] and other["source"].startswith("baseline"):
          rec["x_" + other["source"].replace(" ", "_")] = round(med[(other["set"], other["name"])] / m, 2)
    if c["source"] == "flat fp16":   # the fused flat source against decode + the list form of the same kernel
      rec["x_decode_then_list"] = round(med[(c["set"], "%s, decode then list" % c["kind"])] / m, 2)
    lines.append(rec)
  os.makedirs(a.out, exist_ok=True)
  for rec in lines:
    print(json.dumps(rec), flush=True)
  with open(os.path.join(a.out, "dense_opt.jsonl"), "w") as f:
    for rec in lines:
      f.write(json.dumps(rec) + "\n")
  with open(os.path.join(a.out, "dense_opt.md"), "w") as f:
    f.write("# Dense optimizers: per-call times (one MI355X)\n\n"
            "%d rounds of %d calls, all cases interleaved; median of the rounds, with the fastest and the slowest "
            "round.  Algorithmic bytes per element: Adamom 36 (fp32 gradient) / 34 (fp16), RMSprop 28 / 26; the "
            "baselines and `decode then list` are given the fused fp16 kernel's bytes.  `x per variable` / "
            "`x _foreach`: how many times longer the torch baseline of the same optimizer (V1) takes; `x decode "
            "then list`: the same for aligned_flat_split's decode followed by the list form.\n" % (rounds, reps))
    for set_name in ("dlrm26", "mlp"):
      sub = [r for r in lines if r["set"] == set_name]
      f.write("\n## %s: %d tensors, %d floats\n\n"
              "| case | µs | min .. max (µs) | GB/s | of 8 TB/s | x per variable | x _foreach | x decode then list |\n"
              "|---|---|---|---|---|---|---|---|\n" % (set_name, sub[0]["tensors"], sub[0]["floats"]))
      for r in sub:
        f.write("| %s | %s | %s .. %s | %s | %.1f %% | %s | %s | %s |\n" %
                (r["name"], r["us"], r["us_min"], r["us_max"], r["GBps"], 100 * r["peak_fraction"],
                 r.get("x_baseline_per_variable", ""), r.get("x_baseline_torch._foreach", ""),
                 r.get("x_decode_then_list", "")))


if __name__ == "__main__":
  main()
