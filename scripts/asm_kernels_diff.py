#!/usr/bin/env python3
"""Compares the gfx950 assembly of two builds kernel by kernel.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC -save-temps \\
        -o libmhte.so monolith_amd/csrc/mhte.hip          # in two directories, one per tree
  scripts/asm_kernels_diff.py A/mhte-hip-amdgcn-amd-amdhsa-gfx950.s B/mhte-hip-amdgcn-amd-amdhsa-gfx950.s

Prints the number of kernels (`.amdhsa_kernel` symbols) in each file, the symbols only one of them has and
the kernels whose bodies differ.  A body is the text between the function's label and its end label;
comments are dropped, and so is the function's ordinal inside block and jump-table labels (.LBB<n>_,
.LJTI<n>_, .Lfunc_end<n>, .Lpost_getpc<n>), since it only says where in the file the function was emitted: what is compared
is every label, directive and instruction of the body.  Exit status 0: same symbols, same bodies.
"""
import re
import sys


def kernels(path):
  text = open(path).read()
  names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
  bodies = {}
  for m in re.finditer(r"^(\S+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
    if m.group(1) in names:
      body = re.sub(r"\.(LBB|LJTI|Lfunc_end|Ltmp|Lpost_getpc)\d+", r".\1", m.group(2))
      lines = (ln.split(";", 1)[0].rstrip() for ln in body.split("\n"))   # (comments carry it too)
      bodies[m.group(1)] = "\n".join(ln for ln in lines if ln)
  return names, bodies


def main():
  (na, ba), (nb, bb) = kernels(sys.argv[1]), kernels(sys.argv[2])
  print("kernels: %d and %d" % (len(na), len(nb)))
  only_a, only_b = sorted(na - nb), sorted(nb - na)
  for n in only_a:
    print("only in the first:", n)
  for n in only_b:
    print("only in the second:", n)
  missing = sorted(n for n in na if n not in ba) + sorted(n for n in nb if n not in bb)
  for n in missing:
    print("no body found:", n)
  differ = sorted(n for n in na & nb if ba.get(n) != bb.get(n))
  for n in differ:
    print("body differs:", n)
  print("bodies compared: %d, identical: %d" % (len(na & nb), len(na & nb) - len(differ)))
  return 1 if (only_a or only_b or differ or missing) else 0


if __name__ == "__main__":
  sys.exit(main())
