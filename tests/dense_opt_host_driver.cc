// Host driver of tests/test_dense_optimizers_cpu.py: the element functions and the chunk table of
// monolith_amd/csrc/mhte_dense_opt_core.h, compiled by g++ with MHTE_HOST_ONLY (no HIP).
//   steps <file>   the file: int32 kind (0 adamom, 1 adamom v2, 2 rmsprop, 3 rmsprop v2), dim, steps;
//                  float grad_scale, lr, a, b, eps, wd; float var0[dim]; float g[steps][dim].
//                  Prints var, then m, v (, c) as hex words.
//   table <align> <null index> <len> ...
//                  the chunk table of the list source with a NULL gradient at <null index> (-1: none; -2: the
//                  flat source).  Prints "n_entries n_chunks" and one line "index len off chunk0 ok" per entry:
//                  index = the variable's place in the list (vars[i] is the address i + 1 here), ok = the
//                  entry carries that variable's gradient (none with the flat source).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mhte_dense_opt_core.h"

static void dump(const std::vector<float>& x) {
  for (float f : x) {
    uint32_t u;
    memcpy(&u, &f, 4);
    printf("%08x\n", u);
  }
}

static int run_steps(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  int32_t head[3];
  float hy[6];
  if (fread(head, 4, 3, f) != 3 || fread(hy, 4, 6, f) != 6) return 2;
  const int kind = head[0], dim = head[1], steps = head[2];
  std::vector<float> var(dim), m(dim, 0.f), v(dim, 0.f), c(dim, 0.f), g(size_t(steps) * dim);
  if (fread(var.data(), 4, dim, f) != size_t(dim) || fread(g.data(), 4, g.size(), f) != g.size()) return 2;
  fclose(f);
  const mhte::DenseOptHyper h{hy[0], hy[1], hy[2], hy[3], hy[4], hy[5]};
  for (int s = 0; s < steps; ++s)
    for (int k = 0; k < dim; ++k) {
      const float g0 = g[size_t(s) * dim + k];
      if (kind < 2)
        mhte::dense_adamom_step(var[k], m[k], v[k], c[k], g0, h, /*update_slots=*/true, kind == 1);
      else
        mhte::dense_rmsprop_step(var[k], m[k], v[k], g0, h, kind == 3);
    }
  dump(var);
  dump(m);
  dump(v);
  if (kind < 2) dump(c);
  return 0;
}

static int run_table(int argc, char** argv) {
  const int32_t align = atoi(argv[2]);
  const int null_at = atoi(argv[3]);
  std::vector<int64_t> lens;
  for (int i = 4; i < argc; ++i) lens.push_back(atoll(argv[i]));
  const int32_t n = int32_t(lens.size());
  std::vector<float*> vars(n);
  std::vector<const float*> grads(n);
  for (int32_t i = 0; i < n; ++i) {   // (addresses that are only compared, never followed)
    vars[i] = reinterpret_cast<float*>(uintptr_t(i + 1));
    grads[i] = i == null_at ? nullptr : reinterpret_cast<const float*>(uintptr_t(i + 1));
  }
  std::vector<mhte::DenseOptEntry> e;
  uint32_t chunks = 0;
  if (!mhte::dense_opt_table(vars.data(), null_at == -2 ? nullptr : grads.data(), lens.data(), n, align, e, &chunks)) {
    printf("too many chunks\n");
    return 0;
  }
  printf("%zu %u\n", e.size(), chunks);
  for (const mhte::DenseOptEntry& x : e) {
    const bool grad_ok = null_at == -2 ? x.grad == nullptr : uintptr_t(x.grad) == uintptr_t(x.var);
    printf("%lld %lld %lld %u %d\n", (long long)(uintptr_t(x.var) - 1), x.len, x.off, x.chunk0, grad_ok ? 1 : 0);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "steps")) return run_steps(argv[2]);
  if (argc >= 4 && !strcmp(argv[1], "table")) return run_table(argc, argv);
  fprintf(stderr, "usage: %s steps <file> | table <align> <null index> <len> ...\n", argv[0]);
  return 1;
}
