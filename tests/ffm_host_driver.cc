// Host driver of tests/test_ffm_cpu.py: the element functions and the form selection of
// monolith_amd/csrc/mhte_ffm_core.h, compiled by g++ with MHTE_HOST_ONLY (no HIP).
//   case <file> <vec>   the file: int32 dot (0 multiply, 1 dot), batch, left_cols, right_cols, grad_cols, dim;
//                       float left[batch][left_cols], right[batch][right_cols], grad[batch][grad_cols].
//                       vec 1: the float element functions; vec 4: the FfmF4 ones (dim and the widths must be
//                       multiples of 4), walked with the strides the kernels use.
//                       Prints out, left_grad, right_grad as hex words, one per line.
//   form <L> <R> <D> <aligned>
//                       "vec lds tile_rows counter" of the forward multiply, forward dot, gradient multiply and
//                       gradient dot forms, one line each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mhte_ffm_core.h"

using mhte::FfmF4;

static void dump(const float* x, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    memcpy(&u, x + i, 4);
    printf("%08x\n", u);
  }
}

// V = float or FfmF4; the buffers are 16-byte aligned and, for FfmF4, every width is a multiple of 4
template <class V>
static void run(bool dot, long long B, long long Lc, long long Rc, long long Gc, int D, const float* left,
                const float* right, const float* grad, float* out, float* lg, float* rg) {
  const int VEC = int(sizeof(V) / 4);
  const int Dv = D / VEC;
  const long long L = Lc / D, R = Rc / D, LDv = L * Dv, RDv = R * Dv;
  const long long oc = dot ? L * R : L * R * D;
  for (long long b = 0; b < B; ++b) {
    const V* lrow = reinterpret_cast<const V*>(left + b * Lc);
    const V* rrow = reinterpret_cast<const V*>(right + b * Rc);
    for (long long l = 0; l < L; ++l)
      for (long long r = 0; r < R; ++r) {
        if (dot) {
          out[b * oc + l * R + r] = mhte::ffm_dot_elem(lrow + l * Dv, rrow + r * Dv, Dv);
        } else {
          V* o = reinterpret_cast<V*>(out + b * oc + (l * R + r) * D);
          for (int kv = 0; kv < Dv; ++kv) o[kv] = mhte::ffm_mul(lrow[l * Dv + kv], rrow[r * Dv + kv]);
        }
      }
    V* lgrow = reinterpret_cast<V*>(lg + b * Lc);
    V* rgrow = reinterpret_cast<V*>(rg + b * Rc);
    for (long long c = 0; c < Lc / VEC; ++c) {
      V v = V{};
      if (c < LDv) {
        const long long l = c / Dv, kv = c % Dv;
        if (dot)
          v = mhte::ffm_grad_elem<V>(grad + b * Gc + l * R, 1, rrow + kv, Dv, int(R));
        else
          v = mhte::ffm_grad_elem<V>(reinterpret_cast<const V*>(grad + b * Gc) + l * RDv + kv, Dv, rrow + kv, Dv, int(R));
      }
      lgrow[c] = v;
    }
    for (long long c = 0; c < Rc / VEC; ++c) {
      V v = V{};
      if (c < RDv) {
        const long long r = c / Dv, kv = c % Dv;
        if (dot)
          v = mhte::ffm_grad_elem<V>(grad + b * Gc + r, R, lrow + kv, Dv, int(L));
        else
          v = mhte::ffm_grad_elem<V>(reinterpret_cast<const V*>(grad + b * Gc) + r * Dv + kv, RDv, lrow + kv, Dv, int(L));
      }
      rgrow[c] = v;
    }
  }
}

static int run_case(const char* path, int vec) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  int32_t h[6];
  if (fread(h, 4, 6, f) != 6) return 2;
  const bool dot = h[0] != 0;
  const long long B = h[1], Lc = h[2], Rc = h[3], Gc = h[4];
  const int D = h[5];
  const long long L = Lc / D, R = Rc / D, oc = dot ? L * R : L * R * D;
  if (vec == 4 && (D % 4 || Lc % 4 || Rc % 4 || (!dot && Gc % 4))) return 3;
  // (FfmF4 storage: 16-byte aligned)
  std::vector<FfmF4> left(B * Lc / 4 + 1), right(B * Rc / 4 + 1), grad(B * Gc / 4 + 1), out(B * oc / 4 + 1),
      lg(B * Lc / 4 + 1), rg(B * Rc / 4 + 1);
  float* pl = reinterpret_cast<float*>(left.data());
  float* pr = reinterpret_cast<float*>(right.data());
  float* pg = reinterpret_cast<float*>(grad.data());
  if (fread(pl, 4, B * Lc, f) != size_t(B * Lc) || fread(pr, 4, B * Rc, f) != size_t(B * Rc) ||
      fread(pg, 4, B * Gc, f) != size_t(B * Gc))
    return 2;
  fclose(f);
  float* po = reinterpret_cast<float*>(out.data());
  float* plg = reinterpret_cast<float*>(lg.data());
  float* prg = reinterpret_cast<float*>(rg.data());
  memset(plg, 0xff, B * Lc * 4);   // (NaN: every element must be written)
  memset(prg, 0xff, B * Rc * 4);
  memset(po, 0xff, B * oc * 4);
  if (vec == 4)
    run<FfmF4>(dot, B, Lc, Rc, Gc, D, pl, pr, pg, po, plg, prg);
  else
    run<float>(dot, B, Lc, Rc, Gc, D, pl, pr, pg, po, plg, prg);
  dump(po, B * oc);
  dump(plg, B * Lc);
  dump(prg, B * Rc);
  return 0;
}

static int run_form(char** argv) {
  const long long L = atoll(argv[2]), R = atoll(argv[3]), D = atoll(argv[4]);
  const bool aligned = atoi(argv[5]) != 0;
  for (int kernel = 0; kernel < 2; ++kernel)
    for (int dot = 0; dot < 2; ++dot) {
      const mhte::FfmForm f = kernel == mhte::kFfmForward ? mhte::ffm_forward_form(L, R, D, aligned)
                                                          : mhte::ffm_grad_form(L, R, D, dot != 0, aligned);
      printf("%d %d %d %d\n", f.vec, f.lds, f.tile_rows, mhte::ffm_counter_index(kernel, dot, f));
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "case")) return run_case(argv[2], atoi(argv[3]));
  if (argc == 6 && !strcmp(argv[1], "form")) return run_form(argv);
  fprintf(stderr, "usage: %s case <file> <vec> | form <L> <R> <D> <aligned>\n", argv[0]);
  return 1;
}
