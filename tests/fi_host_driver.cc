// Host driver of csrc/mhte_fi_core.h for tests/test_feature_insight_cpu.py: built by g++ with MHTE_HOST_ONLY, it
// runs the very element, chain and plan functions the kernels call.
//   consts                                   the constants, one "name value" per line
//   plan B E K F                             the plan's fields on one line
//   op IN OUT B K F s_0 .. s_{F-1}           IN: input [B, E], weight [E, K], grad [B, F K] as raw fp32;
//                                            OUT: out [B, F K], agg [B, F], input_grad [B, E], weight_grad [E, K]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mhte_fi_core.h"

using namespace mhte;

static int fail(const char* what) {
  fprintf(stderr, "fi_host_driver: %s\n", what);
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return fail("no command");
  if (!strcmp(argv[1], "consts")) {
    printf("tile %d\nstage %d\nlanes %d\ninline %d\nmax_segments %d\nmax_slabs %d\ntarget_groups %d\ncounters %d\n"
           "max_extent %lld\n",
           kFiTile, kFiStage, kFiLanes, kFiInline, kFiMaxSegments, kFiMaxSlabs, kFiTargetGroups, int(kFiCounters),
           kFiMaxExtent);
    return 0;
  }
  if (!strcmp(argv[1], "plan")) {
    if (argc != 6) return fail("plan B E K F");
    const FiPlan p = fi_plan(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]));
    printf("%d %d %d %d %lld %lld %lld %llu %llu\n", p.row_block, p.col_tile, p.stage, p.inline_segments, p.groups,
           p.slab_rows, p.slabs, p.forward_bytes, p.grad_bytes);
    return 0;
  }
  if (!strcmp(argv[1], "op")) {
    if (argc < 8) return fail("op IN OUT B K F sizes...");
    const long long B = atoll(argv[4]), K = atoll(argv[5]), F = atoll(argv[6]);
    if (argc != 7 + F) return fail("op: F sizes expected");
    std::vector<long long> off(F + 1, 0);
    for (long long f = 0; f < F; ++f) off[f + 1] = off[f] + atoll(argv[7 + f]);
    const long long E = off[F], FK = F * K;
    std::vector<float> x(B * E), w(E * K), g(B * FK);
    FILE* in = fopen(argv[2], "rb");
    if (!in) return fail("cannot open IN");
    const bool ok = fread(x.data(), 4, x.size(), in) == x.size() && fread(w.data(), 4, w.size(), in) == w.size() &&
                    fread(g.data(), 4, g.size(), in) == g.size();
    fclose(in);
    if (!ok) return fail("IN is short");
    std::vector<float> out(B * FK), agg(B * F), ig(B * E), wg(E * K);
    for (long long b = 0; b < B; ++b)
      for (long long f = 0; f < F; ++f) {
        for (long long k = 0; k < K; ++k)
          out[b * FK + f * K + k] =
              fi_chain(x.data() + b * E + off[f], 1, w.data() + off[f] * K + k, K, off[f + 1] - off[f]);
        agg[b * F + f] = fi_agg(out.data() + b * FK + f * K, int(K));
        for (long long j = off[f]; j < off[f + 1]; ++j)
          ig[b * E + j] = fi_chain(g.data() + b * FK + f * K, 1, w.data() + j * K, 1, K);
      }
    const FiPlan p = fi_plan(B, E, K, F);
    std::vector<float> part(p.slabs);
    for (long long f = 0; f < F; ++f)
      for (long long j = off[f]; j < off[f + 1]; ++j)
        for (long long k = 0; k < K; ++k) {
          for (long long i = 0; i < p.slabs; ++i) {
            const long long b0 = i * p.slab_rows, n = B - b0 < p.slab_rows ? B - b0 : p.slab_rows;
            part[i] = fi_chain(g.data() + b0 * FK + f * K + k, FK, x.data() + b0 * E + j, E, n);
          }
          wg[j * K + k] = fi_slab_sum(part.data(), 1, int(p.slabs));
        }
    FILE* o = fopen(argv[3], "wb");
    if (!o) return fail("cannot open OUT");
    fwrite(out.data(), 4, out.size(), o);
    fwrite(agg.data(), 4, agg.size(), o);
    fwrite(ig.data(), 4, ig.size(), o);
    fwrite(wg.data(), 4, wg.size(), o);
    fclose(o);
    return 0;
  }
  return fail("unknown command");
}
