// Host driver of csrc/mhte_bsm_core.h for tests/test_batch_softmax_cpu.py: built with -DMHTE_HOST_ONLY, once plain
// and once under the address and undefined-behaviour sanitizers, and run as a program.
//   consts                the constants and the counter count
//   plan B k              the plan's fields, then its offsets
//   cover B k             walks a sweep as the kernels do (row block, chunk, tile, wavefront, lane, register) and
//                         prints: pairs below B visited, the most often one pair was visited, rows out of the
//                         padded extent (must be 0)
//   merge FILE G          fp32 values from FILE in groups of G: each group's (m, l), merged in order -> lse
//   back FILE k normalize k values g then k values x: the normalisation backward -> k values
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mhte_bsm_core.h"

using namespace mhte;

static std::vector<float> read_floats(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  std::vector<float> v;
  float x;
  while (fread(&x, 4, 1, f) == 1) v.push_back(x);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "consts") {
    printf("max_dim %d\nk_pad %d\ntile %d\nmax_chunks %d\ntarget_groups %d\nfinal_threads %d\ncounters %d\n", kBsmMaxDim,
           kBsmKPad, kBsmTile, kBsmMaxChunks, kBsmTargetGroups, kBsmFinalThreads, int(kBsmCounters));
    return 0;
  }
  if (cmd == "plan" && argc == 4) {
    const BsmPlan p = bsm_plan(atoll(argv[2]), atoi(argv[3]));
    printf("%d %d %d %d %llu %u %u %u %u %llu\n", p.kp, p.nb, p.row_block, p.tile, (unsigned long long)p.bp, p.blocks,
           p.tiles, p.tiles_per_chunk, p.chunks, (unsigned long long)p.bytes);
    const uint64_t offs[] = {p.off_inv_q, p.off_inv_i, p.off_ss_q, p.off_ss_i, p.off_c,   p.off_zd,     p.off_qs,
                             p.off_is,    p.off_ml_m,  p.off_ml_l, p.off_lse,  p.off_dq_part, p.off_di_part};
    const uint64_t rows = p.bp, mat = p.bp * uint64_t(p.kp);
    const uint64_t floats[] = {rows, rows, rows, rows, rows, rows, mat, mat, p.chunks * rows, p.chunks * rows,
                               rows, p.chunks * mat, p.chunks * mat};
    for (int i = 0; i < 13; ++i) printf("%llu %llu\n", (unsigned long long)offs[i], (unsigned long long)(4 * floats[i]));
    return 0;
  }
  if (cmd == "cover" && argc == 4) {
    const long long B = atoll(argv[2]);
    const BsmPlan p = bsm_plan(B, atoi(argv[3]));
    std::vector<unsigned char> seen(size_t(B) * size_t(B), 0);
    unsigned long long out_of_extent = 0;
    for (uint32_t blk = 0; blk < p.blocks; ++blk)
      for (uint32_t c = 0; c < p.chunks; ++c) {
        const uint32_t t0 = c * p.tiles_per_chunk;
        const uint32_t t1 = t0 + p.tiles_per_chunk < p.tiles ? t0 + p.tiles_per_chunk : p.tiles;
        if (t0 >= t1) ++out_of_extent;   // an empty chunk
        for (uint32_t t = t0; t < t1; ++t)
          for (int w = 0; w < p.row_block / 32; ++w)
            for (int lane = 0; lane < 64; ++lane)
              for (int reg = 0; reg < 16; ++reg) {
                const uint64_t row = uint64_t(blk) * p.row_block + 32 * w + (lane & 31);
                const uint64_t col = uint64_t(t) * kBsmTile + bsm_acc_row(reg, lane >> 5);
                if (row >= p.bp || col >= p.bp) ++out_of_extent;
                if (row < uint64_t(B) && col < uint64_t(B)) {
                  unsigned char& s = seen[size_t(row) * size_t(B) + size_t(col)];
                  if (s < 255) ++s;
                }
              }
      }
    unsigned long long visited = 0;
    int most = 0;
    for (unsigned char s : seen) {
      visited += s ? 1 : 0;
      most = s > most ? s : most;
    }
    printf("%llu %d %llu\n", visited, most, out_of_extent);
    return 0;
  }
  if (cmd == "merge" && argc == 4) {
    const std::vector<float> z = read_floats(argv[2]);
    const size_t G = size_t(atoll(argv[3]));
    BsmML all = bsm_empty();
    for (size_t g0 = 0; g0 < z.size(); g0 += G) {
      BsmML part = bsm_empty();
      float m = -INFINITY;
      for (size_t i = g0; i < z.size() && i < g0 + G; ++i) m = fmaxf(m, z[i]);
      if (m > -INFINITY) {
        float l = 0.f;
        for (size_t i = g0; i < z.size() && i < g0 + G; ++i) l += expf(z[i] - m);
        part = BsmML{m, l};
      }
      all = bsm_merge(all, part);
    }
    printf("%.9g %.9g %.9g\n", all.m, all.l, bsm_lse(all));
    return 0;
  }
  if (cmd == "back" && argc == 5) {
    const std::vector<float> v = read_floats(argv[2]);
    const int k = atoi(argv[3]);
    const bool normalize = atoi(argv[4]) != 0;
    if (int(v.size()) != 2 * k) return 2;
    const float* g = v.data();
    const float* x = v.data() + k;
    float s = 0.f;
    for (int i = 0; i < k; ++i) s = fmaf(x[i], x[i], s);
    const float inv = normalize ? bsm_inv(s) : 1.f;
    float dot = 0.f;
    for (int i = 0; i < k; ++i) dot = fmaf(x[i] * inv, g[i], dot);
    for (int i = 0; i < k; ++i) {
      const float dx = normalize ? bsm_dx(g[i], x[i] * inv, dot, inv, bsm_eps_branch(s)) : g[i];
      printf("%.9g\n", bsm_pos_zero(dx));
    }
    printf("%.9g %.9g\n", inv, bsm_c(x[0]));
    return 0;
  }
  return 2;
}
