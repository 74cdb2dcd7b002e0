// Host driver of tests/test_inbatch_auc_cpu.py: the classification, the term functions and the launch plan of
// monolith_amd/csrc/mhte_auc_core.h, compiled by g++ with MHTE_HOST_ONLY (no HIP).
//   consts                 "name value" lines of the tile and chunk constants
//   classify <file>        the file: float32 labels; prints one class per line
//   terms <file>           the file: float32 diffs; prints "t s" as hex words per line, from auc_loss_term and
//                          auc_grad_weight; exits 4 if auc_terms gives other bits than the two
//   split <A> <B> <budget> "a_tiles chunks chunk_len stride"
//   plan <n>               "scan_tiles pair_groups final_groups budget loss_slots bytes", then the offsets
//   pairs <A> <B> <budget> every (a, b) the sweep's work items visit, walked as the pair kernel walks them
//                          (items, threads, stages), one "a b" per line
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mhte_auc_core.h"

using namespace mhte;

static std::vector<float> read_floats(const char* path) {
  std::vector<float> v;
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  float x;
  while (fread(&x, 4, 1, f) == 1) v.push_back(x);
  fclose(f);
  return v;
}
static uint32_t word(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

static int run_pairs(uint32_t A, uint32_t B, uint64_t budget) {
  const AucSplit s = auc_split(A, B, budget);
  if (uint64_t(s.chunks) * s.stride > budget && s.chunks > 1) return 5;   // the partials would not fit
  for (uint64_t k = 0; k < auc_items(s); ++k) {
    const uint32_t c = uint32_t(k / s.a_tiles), at = uint32_t(k % s.a_tiles);
    const uint32_t b0 = c * s.chunk_len, b1 = std::min(B, b0 + s.chunk_len);
    if (b0 >= B) return 6;   // an empty chunk
    for (uint32_t tid = 0; tid < uint32_t(kAucThreads); ++tid) {
      const uint32_t ai = at * uint32_t(kAucTile) + tid;
      if (ai >= A) continue;
      for (uint32_t base = b0; base < b1; base += uint32_t(kAucStage)) {
        const uint32_t cnt = std::min(uint32_t(kAucStage), (b1 - base + 3u) & ~3u);
        for (uint32_t j = 0; j < cnt; ++j)
          if (base + j < b1) printf("%u %u\n", ai, base + j);
      }
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("threads %d\ntile %d\nchunk %d\nstage %d\nscan_tile %d\nmax_groups %d\ngroup_elems %d\nmin_budget %lld\n"
           "counters %d\n",
           kAucThreads, kAucTile, kAucChunk, kAucStage, kAucScanTile, kAucMaxGroups, kAucGroupElems, kAucMinBudget,
           int(kAucCounters));
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "classify")) {
    for (float x : read_floats(argv[2])) printf("%d\n", auc_classify(x));
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "terms")) {
    for (float d : read_floats(argv[2])) {
      float t, s;
      auc_terms(d, &t, &s);
      const float t1 = auc_loss_term(d), s1 = auc_grad_weight(d);
      if (word(t) != word(t1) || word(s) != word(s1)) return 4;
      printf("%08x %08x\n", word(t1), word(s1));
    }
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "split")) {
    const AucSplit s = auc_split(uint32_t(atoll(argv[2])), uint32_t(atoll(argv[3])), uint64_t(atoll(argv[4])));
    printf("%u %u %u %llu\n", s.a_tiles, s.chunks, s.chunk_len, (unsigned long long)s.stride);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "plan")) {
    const AucPlan p = auc_plan(atoll(argv[2]));
    printf("%u %u %u %llu %llu %llu\n", p.scan_tiles, p.pair_groups, p.final_groups, (unsigned long long)p.budget,
           (unsigned long long)p.loss_slots, (unsigned long long)p.bytes);
    printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)p.off_counts,
           (unsigned long long)p.off_tile_counts, (unsigned long long)p.off_tile_offsets,
           (unsigned long long)p.off_pos, (unsigned long long)p.off_neg, (unsigned long long)p.off_rank,
           (unsigned long long)p.off_loss_part, (unsigned long long)p.off_row_part,
           (unsigned long long)p.off_col_part);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "pairs"))
    return run_pairs(uint32_t(atoll(argv[2])), uint32_t(atoll(argv[3])), uint64_t(atoll(argv[4])));
  fprintf(stderr, "usage: %s consts | classify <file> | terms <file> | split <A> <B> <budget> | plan <n> | "
                  "pairs <A> <B> <budget>\n", argv[0]);
  return 1;
}
