// Host driver of tests/test_layout_plan_cpu.py: the plan of fused_embedding_to_layout
// (monolith_amd/csrc/mhte_layout_plan.h), compiled by g++ alone (no HIP).  The function run here is the one
// mhte_embedding_to_layout(_grad) calls before it enqueues anything.  Reads the call from stdin, one record a line:
//   call <forward> <batch> <n_fid> <n_feature> <n_nfl> <flags> <rows_form> <pool_atomics> <n_emb> <n_outputs>
//   emb <row floats> <floats> <address bits>      (address bits: added to a 4096-aligned address)
//   out <floats> <address bits>
//   slice <feature_idx> <start> <dim> <pooling> <max_seq> <out_type> <out_index> <out_offset> <out_row_floats>
// and prints "refused: <message>", or "ext <0|1>", "skip <0|1 per output>", then either "grouped" with its tasks
// ("t": the LayoutTask's fields in order), "t_off" and "t_idx", or per launch "launch <rows|copy|general> mask=<hex>"
// with its tasks and units ("u <first> <count> <addn>").  Exit status 1: a launch that carries zero runs or a
// mask has another form than rows.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "mhte_layout_plan.h"

static void print_task(const mhte::LayoutTask& t) {
  printf("t %d %d %d %d %d %d %d %d\n", t.nfl_idx, t.start, t.dim, t.pooling, t.max_seq, t.out_index, t.out_offset,
         t.out_stride);
}

int main() {
  mhte::LayoutCall c{};
  std::vector<int32_t> emb_stride;
  std::vector<int64_t> emb_count, output_len;
  std::vector<const void*> embeddings, outputs;
  std::vector<mhte_layout_slice> slices;
  char line[256];
  bool have_call = false;
  while (fgets(line, sizeof line, stdin)) {
    long long a[10];
    mhte_layout_slice s{};
    if (sscanf(line, "call %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6,
               a + 7, a + 8, a + 9) == 10) {
      c.forward = a[0] != 0;
      c.batch = int32_t(a[1]);
      c.n_fid = a[2];
      c.n_feature = a[3];
      c.n_nfl = int32_t(a[4]);
      c.flags = int32_t(a[5]);
      c.rows_form = a[6] != 0;
      c.pool_atomics = a[7] != 0;
      c.n_emb = int32_t(a[8]);
      c.n_outputs = int32_t(a[9]);
      have_call = true;
    } else if (sscanf(line, "emb %lld %lld %lld", a, a + 1, a + 2) == 3) {
      emb_stride.push_back(int32_t(a[0]));
      emb_count.push_back(a[1]);
      embeddings.push_back(reinterpret_cast<const void*>(uintptr_t(4096) * (embeddings.size() + 1) + uintptr_t(a[2])));
    } else if (sscanf(line, "out %lld %lld", a, a + 1) == 2) {
      output_len.push_back(a[0]);
      outputs.push_back(reinterpret_cast<const void*>(uintptr_t(1) << 30 | (uintptr_t(4096) * outputs.size() + uintptr_t(a[1]))));
    } else if (sscanf(line, "slice %d %d %d %d %d %d %d %d %d", &s.feature_idx, &s.start, &s.dim, &s.pooling,
                      &s.max_sequence_length, &s.out_type, &s.out_index, &s.out_offset, &s.out_row_floats) == 9) {
      slices.push_back(s);
    } else if (line[0] != '\n' && line[0] != '#') {
      return 2;
    }
  }
  if (!have_call) return 2;
  c.emb_stride = emb_stride.data();
  c.emb_count = emb_count.data();
  c.embeddings = embeddings.data();
  c.outputs = outputs.data();
  c.output_len = output_len.data();
  c.slices = slices.data();
  c.n_slices = int32_t(slices.size());
  mhte::LayoutPlan P;
  const std::string bad = mhte::layout_plan(c, P);
  if (!bad.empty()) {
    printf("refused: %s\n", bad.c_str());
    return 0;
  }
  printf("ext %d\nskip", P.ext ? 1 : 0);
  for (char s : P.skip_fill) printf(" %d", int(s));
  printf("\n");
  if (P.grouped) {
    printf("grouped\n");
    for (auto& t : P.tasks) print_task(t);
    printf("t_off");
    for (uint32_t v : P.t_off) printf(" %u", v);
    printf("\nt_idx");
    for (uint32_t v : P.t_idx) printf(" %u", v);
    printf("\n");
  }
  static const char* const kForm[] = {"rows", "copy", "general"};
  int status = 0;
  for (auto& L : P.launches) {
    printf("launch %s mask=%x\n", kForm[L.form], unsigned(L.zero_missing));
    bool zero_run = false;
    for (int32_t q = 0; q < L.n_tasks; ++q) {
      print_task(L.task[q]);
      zero_run = zero_run || L.task[q].pooling == mhte::kPoolZeroFill;
    }
    for (int32_t q = 0; q < L.n_units; ++q) printf("u %d %d %d\n", L.unit[q].first, L.unit[q].count, L.unit[q].addn);
    if ((zero_run || L.zero_missing != 0) && L.form != mhte::kLayoutFormRows) status = 1;
  }
  return status;
}
