// Host driver of tests/test_sharding_fids_cpu.py: the plan arithmetic of the fused-layout packer
// (monolith_amd/csrc/mhte_sharding_plan.h), compiled by g++ alone (no HIP).  The function run here is the one
// mhte_sharding_sparse_fids calls before its first launch.
//   <ps_num> <count,count,...> <n_ids:n_rows:shared:table_index:feature_in_table_index> ...
// prints "n rows n_pre n_lists", then per feature "id_base row_base ft pre tfc j"; or "refused: <message>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mhte_sharding_plan.h"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int32_t ps = int32_t(atoi(argv[1]));
  std::vector<int32_t> tfc;
  for (char* p = strtok(argv[2], ","); p; p = strtok(nullptr, ",")) tfc.push_back(int32_t(atoi(p)));
  std::vector<mhte_shard_feature> feat;
  static int64_t somewhere[2];
  for (int i = 3; i < argc; ++i) {
    long long n_ids = 0;
    int n_rows = 0, shared = 0, t = 0, j = 0;
    if (sscanf(argv[i], "%lld:%d:%d:%d:%d", &n_ids, &n_rows, &shared, &t, &j) != 5) return 2;
    feat.push_back(mhte_shard_feature{somewhere, somewhere, int64_t(n_ids), n_rows, shared, t, j});
  }
  mhte::ShardPlan P;
  const std::string bad = mhte::sharding_plan(feat.data(), int32_t(feat.size()), tfc.data(), int32_t(tfc.size()), ps, P);
  if (!bad.empty()) {
    printf("refused: %s\n", bad.c_str());
    return 0;
  }
  printf("%u %u %u %u\n", P.n, P.rows, P.n_pre, P.n_lists);
  for (size_t f = 0; f < feat.size(); ++f) {
    const mhte::ShardSlot& q = P.slot[P.ft[f]];
    printf("%u %u %u %u %u %u\n", P.id_base[f], P.row_base[f], P.ft[f], q.pre, q.tfc, q.j);
  }
  return 0;
}
