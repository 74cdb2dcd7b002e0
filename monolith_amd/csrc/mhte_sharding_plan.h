// Plan arithmetic of the fused-layout packer (mhte_sharding_host.h): the checks of a call's feature table and the
// index bases every kernel of the launch sequence reads — where a feature's ids and rows start in the call's
// global numbering, the tables' first pre-output index (get_feature_cfg of the reference's test,
// native_training/fused_embedding_to_layout_test.py:122-175; the op: data/kernels/parse_sparse_feature.cc:106-155)
// and the features in table-major order.  Plain host C++: compiled by hipcc inside mhte.hip and, alone, by
// tests/sharding_plan_host_driver.cc (g++, also under the sanitizers).
#ifndef MHTE_SHARDING_PLAN_H_
#define MHTE_SHARDING_PLAN_H_

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/monolith_amd_hash_table.h"

namespace mhte {

constexpr int32_t kShardMaxPs = 1024;   // (parse_sparse_feature.cc has no bound; one digit pass of the group sort has)

struct ShardSlot {   // a feature seen from its table: entry `ft` of the table-major order
  uint32_t pre;      // the table's first pre-output index (output_pre_index, :139-149)
  uint32_t tfc;      // table_feature_count
  uint32_t j;        // feature_in_table_index
  uint32_t t;        // table_index
};

struct ShardPlan {
  std::vector<uint32_t> id_base, row_base;   // [F + 1]: exclusive sums of n_ids / n_rows in feature order
  std::vector<uint32_t> ft;                  // [F]: the feature's place in table-major order
  std::vector<ShardSlot> slot;               // [F]: by ft
  uint32_t n = 0, rows = 0, n_pre = 0, n_lists = 0;
};

// "" or what is wrong with the call
static inline std::string sharding_plan(const mhte_shard_feature* feat, int32_t n_features,
                                        const int32_t* table_feature_count, int32_t n_tables, int32_t ps_num,
                                        ShardPlan& P) {
  if (ps_num < 1 || ps_num > kShardMaxPs)
    return "ps_num must be in [1, " + std::to_string(kShardMaxPs) + "], got " + std::to_string(ps_num);
  if (n_features < 1) return "n_features must be >= 1, got " + std::to_string(n_features);
  if (n_tables < 1 || n_tables > n_features)
    return "n_tables must be in [1, n_features], got " + std::to_string(n_tables);
  if (!feat) return "null argument: features";
  if (!table_feature_count) return "null argument: table_feature_count";
  std::vector<uint32_t> first(size_t(n_tables) + 1, 0);   // the table's first feature in table-major order
  for (int32_t t = 0; t < n_tables; ++t) {
    if (table_feature_count[t] < 1 || table_feature_count[t] > n_features)
      return "table " + std::to_string(t) + " must hold between 1 and n_features features, got " +
             std::to_string(table_feature_count[t]);
    first[size_t(t) + 1] = first[size_t(t)] + uint32_t(table_feature_count[t]);
    if (first[size_t(t) + 1] > uint32_t(n_features)) break;
  }
  if (first[size_t(n_tables)] != uint32_t(n_features))
    return "the tables' feature counts must add up to n_features = " + std::to_string(n_features);
  if (int64_t(n_features) * ps_num >= (1ll << 31) - 1) return "n_features * ps_num must stay below 2^31 - 1";
  P.id_base.assign(size_t(n_features) + 1, 0);
  P.row_base.assign(size_t(n_features) + 1, 0);
  P.ft.assign(size_t(n_features), 0);
  P.slot.assign(size_t(n_features), ShardSlot{0, 0, 0, 0});
  std::vector<char> seen(size_t(n_features), 0);
  int64_t n = 0, rows = 0;
  for (int32_t f = 0; f < n_features; ++f) {
    const mhte_shard_feature& x = feat[f];
    const std::string who = "feature " + std::to_string(f);
    if (x.table_index < 0 || x.table_index >= n_tables)
      return who + ": table_index " + std::to_string(x.table_index) + " is outside [0, n_tables)";
    const int32_t tfc = table_feature_count[x.table_index];
    if (x.feature_in_table_index < 0 || x.feature_in_table_index >= tfc)
      return who + ": feature_in_table_index " + std::to_string(x.feature_in_table_index) +
             " is outside [0, table_feature_count)";
    const uint32_t ft = first[size_t(x.table_index)] + uint32_t(x.feature_in_table_index);
    if (seen[ft]) return who + ": another feature has its table_index and feature_in_table_index";
    seen[ft] = 1;
    if (x.n_ids < 0) return who + ": n_ids must be >= 0, got " + std::to_string(x.n_ids);
    if (x.n_ids > (1ll << 32) - 1)   // (the low word of fid_offset is the rank)
      return who + ": more than 2^32 - 1 ids in a (feature, shard) do not fit fid_offset's 32-bit rank, got " +
             std::to_string(x.n_ids) + " ids";
    if (x.n_rows < 0) return who + ": n_rows must be >= 0, got " + std::to_string(x.n_rows);
    if (x.shared && x.n_rows > 1) return who + ": a shared feature has one row, got " + std::to_string(x.n_rows);
    if (x.n_rows == 0 && x.n_ids != 0) return who + ": ids without rows";
    if ((x.n_ids > 0 && !x.values) || (x.n_rows > 0 && !x.row_splits)) return who + ": null argument";
    if ((reinterpret_cast<uintptr_t>(x.values) | reinterpret_cast<uintptr_t>(x.row_splits)) & 7u)
      return who + ": values and row_splits must be 8-byte aligned";
    P.ft[size_t(f)] = ft;
    P.slot[ft] = ShardSlot{first[size_t(x.table_index)] * uint32_t(ps_num), uint32_t(tfc),
                           uint32_t(x.feature_in_table_index), uint32_t(x.table_index)};
    n += x.n_ids;
    rows += x.n_rows;
    if (n >= (1ll << 31) - 1) return "the ids of a call must stay below 2^31 - 1, got " + std::to_string(n) + " so far";
    if (rows >= (1ll << 31) - 2) return "the rows of a call must stay below 2^31 - 2";
    P.id_base[size_t(f) + 1] = uint32_t(n);
    P.row_base[size_t(f) + 1] = uint32_t(rows);
  }
  P.n = uint32_t(n);
  P.rows = uint32_t(rows);
  P.n_pre = uint32_t(n_features) * uint32_t(ps_num);
  P.n_lists = uint32_t(n_tables) * uint32_t(ps_num);
  return "";
}

}  // namespace mhte
#endif  // MHTE_SHARDING_PLAN_H_
