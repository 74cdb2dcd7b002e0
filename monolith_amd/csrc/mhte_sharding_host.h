// Host side of the fused-layout packer (mhte_sharding_kernels.h): the checks, the feature table's way to the
// device (one pinned upload), the launch sequence in the workspace's scratch and the one host read.  Included by
// mhte.hip behind mhte_aux_host.h.
#ifndef MHTE_SHARDING_HOST_H_
#define MHTE_SHARDING_HOST_H_

#include "mhte_sharding_kernels.h"

namespace mhte {

struct ShardWs {   // scratch of the packer, one per device, used under AuxWs::mu
  DevBuf<char> table;
  DevBuf<int64_t> ids;
  DevBuf<uint32_t> full, first, slots;
  static ShardWs& of(int device) {
    static std::mutex m;
    static std::map<int, std::unique_ptr<ShardWs>> all;
    std::lock_guard<std::mutex> g(m);
    auto& p = all[device];
    if (!p) p.reset(new ShardWs);
    return *p;
  }
};

static void sharding_sparse_fids(const mhte_shard_feature* features, int32_t n_features,
                                 const int32_t* table_feature_count, int32_t n_tables, int32_t ps_num, int32_t unique,
                                 uint64_t* fid_offset, int32_t* feature_offset, uint32_t* nfl_offset, int64_t* fid_list,
                                 int64_t* key_start, int64_t* row_splits_flat, int64_t* list_bounds, int64_t* host_out,
                                 void* stream) {
  const char* op = "sharding_sparse_fids";
  ShardPlan P;
  const std::string bad = sharding_plan(features, n_features, table_feature_count, n_tables, ps_num, P);
  if (!bad.empty()) arg_bad(op, bad);
  split_check_ptr(op, "fid_offset", fid_offset, P.n > 0, 8);
  split_check_ptr(op, "fid_list", fid_list, P.n > 0, 8);
  split_check_ptr(op, "feature_offset", feature_offset, true, 4);
  split_check_ptr(op, "nfl_offset", nfl_offset, true, 4);
  split_check_ptr(op, "key_start", key_start, true, 8);
  split_check_ptr(op, "row_splits_flat", row_splits_flat, true, 8);
  split_check_ptr(op, "list_bounds", list_bounds, true, 8);
  need_device();
  hipStream_t st = S(stream);
  const uint32_t F = uint32_t(n_features), n = P.n;
  {
    AuxWs& ws = AuxWs::of(current_device());
    ShardWs& sw = ShardWs::of(current_device());
    std::lock_guard<std::mutex> g(ws.mu);
    AuxWs::Use use_(ws, st);
    // ---- the call's tables: the features, then the table-major slots
    const size_t feat_bytes = size_t(F) * sizeof(ShFeat), slot_bytes = size_t(F) * sizeof(ShardSlot);
    std::vector<char> h(feat_bytes + slot_bytes);
    ShFeat* hf = reinterpret_cast<ShFeat*>(h.data());
    for (uint32_t f = 0; f < F; ++f) {
      const mhte_shard_feature& x = features[f];
      const ShardSlot& q = P.slot[P.ft[f]];
      hf[f] = ShFeat{x.values, x.row_splits, P.id_base[f], P.row_base[f], uint32_t(x.n_ids), uint32_t(x.n_rows),
                     P.ft[f], q.pre + q.j, q.tfc, x.shared ? 1u : 0u};
    }
    memcpy(h.data() + feat_bytes, P.slot.data(), slot_bytes);
    sw.table.reserve(h.size());
    PinnedStage::of(current_device()).upload(sw.table.p, h.data(), h.size(), st);
    ShArgs A{};
    A.feat = reinterpret_cast<const ShFeat*>(sw.table.p);
    A.slot = reinterpret_cast<const ShardSlot*>(sw.table.p + feat_bytes);
    A.F = F;
    A.ps = uint32_t(ps_num);
    A.n = n;
    A.rows = P.rows;
    A.n_pre = P.n_pre;
    A.fid_offset = reinterpret_cast<unsigned long long*>(fid_offset);
    A.feature_offset = feature_offset;
    A.nfl_offset = nfl_offset;
    A.fid_list = fid_list;
    A.key_start = key_start;
    A.row_splits_flat = row_splits_flat;
    A.list_bounds = list_bounds;
    HIP_OK(hipMemsetAsync(key_start + P.n_pre + 1, 0, 8, st));   // the status word
    const auto blocks = [](uint64_t items) { return dim3(uint32_t((items + kShThreads - 1) / kShThreads)); };
    if (n) {
      sw.ids.reserve(n);
      sw.full.reserve(n);
      ws.gs_kva.reserve(n);
      ws.k32b.reserve(n);
      ws.seg_pos.reserve(size_t(n) + 1);
      A.ids = sw.ids.p;
      A.full = sw.full.p;
      A.kv = ws.gs_kva.p;
      sh_keys_kernel<<<blocks(n), kShThreads, 0, st>>>(A);
      if (unique) {
        uint64_t cap = 1024;
        while (cap < 2ull * n) cap <<= 1;
        sw.slots.reserve(size_t(cap));
        sw.first.reserve(n);
        A.slots = sw.slots.p;
        A.mask = uint32_t(cap - 1);
        A.first = sw.first.p;
        HIP_OK(hipMemsetAsync(sw.slots.p, 0xff, size_t(cap) * 4, st));
        sh_insert_kernel<<<blocks(n), kShThreads, 0, st>>>(A);
        sh_first_kernel<<<blocks(n), kShThreads, 0, st>>>(A);
      }
      // ---- the stable sort of (sk, g); n_pre itself is a key (the later occurrences, sorted last)
      int bits = 1;
      while ((1ull << bits) <= uint64_t(P.n_pre)) ++bits;
      const int passes = (bits + kGsMaxBits - 1) / kGsMaxBits;
      const int dig = (bits + passes - 1) / passes;
      GsPass G{};
      ws.gs_tiles(G, n);
      if (passes > 1) ws.gs_kvb.reserve(n);
      for (int j = 0; j < passes; ++j) {
        G.shift = uint32_t(j * dig);
        G.bits = uint32_t(std::min(dig, bits - j * dig));
        const bool last = j == passes - 1;
        G.kvin = (j & 1) ? ws.gs_kvb.p : ws.gs_kva.p;
        G.kvout = last ? nullptr : ((j & 1) ? ws.gs_kva.p : ws.gs_kvb.p);
        G.kout = ws.k32b.p;
        G.pout = ws.seg_pos.p;
        gs_hist_kernel<false><<<dim3(G.ntiles), kGsThreads, 0, st>>>(G);
        gs_rowscan_kernel<<<dim3(1u << G.bits), 64, 0, st>>>(G);
        gs_scatter_kernel<false><<<dim3(G.ntiles), kGsThreads, 0, st>>>(G);
      }
      A.skey = ws.k32b.p;
      A.spos = ws.seg_pos.p;
    }
    sh_starts_kernel<<<blocks(uint64_t(P.n_pre) + 1), kShThreads, 0, st>>>(A);
    if (n) {
      sh_emit_kernel<<<blocks(n), kShThreads, 0, st>>>(A);
      if (unique) sh_dups_kernel<<<blocks(n), kShThreads, 0, st>>>(A);
    }
    sh_offsets_kernel<<<blocks(std::max<uint64_t>(uint64_t(P.rows), F) + 1), kShThreads, 0, st>>>(A);
    HIP_OK(hipGetLastError());
  }
  if (host_out) {   // key_start | status
    HIP_OK(hipMemcpyAsync(host_out, key_start, (size_t(P.n_pre) + 2) * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (host_out[P.n_pre + 1] & int64_t(kShBadRowSplits)) arg_bad(op, "The input ragged tensor is invalid.");
  }
}

}  // namespace mhte
#endif  // MHTE_SHARDING_HOST_H_
