// Host-side plumbing of the ops that sit between the sparse step's forward and backward: the per-device
// scratch (AuxWs), the pinned staging ring for small uploads (PinnedStage), the argument checks they share, and
// the upload and dispatch of a chunk table (mhte_chunk_table.h).  Included by mhte.hip behind DedupWs and the
// group kernels, in front of the hosts that need it (mhte_clip_host.h, mhte_flat_host.h, mhte_dense_opt_host.h,
// mhte_ffm_host.h, mhte_auc_host.h, mhte_bsm_host.h, mhte_fi_host.h).
#ifndef MHTE_AUX_HOST_H_
#define MHTE_AUX_HOST_H_

#include "mhte_chunk_table.h"

namespace mhte {

// scratch of the deterministic (list-based) forms of the pooling ops: one per device, serialised
struct AuxWs {
  std::mutex mu;
  DedupWs dd;
  DevBuf<int64_t> keys, uids;
  DevBuf<uint32_t> inverse, seg_off, seg_pos, nu;
  DevBuf<float> clip_partials;   // clip by global norm (mhte_clip_host.h): the 1024 partial sums of squares
  DevBuf<char> clip_table;       // ... and the tensor table of a call with more than 128 tensors
  DevBuf<char> flat_table;       // aligned flat concat (mhte_flat_host.h): the same for its calls
  DevBuf<char> dense_opt_table;  // dense optimizers (mhte_dense_opt_host.h): the same, beyond 96 variables
  DevBuf<int64_t> split_row_splits;   // split by indices (mhte_split_host.h): the caller's row_splits
  DevBuf<char> split_table;           // ... and the pointer table of its gradient
  DevBuf<char> auc;                   // in-batch AUC loss (mhte_auc_host.h): the plan's arrays, by its offsets
  DevBuf<char> bsm;                   // batch softmax loss (mhte_bsm_host.h): the same
  DevBuf<char> fi;                    // FeatureInsight (mhte_fi_host.h): the slab partials of the weight gradient
  static AuxWs& of(int device) {
    static std::mutex m;
    static std::map<int, std::unique_ptr<AuxWs>> all;
    std::lock_guard<std::mutex> g(m);
    auto& p = all[device];
    if (!p) {
      p.reset(new AuxWs);
      p->dd.device = device;
    }
    return *p;
  }
  // the scratch is reused by the next call in stream order; a call on ANOTHER stream is ordered behind
  // the launches of the previous one by an event the stream waits for — the host never does (these
  // ops sit between the forward and the backward of every training step: a host wait here drains the
  // caller's queue once per step)
  hipStream_t last = nullptr;
  bool used = false;
  hipEvent_t done = nullptr;
  void enter(hipStream_t st) {
    if (!done) HIP_OK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    if (used && last != st) HIP_OK(hipStreamWaitEvent(st, done, 0));
    last = st;
    used = true;
  }
  void leave(hipStream_t st) { HIP_OK(hipEventRecord(done, st)); }   // after the call's last launch
  // A stream that is being captured into a graph takes neither the wait nor the record: the graph's own
  // edges order its launches, and an event the capture has touched must not be waited for by a later call
  // outside it.  Whoever replays such a graph beside calls on another stream orders the two themselves.
  struct Use {   // enter now, leave when the caller's launches are enqueued
    AuxWs& ws;
    hipStream_t st;
    bool capturing = false;
    Use(AuxWs& w, hipStream_t s) : ws(w), st(s) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
      capturing = cs == hipStreamCaptureStatusActive;
      if (!capturing) ws.enter(st);
    }
    ~Use() {
      if (!capturing) (void)hipEventRecord(ws.done, st);
    }
  };
  // The same lists for keys known to lie in [0, 2^key_bits), key_bits <= 31: a STABLE radix sort of
  // (key, position) pairs — equal keys keep their positions ascending — and the heads of the sorted runs
  // compacted into uids / seg_off (csrc/mhte_group_kernels.h: this repo's own kernels since round 6; round 5
  // went through rocPRIM's Onesweep sort + run-length encode + scan, ≈ 20 launches per grouping).  The
  // list-building dedup below is a hash table with two device atomics per key and five launches over all n
  // keys; the sort moves 8 bytes per key and pass and needs no atomic.  Keys come out ascending instead of
  // in first-occurrence order; the consumers write one output row per key and do not care.  Keys outside
  // the range are dropped, which is what the consumers did with them.  MHTE_GROUP_DD=1 selects the dedup
  // form (A/B; read per call, so that a test can run both forms in one process).
  DevBuf<uint32_t> k32b, gs_hist, gs_tot, gs_heads;
  DevBuf<uint2> gs_kva, gs_kvb;
  static bool use_sort() {
    const char* e = getenv("MHTE_GROUP_DD");
    return !(e && atoi(e) != 0);
  }
  // the tiles of a pass over n keys (0 < n < 2^31) and its histogram scratch: at most kGsMaxTiles tiles, of one
  // round of kGsRound keys per wavefront while that is enough
  void gs_tiles(GsPass& P, int64_t n) {
    P.n = uint32_t(n);
    const uint64_t per_round = uint64_t(kGsWaves) * kGsRound;
    P.rounds = uint32_t(std::max<uint64_t>(1, (uint64_t(n) + per_round * kGsMaxTiles - 1) / (per_round * kGsMaxTiles)));
    const uint64_t tile_keys = per_round * P.rounds;
    P.ntiles = uint32_t((uint64_t(n) + tile_keys - 1) / tile_keys);
    P.tstride = (P.ntiles + 3u) & ~3u;
    gs_hist.reserve(size_t(kGsMaxBins) * kGsMaxTiles);
    gs_tot.reserve(kGsMaxBins);
    P.hist = gs_hist.p;
    P.tot = gs_tot.p;
  }
  void group_sorted(const int64_t* k, int64_t n, int key_bits, hipStream_t st) {
    if (key_bits < 1) key_bits = 1;
    if (!use_sort() || key_bits > 31 || n >= int64_t(0x7fffffff) || n < 1) {
      group(k, n, st);
      return;
    }
    uids.reserve(size_t(n) + 1);
    seg_off.reserve(size_t(n) + 2);
    seg_pos.reserve(size_t(n) + 1);
    nu.reserve(4);
    k32b.reserve(size_t(n));
    const int bits = key_bits + 1;   // (`limit` = 2^key_bits itself is a key: the dropped ones, sorted last)
    const int passes = (bits + kGsMaxBits - 1) / kGsMaxBits;
    const int dig = (bits + passes - 1) / passes;
    GsPass P{};
    P.limit = 1u << key_bits;
    gs_tiles(P, n);
    if (passes > 1) gs_kva.reserve(size_t(n));
    if (passes > 2) gs_kvb.reserve(size_t(n));
    for (int j = 0; j < passes; ++j) {
      P.shift = uint32_t(j * dig);
      P.bits = uint32_t(std::min(dig, bits - j * dig));
      // (key, position) words ping-pong between two buffers; the last pass writes the consumers' arrays
      const bool last = j == passes - 1;
      P.k64 = j == 0 ? k : nullptr;
      P.kvin = j == 0 ? nullptr : ((j & 1) ? gs_kva.p : gs_kvb.p);
      P.kvout = last ? nullptr : ((j & 1) ? gs_kvb.p : gs_kva.p);
      P.kout = k32b.p;
      P.pout = seg_pos.p;
      gs_hist_kernel<false><<<dim3(P.ntiles), kGsThreads, 0, st>>>(P);
      gs_rowscan_kernel<<<dim3(1u << P.bits), 64, 0, st>>>(P);
      gs_scatter_kernel<false><<<dim3(P.ntiles), kGsThreads, 0, st>>>(P);
    }
    const uint32_t ntsel = uint32_t((uint64_t(n) + kGsSelTile - 1) / kGsSelTile);
    gs_heads.reserve(ntsel);
    gs_heads_count_kernel<<<dim3(ntsel), 1024, 0, st>>>(k32b.p, P.n, gs_heads.p);
    gs_heads_emit_kernel<<<dim3(ntsel), 1024, 0, st>>>(k32b.p, P.n, P.limit, gs_heads.p, uids.p, seg_off.p, nu.p);
    HIP_OK(hipGetLastError());
  }
  // distinct keys + their positions in ascending order -> uids / seg_off / seg_pos / nu
  void group(const int64_t* k, int64_t n, hipStream_t st) {
    uids.reserve(size_t(n) + 1);
    inverse.reserve(size_t(n) + 1);
    seg_off.reserve(size_t(n) + 2);
    seg_pos.reserve(size_t(n) + 1);
    nu.reserve(4);
    dd.unique(k, n, uids.p, inverse.p, seg_off.p, seg_pos.p, nu.p, st);
  }
};
// Small host arrays a call uploads (task tables, pointer tables): staged through a ring of pinned
// buffers, so the H2D copy is asynchronous and no call waits for its stream; a slot is reused after
// its copy has completed (the host waits only when kSlots calls are still in flight).
struct PinnedStage {
  static constexpr int kSlots = 8;
  std::mutex mu;
  char* buf[kSlots] = {};
  size_t cap[kSlots] = {};
  hipEvent_t ev[kSlots] = {};
  bool pending[kSlots] = {};
  int next = 0;
  static PinnedStage& of(int device) {
    static std::mutex m;
    static std::map<int, std::unique_ptr<PinnedStage>> all;
    std::lock_guard<std::mutex> g(m);
    auto& p = all[device];
    if (!p) p.reset(new PinnedStage);
    return *p;
  }
  void upload(void* dst_dev, const void* src, size_t n, hipStream_t st) {
    if (!n) return;
    std::lock_guard<std::mutex> g(mu);
    const int i = next;
    next = (next + 1) % kSlots;
    if (!ev[i]) HIP_OK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    if (pending[i]) HIP_OK(hipEventSynchronize(ev[i]));
    if (cap[i] < n) {
      if (buf[i]) HIP_OK(hipHostFree(buf[i]));
      buf[i] = nullptr;
      const size_t want = std::max<size_t>(n, size_t(1) << 16);
      HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&buf[i]), want, hipHostMallocDefault));
      cap[i] = want;
    }
    memcpy(buf[i], src, n);
    HIP_OK(hipMemcpyAsync(dst_dev, buf[i], n, hipMemcpyHostToDevice, st));
    HIP_OK(hipEventRecord(ev[i], st));
    pending[i] = true;
  }
};
static bool pool_atomics() {   // MHTE_POOL_ATOMICS=1: the float-atomic forms (A/B runs)
  static const bool on = getenv("MHTE_POOL_ATOMICS") != nullptr && atoi(getenv("MHTE_POOL_ATOMICS")) != 0;
  return on;
}
static int current_device() {
  int d = 0;
  HIP_OK(hipGetDevice(&d));
  return d;
}

// ---- the argument checks of the ops behind this header ------------------------------------------------
[[noreturn]] static void arg_bad(const char* op, const std::string& m) {
  throw Error(MHTE_INVALID_ARGUMENT, std::string(op) + ": " + m);
}
// a list's count and lengths; noun: what the list holds ("tensor", "variable")
static void check_lens(const char* op, const char* noun, const int64_t* lens, int32_t n) {
  if (n < 0) arg_bad(op, "n must be >= 0, got " + std::to_string(n));
  for (int32_t i = 0; i < n; ++i)
    if (lens[i] < 0)
      arg_bad(op, std::string(noun) + " " + std::to_string(i) + " has the negative length " + std::to_string(lens[i]));
}
static void need_device() {
  static std::atomic<bool> seen{false};   // (a device, once seen, is not asked for again: these calls sit in the step)
  if (seen.load(std::memory_order_relaxed)) return;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    throw Error(MHTE_UNAVAILABLE, "no HIP device: the MI355X engine has no CPU fallback");
  }
  seen.store(true, std::memory_order_relaxed);
}

// ---- a chunk table's way to the device -----------------------------------------------------------------
// A table that outgrew the kernel arguments goes to buf, one of the workspace's buffers (the caller holds the
// workspace's mutex and has entered the stream), through pinned staging — no wait for the stream.
template <class TABLE>
static void chunk_upload(DevBuf<char>& buf, TABLE& T, hipStream_t st) {
  const size_t total = T.packed_bytes();
  buf.reserve(total);
  std::vector<char> h(total);
  T.pack(h.data(), buf.p);
  PinnedStage::of(current_device()).upload(buf.p, h.data(), total, st);
}
// The launches of a table: f(std::true_type) — the kernels' EXT instances — behind the upload into the
// workspace's buffer `buf`, under the workspace's mutex and in its stream order; f(std::false_type) for a
// table that rides in the arguments, which touches no workspace.  Every op keeps a buffer of its own: a captured
// graph takes no part in the workspace's event ordering, and two ops must not meet in one table through it.
template <class TABLE, class F>
static void chunk_launch(DevBuf<char> AuxWs::*buf, TABLE& T, hipStream_t st, F&& f) {
  if (!T.ext()) {
    f(std::false_type{});
    return;
  }
  AuxWs& ws = AuxWs::of(current_device());
  std::lock_guard<std::mutex> g(ws.mu);
  AuxWs::Use use_(ws, st);
  chunk_upload(ws.*buf, T, st);
  f(std::true_type{});
}

}  // namespace mhte
#endif  // MHTE_AUX_HOST_H_
