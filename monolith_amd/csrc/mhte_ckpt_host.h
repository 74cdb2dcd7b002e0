// Host side of the checkpoints in the reference's on-disk format (the codec: mhte_ckpt.h; the parts
// that need no GPU: mhte_ckpt_parts.h): the staging of a shard job, the shard runner, the walk over
// a table's slots that save, save_as_tensor and mhte_table_dump share, save and restore of a
// MultiHashTable and of one table (the legacy layout), save_as_tensor and feature_stat.  Included
// by mhte.hip behind mhte_sharding_host.h; the extern "C" entry points there only check their handle
// and call in.
#ifndef MHTE_CKPT_HOST_H_
#define MHTE_CKPT_HOST_H_

#include "mhte_ckpt_parts.h"

namespace mhte {

// staging of one checkpoint shard job (device scan output, pinned host copies, codec buffers): kept
// by the table between saves / restores (mhte_multi_table::ckpt_stages) — pinning and unpinning a
// gigabyte per call costs more than the copy it speeds up
struct CkptStage {
  DevBuf<uint32_t> bc;                      // the walk: entries per block of slots, and their prefix sum
  DevBuf<uint64_t> bo;
  std::vector<uint32_t> hc;                 // (their host copies: alive until the stream has taken them)
  std::vector<uint64_t> ho;
  DevBuf<int64_t> d_ids, d_pos;
  DevBuf<uint32_t> d_ts;
  DevBuf<float> d_rows;
  // two sets of everything a save chunk passes from stage to stage (scan -> encode -> write run
  // beside each other, ckpt::run_pipeline3); restore decodes into them in turn
  HostBuf<int64_t> h_ids[2];
  HostBuf<uint32_t> h_ts[2];
  HostBuf<float> h_rows[2];
  uint64_t h_n[2] = {0, 0};                 // rows of the chunk in the set
  std::vector<std::string> parts[2];        // framed records of the chunk, one string per codec thread
  std::vector<uint64_t> part_n[2];
  ckpt::ByteArena arena[2];   // restore: the stretch being decoded and the one being read ahead
};

static std::vector<ckpt::SegLayout> seg_layout(const Table& tb) {
  std::vector<ckpt::SegLayout> v;
  for (uint32_t i = 0; i < tb.nseg; ++i) {
    const SegDesc& d = tb.view.seg[i];
    ckpt::SegLayout s;
    s.dim = d.dim;
    s.kind = d.opt;  // (SegKind values are the engine's OptType)
    s.w_off = d.w_off;
    s.st_off = d.st_off;
    v.push_back(s);
  }
  return v;
}

static int64_t ttl_days_of(const Table& tb, int64_t id) {
  const int64_t slot = (id >> 48) & 0x7fff;  // slot_id_v2, reader_util.h:36-38
  int64_t days = tb.default_expire_days;
  for (size_t i = 0; i < tb.expire_slots.size(); ++i)
    if (tb.expire_slots[i] == slot) days = tb.expire_days[i];
  return days;
}

// shard(sh, stream) for shards 0..n-1 on the shard threads (run_shard_jobs: every shard runs, the
// first failed one is rethrown), each with a stream of its own on the table's device
template <typename F>
static void run_shards(int device, int n, F&& shard) {
  run_shard_jobs(n, [&](int sh) {
    HIP_OK(hipSetDevice(device));
    struct Stream {
      hipStream_t s = nullptr;
      ~Stream() {
        if (s) (void)hipStreamDestroy(s);
      }
    } own;
    HIP_OK(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    shard(sh, own.s);
  });
}

// entries the table holds, the one in the side slot included (sizes a save: pick_nshards)
static int64_t count_entries(Table& tb, hipStream_t st) {
  std::lock_guard<std::mutex> g(tb.mu);
  tb.sync_counters(st);
  return tb.live_keys() + (tb.h_ctr->special_state == 1 ? 1 : 0);
}

// ---- the walk over a table's slots --------------------------------------------------------------
// chunk = what one pipeline stage of a save holds at a time: small enough that a shard has several
// of them in flight (scan | encode | write beside each other) and that the two pinned staging sets
// stay in the hundreds of megabytes, large enough that the per-chunk synchronisations do not show
constexpr uint64_t kWalkSlots = uint64_t(1) << 18;

// The walk over slots [s0, s1) of a table whose lock the caller holds, in partial_dump's order
// (cuckoohash_map.hpp:740-773), in two steps.  walk_count: entries per block of 1024 slots, prefix sum
// on the host -> their number; the blocks' offsets are left on the device for walk_emit, which packs
// ids, slot positions, timestamps and rows into device buffers (still in flight on `st` at return).
static uint64_t walk_count(const Table& tb, uint64_t s0, uint64_t s1, CkptStage& sg, hipStream_t st) {
  const uint32_t nblocks = uint32_t((s1 - s0 + 1023) / 1024);
  sg.bc.reserve(nblocks);
  sg.bo.reserve(nblocks);
  dump_count_kernel<<<nblocks, 256, 0, st>>>(tb.view, s0, s1, sg.bc.p);
  HIP_OK(hipGetLastError());
  sg.hc.resize(nblocks);
  HIP_OK(hipMemcpyAsync(sg.hc.data(), sg.bc.p, sizeof(uint32_t) * nblocks, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  sg.ho.resize(nblocks);
  uint64_t acc = 0;
  for (uint32_t i = 0; i < nblocks; ++i) {
    sg.ho[i] = acc;
    acc += sg.hc[i];
  }
  if (acc) HIP_OK(hipMemcpyAsync(sg.bo.p, sg.ho.data(), sizeof(uint64_t) * nblocks, hipMemcpyHostToDevice, st));
  return acc;
}
static void walk_emit(const Table& tb, uint64_t s0, uint64_t s1, const CkptStage& sg, int64_t* ids, int64_t* pos,
                      uint32_t* ts, float* rows, hipStream_t st) {
  const uint32_t nblocks = uint32_t((s1 - s0 + 1023) / 1024);
  dump_emit_kernel<<<nblocks, 256, 0, st>>>(tb.view, s0, s1, sg.bo.p, ids, pos, ts, rows);
  HIP_OK(hipGetLastError());
}
// both, into the stage's own device buffers (at most kWalkSlots slots at a time); returns the number
// of entries found
static uint64_t walk_slots(const Table& tb, uint64_t s0, uint64_t s1, CkptStage& sg, hipStream_t st) {
  const uint64_t acc = walk_count(tb, s0, s1, sg, st);
  if (acc == 0) return 0;
  sg.d_ids.reserve(acc);
  sg.d_pos.reserve(acc);
  sg.d_ts.reserve(acc);
  sg.d_rows.reserve(acc * tb.row_floats);
  walk_emit(tb, s0, s1, sg, sg.d_ids.p, sg.d_pos.p, sg.d_ts.p, sg.d_rows.p, st);
  return acc;
}

// mhte_table_dump: the whole table in one walk, into the caller's device buffers of `cap` entries
static void dump_table(mhte_multi_table* t, Table& tb, int64_t cap, int64_t* ids, int64_t* positions,
                       uint32_t* ts, float* rows, int64_t* n_out, hipStream_t st) {
  HIP_OK(hipSetDevice(t->device));
  CkptPool::Lease sg(t->ckpt_stages);
  std::lock_guard<std::mutex> g(tb.mu);
  tb.finish_pending(st);
  const uint64_t nslots = (uint64_t(1) << tb.hp) * kSlots;
  const uint64_t acc = walk_count(tb, 0, nslots, *sg, st);
  *n_out = int64_t(acc);
  if (int64_t(acc) > cap) throw Error(MHTE_INVALID_ARGUMENT, "dump buffers too small: need " + std::to_string(acc));
  if (acc == 0) return;
  walk_emit(tb, 0, nslots, *sg, ids, positions, ts, rows, st);
  HIP_OK(hipStreamSynchronize(st));
}

// The one key that lives in the side slot (kEmptyKey itself; the reference's map holds INT64_MIN in
// a bucket like any other key): a walk hands it out behind the last bucket of shard 0.  The caller
// holds the table's lock.  false: the table does not hold it.
static bool fetch_reserved_row(const Table& tb, float* row, uint32_t* ts, hipStream_t st) {
  Counters c;
  HIP_OK(hipMemcpyAsync(&c, tb.ctr, sizeof(Counters), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (c.special_state != 1) return false;
  const uint32_t r = c.special_row;
  const float* src = tb.chunks[r >> tb.chunk_shift] + size_t(r & ((1u << tb.chunk_shift) - 1u)) * tb.row_floats;
  HIP_OK(hipMemcpyAsync(row, src, tb.row_floats * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  *ts = c.special_ts;
  return true;
}

// ---- save ---------------------------------------------------------------------------------------
// One shard of one table: buckets [begin, end) of partial_dump, in chunks; rows expired relative to
// the table's max_update_ts are dropped (multi_hash_table_save_restore_ops.cc:203-211).  Returns the
// number of entries written.
static uint64_t save_table_shard(Table& tb, int shard, int total, ckpt::RecordWriter& w, CkptStage& sg,
                                 hipStream_t st) {
  // the shard's bucket range is a function of the hashpower: a doubling between two chunks (a
  // concurrent update: the table is released between chunks) would leave the rest of the range
  // stale — rows missed or written twice.  The geometry is snapshotted under the lock and checked
  // by every chunk's scan; a change fails the save (the reference holds LockAll for the whole save,
  // hash_table_save_op.cc:106-108).
  uint32_t hp0;
  {
    std::lock_guard<std::mutex> g(tb.mu);
    hp0 = tb.hp;
  }
  const BucketRange range = shard_bucket_range(hp0, shard, total);
  const std::vector<ckpt::SegLayout> segs = seg_layout(tb);
  const uint32_t rf = tb.row_floats;
  uint64_t written = 0;
  auto expired = [&](int64_t id, uint32_t ts) {
    return tb.max_update_ts - int64_t(ts) >= ttl_days_of(tb, id) * int64_t(86400);
  };
  const int P = ckpt_codec_threads();
  for (int b = 0; b < 2; ++b) {
    if (sg.parts[b].size() < size_t(P)) sg.parts[b].resize(size_t(P));
    sg.part_n[b].assign(size_t(P), 0);
    sg.h_n[b] = 0;
  }
  double t_scan = 0, t_enc = 0, t_write = 0;                 // (each written by its stage's thread only)
  const uint64_t slot_begin = range.begin * kSlots, slot_end = range.end * kSlots;
  const size_t n_chunks = size_t((slot_end - slot_begin + kWalkSlots - 1) / kWalkSlots);
  // stage A (this thread: it owns the HIP stream): device scan of the chunk's slots + copy of the
  // rows it found into pinned set b.  The table is held for that only; the (longer) encoding and
  // writing of the chunk run beside the next chunk's scan and the other shards' threads.
  auto scan = [&](size_t c, int b) {
    const double t0 = ckpt_now();
    const uint64_t s0 = slot_begin + uint64_t(c) * kWalkSlots;
    const uint64_t s1 = std::min(slot_end, s0 + kWalkSlots);
    sg.h_n[b] = 0;
    std::lock_guard<std::mutex> g(tb.mu);
    if (tb.hp != hp0)
      throw Error(MHTE_FAILED_PRECONDITION, "table " + tb.name + " was resized by a concurrent update while "
                                            "it was being saved; save again");
    const uint64_t acc = walk_slots(tb, s0, s1, sg, st);
    if (acc != 0) {
      sg.h_ids[b].reserve(acc);
      sg.h_ts[b].reserve(acc);
      sg.h_rows[b].reserve(acc * rf);
      HIP_OK(hipMemcpyAsync(sg.h_ids[b].p, sg.d_ids.p, acc * 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(sg.h_ts[b].p, sg.d_ts.p, acc * 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(sg.h_rows[b].p, sg.d_rows.p, acc * rf * 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      sg.h_n[b] = acc;
    }
    t_scan += ckpt_now() - t0;
  };
  // stage B: EntryDump + TFRecord framing of the chunk's rows on P threads (contiguous ranges, so
  // the file keeps the dump order) into set b's strings
  auto encode = [&](size_t, int b) {
    const double t0 = ckpt_now();
    const uint64_t acc = sg.h_n[b];
    const int64_t* ids = sg.h_ids[b].p;
    const uint32_t* tsv = sg.h_ts[b].p;
    const float* rows = sg.h_rows[b].p;
    std::vector<std::string>& parts = sg.parts[b];
    std::vector<uint64_t>& part_n = sg.part_n[b];
    for (int k = 0; k < P; ++k) {
      parts[size_t(k)].clear();
      part_n[size_t(k)] = 0;
    }
    if (acc)
      parallel_ranges(size_t(acc), P, [&](size_t lo, size_t hi, int k) {
        std::string& out = parts[size_t(k)];
        std::string r;
        uint64_t n = 0;
        for (size_t i = lo; i < hi; ++i) {
          if (expired(ids[i], tsv[i])) continue;
          ckpt::encode_entry(r, ids[i], rows + i * rf, segs, int(tb.dim), tsv[i]);
          ckpt::RecordWriter::frame(out, r);
          ++n;
        }
        part_n[size_t(k)] = n;
      });
    t_enc += ckpt_now() - t0;
  };
  // stage C: the framed bytes through the writer, in range order
  auto write_out = [&](size_t, int b) {
    const double t0 = ckpt_now();
    for (int k = 0; k < P; ++k) {
      if (sg.parts[b][size_t(k)].empty()) continue;
      w.write_framed(sg.parts[b][size_t(k)]);
      written += sg.part_n[b][size_t(k)];
    }
    t_write += ckpt_now() - t0;
  };
  const double t_pipe0 = ckpt_now();
  ckpt::run_pipeline3(n_chunks, scan, encode, write_out);
  if (ckpt_trace())
    fprintf(stderr, "[mhte ckpt] save %s shard %d/%d: %llu rows in %zu chunks, %.3f s (stage seconds, "
                    "overlapped: scan+copy %.3f, encode(%d thr) %.3f, write %.3f)\n", tb.name.c_str(), shard,
            total, (unsigned long long)written, n_chunks, ckpt_now() - t_pipe0, t_scan, P, t_enc, t_write);
  if (shard == 0) {   // the key in the side slot: last entry of shard 0
    std::vector<float> row(rf);
    uint32_t ts = 0;
    std::lock_guard<std::mutex> g(tb.mu);
    if (fetch_reserved_row(tb, row.data(), &ts, st) && !expired(kEmptyKey, ts)) {
      std::string rec;
      ckpt::encode_entry(rec, kEmptyKey, row.data(), segs, int(tb.dim), ts);
      w.write(rec);
      ++written;
    }
  }
  return written;
}

// A MultiHashTable's save (multi_hash_table_save_restore_ops.cc:107-262): per shard a SNAPPY record
// file of EntryDump, the tables one after another, and a .meta sidecar of their entry counts.
// legacy_table >= 0: MonolithHashTableSave for that ONE table (hash_table_save_op.cc:98-173) — an
// uncompressed record file per shard, no sidecar.  Either way a shard is a contiguous bucket range,
// written under a temporary name and renamed; one thread per shard (the reference schedules its
// shards on the op's thread pool, :250-262).
static void save_tables(mhte_multi_table* t, const std::string& basename, int nshards, hipStream_t st,
                        int legacy_table = -1) {
  const bool legacy = legacy_table >= 0;
  const size_t first = legacy ? size_t(legacy_table) : 0, last = legacy ? first + 1 : t->tables.size();
  int64_t total = 0;
  for (size_t i = first; i < last; ++i) total += count_entries(*t->tables[i], st);
  nshards = pick_nshards(total, nshards);
  HIP_OK(hipStreamSynchronize(st));
  const bool trace = ckpt_trace() && !legacy;
  const double t_begin = ckpt_now();
  run_shards(t->device, nshards, [&](int sh, hipStream_t s2) {
    const double tj0 = ckpt_now();
    const ShardFile data(basename, "", sh, nshards), meta(basename, ".meta", sh, nshards);
    {
      ckpt::RecordWriter w(data.tmp, !legacy);
      std::unique_ptr<ckpt::RecordWriter> mw;
      if (!legacy) mw.reset(new ckpt::RecordWriter(meta.tmp, false));
      const double tj1 = ckpt_now();
      {
        CkptPool::Lease sg(t->ckpt_stages);
        std::string mrec;
        for (size_t i = first; i < last; ++i) {
          Table& tb = *t->tables[i];
          const uint64_t n = save_table_shard(tb, sh, nshards, w, *sg, s2);
          if (legacy) continue;
          ckpt::encode_meta(mrec, tb.name, n);
          mw->write(mrec);
        }
      }
      const double tj2 = ckpt_now();
      w.close();
      if (mw) mw->close();
      if (trace)
        fprintf(stderr, "[mhte ckpt] save shard %d: started +%.3f s, setup %.3f s, tables %.3f s, close %.3f s\n",
                sh, tj0 - t_begin, tj1 - tj0, tj2 - tj1, ckpt_now() - tj2);
    }
    if (legacy) publish({&data});
    else publish({&data, &meta});
  });
  if (trace) fprintf(stderr, "[mhte ckpt] save: all shards done +%.3f s\n", ckpt_now() - t_begin);
}

// ---- restore ------------------------------------------------------------------------------------
// rows of one restore batch -> table (upsert of whole rows with their own timestamps)
static void restore_batch(Table& tb, CkptStage& sg, const int64_t* ids, const float* rows,
                          const uint32_t* ts, int64_t n, hipStream_t st) {
  if (n == 0) return;
  tb.finish_pending(st);
  ++tb.mut_epoch;
  tb.ensure_capacity(uint64_t(n), st);
  sg.d_ids.reserve(size_t(n));
  sg.d_ts.reserve(size_t(n));
  sg.d_rows.reserve(size_t(n) * tb.row_floats);
  HIP_OK(hipMemcpyAsync(sg.d_ids.p, ids, n * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(sg.d_ts.p, ts, n * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(sg.d_rows.p, rows, size_t(n) * tb.row_floats * 4, hipMemcpyHostToDevice, st));
  tb.pending.reserve(size_t(n) + 1);
  const dim3 grid(uint32_t((n * 16 + 255) / 256));
  restore_rows_kernel<16><<<grid, 256, 0, st>>>(tb.view, sg.d_ids.p, n, sg.d_rows.p, sg.d_ts.p, tb.pending.p);
  restore_slowpath_kernel<<<1, 64, 0, st>>>(tb.view, sg.d_ids.p, sg.d_rows.p, sg.d_ts.p, tb.pending.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(st));  // the staging buffers are rewritten by the next batch
}

constexpr size_t kRestoreStretch = size_t(64) << 20;   // bytes of the data file read ahead at a time
constexpr size_t kRestoreBatch = size_t(1) << 18;      // rows per upsert batch

// The next `num` records of a shard's stream -> one table, as two stages beside each other over
// batches of kRestoreBatch rows (ckpt::run_pipeline3, the stage's two pinned sets): decode() takes
// the next records and verifies + decodes them on the codec threads into set b, upsert() — on a
// helper thread — cuts the batch into runs of distinct ids and upserts them.
struct TableRestore {
  Table& tb;
  CkptStage& sg;
  RecordStream& in;
  const ckpt::RecordReader& data;   // (verifies the records' checksums)
  const uint64_t num;
  const bool to_eof;                // the legacy layout: the file may end before `num`
  const int device;
  const hipStream_t st;
  // (layout and initial values are fixed at creation: read without the table's lock)
  const std::vector<ckpt::SegLayout> segs = seg_layout(tb);
  const std::vector<float> init = initial_row(tb.view.seg, tb.nseg, tb.row_floats);
  const uint32_t rf = tb.row_floats;
  const int P = ckpt_codec_threads();
  uint64_t done = 0;
  size_t set_n[2] = {0, 0};
  int64_t set_max_ts[2] = {0, 0};
  std::vector<uint32_t> seen;               // next_distinct_run's scratch
  double t_read = 0, t_dec = 0, t_up = 0;   // (read / decode: this thread; upsert: the helper)

  // false: the table's records are all taken
  bool decode(int b) {
    if (done >= num) return false;
    const double t0 = ckpt_now();
    size_t first = 0;
    const size_t nb = in.take(std::min<uint64_t>(kRestoreBatch, num - done), &first);
    if (!nb) {
      if (to_eof) return false;
      throw Error(MHTE_INTERNAL, "checkpoint shard ends early");
    }
    const double t1 = ckpt_now();
    HostBuf<int64_t>& ids = sg.h_ids[b];
    HostBuf<uint32_t>& ts = sg.h_ts[b];
    HostBuf<float>& rows = sg.h_rows[b];
    ids.reserve(nb);
    ts.reserve(nb);
    rows.reserve(nb * rf);
    const char* base = in.base();
    const RecordStream::RecRef* refs = in.refs().data() + first;
    std::vector<int64_t> part_max(size_t(P), 0);
    parallel_ranges(nb, P, [&](size_t lo, size_t hi, int k) {
      int64_t mx = 0;
      for (size_t i = lo; i < hi; ++i) {
        const RecordStream::RecRef& r = refs[i];
        data.verify(base + r.off, r.len, r.crc);
        float* row = rows.p + i * rf;
        memcpy(row, init.data(), sizeof(float) * rf);
        int64_t id;
        uint32_t tsv;
        ckpt::decode_entry(reinterpret_cast<const uint8_t*>(base + r.off), r.len, segs, int(tb.dim), &id, row,
                           &tsv);
        ids.p[i] = id;
        ts.p[i] = tsv;
        mx = std::max<int64_t>(mx, int64_t(tsv));
      }
      part_max[size_t(k)] = mx;
    });
    set_n[b] = nb;
    set_max_ts[b] = *std::max_element(part_max.begin(), part_max.end());
    done += nb;
    t_read += t1 - t0;
    t_dec += ckpt_now() - t1;
    return true;
  }

  void upsert(int b) {
    const double t0 = ckpt_now();
    HIP_OK(hipSetDevice(device));   // (a thread of the pipeline's own)
    const size_t nb = set_n[b];
    const int64_t* ids = sg.h_ids[b].p;
    for (size_t start = 0; start < nb;) {   // one launch per run, in file order
      const size_t end = next_distinct_run(ids, start, nb, seen);
      std::lock_guard<std::mutex> g(tb.mu);
      tb.max_update_ts = std::max<int64_t>(tb.max_update_ts, set_max_ts[b]);
      restore_batch(tb, sg, ids + start, sg.h_rows[b].p + start * rf, sg.h_ts[b].p + start,
                    int64_t(end - start), st);
      start = end;
    }
    t_up += ckpt_now() - t0;
  }

  void run() {
    ckpt::run_pipeline3(
        size_t(-1), [this](size_t, int b) { return decode(b); }, [this](size_t, int b) { upsert(b); },
        [](size_t, int) {});
  }
};

// One shard file -> the tables its .meta sidecar names, in the file's order; a table of the
// checkpoint that this MultiHashTable does not have is skipped (:352-361).
// legacy_table >= 0: the single-table layout of MonolithHashTableSave (hash_table_save_op.cc:147-160) —
// an UNCOMPRESSED TFRecord stream of EntryDump, no .meta sidecar: every record of the file belongs to
// that table (hash_table_restore_op.cc:118-150)
static void restore_shard(mhte_multi_table* t, const std::string& basename, int sh, int total,
                          hipStream_t st, int legacy_table = -1) {
  const bool legacy = legacy_table >= 0;
  ckpt::RecordReader data(ckpt::shard_name(basename, "", sh, total), !legacy);
  std::unique_ptr<ckpt::RecordReader> meta;
  if (!legacy) meta.reset(new ckpt::RecordReader(ckpt::shard_name(basename, ".meta", sh, total), false));
  CkptPool::Lease sg(t->ckpt_stages);
  RecordStream in(data, (*sg).arena, kRestoreStretch, std::min(4, ckpt_codec_threads()));
  std::string mrec, name;
  for (bool more = true; more; more = !legacy) {
    uint64_t num = ~uint64_t(0);
    int idx = legacy_table;
    if (legacy) {
      name = t->tables[size_t(idx)]->name;
    } else {
      if (!meta->read(&mrec)) break;
      ckpt::decode_meta(reinterpret_cast<const uint8_t*>(mrec.data()), mrec.size(), &name, &num);
      for (size_t i = 0; i < t->tables.size(); ++i)
        if (t->tables[i]->name == name) idx = int(i);
    }
    size_t first = 0;
    if (idx < 0) {
      for (uint64_t left = num; left;) {
        const size_t k = in.take(left, &first);
        if (!k) throw Error(MHTE_INTERNAL, "checkpoint shard ends early");
        left -= k;
      }
      continue;
    }
    TableRestore r{*t->tables[size_t(idx)], *sg, in, data, num, legacy, t->device, st};
    r.run();
    if (ckpt_trace())
      fprintf(stderr, "[mhte ckpt] restore %s shard %d/%d: %llu rows, read %.3f s, verify+decode(%d thr) "
                      "%.3f s | dup check + upsert %.3f s (beside each other)\n", name.c_str(), sh, total,
              (unsigned long long)num, r.t_read, r.P, r.t_dec, r.t_up);
  }
  size_t first = 0;
  if (in.take(1, &first)) throw Error(MHTE_INTERNAL, "Couldn't read all of checkpoint shard");
}

// Restore of a MultiHashTable, or (legacy_table >= 0) MonolithHashTableRestore for ONE table
// (hash_table_restore_op.cc:67-100), which is CLEARED first.  The shard set is validated
// (ValidateShardedFiles), then every shard's records are upserted: one thread per shard file —
// decoding (the long part) runs in parallel, a table is held only while a decoded batch is upserted.
static void restore_tables(mhte_multi_table* t, const std::string& basename, hipStream_t st,
                           int legacy_table = -1) {
  const bool legacy = legacy_table >= 0;
  const int total = discover_shards(basename, !legacy);
  if (legacy) {
    Table& tb = *t->tables[size_t(legacy_table)];
    std::lock_guard<std::mutex> g(tb.mu);
    tb.clear(st);
  }
  HIP_OK(hipStreamSynchronize(st));
  run_shards(t->device, total, [&](int sh, hipStream_t s2) { restore_shard(t, basename, sh, total, s2, legacy_table); });
}

// What the four save / restore entry points share behind their handle checks: the basename check,
// the device, and the translation of what the codec and the file layer throw — MHTE_INTERNAL, a
// restore's with the reference's "DataLoss: " in front.
template <typename F>
static void ckpt_entry(mhte_multi_table* t, bool restore, const char* basename, F&& body) {
  if (!basename || !*basename)
    throw Error(MHTE_INVALID_ARGUMENT, std::string(restore ? "restore" : "save") + ": empty basename");
  HIP_OK(hipSetDevice(t->device));
  try {
    body();
  } catch (const Error&) {
    throw;
  } catch (const std::exception& e) {
    throw Error(MHTE_INTERNAL, std::string(restore ? "DataLoss: " : "") + e.what());
  }
}

// ---- save_as_tensor -----------------------------------------------------------------------------
// MonolithHashTableSaveAsTensor's walk (cuckoohash_map.hpp:745-773): the shard's bucket range, the
// resume point inside it, at most `limit` entries (the count is checked AFTER an entry is taken:
// limit <= 0 still yields one) as serialized EntryDump strings.
static void save_as_tensor(mhte_multi_table* t, Table& tb, int32_t shard_idx, int32_t num_shards, int64_t limit,
                           int64_t offset, int64_t* new_offset, char* entries, int64_t cap,
                           int64_t* entry_offsets, int64_t offsets_cap, int64_t* n_entries, int64_t* needed,
                           hipStream_t st) {
  if (!new_offset || !n_entries || !needed) throw Error(MHTE_INVALID_ARGUMENT, "save_as_tensor: null argument");
  if (num_shards < 1 || shard_idx < 0 || shard_idx >= num_shards || offset < 0)
    throw Error(MHTE_INVALID_ARGUMENT, "save_as_tensor: shard " + std::to_string(shard_idx) + " of " +
                                           std::to_string(num_shards) + ", offset " + std::to_string(offset));
  HIP_OK(hipSetDevice(t->device));
  CkptPool::Lease sg(t->ckpt_stages);
  std::lock_guard<std::mutex> g(tb.mu);
  tb.finish_pending(st);
  const BucketRange range = shard_bucket_range(tb.hp, shard_idx, num_shards);
  const uint64_t want = uint64_t(std::max<int64_t>(limit, 1));
  const uint64_t s_begin = range.begin * kSlots, s_end = range.end * kSlots;
  const size_t rf = tb.row_floats;
  std::vector<int64_t> ids;
  std::vector<int64_t> pos;
  std::vector<uint32_t> ts;
  std::vector<float> rows;
  for (uint64_t s0 = s_begin + uint64_t(offset); s0 < s_end && ids.size() < want; s0 += kWalkSlots) {
    const uint64_t acc = walk_slots(tb, s0, std::min(s_end, s0 + kWalkSlots), *sg, st);
    if (!acc) continue;
    const size_t take = size_t(std::min<uint64_t>(acc, want - ids.size())), at = ids.size();
    ids.resize(at + take);
    pos.resize(at + take);
    ts.resize(at + take);
    rows.resize((at + take) * rf);
    HIP_OK(hipMemcpyAsync(ids.data() + at, (*sg).d_ids.p, take * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(pos.data() + at, (*sg).d_pos.p, take * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(ts.data() + at, (*sg).d_ts.p, take * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(rows.data() + at * rf, (*sg).d_rows.p, take * rf * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  // The key in the side slot is handed out behind the last bucket of shard 0, as the checkpoint save
  // writes it.  A walk that is already past the shard's end (offset = the "done" value below) does
  // not see it again.
  bool took_special = false;
  if (shard_idx == 0 && ids.size() < want && s_begin + uint64_t(offset) <= s_end) {
    std::vector<float> row(rf);
    uint32_t sts = 0;
    if (fetch_reserved_row(tb, row.data(), &sts, st)) {
      rows.insert(rows.end(), row.begin(), row.end());
      ids.push_back(kEmptyKey);
      pos.push_back(int64_t(s_end));
      ts.push_back(sts);
      took_special = true;
    }
  }
  // stopped on the limit: resume behind the last entry; ran off the shard's end: one bucket past it
  // (":770 Using +1 here since end might equal to begin")
  if (!took_special && ids.size() >= want) *new_offset = int64_t(uint64_t(pos.back()) - s_begin + 1);
  else *new_offset = int64_t((range.end - range.begin + 1) * kSlots);
  *n_entries = int64_t(ids.size());
  const std::vector<ckpt::SegLayout> segs = seg_layout(tb);
  std::string all, rec;
  std::vector<int64_t> offs(1, 0);
  for (size_t i = 0; i < ids.size(); ++i) {
    ckpt::encode_entry(rec, ids[i], rows.data() + i * rf, segs, int(tb.dim), ts[i]);
    all += rec;
    offs.push_back(int64_t(all.size()));
  }
  *needed = int64_t(all.size());
  if (int64_t(offs.size()) > offsets_cap || !entry_offsets)
    throw Error(MHTE_INVALID_ARGUMENT, "save_as_tensor: entry_offsets holds " + std::to_string(offsets_cap) +
                                           " values, need " + std::to_string(offs.size()));
  memcpy(entry_offsets, offs.data(), offs.size() * sizeof(int64_t));
  if (int64_t(all.size()) > cap || (!entries && !all.empty()))
    throw Error(MHTE_INVALID_ARGUMENT, "save_as_tensor: entries buffer too small: need " +
                                           std::to_string(all.size()));
  if (!all.empty()) memcpy(entries, all.data(), all.size());
}

// ---- feature_stat -------------------------------------------------------------------------------
// MonolithMultiHashTableFeatureStat (multi_hash_table_save_restore_ops.cc:424-497): the entry counts
// of a checkpoint's tables, summed over the .meta sidecars of its shards; names sorted
static void feature_stat(const char* basename, char* names, int64_t names_cap, uint64_t* counts, int32_t cap,
                         int32_t* n_out) {
  if (!basename || !*basename || !n_out) throw Error(MHTE_INVALID_ARGUMENT, "feature_stat: bad arguments");
  const int total = discover_shards(basename);
  std::map<std::string, uint64_t> stat;
  for (int sh = 0; sh < total; ++sh) {
    ckpt::RecordReader meta(ckpt::shard_name(basename, ".meta", sh, total), false);
    std::string rec, name;
    try {
      while (meta.read(&rec)) {
        uint64_t num = 0;
        ckpt::decode_meta(reinterpret_cast<const uint8_t*>(rec.data()), rec.size(), &name, &num);
        stat[name] += num;
      }
    } catch (const std::exception& e) {
      throw Error(MHTE_INTERNAL, std::string("DataLoss: Read table metadata failed! ") + e.what());
    }
  }
  *n_out = int32_t(stat.size());
  int64_t off = 0;
  int32_t k = 0;
  for (auto& kv : stat) {
    if (k >= cap || off + int64_t(kv.first.size()) + 1 > names_cap)
      throw Error(MHTE_INVALID_ARGUMENT, "feature_stat: output buffers too small");
    memcpy(names + off, kv.first.c_str(), kv.first.size() + 1);
    off += int64_t(kv.first.size()) + 1;
    counts[k++] = kv.second;
  }
}

}  // namespace mhte
#endif  // MHTE_CKPT_HOST_H_
