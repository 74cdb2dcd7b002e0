// The parts of the checkpoint path that need no GPU (mhte_ckpt_host.h puts them together with the
// device scans and upserts): the error type of the C ABI, the shard-thread pool, the pool of staging
// sets, the shard arithmetic of partial_dump, the shard set of a checkpoint on disk, the read-ahead
// record stream of a restore, the cut of a batch into runs of distinct ids and the initial row of a
// table.  Compiled by hipcc inside mhte.hip and, for the CPU suite (tests/ckpt_host_driver.cc), by
// g++ with MHTE_HOST_ONLY defined — plain and under the address, undefined-behaviour and thread
// sanitizers: the stream and the pool are the library's only hand-written multi-threaded host code.
#ifndef MHTE_CKPT_PARTS_H_
#define MHTE_CKPT_PARTS_H_

#include <ctype.h>
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <exception>
#include <future>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/monolith_amd_hash_table.h"
#include "mhte_ckpt.h"
#include "mhte_core.h"

namespace mhte {

// ------------------------------------------------------------------------------------------ errors
struct Error : std::runtime_error {
  mhte_status code;
  Error(mhte_status c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// ------------------------------------------------------------------------------------------ threads
// fn(lo, hi, k) over [0, n) cut into `parts` contiguous ranges, on that many host threads (the
// caller's included); the first exception is rethrown
template <typename F>
static void parallel_ranges(size_t n, int parts, F&& fn) {
  parts = int(std::max<size_t>(1, std::min<size_t>(size_t(parts), n)));
  std::vector<std::exception_ptr> err;
  err.resize(size_t(parts));
  auto run = [&](int k) {
    try {
      fn(n * size_t(k) / size_t(parts), n * size_t(k + 1) / size_t(parts), k);
    } catch (...) {
      err[size_t(k)] = std::current_exception();
    }
  };
  std::vector<std::thread> th;
  for (int k = 1; k < parts; ++k) th.emplace_back(run, k);
  run(0);
  for (auto& x : th) x.join();
  for (auto& e : err)
    if (e) std::rethrow_exception(e);
}

// host threads per checkpoint shard for the EntryDump codec (MHTE_CKPT_THREADS; shards run beside
// each other on up to 16 threads of their own)
static inline int ckpt_codec_threads() {
  static const int n = [] {
    if (const char* e = getenv("MHTE_CKPT_THREADS")) return std::max(1, atoi(e));
    const unsigned hw = std::thread::hardware_concurrency();
    return int(std::max(1u, std::min(16u, hw / 8u)));
  }();
  return n;
}

// MHTE_CKPT_TRACE: phase seconds of every shard to stderr, "[mhte ckpt] ..." 
static inline bool ckpt_trace() { return getenv("MHTE_CKPT_TRACE") != nullptr; }
static inline double ckpt_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Shard jobs 0..n-1 on at most 16 host threads (the caller's included).  Every job runs, whatever the
// others do; after all threads have joined, the error of the failed shard with the lowest index is
// rethrown.
constexpr int kMaxShardThreads = 16;
template <typename F>
static void run_shard_jobs(int n, F&& job) {
  if (n <= 0) return;
  std::vector<std::exception_ptr> err;
  err.resize(size_t(n));
  std::atomic<int> next{0};
  auto worker = [&] {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
      try {
        job(i);
      } catch (...) {
        err[size_t(i)] = std::current_exception();
      }
    }
  };
  std::vector<std::thread> th;
  const int extra = std::min(n, kMaxShardThreads) - 1;
  for (int i = 0; i < extra; ++i) th.emplace_back(worker);
  worker();
  for (auto& x : th) x.join();
  for (auto& e : err)
    if (e) std::rethrow_exception(e);
}

// Staging sets kept between calls, one per concurrent shard job: a Lease takes one (a fresh one when
// all are out) and hands it back when it goes out of scope, on every path.
template <class T>
class StagePool {
 public:
  class Lease {
   public:
    explicit Lease(StagePool& pool) : pool_(pool) {
      std::lock_guard<std::mutex> g(pool_.mu_);
      if (!pool_.idle_.empty()) {
        stage_ = std::move(pool_.idle_.back());
        pool_.idle_.pop_back();
      }
      if (!stage_) stage_.reset(new T);
    }
    ~Lease() {
      std::lock_guard<std::mutex> g(pool_.mu_);
      pool_.idle_.push_back(std::move(stage_));
    }
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    T& operator*() const { return *stage_; }

   private:
    StagePool& pool_;
    std::unique_ptr<T> stage_;
  };

 private:
  std::mutex mu_;
  std::vector<std::unique_ptr<T>> idle_;
};
struct CkptStage;   // mhte_ckpt_host.h: the device and pinned buffers of one shard job
using CkptPool = StagePool<CkptStage>;

// ------------------------------------------------------------------------------------------ shards
// buckets [begin, end) of shard `shard` of `total` in a table of 2^hashpower buckets: partial_dump's
// split (cuckoohash_map.hpp:745-751), the first 2^hashpower % total shards one bucket longer
struct BucketRange {
  uint64_t begin, end;
};
static inline BucketRange shard_bucket_range(uint32_t hashpower, int shard, int total) {
  const uint64_t nb = uint64_t(1) << hashpower;
  const uint64_t Q = nb / uint64_t(total), R = nb % uint64_t(total);
  const uint64_t begin = uint64_t(shard) * Q + std::min<uint64_t>(uint64_t(shard), R);
  return BucketRange{begin, begin + Q + (uint64_t(shard) < R ? 1 : 0)};
}

// PickNshards (multi_hash_table_save_restore_ops.cc:240-248, hash_table_save_op.cc:122-127): a
// negative request means one shard per million entries, at most 4
static inline int pick_nshards(int64_t total_entries, int requested) {
  if (requested < 0) requested = int(std::min<int64_t>(4, std::max<int64_t>(1, total_entries / 1000000)));
  return std::max(requested, 1);
}

// A shard file of a save: written under <name>-tmp-<pid>-<shard>, renamed into place once complete
struct ShardFile {
  std::string name, tmp;
  ShardFile(const std::string& basename, const char* infix, int shard, int total)
      : name(ckpt::shard_name(basename, infix, shard, total)),
        tmp(name + "-tmp-" + std::to_string(uint64_t(getpid())) + "-" + std::to_string(shard)) {}
};
// (a shard's files in order, the data file first: the error names that one)
static inline void publish(std::initializer_list<const ShardFile*> files) {
  for (const ShardFile* f : files)
    if (rename(f->tmp.c_str(), f->name.c_str()) != 0)
      throw Error(MHTE_INTERNAL, "checkpoint: cannot rename into " + (*files.begin())->name);
}

// The shard set of a checkpoint: what the directory holds under <basename>-%05d-of-%05d (the
// reference globs <basename>-* and validates the set, ValidateShardedFiles,
// multi_hash_table_save_restore_ops.cc:323-349): one consistent total, every data shard and every
// .meta sidecar present.  Leftovers of an earlier save with another shard count are an error, not
// something to restore silently.
static inline int discover_shards(const std::string& basename, bool want_meta = true) {
  const size_t slash = basename.find_last_of('/');
  const std::string dir = slash == std::string::npos ? "." : basename.substr(0, slash == 0 ? 1 : slash);
  const std::string stem = slash == std::string::npos ? basename : basename.substr(slash + 1);
  std::vector<std::pair<int, int>> data, meta;  // (index, total)
  DIR* dp = opendir(dir.c_str());
  if (!dp) throw Error(MHTE_NOT_FOUND, "no checkpoint shards found for " + basename);
  while (dirent* de = readdir(dp)) {
    const std::string fn = de->d_name;
    for (int is_meta = 0; is_meta < 2; ++is_meta) {
      const std::string pre = stem + (is_meta ? ".meta-" : "-");
      if (fn.size() != pre.size() + 14 || fn.compare(0, pre.size(), pre) != 0) continue;
      const std::string tail = fn.substr(pre.size());  // ddddd-of-ddddd
      if (tail.compare(5, 4, "-of-") != 0) continue;
      bool digits = true;
      for (int k = 0; k < 14; ++k)
        if (k < 5 || k >= 9) digits = digits && isdigit(static_cast<unsigned char>(tail[k]));
      if (!digits) continue;
      (is_meta ? meta : data).emplace_back(atoi(tail.substr(0, 5).c_str()), atoi(tail.substr(9).c_str()));
    }
  }
  closedir(dp);
  if (data.empty()) throw Error(MHTE_NOT_FOUND, "no checkpoint shards found for " + basename);
  const int total = data[0].second;
  auto complete = [&](std::vector<std::pair<int, int>>& v, const char* what) {
    std::sort(v.begin(), v.end());
    bool ok = int(v.size()) == total;
    for (int i = 0; ok && i < total; ++i) ok = v[size_t(i)].first == i && v[size_t(i)].second == total;
    if (!ok)
      throw Error(MHTE_INVALID_ARGUMENT,
                  std::string("checkpoint ") + basename + ": the " + what + " files are not one "
                  "complete set of -%05d-of-%05d shards (stale files of another save?)");
  };
  complete(data, "data");
  if (want_meta) complete(meta, ".meta");
  return total;
}

// ------------------------------------------------------------------------------------------ restore
// The records of a shard's data file, in order, through two stretches of about `stretch` bytes:
// while the records of one are verified, decoded and upserted by the caller, a helper thread reads
// and unpacks the next one (the reader is only ever used by one thread at a time).  The snappy
// blocks of a stretch are unpacked side by side on `unpack_threads` threads of the helper's own.
class RecordStream {
 public:
  using RecRef = ckpt::RecordReader::RecRef;
  // arenas[2]: where the stretches live (a shard job's staging set keeps them between restores)
  RecordStream(ckpt::RecordReader& data, ckpt::ByteArena* arenas, size_t stretch, int unpack_threads)
      : data_(data), arenas_(arenas), stretch_(stretch) {
    unpack_ = [unpack_threads](size_t n, const std::function<void(size_t, size_t)>& fn) {
      parallel_ranges(n, unpack_threads, [&](size_t lo, size_t hi, int) { fn(lo, hi); });
    };
    read_into(0);
  }
  ~RecordStream() {   // never leave the helper running into freed buffers
    if (!ahead_.valid()) return;
    try {
      (void)ahead_.get();
    } catch (...) {
    }
  }
  RecordStream(const RecordStream&) = delete;
  RecordStream& operator=(const RecordStream&) = delete;

  // Up to `want` records of the stream: refs()[*first .. *first + count), their bytes at base() +
  // off — both valid until the next take().  0 at the end of the file, then 0 again.  The reader's
  // errors (a cut or corrupted file) surface here.
  size_t take(uint64_t want, size_t* first) {
    if (cur_ == avail_) {
      if (at_end_) return 0;
      at_end_ = true;                       // (also when the reader's error is rethrown)
      if (!ahead_.get()) return 0;
      at_end_ = false;
      use_ = started_ ? (use_ ^ 1) : 0;
      started_ = true;
      cur_ = 0;
      avail_ = refs_[use_].size();          // (this thread's view: the helper fills the OTHER stretch)
      read_into(use_ ^ 1);
    }
    const size_t k = size_t(std::min<uint64_t>(want, avail_ - cur_));
    *first = cur_;
    cur_ += k;
    return k;
  }
  const char* base() const { return arenas_[use_].data(); }
  const std::vector<RecRef>& refs() const { return refs_[use_]; }

 private:
  void read_into(int b) {
    ahead_ = std::async(std::launch::async,
                        [this, b] { return data_.read_batch(arenas_[b], stretch_, refs_[b], unpack_); });
  }
  ckpt::RecordReader& data_;
  ckpt::ByteArena* arenas_;
  const size_t stretch_;
  ckpt::ParallelFor unpack_;
  std::vector<RecRef> refs_[2];
  std::future<bool> ahead_;   // the read into the other stretch
  int use_ = 0;               // stretch in use
  size_t cur_ = 0, avail_ = 0;
  bool started_ = false, at_end_ = false;
};

// ids inside one upsert launch must be distinct.  A checkpoint holds each id once per table, but a
// foreign writer (or concatenated files) may repeat one: the reference upserts entry after entry,
// so the LATER record wins (cuckoo_embedding_hash_table.cc:303-318).  A batch is therefore applied
// as maximal runs of distinct ids, in file order: the end of the run that starts at `start`.
// `seen`: scratch, an open-addressing set of the run's ids (index + 1, 0 = free).
static inline size_t next_distinct_run(const int64_t* ids, size_t start, size_t n, std::vector<uint32_t>& seen) {
  size_t cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  seen.assign(cap, 0u);
  size_t end = start;
  for (; end < n; ++end) {
    size_t h = size_t(hash_key(ids[end])) & (cap - 1);
    while (seen[h] && ids[seen[h] - 1] != ids[end]) h = (h + 1) & (cap - 1);
    if (seen[h]) break;   // (a repeat)
    seen[h] = uint32_t(end + 1);
  }
  return end;
}

// What a restored row starts from: initializer + optimizer Init (UpsertEntry's init_fn); the dump
// then overwrites what it carries.  A dump always carries `num`, so the initial weight only stands
// in until it is overwritten (random-uniform: 0).
static inline std::vector<float> initial_row(const SegDesc* segs, uint32_t nseg, uint32_t row_floats) {
  std::vector<float> init(row_floats, 0.f);
  for (uint32_t k = 0; k < nseg; ++k) {
    const SegDesc& d = segs[k];
    const float w0 = d.init == kInitRandomUniform ? 0.f : init_weight(d, nullptr);
    const int nv = opt_vectors(d.opt);
    for (int e = 0; e < d.dim; ++e) {
      init[size_t(d.w_off + e)] = w0;
      for (int v = 0; v < nv; ++v) init[size_t(d.st_off + v * d.dim + e)] = opt_state_init(d, v);
    }
    if (opt_scalars(d.opt)) {  // adam_optimizer.cc:52-53
      init[size_t(d.st_off + nv * d.dim)] = d.p[0];
      init[size_t(d.st_off + nv * d.dim + 1)] = d.p[1];
    }
    if (d.opt == kOptGroupAdagrad) init[size_t(d.st_off)] = d.p[0];  // group_adagrad_optimizer.cc:45-48
  }
  return init;
}

}  // namespace mhte
#endif  // MHTE_CKPT_PARTS_H_
