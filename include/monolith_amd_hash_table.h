/* monolith_amd_hash_table.h — C ABI of the MI355X-native MultiHashTable engine (libmhte.so).
 *
 * Drop-in boundary for Monolith's MultiHashTable TensorFlow custom ops.  Every entry point below
 * names the reference interface it replaces; paths are relative to
 * /root/reference/monolith/native_training/runtime/ ("RT/") or .../native_training/ ("NT/").
 * The reference-side binding (a TF OpKernel shim, and the ctypes binding used here) is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns an mhte_status; on failure mhte_last_error() (thread-local) holds a
 *     message.  Codes are TensorFlow's error codes, because the reference maps engine exceptions to
 *     errors::InvalidArgument / errors::ResourceExhausted
 *     (RT/ops/embedding_hash_table_tf_bridge.cc:132-134,365-367).
 *   - "dev" pointers are HIP device pointers on the table's GPU; "host" pointers are ordinary
 *     host memory.  Shape-determining inputs (row splits, slot sizes, learning rates, scalars) are
 *     host memory — the TF kernel registers them as HostMemory inputs.
 *   - `stream` is a hipStream_t passed as void*.  All work is enqueued on it and is ordered with
 *     respect to earlier calls on the same stream (the reference chains ops through the returned
 *     resource handle, RT/ops/multi_hash_table_update_op.cc:87; here stream order is that chain).
 *     A table must be driven from one stream at a time.
 *   - Tables of a MultiHashTable are ordered by sorted name, as NT/multi_hash_table_ops.py:83 does.
 */
#ifndef MONOLITH_AMD_HASH_TABLE_H_
#define MONOLITH_AMD_HASH_TABLE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t mhte_status;
enum {
  MHTE_OK = 0,
  MHTE_INVALID_ARGUMENT = 3,    /* tensorflow::error::INVALID_ARGUMENT */
  MHTE_NOT_FOUND = 5,
  MHTE_RESOURCE_EXHAUSTED = 8,  /* tensorflow::error::RESOURCE_EXHAUSTED */
  MHTE_FAILED_PRECONDITION = 9,
  MHTE_INTERNAL = 13,
  MHTE_UNAVAILABLE = 14         /* no HIP device / runtime error */
};

const char* mhte_last_error(void);
/* ABI version of this header; mhte_abi_version() must return the same value. */
#define MHTE_ABI_VERSION 19
int32_t mhte_abi_version(void);

/* ---- configuration (flat C form of RT/hash_table/embedding_hash_table.proto) --------------- */
enum {                                                                     /* optimizer.proto:210-229 */
  MHTE_OPT_SGD = 0, MHTE_OPT_ADAGRAD = 1, MHTE_OPT_FTRL = 2,
  /* every per-element optimizer below rides the fused training-step kernels too (the single-table,
     multi-table and sharded steps: their FULL instantiations); only GROUP_ADAGRAD — one step needs
     the whole segment — stays on the op-level kernels (mhte_optimize & co) */
  MHTE_OPT_MOMENTUM = 3, MHTE_OPT_ADADELTA = 4, MHTE_OPT_RMSPROP = 5, MHTE_OPT_RMSPROPV2 = 6,
  MHTE_OPT_ADAM = 7, MHTE_OPT_AMSGRAD = 8, MHTE_OPT_MOVING_AVERAGE = 9,
  MHTE_OPT_BATCH_SOFTMAX = 10, /* dim_size 1; uses the ops' global_step argument */
  MHTE_OPT_GROUP_ADAGRAD = 11, /* AdaGradWithGroupLasso: one step needs the whole segment */
  /* OR-ed into opt_type: OptimizerConfig.stochastic_rounding_float16 (optimizer.proto:228) — the
     StochasticRoundingFloat16OptimizerDecorator (optimizer/stochastic_rounding.h:27-59): after every
     Optimize() each weight of the segment becomes one of its two binary16 neighbours, the upper one
     with probability (w - down) / (up - down).  The rounding function is the reference's, value for
     value; its draws there come from a thread-local generator consumed in call order, here from a
     counter-based hash of (element address, unrounded value, update_time, occurrence).  Not with
     GROUP_ADAGRAD (INVALID_ARGUMENT). */
  MHTE_OPT_FLAG_STOCHASTIC_ROUNDING_FP16 = 0x100
};
enum { MHTE_INIT_ZEROS = 0, MHTE_INIT_ONES = 1, MHTE_INIT_CONSTANT = 2, /* initializer_config.proto */
       MHTE_INIT_RANDOM_UNIFORM = 3 /* uniform in [init_value, init_value2): a counter-based draw per
                                       element; the reference's thread-local mt19937
                                       (initializer/random_uniform_initializer.cc:31-37) is not
                                       reproducible, so parity is distributional */ };

/* EntryConfig.Segment (embedding_hash_table.proto:23-43) */
typedef struct {
  int32_t dim_size;
  int32_t opt_type;     /* MHTE_OPT_* */
  float opt_params[8];  /* ADAGRAD:  {initial_accumulator_value, weight_decay_factor, avx_form}
                                     avx_form != 0 (extension): the update of the reference as its
                                     .bazelrc:63-68 builds it, avx_utils.h:96-119 — fused
                                     multiply-adds and, inside blocks of 8 elements, the weight
                                     step taken with the raw gradient (:112); default 0: the
                                     baseline loop (:29-38).  They differ when
                                     weight_decay_factor != 0
                           FTRL:     {initial_accumulator_value, beta, l1, l2}
                           MOMENTUM: {momentum, weight_decay_factor, use_nesterov}
                           ADADELTA: {averaging_ratio, epsilon, weight_decay_factor}
                           RMSPROP / RMSPROPV2: {momentum, weight_decay_factor, learning_rate of the
                                     config (v1 ignores the op's learning-rate input,
                                     rmsprop_optimizer.cc:66)}
                           ADAM / AMSGRAD: {beta1, beta2, epsilon, weight_decay_factor, use_nesterov}
                           MOVING_AVERAGE: {momentum}     BATCH_SOFTMAX: none
                           GROUP_ADAGRAD: {initial_accumulator_value, beta,
                                     l2_regularization_strength, weight_decay_factor} */
  int32_t init_type;    /* MHTE_INIT_* */
  float init_value;     /* ConstantsInitializerConfig.constant; RandomUniform: minval */
  float init_value2;    /* RandomUniformInitializerConfig.maxval */
} mhte_segment_config;

/* EmbeddingHashTableConfig (embedding_hash_table.proto:70-95) + SlotExpireTimeConfig (:54-64) */
typedef struct {
  const char* name;
  int32_t n_segments;
  const mhte_segment_config* segments;
  uint64_t initial_capacity;     /* slots; hashpower = reserve_calc(initial_capacity),
                                    cuckoohash_map.hpp:2114-2121; proto default 1 */
  uint64_t reserve_rows;         /* MI355X extension: rows of HBM slab to allocate up front (0 = grow
                                    on demand in 2^20-row slabs) */
  float max_load_factor;         /* MI355X extension: proactive doubling threshold, 0 -> 0.5 */
  int64_t default_expire_days;   /* SlotExpireTimeConfig.default_expire_time; 0 (unset) -> 36500, the
                                    proto default; negative -> a TTL of 0 days */
  int32_t n_slot_expire;
  const int64_t* expire_slots;   /* host */
  const int32_t* expire_days;    /* host */
  /* SlotOccurrenceThresholdConfig (embedding_hash_table.proto:98-110): an id that is not in the
     table yet is admitted once the attached hash filter has seen it this many times; <= 0: always */
  int32_t default_occurrence_threshold;
  int32_t n_slot_occurrence;
  const int64_t* occurrence_slots;      /* host */
  const int32_t* occurrence_thresholds; /* host */
  /* EmbeddingHashTableConfig.enable_feature_eviction / feature_evict_every_n_hours (:84-87): the
     reference's bridge runs a thread per table that wakes every 10 s and evicts once that many
     hours have passed (RT/ops/embedding_hash_table_tf_bridge.cc:73-104).  A scan that rewrites
     buckets has to be ordered with the table's other work, so here the same check rides on the
     update entry points (Optimize / FusedOptimize / the step's backward) and the scan is enqueued on
     their stream. */
  int32_t enable_feature_eviction;
  int32_t feature_evict_every_n_hours;  /* <= 0 -> 240 */
} mhte_table_config;

typedef struct mhte_multi_table mhte_multi_table;
typedef struct mhte_hash_filter mhte_hash_filter;   /* the admission filter resource, below */

/* CreateMonolithMultiHashTable (RT/ops/multi_hash_table_op.cc:44-112).  `configs` may be in any
 * order; tables are stored sorted by name.  device = HIP device ordinal. */
mhte_status mhte_multi_table_create(const mhte_table_config* configs, int32_t n_tables,
                                    int32_t device, const char* shared_name,
                                    mhte_multi_table** out);
void mhte_multi_table_destroy(mhte_multi_table* t);
/* CreateMonolithMultiHashTable taking its `config` input as is: the serialized
 * MultiEmbeddingHashTableConfig (RT/hash_table/embedding_hash_table.proto:93-96; names / configs of
 * different length -> InvalidArgument as RT/ops/multi_hash_table_op.cc:50-53).  `filter` (may be NULL)
 * is the filter_handle input; its occurrence thresholds (mhte_hash_filter_create_from_proto) become
 * the tables'.  reserve_rows / max_load_factor: the MI355X extensions of mhte_table_config, applied to
 * every table (0: defaults).  learning_rates_out (optional, host float[cap]) receives the configs' own
 * per-segment learning rates in table order (the ops take the live values as an input).
 * Segment.comp_config picks each segment's training retriever as the reference does
 * (RT/hash_table/entry_accessor.cc:283-302; mhte_table_set_retriever below). */
mhte_status mhte_multi_table_create_from_proto(const void* config, int64_t config_len,
                                               mhte_hash_filter* filter, uint64_t reserve_rows,
                                               float max_load_factor, int32_t device,
                                               const char* shared_name, float* learning_rates_out,
                                               int32_t learning_rates_cap, mhte_multi_table** out);
/* ReadMonolithMultiHashTable / IsHashTableInitialized (RT/ops/multi_hash_table_op.cc:137-166): the
 * live table created under `shared_name`, or NULL / 0. */
mhte_multi_table* mhte_multi_table_find(const char* shared_name);
int32_t mhte_multi_table_is_initialized(const char* shared_name);
int32_t mhte_num_tables(const mhte_multi_table* t);
const char* mhte_table_name(const mhte_multi_table* t, int32_t i);
int32_t mhte_table_dim(const mhte_multi_table* t, int32_t i);        /* dim_size() */
int32_t mhte_table_slice_size(const mhte_multi_table* t, int32_t i); /* slice_size() */
int32_t mhte_table_index(const mhte_multi_table* t, const char* name); /* -1 when absent */
const char* mhte_shared_name(const mhte_multi_table* t);

/* MonolithMultiHashTableLookup (RT/ops/multi_hash_table_lookup_op.cc:33-89,200-209).
 * id [dev, id_split[n_split-1]], id_split [host, n_tables+1], embedding [dev, sum n_t*dim_t].
 * Absent ids produce zeros and are not inserted. */
mhte_status mhte_lookup(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                        int64_t n_split, float* embedding, int64_t embedding_len, void* stream);

/* flags for the mutating ops */
enum {
  MHTE_IDS_UNIQUE = 1,   /* caller guarantees ids are distinct within each table segment (they come
                            from unique_key_with_value_and_offset / FusedReorderByIndices); skips
                            the in-op grouping pass */
  MHTE_SUM_DUPLICATES = 2 /* enable_grad_accumulation / enable_dedup: add duplicates' gradients,
                            then ONE optimizer step (RT/ops/embedding_hash_table_tf_bridge.cc:270-310).
                            Default: one optimizer step per occurrence, in order
                            (cuckoo_embedding_hash_table.cc:229-236). */
};

/* MonolithMultiHashTableOptimize (RT/ops/multi_hash_table_update_op.cc:47-100).
 * learning_rate [host, sum slice_size_t]; update_time seconds (stored as uint32). */
mhte_status mhte_optimize(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                          int64_t n_split, const float* value, int64_t value_len,
                          const float* learning_rate, int64_t n_learning_rate, int64_t update_time,
                          int64_t global_step, int32_t flags, void* stream);
/* MonolithMultiHashTableAssign (:106-145) */
mhte_status mhte_assign(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                        int64_t n_split, const float* value, int64_t value_len, int64_t update_time,
                        int32_t flags, void* stream);
/* MonolithMultiHashTableAssignAdd (:147-190) */
mhte_status mhte_assign_add(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                            int64_t n_split, const float* value, int64_t value_len,
                            int64_t update_time, int32_t flags, void* stream);
/* MonolithMultiHashTableReinitialize (:192-245).  id_status [dev, n]: -1 unknown table (not an
 * error), 0 inserted, 1 existed.  `now` replaces absl::Now() so runs are reproducible; pass 0 to
 * use the wall clock. */
mhte_status mhte_reinitialize(mhte_multi_table* t, const char* table_name, const int64_t* id,
                              int64_t n, int32_t* id_status, int64_t now, void* stream);

/* ComputeFusedOffsets (RT/hash_table/utils.h:29-61), host arithmetic. */
mhte_status mhte_compute_fused_offsets(const mhte_multi_table* t, const int32_t* fused_slot_size,
                                       int32_t num_of_shards, int32_t* id_offsets,
                                       int32_t* embedding_offsets, int32_t* embedding_splits,
                                       int64_t* total_ids, int64_t* total_embeddings);
/* MonolithMultiHashTableFusedLookup (RT/ops/multi_hash_table_lookup_op.cc:128-197,229-255).
 * ids [dev], fused_slot_size [host, num_of_shards*n_tables] (shard-major, table-minor);
 * embeddings [dev, total_embeddings from mhte_compute_fused_offsets];
 * embedding_splits [host, num_of_shards], id_offsets / embedding_offsets [host, N*T+1].
 * ONE launch over the N*T segments (the reference loops over the tables inside Shard() over the
 * shards, :150-196) when the model has <= 32 tables whose rows are whole float4s (up to 256 floats)
 * or of any layout up to 64 floats; otherwise table by table. */
mhte_status mhte_fused_lookup(mhte_multi_table* t, const int64_t* ids,
                              const int32_t* fused_slot_size, int32_t num_of_shards,
                              int64_t req_time, float* embeddings, int64_t embeddings_len,
                              int32_t* embedding_splits, int32_t* id_offsets,
                              int32_t* embedding_offsets, void* stream);
/* MonolithMultiHashTableFusedOptimize (RT/ops/multi_hash_table_update_op.cc:247-325).
 * enable_grad_accumulation == (flags & MHTE_SUM_DUPLICATES).
 * With MHTE_IDS_UNIQUE (ids distinct inside every segment, which is what FusedReorderByIndices
 * hands over) the N*T segments are ONE upsert launch + one displacement launch; without it every
 * segment is grouped and applied on its own. */
mhte_status mhte_fused_optimize(mhte_multi_table* t, const int64_t* ids,
                                const int32_t* fused_slot_size, const float* id_grads,
                                int64_t id_grads_len, const int32_t* id_offsets,
                                const int32_t* grad_offsets, const float* learning_rates,
                                int64_t n_learning_rates, int64_t req_time, int64_t global_step,
                                int32_t num_of_shards, int32_t flags, void* stream);

/* MonolithMultiHashTableLookupEntry (RT/ops/multi_hash_table_lookup_op.cc:91-118,214-223): the
 * serialized EntryDump (embedding_hash_table.proto:45-50) of every id — what Save writes for it —
 * and an empty string for an id the table does not hold (cuckoo_embedding_hash_table.cc:174-182).
 * Strings are host data in TF: entries [host, cap bytes] receives them back to back,
 * entry_offsets [host, n + 1] where each starts.  *needed = total bytes; cap too small ->
 * MHTE_INVALID_ARGUMENT with *needed set.  Synchronises. */
mhte_status mhte_lookup_entry(mhte_multi_table* t, const int64_t* id, const int64_t* id_split,
                              int64_t n_split, char* entries, int64_t cap, int64_t* entry_offsets,
                              int64_t* needed, void* stream);
/* MonolithHashTableSaveAsTensor (RT/ops/hash_table/misc_ops.cc:46-94; op :96-109): one table's entries
 * as serialized EntryDump strings, `limit` at a time, resumable — the table iterated in Save's order
 * (cuckoohash_map.hpp:740-773 partial_dump: bucket range of shard `shard_idx` of `num_shards`, resumed
 * `offset` slots into it; the count is checked after an entry is taken, so limit <= 0 still yields one).
 * *new_offset is the op's first output: behind the last entry when the limit stopped the scan, one
 * bucket past the shard's range when the range ran out (call again until *n_entries == 0).
 * entries / entry_offsets [host]: as mhte_lookup_entry (offsets_cap >= limit + 1 values).  Synchronises. */
mhte_status mhte_table_save_as_tensor(mhte_multi_table* t, int32_t table, int32_t shard_idx,
                                      int32_t num_shards, int64_t limit, int64_t offset, int64_t* new_offset,
                                      char* entries, int64_t cap, int64_t* entry_offsets,
                                      int64_t offsets_cap, int64_t* n_entries, int64_t* needed, void* stream);
/* MonolithHashTableLookupGradient (RT/ops/hash_table_lookup_op.cc:110-147; op :254-270): the gradient of
 * a lookup gathered back per (batch row, id) pair of a sparse id tensor:
 *   out_ids[i] = id_values[i],  out_grads[i, :] = input_grads[id_indices[i * index_cols], :]
 * id_indices [dev, n x index_cols] (column 0 = the batch row), id_values [dev, n], input_grads
 * [dev, n_rows x dim] -> out_ids [dev, n], out_grads [dev, n x dim].  A row outside [0, n_rows) is
 * InvalidArgument (its output row is zeros; the reference indexes unchecked).  Synchronises. */
mhte_status mhte_lookup_gradient(const int64_t* id_indices, int64_t n, int64_t index_cols,
                                 const int64_t* id_values, const float* input_grads, int64_t n_rows,
                                 int32_t dim, int64_t* out_ids, float* out_grads, void* stream);
/* MonolithMultiHashTableFeatureStat (RT/ops/multi_hash_table_save_restore_ops.cc:424-497,522-530):
 * entries per table name summed over the .meta sidecars of a checkpoint.  names [host, names_cap
 * bytes]: the names, each NUL-terminated, sorted; counts [host, cap]. */
mhte_status mhte_feature_stat(const char* basename, char* names, int64_t names_cap, uint64_t* counts,
                              int32_t cap, int32_t* n_out);
/* Test hook for the eviction cadence: moves the library's clock forward by `seconds`. */
void mhte_advance_clock_for_testing(double seconds);

/* ---- introspection / maintenance ----------------------------------------------------------- */
/* Size() (RT/hash_table/embedding_hash_table_interface.h); synchronises the stream. */
mhte_status mhte_table_size(mhte_multi_table* t, int32_t table, int64_t* size, void* stream);
/* Contains() for a batch: out [dev, n] 0/1 */
mhte_status mhte_table_contains(mhte_multi_table* t, int32_t table, const int64_t* id, int64_t n,
                                int32_t* out, void* stream);
/* Evict(max_update_time) (cuckoo_embedding_hash_table.cc:251-264).  max_update_time < 0 uses the
 * table's own fuzzy max of all update_times seen (tf_bridge.cc:262-263). */
mhte_status mhte_table_evict(mhte_multi_table* t, int32_t table, int64_t max_update_time,
                             void* stream);
/* Compaction: eviction empties bucket slots but the rows of the evicted ids stay allocated.  This moves
 * the rows of the live entries into the lowest row handles and releases the row slabs above them; keys,
 * bucket positions, timestamps, dump order and every row's bits are unchanged.  Safe between any two
 * calls: whatever was resolved ahead against the table (a step's hints, rows reserved for the next
 * batch) is resolved again.  FAILED_PRECONDITION on a capturing stream.
 * out[0] = row handles in use before, [1] = after (= live keys, + 1 when the reserved key is stored),
 * [2] = rows moved, [3] = bytes of row slabs released.  Synchronises the stream. */
mhte_status mhte_table_compact(mhte_multi_table* t, int32_t table, int64_t out[4], void* stream);
/* min_free_fraction in (0, 1]: after every eviction scan of this table (cadence or explicit) compact
 * when (handles in use - live) / handles in use >= it.  0 (default): never. */
mhte_status mhte_table_set_auto_compact(mhte_multi_table* t, int32_t table, double min_free_fraction);
/* Table geometry: hashpower, rows allocated, lookup hits since last call. Synchronises. */
typedef struct {
  int64_t size;
  int32_t hashpower;
  int64_t rows_allocated;
  int64_t lookup_hits;
  int64_t dropped;      /* ids dropped because displacement failed (0 unless max_load_factor ~ 1) */
  int64_t evicted;
  int64_t max_update_ts;
  int64_t bytes_buckets;
  int64_t bytes_rows;
} mhte_table_stats;
mhte_status mhte_table_get_stats(mhte_multi_table* t, int32_t table, mhte_table_stats* out,
                                 void* stream);
/* Lookup hit counting (the `lookup_fid_hit_rate` metric of RT/ops/multi_hash_table_lookup_op.cc
 * :81-87, emitted by the reference for serving tables only).  Off by default: it costs one global
 * atomic per wavefront. */
mhte_status mhte_table_set_count_hits(mhte_multi_table* t, int32_t table, int32_t enable);
/* Dump in bucket-major order (Save's iteration order, cuckoohash_map.hpp:740-773).
 * All outputs dev, capacity `cap` entries; rows may be NULL; row_floats = dim + optimizer state.
 * Returns the number of entries in *n_out. Synchronises. */
mhte_status mhte_table_dump(mhte_multi_table* t, int32_t table, int64_t cap, int64_t* ids,
                            int64_t* positions, uint32_t* ts, float* rows, int64_t* n_out,
                            void* stream);
int32_t mhte_table_row_floats(const mhte_multi_table* t, int32_t i);

/* ---- the step right after the exchange: gather per merged slot, its gradient, ragged reductions --
 * MonolithFusedGatherEmbeddingsByInput (+Gradient) (RT/ops/map_id_to_embedding.cu.cc:31-118,
 * NT/distribution_ops.py:671-686): outputs[i][j, :] = fused_embeddings[offsets[i][j] + 0 .. dims[i]);
 * gradient: fused_grad (zero-filled here, fused_len floats) += grads[i][j, :] * scale at the same
 * offsets.  No float atomics: the rows that share a destination are grouped and added in row order
 * (rows numbered input after input; acc = 0, acc = acc + g * scale, the product rounded first), each
 * row with its own dims[i] columns, then fused_grad += acc.  Inputs are taken in chunks of 32, added
 * chunk after chunk.  Precondition: two rows either share an offset or their ranges
 * [offset, offset + dim) are disjoint, and every range lies inside fused_len.
 * MHTE_POOL_ATOMICS=1 (read once per process) selects the atomic forms of the gradient and of the
 * unsorted reduction instead: the reference's GpuAtomicAdd, arrival order.
 * offsets / outputs / grads: HOST arrays of n_inputs device pointers; n, dims: host arrays.
 * MonolithReduceSum / ReduceMean / ReduceSquareNorm (RT/ops/reduce_op.cc:29-125,
 * NT/embedding_combiners.py:41-102): out[b, :] over the rows i with indices[i] == b; mode 0 sum,
 * 1 mean (an empty output is NaN), 2 sqrt of the sum of squares.  Both default forms add the rows of
 * an output in index order, bit-identical to the reference's sequential loop: indices_sorted != 0
 * (the layout sparse/ragged inputs have) finds each output's segment by binary search, otherwise the
 * rows are grouped by a stable sort first.  Both ignore an index outside [0, batch); the atomic form
 * uses the index as an address unchecked, as the reference does. */
mhte_status mhte_fused_gather_embeddings_by_input(const float* fused_embeddings, int32_t n_inputs,
                                                  const int32_t* const* offsets, const int64_t* n,
                                                  const int32_t* dims, float* const* outputs,
                                                  void* stream);
mhte_status mhte_fused_gather_embeddings_by_input_gradient(float* fused_grad, int64_t fused_len,
                                                           int32_t n_inputs,
                                                           const float* const* grads,
                                                           const int32_t* const* offsets,
                                                           const int64_t* n, const int32_t* dims,
                                                           float scale, void* stream);
mhte_status mhte_reduce_rows(const int64_t* indices, const float* values, int64_t n, int32_t dim,
                             int64_t batch, int32_t mode, int32_t indices_sorted, float* out,
                             void* stream);
/* MonolithFusedGatherEmbeddingsByInputGradient with the reference's `scale` INPUT left where synchronous
 * GPU training computes it (NT/distributed_ps_sync.py:313-331: min(clip_norm / global_norm, 1), a tensor):
 * scale_dev [dev f32, 1] is read once at the top of every kernel (a uniform load); per addend the same arithmetic as the entry point
 * above called with that value (acc + x * scale), the same launches.  Nothing reaches the host, and a
 * captured graph replays with whatever the word holds then. */
mhte_status mhte_fused_gather_embeddings_by_input_gradient_dev_scale(float* fused_grad, int64_t fused_len,
                                                                     int32_t n_inputs,
                                                                     const float* const* grads,
                                                                     const int32_t* const* offsets,
                                                                     const int64_t* n, const int32_t* dims,
                                                                     const float* scale_dev, void* stream);

/* ---- clip by global norm (csrc/mhte_clip_kernels.h) ------------------------------------------------
 * GlobalL2Reduce, MonolithClipByGlobalNorm, MonolithClipByGlobalNormFused (RT/ops/clip_by_global_norm.h
 * :31-60, clip_by_global_norm_op.cc, clip_by_global_norm.cu.cc, clip_by_global_norm_fused.cu.cc:37-165;
 * NT/clip_ops.py:25-80; the default gradient clip of NT/feature_utils.py:211-264).
 *   tensors / inputs / outputs   HOST arrays of n device pointers (fp32); lens HOST [n], floats per tensor
 *                                (int64: no 2^31 cap; 0 is legal, its pointer is not looked at)
 *   result                       [dev f32, 4]: [0] sum of squares, [1] norm = sqrt([0]), [2] scale =
 *                                norm > clip_norm ? clip_norm / norm : 1 (clip_by_global_norm.h:42-43),
 *                                [3] 0.  A NaN norm gives scale 1, an infinite one scale 0 (the clipped
 *                                values are then NaN, as NT/clip_ops_test.py:53-58 expects).
 * The sum of squares is one fixed tree over chunks of 4096 consecutive floats per tensor — 1024 partial
 * sums, each a thread-serial chain over its chunks followed by halvings, then halvings of the partials;
 * products and sums rounded to fp32 one by one, no FMA, no float atomics (the reference's GPU kernels add
 * block sums with atomicAdd: other bits every run) — so the result depends on the tensors' contents,
 * lengths and order only, not on the grid, the device or the run.  tests/clip_ops_truth.py restates it.
 * The scale stays in HBM: the fused form sums the partials again in the prologue of its second launch
 * (the reference waits for the stream there, clip_by_global_norm_fused.cu.cc:150), and result + 2 is what
 * mhte_scale_tensors_dev and mhte_fused_gather_embeddings_by_input_gradient_dev_scale take.  No entry
 * point waits for the device or reads a device value; the partials live in the per-device auxiliary
 * workspace (allocated by the first call; calls on several streams are ordered by events).  Up to 128
 * non-empty tensors travel in the kernel arguments; more are uploaded per call (any number; such a call
 * cannot be captured into a graph).  out[i] == in[i] is allowed; an in-place tensor is not touched at
 * all when the scale is exactly 1 ("no clip: the outputs are the inputs"), any other is copied.
 * 16-byte accesses where a pointer is 16-byte aligned, else 4-byte ones (same bits).
 * InvalidArgument, checked on the host before any device call, the entry point's name in the message: a
 * null argument, n < 0, a negative length, a null pointer for a non-empty tensor, clip_norm negative or
 * NaN.  n = 0 is legal: sum 0, norm 0, scale 1.
 *   mhte_global_l2_reduce           GlobalL2Reduce + the deferred scale (feature_utils' cond_defer_clip);
 *                                   clip_norm = +inf: the norm alone.  Two launches.
 *   mhte_clip_by_global_norm        MonolithClipByGlobalNorm with the norm on the host: one launch, none
 *                                   for in-place tensors when global_norm <= clip_norm
 *   mhte_clip_by_global_norm_dev    the same with the norm in a device word: one launch
 *   mhte_clip_by_global_norm_fused  MonolithClipByGlobalNormFused: two launches, no wait between them
 *   mhte_scale_tensors_dev          out[i] = in[i] * *scale_dev for all tensors in one launch (the
 *                                   multiply NT/distribution_ops.py:535-549 does per layout tensor with
 *                                   layout_tensors_grad_scale before fused_embedding_to_layout_grad) */
mhte_status mhte_global_l2_reduce(const float* const* tensors, const int64_t* lens, int32_t n, float clip_norm,
                                  float* result, void* stream);
mhte_status mhte_clip_by_global_norm(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                     int32_t n, float global_norm, float clip_norm, void* stream);
mhte_status mhte_clip_by_global_norm_dev(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                         int32_t n, const float* global_norm_dev, float clip_norm, void* stream);
mhte_status mhte_clip_by_global_norm_fused(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                           int32_t n, float clip_norm, float* result, void* stream);
mhte_status mhte_scale_tensors_dev(const float* const* inputs, float* const* outputs, const int64_t* lens,
                                   int32_t n, const float* scale_dev, void* stream);

/* ---- aligned flat concat / split (csrc/mhte_flat_kernels.h) ----------------------------------------
 * MonolithAlignedFlatConcat and MonolithAlignedFlatSplit (RT/ops/aligned_concat_split.cu.cc:32-57, :63-128)
 * with the layout rule of FusedAlignedOutputAllocator (RT/ops/alloc_utils.h:50-95): the allreduce side of
 * the deferred clip (NT/feature_utils.py:48-99 allreduce_cond with fusion 'one', :251-264 cond_defer_clip).
 *   inputs        HOST array of n device pointers (fp32); lens HOST [n], floats per tensor (0 is legal: the
 *                 tensor occupies nothing and its pointer is not looked at)
 *   align_elems   A, the alignment of every tensor's start in ELEMENTS: a power of two in [4, 1024]
 *                 (the reference's is EIGEN_MAX_ALIGN_BYTES / sizeof(float) of its build: 16 for 64 bytes)
 *   offsets       HOST [n + 1]: offsets[i] = the sum of round_up(lens[j], A) over j < i; offsets[n] the total
 *   out           [dev, out_elems] fp32 (wire 0) or fp16 (wire 1), 16-byte aligned; out_elems == offsets[n]
 * out[offsets[i] + k] = in[i][k] * scale for k < lens[i] — one fp32 product, rounded once, then for fp16 one
 * conversion to nearest-even (overflow gives inf, subnormals are kept) — and +0 from there to offsets[i + 1],
 * whatever the scale (the reference's `out[id] = 0.0f`).  scale_dev != NULL: the factor is a device word read
 * once at the top of the kernel (scale is then not used) — result + 2 of mhte_global_l2_reduce; a captured
 * graph replays with whatever the word holds then.  One launch per call, none for n == 0 or a total of 0; no
 * entry point waits for the device, reads a device value or allocates after the first call.  Up to 128
 * non-empty tensors travel in the kernel arguments; more are uploaded per call (such a call cannot be
 * captured into a graph).  Sources that are 16-byte aligned are read with 16-byte loads, others with 4-byte
 * loads: the same bits.
 * InvalidArgument, checked on the host before any device call, the entry point's name in the message: a
 * null argument, n < 0, a negative length, a null pointer for a non-empty tensor, an align_elems that is
 * not a power of two in [4, 1024], a wire other than 0 or 1, out_elems != offsets[n], an out that is not
 * 16-byte aligned, 2^31 or more chunks of 4096 elements.
 *   mhte_aligned_flat_offsets   the layout alone: host only, no device call
 *   mhte_aligned_flat_concat    MonolithAlignedFlatConcat (+ the fp16 compression of the allreduce)
 *   mhte_aligned_flat_decode    out[k] = float(flat[k]) * post_scale over total_elems elements: the way back
 *                               from the wire format and the division by the number of ranks (the
 *                               reference's op=Average); fp32 may be decoded in place (out == flat).
 *                               MonolithAlignedFlatSplit itself copies nothing: its outputs are views at
 *                               offsets[i] (monolith_amd/distribution_ops.py aligned_flat_split) */
mhte_status mhte_aligned_flat_offsets(const int64_t* lens, int32_t n, int32_t align_elems, int64_t* offsets);
mhte_status mhte_aligned_flat_concat(const float* const* inputs, const int64_t* lens, int32_t n, int32_t align_elems,
                                     float scale, const float* scale_dev, int32_t wire, void* out, int64_t out_elems,
                                     void* stream);
mhte_status mhte_aligned_flat_decode(const void* flat, int32_t wire, int64_t total_elems, float post_scale, float* out,
                                     void* stream);

/* ---- dense optimizers (csrc/mhte_dense_opt_core.h, mhte_dense_opt_kernels.h) --------------------------
 * ResourceApplyAdamom (the reference's is CPU only) and ResourceApplyRmsprop V1 / V2
 * (NT/optimizers/{adamom,rmsprop}.py, NT/optimizers/cc/training_ops.cc, NT/optimizers/cc/kernels/
 * training_ops{.h,.cc,_gpu.cu.cc}; the expression trees of kernels/training_ops.cc:34-121), applied to ALL
 * variables in ONE launch: what consumes the gradients of the deferred clip and the aligned flat allreduce.
 *   vars          HOST array of n device pointers (fp32, updated in place); lens HOST [n], floats per variable
 *                 (0 is legal: the variable occupies nothing and its pointer is not looked at)
 *   m, v, c       [dev f32, slot_elems] the FLAT slots, 16-byte aligned, in the layout of
 *                 mhte_aligned_flat_offsets(lens, align_elems): element k of variable i lives at offsets[i] + k,
 *                 slot_elems == offsets[n]; the padding between variables is never read or written
 *   the gradient  exactly one of
 *                   grads       HOST array of n device pointers (fp32; wire must be 0).  A NULL entry: the
 *                               variable takes no part in this call — its var and all its slot elements,
 *                               Adamom's c included, keep their bits (TensorFlow skips None gradients too);
 *                   grads_flat  [dev, slot_elems] ONE flat buffer in the same aligned layout, fp32 (wire 0) or
 *                               fp16 (wire 1), 16-byte aligned: where the allreduce left the gradients
 *   grad_scale / grad_scale_dev, lr / lr_dev   each a kernel argument or, when the pointer is not NULL, a
 *                 device word read once at the top of the kernel (the argument is then not used): result + 2
 *                 of mhte_global_l2_reduce, a learning-rate schedule that stays on the device.  A captured
 *                 graph replays with whatever the words hold then.
 * Per element, everything fp32, every operation rounded on its own (no FMA), sqrt and / correctly rounded,
 * rsqrt(x) := 1 / sqrt(x); g0 the gradient element (an fp16 one converted exactly):
 *   grad = g0 * grad_scale                 (always one rounded product, also for a scale of 1)
 *   g    = (weight_decay * var) + grad
 *   Adamom:   if update_slots:  m = (mom_decay * m) + ((1 - mom_decay) * g);  v = (ada_decay * v) + (g * g);
 *                               c = (ada_decay * c) + 1
 *             v1: var = var - ((m * lr) * rsqrt((v / c) + epsilon))
 *             v2: var = var - ((m * lr) / (sqrt(v / c) + epsilon))
 *             update_slots == 0 still moves var (fresh slots give 0 / 0: NaN, as IEEE has it)
 *   RMSprop:  v1: v = v + (((g * g) - v) * (1 - beta2));  m = (beta1 * m) + ((g * lr) * rsqrt(v + epsilon))
 *             v2: v = (beta2 * v) + (g * g);              m = (beta1 * m) + ((g * lr) / (sqrt(v) + epsilon))
 *             var = var - m;  update_slots == 0 changes nothing at all and launches nothing
 * (not the sparse per-row RMSprop of the tables, RT/hash_table/optimizer/rmsprop_optimizer.cc).
 * One launch per call, none for n == 0 or when no element takes part; no entry point waits for the device,
 * reads a device value or allocates after the first call.  Up to MHTE_DENSE_OPT_INLINE variables that take
 * part travel in the kernel arguments; more are uploaded per call (such a call cannot be captured into a
 * graph).  16-byte accesses where a pointer is 16-byte aligned, else 4-byte ones (same bits); packed 8-byte
 * loads for an fp16 gradient.
 * InvalidArgument, checked on the host before any device call, the entry point's name in the message: a
 * null required argument, n < 0, a negative length, a null vars[i] for a non-empty variable, both or neither
 * of grads / grads_flat, a wire other than 0 or 1, wire 1 with the list, an align_elems that is not a power
 * of two in [4, 1024], slot_elems != offsets[n], a slot or flat buffer that is not 16-byte aligned, 2^31 or
 * more chunks of 4096 elements, update_slots or use_v2 other than 0 or 1. */
#define MHTE_DENSE_OPT_INLINE 96
mhte_status mhte_dense_apply_adamom(float* const* vars, const int64_t* lens, int32_t n, int32_t align_elems, float* m,
                                    float* v, float* c, int64_t slot_elems, const float* const* grads,
                                    const void* grads_flat, int32_t wire, float grad_scale,
                                    const float* grad_scale_dev, float lr, const float* lr_dev, float ada_decay,
                                    float mom_decay, float epsilon, float weight_decay, int32_t update_slots,
                                    int32_t use_v2, void* stream);
mhte_status mhte_dense_apply_rmsprop(float* const* vars, const int64_t* lens, int32_t n, int32_t align_elems, float* m,
                                     float* v, int64_t slot_elems, const float* const* grads, const void* grads_flat,
                                     int32_t wire, float grad_scale, const float* grad_scale_dev, float lr,
                                     const float* lr_dev, float beta1, float beta2, float epsilon, float weight_decay,
                                     int32_t update_slots, int32_t use_v2, void* stream);

/* ---- FFM feature cross (csrc/mhte_ffm_core.h, mhte_ffm_kernels.h, mhte_ffm_host.h) ----------------------
 * The ops FFM and FFMGrad (NT/layers/ops/ffm_ops.cc; shapes and checks NT/layers/kernels/ffm_kernels.h:46-157;
 * loops ffm_kernels.cc:28-103, ffm_kernels.cu.cc:34-168; Python NT/layers/layer_ops.py:24-46), the cross of the
 * GroupInt / FFM layer (NT/layers/feature_cross.py:69-146).  All operands [dev f32], row-major, dense:
 *   left [batch, left_cols], right [batch, right_cols];  L = left_cols / dim_size, R = right_cols / dim_size
 *   (integer division: columns beyond L * dim_size / R * dim_size are never read), D = dim_size
 *   int_type 0, multiply:  out [batch, L R D],  out[b, (l R + r) D + k] = left[b, l D + k] * right[b, r D + k]
 *   int_type 1, dot:       out [batch, L R],    out[b, l R + r] = the sum over k = 0 .. D-1 of those products,
 *                          started from +0 and taken in ascending k
 *   mhte_ffm_grad:  grad [batch, grad_cols] with grad_cols / D (multiply) resp. grad_cols (dot) == L R features,
 *                   left_grad [batch, left_cols], right_grad [batch, right_cols] (full widths; +0 beyond L D / R D):
 *                     left_grad[b, l D + k]  = +0 + g(l,0,k) right[b, 0 D + k] + ... + g(l,R-1,k) right[b, (R-1) D + k]
 *                     right_grad[b, r D + k] = +0 + g(0,r,k) left[b, 0 D + k]  + ... + g(L-1,r,k) left[b, (L-1) D + k]
 *                   g(l,r,k) = grad[b, (l R + r) D + k] (multiply), grad[b, l R + r] (dot); sums left to right
 * Every product and every sum is one fp32 operation rounded on its own (no FMA), no atomics: the same bits on
 * every run and in every kernel form.  One launch per call (the gradient: one for both outputs), none for an empty
 * problem (batch == 0, L == 0 or R == 0; the gradient of an empty cross is cleared without a kernel); no entry
 * point waits for the device, reads a device value or allocates: a call can be captured into a graph.  16-byte
 * accesses when D % 4 == 0, the pointers are 16-byte aligned and the row widths multiples of 4 floats, else
 * 4-byte ones; operands staged in LDS when a batch row's share fits (32 KiB forward, 64 KiB gradient), else read
 * where they lie.
 * mhte_ffm_launch_counts: the launches of this process by kernel form, n must be 16, index
 *   8 * (0 forward, 1 gradient) + 4 * (0 multiply, 1 dot) + 2 * (0 16-byte form, 1 4-byte form) + (0 LDS, 1 direct).
 * InvalidArgument, checked on the host before any device call, the entry point's name and the argument in the
 * message: a null pointer for a non-empty operand, a pointer that is not 4-byte aligned, a negative size,
 * dim_size < 1, an int_type other than 0 / 1, an out_cols that is not L R D resp. L R, gradient features != L R
 * ("the in/out shape not match", as FFMGradOp says), batch, a row width or L R D of 2^31 or more. */
mhte_status mhte_ffm(const float* left, int64_t left_cols, const float* right, int64_t right_cols, int64_t batch,
                     int32_t dim_size, int32_t int_type, float* out, int64_t out_cols, void* stream);
mhte_status mhte_ffm_grad(const float* grad, int64_t grad_cols, const float* left, int64_t left_cols,
                          const float* right, int64_t right_cols, int64_t batch, int32_t dim_size, int32_t int_type,
                          float* left_grad, float* right_grad, void* stream);
mhte_status mhte_ffm_launch_counts(int64_t* out, int32_t n);

/* ---- in-batch AUC loss (csrc/mhte_auc_core.h, mhte_auc_kernels.h, mhte_auc_host.h) -----------------------
 * The ops InbatchAucLoss and InbatchAucLossGrad (RT/ops/inbatch_auc_loss.cc:30-138: CPU only, two nested loops,
 * one float accumulator; Python NT/losses/inbatch_auc_loss.py, test NT/losses/inbatch_auc_loss_test.py): the leg
 * from the dense tower's logit to the dy of its backward.  label, logit [dev f32, n] (any shape, n elements):
 *   element i is positive if label[i] > 0, negative if it is not positive and label[i] > -10000, ignored
 *   otherwise (a NaN label is ignored).  For every positive i and negative j, diff = logit[i] - logit[j]:
 *     -87 < diff < 88:   t = diff - log(1 + exp(diff)),  s = 1 - 1 / (1 + exp(-diff))
 *     diff <= -87:       t = diff,                       s = 1
 *     otherwise (diff >= 88 or NaN):  t = 0,             s = 0
 *   loss = sum t_ij (<= 0, the reference's sign);  logit_grad[i] = grad * sum_j s_ij for a positive,
 *   logit_grad[j] = -grad * neg_weight * sum_i s_ij for a negative, +0 for an ignored element, for every element
 *   when there is no positive or no negative, and wherever the product is a zero of either sign.
 * The middle branch is fp32 in the form that cancels nothing, e = exp(-|diff|): t = -log1p(e) resp.
 * diff - log1p(e), s = e / (1 + e) resp. 1 / (1 + e) for diff >= 0 resp. < 0.  Every sum is fp64, in an order
 * fixed by n and the two counts, rounded to fp32 once (the gradient after the multiplication by neg_weight and
 * grad); no atomics: the same bits on every run.
 *   mhte_inbatch_auc_loss:       loss [dev f32, 1]; unit_grad [dev f32, n] or NULL: the gradient for grad = 1,
 *                                from the same launches (t and s share e).
 *   mhte_inbatch_auc_loss_grad:  logit_grad [dev f32, n]; grad_dev NULL, or a device word that replaces grad.
 * Five launches per call (classes per tile, their scan, the stable compaction of both classes, the pair kernel,
 * the final pass), none for n == 0 (the loss is then cleared to +0 by a memset).  The number of positives and
 * negatives stays in device words: no entry point waits for the device, reads a device value or allocates beyond
 * the first growth of the per-device workspace (about 9 MB at n = 65536), so a call can be captured into a graph.
 * mhte_inbatch_auc_launch_counts: the launches of this process by kernel form, n must be 9, index 0 count,
 *   1 scan, 2 scatter, 3 / 4 / 5 the pair kernel for the loss alone / loss and gradient / gradient alone,
 *   6 / 7 / 8 the final pass for the same.
 * InvalidArgument, checked on the host before any device call, the entry point's name and the argument in the
 * message: a null pointer for a non-empty operand (loss always), a pointer that is not 4-byte aligned, n < 0 or
 * n >= 2^31, a neg_weight outside (0, 1] or NaN (the reference CHECKs it in the forward only; both refuse it). */
mhte_status mhte_inbatch_auc_loss(const float* label, const float* logit, int64_t n, float neg_weight, float* loss,
                                  float* unit_grad, void* stream);
mhte_status mhte_inbatch_auc_loss_grad(const float* label, const float* logit, int64_t n, float grad,
                                       const float* grad_dev, float neg_weight, float* logit_grad, void* stream);
mhte_status mhte_inbatch_auc_launch_counts(int64_t* out, int32_t n);

/* ---- batch softmax loss (csrc/mhte_bsm_core.h, mhte_bsm_kernels.h, mhte_bsm_host.h) ------------------------
 * The sampling-bias-corrected in-batch softmax of the two-tower model (NT/losses/batch_softmax_loss.py:18-57), the
 * consumer of the interval that MHTE_OPT_BATCH_SOFTMAX keeps per item id.  query, item [dev f32, batch x dim],
 * item_step_interval, r [dev f32, batch]:
 *   q^_i = q_i * rsqrt(max(sum q_i^2, 1e-12)), likewise i^_j (normalize = 1; the rows themselves for 0)
 *   z_ij = (q^_i . i^_j) / temperature + log(max(item_step_interval_j, 1))
 *   loss = -sum_i r_i * (z_ii - lse_i),  lse_i = m_i + log sum_j exp(z_ij - m_i),  m_i = max_j z_ij
 * The one defined deviation: the reference takes exp of the unshifted z and divides, which overflows in fp32
 * (normalised rows at temperature 0.01: exp(100) = inf, inf / inf = NaN); this is the same value wherever the
 * reference's own fp32 evaluation is finite and stays finite where it is not.
 * Gradients for query and item only (BatchSoftmaxOptimizer ignores its gradient; r gets none), with
 * G_ij = r_i * (exp(z_ij - lse_i) - [i == j]):  g_q^ = G . I^ / temperature, g_i^ = G^T . Q^ / temperature, then
 * through the normalisation of a row x, s = sum x^2, inv = rsqrt(max(s, 1e-12)):  dx = (g - x^ (x^ . g)) * inv for
 * s >= 1e-12, g * inv below.  A gradient that is a zero of either sign is written as +0.
 * The batch x batch matrix is never stored: tiles of it come from the f32-input MFMA (exact fp32, an fmaf chain
 * in a fixed permuted order), rows keep a running maximum and sum, the backward recomputes the tiles once per gradient.  No
 * atomics; the split of the columns into chunks is a function of (batch, dim) alone: the same bits on every run,
 * and whether a gradient is asked for together with the loss or on its own.
 *   mhte_batch_softmax_loss:       loss [dev f32, 1]; unit_dquery, unit_ditem [dev f32, batch x dim] or NULL: the
 *                                  gradients for grad = 1.  batch == 0: no launch, the loss is cleared to +0.
 *   mhte_batch_softmax_loss_grad:  dquery, ditem (at least one non-NULL), scaled by grad, or by the device word
 *                                  grad_dev when that is not NULL.
 *   mhte_batch_softmax_plan:       n must be 5: out = row block, column tile, chunks per row block, chunks per
 *                                  column block, workspace bytes (needs no device).
 *   mhte_batch_softmax_launch_counts: the launches of this process by kernel form, n must be 6: 0 prep, 1 row
 *                                  (forward), 2 row (gradient), 3 col, 4 final (lse, loss), 5 final (gradients).
 * Launches per call: 3 for the loss alone (prep, row, final), 4 + one per gradient with gradients (prep, row,
 * final, row gradient and / or col, final gradient), in both entry points.  No entry point waits for the device,
 * reads a device value or allocates beyond the first growth of the per-device workspace
 * (4 * (7 bp + 2 bp kp + 2 chunks bp (1 + kp)) bytes, bp and kp the padded extents: 66.2 MiB at 65536 x 64), so a
 * call can be captured into a graph.
 * InvalidArgument, checked on the host before any device call, the entry point's name and the argument in the
 * message: a null pointer for a non-empty operand (loss always), a pointer that is not 4-byte aligned, batch < 0 or
 * >= 2^24, dim outside [1, 256], a temperature that is not > 0 (NaN included), a normalize that is neither 0 nor
 * 1, a grad entry with both outputs NULL. */
mhte_status mhte_batch_softmax_loss(const float* query, const float* item, const float* item_step_interval,
                                    const float* r, int64_t batch, int32_t dim, int32_t normalize, float temperature,
                                    float* loss, float* unit_dquery, float* unit_ditem, void* stream);
mhte_status mhte_batch_softmax_loss_grad(const float* query, const float* item, const float* item_step_interval,
                                         const float* r, int64_t batch, int32_t dim, int32_t normalize,
                                         float temperature, float grad, const float* grad_dev, float* dquery,
                                         float* ditem, void* stream);
mhte_status mhte_batch_softmax_plan(int64_t batch, int32_t dim, int64_t* out, int32_t n);
mhte_status mhte_batch_softmax_launch_counts(int64_t* out, int32_t n);

/* ---- FeatureInsight (csrc/mhte_fi_core.h, mhte_fi_kernels.h, mhte_fi_host.h) -------------------------------
 * The ops FeatureInsight and FeatureInsightGrad (NT/layers/ops/feature_insight_ops.cc,
 * NT/layers/kernels/feature_insight_kernels.cc:70-83 and :148-160, NT/layers/layer_ops.py:49-85): the
 * block-diagonal product of the concatenated embeddings with the first dense layer's kernel, one block per feature.
 * input [dev f32, batch x in_cols], weight [dev f32, in_cols x k], segment_sizes [HOST i32, n_segments], their sum
 * in_cols; segment f covers the columns o_f .. o_f + s_f - 1 of input and the same rows of weight:
 *   out[b, f k + c]    = sum_{j in seg f} input[b, j] * weight[j, c]          [batch x n_segments k]
 *   input_grad[b, j]   = sum_c grad[b, f(j) k + c] * weight[j, c]             [batch x in_cols]
 *   weight_grad[j, c]  = sum_b grad[b, f(j) k + c] * input[b, j]              [in_cols x k]
 *   agg[b, f]          = sum_c out[b, f k + c]^2                              [batch x n_segments]
 * Products are exact fp32: every sum is an fmaf chain from +0 in ascending order (over the segment, over c, over
 * the rows of a batch slab); the slabs of weight_grad are added in slab order; agg squares the very bits the plain
 * op stores, in 16 interleaved chains added in order (csrc/mhte_fi_core.h states the definition).  No atomics; the
 * order of every sum is a function of the shape alone: the same bits on every run, from either entry point, and
 * whichever gradients are asked for.  A segment of size 0 is legal: its k output columns, and its agg entry, are
 * +0.  Every zero written is +0.
 *   mhte_feature_insight:       aggregate 0: out [dev f32, batch x out_cols], out_cols == n_segments * k;
 *                               aggregate 1: the fused form, out is agg, out_cols == n_segments: no intermediate
 *                               and no workspace.  batch == 0: no launch.
 *   mhte_feature_insight_grad:  grad [dev f32, batch x grad_cols], grad_cols == n_segments * k; input_grad,
 *                               weight_grad: either may be NULL, not both.  batch == 0: weight_grad is cleared to
 *                               +0 (one memset), nothing else.
 *   mhte_feature_insight_plan:  n must be 9: out = row block, column tile, chain terms per LDS stage, segments per
 *                               launch, launches per kernel form (groups), rows per batch slab, batch slabs of the
 *                               weight gradient, workspace bytes of the forward (0 in both modes), workspace bytes
 *                               of the gradient (slabs * in_cols * k * 4 for more than one slab, else 0).  Needs no
 *                               device, a function of (batch, in_cols, k, n_segments) alone.
 *   mhte_feature_insight_launch_counts: the launches of this process by kernel form, n must be 5: 0 forward,
 *                               1 aggregate, 2 input gradient, 3 weight gradient, 4 slab sum.
 * The segment offsets of a launch ride in its kernel arguments, 128 segments per launch; a longer list is cut into
 * groups of 128 consecutive segments, one launch per group and kernel form: nothing is uploaded, so nothing can be
 * stale under graph replay or when the list changes between calls.  n_segments is at most 4096 (32 launches).
 * Launches per call: groups (forward, either mode); groups per gradient asked for, groups that hold only empty
 * segments left out, plus the slab sum when the plan has more than one slab.  No entry point waits for the device,
 * reads a device value or allocates beyond the first growth of the per-device workspace (the slab partials), so a
 * call can be captured into a graph.
 * InvalidArgument, checked on the host before any device call, the entry point's name and the argument in the
 * message: a null pointer for a non-empty operand (segment_sizes always), a pointer that is not 4-byte aligned,
 * batch < 0 or > 2^30 - 64, in_cols outside [0, 4194240], k outside [1, 4194240], n_segments outside [1, 4096], a
 * negative segment size, a sum of sizes that is not in_cols, batch * n_segments * k beyond 2^60, a grad_cols or
 * out_cols that does not match, an aggregate that is neither 0 nor 1, a grad entry with both outputs NULL. */
mhte_status mhte_feature_insight(const float* input, const float* weight, int64_t batch, int64_t in_cols, int32_t k,
                                 const int32_t* segment_sizes, int32_t n_segments, int32_t aggregate, float* out,
                                 int64_t out_cols, void* stream);
mhte_status mhte_feature_insight_grad(const float* grad, int64_t grad_cols, const float* input, const float* weight,
                                      int64_t batch, int64_t in_cols, int32_t k, const int32_t* segment_sizes,
                                      int32_t n_segments, float* input_grad, float* weight_grad, void* stream);
mhte_status mhte_feature_insight_plan(int64_t batch, int64_t in_cols, int32_t k, int32_t n_segments, int64_t* out,
                                      int32_t n);
mhte_status mhte_feature_insight_launch_counts(int64_t* out, int32_t n);

/* ---- split by indices (csrc/mhte_split_kernels.h, mhte_split_host.h) -------------------------------------
 * MonolithSplitByIndices, MonolithSplitByIndicesGradient and MonolithRaggedSplitByIndices
 * (RT/ops/split_by_indices_op.cc:28-75, :77-118, :188-243; Python NT/distribution_ops.py:27-78), the shard split
 * of DistributedMultiTypeHashTable (NT/distributed_ps.py:289-291, :497-499).  The ops are stable: inside a split
 * the elements keep their input order (the reference's in-order loops; NT/distribution_ops_test.py:24-33, :67-87).
 *
 * mhte_split_plan (replaces the counting and placing loops, split_by_indices_op.cc:44-48, :66-70, :202-236):
 *   indices [dev i64, n], each in [0, num_splits); num_splits in [1, 1024]; n below 2^31 - 1
 *   pos     [dev i64, n]            the stable permutation, split after split: with off = the exclusive scan of
 *                                   sizes, pos[off[s] .. off[s+1]) are the positions i with indices[i] == s,
 *                                   ascending; the entries behind the last placed element are -1
 *   sizes   [dev i64, num_splits]   the size of every split
 *   n_bad   [dev i64, 1]            the indices outside [0, num_splits): counted here, placed in no split, never
 *                                   the cause of a store outside the outputs
 *   row_splits [host i64, n_row_splits] or NULL with n_row_splits 0: the boundaries of a ragged input (T + 1
 *                                   entries, non-decreasing from 0 to n, else "The input ragged tensor is invalid.")
 *   split_row_splits [dev i64, num_splits * n_row_splits]   entry [s][t]: the elements of split s whose position
 *                                   is < row_splits[t] — the row_splits of split s (:224-230)
 *   host_out [host i64, num_splits + num_splits * n_row_splits + 1] or NULL: sizes | split_row_splits | n_bad,
 *                                   filled after synchronising the stream; with NULL the call waits for nothing
 *   No atomic decides an order: the same input gives the same bits on every run.  One digit pass of the stable
 *   group sort plus one finishing launch (4 launches; n == 0: none, the outputs are cleared).
 * mhte_split_rows (replaces split_by_indices_op.cc:60-70): packed[q, :] = input[pos[q], :] for q < n; rows of
 *   element_size >= 1 elements of elem_bytes 4 (float32) or 8 (int64); split s is the rows
 *   packed[off[s] .. off[s+1]).  An entry of pos outside [0, n) (the -1 tail) moves nothing.
 * mhte_split_rows_grad (replaces split_by_indices_op.cc:107-113): input_grads[pos[q], :] = grads[s][q - off[s], :]
 *   for the placed q; grads is a HOST array of num_splits DEVICE pointers, split s being [sizes[s], element_size];
 *   sizes [dev i64, num_splits] as the plan wrote them.  Rows whose index was out of range are not written.
 * The movers accept any 4-byte-aligned buffer (pos and sizes: 8-byte); 16-byte accesses when a row is whole
 * 16-byte words and every buffer is 16-byte aligned, else 4-byte ones — the same bits either way.  One launch
 * per call, none for n == 0; n * element_size * elem_bytes / 4 must stay below 2^32.
 * mhte_split_launch_counts: the launches of this process by form, n must be 6, index 0 rows / 4-byte form,
 *   1 rows / 16-byte form, 2 gradient / 4-byte form, 3 gradient / 16-byte form, 4 plans that ran the partition,
 *   5 those of them with row_splits.
 * InvalidArgument, checked on the host before any device call: a null pointer for a needed operand, a misaligned
 * pointer, a negative size, num_splits outside [1, 1024], invalid row_splits, an index overflow. */
mhte_status mhte_split_plan(const int64_t* indices, int64_t n, int32_t num_splits, const int64_t* row_splits,
                            int32_t n_row_splits, int64_t* pos, int64_t* sizes, int64_t* split_row_splits,
                            int64_t* n_bad, int64_t* host_out, void* stream);
mhte_status mhte_split_rows(const void* input, int64_t n, int64_t element_size, int32_t elem_bytes,
                            const int64_t* pos, void* packed, void* stream);
mhte_status mhte_split_rows_grad(const void* const* grads, const int64_t* sizes, int32_t num_splits, int64_t n,
                                 int64_t element_size, int32_t elem_bytes, const int64_t* pos, void* input_grads,
                                 void* stream);
mhte_status mhte_split_launch_counts(int64_t* out, int32_t n);

/* ---- the fused-layout packer (csrc/mhte_sharding_plan.h, mhte_sharding_kernels.h, mhte_sharding_host.h) --
 * ShardingSparseFids at op version 2 (NT/data/kernels/parse_sparse_feature.cc:106-155 the index arithmetic,
 * :187-240 FillFidList, :259-424 CreateOffsetTensor; parse_sparse_feature.h:620-990 FeatureParallelParse) for ids
 * that are parsed and on the device: from every feature's ragged ids to the inputs of mhte_embedding_to_layout and
 * the fid lists of the parameter servers, one launch sequence for all features.
 *   features [HOST, n_features] in sorted-name order.  values [dev i64, n_ids], row_splits [dev i64, n_rows + 1];
 *     n_rows is the batch size, 1 for a shared feature (shared != 0), 0 for a feature the batch does not carry;
 *     table_index / feature_in_table_index: the feature's table in sorted-name order and its place among that
 *     table's features (:124-131).  Every (table_index, feature_in_table_index) below table_feature_count occurs once.
 *   table_feature_count [HOST i32, n_tables], every entry >= 1; ps_num in [1, 1024].
 *   With F = n_features, N = the ids of all features, R = their rows, n_pre = F * ps_num (the pre-output indices,
 *   :139-149), n_lists = n_tables * ps_num:
 *   fid_offset [dev u64, N]  in input order: (pre_output_index + shard * table_feature_count +
 *     feature_in_table_index) << 32 | rank with shard = uint64(id) % ps_num (:203, :219 — unsigned).  unique == 0:
 *     rank counts the earlier occurrences of the (feature, shard) (:206); else it is the index of the id's first
 *     occurrence among the distinct ids of the (feature, shard) (:223) — per feature, never across a table.
 *   feature_offset [dev i32, R + 1]  one start per (feature, row), then N (:313-320).
 *   nfl_offset [dev u32, F + 1]  the feature's first row, bit 31 for a shared feature (:307-310); the last entry is
 *     R + 1, the number of entries of feature_offset (:321).  mhte_embedding_to_layout reads it only to see
 *     whether a feature has rows (next - own > 0), as RT/ops/fused_embedding_to_layout.cc does.
 *   fid_list [dev i64, N]  the ids sorted PS-major: shard after shard, inside a shard table after table, inside a
 *     table feature after feature, inside a feature in (first-)occurrence order — for one shard the values of
 *     the ragged tensor its raw lookup takes.  The placed ids (N, or the distinct ones) are key_start[n_pre].
 *   key_start [dev i64, n_pre + 2]  entry shard * F + ft (ft: features numbered table after table) is where that
 *     (feature, shard) starts in fid_list; entry n_pre the placed ids; entry n_pre + 1 the status word (bit 0: a
 *     row_splits that does not run from 0 to n_ids without stepping back).
 *   row_splits_flat [dev i64, n_pre + n_lists]  the reference's fid_list_row_splits, list table_index * ps_num +
 *     shard after list (parse_sparse_feature.h:853-898), table_feature_count + 1 entries each.
 *   list_bounds [dev i64, n_lists * 2]  start and size of list table_index * ps_num + shard inside fid_list.
 *   host_out [HOST i64, n_pre + 2] or NULL: key_start, copied after synchronising the stream — every size in one
 *     read; a set status bit is then "The input ragged tensor is invalid.".  With NULL the call waits for nothing.
 * Ranks come from the stable group sort (ballots) and lower bounds; the unique form finds first occurrences with
 * atomicMin over positions, whose result does not depend on arrival order: the same input gives the same bits on
 * every run.  InvalidArgument, checked on the host before any device call: ps_num outside [1, 1024], a null or
 * misaligned (8 bytes; feature_offset / nfl_offset 4) pointer, an index outside its table, a feature with more
 * than 2^32 - 1 ids (the rank is 32 bits), N of 2^31 - 1 or more. */
typedef struct {
  const int64_t* values;
  const int64_t* row_splits;
  int64_t n_ids;
  int32_t n_rows, shared;
  int32_t table_index, feature_in_table_index;
} mhte_shard_feature;
mhte_status mhte_sharding_sparse_fids(const mhte_shard_feature* features, int32_t n_features,
                                      const int32_t* table_feature_count, int32_t n_tables, int32_t ps_num,
                                      int32_t unique, uint64_t* fid_offset, int32_t* feature_offset,
                                      uint32_t* nfl_offset, int64_t* fid_list, int64_t* key_start,
                                      int64_t* row_splits_flat, int64_t* list_bounds, int64_t* host_out,
                                      void* stream);

/* MonolithFusedReduceAndSplitGPU / MonolithFusedReduceAndSplitGPUGrad (RT/ops/reduce_op.cu.cc:290-379,
 * :392-475 forward; :477-534, :536-... gradient; NT/distribution_ops.py:838-884), the pooling of the
 * feature-column path (NT/feature.py:519-541), and on the same entry points the CPU op
 * MonolithFusedReduceSumAndSplit (+Gradient) (RT/ops/reduce_op.cc:231-321, NT/distribution_ops.py:802-835)
 * for one feature: the ragged sum of every feature's embedding rows per batch row, written straight into
 * the column slices of the features — one launch for all features, one for the gradient.
 *   row_splits         [dev i32] the features' row_splits (bs + 1 each) concatenated
 *   row_split_splits   HOST [n_features + 1]: where each feature's begin (the op's attr);
 *                      bs = row_split_splits[1] - row_split_splits[0] - 1 (reduce_op.cu.cc:417)
 *   embeddings         HOST array of n_features device pointers, matrix i is [emb_rows[i], emb_dims[i]]
 *   slice_dims         HOST, flat, in feature order (the op's attr): the widths the features' columns
 *                      are cut into; a feature's slices add up to its dim
 *   outputs            HOST array of n_slices device pointers, slice s is [bs, slice_dims[s]]
 * out[b, c] = +0 + emb[rs[b], c] + emb[rs[b] + 1, c] + ... added strictly in row order (the reference
 * kernel's `sum = T(0); sum += ...`, :308-316, and the CPU op's accumulation into a zeroed output,
 * reduce_op.cc:253-270): the reference's bits, a row of -0.0 alone gives +0.0, an empty row +0.0; a batch
 * row of any length is one sequential chain.  Ranges are clamped to [0, emb_rows[i]]: a malformed
 * row_splits reads no row outside its matrix.  The gradient is a copy: embeddings_grad[i][r, :] = the
 * feature's slice gradients at the batch row whose range holds r, side by side (:478-499); rows before
 * rs[0] or from rs[bs] on are 0.  No float atomics; nothing is allocated but, beyond 32 lane-column
 * units or 96 slices, the tables of the call (uploaded per call; any number of features and slices).
 * 16-byte accesses where a feature's dim, its slices' starts and widths are multiples of 4 floats and
 * its pointers 16-byte aligned, else 4-byte ones (same bits).
 * InvalidArgument, checked on the host before any device call: a null argument, n_features <= 0, a
 * non-positive dim, a feature whose number of row splits differs from bs + 1, sum(slice_dims) !=
 * sum(emb_dims), a slice that straddles two features (the reference checks none of the last three). */
mhte_status mhte_fused_reduce_and_split(const int32_t* row_splits, const int32_t* row_split_splits,
                                        const float* const* embeddings, const int64_t* emb_rows,
                                        const int32_t* emb_dims, int32_t n_features,
                                        const int32_t* slice_dims, int32_t n_slices, float* const* outputs,
                                        void* stream);
mhte_status mhte_fused_reduce_and_split_grad(const int32_t* row_splits, const int32_t* row_split_splits,
                                             const int64_t* emb_rows, const int32_t* emb_dims,
                                             int32_t n_features, const int32_t* slice_dims, int32_t n_slices,
                                             const float* const* slice_grads, float* const* embeddings_grad,
                                             void* stream);

/* MonolithEmbeddingToLayout / MonolithEmbeddingToLayoutGrad (RT/ops/fused_embedding_to_layout.cc
 * :1037-1066; CUDA kernels RT/ops/fused_embedding_to_layout.cu.cc:96-199,337-...; GatherEmb /
 * ScatterGrad RT/ops/fused_embedding_to_layout.h:204-346): pools the looked-up embeddings of every
 * feature into the dense model's input tensors, and scatters the tensors' gradients back.
 *   embeddings[M]      HOST array of M device pointers: matrix m is [rows_m, emb_row_floats[m]],
 *                      emb_len[m] floats in all (the op's embeddings_list, one per shard x sub-table)
 *   fid_offset         [dev u64, n_fid] (matrix index << 32 | row) of every fid occurrence (:50-54)
 *   feature_offset     [dev i32, n_feature] first fid of every feature instance
 *   nfl_offset         [dev u32, n_nfl] first feature instance of every named feature list; bit 31:
 *                      the feature is shared by all rows of the batch (:56-60)
 *   slices             HOST: the slices of all layouts, layouts in sorted-name order (the op sorts
 *                      them, fused_embedding_to_layout.cc:283), slices in configuration order —
 *                      SliceConfig / OutConfig / FeatureConfig of idl/matrix/proto/example.proto
 *                      :176-221 flattened: feature_idx = the feature's index among the sorted feature
 *                      names (:273-279); pooling 0 SUM, 1 MEAN, 3 FIRSTN (max_sequence_length rows);
 *                      out_type 0 CONCAT, 1 STACK, 2 ADDN, 3 NONE; out_index / out_offset /
 *                      out_row_floats place the slice in its output tensor [batch, out_row_floats]
 *   outputs            HOST array of device pointers, zero-filled first (rows without fids stay 0)
 * SUM / MEAN walk a feature's fids in order (the reference's loop: bit-identical sums); the slices
 * of an ADDN layout are added in configuration order (the reference's CPU order; its CUDA path uses
 * float atomics).  The gradient op zero-fills embeddings_grad and adds, per embedding row, in the
 * order the reference's CPU kernel does (slices in configuration order, batch rows ascending, fids
 * in list order): its sequential fp32 sums bit for bit, no float atomics; a row with more than 1 024
 * contributions to one slice sums 64 contiguous ranges of that sequence and adds the range sums in
 * order (same bits on every run; fp32 re-association against the sequential sum).
 * MHTE_POOL_ATOMICS=1 in the environment selects the reference's CUDA form (float atomics, arrival
 * order).  Any number of matrices and outputs (beyond 64 / 32 their pointers are uploaded per call).
 * flags: MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS — the caller states that every feature instance has exactly
 * one fid and no embedding row is referenced twice (the per-occurrence rows of a lookup feeding a
 * one-id-per-feature model): slices on float4 boundaries then move as float4 copies and the gradient
 * is a plain store instead of a float atomic per element.  The host checks what it can see: widths,
 * strides and pointers that are not float4-aligned take the general kernels, and a gradient call in
 * which two slices of the same feature_idx overlap in [start, start + dim) — the same columns of one
 * feature fed to two layouts — is a sum of two addends per element, so it takes the form it would
 * take without the flag (grouped sums, or float atomics under MHTE_POOL_ATOMICS=1); the forward is
 * unaffected.  What lives on the device stays the caller's promise: one fid per instance, distinct
 * rows, and no shared feature list (nfl_offset bit 31) whose row receives a gradient from more than
 * one batch row. */
enum { MHTE_LAYOUT_ONE_FID_UNIQUE_ROWS = 1 };
typedef struct {
  int32_t feature_idx, start, dim;
  int32_t pooling, max_sequence_length;
  int32_t out_type, out_index, out_offset, out_row_floats;
} mhte_layout_slice;
mhte_status mhte_embedding_to_layout(const float* const* embeddings, const int32_t* emb_row_floats,
                                     const int64_t* emb_len, int32_t n_emb, const uint64_t* fid_offset,
                                     int64_t n_fid, const int32_t* feature_offset, int64_t n_feature,
                                     const uint32_t* nfl_offset, int32_t n_nfl, int32_t batch_size,
                                     const mhte_layout_slice* slices, int32_t n_slices,
                                     float* const* outputs, const int64_t* output_len, int32_t n_outputs,
                                     int32_t flags, void* stream);
mhte_status mhte_embedding_to_layout_grad(float* const* embeddings_grad, const int32_t* emb_row_floats,
                                          const int64_t* emb_len, int32_t n_emb, const uint64_t* fid_offset,
                                          int64_t n_fid, const int32_t* feature_offset, int64_t n_feature,
                                          const uint32_t* nfl_offset, int32_t n_nfl, int32_t batch_size,
                                          const mhte_layout_slice* slices, int32_t n_slices,
                                          const float* const* tensors_grad, const int64_t* tensor_len,
                                          int32_t n_tensors, int32_t flags, void* stream);

/* Admission filter: the reference's SlidingHashFilter (RT/hash_filter/sliding_hash_filter.{h,cc};
 * created by HashFilterOp, RT/ops/hash_filter_op.cc:47-81; the `filter_handle` input of
 * CreateMonolithMultiHashTable, RT/ops/multi_hash_table_op.cc:104-112), in HBM, shared by the tables of
 * a MultiHashTable: max(split_num, 5) counting filters (4-bit saturating counts, HashFilter,
 * RT/hash_filter/hash_filter.h:33-214) of capacity / (split_num - 1) elements each as a sliding window —
 * counts are taken forward in the head split, an id's older count is looked up backward, the window
 * moves on when the head split is full.  While attached, Optimize / Assign (and the training step's
 * apply) drop an id that is not in the table yet and has been seen fewer times than its feature slot's
 * occurrence threshold (RT/ops/embedding_hash_table_tf_bridge.cc:182-185,300-321); AssignAdd consults
 * the filter without the Contains guard, as the reference's multi-table path does (:230-232).  The
 * window moves between launches, not inside one.
 * mhte_hash_filter_save / _restore: MonolithHashFilterSave / Restore (RT/ops/hash_filter_save_op.cc,
 * hash_filter_restore_op.cc): one TFRecord file per split, <basename>-%05d-of-%05d, a
 * HashFilterSplitMetaDump then HashFilterSplitDataDump records (embedding_hash_table.proto:112-137);
 * restore checks the geometry like SlidingHashFilter::RestoreMetaDump.  (Slot positions depend on the
 * hash function — the reference's absl::Hash is unpinned — so files are interchangeable between
 * instances of this engine, not with the reference.)  Both synchronise. */
mhte_status mhte_hash_filter_create(uint64_t capacity, int32_t split_num, int32_t device,
                                    mhte_hash_filter** out);
/* the same with the filter op's `config` attr: a serialized SlotOccurrenceThresholdConfig
 * (embedding_hash_table.proto:100-110).  Tables created from a proto with this filter attached take
 * their occurrence thresholds from it. */
mhte_status mhte_hash_filter_create_from_proto(uint64_t capacity, int32_t split_num,
                                               const void* config, int64_t config_len,
                                               int32_t device, mhte_hash_filter** out);
/* MonolithProbabilisticFilter (RT/ops/hash_filter_op.cc:81-110, RT/hash_filter/probabilistic_filter.cc):
 * no counts are kept — an id the table does not hold is admitted with probability count / threshold
 * per consultation (equal_probability != 0: 1 - (1 - p)^count, p = 1 - 0.05^(1/threshold)); an id the
 * table holds is never filtered.  The reference draws from a time-seeded thread-local xorshift, so
 * parity is the admission rate; here a counter-based generator keyed by (seed, id, update launch,
 * occurrence) — seed 0: taken from the clock.  config: serialized SlotOccurrenceThresholdConfig
 * (may be NULL).  get returns 15, save / restore are no-ops (split_num() == 0), as in the reference. */
mhte_status mhte_hash_filter_create_probabilistic(int32_t equal_probability, uint64_t seed,
                                                  const void* config, int64_t config_len,
                                                  int32_t device, mhte_hash_filter** out);
void mhte_hash_filter_destroy(mhte_hash_filter* f);
mhte_status mhte_multi_table_set_filter(mhte_multi_table* t, mhte_hash_filter* f /* NULL detaches */);
/* Filter::estimated_total_element / failure_count / split_num (RT/hash_filter/filter.h:31-36):
 * out[0] = head, [1] = head_increment, [2] = failure_count (adds that found no usable slot),
 * [3] = number of splits S, [4 .. 4+S) = elements per split; cap >= 4 + S.  Synchronises. */
mhte_status mhte_hash_filter_stats(mhte_hash_filter* f, int64_t* out, int32_t cap, void* stream);
mhte_status mhte_hash_filter_save(mhte_hash_filter* f, const char* basename, void* stream);
mhte_status mhte_hash_filter_restore(mhte_hash_filter* f, const char* basename, void* stream);
/* Filter::get: the seen count of ids (0..15), out [dev u32, n] */
mhte_status mhte_hash_filter_get(mhte_hash_filter* f, const int64_t* id, int64_t n, uint32_t* out,
                                 void* stream);

/* MonolithMultiHashTableSave / Restore (RT/ops/multi_hash_table_save_restore_ops.cc:115-263,
 * 266-420) in the reference's on-disk format, so checkpoints are interchangeable:
 *   <basename>-%05d-of-%05d       TFRecord + SNAPPY stream of EntryDump (embedding_hash_table.proto
 *                                 :45-50: id, num, opt {one SingleOptimizerDump per segment},
 *                                 last_update_ts_sec), tables in sorted-name order, each shard a
 *                                 contiguous bucket range (cuckoohash_map.hpp:740-773)
 *   <basename>.meta-%05d-of-%05d  TFRecord stream of MultiHashTableMetadata {table_name, num_entries}
 * Save drops rows expired relative to the table's max_update_ts (:203-211; per-slot TTLs of the
 * table config).  nshards < 0: min(4, max(1, total_size / 1e6)) (:240-248).
 * Restore upserts every entry of every table it knows (whole row + the entry's own timestamp),
 * skips tables it does not know, reports a short or corrupted shard as an error.  Both synchronise
 * the stream; host-side work is proportional to the table. */
mhte_status mhte_multi_table_save(mhte_multi_table* t, const char* basename, int32_t nshards,
                                  void* stream);
mhte_status mhte_multi_table_restore(mhte_multi_table* t, const char* basename, void* stream);

/* MonolithHashTableSave / MonolithHashTableRestore for ONE table (RT/ops/hash_table_save_op.cc:72-200,
 * RT/ops/hash_table_restore_op.cc:63-160): the single-table layout the reference's exported models
 * carry (model_export/testdata/saved_model/ps_N/.../assets/MonolithHashTable_*):
 *   <basename>-%05d-of-%05d   UNCOMPRESSED TFRecord stream of EntryDump, one file per shard, no .meta
 * Save: nshards < 0 = min(4, max(1, size / 1e6)); each shard a contiguous bucket range, expired
 * rows left out, written under a temporary name and renamed.  Restore validates the shard set
 * (RT/ops/file_utils.cc:34-78), CLEARS the table (restore_op.cc:88), then upserts every record of
 * every shard (whole row + the entry's own timestamp; an entry without last_update_ts_sec gets 0).
 * mhte_table_clear: EmbeddingHashTableInterface::Clear (cuckoo_embedding_hash_table.cc:322-326).
 * All three synchronise the stream. */
mhte_status mhte_table_save(mhte_multi_table* t, int32_t table, const char* basename, int32_t nshards,
                            void* stream);
mhte_status mhte_table_restore(mhte_multi_table* t, int32_t table, const char* basename, void* stream);
mhte_status mhte_table_clear(mhte_multi_table* t, int32_t table, void* stream);

/* ---- caller-side dedup / packing ops on the device ------------------------------------------ */
typedef struct mhte_dedup_ws mhte_dedup_ws;
mhte_status mhte_dedup_ws_create(int32_t device, mhte_dedup_ws** out);
void mhte_dedup_ws_destroy(mhte_dedup_ws* ws);

/* Device form of the per-table dedup inside MonolithUniqueKeyWithValueAndOffset
 * (RT/ops/unique_mapping_ops.cc:82-114) and FusedReorderByIndices (RT/ops/fused_reorder_by_indices.cc
 * :52-60): unique ids in FIRST-OCCURRENCE order, the unique index of every position, and each
 * unique id's occurrence positions in occurrence order (CSR).
 *   ids [dev,n] -> unique_ids [dev, cap n], inverse [dev u32, n], seg_off [dev u32, n+1],
 *   seg_pos [dev u32, n], n_unique_dev [dev u32, 1].
 * n_unique_host (optional, host): filled after synchronising the stream. */
mhte_status mhte_unique(mhte_dedup_ws* ws, const int64_t* ids, int64_t n, int64_t* unique_ids,
                        uint32_t* inverse, uint32_t* seg_off, uint32_t* seg_pos,
                        uint32_t* n_unique_dev, int64_t* n_unique_host, void* stream);
/* Dedup for the fused training step: same key set and occurrence lists as mhte_unique, but the
 * numbering of the unique ids is unspecified (it follows atomic arrival order, like the iteration
 * order of the absl::flat_hash_map the reference dedups with, RT/ops/unique_mapping_ops.cc:82-114
 * keeps insertion order only because it also stores a vector).  Saves the two scan launches that
 * first-occurrence numbering needs.  list_start / list_end [dev u32, n]: positions of unique id u
 * are seg_pos[list_start[u] .. list_end[u]); lists longer than 32 positions are in ascending
 * position order, shorter ones in any order (mhte_table_sum_optimize_n orders them itself). */
mhte_status mhte_unique_unordered(mhte_dedup_ws* ws, const int64_t* ids, int64_t n,
                                  int64_t* unique_ids, uint32_t* inverse, uint32_t* list_start,
                                  uint32_t* list_end, uint32_t* seg_pos, uint32_t* n_unique_dev,
                                  int64_t* n_unique_host, void* stream);
/* FillWithOffsetMap in gather form (RT/ops/unique_mapping_ops.cc:225-242):
 * out[p,:] = src[index[p],:] for p < n. */
mhte_status mhte_gather_rows(const float* src, const uint32_t* index, int64_t n, int32_t dim,
                             float* out, void* stream);
/* FillWithOffsetMapGradient (RT/ops/unique_mapping_ops.cc:307-324): out[u,:] = sum over the
 * occurrence list of u of grads[p,:].  exact_order != 0: strictly sequential sum (bit-exact with
 * the reference); 0: windowed deterministic sum (fp32 re-association only). */
mhte_status mhte_segment_sum(mhte_dedup_ws* ws, const float* grads, const uint32_t* inverse,
                             const uint32_t* seg_off, const uint32_t* seg_pos,
                             const uint32_t* n_unique_dev, int64_t n, int32_t dim, float* out,
                             int32_t exact_order, void* stream);
/* Lookup / optimize of ONE table taking the id count from device memory (n_dev may be NULL):
 * lets dedup -> lookup -> ... -> optimize run without a host round trip. */
mhte_status mhte_table_lookup_n(mhte_multi_table* t, int32_t table, const int64_t* id,
                                int64_t n_max, const uint32_t* n_dev, float* embedding,
                                void* stream);
mhte_status mhte_table_optimize_n(mhte_multi_table* t, int32_t table, const int64_t* id,
                                  int64_t n_max, const uint32_t* n_dev, const float* value,
                                  const float* learning_rate, int64_t n_learning_rate,
                                  int64_t update_time, int64_t global_step, int32_t flags,
                                  void* stream);

/* Fused backward of one table: MonolithFillWithOffsetMapGradient (RT/ops/unique_mapping_ops.cc
 * :284-329) followed by MonolithMultiHashTableOptimize (RT/ops/multi_hash_table_update_op.cc:47-100)
 * on the unique ids, as ONE launch: out-of-order duplicates are summed per unique id and the
 * optimizer is applied once per id, without materialising the summed gradients.
 *   ws              the workspace whose most recent mhte_unique / mhte_unique_unordered produced
 *                   unique_ids / inverse / lists for this batch of n ids
 *                   (MHTE_FAILED_PRECONDITION otherwise)
 *   list_start/end  per unique id, its positions are seg_pos[list_start[u] .. list_end[u]);
 *                   after mhte_unique pass (seg_off, seg_off + 1)
 *   grads           [dev, n, dim] gradient of every occurrence
 *   grad_unique     [dev, n_max, dim] scratch (summed gradients of ids that take the displacement
 *                   slow path; all unique ids when the row is too wide for the fused kernel)
 *   flags           MHTE_EXACT_ORDER: every list is summed strictly in occurrence order (bit-exact
 *                   with the reference); otherwise lists of > 32 occurrences are summed in
 *                   256-entry chunks in a fixed association (deterministic; fp32 re-association
 *                   only).  MHTE_DEFER_SLOWPATH: do not launch the displacement pass for ids whose
 *                   two buckets are full; see mhte_table_finish_pending.
 * Alignment: grads and grad_unique need 4-byte alignment only.  The one-launch form moves a row as
 * float4s when both are 16-byte aligned and one float per lane otherwise, which covers rows of up to
 * 64 floats; a wider row in a buffer that is not 16-byte aligned takes the route of the rows too wide
 * for the fused kernel (segment sum + update of the unique ids: the lists must then be the CSR lists of
 * mhte_unique, MHTE_INVALID_ARGUMENT otherwise).  Same result either way. */
enum { MHTE_EXACT_ORDER = 1, MHTE_DEFER_SLOWPATH = 2 };
mhte_status mhte_table_sum_optimize_n(mhte_multi_table* t, int32_t table, mhte_dedup_ws* ws,
                                      const int64_t* unique_ids, int64_t n_max,
                                      const uint32_t* n_unique_dev, const float* grads,
                                      const uint32_t* inverse, const uint32_t* list_start,
                                      const uint32_t* list_end, const uint32_t* seg_pos, int64_t n,
                                      float* grad_unique, const float* learning_rate,
                                      int64_t n_learning_rate, int64_t update_time,
                                      int64_t global_step, int32_t flags, void* stream);
/* Displacement (BFS) pass for the ids a MHTE_DEFER_SLOWPATH call left queued.  Every other entry
 * point on the table runs it first if it is still outstanding, so calling it is optional; callers
 * that time kernels, or that update several tables back to back, call it once at the end. */
mhte_status mhte_table_finish_pending(mhte_multi_table* t, int32_t table, void* stream);

/* Pipelined training step of one table: TWO launches per step, the dedup of the NEXT batch (it
 * depends on the ids only — the reference prefetches it too, NT/distributed_ps_sync.py:199-203)
 * riding in them, different workgroups doing the jobs side by side on one queue:
 *   mhte_table_step_forward   lookup of id[n] -> embedding (as mhte_table_lookup_n)
 *                             + dedup of id_next[n_next] into ws_next (one phase: per-workgroup
 *                               occurrence runs, see csrc/mhte_step_kernels.h)
 *                             + the displacement pass of the previous update (one wavefront; the
 *                               lookup workgroups wait for it only when it has work)
 *   mhte_table_step_backward  duplicate-gradient sum + upsert + optimizer of the batch held by ws
 *                             (MonolithFillWithOffsetMapGradient + MonolithMultiHashTableOptimize,
 *                             RT/ops/unique_mapping_ops.cc:284-329, multi_hash_table_update_op.cc
 *                             :47-100) + the heavy-list work items of the batch held by ws_next
 * Batches of 1..65 536 ids.  The dedup's device-side results are the unique ids (unspecified
 * order, like the iteration order of the flat_hash_map the reference dedups with) and their count;
 * the occurrence lists stay in the workspace in the step's own run format.
 *   ws / ws_next   two workspaces used alternately; ws_next may be NULL (no following batch)
 *   ws_cur         (step_forward, optional) the workspace that holds THIS batch's run dedup: the
 *                  launch then also reserves, with one counter bump per workgroup, the row handles
 *                  of the ids its update will have to insert (the update's own reservations all
 *                  hit one counter word and pace that launch); NULL: the update reserves itself
 *   flags          MHTE_EXACT_ORDER: every list is summed strictly in occurrence order (bit-exact
 *                  with the reference); otherwise lists of > 32 occurrences are summed as a fixed
 *                  tree over position ranges (deterministic; fp32 re-association only)
 * The first batch of a pipeline is deduplicated by mhte_step_dedup.  The displacement pass left
 * by step_backward is run by the next step_forward, or by any other call on the table
 * (mhte_table_finish_pending).  The table row must satisfy mhte_table_fused_backward_ok.
 * Alignment: embedding (step_forward), grads and grad_unique (step_backward) of a table whose row has
 * more than 64 floats must be 16-byte aligned: these launches give a row one lane group and move it as
 * float4s only.  Anything else is MHTE_INVALID_ARGUMENT, raised before the call changes anything (the
 * next batch's dedup is not begun, the queued displacement pass and the workspaces stay as they were:
 * the call can be repeated with aligned buffers).  Rows of up to 64 floats take any 4-byte aligned
 * buffer (one float per lane). */
mhte_status mhte_step_dedup(mhte_dedup_ws* ws, const int64_t* id, int64_t n, int64_t* unique_ids,
                            uint32_t* n_unique_dev, void* stream);
/* Sender side of the id-sharded step (NT/distributed_ps_sync.py:95-490), on the batch held by ws
 * (mhte_step_dedup):
 *   mhte_shard_partition  FusedReorderByIndices' shard-major packing (RT/ops/fused_reorder_by_indices.cc
 *                         :75-123; shard = floormod(id, num_shards), NT/distributed_ps.py:289) of ids
 *                         that are already unique: send_ids [dev, n_max] shard-major, send_pos
 *                         [dev u32, n_max] position of ids[u] in it, counts [dev u32, num_shards].
 *                         The id count comes from device memory (n_dev).  num_shards <= 64.
 *   mhte_step_scatter     out[p, :] = rows[idx(u), :] for every occurrence p of unique index u
 *                         (MonolithFillWithOffsetMap, RT/ops/unique_mapping_ops.cc:204-268)
 *   mhte_step_sum         out[idx(u), :] = sum over the occurrences p of u of grads[p, :], in
 *                         occurrence order for lists of <= 32, a fixed tree otherwise
 *                         (MonolithFillWithOffsetMapGradient, :284-329)
 * idx(u) = index ? index[u] : u (pass send_pos: rows arrive / gradients leave in send order).
 * dim <= 256. */
mhte_status mhte_shard_partition(mhte_dedup_ws* ws, const int64_t* ids, int64_t n_max,
                                 const uint32_t* n_dev, int32_t num_shards, int64_t* send_ids,
                                 uint32_t* send_pos, uint32_t* counts, void* stream);
mhte_status mhte_step_scatter(mhte_dedup_ws* ws, const float* rows, const uint32_t* index,
                              int32_t dim, float* out, void* stream);
mhte_status mhte_step_sum(mhte_dedup_ws* ws, const float* grads, const uint32_t* index, int32_t dim,
                          float* out, void* stream);
mhte_status mhte_table_step_forward(mhte_multi_table* t, int32_t table, const int64_t* id,
                                    int64_t n, float* embedding, mhte_dedup_ws* ws_next,
                                    const int64_t* id_next, int64_t n_next,
                                    int64_t* unique_ids_next, uint32_t* n_unique_dev_next,
                                    mhte_dedup_ws* ws_cur, void* stream);
mhte_status mhte_table_step_backward(mhte_multi_table* t, int32_t table, mhte_dedup_ws* ws,
                                     mhte_dedup_ws* ws_next, const int64_t* unique_ids,
                                     int64_t n_max, const uint32_t* n_unique_dev,
                                     const float* grads, int64_t n, float* grad_unique,
                                     const float* learning_rate, int64_t n_learning_rate,
                                     int64_t update_time, int64_t global_step, int32_t flags,
                                     void* stream);
/* ... with TWO batches of look-ahead: the run dedup of the batch after the next (id_ahead, into
 * ws_ahead, a third workspace) rides in this launch beside the update and the next batch's numbering.
 * The forward launch of a step whose batch was deduplicated this way carries the lookups alone
 * (mhte_table_step_forward with ws_next NULL): ~4 us less per step at 65 536 ids.  The reference's
 * pipeline prefetches the same way, one stage queue per step of look-ahead
 * (NT/distributed_ps_sync.py:199-203,270-275).  ws_ahead NULL: exactly mhte_table_step_backward.
 * The alignment rule of mhte_table_step_backward holds: a refused call has not begun the dedup of
 * id_ahead either. */
mhte_status mhte_table_step_backward_ahead(mhte_multi_table* t, int32_t table, mhte_dedup_ws* ws,
                                           mhte_dedup_ws* ws_next, const int64_t* unique_ids,
                                           int64_t n_max, const uint32_t* n_unique_dev,
                                           const float* grads, int64_t n, float* grad_unique,
                                           const float* learning_rate, int64_t n_learning_rate,
                                           int64_t update_time, int64_t global_step, int32_t flags,
                                           mhte_dedup_ws* ws_ahead, const int64_t* id_ahead,
                                           int64_t n_ahead, int64_t* unique_ids_ahead,
                                           uint32_t* n_unique_dev_ahead, void* stream);

/* Pipelined training step over ALL tables of a MultiHashTable: what a MonolithModel does per step
 * with MonolithMultiHashTableLookup (RT/ops/multi_hash_table_lookup_op.cc:33-89) and
 * MonolithMultiHashTableOptimize (RT/ops/multi_hash_table_update_op.cc:47-100) on the ragged
 * (id, id_split) batch of its T feature tables (NT/multi_hash_table_ops.py:349-413,
 * NT/multi_type_hash_table.py:253-303), as ONE forward and ONE backward launch for every table
 * together (+ a displacement launch that usually finds nothing to do) instead of 2 T launches:
 *   mhte_multi_step_forward   embedding[sum n_t*dim_t] = rows of id (layout of mhte_lookup: tables in
 *                             sorted-name order, per OCCURRENCE, absent ids -> zeros, no insert)
 *                             + the run dedup of the NEXT batch (id_next, id_split_next; NULL: none)
 *   mhte_multi_step_backward  value[sum n_t*dim_t] = gradient of every occurrence of the forward
 *                             batch: per table duplicate-gradient sum in occurrence order
 *                             (MonolithFillWithOffsetMapGradient, RT/ops/unique_mapping_ops.cc:284-329)
 *                             + upsert + one optimizer step per distinct id, + the numbering of the
 *                             next batch's distinct ids
 * prefetched != 0: the caller states that (id, id_split) is the batch the previous forward call
 * received as id_next (its dedup is picked up; MHTE_FAILED_PRECONDITION if there is none of that
 * shape); 0: the batch is deduplicated now (two more launches), any batch deduplicated ahead is
 * dropped.  Up to max_batch_per_table (<= 65 536) ids per table and step; empty tables are fine.
 * Every table must satisfy mhte_table_fused_backward_ok with segment boundaries on 4-float
 * multiples; embedding / value 16-byte aligned.  flags: MHTE_EXACT_ORDER as in
 * mhte_table_step_backward.  learning_rate [host, sum slice_size_t] as in mhte_optimize.
 * mhte_multi_step_unique_counts: distinct ids per table of the forward batch (host int64[T]);
 * synchronises. */
typedef struct mhte_multi_step mhte_multi_step;
mhte_status mhte_multi_step_create(mhte_multi_table* t, int64_t max_batch_per_table,
                                   mhte_multi_step** out);
void mhte_multi_step_destroy(mhte_multi_step* s);
mhte_status mhte_multi_step_forward(mhte_multi_step* s, const int64_t* id, const int64_t* id_split,
                                    int64_t n_split, float* embedding, int64_t embedding_len,
                                    const int64_t* id_next, const int64_t* id_split_next,
                                    int64_t n_split_next, int32_t prefetched, void* stream);
mhte_status mhte_multi_step_backward(mhte_multi_step* s, const float* value, int64_t value_len,
                                     const float* learning_rate, int64_t n_learning_rate,
                                     int64_t update_time, int64_t global_step, int32_t flags,
                                     void* stream);
mhte_status mhte_multi_step_unique_counts(mhte_multi_step* s, int64_t* counts, void* stream);

/* Id-sharded training step over ALL tables, one process per GPU: the reference's sync-training
 * exchange (NT/distributed_ps_sync.py:95-287 lookup, :289-490 apply_gradients; shard =
 * floormod(id, world), NT/distributed_ps.py:289; packing RT/ops/fused_reorder_by_indices.cc:75-123)
 * driven from C++ (RCCL send / recv groups, or direct peer stores) on the caller's stream.  Rank r's mhte_multi_table
 * holds the ids it owns of every table.  Per step a rank deduplicates its ragged batch, packs the
 * distinct ids into one block per peer that carries its own per-table counts (no size exchange),
 * and the ranks trade: id blocks -> owners look the rows up
 * (no insert) -> row blocks back -> scatter to the occurrences; gradients: per-id sums in
 * occurrence order -> row-shaped blocks to the owners -> every owner applies the peers' blocks one
 * after the other in rank order (the reference's default of one optimizer application per
 * sender).  Three exchanges per step, all tables in each.  Any number of tables (tables x world <=
 * 65535): the kernels of a stage take 32 tables per launch, the exchanges carry all of them.
 *   ids_per_peer_table  id slots per (peer, table) block; 0 (default) = max_batch: a block can hold
 *                       the whole batch, so no step can overflow one and no id is ever dropped —
 *                       the reference's all-to-all is variable-sized.  A smaller value is an explicit
 *                       choice of fixed-size blocks that cross the links whole: a step in which one
 *                       table sends more distinct ids than that to one peer hands those ids zero
 *                       rows, drops their gradients and makes the next call (or
 *                       mhte_shard_step_check, which must then be called before the step's results
 *                       are used) return MHTE_RESOURCE_EXHAUSTED.
 *   unique_id           128 bytes from mhte_shard_unique_id on one rank, distributed by the
 *                       launcher: the step creates its RCCL communicator (collective: every rank
 *                       calls create).  NULL with world == 1: no communicator, the exchange is the
 *                       identity.  NULL with world > 1: the ranks live in this process on one device
 *                       and are driven together through mhte_shard_group_* (device copies stand in
 *                       for the links; tests).
 * RCCL transport: with the default capacity the row / gradient exchanges move only the occupied
 * part of every (peer, table) segment; the counts are the id blocks' headers, copied to pinned host
 * memory behind the id exchange (a step ahead of their use for a batch that was prepared ahead).
 * With an explicit ids_per_peer_table: whole fixed-size blocks, nothing known to the host.
 * MHTE_SHARD_EXACT=0 / 1 in the environment at creation overrides the choice.
 *
 * Peer-store transport (mhte_shard_step_create_ipc): every rank maps every other rank's receive
 * WINDOW (hipIpcGetMemHandle / hipIpcOpenMemHandle — across xGMI between devices, or between
 * processes sharing one device) and an exchange is one copy kernel per rank that stores the
 * occupied part of every (peer, table) segment straight into the peers' windows, sized ON THE
 * DEVICE from the id blocks' headers: exact-size exchanges with no count on the host, no size
 * exchange and no staging copy.  Flow control is two words per (channel, peer) in the windows
 * (ready-to-receive credit, block-arrived sequence number); a consumer launch is preceded by a
 * one-wavefront wait for exactly the peers it needs, so an owner applies a peer's gradient block as
 * soon as that block has landed.  Waits are bounded (MHTE_SHARD_TIMEOUT_MS, default 30 000): a peer
 * that never arrives makes mhte_shard_step_check / the next call return MHTE_UNAVAILABLE instead of
 * hanging the queue.  Creation is three calls: create_ipc (allocates the window), ipc_handle (128
 * bytes for the launcher to gather from every rank), ipc_connect (all ranks' handles, rank-major);
 * ipc_selftest moves a data pattern through every pair of windows, three rounds over the same
 * addresses, checked on the receiving side (collective, synchronises; MHTE_UNAVAILABLE: use RCCL).
 * forward / backward arguments are those of mhte_multi_step_* for this rank's batch; `prefetched`
 * and the next batch must agree across the ranks (the calls are collective).  A table with an
 * occurrence filter is filtered on its OWNER: every id of a sender's block that the owner does not
 * hold asks the owner's filter with count 1 (ids of a block are distinct), as the reference's fused
 * optimize does per (sender, id); the filter's window moves between senders.  Tables with the
 * whole-segment optimizer (GroupAdaGrad) are accepted: the sender side does not look at the
 * optimizer, the owner applies such a table's blocks with an instance of its own.  global_step
 * reaches the optimizers. */
typedef struct mhte_shard_step mhte_shard_step;
mhte_status mhte_shard_unique_id(void* out128);
mhte_status mhte_shard_step_create(mhte_multi_table* t, int64_t max_batch_per_table, int32_t rank,
                                   int32_t world, int64_t ids_per_peer_table, const void* unique_id,
                                   mhte_shard_step** out);
void mhte_shard_step_destroy(mhte_shard_step* s);
mhte_status mhte_shard_step_create_ipc(mhte_multi_table* t, int64_t max_batch_per_table, int32_t rank,
                                       int32_t world, int64_t ids_per_peer_table,
                                       mhte_shard_step** out);
mhte_status mhte_shard_step_ipc_handle(mhte_shard_step* s, void* out128);
mhte_status mhte_shard_step_ipc_connect(mhte_shard_step* s, const void* handles, int32_t n_handles);
mhte_status mhte_shard_step_ipc_selftest(mhte_shard_step* s, void* stream);
mhte_status mhte_shard_step_forward(mhte_shard_step* s, const int64_t* id, const int64_t* id_split,
                                    int64_t n_split, float* embedding, int64_t embedding_len,
                                    const int64_t* id_next, const int64_t* id_split_next,
                                    int64_t n_split_next, int32_t prefetched, void* stream);
mhte_status mhte_shard_step_backward(mhte_shard_step* s, const float* value, int64_t value_len,
                                     const float* learning_rate, int64_t n_learning_rate,
                                     int64_t update_time, int64_t global_step, void* stream);
/* mode 1 (or MHTE_SHARD_OVERLAP=1 at creation): what the NEXT batch needs and the tables do not — its
 * run dedup, the numbering + owner packing of its distinct ids, the id exchange (peer-store
 * transport) — is enqueued by mhte_shard_step_forward on a stream of the step's own and runs beside
 * whatever the caller enqueues between forward and backward (layout -> dense model -> layout
 * gradient); backward then carries the gradient sums only.  Results are the same as mode 0 (nothing
 * stale is read: the reference pipelines the same stages with its prefetch queues,
 * NT/distributed_ps_sync.py:199-203,270-275).  The caller's next-batch ids must stay valid until the
 * following forward call. */
mhte_status mhte_shard_step_set_overlap(mhte_shard_step* s, int32_t mode);
/* bits 16 (or MHTE_SHARD_GRAD_FP16=1 at creation): the gradient exchange carries fp16 — the sender
 * rounds its per-id sums to nearest even, the owner widens them before its update — half the link
 * bytes of exchange 3.  A numerics change the reference offers as an option (`grad_flat` cast to
 * tf.float16 around the gradient all-to-all, NT/distributed_ps_sync.py:47,334-337); every rank of the
 * world must make the same choice, before its first backward.  bits 32: fp32 (default). */
mhte_status mhte_shard_step_set_grad_bits(mhte_shard_step* s, int32_t bits);
/* on != 0: this rank's per-id gradient sums are the reference's SEQUENTIAL sums for every duplicate list
 * (MonolithFillWithOffsetMapGradient adds an id's gradients in occurrence order,
 * RT/ops/unique_mapping_ops.cc:284-329) — lists of up to 32 occurrences are summed that way in any mode; with
 * this the heavy ones are too (one more launch in front of the sums: a workgroup streams a list's rows through LDS,
 * one wavefront adds them in order), instead of a fixed tree within 1e-6 of it.  Every owner's rows are then the
 * reference's bit for bit (its senders applied in rank order, distributed_ps_sync.py:357-479).  A per-rank
 * choice; takes effect at the next backward. */
mhte_status mhte_shard_step_set_exact_order(mhte_shard_step* s, int32_t on);
/* waits for the stream, then reports a block overflow of the steps enqueued so far */
mhte_status mhte_shard_step_check(mhte_shard_step* s, void* stream);
/* distinct ids per table of this rank's forward batch (host int64[T]); synchronises */
mhte_status mhte_shard_step_unique_counts(mhte_shard_step* s, int64_t* counts, void* stream);
/* info[0] = id slots per (peer, table), [1] = bytes of one id block, [2] = bytes of one row block,
 * [3] = transport: 0 identity, 1 RCCL, 2 in-process group, 3 peer stores into fine-grained windows,
 * 4 peer stores into plain device memory (MHTE_SHARD_WINDOW=coarse) */
mhte_status mhte_shard_step_info(mhte_shard_step* s, int64_t info[4]);
/* out[0] / out[1] = kernel launches + exchanges (a peer-store push, a sync, an RCCL send / recv group; in
 * an in-process group one per exchange) the step's last forward / backward call enqueued for this rank.
 * With the one-launch owner update (the shape of MonolithMultiHashTableFusedOptimize,
 * RT/ops/multi_hash_table_update_op.cc:247-308: every shard's segments in one op) the count does not
 * depend on the world size; per 32 tables of the model. */
mhte_status mhte_shard_step_launches(mhte_shard_step* s, int32_t out[2]);
/* Launches of every instance of the one-launch owner update since the step was created (host-side counters, read
 * only): out[((one float per lane ? 2 : 0) + (world > 1 ? 1 : 0)) * 3 + kind], kind 0 = the fast loop of SGD /
 * Adagrad / FTRL tables, 1 = the generic loop (every other optimizer), 2 = the whole-segment optimizer.  Tables
 * with an occurrence filter take the per-peer form and count nowhere here. */
mhte_status mhte_shard_step_apply_launches(mhte_shard_step* s, int64_t out[12]);
/* What the step's last forward + backward put on the wire through send / recv pairs (the RCCL transport and the
 * in-process group, whose device copies stand for the pairs; 0 for identity / peer stores):
 * out[0] = pairs in total, [1] = exchanges, [2] = the most pairs any one exchange took, [3] = times the HOST
 * waited for the id blocks' counts inside the two calls.  The exact-size form (RCCL with whole-batch blocks)
 * packs the occupied part of a peer's table segments back to back: one pair per peer and exchange — [2] <=
 * world (+ world when the next batch's id headers ride in the gradient exchange's group), not world x T —
 * and a batch that was prepared a step ahead finds its counts on the host: [3] = 0.  The reference moves
 * every exchange as ONE all-to-all-v per tensor (native_training/distributed_ps_sync.py:131-159,357-479). */
mhte_status mhte_shard_step_wire_stats(mhte_shard_step* s, int64_t out[4]);
/* out[0] = ncclCommCount, out[1] = ncclCommUserRank of the step's own RCCL communicator (0, 0 when the
 * step has none: identity, peer stores, in-process group) — a launcher checks out[0] == world on
 * every rank before it trusts a multi-GPU number */
mhte_status mhte_shard_step_comm_ranks(mhte_shard_step* s, int32_t out[2]);
/* all `n` ranks of a world living in this process (created with unique_id NULL, world n): the same
 * step, with arrays of per-rank arguments */
mhte_status mhte_shard_group_forward(mhte_shard_step** steps, int32_t n, const int64_t* const* id,
                                     const int64_t* const* id_split, int64_t n_split,
                                     float* const* embedding, const int64_t* embedding_len,
                                     const int64_t* const* id_next,
                                     const int64_t* const* id_split_next, int64_t n_split_next,
                                     int32_t prefetched, void* stream);
mhte_status mhte_shard_group_backward(mhte_shard_step** steps, int32_t n, const float* const* value,
                                      const int64_t* value_len, const float* learning_rate,
                                      int64_t n_learning_rate, int64_t update_time,
                                      int64_t global_step, void* stream);

/* != 0 when table i fits the fused training step (row of <= 256 floats, or <= 64 when segment
 * boundaries are not multiples of 4 floats; no whole-segment optimizer): 1 = SGD / Adagrad / FTRL, 2 =
 * any per-element optimizer (Momentum, Adadelta, RMSProp, Adam, AMSGrad, MovingAverage, BatchSoftmax:
 * the step kernels' FULL instantiations).  0, and 2 for the unpipelined mhte_table_sum_optimize_n:
 * segment sum + optimize, which needs the ordered mhte_unique. */
int32_t mhte_table_fused_backward_ok(const mhte_multi_table* t, int32_t i);

/* ---- Quantization-aware training: the segment retrievers of a TRAINING table ------------------
 * The reference's EntryAccessor reads a row through a retriever (Retrieve in the lookup,
 * RT/hash_table/entry_accessor.cc:169-171; Backward in front of the optimizer, :187-195) that it picks
 * per segment from the segment's comp_config (:283-302; retrievers combine per segment,
 * CombineRetrievers): fixed_r8 ("qat8 in Bytedance PS", compressor/float_compressor.proto:29-33) ->
 * the fake-quant retriever, one_bit -> the HashNet retriever, fp32 / fp16 / none -> the raw one (the
 * compressor itself matters for SERVING entries only, which stay refused).  Rows stay fp32 in HBM.
 *   MHTE_RETRIEVER_FAKE_QUANT_R8  params {r}.  Lookups return FakeQuantizer(r).Quantize(w)
 *       (compressor/fake_quantizer.h:26-70): step = r / 128; NaN -> 0; w +- step / 2 by sign; the
 *       correctly rounded fp32 quotient by step truncated THROUGH AN INTEGER (-0.0 and small negatives
 *       give +0.0), clamped to [-128, 127], times step.  Backward is a no-op
 *       (retriever/fake_quant_retriever.cc:38-39).  A quotient outside int range, or +-inf, is undefined
 *       behaviour in the reference; here it saturates by sign (+127 * step, -128 * step).
 *   MHTE_RETRIEVER_HASH_NET       params {step_size, init_scale, max_scale, amplitude}
 *       (compressor/hash_net_quantizer.h:33-70).  Lookups return amplitude * tanhf(scale * w).  An
 *       Optimize first runs Backward per element on every gradient it hands to the optimizer (each
 *       occurrence's, or the sum's under MHTE_SUM_DUPLICATES / mhte_table_sum_optimize_n): where
 *       global_step % step_size == 0, scale = min(init_scale * powf(1 + 0.005 * global_step, 0.5),
 *       max_scale); then g *= amplitude * scale * (1 - tanhf(scale * w)^2), w the stored weight at that
 *       moment (a new id's: the initializer's value, RT/hash_table/cuckoo_embedding_hash_table.cc:346-353;
 *       a sequential duplicate's: the weight the previous occurrence left).  `scale` is state of the
 *       (table, segment): it starts at init_scale, lookups read the live value, it moves only in a
 *       call in which an id reaches the optimizer (not with n = 0, not when the admission filter drops
 *       every id), and it is not part of a checkpoint.  step_size <= 0 (a division by zero in the
 *       reference) and a GROUP_ADAGRAD segment: MHTE_INVALID_ARGUMENT.
 * Not replicated: the reference scales the CALLER's gradient tensor in place through a const_cast
 * (entry_accessor.cc:190-192); here the caller's buffer is not written.
 * Save / LookupEntry / dump read the stored weights (GetNum, entry_accessor.cc:225-232); Assign,
 * AssignAdd and Reinitialize write them raw.
 * A table with a non-raw retriever does not satisfy mhte_table_fused_backward_ok;
 * mhte_table_step_forward / _backward, mhte_multi_step_create and mhte_shard_step_create(_ipc) refuse
 * it by name (their kernels read rows raw), and the setter refuses a MultiHashTable that already has a
 * multi-table or id-sharded step (MHTE_FAILED_PRECONDITION).
 * mhte_table_set_retriever runs under the table's lock, behind the table's enqueued work, and has
 * taken effect when it returns; it (re)sets the segment's scale to init_scale.
 * mhte_table_get_retriever: the type and up to `cap` of its parameters.
 * mhte_table_hash_net_scale: the live scale of a HashNet segment into host memory; synchronises. */
enum { MHTE_RETRIEVER_RAW = 0, MHTE_RETRIEVER_FAKE_QUANT_R8 = 1, MHTE_RETRIEVER_HASH_NET = 2 };
mhte_status mhte_table_set_retriever(mhte_multi_table* t, int32_t table, int32_t segment, int32_t type,
                                     const float* params, int32_t n_params);
mhte_status mhte_table_get_retriever(mhte_multi_table* t, int32_t table, int32_t segment, int32_t* type,
                                     float* params, int32_t cap);
mhte_status mhte_table_hash_net_scale(mhte_multi_table* t, int32_t table, int32_t segment, float* host_out,
                                      void* stream);

/* MonolithUniqueKeyWithValueAndOffset (RT/ops/unique_mapping_ops.cc:51-155), one table at a time:
 * value_offset[q] = value_base + position*dim for the occurrence lists, value_offset_split[u] =
 * split_base + list start.  Inputs are the outputs of mhte_unique. */
mhte_status mhte_value_offsets(const uint32_t* seg_off, const uint32_t* seg_pos,
                               const uint32_t* n_unique_dev, int64_t n, int64_t value_base,
                               int64_t dim, int64_t split_base, int64_t* value_offset,
                               int64_t* value_offset_split, void* stream);

/* MonolithFillWithOffsetMap / MonolithFillWithOffsetMapGradient for ONE table
 * (RT/ops/unique_mapping_ops.cc:204-329).  pos [dev,n] indexes the unique-key list whose float
 * offsets into the flat buffer are offset_map[split[pos] .. split[pos+1]); value / backprop_grad
 * are [n, dim].  offsets_vec4 != 0 asserts that every offset is a multiple of 4 floats.
 * The reference's `pos < map size` InvalidArgument check is the caller's responsibility here. */
mhte_status mhte_fill_with_offset_map(const int64_t* pos, int64_t n, const float* value,
                                      const int64_t* value_offset_map,
                                      const int64_t* value_offset_map_split, int32_t dim,
                                      int32_t offsets_vec4, float* value_buffer, void* stream);
mhte_status mhte_fill_with_offset_map_gradient(const int64_t* pos, int64_t n, const float* grad,
                                               const int64_t* grad_offset_map,
                                               const int64_t* grad_offset_map_split, int32_t dim,
                                               int32_t offsets_vec4, float* backprop_grad,
                                               void* stream);

/* ---- the dense tower downstream of the embedding path -------------------------------------------
 * The ranking MLP that consumes fused_embedding_to_layout's output (native_training/layers/mlp.py:
 * Dense + ReLU stack ending in one logit; its gradient feeds fused_embedding_to_layout_grad): bf16
 * GEMMs on the matrix cores (csrc/mhte_gemm_kernels.h), fp32 master weights and accumulation, SGD
 * inside backward.  widths[n]: input width, hidden widths, 1 (the last layer has ONE output); every
 * width but the last and every batch are multiples of 128 (the GEMM tile).  Layer l in [0, n - 2]:
 * weight [widths[l+1]][widths[l]] row-major (torch.nn.Linear's layout), bias [widths[l+1]].
 *   forward   x [dev, batch x widths[0] fp32] -> y [dev, batch fp32]; keeps the activations
 *   backward  dy [dev, batch fp32] (the loss gradient at the logit) -> SGD step with learning_rate on
 *             every layer, dx [dev, batch x widths[0] fp32] when not NULL
 * One stream at a time; forward and backward of a step on the same stream. */
typedef struct mhte_dense_mlp mhte_dense_mlp;
mhte_status mhte_dense_mlp_create(const int32_t* widths, int32_t n_widths, int64_t max_batch,
                                  int32_t gpu_ordinal, mhte_dense_mlp** out);
void mhte_dense_mlp_destroy(mhte_dense_mlp* m);
mhte_status mhte_dense_mlp_set_params(mhte_dense_mlp* m, int32_t layer, const float* weight,
                                      const float* bias, void* stream);
mhte_status mhte_dense_mlp_get_params(mhte_dense_mlp* m, int32_t layer, float* weight, float* bias,
                                      void* stream);
mhte_status mhte_dense_mlp_forward(mhte_dense_mlp* m, const float* x, int64_t batch, float* y,
                                   void* stream);
mhte_status mhte_dense_mlp_backward(mhte_dense_mlp* m, const float* dy, float* dx,
                                    float learning_rate, void* stream);
/* Gradients out, parameters in: the joint between the tower and an optimizer that lives outside it (the
 * dense optimizers of this header, an allreduce, a clip over dense and sparse gradients together).
 * Additive to ABI 19: new symbols only; mhte_dense_mlp_backward computes the same bits as before.
 * Both take pointer tables: HOST arrays of n_widths - 1 DEVICE pointers (as mhte_ffm's operands are device
 * pointers and mhte_fused_reduce_and_split's tables host arrays), GEMM layers 0 .. n_widths - 3 first, then
 * the row-dot layer.  Shapes are mhte_dense_mlp_get_params': weight [widths[l+1]][widths[l]] and bias
 * [widths[l+1]]; the row-dot layer [1][widths[n_widths - 2]] and [1].  Neither waits for the device, reads
 * a device value on the host or allocates (the rule of mhte_ffm).
 *
 * mhte_dense_mlp_backward_grads: the backward chain of mhte_dense_mlp_backward (the last layer's backward,
 * per GEMM layer the split-K weight-gradient GEMM, the bias gradient and the GEMM of the gradient below;
 * dx optional as there) WITHOUT the SGD step: masters, biases and both bf16 copies keep their bits.  The
 * fp32 gradients are written to the caller's buffers instead, in the order of every sum of the SGD kernels:
 *   weight_grads[l][i] = ((+0 + slab_0[i]) + slab_1[i]) + ...  ascending over the split-K slabs of THIS
 *                        batch (fewer than the handle owns when batch < max_batch)
 *   bias_grads[l][n]   = the bias gradient as computed (a fixed-order tree over the batch)
 *   row-dot layer      = per element the 256 strided sums over the 64-row blocks' partials, then the 256-wide
 *                        tree (bias_grads[last][0] likewise)
 * so that mhte_dense_mlp_backward(lr) from the same state leaves exactly p - lr * g, rounded once per
 * operation, in every master.  Launches behind the chain: ONE for all layers, the row-dot layer's tree
 * included (the layers travel as a table in the kernel arguments; a tower of more than 16 GEMM layers takes
 * one launch per 16 layers — nothing is uploaded).  A destination that is 16-byte aligned takes 16-byte
 * accesses, any other 4-byte ones of the same elements: the same bits.  Destinations may lie anywhere, also
 * inside ONE flat buffer at mhte_aligned_flat_offsets (lens: the shapes above in list order): a caller that
 * does not clip exports straight into the allreduce buffer and skips mhte_aligned_flat_concat; the padding
 * between the tensors is not written.
 * mhte_dense_mlp_load_params: every layer's fp32 parameters from the caller's buffers into the masters, both
 * bf16 copies (W [N][K] and W^T [K][N], round to nearest even as after mhte_dense_mlp_set_params) and the
 * row-dot layer's vector and bias, in ONE launch (per 16 GEMM layers).  It does not wait: the sources stay
 * alive and unchanged until the stream has passed the call.  16-byte loads from a 16-byte aligned source,
 * 4-byte loads otherwise.
 * Checked on the host before any device call (MHTE_INVALID_ARGUMENT, "<entry point>: ..."):
 *   "dense_mlp_backward_grads: null argument: <m | dy | weight_grads | bias_grads | weight_grads[l] | ...>"
 *   "dense_mlp_backward_grads: <dy | dx | weight_grads[l] | bias_grads[l]> must be 4-byte aligned"
 *   "dense_mlp_load_params: null argument: <m | weights | biases | weights[l] | biases[l]>"
 *   "dense_mlp_load_params: <weights[l] | biases[l]> must be 4-byte aligned"
 * and, without a forward on this handle, MHTE_FAILED_PRECONDITION "dense mlp: backward without a forward".
 * Sizes cannot be checked from a pointer: a short buffer is the caller's error. */
mhte_status mhte_dense_mlp_backward_grads(mhte_dense_mlp* m, const float* dy, float* dx,
                                          float* const* weight_grads, float* const* bias_grads,
                                          void* stream);
mhte_status mhte_dense_mlp_load_params(mhte_dense_mlp* m, const float* const* weights,
                                       const float* const* biases, void* stream);
/* Read-only: GEMM launches of this handle since create, by role and tile shape (tests assert which
 * instantiation a shape reached).  out[2 * role + tile]: role 0 forward, 1 gradient of a hidden
 * layer, 2 gradient of the input (dx), 3 weight gradient; tile 0 = 128 x 128, 1 = 256 x 256. */
mhte_status mhte_dense_mlp_launch_counts(mhte_dense_mlp* m, int64_t out[8]);

/* ---- touched-key set (additive to ABI 19: new symbols only, nothing existing changes) ----------
 * The set of keys (int64 fid, int32 tag) that an update path changed since the last steal: the
 * HopscotchHashSet of RT/hopscotch/hopscotch_hash_set.cc:104-122,173-195 that the table bridge fills
 * on every Optimize / BatchOptimize / Reinitialize (RT/ops/embedding_hash_table_tf_bridge.cc:247-251,
 * 332-336,352-354) and the parameter-sync client drains (RT/ops/parameter_sync_tf_bridge.cc:70-90);
 * also the stand-alone op of NT/touched_key_set_ops.py (tag 0).  It lives on the device: an insert
 * allocates nothing and never synchronises with the host, so a step that records stays capturable.
 * Rule, key by key in segment-major then position-minor order: a set holding more than `capacity`
 * keys is dropped whole (dropped += size, clears += 1) before the key is added.  The reference's loss
 * of a key whose hopscotch displacement fails is not mirrored: this is the mathematical set.
 * Every int64 is a legal fid; tags are >= 0 (an attached set uses the table index).
 * max_insert (0 = capacity + 1) bounds the positions of one device call and with them the memory:
 * 16 bytes x the power of two >= 2 * (capacity + 1 + max_insert) slots; longer inputs are cut into
 * several calls here.  Consecutive calls on different streams are ordered by an event. */
typedef struct mhte_touched_key_set mhte_touched_key_set;
mhte_status mhte_touched_key_set_create(int64_t capacity, int64_t max_insert, int32_t device,
                                        mhte_touched_key_set** out);
/* also detaches the set from the MultiHashTable it is attached to */
void mhte_touched_key_set_destroy(mhte_touched_key_set* set);
/* ids [dev, n_max]; n_dev [dev u32] or NULL (= n_max): the number of leading ids that count */
mhte_status mhte_touched_key_set_insert(mhte_touched_key_set* set, const int64_t* ids, int64_t n_max,
                                        const uint32_t* n_dev, int32_t tag, void* stream);
/* out [host]: size, keys dropped by clears, clears, capacity.  Waits for the stream. */
mhte_status mhte_touched_key_set_stats(mhte_touched_key_set* set, int64_t out[4], void* stream);
/* GetAndClear: ids_out [dev, cap], tags_out [dev, cap] or NULL, *n [host] = keys written, in no
 * particular order.  cap < size: MHTE_INVALID_ARGUMENT and the set is untouched; cap >= capacity + 1
 * always suffices.  Waits for the stream.  Neither `dropped` nor `clears` changes. */
mhte_status mhte_touched_key_set_steal(mhte_touched_key_set* set, int64_t* ids_out, int32_t* tags_out,
                                       int64_t cap, int64_t* n, void* stream);
/* Attaches the set (NULL detaches): from here on mhte_optimize, mhte_fused_optimize, mhte_reinitialize,
 * mhte_table_optimize_n, mhte_table_sum_optimize_n, mhte_table_step_backward(_ahead) and
 * mhte_multi_step_backward insert (id, table index) for the ids they update — the step entry points
 * from the step's unique ids and device-side count, the multi-table step with ONE insert call over all
 * tables.  Assign, AssignAdd and lookups never record.  With an admission filter attached as well, the
 * op-level entry points record the ids the table holds after the update (ids_after_filter of the
 * bridge; the one recording path that may allocate and synchronise: its probe buffer grows when a call
 * brings more ids than any before it); the fused-step entry points refuse the combination with MHTE_INVALID_ARGUMENT (the single
 * table step at the call, the multi step at its creation and here), as the id-sharded step's creation
 * refuses a table with a set, and attaching here is refused while an id-sharded step of the table exists.
 * One set serves one MultiHashTable on its own device; destroying either side detaches.  A MultiHashTable may
 * be destroyed before or after the steps created on it. */
mhte_status mhte_multi_table_set_touched_key_set(mhte_multi_table* t, mhte_touched_key_set* set);

/* ---- measurement aid (no reference counterpart) ---------------------------------------------
 * Kernel-exact timing of the hot kernels for bench.py's `roofline`: after mhte_profile_arm(n) the
 * next n launches of the step kernels made by the calling thread go through
 * hipExtLaunchKernelGGL, whose start/stop HIP events carry the kernel's own begin/end timestamps
 * on its queue (the interval rocprofv3 --kernel-trace reports).  mhte_profile_read disarms,
 * waits for the recorded launches and returns per launch the kernel tag and the duration in
 * microseconds.  Tags: 1 lookup_kernel, 2 sum_apply_kernel, 6 slowpath_kernel, 7 dd_* / rd_*
 * (dedup on its own), 8 upsert_kernel, 9 step_fwd_kernel, 10 step_bwd_kernel, 19 gemm_nt_bf16_kernel.
 * Not for use inside a stream capture. */
mhte_status mhte_profile_arm(int32_t n);
mhte_status mhte_profile_read(int32_t cap, int32_t* kernel_tag, float* usec, int32_t* n_out);
/* Per-wavefront timeline of the step kernels, for finding what bounds a launch.  Between
 * mhte_trace_begin(dev_buf, cap) and mhte_trace_end every launch of a step / lookup / fused-backward
 * kernel made by the calling thread writes, per wavefront w of the launch, eight uint64 words at
 * dev_buf[8 * (offset + w)]: {begin, end} on the 100 MHz wall clock, the role the wavefront played
 * and up to five intermediate time marks (0 = not reached); roles: the role the wavefront
 * played (3 run dedup, 4 displacement pass, 5 lookup, 6 heavy work list, 7 item workgroup of the
 * apply, 8 id-major workgroup of the apply).
 * dev_buf [dev, 8 * cap_records uint64].  mhte_trace_end stops tracing and returns, per traced
 * launch, the kernel tag (as above), grid and block size and `offset`. */
mhte_status mhte_trace_begin(void* dev_buf, int64_t cap_records);
mhte_status mhte_trace_end(int32_t cap, int32_t* kernel_tag, int32_t* grid, int32_t* block,
                           int64_t* offset, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* MONOLITH_AMD_HASH_TABLE_H_ */
