/*
 * gpuq.h -- C ABI of libgpuq.so, the MI355X (gfx950) columnar physical-operator engine that stands
 * behind Ballista's executor as the task runner for the DataFusion hot path
 * (FilterExec / ProjectionExec / AggregateExec / HashJoinExec / SortExec / hash repartition).
 *
 * Drop-in boundary (citations relative to the reference tree, coralogix/arrow-ballista @ 2025-02-02):
 *   - ballista/executor/src/execution_engine.rs:34-60   ExecutionEngine / QueryStageExecutor traits:
 *     a GPU engine implements them in Rust and forwards the operator work to the functions below
 *     (binding shown in INTEGRATION.md).
 *   - ballista/core/src/execution_plans/shuffle_writer.rs:255,341-392  the per-batch pull loop and
 *     BatchPartitioner::partition that gpuq_partition_* replaces.
 *   - DataFusion v34 operators named by ballista/core/src/physical_optimizer/task_group.rs:23-31,
 *     parameter surface pinned by ballista/core/proto/datafusion.proto:1109-1525.
 *
 * Conventions
 *   - Plain C: pointers, sizes, POD structs.  No C++/torch/Arrow-library types.
 *   - Every function returns a gpuq_status (0 = OK); gpuq_last_error(ctx) gives the UTF-8 message.
 *     No exception crosses the boundary.
 *   - All data pointers in gpuq_column / index vectors are DEVICE pointers (HBM) unless a parameter
 *     says otherwise.  Layouts are Arrow's physical layouts (little-endian values, int32 offsets +
 *     bytes for Utf8, LSB-first validity bitmaps), so a host that owns Arrow buffers copies them to
 *     the device byte-for-byte.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work on that
 *     stream; the ones documented as synchronous also wait for it.
 *   - Handles are freed by exactly one *_free; distinct handles may be used from distinct threads.
 *   - There is no CPU fallback: without a usable HIP device gpuq_ctx_create fails.
 */
#ifndef GPUQ_H
#define GPUQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPUQ_ABI_VERSION 2

typedef enum gpuq_status {
  GPUQ_OK = 0,
  GPUQ_ERR_INVALID = 1,      /* bad argument / malformed descriptor */
  GPUQ_ERR_HIP = 2,          /* HIP runtime error (message has the hipError) */
  GPUQ_ERR_UNSUPPORTED = 3,  /* valid request the device path does not implement (fails loudly, never falls back) */
  GPUQ_ERR_CAPACITY = 4,     /* caller-provided output capacity too small; required size reported */
  GPUQ_ERR_INTERNAL = 5,
  GPUQ_ERR_CANCELLED = 6,    /* gpuq_task_cancel reached the task before it finished */
  GPUQ_ERR_RETRY = 7,        /* gpuq_ops_settle: something a deferred run assumed did not hold; run again without deferral */
  GPUQ_ERR_PEER = 8          /* exchange: a rank of the node announced a failure (or cannot hold what it would receive); no payload moved */
} gpuq_status;

/* Which refusal a GPUQ_ERR_UNSUPPORTED was, where a caller answers it by doing the work in another form (the native plan executor
   does, for the first two; a driver hands a plan with a node of the third kind to another executor).  The message is for people;
   this is what code branches on.  See gpuq_last_refusal. */
typedef enum gpuq_refusal {
  GPUQ_REFUSAL_NONE = 0,             /* any other reason: final */
  GPUQ_REFUSAL_LONG_STRING = 1,      /* a Utf8 value longer than 15 bytes reached a packed key or comparison */
  GPUQ_REFUSAL_WIDE_SORT_KEY = 2,    /* the composite sort key needs more than 128 bits */
  GPUQ_REFUSAL_NODE_NOT_NATIVE = 3   /* gpuq_plan_create: a node type the native executor does not run */
} gpuq_refusal;

/* Logical types (subset of ballista/core/proto/datafusion.proto:1004-1040 ArrowType). */
typedef enum gpuq_type {
  GPUQ_NULL = 0, GPUQ_BOOL = 1, GPUQ_INT32 = 2, GPUQ_INT64 = 3, GPUQ_DATE32 = 4, GPUQ_FLOAT64 = 5,
  GPUQ_DECIMAL128 = 6, GPUQ_UTF8 = 7, GPUQ_UINT32 = 8, GPUQ_UINT64 = 9,
  /* second wave: Arrow physical layout as well (1 / 2 / 4 / 8 bytes per value); kernels widen on load and narrow on store */
  GPUQ_INT8 = 10, GPUQ_INT16 = 11, GPUQ_UINT8 = 12, GPUQ_UINT16 = 13, GPUQ_FLOAT32 = 14,
  GPUQ_TIMESTAMP = 15, /* int64 count of `precision` = TimeUnit (0 s, 1 ms, 2 us, 3 ns) since the epoch; the time zone is schema metadata */
  GPUQ_DATE64 = 16,    /* int64 milliseconds since the epoch */
  GPUQ_DURATION = 17   /* int64 count of `precision` = TimeUnit, a span and not a point in time; laid out and carried like GPUQ_TIMESTAMP.
                          JSON {"Duration": "Second" | "Millisecond" | "Microsecond" | "Nanosecond"}, Arrow C data formats tDs tDm tDu tDn.
                          An Interval has no id: it exists as a literal only (the expression grammar below) */
  /* LargeUtf8 and Dictionary(_, T) columns are converted where they enter: gpuq_table_import_arrow and gpuq_ingest_* narrow the offsets / decode the dictionary while staging; inside, Utf8 has 32-bit offsets */
} gpuq_type;

/* Device representation of an output column. */
#define GPUQ_REPR_ARROW 0     /* Arrow physical layout */
#define GPUQ_REPR_PACKED15 1  /* Utf8 of <= 15 bytes as 16-byte value: bytes big-endian in bits 127..8, length in bits 7..0
                                 (convert with gpuq_unpack_utf8) */

typedef struct gpuq_column {
  int32_t type;            /* gpuq_type */
  int32_t precision;       /* Decimal128 */
  int32_t scale;           /* Decimal128 */
  int32_t repr;            /* GPUQ_REPR_* (inputs: ARROW) */
  const void* data;        /* values; Utf8: bytes; Bool: bitmap */
  const int32_t* offsets;  /* Utf8: length+1 offsets, else NULL */
  const uint8_t* validity; /* Arrow validity bitmap or NULL (no nulls) */
  int64_t length;
} gpuq_column;

typedef struct gpuq_field_info {
  char name[256];
  int32_t type, precision, scale, nullable, repr, width; /* width = bytes per row in the fixed-width device layout */
} gpuq_field_info;

typedef struct gpuq_ctx gpuq_ctx;
typedef struct gpuq_op gpuq_op;
typedef struct gpuq_join_table gpuq_join_table;

/* ---- context ----------------------------------------------------------------------------- */
/* Streams and threads: every call takes the HIP stream its work is queued on.  Calls made on ONE stream are ordered by that
   stream.  Several host threads may drive one device -- through one context or several -- each on its own stream and with its
   own operators / plans / join tables (the reference runs `concurrent_tasks` tasks on its task-runner pool,
   cpu_bound_executor.rs:94-131): the library recycles device memory through a process-wide pool and orders a block released
   under one stream behind its next user on another with an event (csrc/devbuf.h).  One operator, plan or join table must not be
   used from two threads at once.  gpuq_last_error() is per calling thread. */
int gpuq_abi_version(void);
/* json_opts: NULL or {"device":N}.  Fails (returns NULL) when no HIP device is usable;
   gpuq_last_error(NULL) then holds the reason. */
gpuq_ctx* gpuq_ctx_create(int device_ordinal, const char* json_opts);
void gpuq_ctx_free(gpuq_ctx* ctx);
const char* gpuq_last_error(gpuq_ctx* ctx);
/* The gpuq_refusal of the calling thread's last failing call, whichever gpuq_*_last_error its message went to.  Per calling thread,
   like the messages; meaningful right after a call on this thread returned GPUQ_ERR_UNSUPPORTED (a call that fails with any other
   status leaves GPUQ_REFUSAL_NONE, a call that succeeds leaves it alone).  gpuq_task_wait restores the worker thread's. */
int gpuq_last_refusal(void);
int gpuq_ctx_device_info(gpuq_ctx* ctx, char* buf, size_t cap); /* JSON: name, arch, cus, hbm_bytes */
/* Tuning switches (strings): "join_dense" = "0" | "1" (default 1; env GPUQ_JOIN_DENSE at ctx creation): join tables over ONE
   Int32 / Int64 / Date32 key whose build values span a bounded range are direct-addressed arrays instead of hash tables;
   "join_dense_ratio" = largest range / key-count ratio that still takes the array (default 4096);
   "join_radix" = "off" | "auto" | "force": partitioned probe (one LDS-staged radix pass over the probe rows on the high bits of
   key - min, then lookups that stay inside one L2-sized slice of the array at a time) for Inner / RightSemi joins over such
   an array; the pairs then come out in partition order instead of probe order.  Default "off": on MI355X the pass costs about
   what the random accesses it removes cost (2^28 probes: 5.5 vs 6.3 ms at 2^24 keys, 7.2 vs 7.3 ms at 2^27).
   "auto" takes it for >= 2^24 probe rows against a table of >= 64 MiB when a sample of the probe keys shows no locality;
   "join_radix_slice_log2" = table entries per partition (default 18 = 1 MiB slices). */
int gpuq_ctx_set_option(gpuq_ctx* ctx, const char* key, const char* value);

/* ---- runtime specialisation (JIT) ---------------------------------------------------------- */
/* The row front-end (column loads + expressions) of every operator exists twice: as interpreter kernels
   compiled ahead of time (always available, best for small inputs) and as a typed straight-line function
   generated from the same expression DAG and compiled with hiprtc on first use (best for large inputs).
   mode: "off" | "auto" | "wait" | "force".  "auto" (the default): nobody waits for a compile -- an input of >= min_rows rows hands its
   source to a worker thread on its first run and runs the interpreter kernels until the code object is there (a one-shot query does not
   pay hiprtc's 0.2-0.3 s per pipeline; smaller inputs are specialised when their program comes back a third time); gpuq_jit_wait
   blocks until the queue is empty (steady-state benches call it after their warm-up).  "wait": an input of >= min_rows rows waits for
   its compile (round 2's "auto").  "force": every input waits, errors are reported.  Falls back to the interpreter kernels when hiprtc
   is missing.  min_rows default 2^21; env GPUQ_JIT overrides at ctx creation. */
int gpuq_ctx_set_jit(gpuq_ctx* ctx, const char* mode, int64_t min_rows /* <0 = keep */);
int gpuq_ctx_jit_stats(gpuq_ctx* ctx, int* available, int* launches, char* last_error, size_t cap);
/* In "auto" mode a program that runs for the third time on inputs below min_rows is handed to a background thread for
   specialisation; its callers keep running the interpreter kernels until the compiled function is there.  This call waits
   until every compile requested so far has finished (benchmarks call it at the end of their warm-up). */
int gpuq_ctx_jit_wait(gpuq_ctx* ctx);
/* Call before the process exits (the Python binding registers it with atexit): waits for background compiles still in flight.  The
   run-time compiler's libraries are loaded on first use, i.e. after this library registered its own exit handler, so they are torn
   down first -- a worker thread still inside one of them at that moment takes the process down with it. */
void gpuq_jit_quiesce(void);
/* Compiled code objects are kept on disk ($GPUQ_JIT_CACHE_DIR, default $XDG_CACHE_HOME/gpuq-jit or ~/.cache/gpuq-jit; "off"
   disables), keyed by a hash of the whole translation unit, so only the first process on a host pays hiprtc for a pipeline
   (0.3-1.9 s); later processes load the code object (~ms).  Counters of this process: */
int gpuq_jit_cache_stats(int* disk_hits, int* compiles);

/* ---- device memory + Arrow C Data Interface ingest/egress ---------------------------------- */
/* A host that owns Arrow RecordBatches (arrow-rs `arrow::ffi`, pyarrow `_export_to_c`) hands them over
   here; buffers are copied to HBM through double-buffered pinned staging on `stream`.
   The structs are the Arrow C Data Interface ABI (https://arrow.apache.org/docs/format/CDataInterface.html). */
struct ArrowSchema {
  const char* format; const char* name; const char* metadata; int64_t flags; int64_t n_children;
  struct ArrowSchema** children; struct ArrowSchema* dictionary; void (*release)(struct ArrowSchema*); void* private_data;
};
struct ArrowArray {
  int64_t length; int64_t null_count; int64_t offset; int64_t n_buffers; int64_t n_children;
  const void** buffers; struct ArrowArray** children; struct ArrowArray* dictionary; void (*release)(struct ArrowArray*); void* private_data;
};
typedef struct gpuq_table gpuq_table;

/* Memory budget.  The reference runs operators under DataFusion's MemoryPool (RuntimeConfig::with_memory_limit; a SortExec or a join
   build that cannot reserve fails with ResourcesExhausted).  Every device byte this library holds -- operator workspaces, join tables,
   plan intermediates, imported / decoded tables -- is counted process-wide; with a limit set (bytes > 0; 0 = none; also the environment
   variable GPUQ_MEMORY_LIMIT at start-up) the allocation that would cross it fails with GPUQ_ERR_CAPACITY ("Resources exhausted: ...") and
   the call that needed it returns that status: the task fails, the process and its other tasks go on.  The caller's own input columns
   are not counted.  Nothing is spilled: the executors hold whole partitions, a partition that does not fit the budget has to be split
   by the planner (more partitions), as on the reference when spilling is disabled.
   gpuq_memory_stats: bytes in use now, the high-water mark (reset_peak != 0 sets it back to the current value after reading), bytes cached
   in the library's free list, and the limit. */
int gpuq_memory_limit(int64_t bytes);
int gpuq_memory_stats(int64_t* in_use_out, int64_t* peak_out, int64_t* cached_out, int64_t* limit_out, int reset_peak);

int gpuq_buffer_alloc(gpuq_ctx* ctx, size_t bytes, void** dev_out);
int gpuq_buffer_free(gpuq_ctx* ctx, void* dev);
int gpuq_copy_h2d(gpuq_ctx* ctx, void* stream, void* dst_dev, const void* src_host, size_t bytes); /* returns after the copy is enqueued and the host buffer is reusable */
int gpuq_copy_d2h(gpuq_ctx* ctx, void* stream, void* dst_host, const void* src_dev, size_t bytes); /* synchronous */

/* Import one RecordBatch (a struct-typed ArrowArray + its ArrowSchema).  The batch is NOT consumed: the
   caller keeps ownership and releases it as usual.  Supported column formats: b c C s S i I l L f g tdD tdm ts{s,m,u,n}:tz d:p,s u,
   and, converted while they are staged: U (LargeUtf8 -> 32-bit offsets; a column beyond 2^31 bytes is refused) and dictionary-encoded
   columns of any of these (decoded: the device column has the value type). */
int gpuq_table_import_arrow(gpuq_ctx* ctx, void* stream, const struct ArrowArray* batch, const struct ArrowSchema* schema, gpuq_table** out);
int64_t gpuq_table_num_rows(const gpuq_table* t);
int gpuq_table_num_columns(const gpuq_table* t);
int gpuq_table_column(const gpuq_table* t, int i, gpuq_column* col_out, gpuq_field_info* field_out);
void gpuq_table_free(gpuq_table* t);
/* Export device columns (GPUQ_REPR_ARROW or PACKED15) as a host RecordBatch; the caller releases `out`
   and `out_schema` through their release callbacks.  Synchronous. */
int gpuq_export_arrow(gpuq_ctx* ctx, void* stream, const gpuq_column* cols, const gpuq_field_info* fields, int n_cols, int64_t n_rows,
                      struct ArrowArray* out, struct ArrowSchema* out_schema);

/* ---- streaming ingest of a partition ------------------------------------------------------------------------------------
   The per-batch pull loop of a task (`stream.next()`, shuffle_writer.rs:341 / utils.rs:198) seen from the device: host Arrow
   RecordBatches (BASELINE configs[1]: 64 Ki rows each) are appended to ONE set of preallocated device columns.
   gpuq_ingest_push only queues a batch (it is MOVED, Arrow C Data Interface: the library calls its release callback once the
   copies have landed); n_threads workers (0 = 8) copy the buffers into their own pinned slots in parallel -- one thread feeding
   pinned memory cannot fill PCIe -- and issue the H2D copies on their own streams.  Batches land out of order; "rows landed" is
   the contiguous prefix that is complete.  A consumer reads the landed prefix through gpuq_ingest_columns (narrow `length`, or
   offset the pointers, to the row range it wants) on any stream while later batches are still in flight.
   max_rows / max_utf8_bytes (per Utf8 column) size the device columns; exceeding them is GPUQ_ERR_CAPACITY.  Nullable and
   Boolean columns need every batch but the last to hold a multiple of 8 rows.  Errors: gpuq_ingest_last_error(). */
typedef struct gpuq_ingest gpuq_ingest;
int gpuq_ingest_create(gpuq_ctx* ctx, const struct ArrowSchema* schema, int64_t max_rows, int64_t max_utf8_bytes, int n_threads, gpuq_ingest** out);
int gpuq_ingest_push(gpuq_ingest* ingest, struct ArrowArray* batch);
int gpuq_ingest_rows_landed(gpuq_ingest* ingest, int64_t* rows_out);
/* blocks until at least `rows` rows have landed, or everything pushed so far has; *rows_out = the landed prefix */
int gpuq_ingest_wait_rows(gpuq_ingest* ingest, int64_t rows, int64_t* rows_out);
int gpuq_ingest_columns(gpuq_ingest* ingest, gpuq_column* cols_out, gpuq_field_info* fields_out, int cap, int* n_out);
int gpuq_ingest_stats(gpuq_ingest* ingest, int64_t* rows_pushed, int64_t* rows_landed, int64_t* bytes_copied);
void gpuq_ingest_free(gpuq_ingest* ingest);      /* also frees the device columns */
const char* gpuq_ingest_last_error(void);

/* ---- scan-side decode ------------------------------------------- */
/* The leaves of the reference's TPC-H plans are CsvExec / ParquetExec over the files benchmarks/src/bin/tpch.rs:801-862
   registers (`.tbl` text with '|' and no header, or Parquet written by its `convert` command).  These entry points take the
   FILE bytes in host memory (read or mmap'ed by the caller -- the object-store read stays the reference's), move them to the
   device once and produce Arrow-layout columns in HBM as a gpuq_table; no value is parsed on the host.
   gpuq_csv_decode: `file_fields` describes every field of a line in order (name, type, precision/scale, nullable: an empty field
   of a nullable non-Utf8 column is NULL, as arrow-csv reads it); `projection` (or NULL = all) picks output columns by file index.
   A trailing delimiter before the newline (TPC-H .tbl) is accepted.  Types: Int32 Int64 Date32 (yyyy-mm-dd) Decimal128 Float64
   Boolean Utf8.  Refused loudly rather than decoded differently: quoted fields, a Float64 field outside the exactly-rounded fast
   path (written digits of 2^53 or more, or an exponent beyond -22..22 after the fraction), lines whose field count differs from the schema,
   blank lines, a carriage return that is not followed by a line feed, > 4 GiB per call.  A field outside its type's grammar or range
   (scan-side decode) is an error, never a clamped or wrapped value.
   gpuq_parquet_decode: flat schemas; physical BOOLEAN INT32 INT64 DOUBLE BYTE_ARRAY FIXED_LEN_BYTE_ARRAY(decimal); DATE and
   DECIMAL annotations; required / optional columns; PLAIN, PLAIN_DICTIONARY / RLE_DICTIONARY and RLE-boolean pages (v1 and v2); UNCOMPRESSED
   SNAPPY, LZ4_RAW and ZSTD column chunks (Snappy / LZ4 pages are decompressed without a serial walk: element positions by doubling, copies by
   pointer jumping; ZSTD pages -- the reference's `convert` default -- one wave per page: FSE / Huffman tables in LDS, the four literal streams on four
   lanes, copies on all 64; GZIP, BROTLI, LZO and the deprecated framed LZ4 are GPUQ_ERR_UNSUPPORTED).  `columns` (or NULL = all) projects by name; only the projected
   chunks' bytes cross PCIe.  The host parses the Thrift footer and page headers, one wave decodes one page.
   Errors: gpuq_scan_last_error() (thread-local). */
typedef struct gpuq_csv_options { char delimiter; char quote; int32_t has_header; } gpuq_csv_options;   /* 0 = default ',' / '"' */
int gpuq_csv_decode(gpuq_ctx* ctx, void* stream, const uint8_t* text, int64_t n_bytes, const gpuq_field_info* file_fields, int n_file_fields,
                    const int32_t* projection, int n_projection, const gpuq_csv_options* options, gpuq_table** out);
int gpuq_parquet_decode(gpuq_ctx* ctx, void* stream, const uint8_t* file, int64_t n_bytes, const char* const* columns, int n_columns, gpuq_table** out);
/* the same over selected row groups (indices into the file's row groups, in the order given): predicate push-down stays where the
   reference has it -- ParquetExec prunes row groups from footer statistics on the host -- and only the surviving groups' chunks
   cross PCIe.  gpuq_parquet_row_groups: rows of every row group (host only), so that a caller can map its pruning to indices. */
int gpuq_parquet_decode_groups(gpuq_ctx* ctx, void* stream, const uint8_t* file, int64_t n_bytes, const char* const* columns, int n_columns,
                               const int32_t* row_groups, int n_row_groups, gpuq_table** out);
int gpuq_parquet_row_groups(const uint8_t* file, int64_t n_bytes, int64_t* rows_out, int cap, int* n_out);
/* host only: leaf columns (type = -1 where the device has no decoder) and row count from the footer */
int gpuq_parquet_schema(const uint8_t* file, int64_t n_bytes, gpuq_field_info* fields_out, int cap, int* n_out, int64_t* rows_out);
/* Host only: row-group pruning as the reference's ParquetExec does it, from the byte range of a PartitionedFile and the footer's
   chunk Statistics (csrc/parquet_prune.h).
   row groups of `file` that lie in [range_start, range_end) (range_end < 0: the whole file) and that the predicate
   (expression JSON over `file_fields`, or NULL) may be true in: indices ascending into row_groups_out (cap entries),
   their number into *n_out, the number the range alone selected into *n_in_range_out.  row_groups_out NULL with cap 0 only counts.
   A group is dropped only when its statistics PROVE that no row makes the predicate true; whatever is not understood keeps it:
   - understood: `column op literal` / `literal op column` with op in = < <= > >= and a literal of EXACTLY the column's type (a decimal:
     same precision and scale; nothing under a cast); `column IN (literals)`, not negated (any element in [min, max]); IS NULL (unless
     null_count is present and 0); IS NOT NULL (unless null_count is present and equals the chunk's num_values); AND (both sides), OR
     (either side); NOT over such a comparison (the operator is negated; any other NOT keeps).  `!=` never prunes.  A NULL literal in a
     comparison drops every group; so does any comparison over a group whose null_count equals num_values (null_count absent: not
     known to be all NULL).
   - columns are named, against `file_fields`; a column that is not in the file, or is declared with another type than the file
     holds, keeps the group.
   - min / max are bounds, never attained values (string bounds may be truncated): `>` against a max equal to the literal prunes,
     `>=` keeps.
   - min_value / max_value are used for every supported type; the deprecated min / max only for INT32 / INT64 physical columns that
     are signed integers, dates, timestamps or decimals (never BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY, unsigned integers).
   - bytes: signed integers, Date32, Timestamp and INT32 / INT64 decimals little-endian signed; UInt8..UInt64 unsigned; decimals on
     FIXED_LEN_BYTE_ARRAY / BYTE_ARRAY big-endian two's complement of 1..16 bytes; Utf8 bytewise unsigned, a proper prefix first
     (gpuq_utf8_compare's order); Boolean one byte; INT96 none.
   - Float32 / Float64 columns are never pruned on (writers leave NaN out of min / max; what a NaN row compares to is the comparison
     kernel's business and nothing here depends on it).
   - a value whose length does not fit its physical type, or min > max in the column's order: the group is kept, the call succeeds.
   - a row group belongs to the range that holds the file offset of its first column chunk's first page (dictionary page if there is
     one); ranges that tile [0, file size) select every row group exactly once. */
int gpuq_parquet_prune(const uint8_t* file, int64_t n_bytes, const char* predicate_json,
                       const gpuq_field_info* file_fields, int n_file_fields,
                       int64_t range_start, int64_t range_end,
                       int32_t* row_groups_out, int cap, int* n_out, int* n_in_range_out);
const char* gpuq_scan_last_error(void);

/* ---- compiled operators ------------------------------------------------------------------ */
/* Descriptor JSON (see INTEGRATION.md for the grammar).  Expression nodes mirror PhysicalExprNode
   (datafusion.proto:1142-1180): column, literal, binary_expr (+ - * / %, the comparisons, AND / OR, & | ^ over two integers
   of one type, and + - over dates, timestamps, Intervals and Durations: below), scalar_function (date_part, substr, coalesce, nullif, nanvl, isnan, iszero, abs, signum, ceil, floor, trunc, round, sqrt:
   INTEGRATION.md has the argument types), cast, try_cast, not_expr, is_null_expr,
   is_not_null_expr, negative, in_list, case_ (like_expr is evaluated by gpuq_like_utf8 and lowered to a Boolean column by the plan
   executor).  "op" is one of
     "filter"      FilterExec        {input, predicate}
     "project"     ProjectionExec    {input, exprs:[{expr,name}]}
     "aggregate"   AggregateExec     {input, mode:Partial|Final|FinalPartitioned|Single|Merge, group_expr:[{expr,name}],
                                      aggr_expr:[{fn, expr, expr2?, name, filter?}], predicate?, strategy?:auto|tiny|hash|lds|radix|runs, expected_groups?}
                   mode Merge (no DataFusion mode: it exists for the plan executor's lowering of grouping sets, below) reads state columns
                   as a Final does, by position, and emits them as a Partial does: its output fields have the names and types of the
                   Partial over the same functions, one row per key tuple.
                   fn (any letter case; one row of AGG_FNS in csrc/agg_compile.cpp each) and the state columns "<name>[..]" its Partial emits
                   and its Final reads, by position, after the group columns:
                     COUNT (expr optional: COUNT(*))                   [count]
                     SUM                                               [sum]
                     AVG                                               [count] [sum]
                     MIN | MAX                                         [min] | [max]
                     VARIANCE = VAR = VAR_SAMP, VARIANCE_POP = VAR_POP,
                     STDDEV = STDDEV_SAMP, STDDEV_POP                  [count] [mean] [m2]
                     COVARIANCE = COVAR = COVAR_SAMP,
                     COVARIANCE_POP = COVAR_POP   (expr, expr2)        [count] [mean1] [mean2] [algoConst]
                     CORRELATION = CORR           (expr, expr2)        [count] [mean1] [m2_1] [mean2] [m2_2] [algoConst]
                     BIT_AND | BIT_OR | BIT_XOR  (Int8..Int64, UInt8..UInt64; result and state: the argument's type)
                                                                       [bit_and] | [bit_or] | [bit_xor]
                     BOOL_AND | BOOL_OR          (Boolean)             [bool_and] | [bool_or]
     "join_build"  HashJoinExec build (left) side  {input, on:[expr], predicate?, null_equals_null?,
                                                     build_side_rows?: false = gpuq_join_build_side_rows will not be called (Inner / Right / RightSemi / RightAnti)}
     "join_probe"  HashJoinExec probe (right) side {input, on:[expr], predicate?, join_type, null_equals_null?}
     "sort"        SortExec          {input, expr:[{expr, asc, nulls_first}], fetch?}
     "partition"   BatchPartitioner  {input, hash_expr:[expr], partition_count}
   "input" = {"fields":[{"name","type","nullable","side"}]}; side k>0 means the column is addressed
   through index vector k of the call (late materialisation after a filter or join).

   Interval and Duration arithmetic (values as arrow-arith 49 computes them under DataFusion 34).  u is a TimeUnit.
     Date32       + -  Interval      -> Date32            Interval    +  Date32 / Timestamp(u)  -> the same, commuted
     Timestamp(u) + -  Interval      -> Timestamp(u)      Timestamp(u) -  Timestamp(u)          -> Duration(u)
     Timestamp(u) + -  Duration(u)   -> Timestamp(u)      Duration(u)  +  Timestamp(u)          -> Timestamp(u)
     Duration(u)  + -  Duration(u)   -> Duration(u)       negative Duration(u)                  -> Duration(u)
   The result is nullable iff an operand is; a NULL Interval literal makes it NULL.  Date32 + - integer -> Date32 and
   Date32 - Date32 -> Int32 are as before.
   An Interval is a LITERAL: {"literal": {"type": {"Interval": kind}, "value": v}} with
     kind "YearMonth"     v = the months (i32) as a string, like the other integer literals
     kind "DayTime"       v = {"days": i32, "milliseconds": i32}
     kind "MonthDayNano"  v = {"months": i32, "days": i32, "nanoseconds": i64}
   A missing member, a non-integer or a value out of its width is GPUQ_ERR_INVALID and names the member.  An Interval as a field's
   type, a cast's target or an expression's result is refused ("Interval columns are not carried").
   A Duration is a column type (GPUQ_DURATION) and a literal ({"type": {"Duration": unit}, "value": count}).  It passes as an opaque
   64-bit integer wherever a Timestamp does: import / export, ingest, projection, filter, comparison with a Duration of its unit,
   sort / group / join key, COUNT / MIN / MAX.  cast Duration(u) <-> Int64 keeps the count.
   Values:
     months     (y, m, d) -> month index y * 12 + (m - 1) + - k -> (y', m'), d' = min(d, days in month (y', m')); proleptic Gregorian
     Date32     months first, then + - days, then + - the sub-day part as whole days truncated toward zero (a DayTime of
                -86,399,999 ms leaves a date unchanged)
     Timestamp  the count is split by floor division into (day, time of day), the day is shifted by the months and the time of day
                kept, then days of 86,400 s, then the sub-day part exactly; a part that is not a whole number of u floors the
                exact instant to u (Timestamp(Second) + 1,500 ms adds one second, - 1,500 ms takes two)
     Timestamp - Timestamp, Timestamp + - Duration, Duration + - Duration: 64-bit wrapping, at the node
   A Date32 result outside int32 days or a Timestamp result outside int64 is an error of the run (GPUQ_ERR_INVALID, the message names
   the expression), as a decimal overflow is: never a silent value.  Years beyond chrono's +-262,143, where arrow-arith raises, are
   computed, not refused.
   Refused by name (GPUQ_ERR_UNSUPPORTED, GPUQ_REFUSAL_NONE): Date64 + - Interval; Date32 + - Duration; Timestamp + - Interval over a
   field whose type carries a time zone other than none / "UTC" / "+00:00" (month arithmetic in local time is not built; Duration
   arithmetic is zone-free and allowed); two Timestamp or Duration operands of different units (the plan carries the casts);
   Interval op Interval; * / % with an Interval or a Duration; a comparison with an Interval operand; Interval - Date32 / Timestamp;
   a cast between two Duration units or between a Duration and anything but Int64; SUM / AVG and the moment family over a Duration. */
int gpuq_op_create(gpuq_ctx* ctx, const char* json, gpuq_op** out);
/* Host-only: compiles the descriptor without a device and writes a JSON description (program
   listing, output schema; an aggregate also "posts": every program of its result projection, in order, "post" being the first
   and "post_programs" their number) to buf.  Used for plan validation and by the CPU test-suite. */
int gpuq_compile_check(const char* json, char* buf, size_t cap);
/* Host-only: the source the JIT path would hand to hiprtc for this descriptor and sink kernel id. */
int gpuq_compile_jit_source(const char* json, int kernel_id, char* buf, size_t cap);
void gpuq_op_free(gpuq_op* op);
int gpuq_op_num_outputs(gpuq_op* op);
int gpuq_op_output_field(gpuq_op* op, int i, gpuq_field_info* out);

/* Input of one operator call: columns in the order of the descriptor's input.fields.
   n_rows = number of driving positions: the table length, or the length of the index vectors when
   any are given (every index vector has n_rows entries; 0xFFFFFFFF = no row -> NULLs). */
typedef struct gpuq_input {
  const gpuq_column* cols;
  int32_t n_cols;
  int32_t n_via;
  int64_t n_rows;
  const uint32_t* via[3];
  /* Deferred execution (below): NULL, or a device u64 holding the ACTUAL number of driving positions; n_rows is then only an
     upper bound (it sizes grids and workspaces) and the kernels stop at min(n_rows, *n_rows_dev).  This is how one operator's
     count -- join pairs, filter survivors, groups -- reaches the next without a host round trip.  Honoured by gpuq_filter_run,
     gpuq_project_run, gpuq_aggregate_run_deferred, gpuq_join_build_run, gpuq_join_probe_run and gpuq_sort_run; every other
     entry point refuses an input that carries it (GPUQ_ERR_INVALID). */
  const uint64_t* n_rows_dev;
} gpuq_input;

/* FilterExec.  Writes the passing driving positions (or via[payload_via-1][pos] when payload_via>0),
   in input order, to sel_out (capacity n_rows) and their number to *count_out (device u64).
   Asynchronous.  NULL predicate results drop the row. */
int gpuq_filter_run(gpuq_op* op, void* stream, const gpuq_input* in, int payload_via, uint32_t* sel_out, uint64_t* count_out);

/* ProjectionExec / take: evaluates the expressions for every driving position into caller-allocated
   fixed-width columns (outs[i].data: n_rows * width bytes; outs[i].validity: ceil(n_rows/64)*8 bytes or
   NULL).  Asynchronous. */
int gpuq_project_run(gpuq_op* op, void* stream, const gpuq_input* in, gpuq_column* outs, int n_outs);

/* AggregateExec.  Strategy "auto" picks the kernel by cardinality: <= 64 groups an LDS dictionary with per-lane accumulators;
   a few hundred to a few thousand, block-local LDS tables flushed to a global one ("lds"); >= 4096 known groups on >= 2^20
   rows, radix partitioning + one LDS table per bucket ("radix"); otherwise / unknown a global hash table ("hash").  Where the
   table would be next, input of >= 2^20 rows whose key packs into one 62-bit word and whose accumulators are integer sums, counts
   or bitwise is first tried as runs of equal keys with increasing heads ("runs": one result row per run, in input order, no
   table); input that is not so clustered falls to the table in the same call and is not tried again.  The
   group count is taken from expected_groups, else from this operator's previous run -- keep operators alive across the
   partitions of a stage.  outs: caller-allocated columns of capacity `cap` rows in output-schema order.
   Synchronous (the group count decides the strategy and the result length); *n_groups_out (host)
   receives the number of groups.  GPUQ_ERR_CAPACITY when cap is too small. */
int gpuq_aggregate_run(gpuq_op* op, void* stream, const gpuq_input* in, gpuq_column* outs, int n_outs, int64_t cap,
                       int64_t* n_groups_out);

/* HashJoinExec build side: inserts every passing row; the table keeps, per key, the chain of build
   row ids (payload = driving position, or via[payload_via-1][pos]).  build_rows_bound = exclusive
   upper bound of payload values.  Synchronous. */
int gpuq_join_build_run(gpuq_op* op, void* stream, const gpuq_input* in, int payload_via, int64_t build_rows_bound,
                        gpuq_join_table** out);
void gpuq_join_table_free(gpuq_join_table* t);
/* Chain fusion for (A |x| B) |x| C when A's keys are unique: the second join's build side is "the rows of B whose key is in A's
   table".  Instead of probing A with B, materialising the pairs and building from them through an index vector, build the second
   table straight from B: the operator's descriptor carries "semi_on" (B's key expressions for A, next to "on", B's key expressions
   for C), every row of `in` (= B) that passes the fused predicate is looked up in semi_table (= A's table, gpuq_join_build_run)
   and inserted when found -- one pass over B, the build row is B's position (payload_via must be 0).  semi_hits_out (device u32 per
   row of B, or NULL) receives A's row for every surviving position (A's columns are then read through it as an index vector);
   rows_out (device u64, or NULL) the number of surviving rows.  GPUQ_ERR_INVALID when semi_table holds duplicate keys
   (gpuq_join_table_has_duplicates): fall back to the two-step form.  Otherwise as gpuq_join_build_run. */
int gpuq_join_build_run_semi(gpuq_op* op, void* stream, const gpuq_input* in, int payload_via, int64_t build_rows_bound,
                             gpuq_join_table* semi_table, uint32_t* semi_hits_out, uint64_t* rows_out, gpuq_join_table** out);
int gpuq_join_table_has_duplicates(const gpuq_join_table* t);
/* Probe side.  Emits matching (build_row, probe_row) pairs (probe_row = position or via[..]) into
   out_build/out_probe (capacity out_cap pairs; out_build may be NULL for RightSemi/RightAnti) and the
   total pair count into *count_out (device u64).  Join types follow datafusion.proto:280-289; the
   build side is DataFusion's LEFT input.  For Left/Full/LeftSemi/LeftAnti the build rows reached are
   marked in the table; fetch them with gpuq_join_build_side_rows.  Asynchronous; call
   gpuq_op_check afterwards to learn about capacity overflow. */
int gpuq_join_probe_run(gpuq_op* op, void* stream, gpuq_join_table* t, const gpuq_input* in, int payload_via,
                        uint32_t* out_build, uint32_t* out_probe, uint64_t out_cap, uint64_t* count_out);
/* matched != 0: build rows with >= 1 match (LeftSemi); matched == 0: build rows never matched
   (Left/Full outer remainder, LeftAnti).  Ordered.  Asynchronous. */
int gpuq_join_build_side_rows(gpuq_join_table* t, void* stream, int matched, uint32_t* rows_out, uint64_t* count_out);

/* HashJoinExec with a JoinFilter on a non-inner join (datafusion.proto:1346-1360 `filter`): a pair that fails the filter does not
   count as a match.  The executors probe as Inner, filter the pairs, and derive the outer / semi / anti parts from the pairs
   that survive: gpuq_mark_rows sets bitmap bit rows[i] for every surviving pair (0xFFFFFFFF skipped; bitmap zeroed by the
   caller, 8-byte aligned, one bit per row of that side); the unmarked / marked rows are then selected with an ordinary filter
   over that Boolean column.  Asynchronous. */
int gpuq_mark_rows(gpuq_ctx* ctx, void* stream, const uint32_t* rows, int64_t n, uint8_t* bitmap);

/* CrossJoinExec (datafusion.proto:1382-1385; what DataFusion plans for an uncorrelated scalar subquery: q11 / q15 / q22's threshold is a
   one-row side): the row pairs of left x right, left-major -- left_rows_out[i] = i / n_right, right_rows_out[i] = i % n_right for
   i < n_left * n_right (< 2^32).  The executor reads both sides through these index vectors like a hash join's pairs.  Asynchronous. */
int gpuq_cross_pairs(gpuq_ctx* ctx, void* stream, int64_t n_left, int64_t n_right, uint32_t* left_rows_out, uint32_t* right_rows_out);

/* gpuq_sort_run that also hands back the FIRST key's column in sorted order when it can be rebuilt from the sorted records (one key of
   an integer-like type -- Int8..Int64, UInt*, Date32 / Date64, Timestamp, Decimal128 -- whose values span at most 2^63, more rows than one block
   sorts): key_data_out = n values of the key's width, key_validity_out = (n + 63) / 64 * 8 bytes (NULL when the key cannot be NULL).
   *decoded_out = 1: written (a sequential pass; the caller need not gather that column through the permutation), 0: not written. */
int gpuq_sort_run_keys(gpuq_op* op, void* stream, const gpuq_input* in, uint32_t* perm_out, void* key_data_out, uint8_t* key_validity_out, int* decoded_out);

/* SortExec: writes the permutation (driving positions in sorted order; stable) to perm_out (n_rows).
   The call reads the key range back (one stream synchronisation in the middle).  From 2^22 rows on the range comes from a row
   sample and the pack kernel verifies it; the call then waits for one word at the end and re-runs with the exact range when the
   guess did not hold (env GPUQ_SORT_SPECULATE=0: always the exact range, the permutation is the same either way). */
int gpuq_sort_run(gpuq_op* op, void* stream, const gpuq_input* in, uint32_t* perm_out);

/* Ordered fan-in -- CoalesceTasksExec with `order_by` / SortPreservingMergeExec (coalesce_tasks.rs:162-170 `streaming_merge`):
   `in` is the concatenation of n_runs runs, run r = rows [run_offsets[r], run_offsets[r+1]) (host array of n_runs + 1 entries,
   empty runs allowed), each already in the order of `op` (a "sort" operator).  Writes the permutation of the merged order; equal
   keys keep (run, row) order, i.e. the result equals the stable sort of the concatenation.  log2(n_runs) merge-path rounds on the
   device, one read + one write of the (key, row) records per round -- or, when the packed key is so narrow that its radix passes
   cost less than the rounds (many runs, <= 32 key bits), those passes: the permutation is the same.  Runs that are NOT sorted
   give an unspecified permutation through the rounds. */
int gpuq_merge_run(gpuq_op* op, void* stream, const gpuq_input* in, const int64_t* run_offsets, int n_runs, uint32_t* perm_out);

/* Hash repartition (BatchPartitioner::partition call site, shuffle_writer.rs:336-391):
   perm_out lists driving positions grouped by partition (input order inside a partition),
   part_offsets_out[p]..[p+1] (device u64, partition_count+1 entries) delimit partition p.
   partition = mix64-hash(keys) % partition_count -- gpuq's own function (ahash
   assignment is not a portable contract).  Asynchronous. */
int gpuq_partition_run(gpuq_op* op, void* stream, const gpuq_input* in, uint32_t* perm_out, uint64_t* part_offsets_out);

/* Deferred execution: one host round trip per plan instead of one or two per operator.
   An operator's synchronous entry points read small things back (a build side's key range, "did the table fill up", the number of
   groups, a sort key's range) because the next decision depends on them.  An operator that has completed a synchronous run
   REMEMBERS what it learned; with gpuq_op_set_deferred(op, 1) its next runs assume the same answers, queue all their kernels
   without waiting, let the kernels verify the assumptions (a key outside the remembered range, a table or an output that turned
   out too small, a row that does not fit the remembered sort-key layout raise bits in the operator's status word) and hand row
   counts on as device words (gpuq_input.n_rows_dev).  The caller then settles everything at once: gpuq_ops_settle waits for the
   stream ONCE, reads the status words of all the operators and any number of count words in one copy, and returns GPUQ_OK, or
   GPUQ_ERR_RETRY when an assumption did not hold -- the results of the deferred runs are then void and the caller runs the
   operators again synchronously (which refreshes what they remember).  gpuq_op_can_defer tells whether an operator has a
   completed synchronous run to go by; without one a deferred call simply runs synchronously.  The native plan executor drives
   its plans this way from their second execution on (csrc/plan_exec.cpp). */
int gpuq_op_set_deferred(gpuq_op* op, int on);
int gpuq_op_can_defer(gpuq_op* op);
/* gpuq_aggregate_run without the wait: *n_bound_out (host) = capacity bound of the result, *n_groups_dev_out = device u64 holding
   the actual group count (valid until the operator's next run); the result columns hold that many rows.  When the operator
   cannot defer (no completed synchronous run, or a strategy without a deferred form) this IS gpuq_aggregate_run: *n_bound_out is
   then exact and *n_groups_dev_out NULL. */
int gpuq_aggregate_run_deferred(gpuq_op* op, void* stream, const gpuq_input* in, gpuq_column* outs, int n_outs, int64_t cap,
                                int64_t* n_bound_out, const uint64_t** n_groups_dev_out);
/* One wait for everything deferred on `stream`: the status words of ops[0..n_ops) and the device u64 words[0..n_words) (copied to
   words_out, host).  GPUQ_ERR_RETRY when an operator's assumptions did not hold (it forgets them); other errors as gpuq_op_check. */
int gpuq_ops_settle(gpuq_ctx* ctx, void* stream, gpuq_op* const* ops, int n_ops, const uint64_t* const* words, int n_words, uint64_t* words_out);

/* Waits for `stream`, then reports device-side conditions raised by the op's kernels since the last
   check (string longer than 15 bytes in a packed comparison, output capacity overflow, ...). */
int gpuq_op_check(gpuq_op* op, void* stream);
/* Debug: the full source handed to hiprtc for sink kernel `kernel_id`: 1 filter bitmap, 2 project, 3 tiny aggregate,
   4 hash aggregate, 5 join build, 6 chained probe, 7 unique probe, 8 sort min/max, 9 sort pack, 10 partition ids,
   11 radix-aggregate bucket ids, 12 radix-aggregate buckets, 13 block-local (LDS) aggregate, 14 join key range,
   15 partitioned-probe pack (GPUQ_SINK_* in csrc/gpuq_kernels.h). */
int gpuq_op_jit_source(gpuq_op* op, int kernel_id, char* buf, size_t cap);

/* arrow `take` for Utf8 payload columns of ANY string length (datafusion's materialisation of a join / filter / sort output):
   out[j] = col[idx[j]] (idx == NULL: identity; 0xFFFFFFFF or a NULL value -> NULL, length 0).  col must be Arrow layout
   (offsets + bytes).  offsets_out: n+1 int32; validity_out (optional, 8-byte aligned, ((n+63)/64)*8 bytes): written in full;
   data_out capacity data_cap bytes.  Two-call protocol: with data_cap too small (e.g. 0) the call computes offsets and
   validity, reports the required size in *data_len_out and returns GPUQ_ERR_CAPACITY; call again with a large enough
   buffer.  Synchronous up to the size read-back; the byte copy is queued on `stream`. */
int gpuq_take_utf8(gpuq_ctx* ctx, void* stream, const gpuq_column* col, const uint32_t* idx, int64_t n, int32_t* offsets_out, uint8_t* validity_out,
                   uint8_t* data_out, int64_t data_cap, int64_t* data_len_out);

/* Utf8 values of ANY length as group-by / join keys (q10's c_name, q16's p_type): the expression
   programs carry strings as 16-byte integers (<= 15 bytes); longer key columns are replaced by exact dictionary codes first.
   gpuq_utf8_max_len: the longest value of an Arrow-layout Utf8 column (rows through `idx` when given) -- tells an executor
   whether the rewrite is needed.  gpuq_utf8_dict_create(capacity_rows = rows that will be inserted) / gpuq_utf8_intern:
   insert != 0 fills the dictionary from ONE column and returns every row's code = the row id (in that column) of the string's
   representative; insert == 0 looks rows of ANOTHER column up (a join's probe side).  codes_out: int64[n];
   validity_out: (n + 63) / 64 * 8 bytes, bit i = row i has a code (0: the value is NULL, or -- lookup -- not in the dictionary, which
   an equi-join treats the same way).  Equal strings get equal codes, different strings different ones, whatever they hash to: a
   tag match is verified byte for byte.  The string of a code comes back with gpuq_take_utf8(dictionary column, rows = codes). */
/* Utf8 values of any length as SORT keys: gpuq_utf8_sort_piece writes piece `piece` of every string (rows through `idx` when
   given) as a 16-byte integer that compares like the bytes [14 piece, 14 piece + 14) do -- the bytes big-endian and zero padded,
   times 256, plus the number of bytes the piece holds, so that "ab" < "ab\0".  Sorting stably by the last piece, then the one
   before, ... (ceil(max_len / 14) passes; the executors' SortExec does this after the packed 15-byte key has refused) yields
   the bytewise order of the strings, which is Arrow's.  keys_out: n x 16 bytes (values < 2^120: a Decimal128(38, 0) column);
   validity_out: (n + 63) / 64 * 8 bytes, bit i = row i is not NULL.  Asynchronous. */
int gpuq_utf8_sort_piece(gpuq_ctx* ctx, void* stream, const gpuq_column* col, const uint32_t* idx, int64_t n, int piece, void* keys_out, uint8_t* validity_out);
typedef struct gpuq_utf8_dict gpuq_utf8_dict;
int gpuq_utf8_max_len(gpuq_ctx* ctx, void* stream, const gpuq_column* col, const uint32_t* idx, int64_t n, int32_t* max_len_out);
int gpuq_utf8_dict_create(gpuq_ctx* ctx, void* stream, int64_t capacity_rows, gpuq_utf8_dict** out);
int gpuq_utf8_intern(gpuq_utf8_dict* dict, void* stream, const gpuq_column* col, const uint32_t* idx, int64_t n, int insert, int64_t* codes_out, uint8_t* validity_out);
void gpuq_utf8_dict_free(gpuq_utf8_dict* dict);
/* an Int64 (or UInt32: codes are row ids) code column, with or without validity -> the row ids a take wants (NULL -> 0xFFFFFFFF) */
int gpuq_utf8_code_rows(gpuq_ctx* ctx, void* stream, const gpuq_column* codes, int64_t n, uint32_t* rows_out);

/* LikeExpr (PhysicalLikeExprNode, datafusion.proto:1240-1245: negated, case_insensitive, expr, pattern) of a Utf8 column in Arrow
   layout against a literal pattern: '%' any run of characters, '_' one character, "\\%" / "\\_" the literal characters (arrow-string's
   `like` / `nlike` with a scalar pattern).  idx (optional) addresses the column through an index vector; 0xFFFFFFFF or a NULL
   value gives NULL.  bits_out / validity_out: bitmaps of ((n+63)/64)*8 bytes, 8-byte aligned, written in full (validity_out may
   be NULL).  case_insensitive != 0 is GPUQ_ERR_UNSUPPORTED.  Asynchronous.  The result is a Boolean column an operator's
   expression can read like any other. */
int gpuq_like_utf8(gpuq_ctx* ctx, void* stream, const gpuq_column* col, const uint32_t* idx, int64_t n, const char* pattern, int negated, int case_insensitive,
                   uint8_t* bits_out, uint8_t* validity_out);

/* A comparison of two Utf8 operands of ANY length -- the register programs hold 15 bytes: `<` between longer values, or `=` between two
   columns, is refused there and the executors lower the comparison to a Boolean column computed here, over the Arrow-layout bytes
   (arrow-ord's order: bytewise, a proper prefix first).  op: 0 = , 1 != , 2 < , 3 <= , 4 > , 5 >= .  a (through idx_a) against b (through
   idx_b) or, with b == NULL, against the `literal_len` bytes at `literal` (host memory).  A NULL on either side gives NULL.
   bits_out / validity_out as gpuq_like_utf8.  Asynchronous. */
int gpuq_utf8_compare(gpuq_ctx* ctx, void* stream, const gpuq_column* a, const uint32_t* idx_a, const gpuq_column* b, const uint32_t* idx_b, const char* literal,
                      int64_t literal_len, int64_t n, int op, uint8_t* bits_out, uint8_t* validity_out);

/* MEDIAN (AggregateFunction MEDIAN = 18 in datafusion.proto; DataFusion 34's MedianAccumulator [UPSTREAM-KNOWLEDGE: the crate source is
   not in the reference tree]).  Its state is the group's values, not a cell, so it is not a row of the operator's accumulator table: the
   "aggregate" descriptor of gpuq_op_create / gpuq_compile_check refuses it, and the native plan executor lowers an AggregateExec in mode
   Single that holds MEDIANs (next to any other aggregates) to one sort by (keys..., argument) per distinct argument plus the two entry
   points below.  The rules:
     argument   Int8..Int64, UInt8..UInt64, Float32, Float64, Decimal128(p, s); anything else is refused ("MEDIAN over <type>").
                The result has the argument's type (a decimal keeps p and s) and is always nullable.
     values     NULL arguments are ignored; with FILTER (WHERE p) -- the "filter" member of the aggregate entry -- a row where p is not
                true counts as a NULL argument.  The v non-NULL values of a group are ordered as SortExec orders them (floats by
                IEEE-754 totalOrder: -0.0 before 0.0, a positive NaN last).
     result     v = 0: NULL.  v odd: the value at rank v / 2.  v even: lo = rank v / 2 - 1 and hi = rank v / 2 combined on the
                column's own type -- integers and decimals: lo + hi wrapping at the declared width (8 / 16 / 32 / 64 / 128 bits), then
                divided by 2 truncating toward zero (Int8 100, 120 -> -18; -3, 0 -> -1); floats: (lo + hi) / 2 in the column's
                precision.
     no rows    ungrouped: one row holding NULL; grouped: no rows.
   Refused, with MEDIAN in the message: modes Partial / Final / FinalPartitioned (the state would be a list column), `distinct`, a
   Float32 / Float64 group key on a node with a MEDIAN (bytewise segment heads and the hash aggregate need not agree on -0.0 / NaN),
   group keys holding strings beyond 15 bytes.  APPROX_MEDIAN / APPROX_PERCENTILE_CONT are t-digest answers and stay refused.

   gpuq_segment_heads: the segments of a table whose rows are sorted by `key_cols` (n_keys fixed-width columns of n rows as they lie:
   Arrow layout, Utf8 as PACKED15; n_keys = 0: one segment).  Row i starts a segment when i = 0 or any key column differs from row
   i - 1: validity first (NULL equals NULL), then the value's bytes.  seg_id_out (int32[n], or NULL): every row's segment, dense from 0;
   starts_out (int32[starts_cap + 1]): the first row of segment g for g < min(G, starts_cap) and starts_out[G] = n when G <= starts_cap
   (starts_cap = n always suffices); *n_groups_dev (device u64) = G.  n >= 2^31 is GPUQ_ERR_UNSUPPORTED (the scan is 32-bit).
   gpuq_segment_median: one median per segment [starts[g], starts[g + 1]) of `value_col`, whose values are ascending inside every
   segment with the NULLs last.  out_data: n_groups values of the column's width; out_validity: (n_groups + 63) / 64 * 8 bytes, 8-byte
   aligned, written as whole words.  Both asynchronous. */
int gpuq_segment_heads(gpuq_ctx* ctx, void* stream, const gpuq_column* key_cols, int n_keys, int64_t n, int32_t* seg_id_out, int32_t* starts_out, int64_t starts_cap,
                       uint64_t* n_groups_dev);
int gpuq_segment_median(gpuq_ctx* ctx, void* stream, const gpuq_column* value_col, const int32_t* starts, int64_t n_groups, void* out_data, uint8_t* out_validity);

/* APPROX_DISTINCT (AggregateFunction APPROX_DISTINCT in datafusion.proto:637-648; DataFusion 34's HyperLogLog [UPSTREAM-KNOWLEDGE:
   physical-expr aggregate/approx_distinct.rs, hyperloglog.rs; the crate source is not in the reference tree]; the known answer
   approx_distinct(id) = 8 of ballista/client/src/context.rs:817-829).  Its state is a 16 KB sketch per group, so like MEDIAN it is no row
   of the operator's accumulator table: the "aggregate" descriptor of gpuq_op_create / gpuq_compile_check refuses it, and the native plan
   executor lowers an AggregateExec in mode Single that holds one (next to MEDIANs and any other aggregates) to a sort by the keys -- none
   when the node is ungrouped; MEDIAN's sorts when it holds MEDIANs too -- gpuq_segment_heads and the entry point below.  The rules:
     spelling   {"fn": "APPROX_DISTINCT", "expr": e, "name": n, "filter"?: p}; the name is matched without regard to case.
     argument   Int8..Int64, UInt8..UInt64, Date32, Date64, Timestamp, Decimal128, Float32, Float64; Utf8 while every value fits the
                packed 15 bytes (refused by name beyond that); Boolean and anything else is refused ("APPROX_DISTINCT over <type>").
     result     UInt64, never NULL: 0 for a group with no non-NULL argument.
     values     NULL arguments are ignored; with FILTER (WHERE p) a row where p is not true counts as a NULL argument.  Floats count by
                value: -0.0 and 0.0 are one value, every NaN is one value.
     no rows    ungrouped: one row holding 0; grouped: no rows.
     sketch     precision p = 14: m = 16384 one-byte registers, q = 50.  DataFusion's ahash is CPU-feature dependent, so the hash is this
                library's: h = mix64(lo ^ mix64(hi + 0x632BE59BD9B4E019)), the value half of the partition hash.  Types of 8 bytes or
                fewer: lo = the value widened to 64 bits (integers sign- or zero-extended by their type; floats their canonical bit
                pattern, zero-extended, Float32 its own 32 bits), hi = 0.  Decimal128 and packed Utf8: lo, hi = the two words as they
                lie.  idx = h & 16383; rho = ctz((h >> 14) | (1 << 50)) + 1 in 1..51; reg[idx] = max(reg[idx], rho).
     estimator  Ertl's improved estimator over the histogram C[0..51] of the register values, in Float64 without contraction
                (csrc/hll_estimate.h): z = m tau((m - C[51]) / m); for k = 50 .. 1: z = 0.5 (z + C[k]); z += m sigma(C[0] / m);
                E = floor(0.5 / ln 2 * m^2 / z + 0.5), and 0 when z is infinite (every register 0).
                sigma(x): x = 1: +inf; else y = 1, z = x; repeat x *= x, z += x y, y += y until z stops changing.
                tau(x): x = 0 or 1: 0; else y = 1, z = 1 - x; repeat x = sqrt(x), y *= 0.5, z -= (1 - x)^2 y until z stops changing; z / 3.
                The estimate is exact for a handful of values and within about 1.04 / sqrt(m) = 0.8 % (one standard error) beyond; it
                does not depend on the order of the rows, so it is reproducible bit for bit.
   Refused, with APPROX_DISTINCT in the message: modes Partial / Final / FinalPartitioned (the state would be a 16 KB binary column per
   group, and there is no Binary type yet), `distinct`, a DISTINCT aggregate on the same node, a Float32 / Float64 group key (bytewise
   segment heads and the hash aggregate need not agree on -0.0 / NaN), group keys holding strings beyond 15 bytes, 2^31 rows or more in
   a partition.

   gpuq_segment_approx_distinct: out[g] (n_groups device words) = the estimate over segment [starts[g], starts[g + 1]) of the first n_rows
   rows of `value_col` (Arrow layout as it lies; Utf8 as PACKED15); starts: n_groups + 1 ascending device int32.  Rows are in any order
   inside a segment; an empty segment gives 0; n_groups = 0 writes nothing.  tile_rows: the rows one block walks -- 0 for the library's
   choice, else a multiple of 256 (the result does not depend on it).  Scratch (two 16 KB sketches per tile) comes from the context's pool
   and counts against gpuq_memory_limit.  Asynchronous on `stream`. */
int gpuq_segment_approx_distinct(gpuq_ctx* ctx, void* stream, const gpuq_column* value_col, const int32_t* starts, int64_t n_groups, int64_t n_rows, int64_t tile_rows,
                                 uint64_t* out);

/* DISTINCT aggregates beside plain ones and over several arguments (AggregateExprNode.distinct, datafusion.proto; DataFusion 34's
   DistinctCount / DistinctSum / DistinctBitXor keep a hash set of ScalarValues per group [UPSTREAM-KNOWLEDGE: physical-expr aggregate/
   count_distinct.rs, sum_distinct.rs, bit_and_or_xor.rs; the crate source is not in the reference tree]).  The "aggregate" descriptor of
   gpuq_op_create / gpuq_compile_check keeps refusing `distinct`; the native plan executor lowers the node.
     scope      an AggregateExec of mode Single in which some entry has "distinct": true and which the two-level rewrite does not take
                (that one: every aggregate DISTINCT over the same argument, no filter, at most three group keys -- it stays as it is).
                Let D be the set of distinct (expr, filter) pairs among the node's DISTINCT entries: the input is projected to [keys, one
                column per member of D, what the other aggregates read], sorted once per member by (keys..., argument), the segments come
                from gpuq_segment_heads over the first sort, and the entry point below reduces every segment's run heads.
     result     agg(DISTINCT x) [FILTER (WHERE p)] runs over the set of non-NULL values of x in the group; a row where p is not true
                counts as a NULL x.
                  COUNT      Int64, never NULL.
                  SUM        the operator's SUM type and wrapping in mode Single: integers at 64 bits (Int64 / UInt64), Decimal128 at
                             128 bits with the operator's result precision, floats as Float64 (Float32 widened first); NULL when the set
                             is empty.
                  BIT_XOR    the operator's type (the argument's, integers only); NULL when the set is empty.
                  MIN, MAX, BIT_AND, BIT_OR, BOOL_AND, BOOL_OR: DISTINCT changes nothing; they run as the plain aggregate with its filter.
                  AVG and the VARIANCE / STDDEV / COVARIANCE / CORRELATION family are refused by name ("AVG(DISTINCT ...)"): DataFusion 34
                             plans none of them as DISTINCT [UPSTREAM-KNOWLEDGE: create_aggregate_expr; the crate is not in the tree].
                             AVG(DISTINCT x) alone keeps working through the two-level rewrite.
     argument   Int8..Int64, UInt8..UInt64: all three; Decimal128: COUNT and SUM (the operator has no BIT_XOR over decimals); Float32 /
                Float64: COUNT and SUM; Date32 / Date64 / Timestamp and Utf8 while every value fits the packed 15 bytes (refused by name
                beyond that): COUNT only; Boolean and anything else is refused ("COUNT(DISTINCT) over <type>").
     equality   two values are the same when their bytes are the same: -0.0 and 0.0 are two values, NaNs differ by payload -- ScalarValue
                equality on to_bits() in DataFusion [UPSTREAM-KNOWLEDGE], and what adjacency under the sort's totalOrder gives.
     no rows    ungrouped: one row, COUNT 0, SUM / BIT_XOR NULL; grouped: no rows.
   Refused (GPUQ_ERR_UNSUPPORTED, GPUQ_REFUSAL_NONE, the message names the function): modes Partial / Final / FinalPartitioned (the
   state would be a list column, as for MEDIAN); a DISTINCT on a node that also holds a MEDIAN or an APPROX_DISTINCT; Float32 / Float64
   group keys on a node lowered here; group keys or Utf8 arguments beyond 15 bytes; 2^31 rows or more in a partition.

   gpuq_segment_distinct: over segment [starts[g], starts[g + 1]) of the first n_rows rows of `value_col` (Arrow layout as it lies, width
   1 / 2 / 4 / 8 / 16 bytes; Utf8 as PACKED15) -- starts: n_groups + 1 ascending device int32, starts[0] = 0, starts[n_groups] = n_rows;
   gpuq_segment_median's precondition: values ascending inside every segment, NULLs last.  Row i is a run head when it is not NULL and
   either i = starts[g] or its bytes differ from row i - 1.  Per segment, each pointer optional (NULL: not computed):
     out_count     int64: the number of run heads.
     out_sum       the SUM of the run heads' values: integers and decimals in a 128-bit cell (the operator's, wrapping), stored at
                   sum_width = 8 (the low word) or 16 bytes; floats in Float64 (sum_width 8), Float32 widened first.
     out_xor       the XOR of the low 64 bits of the run heads' two's-complement patterns, its low xor_width = 1 / 2 / 4 / 8 bytes stored.
                   (The entry point takes a Decimal128 column here too, by its low word; no plan reaches that: the lowering refuses
                   BIT_XOR(DISTINCT) over decimals, as above.)
     out_validity  bit g = count > 0, written as whole 64-bit words (8-byte aligned, padded to a multiple of 8 bytes).
   An empty segment gives 0 / NULL; n_groups = 0 writes nothing.  One segmented scan of the window functions' shape per accumulator
   (SUM, BIT_XOR; COUNT comes with either, or runs alone): three launches, work proportional to n_rows whatever the segments are, no
   atomics -- the order of combination depends on (n_rows, starts) only, so a Float64 SUM is the same bits on every run.  Scratch (one scan
   element per 2,048 rows) comes from the context's pool and counts against gpuq_memory_limit.  Asynchronous on `stream`. */
int gpuq_segment_distinct(gpuq_ctx* ctx, void* stream, const gpuq_column* value_col, const int32_t* starts, int64_t n_groups, int64_t n_rows, int64_t* out_count, void* out_sum,
                          int sum_width, void* out_xor, int xor_width, uint8_t* out_validity);

/* Grouping sets: GROUP BY ROLLUP / CUBE / GROUPING SETS (AggregateExecNode.groups and .null_expr, datafusion.proto:1437-1450; the rules
   are DataFusion 34's [UPSTREAM-KNOWLEDGE: physical-plan aggregates/mod.rs PhysicalGroupBy, evaluate_group_by; the crate is not in the
   reference tree]).  The "aggregate" descriptor knows no sets; the native plan executor lowers an AggregateExec that carries them.
     meaning    "groups" is S grouping sets, one bool per group expression: true = the key is NULL in that set (a NULL of the key's type;
                null_expr is checked for its length and not evaluated).  Every input row that passes the fused predicate is counted once
                per set, with NULL wherever the set masks a key, and all tuples of all sets go into ONE table.  This version has no
                grouping id, so -- as in DataFusion 34 --
                  * a row whose key is really NULL lands in the same group as the set that masks that key, and
                  * two equal sets count every row twice.
                An empty set () gives the grand-total row; no input rows give no output rows (the node is grouped).  Output key field k
                is nullable when its expression is, or when any set masks it.  The GROUPING() function has no physical plan there, or here.
     lowering   the input is aggregated once, at the finest grain, and the sets are made from the state table:
                  Single :  Final ( Expand ( Partial[all group_expr]( input ) ) )
                  Partial:  Merge ( Expand ( Partial[all group_expr]( input ) ) )
                The inner Partial keeps the node's group_expr, aggr_expr (with filter), strategy, expected_groups, output_capacity and its
                fusion with the filters / projections below; Expand is the entry point below over every column (state columns unmasked);
                the outer node groups by the key columns by name and reads states by position.  A Partial with sets therefore emits one row
                per key tuple of each set, not the finest set's rows S times.  The expansion settles a deferred execution first.
     accepted   no "groups", or one all-false set: the plain node, untouched.  Modes Partial and Single (a Final's group-by is plain).
   Refused: GPUQ_ERR_INVALID -- a set of the wrong length, "groups" with no group expressions, an empty "groups" list, null_expr of the
   wrong length, sets on Final / FinalPartitioned; GPUQ_ERR_UNSUPPORTED -- more than 64 sets, sets beside MEDIAN, APPROX_DISTINCT or any
   `distinct` aggregate, and (GPUQ_REFUSAL_LONG_STRING) "grouping sets: group key '<name>' holds strings longer than 15 bytes".

   gpuq_grouping_expand: rows [0, n) of `col`, n_sets times over, row-interleaved: output row i * n_sets + s is input row i, and it is
   NULL when bit s of null_sets is set (or row i is NULL; col->validity == NULL: every row is valid).  No output position depends on n.
   Types of width 1 / 2 / 4 / 8 / 16 bytes (Utf8 as PACKED15: 16) and Boolean, whose data is a bitmap: out_data holds n * n_sets values,
   or that many bits in whole 64-bit words.  A NULL row's data is zero.  out_validity: whole 64-bit words (8-byte aligned), the last one
   zero-padded; it may be NULL only when null_sets == 0 and the input has no validity.  State columns pass null_sets = 0.  One lane per
   output row, no scratch, no atomics; asynchronous on `stream`.  Refused (GPUQ_ERR_UNSUPPORTED, GPUQ_REFUSAL_NONE, "gpuq_grouping_expand
   (AggregateExec grouping sets): ..."): n_sets outside 1..64; n * n_sets >= 2^31 (checked before any pointer is looked at); a Utf8
   column in Arrow layout. */
int gpuq_grouping_expand(gpuq_ctx* ctx, void* stream, const gpuq_column* col, int64_t n, int n_sets, uint64_t null_sets, void* out_data, uint8_t* out_validity);

/* Window functions over an ordered table (WindowAggExecNode with partition_search_mode set, datafusion.proto:1417-1427: DataFusion's
   BoundedWindowAggExec; window expressions :1198-1209, frames :780-799).  The native plan executor's BoundedWindowAggExec node (grammar
   and rules with the plan nodes below) runs on these four entry points over a table that is ordered by (partition_by, order_by):
   gpuq_segment_heads gives the partitions (part_id / part_starts) and the peer groups (peer_id / peer_starts: the heads over
   partition_by + order_by), each `starts` array one entry longer than its number of segments.  n >= 2^31 is GPUQ_ERR_UNSUPPORTED.
   All asynchronous on `stream`; scratch comes from the context's pool and counts against gpuq_memory_limit.

   gpuq_window_scan: the running SUM / COUNT / MIN / MAX (fn) of `value_col` (Arrow layout, any fixed-width numeric or temporal type)
   inside every partition (seg_id = part_id, or NULL: one partition): a segmented inclusive scan of one accumulator cell of the
   aggregate operator -- SUM of integers and decimals in 128 bits (cell_width 16; cell_width 8 keeps the low word: Int64 / UInt64
   wrapping), SUM of floats in Float64 (Float32 widened), MIN / MAX of integers, temporals and decimals in 64 bits, of floats by total
   order as a Float64 -- in three launches (tile totals, one block over them, a downsweep), in a fixed order of combination.
   out_cells: n cells of cell_width bytes; out_count (n x int64, or NULL): the non-NULL values so far; out_validity ((n + 63) / 64 * 8
   bytes, 8-byte aligned, or NULL): bit = count > 0, written as whole words.  status_dev (device u32, zeroed by the caller, or NULL): bit
   0 is set when a MIN / MAX operand lies outside int64 (a Decimal128 or UInt64 beyond it: what the aggregate operator refuses too).
   gpuq_window_rank: row_number = i - part_start + 1, rank = peer_start - part_start + 1, dense_rank = peer_id - peer_id(part_start) + 1,
   each n x uint64 or NULL.
   gpuq_window_shift (LAG: delta = -offset, LEAD: delta = +offset): out[i] = value[i + delta] with its validity when row i + delta lies in
   row i's partition, else default_col[i] (a column of value_col's type; NULL: the default is NULL).  Utf8 and Boolean are refused.
   gpuq_window_frame: the frames the scan does not give directly, and the results that are not a cell.  With P the running cells (and C
   the counts, or NULL: the result is never NULL) the value of row i is P[hi] - P[lo - 1], P[part_start - 1] = 0, wrapping:
     GPUQ_FRAME_ROWS     lo = part_start, hi = i                      GPUQ_FRAME_RANGE    lo = part_start, hi = peer_end(i) - 1
     GPUQ_FRAME_SLIDING  lo = max(part_start, i - preceding) (preceding < 0: UNBOUNDED), hi = min(part_end - 1, i + following)
   (a difference is only right for SUM / COUNT cells of integers and decimals).  out_kind: the cell in out_width bytes (truncated, an
   8-byte cell sign-extended to 16; out_f32: the Float64 cell stored as a Float32) | AVG of a 16-byte integer sum: one conversion to
   Float64, one division | AVG of a Float64 sum | AVG of a 16-byte decimal sum: sum * 10^avg_scale_digits / count, truncating.
   out_validity: bit = count > 0, whole words. */
enum { GPUQ_WINDOW_SUM = 0, GPUQ_WINDOW_COUNT = 1, GPUQ_WINDOW_MIN = 2, GPUQ_WINDOW_MAX = 3 };
enum { GPUQ_FRAME_ROWS = 0, GPUQ_FRAME_RANGE = 1, GPUQ_FRAME_SLIDING = 2 };
enum { GPUQ_WINDOW_OUT_CELL = 0, GPUQ_WINDOW_OUT_AVG_INT = 1, GPUQ_WINDOW_OUT_AVG_FLOAT = 2, GPUQ_WINDOW_OUT_AVG_DECIMAL = 3 };
typedef struct gpuq_window_frame_spec {
  const void* cells; const int64_t* counts; int32_t cell_width;
  int32_t mode; int64_t preceding, following;
  const int32_t *part_id, *part_starts, *peer_id, *peer_starts;
  int32_t out_kind, out_width, out_f32, avg_scale_digits;
  void* out; uint8_t* out_validity;
} gpuq_window_frame_spec;
int gpuq_window_scan(gpuq_ctx* ctx, void* stream, const gpuq_column* value_col, const int32_t* seg_id, int64_t n, int fn, void* out_cells, int cell_width, int64_t* out_count,
                     uint8_t* out_validity, uint32_t* status_dev);
int gpuq_window_rank(gpuq_ctx* ctx, void* stream, const int32_t* part_id, const int32_t* part_starts, const int32_t* peer_id, const int32_t* peer_starts, int64_t n,
                     uint64_t* row_number_out, uint64_t* rank_out, uint64_t* dense_rank_out);
int gpuq_window_shift(gpuq_ctx* ctx, void* stream, const gpuq_column* value_col, const int32_t* part_id, const int32_t* part_starts, int64_t n, int64_t delta,
                      const gpuq_column* default_col, void* out_data, uint8_t* out_validity);
int gpuq_window_frame(gpuq_ctx* ctx, void* stream, const gpuq_window_frame_spec* f, int64_t n);

/* dst[i] = src[i] + delta for n Utf8 offsets: joining the offset arrays of partitions that are concatenated (fan-in). */
int gpuq_offsets_rebase(gpuq_ctx* ctx, void* stream, const int32_t* src, int64_t n, int32_t delta, int32_t* dst);

/* Utf8 PACKED15 -> Arrow offsets+bytes.  offsets_out: n+1 int32; data_out capacity data_cap bytes.
   Synchronous; *data_len_out (host) = bytes written. */
int gpuq_unpack_utf8(gpuq_ctx* ctx, void* stream, const void* packed, int64_t n, int32_t* offsets_out, uint8_t* data_out,
                     int64_t data_cap, int64_t* data_len_out);

/* Bitmap concatenation for CoalesceTasksExec / CoalescePartitionsExec / UnionExec fan-in (coalesce_tasks.rs:130-229:
   P partition streams -> 1): dst bits [dst_bit_offset, +n_bits) |= src bits [0, n_bits); src == NULL appends ones
   (a piece without a validity buffer).  dst (8-byte aligned, padded to a multiple of 8 bytes) must be zeroed first.
   Fixed-width data buffers are concatenated with plain device copies.  Asynchronous on `stream`. */
int gpuq_concat_bitmap(gpuq_ctx* ctx, void* stream, uint8_t* dst, int64_t dst_bit_offset, const uint8_t* src, int64_t n_bits);
/* Same with a source bit offset: dst bits [dst_bit_offset, +n_bits) |= src bits [src_bit_offset, +n_bits).  Row ranges of a
   bitmap (GlobalLimitExec skip, datafusion.proto:1453-1458). */
int gpuq_copy_bits(gpuq_ctx* ctx, void* stream, uint8_t* dst, int64_t dst_bit_offset, const uint8_t* src, int64_t src_bit_offset, int64_t n_bits);

/* ---- native plan executor ------------------------------------------------------------------
   The C++ host side above the operator calls: executes a physical plan tree, keeping data on the device between operators
   (fused Filter -> Projection -> consumer chains, index-vector views, pooled allocations).  Stands in for the walk an
   ExecutionEngine makes over the stage plan (ballista/executor/src/execution_engine.rs:34-60; `plan.execute(0, ctx)` at
   ballista/core/src/execution_plans/shuffle_writer.rs:255).  plan_json mirrors the PhysicalPlanNode messages of
   ballista/core/proto/datafusion.proto, one key per node:
     {"MemoryExec": {"schema": [{"name","type","nullable"}], "partitions": [input_slot, ...], "dense"?: bool, "sides"?: [..]}}
     {"FilterExec": {"input": node, "expr": expr}}                                   (:1291-1294)
     {"ProjectionExec": {"input": node, "expr": [expr], "expr_name": [str]}}         (:1399-1403)
     {"AggregateExec": {"input", "mode", "group_expr": [{"expr","name"}], "aggr_expr": [{"fn","expr","expr2"?,"name"}],
                        "strategy"?, "expected_groups"?, "output_capacity"?,
                        "groups"?: [[bool x len(group_expr)] x S], "null_expr"?: [expr]}}    (:1405-1450)
         groups / null_expr: grouping sets (ROLLUP / CUBE / GROUPING SETS), modes Single and Partial; see gpuq_grouping_expand
         fn: the operator's functions, and -- mode Single, this executor only -- MEDIAN ("expr", "filter"?; see gpuq_segment_median)
             and APPROX_DISTINCT ("expr", "filter"?; see gpuq_segment_approx_distinct)
             "distinct"?: true on COUNT / SUM / BIT_XOR / MIN / MAX / BIT_AND / BIT_OR / BOOL_AND / BOOL_OR ("filter"? allowed), beside plain
             aggregates and over several arguments -- mode Single; see gpuq_segment_distinct
     {"HashJoinExec": {"left", "right", "on": [{"left": expr, "right": expr}], "join_type", "partition_mode",
                       "null_equals_null", "filter"?}}                               (:1346-1360)
     {"SortExec" | "SortPreservingMergeExec": {"input", "expr": [{"expr","asc","nulls_first"}], "fetch"?}}   (:1465-1478)
     {"BoundedWindowAggExec": {"input": node,
        "window_expr": [{"fn": name, "args": [expr], "partition_by": [expr], "order_by": [{"expr","asc","nulls_first"}],
                         "window_frame"?: {"units": "ROWS" | "RANGE",
                                           "start_bound": {"type": "PRECEDING" | "CURRENT_ROW" | "FOLLOWING", "value": null | int},
                                           "end_bound":   {...}},
                         "name": str}],
        "partition_keys"?: [expr], "partition_search_mode": "Sorted"}}                (:1198-1209, :780-799, :1417-1427)
         WindowAggExecNode with partition_search_mode set: the node DataFusion plans when every window expression has a bounded frame.
         Output: the input's fields, then one per window expression; rows keep the input's order, partitions are the input's.
         Ordering: as in DataFusion the node does not sort and does not check.  Mode Sorted promises input ordered by (partition_by,
         order_by) -- EnforceSorting puts a SortExec below.  A partition is a maximal run of adjacent rows equal on every partition_by
         column, a peer group a maximal run equal on partition_by + order_by; equality is gpuq_segment_heads's (validity first, NULL
         equals NULL, then bytes).  No partition_by: one partition; no order_by: every row of a partition is a peer.
         Functions (names without regard to case):
           ROW_NUMBER, RANK, DENSE_RANK   no arguments; UInt64, not nullable
           LAG, LEAD      x [, offset literal >= 0, default 1 [, default literal or NULL]]; x's type, nullable.  The value `offset` rows
                          before / after in the same partition, NULLs included (a NULL x is a value); outside the partition the default.
                          Every fixed-width type; Utf8 and Boolean are refused by name.
           COUNT          x (any type); Int64, not nullable: the non-NULL x in the frame
           SUM, MIN, MAX, AVG   x; the type the aggregate operator's function of the same name gives in mode Single, nullable: NULL while
                          the frame holds no non-NULL x.  The accumulators are that operator's (integer SUM wraps at 64 bits, Decimal128 SUM
                          at 128, Float32 sums in Float64, float MIN / MAX by total order; a MIN / MAX operand outside int64 is refused at
                          run time, the function named), with one difference: AVG of an integer keeps the exact 128-bit sum and rounds
                          twice (its conversion to Float64, the division), so that a frame can be a difference of two running sums.
         Frames of COUNT / SUM / MIN / MAX / AVG (the other functions ignore theirs); none: RANGE UNBOUNDED PRECEDING .. CURRENT ROW:
           ROWS  UNBOUNDED PRECEDING .. CURRENT ROW     the rows of the partition up to and including this one
           RANGE UNBOUNDED PRECEDING .. CURRENT ROW     ... up to and including the row's last peer
           ROWS  k PRECEDING .. CURRENT ROW | m FOLLOWING (k may be UNBOUNDED; k, m literals; clipped to the partition): SUM / COUNT / AVG
                 over integer and Decimal128 arguments -- a difference of two running values, exact in wrapping arithmetic
         GPUQ_ERR_UNSUPPORTED (GPUQ_REFUSAL_NONE; the message names the function and the frame, the mode or the column): an end bound of
         UNBOUNDED FOLLOWING or PRECEDING, a start bound of FOLLOWING; RANGE with a numeric offset; GROUPS; sliding frames for MIN / MAX (a
         running extreme cannot be taken back) and for any Float32 / Float64 argument (a difference of prefix sums cancels, and
         DataFusion's retracting sum rounds differently again); partition_search_mode Linear / PartiallySorted; window expressions of one
         node that differ in partition_by or order_by; Float32 / Float64 partition_by columns (bytewise heads: -0.0 and the NaNs);
         partition_by / order_by strings beyond 15 bytes; FIRST_VALUE / LAST_VALUE / NTH_VALUE and every other function; 2^31 rows or
         more in a partition of the plan.  A frame value that is not a whole number >= 0 or a negative offset is GPUQ_ERR_INVALID.
         "WindowAggExec", the unbounded-frame node (PERCENT_RANK, CUME_DIST, NTILE, SUM() OVER (PARTITION BY k)), stays
         GPUQ_REFUSAL_NODE_NOT_NATIVE.  The node runs synchronously (it needs an exact row count); see gpuq_window_scan for its kernels.
     {"CoalesceBatchesExec": {"input"}}  {"LocalLimitExec": {"input","fetch"}}       (:1487-1490, :1460-1463)
     {"GlobalLimitExec": {"input","skip","fetch"}}  {"UnionExec": {"inputs": [node]}}  {"CoalescePartitionsExec": {"input"}}   (:1453, :1319, :1492)
     {"CoalesceTasksExec": {"input","partitions": [p],"order_by"?: [sort expr]}}     (ballista coalesce_tasks.rs:46-70)
     {"ShuffleWriterExec": {"input","job_id","stage_id","work_dir","output_partitioning"?: {"hash_expr": [expr], "partition_count": n},
                            "batch_rows"?: rows per RecordBatch, default 2^20,
                            "partitions"?: [stage partitions of this task, shuffle_writer.rs:118-119: echoed by gpuq_plan_metrics
                                            for ShuffleWritePartition.partitions, the CoalesceTasksExec child does the work]}}
                                                                                   (ballista shuffle_writer.rs:234-456: the stage root)
         writes <work_dir>/<job_id>/<stage_id>/<q>/<uuid>.arrow per non-empty output partition q (unpartitioned:
         .../<stage_id>/<uuid>/data.arrow), Arrow IPC stream + LZ4_FRAME; result = one row per file:
         partition UInt32, path Utf8, num_rows / num_batches / num_bytes UInt64 (shuffle_writer.rs:470-520)
     {"RepartitionExec": {"input","hash_expr": [expr],"partition_count": ranks}}  {"BroadcastExec": {"input"}}
         the exchange between the GPUs of one node (gpuq_plan_set_comm; "exchange" section below): the stand-ins for a stage
         boundary of the reference -- RepartitionExec(Hash) is where planner.rs:137-151 splits stages; BroadcastExec is a
         CollectLeft build side read by every reduce task
     {"ShuffleReaderExec": {"schema": [{"name","type","nullable"}], "partition": [[{"path"} | path, ...], ...]}}   (shuffle_reader.rs:149-177;
         local files; a file that cannot be opened is reported as "FetchFailed: ...")
     {"ParquetExec": {"file_groups": [[{"path": str, "range"?: [start, end]} | path, ...], ...], "schema": [field],   -- the FILE schema
                      "projection"?: [index into schema], "limit"?: n, "predicate"?: expr over schema, "pruning"?: bool = true}}
     {"CsvExec":     {"file_groups": ..., "schema": [field], "projection"?: ..., "limit"?: n,
                      "has_header": bool, "delimiter": one byte, "quote"?: one byte}}
         (ParquetScanExecNode / CsvScanExecNode over FileScanExecConf, datafusion.proto.)  The leaves of plans over registered files.
         Output partition p = the files of file group p in the order given, concatenated as ShuffleReaderExec concatenates its
         locations; an empty group is an empty table.  The output schema is the projected fields, in projection order.  Files are
         mapped read-only (only what a decoder uploads is read from disk) and read again on every execution; a file that cannot be
         opened or mapped is an error naming the path and strerror.  "limit": at most n rows per partition -- the first in file order,
         after pruning -- and no further row group or file is decoded once they are there.
         ParquetExec: per file the row groups of its byte range that the predicate may be true in (gpuq_parquet_prune; "pruning": false
         applies the range only) are decoded by gpuq_parquet_decode_groups, projected by name; a projected column whose type in the file
         differs from the declared one is refused, both types named.  The predicate is NOT applied to rows: the FilterExec above does that.
         CsvExec: gpuq_csv_decode over the file's bytes, or over the lines of the range: a line belongs to the range in which its first
         byte lies, the header line is skipped only by the range that holds offset 0, so ranges that tile the file yield every line
         once.  More than one call's 4 GiB is cut at line boundaries.  What the decoder refuses stays refused, status and message.
         "table_partition_cols", "output_ordering" (non-empty) and a CSV "escape" are GPUQ_REFUSAL_NODE_NOT_NATIVE: such a scan stays
         a host leaf.  Any other unknown member is GPUQ_ERR_INVALID and named.
         gpuq_plan_metrics adds to a scan leaf: "row_groups" (in range), "row_groups_pruned", "bytes_scanned" (chunk / text bytes
         uploaded), "files".
   Expressions are the PhysicalExprNode mirror of gpuq_op_create; columns are resolved by NAME against each operator's input.
   gpuq_plan_execute runs one output partition: inputs[k] is the table MemoryExec leaves refer to as slot k (caller-owned device
   memory, must stay valid until the call returns); *out is a materialised result owned by the library (gpuq_result_free).
   Synchronous.  Errors: status code + gpuq_plan_last_error(). */
typedef struct gpuq_plan gpuq_plan;
typedef struct gpuq_result gpuq_result;
int gpuq_plan_create(gpuq_ctx* ctx, const char* plan_json, gpuq_plan** out);
void gpuq_plan_free(gpuq_plan* plan);
int gpuq_plan_num_partitions(gpuq_plan* plan);
/* The plan's output schema BEFORE anything runs -- QueryStageExecutor::schema() (execution_engine.rs:59), which the executor
   reads to parse the stage's output partitioning ahead of execution (executor_server.rs:530-534).  Host only (no device work):
   expressions are typed by the same compiler that builds the operators.  Size query with fields_out == NULL && cap == 0;
   GPUQ_ERR_CAPACITY when cap is too small (*n_out set). */
int gpuq_plan_schema(gpuq_plan* plan, gpuq_field_info* fields_out, int cap, int* n_out);
int gpuq_plan_execute(gpuq_plan* plan, void* stream, int partition, const gpuq_input* inputs, int n_inputs, gpuq_result** out);
/* Asynchronous execution and cancellation.  The reference runs a task as a future on its task-runner pool and cancels it by
   dropping that future (ballista/executor/src/executor.rs:201-240; whatever holds resources cleans up in Drop).  Here
   gpuq_plan_execute_async starts the plan on a worker thread (same semantics as gpuq_plan_execute; the gpuq_input / gpuq_column
   arrays are copied, the device buffers they point to must stay valid until the task is done) and returns at once;
   gpuq_task_wait blocks and hands over the result (or the error: GPUQ_ERR_CANCELLED after a cancel that came in time);
   gpuq_task_cancel raises a flag the executor checks between operator calls -- the worker then drains `stream` and returns every
   pooled buffer it held, so the plan, the stream and the context are immediately usable again; gpuq_task_free on a running task
   cancels and joins it (the Drop of the Rust wrapper).  One task per plan at a time. */
typedef struct gpuq_task gpuq_task;
int gpuq_plan_execute_async(gpuq_plan* plan, void* stream, int partition, const gpuq_input* inputs, int n_inputs, gpuq_task** out);
int gpuq_task_poll(gpuq_task* task, int* done_out);
int gpuq_task_cancel(gpuq_task* task);
int gpuq_task_wait(gpuq_task* task, gpuq_result** out);
void gpuq_task_free(gpuq_task* task);
/* The ranks of the node for RepartitionExec / BroadcastExec nodes (the comm outlives the plan; NULL detaches). */
struct gpuq_comm;
int gpuq_plan_set_comm(gpuq_plan* plan, struct gpuq_comm* comm);
/* How the plan's last execution went: *deferred_out = 1 when it ran deferred (see "Deferred execution" above: from a plan's second
   execution on, env GPUQ_DEFER=0 switches it off) and held; *settles_out = host round trips that settled deferred operators (1 for
   a single-GPU plan without files); *host_syncs_out = count / status read-backs of the operators that ran synchronously;
   *retries_out = deferred executions of this plan that had to be redone synchronously so far.  Any pointer may be NULL. */
int gpuq_plan_exec_stats(gpuq_plan* plan, int* deferred_out, int* settles_out, int* host_syncs_out, int* retries_out);
int gpuq_plan_metrics(gpuq_plan* plan, char* json_out, size_t cap);     /* per node: output_rows, elapsed_compute (ns) -- utils.rs:470-481; ShuffleWriterExec adds write_time, repart_time, input_rows (shuffle_writer.rs:139-160) */
const char* gpuq_plan_last_error(void);
/* gpuq_op_profile over every operator the plan has compiled: enable/disable the HIP-event bracket around each operator's
   dominant kernel and report the operator with the most accumulated kernel time (its descriptor text in op_desc_out). */
int gpuq_plan_profile(gpuq_plan* plan, int enable, float* kernel_ms_out, int* launches_out, char* op_desc_out, size_t cap);
/* Every operator the plan has compiled, as a JSON array [{"op": kind, "kernel_ms": accumulated ms, "launches": n, "desc": descriptor}]
   (an aggregate also "agg_path": gpuq_op_agg_path)
   (reads and resets the accumulators; profiling stays as it was set by gpuq_plan_profile).  GPUQ_ERR_CAPACITY when cap is too small. */
int gpuq_plan_profile_all(gpuq_plan* plan, char* json_out, size_t cap);
int64_t gpuq_result_num_rows(const gpuq_result* r);
int gpuq_result_num_columns(const gpuq_result* r);
int gpuq_result_column(const gpuq_result* r, int i, gpuq_column* col_out, gpuq_field_info* field_out);
void gpuq_result_free(gpuq_result* r);
/* When all columns of the result live in ONE device allocation of the fixed "record" layout (an aggregate's output: 256-byte
   header, then per column data and validity, 256-byte aligned, for *cap_out rows), returns it: such a result can be shipped
   between GPUs as it lies.  *base_out = NULL otherwise. */
int gpuq_result_record(const gpuq_result* r, void** base_out, size_t* bytes_out, int64_t* cap_out);

/* ---- shuffle codec: Arrow IPC stream messages with LZ4_FRAME buffers, device side -------------------
   Stands in for the reference's shuffle sink and source: `StreamWriter::try_new_with_options(.., LZ4_FRAME)` + `write(&batch)`
   (ballista/core/src/execution_plans/shuffle_writer.rs:365-378, ballista/core/src/utils.rs:179-219) and the IPC stream reader
   behind ShuffleReaderExec / the Flight client (ballista/core/src/execution_plans/shuffle_reader.rs, ballista/core/src/client.rs).
   A shuffle file is: the Schema message (the caller's Arrow library serialises it -- arrow-rs `IpcDataGenerator::schema_to_bytes`,
   pyarrow `Schema.serialize()`), RecordBatch messages, then the end-of-stream marker FF FF FF FF 00 00 00 00.  These entry points
   encode / decode ONE encapsulated RecordBatch message; the buffers are (de)compressed on the device (one wave per 64 KiB block),
   the host only frames.  Frames are written with independent 64 KiB blocks, no checksums (what lz4_flex writes for arrow-ipc);
   frames with linked blocks (Arrow C++), stored blocks, block checksums and content size are read.  ZSTD is GPUQ_ERR_UNSUPPORTED.
   Errors: status code + gpuq_ipc_last_error(). */
typedef struct gpuq_ipc_info {
  int32_t header_type;     /* Message.fbs MessageHeader: 1 Schema, 2 DictionaryBatch, 3 RecordBatch; 0 = end-of-stream marker */
  int32_t codec;           /* -1 none, 0 LZ4_FRAME, 1 ZSTD */
  int64_t metadata_bytes;  /* from the start of the message to the start of its body (8 + flatbuffer incl. padding) */
  int64_t body_bytes;
  int64_t n_rows;
  int32_t n_nodes, n_buffers;
} gpuq_ipc_info;
typedef struct gpuq_ipc_batch gpuq_ipc_batch;
/* Host only: parses the message that starts at `bytes`.  GPUQ_ERR_CAPACITY when `avail` does not cover the metadata yet
   (out->metadata_bytes is set once the first 8 bytes are there). */
int gpuq_ipc_peek(const uint8_t* bytes, int64_t avail, gpuq_ipc_info* out);
/* Host only: the encapsulated Schema message that opens a stream of these fields (name, type, precision, scale, nullable are
   read) -- what `IpcDataGenerator::schema_to_bytes` / `Schema.serialize()` produce.  Size query with out == NULL && cap == 0. */
int gpuq_ipc_schema_message(const gpuq_field_info* fields, int n_cols, uint8_t* out, int64_t cap, int64_t* len_out);
/* Host only: the same with Schema.custom_metadata key / value pairs (what arrow-rs writes for `Schema::metadata`). */
int gpuq_ipc_schema_message_kv(const gpuq_field_info* fields, int n_cols, const char* const* keys, const char* const* values, int n_kv, uint8_t* out, int64_t cap,
                               int64_t* len_out);
/* Host only: looks `key` up in the custom_metadata of the Schema message that starts at `bytes`; *found_out = 0 / 1. */
int gpuq_ipc_schema_metadata(const uint8_t* bytes, int64_t avail, const char* key, char* value_out, size_t cap, int* found_out);
/* The partition function of a hash-partitioned shuffle file written by this engine, recorded as schema metadata
   "gpuq.partition_fn" (files written by DataFusion's BatchPartitioner -- fixed-seed ahash -- carry no such key).  Equal keys only
   meet in one output partition when EVERY map task of a stage used the same function: ShuffleReaderExec refuses a partition
   whose files disagree (all map tasks of a hash-partitioned stage must run on the same engine). */
#define GPUQ_PARTITION_FN_KEY "gpuq.partition_fn"
#define GPUQ_PARTITION_FN "gpuq-mix64-v1"
/* cols: device columns in GPUQ_REPR_ARROW layout, all of n_rows rows.  codec: 0 = LZ4_FRAME, -1 = uncompressed.  Writes the
   message to out_host (host memory, cap bytes) and its length to *len_out.  out_host == NULL && cap == 0: size query (the
   compression runs, nothing is copied).  GPUQ_ERR_CAPACITY (with *len_out set) when cap is too small.  Synchronous. */
int gpuq_ipc_encode_batch(gpuq_ctx* ctx, void* stream, const gpuq_column* cols, int n_cols, int64_t n_rows, int codec, uint8_t* out_host, int64_t cap,
                          int64_t* len_out);
/* msg: one whole encapsulated RecordBatch message in host memory; fields: the stream's schema (type / precision / scale are
   read).  The decoded columns live in device memory owned by *out (gpuq_ipc_batch_free).  Synchronous. */
int gpuq_ipc_decode_batch(gpuq_ctx* ctx, void* stream, const uint8_t* msg, int64_t msg_bytes, const gpuq_field_info* fields, int n_cols, gpuq_ipc_batch** out);
/* The same for a whole byte range of encapsulated messages (a shuffle file after -- or including -- its Schema message, up to
   the end-of-stream marker or n_bytes): every RecordBatch is decoded in ONE launch (a unit of work per LZ4 block of every
   buffer of every batch) straight into the concatenated columns.  This is the call for files written with the reference's
   8192-row batches, whose buffers hold one or two blocks each. */
int gpuq_ipc_decode_stream(gpuq_ctx* ctx, void* stream, const uint8_t* bytes, int64_t n_bytes, const gpuq_field_info* fields, int n_cols, gpuq_ipc_batch** out);
int64_t gpuq_ipc_batch_num_rows(const gpuq_ipc_batch* b);
int gpuq_ipc_batch_num_columns(const gpuq_ipc_batch* b);
int gpuq_ipc_batch_column(const gpuq_ipc_batch* b, int i, gpuq_column* col_out);
void gpuq_ipc_batch_free(gpuq_ipc_batch* b);
const char* gpuq_ipc_last_error(void);

/* ---- exchange between the GPUs of one node ---------------------------------------------------------
   Stands in for a stage boundary of the reference between executors that each own one GPU of a node: ShuffleWriterExec
   hash-partitioning into Arrow-IPC files (ballista/core/src/execution_plans/shuffle_writer.rs:328-392) that the next stage's
   ShuffleReaderExec fetches (shuffle_reader.rs:226-298).  Here it is one exchange step: an all-to-all of per-destination counts,
   then one variable-size all-to-all per column buffer, posted as grouped RCCL sends / receives so that all xGMI links of a GPU
   carry traffic at once; nothing is compressed or written to disk.  One process per GPU; every rank makes the same calls in
   the same order (they are collectives).  Errors: status code + gpuq_exchange_last_error(). */
typedef struct gpuq_comm gpuq_comm;
#define GPUQ_COMM_ID_BYTES 128
/* Rank 0 creates the id; the host hands it to the other ranks over its own channel (the executors' gRPC, a torch.distributed
   store, a file), then every rank calls gpuq_comm_create (collective: ncclCommInitRank on the context's device). */
int gpuq_comm_unique_id(uint8_t* id_out /* GPUQ_COMM_ID_BYTES */);
int gpuq_comm_create(gpuq_ctx* ctx, const uint8_t* id /* GPUQ_COMM_ID_BYTES */, int rank, int world, gpuq_comm** out);
/* Host-staged transport instead of RCCL: the library stages every buffer through pinned host memory and the caller moves the
   bytes (tests with several ranks on one GPU; a host that ships bytes over its own network service).  all_to_all_v: this rank
   sends send_counts[d] bytes to rank d from `send` (host memory, packed in rank order) and receives recv_counts[s] bytes from
   rank s into `recv` (packed in rank order); returns 0 on success.  Collective. */
typedef struct gpuq_transport {
  void* user;
  int (*all_to_all_v)(void* user, const void* send, const int64_t* send_counts, void* recv, const int64_t* recv_counts, int world);
} gpuq_transport;
int gpuq_comm_create_host(gpuq_ctx* ctx, const gpuq_transport* transport, int rank, int world, gpuq_comm** out);
void gpuq_comm_free(gpuq_comm* comm);
/* Failing together.  Every exchange starts with a fixed-size meta round that carries, next to the row counts, a status word per
   rank: 0 fine, 1 "I have failed", 2 "my deferred execution did not hold" (GPUQ_ERR_RETRY on every rank: all of them run again,
   synchronously).  gpuq_comm_set_status arms the word for this rank's NEXT collective call; gpuq_comm_announce is that meta round
   alone (no table): a rank whose plan failed below an exchange calls set_status(1) + announce so that the peers waiting in the
   exchange return GPUQ_ERR_PEER instead of hanging, and with status 0 everywhere it is the barrier that closes a deferred execution
   ("nobody has to redo anything").  A second, one-word round agrees on limits the counts imply (2^32 rows / 2 GiB of strings on a
   rank) before any payload moves; a failure inside the payload round aborts the communicator (ncclCommAbort).  Collective. */
/* The rows an exchanged table received from rank 0, 1, ... (it holds them in this order): the run boundaries of an ordered fan-in
   (gpuq_merge_run) after a range exchange.  n_out = number of ranks; rows_out may be NULL to ask for it. */
int gpuq_table_piece_rows(const gpuq_table* t, int64_t* rows_out, int cap, int* n_out);
int gpuq_comm_set_status(gpuq_comm* comm, int status);
int gpuq_comm_announce(gpuq_comm* comm, void* stream);
int gpuq_comm_rank(const gpuq_comm* comm);
int gpuq_comm_world(const gpuq_comm* comm);
/* Hash-repartition exchange.  cols / fields: device columns (Arrow layout, Utf8 of any length included, or PACKED15) whose rows
   are GROUPED BY DESTINATION: rows [dest_offsets[d], dest_offsets[d+1]) go to rank d (host array of world+1 entries; produce
   the grouping with gpuq_partition_run(partition_count = world) + a take, as the native executor's RepartitionExec does).
   *out = the rows every rank sent here, concatenated in rank order, in buffers the library owns (gpuq_table_free).
   fields[i].nullable decides whether a validity bitmap travels (the same on every rank).  Synchronous. */
int gpuq_exchange_partitions(gpuq_comm* comm, void* stream, const gpuq_column* cols, const gpuq_field_info* fields, int n_cols, const int64_t* dest_offsets,
                             gpuq_table** out);
/* Every rank receives all ranks' rows, in rank order: CollectLeft build sides (the reference's reduce task reads every partition
   of the build stage), partial-aggregate states. */
int gpuq_allgather_table(gpuq_comm* comm, void* stream, const gpuq_column* cols, const gpuq_field_info* fields, int n_cols, int64_t n_rows, gpuq_table** out);
const char* gpuq_exchange_last_error(void);

/* ---- timing support for bench.py: HIP events on the caller's stream ---------------------- */
typedef struct gpuq_timer gpuq_timer;
int gpuq_timer_create(gpuq_ctx* ctx, gpuq_timer** out);
int gpuq_timer_start(gpuq_timer* t, void* stream);
int gpuq_timer_stop(gpuq_timer* t, void* stream);
int gpuq_timer_elapsed_ms(gpuq_timer* t, float* ms_out); /* synchronises on the stop event */
void gpuq_timer_free(gpuq_timer* t);
/* Per-op device time of the last call(s): the op brackets its dominant kernel with HIP events when
   enabled; returns the accumulated ms and launch count since the last reset.  enable < 0 keeps the current setting. */
int gpuq_op_profile(gpuq_op* op, int enable, float* kernel_ms_out, int* launches_out);
/* ... and of EVERYTHING the op's run calls queued in the interval the last gpuq_op_profile call closed (the dominant kernel plus table
   initialisation, scans, compactions, the result projection): the operator's share of a step. */
int gpuq_op_profile_total(gpuq_op* op, float* total_ms_out);
/* The way an aggregate operator's last run took: "tiny", "table", "radix" or "runs"; "" before its first run and for other operators.
   gpuq_plan_profile_all reports it as "agg_path" next to the descriptor. */
const char* gpuq_op_agg_path(gpuq_op* op);

#ifdef __cplusplus
}
#endif
#endif /* GPUQ_H */
