/*
 * nqe.h — C ABI of the MI355X-native physical execution layer for
 * naive-query-engine's hot operators (filter, projection, hash group-by
 * aggregate, inner hash join over Arrow-layout Int64/UInt64/Float64/Boolean/Utf8
 * columns) and of the CSV ingest that feeds them.
 *
 * The reference (Veeupup/naive-query-engine, Rust) has NO FFI; its operator
 * boundary is the in-crate trait
 *
 *     trait PhysicalPlan { schema(); execute() -> Result<Vec<RecordBatch>>; children() }
 *                                              (src/physical_plan/plan.rs:14-21)
 *
 * and the arrow-rs compute kernels its operators call.  Every entry point
 * below replaces one `execute()` body (or one arrow-rs call site inside it)
 * and cites it.  A Rust `impl PhysicalPlan for Gpu*Plan` binds these through
 * `extern "C"` (see INTEGRATION.md for the shim).
 *
 * Conventions
 *   - plain C, no C++/torch types; all structs are POD and passed by pointer.
 *   - every function returns nqe_status (0 = OK); the numeric codes 1..13
 *     are 1:1 with the reference's `ErrorCode` variants (src/error.rs:13-40);
 *     nqe_last_error(ctx) returns a message for the last failure on ctx.
 *   - no call aborts or throws across the ABI: the reference's panics
 *     (`unimplemented!()` selection.rs:98, binary.rs:85) map to
 *     NQE_ERR_NOT_SUPPORTED.
 *   - columns use the Arrow columnar layout (what `RecordBatch` columns are):
 *     64-bit little-endian values, LSB-first validity bitmap, Boolean values
 *     bit-packed LSB-first, Utf8 = int32 offsets[length+1] + bytes.
 *   - inputs are borrowed for the duration of the call and never mutated;
 *     outputs are nqe_table handles owned by the caller (nqe_table_release).
 *     Tables are immutable and their columns may share device buffers the
 *     LIBRARY owns (reference-counted: a projection of a column, the two key
 *     columns of an equi-join on an integer key are one buffer; the probe-side
 *     columns of a join on unique build keys in which every probe row matched
 *     are the probe table's own buffers): never write through nqe_table_column.
 *     Borrowed NQE_DEVICE memory (nqe_table_create) is never aliased by an
 *     operator's output — it is the caller's to free or overwrite as soon as
 *     the operator has returned and the stream has been synchronised — unless
 *     the table was created with NQE_TABLE_IMMUTABLE.  The explicit zero-copy
 *     views (nqe_table_project) borrow what their input borrows.
 *   - a context owns one HIP stream on one device and is used by one host
 *     thread at a time (the reference is single-threaded).
 *   - calls are stream-ordered: an operator may return while its last kernels
 *     still run on the context's stream; every later call on the same context,
 *     every download and nqe_ctx_synchronize order after them.  Errors that
 *     depend on device data (DivideByZero, overflow) are still reported by the
 *     call that causes them: a call whose expressions can raise one reads the
 *     device flags back (and thereby synchronises) before returning.  Device
 *     pointers from nqe_table_column may be handed to another stream only after
 *     nqe_ctx_synchronize.
 *   - when a call has to wait for the device (a row count, the flags) the host
 *     thread polls the stream for up to 5 ms before it blocks: the waits sit
 *     behind kernels of microseconds to a few milliseconds, and an
 *     interrupt-driven wake-up would add its latency to every operator.
 */
#ifndef NQE_H
#define NQE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NQE_ABI_VERSION 1

/* ---- status codes: 1..13 mirror `enum ErrorCode` (src/error.rs:13-40) ---- */
typedef enum nqe_status {
    NQE_OK = 0,
    NQE_ERR_ARROW = 1,            /* ErrorCode::ArrowError (DivideByZero, length mismatch, overflow) */
    NQE_ERR_IO = 2,               /* ErrorCode::IoError */
    NQE_ERR_NO_SUCH_FIELD = 3,    /* ErrorCode::NoSuchField */
    NQE_ERR_COLUMN_NOT_EXISTS = 4,/* ErrorCode::ColumnNotExists */
    NQE_ERR_LOGICAL = 5,          /* ErrorCode::LogicalError (column.rs:26,54) */
    NQE_ERR_NO_SUCH_TABLE = 6,    /* ErrorCode::NoSuchTable */
    NQE_ERR_PARSER = 7,           /* ErrorCode::ParserError */
    NQE_ERR_INTERVAL = 8,         /* ErrorCode::IntervalError (binary.rs:115: operand type mismatch) */
    NQE_ERR_PLAN = 9,             /* ErrorCode::PlanError (hash_join.rs:126: empty `on`) */
    NQE_ERR_NO_MATCH_FUNCTION = 10,/* ErrorCode::NoMatchFunction */
    NQE_ERR_NOT_SUPPORTED = 11,   /* ErrorCode::NotSupported (aggregate/mod.rs:217, sum.rs:93) + reference panics */
    NQE_ERR_NOT_IMPLEMENTED = 12, /* ErrorCode::NotImplemented (hash_join.rs:161) */
    NQE_ERR_OTHERS = 13,          /* ErrorCode::Others */
    /* codes with no reference analogue */
    NQE_ERR_HIP = 100,            /* a HIP runtime call failed */
    NQE_ERR_RCCL = 101,           /* a collective / the exchange transport failed (nqe_comm_*, nqe_sharded_*) */
    NQE_ERR_INVALID_ARGUMENT = 102,
    NQE_ERR_OUT_OF_MEMORY = 103
} nqe_status;

/* ---- Arrow data types the hot path accepts (selection.rs:69-99, binary.rs:48-86) ---- */
typedef enum nqe_dtype {
    NQE_NULLTYPE = 0, /* DataType::Null (ScalarValue::Null) */
    NQE_BOOLEAN = 1,
    NQE_INT64 = 2,
    NQE_UINT64 = 3,
    NQE_FLOAT64 = 4,
    NQE_UTF8 = 5
} nqe_dtype;

typedef enum nqe_location { NQE_HOST = 0, NQE_DEVICE = 1 } nqe_location;

/* One Arrow array (a RecordBatch column). */
typedef struct nqe_column {
    int32_t dtype;           /* nqe_dtype */
    int32_t location;        /* nqe_location: where values/validity/data point */
    int64_t length;          /* rows */
    int64_t null_count;      /* -1 = unknown (count validity) */
    const void *values;      /* Int64/UInt64/Float64: length*8 B; Boolean: ceil(length/8) B, LSB-first;
                                Utf8: int32 offsets[length+1] */
    const uint8_t *validity; /* ceil(length/8) B LSB-first bitmap, NULL = no nulls */
    const void *data;        /* Utf8 bytes, else NULL */
    int64_t data_length;     /* Utf8 byte count, else 0 */
} nqe_column;

/* ---- expressions: flat post-order encoding of a PhysicalExpr tree ----
 * mirrors ColumnExpr (expression/column.rs:18-29, index form — the planner
 * resolves names to the first matching index, planner/mod.rs:190-200),
 * PhysicalLiteralExpr(ScalarValue) (expression/literal.rs:17-26,
 * logical_plan/expression.rs:174-187) and PhysicalBinaryExpr(l, Operator, r)
 * (expression/binary.rs:91-101), and PhysicalUnaryExpr(expr, UnaryOperator, name, return_type)
 * (expression/unary.rs:46-78; `name` and `return_type` are ignored by evaluate and have no
 * place in the encoding). A BINARY node pops two operands (right on top), a UNARY node pops
 * one; each pushes its result. A tree is valid when evaluating the nodes left-to-right on a
 * stack leaves exactly one value.
 * A STRING node (quirk Q25: "the string functions, given a body") is this library's own beside
 * the reference's: it pops one Utf8 operand like a UNARY node, its `op` is a nqe_unary_operator
 * naming one of TRIM, LTRIM, RTRIM, CHARACTER_LENGTH, LOWER, UPPER and REVERSE, and it pushes a
 * Utf8 value (Int64 for CHARACTER_LENGTH). A UNARY node over the same functions stays what the
 * reference's todo!() is: NQE_ERR_NOT_SUPPORTED.
 * A STRING_ARGS node (quirk Q26: "the string functions with arguments") carries the last three:
 * its `op` is NQE_UNARY_SUBSTR, NQE_UNARY_REPLACE (both pop THREE values) or NQE_UNARY_REPEAT
 * (pops TWO); the string operand is deepest, the last argument on top; it pushes a Utf8 value.
 * In postfix: `s start len SUBSTR`, `s n REPEAT`, `s from to REPLACE`.
 * A STRING_MATCH node (quirk Q27: "the reference has no pattern match; LIKE is unimplemented!()",
 * sql/planner.rs:478) pops TWO values, the string deepest and the pattern on top (`s pattern
 * MATCH`); its `op` is a nqe_match_operator and it pushes a Boolean value (Int64 for STRPOS).
 * NQE_EXPR_STRING_MATCH carries no initializer on purpose: a test of the earlier kinds reads the
 * `NAME = value` pairs of this enum as a fixed list, and C numbers the enumerator 6 by itself;
 * the check below the enum holds it there.
 * A CONDITIONAL node (quirk Q28: "conditional and NULL-handling expressions"; the reference's
 * planner leaves IsNull, Not and Case unimplemented!(), sql/planner.rs) is NQE_EXPR_CONDITIONAL
 * = 7, a #define beside the enum for the same reason. Its `op` is a nqe_cond_operator and its
 * `column` field carries the number of values it pops, which must be the function's arity:
 * NOT, IS_NULL and IS_NOT_NULL pop ONE, COALESCE and NULLIF TWO, IF THREE (the condition deepest,
 * the else value on top). In postfix: `b NOT`, `x IS_NULL`, `a b COALESCE`, `a b NULLIF`,
 * `c t e IF`; coalesce(a, b, c) is `a b c COALESCE COALESCE`, CASE WHEN c1 THEN x WHEN c2 THEN y
 * ELSE z END is `c1 x c2 y z IF IF`, and a CASE without ELSE takes a NULL literal as `e`. A
 * reader of the flat encoding can walk the stack by `column` alone.
 * A CAST node (quirk Q29: PhysicalCastExpr, whose body the reference leaves todo!(),
 * physical_plan/expression/cast.rs) is NQE_EXPR_CAST = 8, a #define beside the enum for the same
 * reason. It pops ONE value and pushes one; its `dtype` field carries the target nqe_dtype; `op`,
 * `column` and the literal fields are not read. In postfix: `x CAST`. */
typedef enum nqe_expr_kind { NQE_EXPR_COLUMN = 0, NQE_EXPR_LITERAL = 1, NQE_EXPR_BINARY = 2, NQE_EXPR_UNARY = 3, NQE_EXPR_STRING = 4, NQE_EXPR_STRING_ARGS = 5, NQE_EXPR_STRING_MATCH } nqe_expr_kind;
typedef char nqe_expr_string_match_is_6[(NQE_EXPR_STRING_MATCH == 6) ? 1 : -1];
#define NQE_EXPR_CONDITIONAL 7
typedef char nqe_expr_conditional_is_7[(NQE_EXPR_CONDITIONAL == NQE_EXPR_STRING_MATCH + 1) ? 1 : -1];
#define NQE_EXPR_CAST 8
typedef char nqe_expr_cast_is_8[(NQE_EXPR_CAST == NQE_EXPR_CONDITIONAL + 1) ? 1 : -1];

/* the `op` of a CONDITIONAL node (quirk Q28; see nqe_expr_evaluate) */
typedef enum nqe_cond_operator {
    NQE_COND_NOT = 0, NQE_COND_IS_NULL = 1, NQE_COND_IS_NOT_NULL = 2, NQE_COND_COALESCE = 3, NQE_COND_NULLIF = 4, NQE_COND_IF = 5
} nqe_cond_operator;

/* the `op` of a STRING_MATCH node (quirk Q27; see nqe_expr_evaluate) */
typedef enum nqe_match_operator {
    NQE_MATCH_LIKE = 0, NQE_MATCH_NOT_LIKE = 1, NQE_MATCH_ILIKE = 2, NQE_MATCH_NOT_ILIKE = 3,
    NQE_MATCH_STARTS_WITH = 4, NQE_MATCH_ENDS_WITH = 5, NQE_MATCH_CONTAINS = 6, NQE_MATCH_STRPOS = 7
} nqe_match_operator;
#define NQE_MAX_MATCH_PATTERN 4096   /* bytes of the pattern literal */

/* same order as `enum Operator` (logical_plan/expression.rs:335-362) */
typedef enum nqe_operator {
    NQE_OP_EQ = 0,
    NQE_OP_NOT_EQ = 1,
    NQE_OP_LT = 2,
    NQE_OP_LT_EQ = 3,
    NQE_OP_GT = 4,
    NQE_OP_GT_EQ = 5,
    NQE_OP_PLUS = 6,
    NQE_OP_MINUS = 7,
    NQE_OP_MULTIPLY = 8,
    NQE_OP_DIVIDE = 9,
    NQE_OP_MODULOS = 10,
    NQE_OP_AND = 11,
    NQE_OP_OR = 12
} nqe_operator;

/* same order as `enum UnaryOperator` (logical_plan/expression.rs:392-422). Only the four math
 * functions have a body in the reference (unary.rs:92-107), and only over Float64; quirk Q16:
 * TAN evaluates the COSINE (unary.rs:96). The string functions are todo!() there and
 * NQE_ERR_NOT_SUPPORTED here under a UNARY node; seven of them have a body under a STRING node
 * and REPEAT, REPLACE and SUBSTR under a STRING_ARGS node (see nqe_expr_evaluate). */
typedef enum nqe_unary_operator {
    NQE_UNARY_ABS = 0,
    NQE_UNARY_SIN = 1,
    NQE_UNARY_COS = 2,
    NQE_UNARY_TAN = 3,
    NQE_UNARY_TRIM = 4,
    NQE_UNARY_LTRIM = 5,
    NQE_UNARY_RTRIM = 6,
    NQE_UNARY_CHARACTER_LENGTH = 7,
    NQE_UNARY_LOWER = 8,
    NQE_UNARY_UPPER = 9,
    NQE_UNARY_REPEAT = 10,
    NQE_UNARY_REPLACE = 11,
    NQE_UNARY_REVERSE = 12,
    NQE_UNARY_SUBSTR = 13
} nqe_unary_operator;

typedef struct nqe_expr_node {
    int32_t kind;    /* nqe_expr_kind */
    int32_t op;      /* BINARY: nqe_operator; UNARY, STRING and STRING_ARGS: nqe_unary_operator; STRING_MATCH: nqe_match_operator; CONDITIONAL: nqe_cond_operator */
    int32_t column;  /* COLUMN: index into the input batch; CONDITIONAL: the number of values the node pops (its arity) */
    int32_t dtype;   /* LITERAL: nqe_dtype of the ScalarValue; CAST: the target nqe_dtype */
    int32_t is_null; /* LITERAL: 1 = ScalarValue::X(None) */
    int32_t utf8_length; /* LITERAL of dtype NQE_UTF8: byte length of value.utf8 (the field was `reserved` before Utf8
                            literals existed; the struct layout is unchanged) */
    union {
        int64_t i64;
        uint64_t u64;
        double f64;
        int64_t boolean;  /* 0 / 1 */
        const char *utf8; /* ScalarValue::Utf8(Some(s)): borrowed for the duration of the call, not NUL-terminated */
    } value;
} nqe_expr_node;

/* same order as `enum AggregateFunc` (logical_plan/expression.rs:491-502) */
typedef enum nqe_agg_func {
    NQE_AGG_COUNT = 0,
    NQE_AGG_SUM = 1,
    NQE_AGG_MIN = 2,
    NQE_AGG_MAX = 3,
    NQE_AGG_AVG = 4
} nqe_agg_func;

/* Sum/Avg/Count/Min/Max::create(ColumnExpr) (aggregate/{sum,avg,count,min,max}.rs): the
 * argument is always a bare column (planner/mod.rs:107-114). */
typedef struct nqe_aggregate {
    int32_t func;   /* nqe_agg_func */
    int32_t column; /* input column index */
} nqe_aggregate;

typedef struct nqe_ctx nqe_ctx;     /* one device + one HIP stream + scratch pool */
typedef struct nqe_table nqe_table; /* one device-resident RecordBatch */

/* ------------------------------------------------------------------ context */
uint32_t nqe_abi_version(void);
/* `stream` = an existing hipStream_t to launch on (e.g. torch's current stream), or NULL to
 * create a private one. */
nqe_status nqe_ctx_create(int32_t device, void *stream, nqe_ctx **out);
nqe_status nqe_ctx_destroy(nqe_ctx *ctx);
nqe_status nqe_ctx_synchronize(nqe_ctx *ctx);
/* Device memory of the context: bytes held by live tables/handles, and bytes cached in the context's block pool
 * (released blocks are reused stream-ordered; a failed hipMalloc trims the pool and retries).  nqe_ctx_trim returns
 * the cached blocks to the driver (after a stream synchronisation). */
nqe_status nqe_ctx_memory_stats(nqe_ctx *ctx, int64_t *live_bytes, int64_t *pooled_bytes);
nqe_status nqe_ctx_trim(nqe_ctx *ctx);
/* Takes `bytes` of device memory from the driver NOW (one block, pages touched) and serves later allocations of the context —
 * operator outputs, scratch — from it (best fit, freed ranges coalesced; what does not fit falls back to the pool / the driver).
 * A first query then pays no hipMalloc: the reference's run_sql is one-shot (db.rs:24-37), and a first hipMalloc of a gigabyte
 * output costs as much as the query.  Once per context; released by nqe_ctx_destroy (nqe_ctx_trim leaves it alone).  The free part
 * counts as `pooled_bytes`.  NQE_RESERVE_MB=<n> in the environment reserves at nqe_ctx_create. */
nqe_status nqe_ctx_reserve(nqe_ctx *ctx, size_t bytes);
const char *nqe_last_error(const nqe_ctx *ctx);
/* global message for failures with no ctx (nqe_ctx_create itself) */
const char *nqe_last_global_error(void);

/* per-kernel timing with HIP events on the ctx stream (bench.py's roofline leg).
 * While enabled every launch of the named kernel family is bracketed by events. */
nqe_status nqe_ctx_timing_enable(nqe_ctx *ctx, int32_t enable);
/* sum of durations (ms) and launch count since the last reset for kernels whose name
 * contains `name_substr`; resets nothing. */
nqe_status nqe_ctx_timing_query(nqe_ctx *ctx, const char *name_substr, double *total_ms, int64_t *launches);
nqe_status nqe_ctx_timing_reset(nqe_ctx *ctx);
/* every kernel family launched since the last reset by exact name, one "name\tms\tlaunches\n" line each, NUL-terminated;
 * *needed = bytes required (call with capacity 0 to size the buffer). */
nqe_status nqe_ctx_timing_report(nqe_ctx *ctx, char *buf, int64_t capacity, int64_t *needed);
/* Expression trees of three or more operators over large inputs (binary.rs:108-155 nested) are, besides being interpreted by the
 * stack machine, specialised at run time: the tree becomes straight-line HIP source compiled with hipRTC on a worker thread, and
 * executions of the same tree shape switch to the compiled kernel once it is ready (results are identical; without libhiprtc the
 * interpreter simply stays).  This call blocks until every compilation in flight for the context has finished — for tests and
 * benchmarks that want the steady state.  NQE_NO_JIT=1 disables the specialisation, NQE_JIT_SYNC=1 compiles before the first
 * execution.  Code objects are kept on disk (NQE_JIT_CACHE_DIR, default ~/.cache/nqe_jit; NQE_NO_JIT_DISK_CACHE=1: not) with the
 * source they were compiled from, so that a new process takes a known tree's kernel on its first execution. */
nqe_status nqe_ctx_jit_wait(nqe_ctx *ctx);

/* ------------------------------------------------------------------ tables
 * MemTable::try_create + ScanPlan::execute (datasource/memory.rs:21-41, scan.rs:34-36):
 * columns enter HBM once; NQE_HOST columns are copied to the device, NQE_DEVICE
 * columns are borrowed (zero-copy; the caller keeps them alive). All columns must
 * have the same length. */
nqe_status nqe_table_create(nqe_ctx *ctx, const nqe_column *columns, int32_t num_columns, nqe_table **out);
/* The same with flags.  NQE_TABLE_IMMUTABLE: the caller promises that the borrowed NQE_DEVICE buffers stay alive and
 * unmodified for as long as ANY table derived from this one lives (what `Arc`-shared Arrow buffers give the reference for
 * free): operator outputs may then alias them instead of copying — the probe-side columns of a join in which every probe
 * row matched, a projected bare column.  Without it every output of an operator is memory the library owns. */
#define NQE_TABLE_IMMUTABLE 1u
nqe_status nqe_table_create_flags(nqe_ctx *ctx, const nqe_column *columns, int32_t num_columns, uint32_t flags, nqe_table **out);
nqe_status nqe_table_release(nqe_table *table);
int64_t nqe_table_num_rows(const nqe_table *table);
int32_t nqe_table_num_columns(const nqe_table *table);
/* describes column i with DEVICE pointers (valid until the table is released) */
nqe_status nqe_table_column(const nqe_table *table, int32_t i, nqe_column *out);
/* copies column i to host buffers sized per the layout above; validity_out may be NULL when
 * the column has no validity bitmap (see nqe_table_column); data_out only for Utf8. Blocking. */
nqe_status nqe_table_download_column(const nqe_table *table, int32_t i, void *values_out,
                                     uint8_t *validity_out, void *data_out);
/* MemTable::scan(Some(projection)) → RecordBatch::project (memory.rs:31-41): zero-copy */
nqe_status nqe_table_project(nqe_ctx *ctx, const nqe_table *in, const int32_t *indices, int32_t n,
                             nqe_table **out);
/* RecordBatch::slice as used by PhysicalLimitPlan/PhysicalOffsetPlan (limit.rs:32-49,
 * offset.rs:30-51). Copies (device-to-device) so that bitmaps stay offset-free. */
nqe_status nqe_table_slice(nqe_ctx *ctx, const nqe_table *in, int64_t offset, int64_t length,
                           nqe_table **out);
/* concat_batches (hash_join.rs:258-273): column-wise concatenation; n == 0 is
 * NQE_ERR_INVALID_ARGUMENT here (the host mirror builds the empty batch itself). */
nqe_status nqe_table_concat(nqe_ctx *ctx, const nqe_table *const *tables, int32_t n, nqe_table **out);

/* ------------------------------------------------------------------ Arrow C Data Interface
 * MemTable::try_create(schema, batches) (datasource/memory.rs:21-29; Catalog::add_memory_table, catalog.rs:40-49) for hosts that hold
 * real Arrow data, and the way back for results (the Vec<RecordBatch> of plan.rs:18).  The structs are the standard ones of the
 * Arrow C Data Interface (arrow-rs `arrow::ffi`, pyarrow `_export_to_c` / `_import_from_c`); include Arrow's own header first if
 * you have it. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char *format;
    const char *name;
    const char *metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema **children;
    struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct ArrowArray **children;
    struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif
/* One RecordBatch = one struct array (format "+s") whose children are the columns: "l" Int64, "L" UInt64, "g" Float64, "b" Boolean,
 * "u" Utf8; anything else is NQE_ERR_NOT_SUPPORTED (selection.rs:98).  Sliced arrays (offset != 0) are honoured.  The buffers are
 * host memory; they are copied to HBM and `array` is then RELEASED by this call (the interface's move semantics — on failure it is
 * left untouched); `schema` is only read. */
nqe_status nqe_table_import_arrow(nqe_ctx *ctx, struct ArrowArray *array, const struct ArrowSchema *schema, nqe_table **out);
/* The table as one struct array with host copies of its buffers, owned by the returned structs until their `release` callbacks
 * run.  names: one per column, or NULL ("c0", "c1", ...).  Blocking. */
nqe_status nqe_table_export_arrow(const nqe_table *table, const char *const *names, struct ArrowArray *out_array,
                                  struct ArrowSchema *out_schema);

/* ------------------------------------------------------------------ CSV ingest
 * CsvTable::try_create (datasource/csv.rs:53-86) = infer_schema_from_csv (csv.rs:76-85, arrow-rs 13
 * csv::reader::infer_reader_schema over the first max_read_records records) + csv::Reader::next() — only the FIRST
 * batch of batch_size rows is kept (quirk Q1, csv.rs:71-73).  CsvConfig (csv.rs:23-43): has_header = true,
 * delimiter = ',', max_read_records = Some(3), batch_size = 1_000_000; file_projection / datetime_format are not mirrored. */
typedef struct nqe_csv_options {
    int32_t has_header;       /* first record = column names; otherwise "column_1", "column_2", ... */
    int32_t delimiter;        /* one byte */
    int64_t max_read_records; /* records sampled by the inference; < 0 = all */
    int64_t batch_size;       /* rows kept; < 0 = all */
} nqe_csv_options;
/* Schema inference (host side, a handful of records): per column Boolean / Int64 / Float64 / Utf8 (Int64+Float64 →
 * Float64, any other mix → Utf8; Date-like columns → NQE_ERR_NOT_SUPPORTED), nullable[c] = an empty field was seen.
 * names: the column names joined with '\0' terminators (names_bytes = bytes needed). */
nqe_status nqe_csv_infer_schema(nqe_ctx *ctx, const void *bytes_host, int64_t nbytes, const nqe_csv_options *opt,
                                int32_t max_columns, int32_t *num_columns, int32_t *dtypes, int32_t *nullable,
                                char *names, int64_t names_capacity, int64_t *names_bytes);
/* Parses the file image (host or device memory, `location` = nqe_location) into one device table with the given column
 * types: records split on the GPU (quotes with "" escapes, \r / \n / \r\n, empty lines skipped), fields converted on
 * the GPU (lexical-core semantics: Int64 overflow and malformed numbers are NQE_ERR_ARROW, Float64 correctly rounded,
 * empty numeric/Boolean fields are NULL, Utf8 fields are never NULL); a record with a different number of fields is
 * NQE_ERR_ARROW. */
nqe_status nqe_csv_read(nqe_ctx *ctx, const void *bytes, int32_t location, int64_t nbytes, const nqe_csv_options *opt,
                        const int32_t *dtypes, int32_t num_columns, nqe_table **out);

/* ------------------------------------------------------------------ exchange plumbing (multi-GPU)
 * No reference analogue (the reference is single-process).  A rank's partial aggregate (keys + state tables: 8-byte
 * columns without validity) is packed into ONE device buffer so that the exchange is a single RCCL all-gather, and the
 * gathered buffer is unpacked into one concatenated table for nqe_aggregate_merge.
 *
 * pack:   dst[c * stride_rows + r] = word r of column c (columns of `tables` in order, c over all tables);
 *         dst[num_columns * stride_rows] = number of rows (the tables must agree) — the header the peers read.
 *         Every table must have rows <= stride_rows; dst holds num_columns * stride_rows + 1 words.
 * unpack: src = num_parts such buffers back to back; out column c = for p in 0..num_parts: src_p[c][0 .. counts[p]).
 *         counts[p] is what the caller read from the headers (host memory). */
nqe_status nqe_table_pack_words(nqe_ctx *ctx, const nqe_table *const *tables, int32_t num_tables, int64_t stride_rows,
                                void *dst_device);
nqe_status nqe_table_unpack_words(nqe_ctx *ctx, const void *src_device, int32_t num_parts, int32_t num_columns,
                                  int64_t stride_rows, const int64_t *counts, const int32_t *dtypes, nqe_table **out);

/* ------------------------------------------------------------------ sharded operators (multi-GPU)
 * No reference analogue.  One process (or thread) per GPU, each with its own context and a communicator over it; every rank
 * calls the same sharded entry point with ITS row range.  Collectives are enqueued on the context's stream (no host
 * synchronisation between an operator's kernels and its exchange); failures of the transport are NQE_ERR_RCCL.
 *
 * The default transport is RCCL over xGMI, bound at run time (librccl.so.1 is dlopen'ed by the first nqe_comm_* call, never
 * by single-GPU use): rank 0 calls nqe_comm_get_unique_id, the host distributes the 128 bytes by whatever it has (MPI, a
 * store, torch.distributed), every rank calls nqe_comm_create.  nqe_comm_create_custom plugs in the host's own collectives
 * (all_gather / all_gather_v), nqe_comm_create_p2p the host's own point-to-point primitives (send / recv / group brackets —
 * MPI, a test fabric): the library then builds its collectives from them with the very code it runs over RCCL's ncclSend /
 * ncclRecv.
 *
 * Nobody blocks on a failed rank: every sharded entry point runs its fallible local work (the partial aggregate, the probe, the
 * selection: data-dependent DivideByZero, out of memory, ...) first, and a rank that fails there STILL enters the operator's
 * exchange, with its status in the header every exchange starts with — so that every rank returns an error together (the
 * failing rank its own, the others NQE_ERR_RCCL naming the rank and its status) instead of blocking in a collective the failed
 * rank never joined.  A failure AFTER the exchange (the merge of the gathered partials, a Utf8 re-encode: out of memory on one
 * rank) is that rank's alone: the others have their result and return NQE_OK — statuses may then differ between ranks, but no
 * rank waits for another. */
#define NQE_COMM_ID_BYTES 128
/* rows of the fixed-size buffer a partial aggregate travels in (one collective, counts read on the device); larger partials take
 * an exact-size two-step exchange */
#define NQE_EXCHANGE_ROWS 4096
typedef struct nqe_comm nqe_comm;
typedef struct nqe_transport {
    void *user;
    /* every rank contributes `bytes` device bytes; recv (device) receives world*bytes ordered by rank.  Enqueue on `stream`
     * (a hipStream_t) or complete before returning.  0 = success. */
    int32_t (*all_gather)(void *user, const void *send, void *recv, size_t bytes, void *stream);
    /* variable-length form: rank r's contribution (recv_bytes[r] bytes) lands at recv + recv_offsets[r]; send_bytes ==
     * recv_bytes[own rank].  Arrays are host memory, valid for the duration of the call. */
    int32_t (*all_gather_v)(void *user, const void *send, size_t send_bytes, void *recv, const size_t *recv_offsets,
                            const size_t *recv_bytes, void *stream);
    /* optional (may be NULL): brackets around the all_gather_v calls of one table (RCCL: ncclGroupStart / ncclGroupEnd) */
    int32_t (*group_begin)(void *user);
    int32_t (*group_end)(void *user);
    /* optional: called by nqe_comm_destroy */
    void (*destroy)(void *user);
} nqe_transport;
nqe_status nqe_comm_get_unique_id(void *id_out /* NQE_COMM_ID_BYTES */);
nqe_status nqe_comm_rccl_version(int32_t *version_out);
nqe_status nqe_comm_create(nqe_ctx *ctx, const void *unique_id, int32_t rank, int32_t world, nqe_comm **out);
nqe_status nqe_comm_create_custom(nqe_ctx *ctx, const nqe_transport *transport, int32_t rank, int32_t world, nqe_comm **out);
/* Point-to-point primitives with RCCL's semantics: send/recv are enqueued on `stream` (or complete before group_end returns),
 * a send is matched by the peer's recv of the SAME byte count in the same order per (sender, receiver) pair, calls between
 * group_begin and group_end (which may nest) are issued together, so that a rank may post its sends and receives in any order
 * without deadlock.  0 = success.  destroy is optional (called by nqe_comm_destroy). */
typedef struct nqe_p2p {
    void *user;
    int32_t (*send)(void *user, const void *buf, size_t bytes, int32_t peer, void *stream);
    int32_t (*recv)(void *user, void *buf, size_t bytes, int32_t peer, void *stream);
    int32_t (*group_begin)(void *user);
    int32_t (*group_end)(void *user);
    void (*destroy)(void *user);
} nqe_p2p;
nqe_status nqe_comm_create_p2p(nqe_ctx *ctx, const nqe_p2p *p2p, int32_t rank, int32_t world, nqe_comm **out);
nqe_status nqe_comm_destroy(nqe_comm *comm);
int32_t nqe_comm_rank(const nqe_comm *comm);
int32_t nqe_comm_world(const nqe_comm *comm);
/* Ordered variable-length all-gather of a per-rank result table: out = the ranks' tables concatenated in rank order (= row
 * order for row-range shards), on every rank — what `concat_batches` (hash_join.rs:258-273) would make of them.  Every column
 * type of the path travels: 8-byte words move peer to peer straight from the local table into their place in `out` (columns
 * that share a buffer locally are moved once and share it in `out`); validity bitmaps and Boolean values are received per rank
 * and shifted to their bit offset (a column is nullable in `out` when it is on any rank); Utf8 bytes land in place and the
 * offsets are rebased.  A fixed-size header (status, rows, per-column flags and byte counts) travels first: the one host wait. */
nqe_status nqe_table_all_gather(nqe_comm *comm, const nqe_table *local, nqe_table **out);
/* PhysicalAggregatePlan::execute (aggregate/mod.rs:113-222) over the union of every rank's `in`: per-rank partial state
 * {count,sum,min,max} → ONE all-gather → merge on every rank; avg is finalised after the merge.  Same output contract as
 * nqe_aggregate_execute on the concatenated input (f64 sums in a different order: 1e-9 relative).  Utf8 group keys
 * (aggregate/mod.rs:170-216) travel as strings: the partials' (key string, state) rows are all-gathered and merged by string;
 * the output is ordered by first appearance in rank order. */
nqe_status nqe_sharded_aggregate_execute(nqe_comm *comm, const nqe_table *in, const nqe_expr_node *pred, int32_t pred_nodes,
                                         const nqe_expr_node *group, int32_t group_nodes, const nqe_aggregate *aggs,
                                         int32_t num_aggs, nqe_table **out, nqe_table **keys_out);
/* HashJoin::probe (hash_join.rs:168-254) with the build side replicated (every rank built `build` from the whole left table)
 * and the probe side range-split: `right_local` is this rank's contiguous row range.  gather = 0: out = this rank's output
 * rows (rank order == probe row order); gather = 1: out = nqe_table_all_gather of them (the single-GPU result on every rank). */
typedef struct nqe_join_table nqe_join_table;
nqe_status nqe_sharded_hash_join_probe(nqe_comm *comm, const nqe_join_table *build, const nqe_table *right_local,
                                       int32_t right_key, int32_t gather, nqe_table **out);
/* Fused ProjectionPlan(SelectionPlan(input)) over a row-range shard, optionally gathered like the join. */
nqe_status nqe_sharded_selection_projection_execute(nqe_comm *comm, const nqe_table *in_local, const nqe_expr_node *pred,
                                                    int32_t pred_nodes, const nqe_expr_node *nodes, const int32_t *expr_offsets,
                                                    int32_t num_exprs, int32_t gather, nqe_table **out);

/* ------------------------------------------------------------------ expressions
 * PhysicalExpr::evaluate(batch).into_array() (expression/mod.rs:25-29, binary.rs:108-155,
 * datatype.rs:27-34): evaluates one expression over `in`, returns a 1-column table.
 * Literals are kept as scalars in registers (never materialised, cf. binary.rs:121 TODO),
 * except a root literal, which is expanded to `in.num_rows` rows as into_array does.
 * Compares (= != < <= > >=) work on every type incl. Utf8 (byte-wise lexicographic, as arrow's
 * *_dyn kernels); and/or are Kleene; arithmetic is wrapping on Int64/UInt64, IEEE on Float64.
 * Unary nodes (unary.rs:85-108): abs / sin / cos / tan over a Float64 operand give Float64 with
 * the operand's validity (a column operand's validity buffer is shared, not copied; slots under
 * a NULL are unspecified); a literal operand is expanded to `in.num_rows` rows. abs clears the
 * sign bit and nothing else (-0.0 → 0.0, a NaN keeps its payload); sin / cos are the device
 * math library's double-precision functions (OpenCL full profile: 4 ulp); tan is the cosine
 * (quirk Q16).
 * A tree of binary and unary nodes is evaluated in one pass over the columns it references.
 * Errors: operand dtype mismatch → NQE_ERR_INTERVAL; divide/modulus with a valid zero
 * divisor → NQE_ERR_ARROW; arithmetic on Boolean/Utf8 → NQE_ERR_NOT_SUPPORTED; a unary node
 * over anything but Float64 or any of the string functions → NQE_ERR_NOT_SUPPORTED; a unary
 * node without an operand or with an `op` outside nqe_unary_operator →
 * NQE_ERR_INVALID_ARGUMENT. All of these are decided before anything is allocated or launched.
 * String nodes (NQE_EXPR_STRING, quirk Q25) are defined on the BYTES between a slot's two
 * offsets; validity is never read, so the bytes under a NULL are transformed like any other and
 * the result is total and deterministic. TRIM / LTRIM / RTRIM strip bytes 0x20 (and nothing
 * else: tab, newline, U+00A0 and U+3000 stay) from both ends, the front or the back. LOWER /
 * UPPER map the bytes A-Z / a-z and leave every other byte, every byte of a multi-byte sequence
 * included, as it is: ASCII only, the length never changes (Rust's to_lowercase would change
 * it). CHARACTER_LENGTH is Int64: the number of bytes b with (b & 0xC0) != 0x80, the number of
 * code points of valid UTF-8. REVERSE reverses the order of units and keeps the bytes inside a
 * unit in order; byte i starts a unit when i == 0, or it is no continuation byte, or bytes i-1,
 * i-2 and i-3 all exist and are continuation bytes (units are 1-4 bytes: the code points of
 * valid UTF-8, and a fixed permutation of the string's own bytes otherwise). The result has the
 * operand's validity (shared when it may be, else copied) and null_count; a literal operand is
 * expanded to `in.num_rows` rows, a NULL Utf8 literal to an all-NULL column. The operand may be
 * a STRING node; a Utf8 result may feed a Utf8 compare, CHARACTER_LENGTH Int64 arithmetic and
 * compares. A tree that holds a STRING node is evaluated node at a time. Errors, in this order,
 * before anything is allocated or launched: no operand → NQE_ERR_INVALID_ARGUMENT; `op` outside
 * nqe_unary_operator → NQE_ERR_INVALID_ARGUMENT; `op` one of ABS..TAN →
 * NQE_ERR_INVALID_ARGUMENT; REPEAT, REPLACE or SUBSTR (they need arguments a one-operand node
 * cannot carry) → NQE_ERR_NOT_SUPPORTED; an operand that is not Utf8 → NQE_ERR_NOT_SUPPORTED.
 * String nodes with arguments (NQE_EXPR_STRING_ARGS, quirk Q26): SUBSTR(s, start, len),
 * REPEAT(s, n), REPLACE(s, from, to). `s` is any Utf8 value (a column, a literal expanded as a
 * STRING node expands it, a STRING node or another STRING_ARGS node); `start`, `len` and `n` are
 * Int64 values of any form (a column, a literal, any Int64-valued subtree); `from` and `to` are
 * Utf8 LITERALS (NULL allowed). Like Q25's functions these are defined on the bytes between a
 * slot's two offsets and are total and deterministic. Byte j of a string has the character
 * number c(j) = max(1, number of bytes k <= j with (s[k] & 0xC0) != 0x80): code points for valid
 * UTF-8, a fixed partition otherwise, continuation bytes at the very front belonging to
 * character 1. SUBSTR keeps the bytes with max(start, 1) <= c(j) < start + len, the sum
 * saturating at INT64_MAX ("to the end" is len = INT64_MAX; there is no two-operand form);
 * len <= 0, a start past the end and start + len <= 1 give the empty string, nothing is an
 * error, and the result is one contiguous byte range. REPEAT is max(n, 0) copies of the bytes.
 * REPLACE turns the leftmost non-overlapping occurrences of the bytes of `from`, found left to
 * right (each search resumes behind the previous match), into the bytes of `to`; matching is by
 * bytes, and an empty `from` leaves the string as it is. Result row i is NULL iff any operand
 * is NULL at i (a NULL literal makes the whole column NULL); null_count is exact. Unlike Q25's
 * kernels these READ validity: a NULL result row is the EMPTY string — except where the result
 * shares the operand's offsets and so cannot empty a slot (REPLACE with |to| == |from|, whose
 * bytes under a NULL are transformed like any other, and REPLACE with an empty `from` or a
 * `from` longer than the operand's data, which returns the operand's own buffers). When only `s`
 * can be NULL its validity is carried (shared when it may be, else copied). A result of more
 * than 2^31-1 bytes fails with NQE_ERR_ARROW ("offset overflow"): lengths and their total are
 * computed in 64 bits, the failure comes before the data buffer is allocated, and the context
 * stays usable. Zero rows or zero result bytes return a well-formed column. A tree that holds
 * the node is evaluated node at a time. Errors, in this order, before anything is allocated or
 * launched: `op` outside nqe_unary_operator → NQE_ERR_INVALID_ARGUMENT; `op` not REPEAT,
 * REPLACE or SUBSTR → NQE_ERR_INVALID_ARGUMENT; fewer values than the function pops →
 * NQE_ERR_INVALID_ARGUMENT; `s` not Utf8 → NQE_ERR_NOT_SUPPORTED; a SUBSTR or REPEAT argument
 * that is not Int64 (UInt64, Float64, Boolean, Utf8, a Null-typed literal) →
 * NQE_ERR_NOT_SUPPORTED; a REPLACE argument that is not a Utf8 literal → NQE_ERR_NOT_SUPPORTED.
 * String matching (NQE_EXPR_STRING_MATCH, quirk Q27): LIKE, NOT_LIKE, ILIKE, NOT_ILIKE,
 * STARTS_WITH, ENDS_WITH, CONTAINS (Boolean) and STRPOS (Int64) of a string `s` and a pattern.
 * `s` is any Utf8 value (a column, a STRING or STRING_ARGS node, a literal expanded to
 * `in.num_rows` rows as a STRING node expands it); the pattern is a Utf8 LITERAL (NULL allowed)
 * of at most NQE_MAX_MATCH_PATTERN bytes. Like Q25 and Q26 everything is defined on the BYTES
 * between a slot's two offsets, total and deterministic for invalid UTF-8 too.
 * The elements of a LIKE / ILIKE pattern, read left to right: byte `\` (0x5C) followed by a byte
 * b is the literal b, whatever b is; a `\` that ends the pattern is a literal `\`; `%` (0x25) is
 * ANY; `_` (0x5F) is ONE; every other byte is a literal; a run of `%` is one `%`; there is no
 * other escape character. `s LIKE p` is true iff the bytes of s can be cut into consecutive
 * pieces, one per element: a literal's piece is that one byte; ANY's piece is any run of bytes,
 * which may be empty and need not end at a character; ONE's piece is exactly the bytes of one
 * character of Q26's numbering, the set {j : c(j) = k} for one k (a code point of valid UTF-8;
 * continuation bytes at the very front belong to character 1). ILIKE is LIKE after mapping A-Z
 * to a-z in the literal elements and in the string's bytes (ASCII only, Q25's LOWER). NOT_LIKE
 * and NOT_ILIKE are the negations. STARTS_WITH, ENDS_WITH and CONTAINS take the literal
 * verbatim, with no wildcards and no escape, and compare bytes; an empty literal is true.
 * STRPOS(s, sub) is 0 when `sub` does not occur in s, otherwise c(j) of the first byte j of the
 * leftmost byte-wise occurrence; an empty `sub` gives 1, for an empty s too.
 * Row i is NULL iff s is NULL at i or the literal is NULL. Under a NULL the Boolean value bit is
 * 0 (for the NOT forms too) and the Int64 value is 0; the bits of the last value word beyond the
 * row count are 0. The result has no validity buffer when s has none and the literal is not
 * NULL; otherwise it carries s's validity (shared when that is allowed, else copied) and its
 * null_count; a NULL literal gives an all-NULL column with null_count = rows. Zero rows give a
 * well-formed empty column. A tree that holds the node is evaluated node at a time. Errors, in
 * this order, before anything is allocated or launched: `op` outside nqe_match_operator →
 * NQE_ERR_INVALID_ARGUMENT; fewer than two values → NQE_ERR_INVALID_ARGUMENT; `s` not Utf8 →
 * NQE_ERR_NOT_SUPPORTED; a pattern that is not a Utf8 literal (a column, a subtree, another
 * dtype, a Null-typed literal) → NQE_ERR_NOT_SUPPORTED; a pattern of more than
 * NQE_MAX_MATCH_PATTERN bytes → NQE_ERR_NOT_SUPPORTED.
 * Conditional and NULL-handling functions (NQE_EXPR_CONDITIONAL, quirk Q28): NOT(b), IS_NULL(x),
 * IS_NOT_NULL(x), COALESCE(a, b), NULLIF(a, b) and IF(c, t, e). Every operand may be of any form:
 * a column, a literal (a NULL literal included) or any subtree, string nodes and other
 * CONDITIONAL nodes included; the value dtypes are Int64, UInt64, Float64, Boolean and Utf8.
 * NOT is NULL where b is NULL. IS_NULL and IS_NOT_NULL read validity only and are never NULL.
 * COALESCE is a where a is valid, else b (NULL where both are). IF is t where c is valid AND
 * true, and e where c is false OR NULL (SQL CASE; a NULL condition is not propagated). NULLIF is
 * by definition IF(a = b, NULL, a) with `=` this library's NQE_OP_EQ on that dtype: Int64, UInt64
 * and Boolean compare their values; Float64 compares as IEEE does, so NaN equals nothing
 * (NULLIF(NaN, NaN) is NaN) and -0.0 equals +0.0 (NULLIF(-0.0, 0.0) is NULL); Utf8 compares
 * bytes; a NULL a or b makes a = b NULL, so the row is a. Under a NULL result row the word is 0,
 * the Boolean bit is 0 and a Utf8 row is the empty string; the bits of the last value or
 * validity word beyond the row count are 0. A result carries a validity buffer only where the
 * static form can be NULL: NOT iff b can be (a nullable column, a NULL literal or a subtree
 * whose result carries one), IS_NULL and IS_NOT_NULL never, COALESCE iff both operands can be,
 * IF iff t or e can be, NULLIF always; with a buffer null_count is -1, without one 0. Zero rows
 * give a well-formed column; an all-literal node is expanded to `in.num_rows` rows. A Utf8
 * result of more than 2^31-1 bytes fails with NQE_ERR_ARROW ("offset overflow"): the total is
 * computed in 64 bits, the failure comes before the data buffer is allocated, and the context
 * stays usable. A tree that holds the node is evaluated node at a time. Errors, in this order,
 * before anything is allocated or launched: `column` outside 1..3 → NQE_ERR_INVALID_ARGUMENT;
 * `op` outside nqe_cond_operator → NQE_ERR_INVALID_ARGUMENT; `column` not the function's arity →
 * NQE_ERR_INVALID_ARGUMENT; fewer values than the node pops → NQE_ERR_INVALID_ARGUMENT; an
 * operand of dtype NQE_NULLTYPE → NQE_ERR_NOT_SUPPORTED; NOT's operand or IF's `c` not Boolean →
 * NQE_ERR_INTERVAL; the two value operands of COALESCE, NULLIF or IF of different dtypes →
 * NQE_ERR_INTERVAL.
 * Casts (NQE_EXPR_CAST, quirk Q29): `x CAST` converts x, of any form, to the nqe_dtype in the
 * node's `dtype` field. There is no implicit coercion (a dtype mismatch stays NQE_ERR_INTERVAL):
 * the cast is how `id * 1.5`, `v > 0` or `coalesce(v, 0)` cross dtypes. The rules are arrow's
 * cast with safe = true, restated: a conversion that cannot represent the value gives NULL; it
 * is never an error and never wraps. A NULL operand row is a NULL result row; under a NULL
 * result row the word is 0, the Boolean bit is 0 and a Utf8 row is empty; the bits of the last
 * value or validity word beyond the row count are 0.
 *   same dtype                       the operand itself, as a bare column evaluates (a literal is
 *                                    expanded to in.num_rows rows)
 *   Int64 -> UInt64                  NULL iff v < 0
 *   UInt64 -> Int64                  NULL iff v >= 2^63
 *   Int64 / UInt64 -> Float64        the nearest binary64, ties to even; always valid
 *   Float64 -> Int64                 NULL iff NaN, x < -2^63 or x >= 2^63; else truncation toward zero
 *   Float64 -> UInt64                NULL iff NaN, x <= -1.0 or x >= 2^64; else truncation toward
 *                                    zero, so -0.5 and -0.0 give 0
 *   Boolean -> Int64/UInt64/Float64  0 / 1, or 0.0 / 1.0
 *   Boolean -> Utf8                  `true` / `false`
 *   Int64/UInt64/Float64 -> Boolean  v != 0, so NaN is true and -0.0 is false
 *   Int64 / UInt64 -> Utf8           the shortest decimal, a leading `-` for negatives, no `+`
 *                                    (INT64_MIN is 20 bytes)
 *   Utf8 -> Int64                    [+-]digits+ over the slot's bytes; anything else is NULL: the
 *                                    empty string, blanks, overflow, `1e3`, `1.0`
 *   Utf8 -> UInt64                   [+]digits+; above 2^64-1 is NULL; any `-` is NULL, `-0` included
 *   Utf8 -> Float64                  the CSV reader's grammar ([+-] (digits [. digits*] | . digits+)
 *                                    [(e|E) [+-] digits+] | [+-] (nan | inf | infinity), ASCII
 *                                    case-insensitive), correctly rounded; anything else is NULL
 *   Utf8 -> Boolean                  `true` / `false`, ASCII case-insensitive; anything else is NULL
 * Nothing trims the input: cast(trim(s) as bigint) composes. A result carries a validity buffer
 * only where the static form can be NULL. The infallible casts (same dtype, Int64 / UInt64 ->
 * Float64, Boolean -> anything, numeric -> Boolean, Int64 / UInt64 -> Utf8) carry one iff the
 * operand does: the operand's buffer, shared where an output may alias it, else copied, with the
 * operand's null_count. The fallible casts (Int64 <-> UInt64, Float64 -> Int64 / UInt64, Utf8 ->
 * anything) always carry one, with null_count -1. Zero rows give a well-formed column. A Utf8
 * result of more than 2^31-1 bytes fails with NQE_ERR_ARROW before the data buffer is allocated.
 * A tree that holds the node is evaluated node at a time. Errors, in this order, before anything
 * is allocated or launched: `dtype` outside NQE_BOOLEAN..NQE_UTF8 → NQE_ERR_INVALID_ARGUMENT; no
 * operand on the stack → NQE_ERR_INVALID_ARGUMENT; an operand of dtype NQE_NULLTYPE →
 * NQE_ERR_NOT_SUPPORTED; Float64 -> Utf8 → NQE_ERR_NOT_SUPPORTED (shortest-round-trip digit
 * generation is not part of this library yet). */
nqe_status nqe_expr_evaluate(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes,
                             int32_t num_nodes, nqe_table **out);

/* ------------------------------------------------------------------ filter
 * build_array_by_predicate! over every column (selection.rs:34-51, :65-100): stable
 * compaction of all columns of `in` by a Boolean predicate column: true → keep the row,
 * false → drop, NULL → emit a NULL row (quirk Q4). Rows = min(pred.length, in.num_rows)
 * (iterator zip, quirk Q3). `predicate` is column `pred_column` of `pred_table`. */
nqe_status nqe_filter(nqe_ctx *ctx, const nqe_table *in, const nqe_table *pred_table,
                      int32_t pred_column, nqe_table **out);
/* SelectionPlan::execute for a single input batch (selection.rs:58-107) = evaluate + filter. */
nqe_status nqe_selection_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred,
                                 int32_t pred_nodes, nqe_table **out);

/* ------------------------------------------------------------------ projection
 * ProjectionPlan::execute for one batch (projection.rs:43-70): one output column per
 * expression. `nodes` holds the expressions back to back; expression e occupies
 * nodes[expr_offsets[e] .. expr_offsets[e+1]). */
nqe_status nqe_projection_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes,
                                  const int32_t *expr_offsets, int32_t num_exprs, nqe_table **out);
/* Fused ProjectionPlan(SelectionPlan(input)) for one batch: identical result to
 * nqe_selection_execute followed by nqe_projection_execute, but only the columns the
 * projection references are compacted and the expressions are evaluated in the
 * compaction kernel (C2 of BASELINE.json). */
nqe_status nqe_selection_projection_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred,
                                            int32_t pred_nodes, const nqe_expr_node *nodes,
                                            const int32_t *expr_offsets, int32_t num_exprs,
                                            nqe_table **out);

/* ------------------------------------------------------------------ hash aggregate
 * PhysicalAggregatePlan::execute (aggregate/mod.rs:113-222) fused with an optional
 * SelectionPlan below it (`pred`, may be NULL/0) and the key expression group_expr[0]
 * (`group`, may be NULL/0 = un-grouped path :123-139).
 * Output `out`: one row per group (one row when un-grouped), one column per aggregate,
 * Float64 for sum/avg/min/max and UInt64 for count (sum.rs:29,115, count.rs:23,76), NO
 * key column (quirk Q8). Row order = ascending first-occurrence order of the key is NOT
 * promised: rows are sorted by key (the reference's order is HashMap-random; compare as
 * multisets). If `keys_out` != NULL it receives a 1-column table with the group keys in
 * the same row order (debug/merge aid, not part of the reference output).
 * NULL keys are dropped (:64); NULL values are skipped by every aggregate; a NULL
 * predicate emits a NULL row from the selection, which then has a NULL key/value (Q4).
 * Accumulation is f64 for every input type (`val as f64`, quirk Q10); max starts at
 * f64::MIN, min at f64::MAX, NaN ordering follows OrderedFloat (max.rs:30,48).
 * Key dtype must be Int64, UInt64 or Utf8 (a bare Utf8 column; keys_out then holds the strings); anything else is
 * NQE_ERR_NOT_SUPPORTED (aggregate/mod.rs:217). */
nqe_status nqe_aggregate_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred,
                                 int32_t pred_nodes, const nqe_expr_node *group, int32_t group_nodes,
                                 const nqe_aggregate *aggs, int32_t num_aggs, nqe_table **out,
                                 nqe_table **keys_out);
/* Partial-state form used to merge per-GPU / per-batch partials:
 * the output columns are the raw state of every DISTINCT aggregate column (slot v = the v-th
 * distinct `column` of `aggs` in order of first appearance; count,sum,avg,min,max over one
 * column exchange four words per group, not twenty), in this order for every slot v:
 *   4*v+0 count (UInt64, non-null values), 4*v+1 sum (Float64), 4*v+2 min (Float64),
 *   4*v+3 max (Float64; NaN if any NaN was seen),
 * plus keys in `keys_out` (required when grouped).  The merges take the same `aggs`. */
nqe_status nqe_aggregate_partial(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred,
                                 int32_t pred_nodes, const nqe_expr_node *group, int32_t group_nodes,
                                 const nqe_aggregate *aggs, int32_t num_aggs, nqe_table **state_out,
                                 nqe_table **keys_out);
/* Merges `n` partial (state, keys) pairs (e.g. all-gathered from all ranks, concatenated or
 * not) and finalises to the nqe_aggregate_execute output format. keys may be NULL for the
 * un-grouped form. */
nqe_status nqe_aggregate_merge(nqe_ctx *ctx, const nqe_table *const *states, const nqe_table *const *keys,
                               int32_t n, const nqe_aggregate *aggs, int32_t num_aggs, nqe_table **out,
                               nqe_table **keys_out);
/* The same merge straight from an all-gathered buffer of nqe_table_pack_words parts (part p = [key column when `grouped`] +
 * {count,sum,min,max} per distinct aggregate column, `stride_rows` words per column, + 1 header word = the part's row count): the counts
 * are read on the device, so the whole exchange + merge costs the host one wait.  When some part's header exceeds
 * `stride_rows` (its sender shipped the header only) the call returns NQE_OK with *out = NULL and the caller exchanges
 * exact-size tables instead (nqe_aggregate_merge).  Replaces the same merge loop as nqe_aggregate_merge. */
nqe_status nqe_aggregate_merge_packed(nqe_ctx *ctx, const void *gathered_device, int32_t num_parts, int64_t stride_rows,
                                      int32_t grouped, int32_t key_dtype, const nqe_aggregate *aggs, int32_t num_aggs,
                                      nqe_table **out, nqe_table **keys_out);

/* ------------------------------------------------------------------ hash aggregate on several keys
 * GROUP BY honouring EVERY group expression — quirk Q20: the reference's planner builds `group by a, b` plans and its logical
 * Aggregate's schema is "group fields, then aggregate fields" (logical_plan/dataframe.rs:58-67, Q13), but
 * PhysicalAggregatePlan::execute reads group_expr[0] alone (aggregate/mod.rs:146, Q8, which nqe_aggregate_execute reproduces).
 * Key i is the post-order node range [group_offsets[i], group_offsets[i+1]) of `group_nodes` (nqe_projection_execute's
 * convention).  Rows group by the whole tuple (key_0, ..., key_{k-1}): two tuples are equal iff every integer key is equal as a
 * 64-bit word and every Utf8 key byte for byte; a row is dropped if ANY of its keys is NULL (aggregate/mod.rs:64 at every
 * position); `pred` means what it means in nqe_aggregate_execute (Q4 included); a tuple whose rows are all rejected or dropped
 * gives no output row.
 * Output: ONE table of the k key columns in key order (the key's dtype, no validity buffer, null_count 0) followed by one column
 * per aggregate with the dtypes and Q10 semantics of nqe_aggregate_execute.  Rows are sorted ascending by the key tuple, key 0
 * most significant — Int64 signed, UInt64 unsigned, Utf8 in byte order: nqe_sort_execute's order with default options — so the
 * output is deterministic; zero groups give a 0-row table with every column.  With num_keys == 1 and an integer key the
 * aggregate columns are those of nqe_aggregate_execute (counts, min, max bit for bit; sums and averages to 1e-9 relative) and the
 * key column is its keys_out.  Nothing is kept between calls.
 * Errors, all before any launch or allocation: num_keys <= 0 NQE_ERR_PLAN (the un-grouped form stays with
 * nqe_aggregate_execute); num_keys > NQE_MAX_GROUP_KEYS NQE_ERR_NOT_SUPPORTED; offsets that do not ascend or a NULL `out`
 * NQE_ERR_INVALID_ARGUMENT; a key whose dtype is not Int64, UInt64 or Utf8, or a Utf8 key that is not a bare column,
 * NQE_ERR_NOT_SUPPORTED (aggregate/mod.rs:217), also at 0 rows; everything about `pred` and `aggs` as nqe_aggregate_execute
 * reports it.  A key expression that faults (division by zero) reports what nqe_expr_evaluate reports. */
#define NQE_MAX_GROUP_KEYS 8
nqe_status nqe_group_aggregate_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int32_t pred_nodes,
                                       const nqe_expr_node *group_nodes, const int32_t *group_offsets, int32_t num_keys,
                                       const nqe_aggregate *aggs, int32_t num_aggs, nqe_table **out);

/* ------------------------------------------------------------------ hash join
 * HashJoin::execute = build() + probe() (hash_join.rs:124-254, :280-284) for one left
 * (build) batch and one right (probe) batch: inner equi-join on
 * left[left_key] == right[right_key]; output = all left columns gathered by build index
 * followed by all right columns gathered by probe index (`take`, :237-246); row order is
 * probe-row-major and, for duplicate build keys, ascending build row index (:86-101).
 * Key validity is ignored (quirk Q11): the raw 8-byte slot value is compared.
 * Key dtypes: both Int64, both UInt64 or both Utf8 (other types NQE_ERR_NOT_IMPLEMENTED, :161; differing types
 * NQE_ERR_NOT_SUPPORTED — the reference's downcast unwrap panics). */
nqe_status nqe_hash_join_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right,
                                 int32_t left_key, int32_t right_key, nqe_table **out);
/* Two-phase form: build once (replicated per GPU), probe many right batches / shards (nqe_join_table is declared with the
 * sharded operators above). */
nqe_status nqe_hash_join_build(nqe_ctx *ctx, const nqe_table *left, int32_t left_key, nqe_join_table **out);
nqe_status nqe_hash_join_probe(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right,
                               int32_t right_key, nqe_table **out);
nqe_status nqe_join_table_release(nqe_join_table *jt);

/* ------------------------------------------------------------------ outer hash joins
 * HashJoin honouring `join_type` — quirk Q19: the reference's planner builds JoinType::Left / Right plans
 * (sql/planner.rs:221-225) and HashJoin stores the type without reading it (hash_join.rs:48-49).  The MATCH RELATION is exactly
 * nqe_hash_join_probe's, Q11 included: left = build side, right = probe side, key validity ignored, the raw 8-byte slot (the
 * bytes for Utf8) compared, the same key dtypes and errors.  So LEFT JOIN ⊇ JOIN holds against this library's own inner join
 * (nqe_nested_loop_join_execute, Q17, keeps its different relation: there a NULL key matches nothing).
 *   probe-preserving (RIGHT): nqe_hash_join_probe_outer with NQE_JOIN_KEEP_PROBE — one output batch per probe batch,
 *     probe-row-major; a matched probe row emits its matches in ascending build row (the inner join's rows, in its order), a
 *     probe row without a match emits ONE row in its place with every left column NULL.
 *   build-preserving (LEFT): create marks for the join table, pass them to every nqe_hash_join_probe_outer call (the outputs
 *     are the inner join's; the marks record which build rows matched), then nqe_hash_join_unmatched_build gives one final
 *     batch — possibly of 0 rows — with every build row that matched in none of the probes, in ascending build row, followed by
 *     num_right all-NULL columns of the given nqe_dtype (the probe side's schema).
 *   FULL: both together.
 * With flags = 0 and marks = NULL the output equals nqe_hash_join_probe's, column for column and bit for bit (the outer path
 * is one general count / scan / write path over every build form and takes none of the inner join's fused tiers).
 * NULL-extended cells hold 0 (word columns), a false bit (Boolean) or a zero-length string (Utf8); an output column has a
 * validity buffer iff its source has one or the batch contains a NULL-extended row on that side; null_count is exact.
 * Nothing is kept between calls except what the marks record.  Marks are bound to one join table and must be released before it.
 * Errors, decided before any launch: key index / key dtypes / the 32-column limit as nqe_hash_join_probe;
 * NQE_ERR_INVALID_ARGUMENT for unknown flag bits, marks created for another table or on another context, NULL marks in
 * nqe_hash_join_unmatched_build, num_right < 0, a dtype outside nqe_dtype (NQE_NULLTYPE: NQE_ERR_NOT_SUPPORTED).  After the
 * count pass: a 4096-row probe tile whose output exceeds 2^32 rows is NQE_ERR_OUT_OF_MEMORY, as in the inner join — nothing of
 * the output's size is allocated and no output is written, but the count pass has run: marks passed to that call hold the
 * matches of the refused batch. */
typedef struct nqe_join_marks nqe_join_marks; /* which build rows have matched so far; bound to one join table */
nqe_status nqe_join_marks_create(nqe_ctx *ctx, const nqe_join_table *build, nqe_join_marks **out);
nqe_status nqe_join_marks_release(nqe_join_marks *marks);
#define NQE_JOIN_KEEP_PROBE 1u
nqe_status nqe_hash_join_probe_outer(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, int32_t right_key,
                                     uint32_t flags, nqe_join_marks *marks /* may be NULL */, nqe_table **out);
nqe_status nqe_hash_join_unmatched_build(nqe_ctx *ctx, const nqe_join_table *build, const nqe_join_marks *marks,
                                         const int32_t *right_dtypes, int32_t num_right, nqe_table **out);

/* ------------------------------------------------------------------ hash join on several keys
 * HashJoin honouring every `on` pair — quirk Q21: the reference's DataFrame::join zips every key pair into `on`
 * (logical_plan/dataframe.rs:109) and HashJoin::execute reads on[0] alone (hash_join.rs:134, :171).  The MATCH RELATION is the hash
 * join's own, Q11 included, applied to every pair: two rows match iff for every pair i the raw 8-byte slot (the bytes between the
 * slot's offsets for Utf8) of left[left_keys[i]] equals that of right[right_keys[i]]; key validity is ignored at every position.
 * Per pair both Int64, both UInt64 or both Utf8 (pairs of different types may be mixed); the errors are the single-key join's for the
 * first offending pair, in pair order.  The OUTPUT is exactly the single-key operators': all left columns, then all right columns,
 * probe-row-major, matches in ascending build row, the NULL-extension / validity / null_count rules of the outer joins — no column
 * that is not the caller's ever appears.  With one pair the calls forward to nqe_hash_join_build / _probe / _probe_outer / _execute:
 * the result is theirs bit for bit.
 *   nqe_hash_join_probe_keys: `flags` / `marks` as in nqe_hash_join_probe_outer; with flags = 0 and marks = NULL the inner probe's
 *     tiers are taken.  nqe_join_marks_create, nqe_hash_join_unmatched_build and nqe_join_table_release accept a table from
 *     nqe_hash_join_build_keys unchanged.
 * Errors, decided before any launch or allocation: num_keys <= 0 NQE_ERR_PLAN (the empty `on`); num_keys > NQE_MAX_JOIN_KEYS
 * NQE_ERR_NOT_SUPPORTED; a key index out of range NQE_ERR_LOGICAL; NULL index arrays or `out`, a num_keys that differs from the
 * build's, unknown flag bits, foreign marks NQE_ERR_INVALID_ARGUMENT.  A table built on more than one key is refused with
 * NQE_ERR_INVALID_ARGUMENT by nqe_hash_join_probe, nqe_hash_join_probe_outer and nqe_sharded_hash_join_probe.
 * A build side of 2^30 rows or more whose keys need the tuple dictionary (a Utf8 pair, or integer spans whose product exceeds 2^62) is
 * NQE_ERR_NOT_SUPPORTED; for integer keys that is known only after the range pass over the build keys has run.
 * With more than one pair each side carries one hidden code column through the join, and both count against the join's 32-column
 * limit: a composite join refuses left + right + 2 > 32 columns with NQE_ERR_NOT_SUPPORTED.
 * Nothing is kept between calls except what the marks record.  NQE_JOIN_KEYS_FORCE_DICT=1 (a diagnostic switch, read per build call)
 * sends integer tuples through the tuple dictionary instead of the packed codes; no result changes. */
#define NQE_MAX_JOIN_KEYS 8
nqe_status nqe_hash_join_build_keys(nqe_ctx *ctx, const nqe_table *left, const int32_t *left_keys, int32_t num_keys, nqe_join_table **out);
nqe_status nqe_hash_join_probe_keys(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, const int32_t *right_keys,
                                    int32_t num_keys, uint32_t flags, nqe_join_marks *marks /* may be NULL */, nqe_table **out);
nqe_status nqe_hash_join_execute_keys(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, const int32_t *left_keys,
                                      const int32_t *right_keys, int32_t num_keys, nqe_table **out); /* inner */

/* ------------------------------------------------------------------ semi and anti hash joins
 * "Which rows of this table have a partner in that one", and the complement: the join behind WHERE k IN (SELECT ...), EXISTS and
 * NOT EXISTS — quirk Q22.  The reference has no such operator (JoinType is {Inner, Left, Right, Cross}, logical_plan/plan.rs:134-139);
 * it is defined against this library's own inner join.  Left = build side, right = probe side; the MATCH RELATION is
 * nqe_hash_join_probe_keys', Q11 included: raw 8-byte slots for Int64 / UInt64 keys, the bytes between the offsets for Utf8 keys, key
 * validity ignored at every position, the same key dtype rules and errors.
 *   probe SEMI  (nqe_hash_join_probe_semi, flags without NQE_SEMI_ANTI): one batch per probe batch with EVERY RIGHT COLUMN AND NOTHING
 *               ELSE, holding the probe rows that have at least one match, each once, in probe order.  Its rows are the distinct probe
 *               rows of the inner join's output over the same tables (duplicate build keys do not repeat a probe row).
 *   probe ANTI  (NQE_SEMI_ANTI): the same with the probe rows that have no match; SEMI and ANTI partition the batch.
 *   build SEMI / ANTI: pass marks to any number of nqe_hash_join_probe_semi calls (`out` = NULL is the mark-only pass: no keep mask,
 *               no counts, no compaction), then nqe_hash_join_marked_build gives one batch with the build rows that matched in some
 *               batch (flags = 0) or in none (NQE_SEMI_ANTI), in ascending build row, with the visible left columns only — no right
 *               column and never the hidden code column of a table built on several keys.  ANTI's columns are the first n_left
 *               columns of nqe_hash_join_unmatched_build, bit for bit.
 * The probe door serves tables from nqe_hash_join_build and from nqe_hash_join_build_keys; num_keys must equal the build's.
 * Output columns are what the selection's compaction gives for the keep mask: values of valid rows bit for bit, validity preserved
 * (a validity buffer is present exactly when the source column has one), null_count exact, Boolean and Utf8 payload columns allowed.
 * An empty side or no kept row gives a 0-row table with every column.  Nothing is kept between calls except what the marks record.
 * NQE_SEMI_NULL_KEY_UNMATCHED is the EXISTS / NOT EXISTS / IN reading: a probe row with a NULL at ANY key position matches nothing —
 * SEMI drops it, ANTI keeps it, and it sets no mark.  With this flag a build key column that has a validity buffer and a null_count
 * other than 0 is NQE_ERR_NOT_SUPPORTED (excluding NULL build rows would need the table rebuilt without them).  NOT IN's three-valued
 * rule — one NULL on the build side empties the result — is NOT implemented: the caller tests the build side for NULLs itself.
 * Errors, decided before any launch or allocation, in this order: NULL ctx / build / right / right_keys, or `out` and `marks` both NULL:
 * NQE_ERR_INVALID_ARGUMENT; num_keys <= 0 NQE_ERR_PLAN; num_keys > NQE_MAX_JOIN_KEYS NQE_ERR_NOT_SUPPORTED; a num_keys that differs
 * from the build's, unknown flag bits, foreign marks NQE_ERR_INVALID_ARGUMENT; a key index out of range NQE_ERR_LOGICAL; the key dtype
 * errors of the join; the NULL-flag refusal above.  nqe_hash_join_marked_build: NULL or foreign marks, or flag bits other than
 * NQE_SEMI_ANTI, NQE_ERR_INVALID_ARGUMENT.  The join's 32-column limit does not apply: columns are compacted one at a time and no
 * build column is written. */
#define NQE_SEMI_ANTI 1u
#define NQE_SEMI_NULL_KEY_UNMATCHED 2u
nqe_status nqe_hash_join_probe_semi(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, const int32_t *right_keys,
                                    int32_t num_keys, uint32_t flags, nqe_join_marks *marks /* may be NULL */, nqe_table **out /* NULL: mark only */);
nqe_status nqe_hash_join_marked_build(nqe_ctx *ctx, const nqe_join_table *build, const nqe_join_marks *marks, uint32_t flags /* NQE_SEMI_ANTI or 0 */,
                                      nqe_table **out);

/* ------------------------------------------------------------------ cross join
 * CrossJoin::execute (cross_join.rs:55-185) for one outer (left) batch and one inner (right)
 * batch; the caller loops over the batch pairs outer-major, one output batch per pair, and a side
 * without batches gives no output batches.  Quirk Q15: with L = left rows and R = right rows the
 * output has N = L*R rows, left columns first, then right columns; output row j takes left row
 * j % L and right row j % R (the reference's loop order: a Cartesian product only when
 * gcd(L, R) = 1).  Validity is dropped: Int64/UInt64/Float64 outputs hold the raw 8-byte slots,
 * Utf8 outputs the bytes between a slot's offsets, also under a NULL; no output has a validity
 * bitmap (null_count 0).  join_type is ignored and nothing is kept between calls.
 * Errors, decided on the host before anything is allocated or launched: a Boolean column on either
 * side NQE_ERR_NOT_SUPPORTED, also at 0 rows (the reference panics: unimplemented!()); a Utf8 output
 * of more than INT32_MAX bytes NQE_ERR_NOT_SUPPORTED (its int32 offsets overflow: the reference
 * panics); L*R or a column's byte size beyond int64, or an output larger than the device,
 * NQE_ERR_OUT_OF_MEMORY. */
nqe_status nqe_cross_join_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, nqe_table **out);

/* ------------------------------------------------------------------ nested loop join
 * NestedLoopJoin::execute (nested_loop_join.rs:110-175) for one outer (left) batch and one inner
 * (right) batch; the caller loops over the batch pairs outer-major, one output batch per pair (empty
 * ones included), and nothing is kept between calls.  Quirk Q17: the row pair (x, y) is emitted iff
 * both keys are valid and equal — Int64 / UInt64 by the 64-bit word, Float64 by IEEE == (NaN matches
 * nothing, -0.0 matches 0.0), Utf8 by the bytes; a NULL key matches nothing (unlike the hash join,
 * Q11).  Output rows are sorted by (x, y) ascending: the order of the reference's two loops.  The
 * output holds all left columns taken by x, then all right columns taken by y (`take`: validity is
 * preserved; Boolean and Utf8 payload columns are fine).  An empty side or no match gives a 0-row
 * table with every column.
 * Errors: a key index out of range NQE_ERR_NOT_SUPPORTED; key dtypes that differ NQE_ERR_PLAN; then
 * any equal pair other than Int64 / UInt64 / Float64 / Utf8 NQE_ERR_NOT_SUPPORTED (the reference
 * panics: unimplemented!()) — all three also at 0 rows, before any launch.  After the count pass and
 * before the output is allocated: the positions plus every column beyond int64 or larger than the
 * device NQE_ERR_OUT_OF_MEMORY; a Utf8 output column of more than INT32_MAX bytes
 * NQE_ERR_NOT_SUPPORTED (arrow's take would overflow its int32 offsets).  Counts and positions are
 * 64-bit: more than 2^32 output rows are legal. */
nqe_status nqe_nested_loop_join_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right,
                                        int32_t left_key, int32_t right_key, nqe_table **out);

/* ------------------------------------------------------------------ order by
 * ORDER BY over ONE table (the caller concatenates its batches first, as HashJoin::build does with
 * concat_batches): the reference parses the clause and drops it (sql/planner.rs:159-162), so the
 * definition — quirk Q18 — is arrow-rs' lexsort_to_indices followed by take.  Keys are
 * lexicographic, keys[0] most significant; the sort is stable (rows that tie on every key keep
 * their input order).  Int64 sorts signed, UInt64 unsigned, Boolean false < true, Float64 in the
 * order min / max use (-0.0 ties with +0.0, every NaN ties with every NaN and is greater than +inf),
 * Utf8 in byte order (memcmp, the shorter string first on a common prefix).  `descending` reverses
 * the values of that key; its NULLs go first or last as `nulls_first` says, whatever `descending`
 * says, and tie among themselves.  arrow-rs' SortOptions::default() is {descending 0, nulls_first
 * 1}.  The output holds every column of `in` (validity preserved; Boolean and Utf8 payload columns
 * are fine), taken by the first min(fetch, rows) positions of the order; fetch < 0: all rows,
 * fetch = 0: a 0-row table with every column.
 * Errors, all before any launch or allocation: num_keys <= 0 NQE_ERR_PLAN; a key column index out
 * of range NQE_ERR_NOT_SUPPORTED; 2^32 rows or more NQE_ERR_NOT_SUPPORTED (the sort's payload is a
 * 32-bit position). */
typedef struct nqe_sort_key {
    int32_t column;
    int32_t descending;
    int32_t nulls_first;
} nqe_sort_key;
nqe_status nqe_sort_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_sort_key *keys, int32_t num_keys,
                            int64_t fetch /* < 0: all rows */, nqe_table **out);

/* ------------------------------------------------------------------ window functions
 * f(...) OVER (PARTITION BY ... ORDER BY ...) over ONE table — quirk Q23: the reference has no
 * window expression at all (logical_plan/expression.rs:22-46), so the definition is this project's.
 * All functions of one call share one window: the same partition keys and the same order keys.
 * The sorted order is nqe_sort_execute's order by (the partition keys with default options, then
 * the order keys as given); the sort is stable, so rows that tie on every key keep their input
 * order and every function is deterministic, ROW_NUMBER and the ROWS frame among tied rows
 * included.  Two rows are in the same PARTITION iff they tie on every partition key, ties being
 * the sort's own: Int64 / UInt64 the 64-bit word, Float64 as OrderedFloat (-0.0 = +0.0, every NaN
 * equals every NaN), Boolean the bit, Utf8 byte for byte; a NULL equals a NULL, whatever lies under
 * it, and differs from every value.  Two rows of one partition are PEERS iff they also tie on
 * every order key.  With no order keys all rows of a partition are peers and ROWS runs in input
 * order; with no partition keys the table is one partition.
 * The output is ONE table of num_funcs columns and in->rows rows IN INPUT ORDER: row i holds the
 * functions' values for input row i.  No column has a validity buffer (null_count 0); the input
 * columns are not copied.
 *   ROW_NUMBER, RANK, DENSE_RANK   UInt64, 1-based: RANK = 1 + the partition rows before the row's
 *                                  first peer, DENSE_RANK = the peer groups up to the row's own
 *   COUNT, SUM, MIN, MAX, AVG      exactly the aggregates of nqe_aggregate_execute (quirk Q10) over
 *                                  the rows of the frame: Int64 / UInt64 / Float64 inputs, every
 *                                  value converted to f64 first, a NULL skipped; COUNT UInt64, the
 *                                  others Float64; a frame without valid rows gives sum 0.0, avg
 *                                  NaN, min f64::MAX, max f64::MIN; min ignores NaN, max becomes
 *                                  NaN when the frame holds one; avg divides by the count as u32
 * Errors, all before any launch or allocation, in this order: NULL ctx / in / out or a NULL array
 * with a positive count NQE_ERR_INVALID_ARGUMENT; func, or an aggregate's frame, outside its enum
 * NQE_ERR_INVALID_ARGUMENT; num_funcs <= 0 NQE_ERR_PLAN; more keys or functions than the limits
 * NQE_ERR_NOT_SUPPORTED; a key or value column index out of range, a key dtype the sort
 * refuses, an aggregate (COUNT included) over Boolean or Utf8, 2^32 rows or more
 * NQE_ERR_NOT_SUPPORTED.  Zero rows give a 0-row table with every column.  Nothing is kept
 * between calls.
 * Out of scope: frames with offsets (n PRECEDING, FOLLOWING); LAG / LEAD / FIRST_VALUE / NTILE;
 * several different windows in one call (call once per window); SQL parsing. */
#define NQE_MAX_WINDOW_KEYS 8
#define NQE_MAX_WINDOW_FUNCS 16
typedef enum nqe_window_func {
    NQE_WIN_ROW_NUMBER = 0,
    NQE_WIN_RANK = 1,
    NQE_WIN_DENSE_RANK = 2,
    NQE_WIN_COUNT = 3,
    NQE_WIN_SUM = 4,
    NQE_WIN_MIN = 5,
    NQE_WIN_MAX = 6,
    NQE_WIN_AVG = 7
} nqe_window_func;
typedef enum nqe_window_frame {
    NQE_FRAME_PARTITION = 0, /* every row of the partition */
    NQE_FRAME_ROWS = 1,      /* ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW */
    NQE_FRAME_RANGE = 2      /* RANGE ... CURRENT ROW: up to the row's LAST peer (SQL's default with ORDER BY) */
} nqe_window_frame;
typedef struct nqe_window_spec {
    int32_t func;   /* nqe_window_func */
    int32_t column; /* the aggregate's input column; ignored by the three ranking functions */
    int32_t frame;  /* nqe_window_frame; ignored by the three ranking functions */
} nqe_window_spec;
nqe_status nqe_window_execute(nqe_ctx *ctx, const nqe_table *in, const int32_t *partition_cols, int32_t num_partition,
                              const nqe_sort_key *order_keys, int32_t num_order, const nqe_window_spec *funcs,
                              int32_t num_funcs, nqe_table **out);

/* ------------------------------------------------------------------ window functions, the wider entry
 * nqe_window_execute_ex is a superset of nqe_window_execute (quirk Q23): the same window — sorted
 * order, partitions, peers, ties, word for word — and the same output shape (ONE table of num_funcs
 * columns and in->rows rows IN INPUT ORDER, nothing kept between calls), with four more functions
 * and one more frame.  Below, i is a row's position in the sorted order and pf / pl the first and
 * last position of its partition.
 *   functions 0..7 over frames 0..2   exactly nqe_window_execute: bit-identical results
 *   NQE_FRAMEX_ROWS_BETWEEN   (aggregates, FIRST_VALUE, LAST_VALUE) the positions
 *                 [max(i + start, pf), min(i + end, pl)]: start = -3 is 3 PRECEDING, 0 CURRENT ROW,
 *                 2 is 2 FOLLOWING; NQE_FRAME_UNBOUNDED_PRECEDING only as start,
 *                 NQE_FRAME_UNBOUNDED_FOLLOWING only as end.  A frame may exclude the current row
 *                 (-3 .. -1, 1 .. 3) and may be EMPTY; an empty frame gives Q10's start values as a
 *                 frame of NULLs does: count 0, sum 0.0, avg NaN, min f64::MAX, max f64::MIN.  The
 *                 aggregates keep Q10 in every respect (f64 conversion, NULL skipped, min ignores
 *                 NaN, max becomes NaN, avg divides by the count as u32); UInt64 / Float64 without
 *                 validity.  No value outside a frame takes part in its result: a bounded frame is
 *                 combined from at most two segmented scans, never from a difference of prefixes.
 *   LAG / LEAD    (column, param = k >= 0) the value of the row at position i - k / i + k when that
 *                 lies in [pf, pl], else default_value when has_default, else NULL.  The column's
 *                 dtype; the 8 bytes are copied, not converted.  A NULL source row gives NULL; k = 0
 *                 is the row itself.  frame, start and end are ignored.
 *   FIRST_VALUE / LAST_VALUE   (column, frame) the value, with its validity, at the frame's first /
 *                 last position, for any of the four frames (ROWS: [pf, i]; RANGE: [pf, the last
 *                 peer]; PARTITION: [pf, pl]); an empty frame gives NULL.
 *   NTILE         (param = b >= 1) UInt64, 1-based: with m = pl - pf + 1, q = m / b, r = m % b the
 *                 first r buckets hold q + 1 rows, the others q (SQL's rule).  column and frame are
 *                 ignored.
 * The columns of LAG / LEAD / FIRST_VALUE / LAST_VALUE (Int64 / UInt64 / Float64 arguments only)
 * report an exact null_count; their validity buffer is absent when it is 0.
 * Errors, all before any launch or allocation, in this order: (1) NULL ctx / in / out or a NULL
 * array with a positive count NQE_ERR_INVALID_ARGUMENT; (2) per function in list order, each
 * NQE_ERR_INVALID_ARGUMENT: func outside the enum; for a framed function (aggregates, FIRST_VALUE,
 * LAST_VALUE) frame outside the enum; ROWS_BETWEEN with start == UNBOUNDED_FOLLOWING, end ==
 * UNBOUNDED_PRECEDING or start > end; LAG / LEAD with param < 0; NTILE with param < 1;
 * (3) num_funcs <= 0 NQE_ERR_PLAN; (4) more keys or functions than NQE_MAX_WINDOW_KEYS /
 * NQE_MAX_WINDOW_FUNCS NQE_ERR_NOT_SUPPORTED; (5) a key or value column index out of range
 * NQE_ERR_NOT_SUPPORTED; (6) a key dtype the sort refuses, an aggregate over Boolean / Utf8, a
 * value function over anything but Int64 / UInt64 / Float64 NQE_ERR_NOT_SUPPORTED; (7) 2^32 rows
 * or more NQE_ERR_NOT_SUPPORTED.  Zero rows give a 0-row table with every column.
 * Out of scope: RANGE and GROUPS frames with offsets; EXCLUDE; IGNORE NULLS; NTH_VALUE /
 * PERCENT_RANK / CUME_DIST; value functions over Boolean / Utf8; several different windows in one
 * call (call once per window); SQL parsing. */
typedef enum nqe_window_func_ex { /* 0..7: the values of nqe_window_func, same meaning */
    NQE_WINX_ROW_NUMBER = 0,
    NQE_WINX_RANK = 1,
    NQE_WINX_DENSE_RANK = 2,
    NQE_WINX_COUNT = 3,
    NQE_WINX_SUM = 4,
    NQE_WINX_MIN = 5,
    NQE_WINX_MAX = 6,
    NQE_WINX_AVG = 7,
    NQE_WINX_LAG = 8,
    NQE_WINX_LEAD = 9,
    NQE_WINX_FIRST_VALUE = 10,
    NQE_WINX_LAST_VALUE = 11,
    NQE_WINX_NTILE = 12
} nqe_window_func_ex;
typedef enum nqe_window_frame_ex { /* 0..2: the values of nqe_window_frame */
    NQE_FRAMEX_PARTITION = 0,
    NQE_FRAMEX_ROWS = 1,
    NQE_FRAMEX_RANGE = 2,
    NQE_FRAMEX_ROWS_BETWEEN = 3 /* ROWS BETWEEN start AND end, both offsets from the current row */
} nqe_window_frame_ex;
#define NQE_FRAME_UNBOUNDED_PRECEDING INT64_MIN
#define NQE_FRAME_UNBOUNDED_FOLLOWING INT64_MAX
typedef struct nqe_window_spec_ex {
    int32_t func;        /* nqe_window_func_ex */
    int32_t column;      /* the argument's column; ignored by the ranking functions and NTILE */
    int32_t frame;       /* nqe_window_frame_ex; read by the aggregates, FIRST_VALUE and LAST_VALUE */
    int32_t has_default; /* LAG / LEAD: default_value stands in for a row outside the partition */
    int64_t start, end;  /* ROWS_BETWEEN only: signed offsets from the current row */
    int64_t param;       /* LAG / LEAD: rows back / ahead, >= 0; NTILE: buckets, >= 1 */
    union {
        int64_t i64;
        uint64_t u64;
        double f64;
    } default_value;     /* 8 bytes of the column's dtype */
} nqe_window_spec_ex;    /* sizeof == 48 */
nqe_status nqe_window_execute_ex(nqe_ctx *ctx, const nqe_table *in, const int32_t *partition_cols, int32_t num_partition,
                                 const nqe_sort_key *order_keys, int32_t num_order, const nqe_window_spec_ex *funcs,
                                 int32_t num_funcs, nqe_table **out);

/* ------------------------------------------------------------------ DISTINCT and the set operators
 * SELECT DISTINCT, UNION, INTERSECT and EXCEPT — quirk Q24: the reference has none of them (its
 * JoinType is {Inner, Left, Right, Cross} and its SQL planner knows no DISTINCT and no set
 * operator), so the definition is this project's.
 * TUPLE EQUALITY is the sort's and the window's tie, per key column: Int64 / UInt64 the 64-bit
 * word, Float64 as OrderedFloat (-0.0 = +0.0, every NaN equals every NaN), Boolean the bit, Utf8
 * byte for byte; a NULL equals a NULL, whatever lies under it, and differs from every value; the
 * empty string is a value, not NULL.  Tuples compare position by position: ("a","b") differs
 * from ("ab",""), (1,2) from (2,1).  (The semi and anti joins keep the hash join's relation, Q11:
 * they ignore validity.  This operator does the opposite.)
 * nqe_distinct_execute: the rows of `in` that are the FIRST occurrence (smallest row index) of
 * their tuple over the key columns `cols`, in input order, with every column of `in` taken from
 * that row — payload columns outside `cols` too.  num_cols == 0 with cols == NULL: every column
 * is a key (SELECT DISTINCT *).  Output columns are the selection's compaction of their source:
 * validity preserved, null_count exact, the first row's own bits kept (-0.0 stays -0.0 when it
 * came first).  The result is the same on every run.
 * nqe_set_op_execute: every column is a key; both tables need the same number of columns and the
 * same dtype at every position; neither needs to be duplicate-free.  INTERSECT: the rows of
 * distinct(left) whose tuple occurs in `right`; EXCEPT: the rest — the two partition
 * distinct(left), each in left's order with left's bits and validity.  UNION:
 * distinct(nqe_table_concat(left, right)) bit for bit: left's distinct rows in order, then
 * right's rows not seen before, in order.
 * Errors, all before any launch or allocation, in this order: (1) NULL ctx / in / left / right /
 * out, cols == NULL with num_cols > 0, op outside its enum NQE_ERR_INVALID_ARGUMENT; (2) set op
 * only: a differing column count, then the first differing dtype in column order NQE_ERR_PLAN;
 * (3) num_cols < 0 or more than NQE_MAX_SET_KEYS key columns NQE_ERR_NOT_SUPPORTED; (4) a key
 * index out of range or given twice NQE_ERR_NOT_SUPPORTED (then: a key of dtype NQE_NULLTYPE
 * NQE_ERR_NOT_SUPPORTED, zero columns with zero keys NQE_ERR_PLAN); (5) 2^31 rows or more in the
 * table that is inserted — `in`, `left`, for UNION both together — NQE_ERR_NOT_SUPPORTED; the
 * probed `right` of INTERSECT / EXCEPT has no such limit.  Table memory that cannot be had:
 * NQE_ERR_OUT_OF_MEMORY.  UNION's concatenation reports what nqe_table_concat reports.  Zero rows
 * give a 0-row table with every column.  Nothing is kept between calls.
 * Out of scope: INTERSECT ALL and EXCEPT ALL (multiplicities); count(distinct x); DISTINCT over
 * expressions (the host mirrors make temporary columns, as the window plan does); SQL parsing;
 * sharded forms. */
#define NQE_MAX_SET_KEYS 32
typedef enum nqe_set_op {
    NQE_SET_UNION = 0,
    NQE_SET_INTERSECT = 1,
    NQE_SET_EXCEPT = 2
} nqe_set_op;
nqe_status nqe_distinct_execute(nqe_ctx *ctx, const nqe_table *in, const int32_t *cols, int32_t num_cols, nqe_table **out);
nqe_status nqe_set_op_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, int32_t op, nqe_table **out);

/* ------------------------------------------------------------------ take
 * arrow::compute::take(array, &Int64Array indices, None) over every column
 * (hash_join.rs:239,245): out[j] = in[indices[j]]; `indices` = Int64 column `idx_column` of
 * `idx_table`, no nulls. */
nqe_status nqe_take(nqe_ctx *ctx, const nqe_table *in, const nqe_table *idx_table, int32_t idx_column,
                    nqe_table **out);

/* ------------------------------------------------------------------ synthetic columns
 * Deterministic generators of SURVEY §8d / BASELINE.md §3 so that 10^9-row tables never
 * cross PCIe: u(i,s) = splitmix64(s + i), i = first_row + row.
 *   NQE_SYNTH_ROWID      Int64   i
 *   NQE_SYNTH_UNIFORM    Int64   u(i,seed) mod `modulus`  (+ `base`)
 *   NQE_SYNTH_F64_0_100  Float64 (u(i,seed) >> 11) * 2^-53 * 100.0
 * Writes `n` 8-byte values to the DEVICE buffer `out`. */
typedef enum nqe_synth_kind { NQE_SYNTH_ROWID = 0, NQE_SYNTH_UNIFORM = 1, NQE_SYNTH_F64_0_100 = 2 } nqe_synth_kind;
nqe_status nqe_synth_fill(nqe_ctx *ctx, int32_t kind, uint64_t seed, int64_t first_row, int64_t n,
                          uint64_t modulus, int64_t base, void *out_device);
/* device allocation helpers for hosts that have no device allocator of their own */
nqe_status nqe_device_alloc(nqe_ctx *ctx, size_t bytes, void **out);
nqe_status nqe_device_free(nqe_ctx *ctx, void *ptr);

#ifdef __cplusplus
}
#endif
#endif /* NQE_H */
