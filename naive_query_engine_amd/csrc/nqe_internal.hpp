// nqe_internal.hpp — host-side internals of libnqe_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>

#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <atomic>
#include <vector>

#include "../../include/nqe.h"
#include "aggregate_memo.hpp"
#include "expr_shapes.hpp" // OpAux, SimpleExpr, FastPred, ConjPred, TreePred, ExprInfo, is_word_type
#include "nqe_error.hpp"   // Error, fail

namespace nqe {

#define NQE_HIP_CHECK(expr)                                                                                  \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            ::nqe::fail(_e == hipErrorOutOfMemory ? NQE_ERR_OUT_OF_MEMORY : NQE_ERR_HIP,                     \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                                  \
    } while (0)

inline size_t bitmap_bytes(int64_t n) { return size_t((n + 7) / 8); }
// bitmaps we allocate are padded to whole 64-bit words so kernels may store u64 words
inline size_t bitmap_alloc_bytes(int64_t n) { return size_t((n + 63) / 64) * 8; }

} // namespace nqe

// Device error flag slots (ctx->d_flags[i])
enum { NQE_FLAG_DIV_ZERO = 0, NQE_FLAG_OVERFLOW = 1, NQE_FLAG_TABLE_FULL = 2, NQE_FLAG_OOB = 3, NQE_FLAG_NEED_PARTITION = 4, NQE_FLAG_NEED_LEVEL2 = 5, NQE_FLAG_DENSE_OVERFLOW = 6,
       NQE_FLAG_GROUP_COUNT = 7 /* not an error: the aggregate's group count rides along with the flag read-back */,
       NQE_FLAG_SLAB_OVERFLOW = 8 /* a partition slab of the count-free scatter is full: the host takes the exact form */,
       NQE_FLAG_KEY32_OVERFLOW = 9 /* a group key outside the int32 range met the 12-byte-tuple slab form: the host takes 16-byte tuples */, NQE_NUM_FLAGS = 10 };
// words of the pinned flag mirror past the flags: results a tail kernel sends along with the flag read-back (aggregate.hip: the dense table's
// group count and key range)
constexpr int NQE_FLAG_MIRROR_EXTRA = 8;

// Run-time settings of the aggregate operator (aggregate.hip), read when a context is created: a test hook and the tier trace.  What the A/B
// runs of rounds 2-6 decided is a named constant next to what it sizes (aggregate_common.hpp: FLAG_CHECK_MASK … RANGE_SLOTS_LOG2; aggregate_tail.hpp) or
// simply the code; DESIGN.md §9 "retired switches" lists the measurements.  (The switches the tests flip between calls — NQE_NO_PLAN_HINTS,
// NQE_NO_KEY_SAMPLE, NQE_NO_RANGE_PARTITION, NQE_NO_RANGE_TAIL, NQE_NO_AGG_JIT, NQE_NO_WIDE_DIRECT, NQE_TEST_SLAB_OOM — are read per call
// where they are used.)
struct AggSwitches {
    int tiny_unpack_tiles = 4096;      // NQE_TINY_UNPACK_TILES: tiles between two unpackings of the register kernel's packed row counters (1..4096; a TEST hook: at 4096 the branch first runs beyond ~2 x 10^9 rows)
    bool debug = false;                // NQE_DEBUG=1: the tier decisions on stderr
    void read_environment();
};

struct nqe_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    std::string last_error;

    // caching device allocator: freed blocks are reused by later (stream-ordered) work
    std::multimap<size_t, void *> pool;
    size_t pool_bytes = 0;
    // nqe_ctx_reserve: one block taken from the driver up front and sub-allocated (best fit, free neighbours coalesced): the scratch
    // and output buffers of a FIRST query then cost no hipMalloc (a first hipMalloc of a gigabyte block is a millisecond and more —
    // the reference's run_sql is one-shot, so the first execution is the one that counts).  Reuse is stream-ordered like the pool's.
    char *arena_base = nullptr;
    size_t arena_size = 0, arena_free_bytes = 0;
    std::map<size_t, size_t> arena_free; // offset -> bytes, address-ordered
    size_t live_bytes = 0;

    // per-kernel timing (bench.py roofline leg)
    bool timing = false;
    struct TimingRec {
        std::string name;
        hipEvent_t start, stop;
    };
    std::vector<TimingRec> timings;

    AggSwitches agg_sw;
    // What grouped aggregates remember per query shape (aggregate_memo.hpp; keyed by a hash of the key column's buffer, the row count, the
    // key expression, the predicate and the value columns): the tier an earlier execution ended in — the next execution of the same query
    // over the same table starts there instead of paying for abandoned attempts and their read-backs first — and the value range of a plain
    // integer key column.  Only starting points: every tier checks what it is given, and the column's contents may have changed under the entry.
    nqe::AggMemoTable agg_memo;
    // PK-FK joins whose optimistic one-pass probe failed (some foreign key without its primary key), by (build key column, build
    // rows, probe key column, probe rows): HashJoin::execute builds a fresh join table per call (nqe_hash_join_execute), so the
    // verdict has to outlive the table for the next execution of the same join to go straight to the two-pass form
    std::map<uint64_t, uint8_t> join_hints;
    // run-time specialised expression kernels (expr_jit.hpp: JitCache — worker threads, code objects), created on first use
    std::shared_ptr<void> jit;

    size_t lds_per_block = 160 * 1024; // LDS a workgroup may ask for on this device (hipDeviceProp_t::sharedMemPerBlock)
    std::string arch = "gfx950";      // the device's ISA name (hipRTC target of the run-time specialised kernels)
    int *d_flags = nullptr; // NQE_NUM_FLAGS ints on the device
    int *h_flags = nullptr; // pinned host mirror
    int *h_flags_dev = nullptr; // the mirror's address as seen by kernels (a tail kernel may write it directly)
    // d_flags known to be all zero at the current stream position: set by a read-back that saw only zeros (or a reset), cleared
    // by every kernel launch — lets the next operator skip its reset (one fill launch per operator)
    bool flags_clean = false;
};

namespace nqe {

// A device allocation (owned → returned to the ctx pool) or a borrowed device pointer.
struct DevBuf {
    nqe_ctx *ctx = nullptr;
    void *ptr = nullptr;
    size_t bytes = 0;    // usable size requested
    size_t capacity = 0; // pooled block size
    bool owned = false;
    bool in_arena = false; // a range of the context's reserved block (returned to its free list)
    // the memory belongs to the context's pool (an allocation of ours, or a view into one): its reuse is ordered on the context's
    // stream, so work enqueued on that stream may still be reading it when the last reference goes away.  false: the caller's.
    bool lib_memory = false;
    // borrowed memory the caller has promised to keep alive and unmodified while any table derived from it lives
    // (NQE_TABLE_IMMUTABLE at nqe_table_create_flags): an output may then alias it, as it may alias the library's own buffers
    bool caller_immutable = false;
    ~DevBuf();
};
using BufRef = std::shared_ptr<DevBuf>;
// may an OUTPUT table reference this buffer instead of a copy?  The library's own memory is reference-counted, so an alias keeps
// it alive; borrowed memory is the caller's to free or overwrite the moment the producing call returns — unless promised otherwise.
inline bool buf_shareable(const BufRef &b) { return !b || b->lib_memory || b->caller_immutable; }

BufRef dev_alloc(nqe_ctx *ctx, size_t bytes);
BufRef dev_alloc_zero(nqe_ctx *ctx, size_t bytes);
BufRef dev_borrow(nqe_ctx *ctx, const void *ptr, size_t bytes);
// a sub-range of `parent` (keeps the parent alive)
BufRef dev_view(const BufRef &parent, size_t offset, size_t bytes);
void pool_trim(nqe_ctx *ctx);

// One Arrow array resident in HBM.
struct DevColumn {
    int dtype = NQE_NULLTYPE;
    int64_t length = 0;
    int64_t null_count = 0; // -1 unknown; 0 ⇒ validity may still be present (all ones)
    BufRef values;          // 8 B/row words, packed bits (Boolean), or int32 offsets (Utf8)
    BufRef validity;        // packed bits or null
    BufRef data;            // Utf8 bytes
    int64_t data_length = 0;

    const uint64_t *words() const { return values ? static_cast<const uint64_t *>(values->ptr) : nullptr; }
    const uint8_t *bits() const { return values ? static_cast<const uint8_t *>(values->ptr) : nullptr; }
    const uint8_t *valid() const { return validity ? static_cast<const uint8_t *>(validity->ptr) : nullptr; }
    bool shareable() const { return buf_shareable(values) && buf_shareable(validity) && buf_shareable(data); }
};

} // namespace nqe

inline uint64_t nqe_next_table_uid() {
    static std::atomic<uint64_t> counter{1};
    return counter.fetch_add(1, std::memory_order_relaxed);
}
struct nqe_table {
    nqe_ctx *ctx = nullptr;
    std::vector<nqe::DevColumn> cols;
    int64_t rows = 0;
    // identity of this handle: what a context remembers about a query (aggregate plan hints, key ranges) is keyed by it as well as by
    // the buffers — a NEW table over the same device memory (a caller refilling its buffers, the pool handing a block out again)
    // holds other data and starts from nothing instead of from the previous table's plan
    uint64_t uid = nqe_next_table_uid();
};

namespace nqe {

// ---- code objects ------------------------------------------------------------------------
// HIP loads a translation unit's code object (1-5 MB each here) on the FIRST launch of one of its kernels: 2-5 ms that the first
// query of a process would pay per operator family (the reference's run_sql is one-shot, db.rs:24-37).  Every translation unit
// registers one of its kernels at static-initialisation time; nqe_ctx_create asks the runtime for that kernel's attributes, which
// loads the unit for the context's device (NQE_LAZY_MODULES=1 leaves the loading to the first launch).
void register_module_probe(const void *kernel);
#define NQE_MODULE_PROBE(kernel) static const bool nqe_module_probe_ = (nqe::register_module_probe(reinterpret_cast<const void *>(&kernel)), true)

// ---- launch helpers ---------------------------------------------------------------------
struct TimerScope {
    nqe_ctx *ctx;
    size_t idx = size_t(-1);
    TimerScope(nqe_ctx *c, const char *name) : ctx(c) {
        if (ctx->timing) {
            nqe_ctx::TimingRec r;
            r.name = name;
            NQE_HIP_CHECK(hipEventCreate(&r.start));
            NQE_HIP_CHECK(hipEventCreate(&r.stop));
            NQE_HIP_CHECK(hipEventRecord(r.start, ctx->stream));
            ctx->timings.push_back(r);
            idx = ctx->timings.size() - 1;
        }
    }
    ~TimerScope() {
        if (idx != size_t(-1)) (void)hipEventRecord(ctx->timings[idx].stop, ctx->stream);
    }
};

template <typename K, typename... Args>
inline void launch(nqe_ctx *ctx, const char *name, K kernel, dim3 grid, dim3 block, size_t shmem, Args... args) {
    TimerScope t(ctx, name);
    ctx->flags_clean = false;
    hipLaunchKernelGGL(kernel, grid, block, shmem, ctx->stream, args...);
    NQE_HIP_CHECK(hipGetLastError());
}

// grid for a streaming kernel: enough blocks to fill the chip, grid-stride the rest
inline int stream_grid(nqe_ctx *ctx, int64_t work_items, int per_block, int blocks_per_cu = 8) {
    int64_t need = (work_items + per_block - 1) / per_block;
    int64_t cap = int64_t(ctx->num_cus) * blocks_per_cu;
    if (need < 1) need = 1;
    return int(need < cap ? need : cap);
}

void flags_reset(nqe_ctx *ctx);
// expr.hip: waits for the run-time specialisations being compiled for this context
void jit_wait(nqe_ctx *ctx);
// synchronises the stream, returns flag values
void flags_read(nqe_ctx *ctx, int out[NQE_NUM_FLAGS]);
// the same when the last kernel of the stream copied the flags into the pinned mirror itself (no device-to-host copy)
void flags_read_mirrored(nqe_ctx *ctx, int out[NQE_NUM_FLAGS]);
void throw_on_flags(nqe_ctx *ctx);

// Host wait for the stream.  The operators wait for a handful of bytes (flags, a row count) right behind kernels that run for
// microseconds to a few milliseconds, and an interrupt-driven hipStreamSynchronize adds its wake-up latency to every such step:
// poll the stream for the first milliseconds, then block.
inline void sync(nqe_ctx *ctx) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        hipError_t e = hipStreamQuery(ctx->stream);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) NQE_HIP_CHECK(e);
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
    }
    NQE_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

template <typename T> inline T read_scalar(nqe_ctx *ctx, const T *dptr) {
    T v;
    NQE_HIP_CHECK(hipMemcpyAsync(&v, dptr, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    sync(ctx);
    return v;
}

// ---- column utilities (columns.hip) -----------------------------------------------------
DevColumn make_word_column(nqe_ctx *ctx, int dtype, int64_t n, bool with_validity);
DevColumn make_bool_column(nqe_ctx *ctx, int64_t n, bool with_validity);
// out[j] = in[idx[j]] for every column (arrow take); idx are int64 row numbers on the device
DevColumn take_column(nqe_ctx *ctx, const DevColumn &src, const int64_t *idx, int64_t m);
// Utf8 gather; idx < 0 emits NULL when allow_null_idx (else out of bounds)
DevColumn take_utf8(nqe_ctx *ctx, const DevColumn &src, const int64_t *idx, int64_t m, bool allow_null_idx);
BufRef iota_i64(nqe_ctx *ctx, int64_t first, int64_t n);
DevColumn slice_column(nqe_ctx *ctx, const DevColumn &src, int64_t off, int64_t len);
DevColumn concat_columns(nqe_ctx *ctx, const std::vector<const DevColumn *> &parts);
// dst bits [dst_off, dst_off + n) |= src bits [0, n) (src == nullptr: ones); dst zero-initialised and padded to whole words + 8 bytes
void bitmap_place(nqe_ctx *ctx, const uint8_t *src, uint64_t *dst, int64_t dst_off, int64_t n);
// dst[i] = src[i] - src[0] + delta for i in [0, n]: the offsets of a Utf8 part moved behind `delta` bytes of earlier parts
void utf8_rebase_offsets(nqe_ctx *ctx, const int32_t *src, int64_t n, int32_t delta, int32_t *dst);
// exclusive prefix sum of n uint32 counts into uint64 offsets (offsets[n] = total); device arrays
void exclusive_scan_u32_to_u64(nqe_ctx *ctx, const uint32_t *counts, uint64_t *offsets, int64_t n);
void exclusive_scan_u32_inplace(nqe_ctx *ctx, uint32_t *data, int64_t n);
// packs one byte per row (0/1) into an LSB-first bitmap
void pack_bytes_to_bits(nqe_ctx *ctx, const uint8_t *bytes, int64_t n, uint64_t *bitmap_words);
// stable LSD radix sort of (key, value) pairs by 64-bit key; keys_out/vals_out are device arrays of n
void radix_sort_pairs_u64(nqe_ctx *ctx, const uint64_t *keys_in, const uint32_t *vals_in, uint64_t *keys_out,
                          uint32_t *vals_out, int64_t n, bool signed_order);

// ---- the ORDER BY permutation (order_by.hip), shared with the window operator (window.hip)
// the buffers of one permutation build; `cur` is the u32 permutation (output position -> input row), null while it is the identity
struct SortPermutation {
    BufRef keys_in, keys_out, iota, perm[2], order;
    const uint32_t *cur = nullptr;
};
// The stable multi-key permutation of nqe_sort_execute: keys[0] most significant, built least significant key first.  The caller has
// checked the keys (column indices, dtypes) and that 1 < in->rows < 2^32.  Returns hold->cur; `hold` keeps the buffers alive.
const uint32_t *build_sort_permutation(nqe_ctx *ctx, const nqe_table *in, const nqe_sort_key *keys, int32_t num_keys, SortPermutation *hold);

// ---- Utf8 keys (strings.hip): exact string → representative-row encoding
struct Utf8Dict {
    BufRef slots;      // int64 representative build row per slot, -1 = empty
    uint32_t cap = 0;
    int shift = 0;
    DevColumn build;   // the encoded (build) column: its strings back the table
};
// codes[i] = representative row of string i (Int64 column sharing the strings' validity)
DevColumn utf8_encode_build(nqe_ctx *ctx, const DevColumn &col, Utf8Dict *dict);
// codes[i] = representative BUILD row of the equal build string, or a negative value that matches nothing
DevColumn utf8_encode_probe(nqe_ctx *ctx, const DevColumn &col, const Utf8Dict &dict);

// ---- expressions (expr.hip; the analysis itself: expr_plan.hpp) -------------------------------------------------------------
// (the shapes handed to the consumers of expressions — SimpleExpr, FastPred, ConjPred, TreePred, ExprInfo — are in expr_shapes.hpp)
// false: the tree does not fit (nullable / non-word columns, NULL or Utf8 literals, more columns or instructions, a deeper stack, a
// divisor that is not a literal other than 0 and -1 — anything that could raise a device flag)
bool match_tree_pred(const nqe_table *in, const nqe_expr_node *nodes, int n, TreePred *out);
// recognises the shape (see expr_plan.hpp); cols[CONJ_MAX] receive the tested column of every test
bool match_conj(const nqe_table *in, const nqe_expr_node *nodes, int n, ConjPred *out, int *cols);
// FastPred "bit r of a non-null Boolean bitmap is set"
FastPred bitmap_fast_pred();
// returns false when the SimpleExpr is not a single Int64/UInt64/Float64 compare against a literal
bool make_fast_pred(const SimpleExpr &pe, FastPred *fp);

// type-checks (IntervalError / NotSupported exactly where the reference raises them) and
// recognises the fusable shape
ExprInfo analyze_expr(const nqe_table *in, const nqe_expr_node *nodes, int n);
// general evaluator: one streaming kernel per binary node, literals kept scalar
DevColumn evaluate_expr(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, int n);

// ---- filter (selection.hip) ---------------------------------------------------------------
struct KeepMask {
    BufRef keep;          // bit i = row i is emitted (pred true OR pred NULL)
    BufRef pvalid;        // predicate validity (null if predicate has no nulls)
    BufRef tile_offsets;  // uint64 per 4096-row tile (exclusive), [ntiles] = total
    int64_t n = 0;        // rows covered
    int64_t ntiles = 0;
    int64_t total = 0;    // emitted rows
    mutable BufRef kept_idx; // int64 source row per emitted row (-1: NULL row from a NULL predicate); built on demand for Utf8
};
// source-row list of the emitted rows (cached in the mask)
const int64_t *kept_rows(nqe_ctx *ctx, const KeepMask &km);
KeepMask build_keep_mask(nqe_ctx *ctx, const DevColumn &pred, int64_t n_rows);
// predicate given as a fused SimpleExpr over `in`
KeepMask build_keep_mask_simple(nqe_ctx *ctx, const nqe_table *in, const SimpleExpr &pred);
DevColumn compact_column(nqe_ctx *ctx, const DevColumn &src, const KeepMask &km);
// out row r (r-th kept row i) = src[gidx[i]]
DevColumn compact_gather_column(nqe_ctx *ctx, const DevColumn &src, const uint32_t *gidx, const KeepMask &km);
// scans the per-tile counts into km.tile_offsets and reads back km.total
KeepMask finish_mask(nqe_ctx *ctx, KeepMask km, BufRef tile_counts);
// Utf8 comparison; a null column pointer means that side is the literal (lit, lit_null)
DevColumn utf8_compare(nqe_ctx *ctx, int op, const DevColumn *lcol, const std::string &llit, bool llit_null, const DevColumn *rcol,
                       const std::string &rlit, bool rlit_null, int64_t n);
DevColumn utf8_literal_column(nqe_ctx *ctx, const std::string &lit, bool lit_null, int64_t n);
// string_fn.hip: one string function of an NQE_EXPR_STRING node (`op`: TRIM, LTRIM, RTRIM, CHARACTER_LENGTH, LOWER, UPPER or REVERSE of
// nqe_unary_operator, checked by the parser) over the Utf8 column `src`; Utf8, or Int64 for CHARACTER_LENGTH, with src's validity
DevColumn string_fn(nqe_ctx *ctx, int op, const DevColumn &src);
// (string_fn.hip) the operand's validity as the result's — shared (reference-counted) when an output may alias it, else copied — with its
// null_count; the operand's offsets as the result's, shared or copied likewise; a well-formed Utf8 column of no rows
void carry_validity(nqe_ctx *ctx, const DevColumn &src, DevColumn *out);
BufRef carry_offsets(nqe_ctx *ctx, const DevColumn &src);
DevColumn empty_utf8(nqe_ctx *ctx);
// string_args.hip: one function of an NQE_EXPR_STRING_ARGS node (quirk Q26) over the Utf8 column `src`.  An Int64 argument is a column
// or a literal (`col` null: `lit`, `lit_null`); REPLACE's `from` and `to` are Utf8 literals.
struct StrIntArg {
    const DevColumn *col = nullptr;
    int64_t lit = 0;
    bool lit_null = false;
};
DevColumn string_substr(nqe_ctx *ctx, const DevColumn &src, const StrIntArg &start, const StrIntArg &len);
DevColumn string_repeat(nqe_ctx *ctx, const DevColumn &src, const StrIntArg &n);
DevColumn string_replace(nqe_ctx *ctx, const DevColumn &src, const std::string &from, bool from_null, const std::string &to, bool to_null);
// string_match.hip: an NQE_EXPR_STRING_MATCH node (quirk Q27) over the Utf8 column `src`: `op` is a nqe_match_operator, the pattern a Utf8
// literal the parser has checked; Boolean, or Int64 for STRPOS, with src's validity (all NULL under a NULL pattern)
DevColumn string_match(nqe_ctx *ctx, int op, const DevColumn &src, const std::string &pattern, bool pattern_null);
// (string_args.hip) `lens` (n + 1 counts in out->values) become the offsets and the data buffer is allocated — after the 64-bit total has been
// read back and found to fit (more than 2^31-1 bytes: NQE_ERR_ARROW, nothing allocated).  Returns the total; 0: nothing to copy, and
// `out` holds n empty rows (utf8_empty_rows: offsets of zeros, no bytes, nothing launched).
uint32_t utf8_size_output(nqe_ctx *ctx, const BufRef &total64, int64_t n, DevColumn *out);
void utf8_empty_rows(nqe_ctx *ctx, int64_t n, DevColumn *out);
// conditional.hip: an NQE_EXPR_CONDITIONAL node (quirk Q28).  An operand is a column or, when `col` is null, a literal; Utf8 operands of
// COALESCE, NULLIF and IF are columns (the caller expands literals).  `a` is the one operand of NOT / IS_NULL / IS_NOT_NULL; a and b are
// COALESCE's and NULLIF's; IF takes the condition `c` and t = a, e = b.  `dtype` is the value operands' (the parser has checked them).
struct CondArg {
    const DevColumn *col = nullptr;
    uint64_t lit = 0;
    bool lit_null = false;
};
DevColumn conditional(nqe_ctx *ctx, int op, int dtype, const CondArg &a, const CondArg &b, const CondArg &c, int64_t n);
// cast.hip: an NQE_EXPR_CAST node (quirk Q29) over the column `src` (the caller expands literals) to the nqe_dtype `to`; the parser has
// refused Float64 -> Utf8.  An infallible cast carries src's validity, a fallible one a buffer of its own (include/nqe.h).
DevColumn cast_column(nqe_ctx *ctx, const DevColumn &src, int to);
// general tree `nodes` over the rows of `km`, compacted in the same pass; false = does not fit the stack machine
bool evaluate_expr_compacted(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, int n, const KeepMask &km, DevColumn *result);
// the whole projection list behind a selection in ONE run-time specialised kernel (expr_jit.hpp); false when the list does not fit it
// or its kernel is not compiled yet (the caller then takes the per-expression path)
bool project_specialised(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, const int32_t *expr_offsets, int num_exprs, const KeepMask &km,
                         std::vector<DevColumn> *out);
// selection + projection in one run-time specialised pass (tree predicate, inputs without NULLs, word-typed outputs); false: take the mask + compaction path
bool select_project_fused(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int pred_nodes, const nqe_expr_node *nodes, const int32_t *expr_offsets,
                          int num_exprs, std::vector<DevColumn> *result, int64_t *total_out);
// the streaming aggregate of `val_col` grouped by a key `… % m` (any fault-free integer chain or tree ending in a literal modulus), under an
// optional predicate, through the lean run-time specialised kernel (expr.hip); on success *partials holds every workgroup's table for
// aggregate.hip's merge kernel
bool aggregate_tree_specialised(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int pred_nodes, const nqe_expr_node *group, int group_nodes,
                                int val_col, int grid, BufRef *partials, uint32_t *span_out, int64_t *bias_out, bool dry_run = false);
// evaluates `e` over `in` and compacts the result in the same pass
DevColumn compact_simple_expr(nqe_ctx *ctx, const nqe_table *in, const SimpleExpr &e, const KeepMask &km);
// hash_join.hip: the exact null_count of every column of `out` that has a validity buffer and a null_count still unknown (< 0) — one
// counting launch per such column under `label`, one read-back for all of them; true when it waited for the stream
bool count_nulls_exact(nqe_ctx *ctx, nqe_table *out, const char *label = "join_outer_null_count");
// aggregate.hip: fails as nqe_aggregate_execute would for this aggregate list (count, function, column index, column type); launches nothing
void check_aggregates(const nqe_table *in, const nqe_aggregate *aggs, int naggs);

} // namespace nqe

// wraps a C entry point: exceptions → status + ctx->last_error
#define NQE_API_BEGIN(ctxptr)                                                                                \
    nqe_ctx *_api_ctx = (ctxptr);                                                                            \
    try {                                                                                                    \
        if (_api_ctx) (void)hipSetDevice(_api_ctx->device);
#define NQE_API_END()                                                                                        \
    }                                                                                                        \
    catch (const ::nqe::Error &e) {                                                                          \
        if (_api_ctx) _api_ctx->last_error = e.msg;                                                          \
        ::nqe::set_global_error(e.msg);                                                                      \
        return (nqe_status)e.code;                                                                           \
    }                                                                                                        \
    catch (const std::bad_alloc &) {                                                                         \
        if (_api_ctx) _api_ctx->last_error = "host out of memory";                                           \
        return NQE_ERR_OUT_OF_MEMORY;                                                                        \
    }                                                                                                        \
    catch (const std::exception &e) {                                                                        \
        if (_api_ctx) _api_ctx->last_error = e.what();                                                       \
        return NQE_ERR_OTHERS;                                                                               \
    }                                                                                                        \
    return NQE_OK;

namespace nqe {
void set_global_error(const std::string &msg);
}
