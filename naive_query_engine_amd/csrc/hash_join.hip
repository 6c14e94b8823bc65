// hash_join.hip — HashJoin::execute = build() + probe() (reference: src/physical_plan/hash_join.rs:124-254).
//
// Reference: HashMap<XxHash64(key), Vec<build row>> chains, per probe row a chain walk with an
// equality re-check (:86-101), then `take` of every left column by build index and every right
// column by probe index (:237-246).  Output order: probe-row-major, duplicate build keys in
// ascending build row.
//
// Device design
//   build : stable radix sort of (key, build row) → equal keys adjacent, rows ascending;
//           run heads → unique keys with (start, count) into the sorted row list `perm`;
//           open-addressing table of 16-byte slots {key, start<<32|count} (Fibonacci hash, one
//           128-bit load per probe step).  The XxHash64 value itself is unobservable in results
//           (equality is re-checked), so any hash is parity-safe.  When every build key is
//           unique the slot stores the build row directly (no `perm` indirection).
//   probe : pass 1 looks every probe key up once and records its (start,count) word plus
//           per-tile match counts; an exclusive scan gives each 4096-row tile its output base;
//           pass 2 re-reads the recorded words, ranks rows inside the tile with wave scans and
//           writes all output columns (gather of left columns by build row, copy of right
//           columns) in probe order — exactly the order of the reference's outer_pos/inner_pos.
// Key validity is ignored (quirk Q11): raw 8-byte slot values are compared.
//
// Map: build form → fields of nqe_join_table (hash_join_table.hpp) → probe form that reads them
//   build_unique_dense   (unique keys, dense range; table laid out by build_dense_partitioned / _scatter / _atomic):
//                        direct, dense, dense_min/span; with plain payloads also presence, dense_cols/_packed/_base, dense_payload,
//                        dense_full → probe_dense_payload (plain probe side), else probe_unique through `dense` (lookup probe)
//   build_hashed_unique  (unique keys, sparse): direct, slots/cap/shift; one plain payload column: slotsp + pis_col with pp (packed
//                        pairs) or filler (16-byte pairs); otherwise the check form → probe_unique (pairs / packed / coop lookups)
//   build_sorted         (duplicate keys, or an empty build side): perm, slots/cap/shift, direct = no duplicates after all;
//                        build_sorted_dense adds dense (+ ustart, or the payload fields above when unique); sorted_cols for
//                        duplicates → probe_duplicates (direct: probe_unique / probe_dense_payload as above)
// probe_duplicates and the outer probe (probe_outer, quirk Q19, over every build form) are the two entries of ONE count → scan →
// expand-and-write path, probe_expand: its column list is hash_join_expand_plan.hpp's (plain C++), its kernels one body per pass
// (expand_count / expand_write in hash_join_probe_kernels.hpp; the outer entries' wrappers in hash_join_outer_kernels.hpp).
// (the semi / anti probe, quirk Q22, reads the same fields for existence alone: its map from build form to existence form is at probe_semi)
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "hash_join_expand_plan.hpp"
#include "hash_join_semi_kernels.hpp" // (and through it hash_join_outer_kernels.hpp, hash_join_probe_kernels.hpp, hash_join_build_kernels.hpp, hash_join_table.hpp)

// which build rows have matched so far (quirk Q19): bit `start` per matched key, left_rows bits in 32-bit words, bound to one join table
struct nqe_join_marks {
    nqe_ctx *ctx = nullptr;
    const nqe_join_table *table = nullptr;
    int64_t rows = 0;
    nqe::BufRef bits;
};

namespace nqe {

namespace {

void check_key_types(int ldt, int rdt) {
    auto joinable = [](int d) { return d == NQE_INT64 || d == NQE_UINT64 || d == NQE_UTF8; };
    if (!joinable(ldt)) fail(NQE_ERR_NOT_IMPLEMENTED, "NotImplemented: join key type (hash_join.rs:161)");
    if (rdt < 0) return;
    if (!joinable(rdt)) fail(NQE_ERR_NOT_IMPLEMENTED, "NotImplemented: join key type (hash_join.rs:232)");
    if (rdt != ldt) fail(NQE_ERR_NOT_SUPPORTED, "join key types differ (downcast unwrap panics, hash_join.rs:83)");
}

// ---- small helpers shared by the build and probe forms
// a plain 8-byte column without validity: what the key-ordered, slot-carried and sorted payload copies and the fused writes take
bool is_plain_word(const DevColumn &c) { return is_word_type(c.dtype) && !c.validity; }
// XOR that makes unsigned order the column's own order (Int64: the sign bit)
uint64_t order_flip(int dtype) { return dtype == NQE_INT64 ? 0x8000000000000000ull : 0ull; }
// slots of an open-addressing table for `entries` keys at load <= 1/2 (a power of two >= 64); *shift: of the Fibonacci hash
uint32_t table_capacity(uint64_t entries, int *shift) {
    uint32_t cap = 64;
    while (uint64_t(cap) < 2ull * entries) cap <<= 1;
    int lg = 0;
    while ((1u << lg) < cap) ++lg;
    *shift = 64 - lg;
    return cap;
}
// a direct-address table over the key range pays: at most 4 entries per row (span 0 = the range wrapped around)
bool dense_eligible(uint64_t span, int64_t n) { return span != 0 && span <= std::max<uint64_t>(4ull * uint64_t(n), 1024ull) && span < (1ull << 31); }
// the row numbers 0 .. rows-1 as an Int64 column: gathered like a payload they give the reference's outer_pos / inner_pos for Utf8 `take`
DevColumn rowid_column(nqe_ctx *ctx, int64_t rows) {
    DevColumn c;
    c.dtype = NQE_INT64;
    c.length = rows;
    c.values = iota_i64(ctx, 0, rows);
    return c;
}
// the build key of a match is bit-identical to the probe key: the probe key column stands in for it (validity comes from the
// build column, which has none where this is used) and is copied coalesced instead of gathered
DevColumn as_build_key(const DevColumn &probe_key) {
    DevColumn c = probe_key;
    c.validity = nullptr;
    c.null_count = 0;
    return c;
}
KeepMask new_keep_mask(nqe_ctx *ctx, int64_t n, BufRef *counts) {
    KeepMask km;
    km.n = n;
    km.ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    km.keep = dev_alloc(ctx, size_t((n + 63) / 64) * 8 + 8);
    *counts = dev_alloc(ctx, size_t(km.ntiles + 1) * 4);
    return km;
}
// the output may reference the probe table's buffers only where an alias keeps them alive (the library's own memory) or the
// caller has promised to (NQE_TABLE_IMMUTABLE); borrowed columns are copied — the caller may free them once the join returned.
// NQE_JOIN_NO_SHARED_PROBE_COLUMNS (read per call: bench.py times both forms) turns the sharing off.
bool share_probe_allowed(const nqe_table *right) {
    if (getenv("NQE_JOIN_NO_SHARED_PROBE_COLUMNS") != nullptr) return false;
    for (auto &c : right->cols)
        if (!c.shareable()) return false;
    return true;
}
// the build-side key column of an equi-join's output can alias the probe-side one: plain integer keys of one type, where equal
// means identical bits (Float64 keys compare -0.0 == 0.0 with different bits; Utf8 keys are not 8-byte words)
bool share_key_column(const DevColumn &left_key, const DevColumn &right_key) {
    return left_key.dtype == right_key.dtype && (left_key.dtype == NQE_INT64 || left_key.dtype == NQE_UINT64) && !left_key.validity &&
           !right_key.validity;
}
// what the context remembers of a join whose all-match probe failed (the table itself may be a fresh one: nqe_hash_join_execute
// builds per call): FNV-1a over the two key buffers' addresses and lengths
uint64_t join_hint_key(const nqe_join_table *jt, const DevColumn &rk, int64_t n) {
    uint64_t h = 1469598103934665603ull;
    const DevColumn &lkc = jt->left_cols[size_t(jt->left_key)];
    const void *lp = lkc.values ? lkc.values->ptr : nullptr, *rp = rk.values->ptr;
    const int64_t lrows = lkc.length;
    auto mix = [&](const void *p, size_t nb) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < nb; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    mix(&lp, sizeof(lp));
    mix(&lrows, sizeof(lrows));
    mix(&rp, sizeof(rp));
    mix(&n, sizeof(n));
    return h;
}

// ================================================================ build
// ---- sort-free build for unique keys (kernels: hash_join_build_kernels.hpp).  What its one round trip measures:
struct KeyRanges {
    bool payload_plain = false; // plain key, and every payload column is a plain word column
    std::vector<int> cols;      // the measured columns: [0] = the key (-1), then the integer payload columns (only when payload_plain)
    std::vector<uint64_t> mm;   // min, max of cols[k] at [2k], [2k + 1] (payloads: order-flipped)
    uint64_t kmin = 0, kmax = 0;
    bool ascending = false;     // (nearly) ascending keys: fewer than one descent per 64 rows
    BufRef scratch;             // the device words, held until the build returns (a released block would be handed out again)
};
KeyRanges measure_ranges(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *left, const DevColumn &kc, bool plain_key) {
    const int64_t n = left->rows;
    KeyRanges kr;
    kr.payload_plain = plain_key;
    for (size_t ci = 0; ci < left->cols.size(); ++ci)
        if (int(ci) != jt->left_key) kr.payload_plain = kr.payload_plain && is_plain_word(left->cols[ci]);
    kr.cols.push_back(-1);
    if (kr.payload_plain)
        for (size_t ci = 0; ci < left->cols.size(); ++ci)
            if (int(ci) != jt->left_key && (left->cols[ci].dtype == NQE_INT64 || left->cols[ci].dtype == NQE_UINT64)) kr.cols.push_back(int(ci));
    const size_t K = kr.cols.size();
    BufRef mm = kr.scratch = dev_alloc(ctx, K * 16 + 8); // [K mins][K maxs][descents of the key]
    NQE_HIP_CHECK(hipMemsetAsync(mm->ptr, 0xFF, K * 8, ctx->stream));
    NQE_HIP_CHECK(hipMemsetAsync(static_cast<char *>(mm->ptr) + K * 8, 0, K * 8 + 8, ctx->stream));
    MinMaxCols mc;
    std::memset(&mc, 0, sizeof(mc));
    for (size_t k = 0; k < K; ++k) {
        const DevColumn &c = kr.cols[k] < 0 ? kc : left->cols[size_t(kr.cols[k])];
        mc.src[k] = c.words();
        mc.flip[k] = kr.cols[k] >= 0 ? order_flip(c.dtype) : 0ull; // the key range is taken unsigned
    }
    launch(ctx, "join_build_minmax", minmax_cols_kernel, dim3(unsigned(std::min<int64_t>(n >= (int64_t(1) << 22) ? 4 * ctx->num_cus : 256, (n + 255) / 256)), unsigned(K)), dim3(256), 0, mc, n,
           (unsigned long long *)mm->ptr, (unsigned long long *)mm->ptr + K, (unsigned long long *)mm->ptr + 2 * K);
    std::vector<uint64_t> mmraw(K * 2 + 1);
    NQE_HIP_CHECK(hipMemcpyAsync(mmraw.data(), mm->ptr, K * 16 + 8, hipMemcpyDeviceToHost, ctx->stream));
    sync(ctx);
    // (nearly) ascending keys: the scatter / finish form is then coalesced at any size
    kr.ascending = getenv("NQE_JOIN_NO_ASCENDING") == nullptr && mmraw[K * 2] * 64 <= uint64_t(n);
    kr.mm.resize(K * 2);
    for (size_t k = 0; k < K; ++k) kr.mm[2 * k] = mmraw[k], kr.mm[2 * k + 1] = mmraw[K + k];
    kr.kmin = kr.mm[0], kr.kmax = kr.mm[1];
    return kr;
}

// ---- dense keys: the direct-address table, + key-ordered payload columns and the presence bitmap when everything is plain
struct DensePlan {
    uint64_t kmin = 0, span = 0;
    BufRef dense, presence;
    bool with_payload = false;
    DensePayload dp;
    std::vector<BufRef> cols; // per left column: its key-ordered copy, the packing (nqe_join_table::dense_packed) and its base
    std::vector<int> packed;
    std::vector<uint64_t> base;
    // the paths that scatter into the tables zero them first; the two-level partitioned build writes every entry itself
    std::vector<std::pair<BufRef, size_t>> to_zero;
    bool zeroed = false;
    void zero_tables(nqe_ctx *ctx) {
        if (zeroed) return;
        for (auto &z : to_zero) NQE_HIP_CHECK(hipMemsetAsync(z.first->ptr, 0, z.second, ctx->stream));
        zeroed = true;
    }
};
// allocates the tables and picks each payload column's packing from its measured range
void plan_dense_payload(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *left, const KeyRanges &kr, DensePlan &pl) {
    const size_t ncols = left->cols.size();
    const uint64_t span = pl.span;
    pl.dense = dev_alloc(ctx, size_t(span) * 4);
    pl.presence = dev_alloc(ctx, size_t((span + 63) / 64) * 8);
    pl.to_zero = {{pl.dense, size_t(span) * 4}, {pl.presence, size_t((span + 63) / 64) * 8}};
    std::memset(&pl.dp, 0, sizeof(pl.dp));
    pl.cols.resize(ncols);
    pl.packed.assign(ncols, 0);
    pl.base.assign(ncols, 0);
    pl.with_payload = kr.payload_plain && span * 8 * ncols <= (size_t(8) << 30) && ncols <= size_t(MAX_JOIN_COLS);
    if (!pl.with_payload) return;
    DensePayload &dp = pl.dp;
    for (size_t ci = 0; ci < ncols; ++ci) {
        if (int(ci) == jt->left_key) continue;
        const DevColumn &pc = left->cols[ci];
        int packed = 0;
        for (size_t k = 1; k < kr.cols.size(); ++k)
            if (kr.cols[k] == int(ci) && kr.mm[2 * k + 1] - kr.mm[2 * k] <= 0xffffffffull) { // value range within 32 bits → uint32 offsets
                // … within 25 bits → exactly as many bits per entry as the range needs: the smaller the key-ordered table, the more
                // of the probe's gathers hit the 4 MB L2 (10^6 keys of a 20-bit attribute: 2.5 MB instead of 4)
                const uint64_t range = kr.mm[2 * k + 1] - kr.mm[2 * k];
                int bits = 2;
                while (bits < 32 && (range >> bits) != 0) ++bits;
                packed = bits > 25 ? 1 : bits; // <= 25 bits: any entry lies inside one unaligned 4-byte window
                pl.base[ci] = kr.mm[2 * k] ^ order_flip(pc.dtype);
            }
        pl.packed[ci] = packed;
        const size_t col_bytes = packed >= 2 ? size_t((span + 63) / 64) * 8 * size_t(packed) + 16 // whole 64-entry groups (dense_finish_kernel)
                                             : (packed ? size_t(span) * 4 + 8 : size_t(span) * 8);
        pl.cols[ci] = dev_alloc(ctx, col_bytes);
        if (packed) pl.to_zero.push_back({pl.cols[ci], col_bytes});
        dp.src[dp.n] = pc.words();
        dp.dst[dp.n] = pl.cols[ci]->ptr;
        dp.base[dp.n] = pl.base[ci];
        dp.packed[dp.n] = pl.packed[ci];
        dp.n++;
    }
}

// ---- partitioned form (see part_build_* in hash_join_build_kernels.hpp): the shape of its passes
struct PartPlan {
    PartBuild pb;
    bool two_level = false; // part_build_split / part_build_fill instead of the place pass
    int bins = 0;           // fine bins of the two-level form
    int rpt = 1;            // rows per thread of the scatter
    int64_t tile = 0;       // = PB_BLOCK * rpt
    bool lds_ok = false;    // the scatter tile fits this device's LDS
    int twp = 0;            // words of a key-ordered record {row + 1, payload words} (even: 16-byte aligned), one-level form with payload
};
PartPlan plan_partitions(nqe_ctx *ctx, const DevColumn &kc, int64_t n, const DensePlan &pl) {
    PartPlan pp;
    const uint64_t span = pl.span;
    const int nc = pl.with_payload ? pl.dp.n : 0;
    constexpr int slice_kb = 3072; // table bytes per partition (4-byte entries: 1.35 ms per 10^8 rows at 3 MB, 1.8 at 6, 2.5 at 24; 16-byte records: 2.1 either way)
    PartBuild &pb = pp.pb;
    std::memset(&pb, 0, sizeof(pb));
    int shift = 10; // the widest slice of 4 + 8 nc bytes per entry within slice_kb, and no more than PB_MAX_PARTS of them
    while (shift < 31 && (uint64_t(2) << shift) * uint64_t(4 + 8 * nc) <= uint64_t(slice_kb) * 1024) ++shift;
    while (((span - 1) >> shift) + 1 > uint64_t(PB_MAX_PARTS)) ++shift;
    // two-level form (part_build_split / part_build_fill): at most one payload word, a key range of at most PB_MAX_PARTS x
    // 2^fine_log2 fine bins (2.7 x 10^8 keys).  NQE_JOIN_PART_ONE_LEVEL=1 (read per call): the place pass (A/B)
    pp.two_level = nc <= 1 && span <= (uint64_t(PB_MAX_FINE) << PB_FILL_LOG2) && getenv("NQE_JOIN_PART_ONE_LEVEL") == nullptr &&
                   size_t(PB_FILL_KEYS) * size_t(4 + 8 * nc) + 4096 <= ctx->lds_per_block && size_t(PB_MAX_FINE) * 4 <= ctx->lds_per_block;
    pp.bins = pp.two_level ? int(((span - 1) >> PB_FILL_LOG2) + 1) : 0;
    if (pp.two_level) {
        // fine bins per partition (at most 64): as few partitions as keep about one workgroup of the second scatter per CU —
        // the first scatter slows down with its partition count (10^8 rows + a payload: 0.77 ms into 191 partitions, 0.86 into
        // 382, 1.09 into 763), the second one hardly cares how many bins a partition has (profiles/r06/probe_build_fine_bins.txt:
        // 10^8 keys 64 bins x 191 partitions 2.49 ms, 32 x 382 2.60; 2^25 keys 16 x 256 0.91 / 0.51, 32 x 128 0.91 / 0.57)
        int fl = PB_FINE_LOG2_MAX;
        auto parts_at = [&](int l) { return ((span - 1) >> (PB_FILL_LOG2 + l)) + 1; };
        while (fl > 0 && parts_at(fl) * 10 < uint64_t(ctx->num_cus) * 7 && parts_at(fl - 1) <= uint64_t(PB_MAX_PARTS)) --fl;
        while (parts_at(fl) > uint64_t(PB_MAX_PARTS)) ++fl;
        shift = PB_FILL_LOG2 + fl;
    }
    pb.keys = kc.words();
    pb.n = n;
    pb.dmin = pl.kmin;
    pb.shift = shift;
    pb.parts = int(((span - 1) >> shift) + 1);
    pb.nc = nc;
    for (int c = 0; c < nc; ++c) pb.src[c] = pl.dp.src[c];
    int rpt = nc <= 1 ? 8 : (nc <= 3 ? 4 : (nc <= 7 ? 2 : 1)); // 1024 * rpt tuples of 8 * (1 + nc) bytes in <= 128 KB of LDS
    // (gfx950 has 160 KB per workgroup; a device with less takes fewer rows per thread, and the one-kernel build when even one does not fit)
    while (rpt > 1 && size_t(PB_BLOCK) * size_t(rpt) * size_t(1 + nc) * 8 + size_t(PB_MAX_PARTS) * 12 > ctx->lds_per_block) rpt >>= 1;
    pp.lds_ok = size_t(PB_BLOCK) * size_t(rpt) * size_t(1 + nc) * 8 + size_t(PB_MAX_PARTS) * 12 <= ctx->lds_per_block;
    pp.rpt = rpt;
    pp.tile = int64_t(PB_BLOCK) * rpt;
    pb.W = int(std::min<int64_t>(ctx->num_cus, (n + pp.tile - 1) / pp.tile));
    pb.chunk = ((n + pb.W - 1) / pb.W + pp.tile - 1) / pp.tile * pp.tile;
    pp.twp = nc ? (1 + nc + 1) / 2 * 2 : 0;
    return pp;
}
enum PartResult { PART_NOT_DONE, PART_DONE, PART_DUP };
// Builds of >= 2^25 rows (NQE_JOIN_PART_BUILD_MIN, read per call: the tests lower it for some builds only) that are not ascending.
// PART_NOT_DONE: not eligible, or its extra memory does not fit — one of the forms below still may; PART_DUP: a key occurs twice.
PartResult build_dense_partitioned(nqe_ctx *ctx, const DevColumn &kc, int64_t n, const KeyRanges &kr, DensePlan &pl) {
    const char *part_min_env = getenv("NQE_JOIN_PART_BUILD_MIN");
    const int64_t part_min = part_min_env ? atoll(part_min_env) : (int64_t(1) << 25);
    if (!(n >= part_min && !kr.ascending && (!pl.with_payload || pl.dp.n <= 15) && pl.span <= 0xffffffffull)) return PART_NOT_DONE;
    const PartPlan pp = plan_partitions(ctx, kc, n, pl);
    const PartBuild &pb = pp.pb;
    const uint64_t span = pl.span;
    const int nc = pb.nc, twp = pp.twp, bins = pp.bins;
    const DensePayload &dp = pl.dp;
    const size_t cells = size_t(pb.parts) * size_t(pb.W);
    BufRef counts, offsets, tuples, kord, tuples2, finehist, fine_start;
    try { // the tuple stream and the records come on top of the table: when they do not fit, the one-kernel form still may
        if (getenv("NQE_TEST_PART_BUILD_OOM")) fail(NQE_ERR_OUT_OF_MEMORY, "partitioned build (NQE_TEST_PART_BUILD_OOM)"); // tests: as if the allocation had failed
        if (!pp.lds_ok) fail(NQE_ERR_OUT_OF_MEMORY, "partitioned build: the scatter tile does not fit this device's LDS");
        counts = dev_alloc(ctx, cells * 4);
        offsets = dev_alloc(ctx, (cells + 1) * 8);
        tuples = dev_alloc(ctx, size_t(n) * size_t(1 + nc) * 8 + 16);
        if (pp.two_level) {
            tuples2 = dev_alloc(ctx, size_t(n) * size_t(1 + nc) * 8 + 16);
            finehist = dev_alloc(ctx, size_t(pb.W) * size_t(bins) * 4);
            fine_start = dev_alloc(ctx, (size_t(bins) + 1) * 8);
        } else if (nc) // key-ordered records, zeroed: an entry nobody wrote is absent
            kord = dev_alloc(ctx, size_t(span) * size_t(twp) * 8);
    } catch (const Error &e) {
        if (e.code != NQE_ERR_OUT_OF_MEMORY) throw;
        return PART_NOT_DONE;
    }
    if (!pp.two_level) pl.zero_tables(ctx);
    if (kord) NQE_HIP_CHECK(hipMemsetAsync(kord->ptr, 0, size_t(span) * size_t(twp) * 8, ctx->stream));
    if (pp.two_level)
        launch(ctx, "join_build_part_count", part_build_count_fine_kernel, dim3(unsigned(pb.W)), dim3(PB_BLOCK), size_t(bins) * 4, pb, (uint32_t *)counts->ptr, (uint32_t *)finehist->ptr, bins);
    else
        launch(ctx, "join_build_part_count", part_build_count_kernel, dim3(unsigned(pb.W)), dim3(PB_BLOCK), 0, pb, (uint32_t *)counts->ptr);
    exclusive_scan_u32_to_u64(ctx, (const uint32_t *)counts->ptr, (uint64_t *)offsets->ptr, int64_t(cells));
    const size_t shmem = size_t(pp.tile) * size_t(1 + nc) * 8 + size_t(PB_MAX_PARTS) * 12;
    const int rpt = pp.rpt;
    auto sk = rpt == 8 ? part_build_scatter_kernel<8> : (rpt == 4 ? part_build_scatter_kernel<4> : (rpt == 2 ? part_build_scatter_kernel<2> : part_build_scatter_kernel<1>));
    if (nc <= 1 && rpt == 8) sk = nc ? part_build_scatter1_kernel<1> : part_build_scatter1_kernel<0>; // (its tile in registers, the next one prefetched)
    launch(ctx, "join_build_part_scatter", sk, dim3(unsigned(pb.W)), dim3(PB_BLOCK), shmem, pb, (const uint64_t *)offsets->ptr, (uint64_t *)tuples->ptr);
    BufRef occupied, cursor;
    if (pp.two_level) {
        launch(ctx, "join_build_part_fine_offsets", part_build_fine_offsets_kernel, dim3(unsigned(pb.parts)), dim3(256), 0, (const uint32_t *)finehist->ptr, pb.W, bins, pb.parts, pb.shift - PB_FILL_LOG2,
               (const uint64_t *)offsets->ptr, (uint64_t *)fine_start->ptr);
        launch(ctx, "join_build_part_split", nc ? part_build_split_kernel<1> : part_build_split_kernel<0>, dim3(unsigned(std::min(pb.parts, 2 * ctx->num_cus))), dim3(PB_BLOCK),
               size_t(PB_SPLIT_TILE) * size_t(1 + nc) * 8, pb, (const uint64_t *)offsets->ptr, (const uint64_t *)fine_start->ptr, bins, (const uint64_t *)tuples->ptr, (uint64_t *)tuples2->ptr);
        occupied = dev_alloc_zero(ctx, 8);
        launch(ctx, "join_build_part_fill", nc ? part_build_fill_kernel<1> : part_build_fill_kernel<0>, dim3(unsigned(std::min(bins, 2 * ctx->num_cus))), dim3(PB_BLOCK),
               size_t(PB_FILL_KEYS) * size_t(4 + 8 * nc), (const uint64_t *)fine_start->ptr, bins, (const uint64_t *)tuples2->ptr, span, (uint32_t *)pl.dense->ptr, (uint32_t *)pl.presence->ptr, dp,
               (unsigned long long *)occupied->ptr);
    } else {
        cursor = dev_alloc_zero(ctx, size_t(pb.parts) * 4);
        constexpr int place_by_block = 0; // (1: XCD = blockIdx % 8 instead of the hardware register — no difference measured)
        constexpr int place_chunk = PB_CHUNK;
        constexpr int place_bpc = 3; // workgroups per CU (measured per 10^8 records: 8 -> 2.6 ms, 2-4 -> 2.1, 1 -> 3.1)
        launch(ctx, "join_build_part_place", part_build_place_kernel, dim3(unsigned(place_bpc * ctx->num_cus)), dim3(256), 0, pb, (const uint64_t *)offsets->ptr,
               (const uint64_t *)tuples->ptr, (uint32_t *)pl.dense->ptr, kord ? (uint64_t *)kord->ptr : (uint64_t *)nullptr, twp, (uint32_t *)cursor->ptr, place_by_block, uint32_t(place_chunk));
        occupied = dev_alloc_zero(ctx, 8);
        launch(ctx, "join_build_finish", (kord && (twp == 2 || twp == 4)) ? dense_finish_kernel<true> : dense_finish_kernel<false>, dim3(stream_grid(ctx, int64_t((span + 63) / 64), 4)),
               dim3(256), 0, (uint32_t *)pl.dense->ptr, span, (uint32_t *)pl.presence->ptr, dp, (unsigned long long *)occupied->ptr,
               kord ? (const uint64_t *)kord->ptr : (const uint64_t *)nullptr, twp);
    }
    // (the read also keeps the tuple streams and the records alive until the kernels are done)
    return read_scalar(ctx, (const unsigned long long *)occupied->ptr) != (unsigned long long)n ? PART_DUP : PART_DONE;
}
// larger builds: scatter row numbers, then finish in key order (see dense_finish_kernel) — no device-scope atomics.  Returns dup.
bool build_dense_scatter(nqe_ctx *ctx, const DevColumn &kc, int64_t n, DensePlan &pl) {
    BufRef occupied = dev_alloc_zero(ctx, 8);
    launch(ctx, "join_build_dense", dense_scatter_rows_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), n, pl.kmin, (uint32_t *)pl.dense->ptr);
    launch(ctx, "join_build_finish", dense_finish_kernel<false>, dim3(stream_grid(ctx, int64_t((pl.span + 63) / 64), 4)), dim3(256), 0, (uint32_t *)pl.dense->ptr, pl.span,
           (uint32_t *)pl.presence->ptr, pl.dp, (unsigned long long *)occupied->ptr, (const uint64_t *)nullptr, 0);
    return read_scalar(ctx, (const unsigned long long *)occupied->ptr) != (unsigned long long)n;
}
// the one-kernel form with device atomics serves builds below 2^16 rows (forced on larger ones it measured 10^7 rows 0.67 -> 1.29 ms,
// 10^8 rows 11 -> 22 ms).  Returns dup.
bool build_dense_atomic(nqe_ctx *ctx, const DevColumn &kc, int64_t n, DensePlan &pl, const BufRef &dupflag) {
    launch(ctx, "join_build_dense", dense_unique_build_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), n, pl.kmin, (uint32_t *)pl.dense->ptr,
           (uint32_t *)pl.presence->ptr, pl.dp, (int *)dupflag->ptr);
    return read_scalar(ctx, (const int *)dupflag->ptr) != 0;
}
bool build_unique_dense(nqe_ctx *ctx, nqe_join_table *jt, const nqe_table *left, const DevColumn &kc, const KeyRanges &kr, uint64_t span, const BufRef &dupflag) {
    const int64_t n = left->rows;
    DensePlan pl;
    pl.kmin = kr.kmin;
    pl.span = span;
    plan_dense_payload(ctx, jt, left, kr, pl);
    const PartResult part = build_dense_partitioned(ctx, kc, n, kr, pl);
    bool dup = part == PART_DUP;
    if (part == PART_NOT_DONE) {
        pl.zero_tables(ctx);
        dup = (n >= (int64_t(1) << 16) && (n < (int64_t(1) << 25) || kr.ascending)) ? build_dense_scatter(ctx, kc, n, pl) : build_dense_atomic(ctx, kc, n, pl, dupflag);
    }
    if (dup) return false;
    jt->direct = true;
    jt->dense = pl.dense;
    jt->dense_min = pl.kmin;
    jt->dense_span = span;
    jt->cap = 0; // no hash table: every lookup goes through the direct-address table
    if (pl.with_payload) {
        jt->presence = pl.presence;
        jt->dense_cols = pl.cols;
        jt->dense_packed = pl.packed;
        jt->dense_base = pl.base;
        jt->dense_payload = true;
        jt->dense_full = (span == uint64_t(n));
    }
    return true;
}

// ---- sparse keys: open addressing, one slot per row; with exactly one plain payload column it rides in a second table's slots —
// packed into 8 bytes with the key where both fit, else as {key, payload} pairs — and otherwise a check pass establishes uniqueness
bool build_hashed_unique(nqe_ctx *ctx, nqe_join_table *jt, const nqe_table *left, const DevColumn &kc, const KeyRanges &kr, const BufRef &dupflag) {
    const int64_t n = left->rows;
    const size_t ncols = left->cols.size();
    const uint64_t kmin = kr.kmin, kmax = kr.kmax;
    int shift = 0;
    const uint32_t cap = table_capacity(uint64_t(n), &shift);
    BufRef slots = dev_alloc_zero(ctx, size_t(cap) * 16);
    launch(ctx, "join_build_insert", hashed_insert_rows_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), n, (ulonglong2 *)slots->ptr, cap, shift,
           (int *)dupflag->ptr);
    BufRef slotsp;
    uint64_t filler = 0;
    int pis_col = -1;
    const bool have_filler = kmax != ~0ull || kmin != 0ull; // a value outside [kmin, kmax] (unsigned) is not a build key
    auto bit_length = [](uint64_t x) {
        int b = 0;
        while (b < 64 && (x >> b) != 0) ++b;
        return b;
    };
    PackedPairs pp{};
    if (kr.payload_plain && ncols == 2 && kr.cols.size() == 2) { // one integer payload column whose offset fits a word together with the key's
        const int kbits = std::max(1, bit_length(kmax - kmin)), pbits = std::max(1, bit_length(kr.mm[3] - kr.mm[2]));
        const uint64_t nb = uint64_t(n) * 5 / 48 + 1; // 16-slot buckets at load 0.6
        if (kbits + pbits <= 63 && nb * PACKED_BUCKET < (1ull << 31)) {
            pis_col = jt->left_key == 0 ? 1 : 0;
            pp.kmin = kmin;
            pp.kspan = kmax - kmin;
            pp.pbase = kr.mm[2] ^ order_flip(left->cols[size_t(pis_col)].dtype);
            pp.nb = uint32_t(nb);
            pp.pbits = pbits;
            slotsp = dev_alloc(ctx, size_t(nb) * PACKED_BUCKET * 8);
            NQE_HIP_CHECK(hipMemsetAsync(slotsp->ptr, 0xFF, size_t(nb) * PACKED_BUCKET * 8, ctx->stream));
            launch(ctx, "join_build_insert", packed_insert_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), left->cols[size_t(pis_col)].words(), n,
                   (unsigned long long *)slotsp->ptr, pp, (int *)dupflag->ptr);
        }
    }
    if (slotsp) { // (the packed insert has checked uniqueness itself)
    } else if (kr.payload_plain && ncols == 2 && have_filler) { // exactly one payload column: it rides in the slot
        filler = kmax != ~0ull ? kmax + 1 : kmin - 1;
        pis_col = jt->left_key == 0 ? 1 : 0;
        slotsp = dev_alloc(ctx, size_t(cap) * 16);
        launch(ctx, "join_build_fill", fill_pairs_kernel, dim3(stream_grid(ctx, cap, 256)), dim3(256), 0, (ulonglong2 *)slotsp->ptr, cap, filler);
        launch(ctx, "join_build_insert", hashed_insert_pairs_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), left->cols[size_t(pis_col)].words(), n,
               (ulonglong2 *)slotsp->ptr, cap, shift, filler, (int *)dupflag->ptr);
    } else {
        launch(ctx, "join_build_check", hashed_check_unique_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), n, (const ulonglong2 *)slots->ptr,
               cap, shift, (int *)dupflag->ptr);
    }
    if (read_scalar(ctx, (const int *)dupflag->ptr)) return false;
    jt->direct = true;
    jt->slots = slots;
    jt->cap = cap;
    jt->shift = shift;
    jt->slotsp = slotsp;
    jt->filler = filler;
    jt->pis_col = pis_col;
    jt->pp = pp;
    return true;
}

// Sort-free build.  Uniqueness is established by the build itself: returns false — with `jt` untouched apart from buffers it will
// overwrite — when the keys turn out not to be unique; the caller then runs the sort-based build.  `plain_key`: the key column is a
// plain 8-byte column without validity (Utf8 keys arrive as codes and keep the generic probe).
bool build_unique_fast(nqe_ctx *ctx, nqe_join_table *jt, const nqe_table *left, const DevColumn &kc, bool plain_key) {
    const KeyRanges kr = measure_ranges(ctx, jt, left, kc, plain_key);
    const uint64_t span = kr.kmax - kr.kmin + 1; // 0 on wrap-around: not dense
    BufRef dupflag = dev_alloc_zero(ctx, 4);
    if (dense_eligible(span, left->rows)) return build_unique_dense(ctx, jt, left, kc, kr, span, dupflag);
    return build_hashed_unique(ctx, jt, left, kc, kr, dupflag);
}

// ---- sort-based build: its dense add-on — a direct-address table over a dense key range (the keys are sorted unsigned: first / last
// are min / max), and for unique keys with plain payloads the key-ordered payload copies + presence bitmap of the sort-free build
void build_sorted_dense(nqe_ctx *ctx, nqe_join_table *jt, const nqe_table *left, const DevColumn &kc, bool plain_key, const BufRef &skeys, const BufRef &ustart, uint32_t U) {
    const int64_t n = left->rows;
    const size_t ncols = left->cols.size();
    uint64_t kmin = read_scalar(ctx, (const uint64_t *)skeys->ptr);
    uint64_t kmax = read_scalar(ctx, (const uint64_t *)skeys->ptr + (n - 1));
    uint64_t span = kmax - kmin + 1; // 0 on wrap-around: not dense
    if (!dense_eligible(span, n)) return;
    jt->dense = dev_alloc_zero(ctx, size_t(span) * 4);
    jt->dense_min = kmin;
    jt->dense_span = span;
    launch(ctx, "join_fill_dense", fill_dense_kernel, dim3(stream_grid(ctx, U, 256)), dim3(256), 0, (const uint64_t *)skeys->ptr,
           (const uint32_t *)ustart->ptr, (const uint32_t *)jt->perm->ptr, U, kmin, (uint32_t *)jt->dense->ptr, jt->direct ? 1 : 0);
    if (!jt->direct) jt->ustart = ustart;
    bool plain = jt->direct && plain_key;
    for (size_t ci = 0; ci < ncols; ++ci)
        if (int(ci) != jt->left_key) plain = plain && is_plain_word(left->cols[ci]);
    if (!(plain && span * 8 * ncols <= (size_t(8) << 30))) return;
    jt->presence = dev_alloc_zero(ctx, size_t((span + 31) / 32) * 4);
    jt->dense_cols.resize(ncols);
    jt->dense_packed.assign(ncols, 0);
    jt->dense_base.assign(ncols, 0);
    bool first = true; // the first scatter also sets the presence bits
    for (size_t ci = 0; ci < ncols; ++ci) {
        if (int(ci) == jt->left_key) continue;
        const DevColumn &pc = left->cols[ci];
        uint32_t *presence = first ? (uint32_t *)jt->presence->ptr : (uint32_t *)nullptr;
        first = false;
        if (pc.dtype == NQE_INT64 || pc.dtype == NQE_UINT64) { // value range within 32 bits → uint32 offsets
            const uint64_t flip = order_flip(pc.dtype);
            BufRef mm = dev_alloc(ctx, 16);
            const uint64_t init[2] = {~0ull, 0ull};
            NQE_HIP_CHECK(hipMemcpyAsync(mm->ptr, init, 16, hipMemcpyHostToDevice, ctx->stream));
            launch(ctx, "join_payload_minmax", minmax_u64_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, pc.words(), n, flip,
                   (unsigned long long *)mm->ptr, (unsigned long long *)mm->ptr + 1);
            const uint64_t mn = read_scalar(ctx, (const uint64_t *)mm->ptr), mx = read_scalar(ctx, (const uint64_t *)mm->ptr + 1);
            if (mx - mn <= 0xffffffffull) {
                jt->dense_packed[ci] = 1;
                jt->dense_base[ci] = mn ^ flip;
                jt->dense_cols[ci] = dev_alloc_zero(ctx, size_t(span) * 4 + 8);
                launch(ctx, "join_scatter_payload", scatter_dense_payload32_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, kc.words(), n,
                       kmin, pc.words(), jt->dense_base[ci], (uint32_t *)jt->dense_cols[ci]->ptr, presence);
                continue;
            }
        }
        jt->dense_cols[ci] = dev_alloc(ctx, size_t(span) * 8);
        launch(ctx, "join_scatter_payload", scatter_dense_payload_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0,
               kc.words(), n, kmin, pc.words(), (uint64_t *)jt->dense_cols[ci]->ptr, presence);
    }
    if (first) // key-only build side: presence bitmap only
        launch(ctx, "join_scatter_payload", scatter_dense_payload_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0,
               kc.words(), n, kmin, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)jt->presence->ptr);
    jt->dense_payload = true;
    jt->dense_full = (span == uint64_t(U));
}
// duplicate keys: plain payload columns in sorted-row order (see nqe_join_table::sorted_cols).  An optimisation on top of
// everything the table needs: a copy that does not fit is left out and the probe gathers that column through the permutation
// instead (probe_duplicates: need_perm)
void copy_sorted_payloads(nqe_ctx *ctx, nqe_join_table *jt, const nqe_table *left) {
    const int64_t n = left->rows;
    jt->sorted_cols.resize(left->cols.size());
    const bool test_oom = getenv("NQE_TEST_SORTED_COLS_OOM") != nullptr; // tests: as if the allocation had failed
    for (size_t ci = 0; ci < left->cols.size(); ++ci) {
        const DevColumn &pc = left->cols[ci];
        if (int(ci) == jt->left_key || !is_plain_word(pc)) continue;
        try {
            if (test_oom) fail(NQE_ERR_OUT_OF_MEMORY, "sorted payload copy (NQE_TEST_SORTED_COLS_OOM)");
            jt->sorted_cols[ci] = dev_alloc(ctx, size_t(n) * 8 + 8);
        } catch (const Error &e) {
            if (e.code != NQE_ERR_OUT_OF_MEMORY) throw;
            jt->sorted_cols[ci] = nullptr;
            continue;
        }
        launch(ctx, "join_permute_payload", permute_words_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, pc.words(), (const uint32_t *)jt->perm->ptr, n,
               (uint64_t *)jt->sorted_cols[ci]->ptr);
    }
}
// duplicate keys (their matches must come out in ascending build row), or an empty build side
void build_sorted(nqe_ctx *ctx, nqe_join_table *jt, const nqe_table *left, const DevColumn &kc, bool plain_key) {
    const int64_t n = left->rows;
    BufRef idx = dev_alloc(ctx, size_t(n) * 4 + 8), skeys = dev_alloc(ctx, size_t(n) * 8 + 8);
    jt->perm = dev_alloc(ctx, size_t(n) * 4 + 8);
    uint32_t U = 0;
    BufRef ustart;
    if (n) {
        launch(ctx, "join_iota", iota_u32_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, (uint32_t *)idx->ptr, n);
        radix_sort_pairs_u64(ctx, kc.words(), (const uint32_t *)idx->ptr, (uint64_t *)skeys->ptr, (uint32_t *)jt->perm->ptr, n,
                             false);
        // run heads of the sorted keys → unique keys
        BufRef flags = dev_alloc(ctx, size_t(n + 1) * 4);
        launch(ctx, "join_mark_heads", mark_heads_kernel, dim3(stream_grid(ctx, n + 1, 256)), dim3(256), 0,
               (const uint64_t *)skeys->ptr, n, (uint32_t *)flags->ptr);
        BufRef offs = dev_alloc(ctx, size_t(n + 2) * 8);
        exclusive_scan_u32_to_u64(ctx, (const uint32_t *)flags->ptr, (uint64_t *)offs->ptr, n + 1);
        U = uint32_t(read_scalar(ctx, (const uint64_t *)offs->ptr + (n + 1)));
        ustart = dev_alloc(ctx, size_t(U + 1) * 4);
        launch(ctx, "join_fill_ustart", fill_ustart_kernel, dim3(stream_grid(ctx, n + 1, 256)), dim3(256), 0,
               (const uint32_t *)flags->ptr, (const uint64_t *)offs->ptr, n, U, (uint32_t *)ustart->ptr);
    }
    jt->direct = (int64_t(U) == n);
    jt->cap = table_capacity(U, &jt->shift);
    jt->slots = dev_alloc_zero(ctx, size_t(jt->cap) * 16);
    if (U)
        launch(ctx, "join_insert", insert_unique_kernel, dim3(stream_grid(ctx, U, 256)), dim3(256), 0, (const uint64_t *)skeys->ptr,
               (const uint32_t *)ustart->ptr, (const uint32_t *)jt->perm->ptr, U, (ulonglong2 *)jt->slots->ptr, jt->cap, jt->shift,
               jt->direct ? 1 : 0);
    if (n > 0 && U > 0) build_sorted_dense(ctx, jt, left, kc, plain_key, skeys, ustart, U);
    if (!jt->direct && n > 0) copy_sorted_payloads(ctx, jt, left);
    sync(ctx); // skeys/flags/ustart are released on return
    if (getenv("NQE_DEBUG"))
        fprintf(stderr, "[nqe] join build: n=%lld U=%u direct=%d dense_span=%llu dense_payload=%d dense_full=%d cap=%u\n", (long long)n, U, int(jt->direct),
                (unsigned long long)jt->dense_span, int(jt->dense_payload), int(jt->dense_full), jt->cap);
}

std::unique_ptr<nqe_join_table> build_table(nqe_ctx *ctx, const nqe_table *left, int left_key) {
    if (left_key < 0 || size_t(left_key) >= left->cols.size()) fail(NQE_ERR_LOGICAL, "ColumnExpr must has name or idx");
    const DevColumn &kc_orig = left->cols[size_t(left_key)];
    check_key_types(kc_orig.dtype, -1);
    const int64_t n = left->rows;
    Utf8Dict dict;
    DevColumn kc_codes;
    if (kc_orig.dtype == NQE_UTF8) kc_codes = utf8_encode_build(ctx, kc_orig, &dict);
    const DevColumn &kc = kc_orig.dtype == NQE_UTF8 ? kc_codes : kc_orig;
    if (n >= (int64_t(1) << 32)) fail(NQE_ERR_NOT_SUPPORTED, "build side with 2^32 or more rows is not supported");
    auto jt = std::make_unique<nqe_join_table>();
    jt->ctx = ctx;
    jt->left_cols = left->cols;
    jt->left_rows = n;
    jt->key_dtype = kc_orig.dtype;
    jt->left_key = left_key;
    jt->dict = dict;
    const bool plain_key = kc_orig.dtype != NQE_UTF8 && !kc.validity;
    if (n > 0 && build_unique_fast(ctx, jt.get(), left, kc, plain_key)) {
        if (getenv("NQE_DEBUG"))
            fprintf(stderr, "[nqe] join build (sort-free): n=%lld dense_span=%llu dense_payload=%d dense_full=%d cap=%u pis=%d\n", (long long)n,
                    (unsigned long long)jt->dense_span, int(jt->dense_payload), int(jt->dense_full), jt->cap, jt->pis_col);
        return jt;
    }
    build_sorted(ctx, jt.get(), left, kc, plain_key);
    return jt;
}

// ================================================================ probe
Lookup lookup_of(const nqe_join_table *jt) {
    Lookup L;
    std::memset(&L, 0, sizeof(L));
    L.slots = jt->slots ? (const ulonglong2 *)jt->slots->ptr : nullptr;
    L.cap = jt->cap;
    L.shift = jt->shift;
    L.dense = jt->dense ? (const uint32_t *)jt->dense->ptr : nullptr;
    L.ustart = jt->ustart ? (const uint32_t *)jt->ustart->ptr : nullptr;
    L.dense_min = jt->dense_min;
    L.dense_span = jt->dense_span;
    L.direct = jt->direct ? 1 : 0;
    return L;
}

// how join_fused_write_kernel produces one build-side column (FusedCols::kind / src / base / bits)
struct LeftOut {
    int kind;
    const uint64_t *src;
    uint64_t base;
    int bits;
};
// The output table of a fused write (every column a plain word column) and the kernel's column list, from the description of
// the build-side columns.  Two aliasings, both observable:
//  * in an equi-join on an integer key the build key column of the output IS the probe key column of the output, bit for bit: it
//    is written once and the two output columns share the buffer (tables are immutable; 8 of the 32 output bytes per row of C4
//    are never written);
//  * `share_probe` (output row = probe row): the probe-side columns of the output ARE the probe table's columns — tables are
//    immutable and their columns may share buffers — so only the build-side columns are written.
std::unique_ptr<nqe_table> fused_output(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key, const DevColumn &rk, int64_t out_rows,
                                        const std::vector<LeftOut> &left, bool share_probe, FusedCols &fc) {
    auto out = std::make_unique<nqe_table>();
    out->ctx = ctx;
    out->rows = out_rows;
    std::memset(&fc, 0, sizeof(fc));
    const bool share_key = share_key_column(jt->left_cols[size_t(jt->left_key)], rk);
    int share_pos = -1, right_key_pos = -1;
    for (size_t ci = 0; ci < jt->left_cols.size(); ++ci) {
        if (int(ci) == jt->left_key && share_key) {
            share_pos = int(out->cols.size());
            out->cols.push_back(DevColumn{});
            continue;
        }
        out->cols.push_back(make_word_column(ctx, jt->left_cols[ci].dtype, out_rows, false));
        fc.kind[fc.n] = left[ci].kind;
        fc.bits[fc.n] = left[ci].bits;
        fc.base[fc.n] = left[ci].base;
        fc.src[fc.n] = left[ci].src;
        fc.dst[fc.n] = (uint64_t *)out->cols.back().values->ptr;
        fc.n++;
    }
    for (size_t cj = 0; cj < right->cols.size(); ++cj) {
        const DevColumn &c = right->cols[cj];
        if (int(cj) == right_key) right_key_pos = int(out->cols.size());
        if (share_probe) {
            out->cols.push_back(c);
            out->cols.back().null_count = 0;
            continue;
        }
        out->cols.push_back(make_word_column(ctx, c.dtype, out_rows, false));
        // the probe key column is in registers already (kind 1): loading it again as a probe-side column cost pass 2 8-15 %
        // (C4 1.13 -> 1.04 ms, a 10 %-match join 0.70 -> 0.60 ms).  Requesting one more probe-side column together with the
        // keys (33 more VGPRs) was neutral on top of that.
        fc.kind[fc.n] = int(cj) == right_key ? 1 : 0;
        fc.src[fc.n] = c.words();
        fc.dst[fc.n] = (uint64_t *)out->cols.back().values->ptr;
        fc.n++;
    }
    if (share_pos >= 0) {
        out->cols[size_t(share_pos)] = out->cols[size_t(right_key_pos)];
        out->cols[size_t(share_pos)].dtype = jt->left_cols[size_t(jt->left_key)].dtype;
    }
    return out;
}

// ---- unique + dense keys with key-ordered plain payloads, plain probe side (PK–FK)
std::unique_ptr<nqe_table> probe_dense_payload(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key, const DevColumn &rk) {
    const int64_t n = right->rows;
    const bool may_share = share_probe_allowed(right);
    std::vector<LeftOut> left(jt->left_cols.size());
    for (size_t ci = 0; ci < left.size(); ++ci) {
        const int packed = jt->dense_packed[ci];
        if (int(ci) == jt->left_key) left[ci] = {1, nullptr, 0, packed};
        else left[ci] = {packed >= 2 ? 4 : (packed ? 3 : 2), (const uint64_t *)jt->dense_cols[ci]->ptr, jt->dense_base[ci], packed};
    }
    // Optimistic form: a build side whose keys fill their range without gaps is a primary key; a foreign key then matches on
    // every row, the output row of a probe row is the probe row, and ONE pass (no presence pass, no scan, the probe keys read
    // once) writes everything — while checking every key against the range.  A key outside it discards the output, and this
    // join table (and, through the context's join hints, this join) takes the two-pass form from then on.
    // (a table built on several keys takes no hint and leaves none: both of its key buffers are pool-allocated code columns, whose
    // addresses recur across unrelated joins of equal sizes — the verdict stays with the table, all_match_failed)
    const bool hinted = !jt->keys;
    const uint64_t jhint = hinted ? join_hint_key(jt, rk, n) : 0;
    if (hinted && ctx->join_hints.count(jhint)) jt->all_match_failed = true;
    if (jt->dense_full && !jt->all_match_failed && n > 0) {
        FusedCols fc;
        auto out = fused_output(ctx, jt, right, right_key, rk, n, left, may_share, fc);
        BufRef miss = dev_alloc_zero(ctx, 4);
        const int64_t ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
        if (n >= (int64_t(1) << 20))
            launch(ctx, "join_sample_range", join_sample_range_kernel, dim3(256), dim3(256), 0, rk.words(), n, jt->dense_min, jt->dense_span, (int *)miss->ptr);
        launch(ctx, "join_fused_write", join_fused_write_kernel<FUSED_WRITE_ROWS, true>, dim3(stream_grid(ctx, ntiles, 4)), dim3(256), 0, rk.words(), n, ntiles,
               (const uint64_t *)nullptr, (const uint64_t *)nullptr, jt->dense_min, (const uint32_t *)nullptr, fc, jt->dense_span, (int *)miss->ptr);
        if (!read_scalar(ctx, (const int *)miss->ptr)) return out;
        jt->all_match_failed = true;
        if (hinted) {
            if (ctx->join_hints.size() >= 256) ctx->join_hints.clear();
            ctx->join_hints[jhint] = 1;
        }
    }
    // two passes: presence test + counts, scan, then one fused write of every output column
    BufRef counts;
    KeepMask km = new_keep_mask(ctx, n, &counts);
    dim3 grid(stream_grid(ctx, km.ntiles, 4)), block(256);
    if (km.ntiles) {
        const size_t pbytes = size_t((jt->dense_span + 31) / 32) * 4;
        dim3 pgrid(stream_grid(ctx, km.ntiles, 16, 1)), pblock(1024);
        const uint32_t *pp = (const uint32_t *)jt->presence->ptr;
        uint64_t *kp = (uint64_t *)km.keep->ptr;
        uint32_t *cp = (uint32_t *)counts->ptr;
        if (jt->dense_full)
            launch(ctx, "join_probe_presence", probe_presence_kernel<0>, dim3(stream_grid(ctx, km.ntiles, 16, 2)), pblock, 0, rk.words(),
                   n, km.ntiles, pp, jt->dense_min, jt->dense_span, kp, cp);
        else if (pbytes <= 128 * 1024)
            launch(ctx, "join_probe_presence", probe_presence_kernel<1>, pgrid, pblock, pbytes, rk.words(), n, km.ntiles, pp,
                   jt->dense_min, jt->dense_span, kp, cp);
        else
            launch(ctx, "join_probe_presence", probe_presence_kernel<2>, dim3(stream_grid(ctx, km.ntiles, 16, 2)), pblock, 0, rk.words(),
                   n, km.ntiles, pp, jt->dense_min, jt->dense_span, kp, cp);
    }
    km = finish_mask(ctx, km, counts);
    FusedCols fc;
    // (every probe row matched after all — a primary key with gaps, say: share the probe columns)
    auto out = fused_output(ctx, jt, right, right_key, rk, km.total, left, km.total == n && may_share, fc);
    if (km.ntiles && km.total > 0)
        launch(ctx, "join_fused_write", join_fused_write_kernel<FUSED_WRITE_ROWS>, grid, block, 0, rk.words(), n, km.ntiles, (const uint64_t *)km.keep->ptr,
               (const uint64_t *)km.tile_offsets->ptr, jt->dense_min, (const uint32_t *)nullptr, fc, uint64_t(0), (int *)nullptr);
    sync(ctx);
    return out;
}

// ---- unique build keys: every probe row yields 0/1 rows → a lookup pass, then stream compaction with a gather
struct UniqueMatches {
    KeepMask km;
    BufRef counts;
    BufRef bidx;    // build row per probe row (coop / lookup probe)
    BufRef payload; // `pairs`: the payload word per probe row instead — its values arrive with the lookup
};
UniqueMatches probe_unique_lookup(nqe_ctx *ctx, const nqe_join_table *jt, const DevColumn &rk, int64_t n, bool pairs) {
    UniqueMatches m;
    KeepMask &km = m.km = new_keep_mask(ctx, n, &m.counts);
    if (pairs) {
        m.payload = dev_alloc(ctx, size_t(n) * 8 + 8);
        if (km.ntiles && jt->pp.pbits)
            launch(ctx, "join_probe_pairs", probe_packed_kernel, dim3(stream_grid(ctx, km.ntiles, 4)), dim3(256), 0, rk.words(), n, km.ntiles,
                   (const ulonglong2 *)jt->slotsp->ptr, jt->pp, (uint64_t *)km.keep->ptr, (uint64_t *)m.payload->ptr, (uint32_t *)m.counts->ptr);
        else if (km.ntiles)
            launch(ctx, "join_probe_pairs", probe_pairs_kernel, dim3(stream_grid(ctx, km.ntiles, 4)), dim3(256), 0, rk.words(), n, km.ntiles,
                   (const ulonglong2 *)jt->slotsp->ptr, jt->cap, jt->shift, jt->filler, (uint64_t *)km.keep->ptr, (uint64_t *)m.payload->ptr,
                   (uint32_t *)m.counts->ptr);
    } else {
        m.bidx = dev_alloc(ctx, size_t(n) * 4 + 8);
        if (km.ntiles && !jt->dense)
            launch(ctx, "join_probe_unique", probe_unique_coop_kernel, dim3(stream_grid(ctx, km.ntiles, 4)), dim3(256), 0, rk.words(), n, km.ntiles,
                   (const ulonglong2 *)jt->slots->ptr, jt->cap, jt->shift, (uint64_t *)km.keep->ptr, (uint32_t *)m.bidx->ptr, (uint32_t *)m.counts->ptr);
        else if (km.ntiles)
            launch(ctx, "join_probe_unique", probe_unique_kernel, dim3(stream_grid(ctx, km.ntiles, 4)), dim3(256), 0, rk.words(), n,
                   km.ntiles, lookup_of(jt), (uint64_t *)km.keep->ptr, (uint32_t *)m.bidx->ptr, (uint32_t *)m.counts->ptr);
    }
    km = finish_mask(ctx, km, m.counts);
    return m;
}
// general columns (validity, Boolean, Utf8): one compaction per column
void compact_unique_columns(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, const DevColumn &rk, const UniqueMatches &m, nqe_table *out) {
    const KeepMask &km = m.km;
    DevColumn outer_pos;
    for (size_t ci = 0; ci < jt->left_cols.size(); ++ci) {
        const DevColumn &c = jt->left_cols[ci];
        if (int(ci) == jt->left_key && !c.validity && c.dtype != NQE_UTF8) {
            out->cols.push_back(compact_column(ctx, as_build_key(rk), km)); // (a coalesced compaction instead of a random gather)
        } else if (c.dtype == NQE_UTF8) {
            // outer_pos (the reference's Int64 index array, hash_join.rs:230-231) = build rows of the matches,
            // obtained by gathering a row-number column; then the Utf8 `take`
            if (!outer_pos.values) outer_pos = compact_gather_column(ctx, rowid_column(ctx, jt->left_rows), (const uint32_t *)m.bidx->ptr, km);
            out->cols.push_back(take_utf8(ctx, c, (const int64_t *)outer_pos.words(), km.total, false));
        } else {
            out->cols.push_back(compact_gather_column(ctx, c, (const uint32_t *)m.bidx->ptr, km));
        }
    }
    for (auto &c : right->cols) out->cols.push_back(compact_column(ctx, c, km));
}
std::unique_ptr<nqe_table> probe_unique(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key, const DevColumn &rk, bool right_plain) {
    const int64_t n = right->rows;
    bool left_plain = true;
    for (auto &c : jt->left_cols) left_plain = left_plain && is_plain_word(c);
    // one plain payload column riding in the table's slots
    const bool pairs = jt->slotsp != nullptr && left_plain && right_plain && !jt->dense;
    const UniqueMatches m = probe_unique_lookup(ctx, jt, rk, n, pairs);
    const KeepMask &km = m.km;
    const bool may_share = share_probe_allowed(right);
    if (pairs && km.total == n && n > 0 && may_share && share_key_column(jt->left_cols[size_t(jt->left_key)], rk)) {
        // every probe row matched: output row = probe row.  The payload words the lookup wrote per probe row ARE the build
        // payload column of the output, and the other three columns are the probe table's own (shared buffers): no second pass
        auto out = std::make_unique<nqe_table>();
        out->ctx = ctx;
        out->rows = km.total;
        for (size_t ci = 0; ci < jt->left_cols.size(); ++ci) {
            DevColumn c;
            if (int(ci) == jt->left_key) {
                c = rk;
            } else {
                c.length = n;
                c.values = m.payload;
            }
            c.dtype = jt->left_cols[ci].dtype;
            c.null_count = 0;
            out->cols.push_back(c);
        }
        for (auto &c : right->cols) out->cols.push_back(c);
        sync(ctx);
        return out;
    }
    if (left_plain && right_plain) {
        // every column is a plain 8-byte column: ONE pass writes all of them (probe columns streamed, the build key taken
        // from the probe key, build payloads gathered by the recorded build row — or, `pairs`, streamed like a probe column)
        std::vector<LeftOut> left(jt->left_cols.size());
        for (size_t ci = 0; ci < left.size(); ++ci) {
            const bool key = int(ci) == jt->left_key;
            left[ci] = {key ? 1 : (pairs ? 0 : 2), pairs && !key ? (const uint64_t *)m.payload->ptr : jt->left_cols[ci].words(), 0, 0};
        }
        FusedCols fc;
        auto out = fused_output(ctx, jt, right, right_key, rk, km.total, left, km.total == n && may_share, fc);
        if (km.ntiles && km.total > 0)
            launch(ctx, "join_fused_write", join_fused_write_kernel<FUSED_WRITE_ROWS>, dim3(stream_grid(ctx, km.ntiles, 4)), dim3(256), 0, rk.words(), n, km.ntiles,
                   (const uint64_t *)km.keep->ptr, (const uint64_t *)km.tile_offsets->ptr, uint64_t(0), pairs ? (const uint32_t *)nullptr : (const uint32_t *)m.bidx->ptr, fc,
                   uint64_t(0), (int *)nullptr);
        sync(ctx);
        return out;
    }
    auto out = std::make_unique<nqe_table>();
    out->ctx = ctx;
    out->rows = km.total;
    compact_unique_columns(ctx, jt, right, rk, m, out.get());
    sync(ctx); // bidx / mask are released on return
    return out;
}

// the probe key as the lookups take it: a Utf8 key re-encoded through the build side's dictionary (into `codes`), else the column itself
const DevColumn &encoded_probe_key(nqe_ctx *ctx, const nqe_join_table *jt, const DevColumn &rk_orig, DevColumn &codes) {
    if (rk_orig.dtype != NQE_UTF8) return rk_orig;
    codes = utf8_encode_probe(ctx, rk_orig, jt->dict);
    return codes;
}

// ---- the expand path: count pass (expand_count), scan, output-driven write pass (expand_write) — ONE path with two entries.
//   probe_duplicates: the inner probe of a duplicate-key table (probe_count_kernel / probe_write_kernel, labels join_probe_*);
//   probe_outer:      the outer joins (quirk Q19: HashJoin honouring join_type; outer_count_kernel / outer_write_kernel, labels
//                     join_outer_*), over EVERY build form — lookup_of(jt) is complete for all of them (`dense` or `slots` is always
//                     filled) — taking none of the fused one-pass tiers; the build-preserving side adds a pass over the build rows
//                     (unmatched_build).  The match relation is the inner join's, Q11 included.
// Which kernel column reads what and lands where is hash_join_expand_plan.hpp's list (plain C++, tested on the CPU for both entries).
struct ExpandMode {
    bool null_extend;  // the outer entry: NULL-extended rows, exact null counts
    bool keep_probe;   // … whose unmatched probe rows stay
    uint32_t *marks;   // … the bitmap of nqe_join_marks (bit `start` per matched key), or null
    const char *count_label, *write_label;
};
// pass 2 and what follows it: allocates the destination of every kernel column, writes, packs the byte-staged Boolean values and
// validity, places the columns and takes the Utf8 columns
void write_matches(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, const ExpandMode &mode, bool has_null, int64_t M, const BufRef &pmeta, const BufRef &offs,
                   int grid, const jx::ExpandPlan &plan, const std::vector<DevColumn> &srcs, nqe_table *out) {
    const int64_t n = right->rows;
    const size_t nleft = jt->left_cols.size(), ncols = plan.cols.size();
    ExpandCols ec;
    std::memset(&ec, 0, sizeof(ec));
    ec.n = int(ncols);
    ec.n_left = plan.n_left;
    ec.need_perm = plan.need_perm ? 1 : 0;
    DevColumn outer_pos, inner_pos;
    out->cols.resize(nleft + right->cols.size());
    std::vector<BufRef> bool_bytes(ncols), valid_bytes(ncols);
    std::vector<DevColumn> dsts(ncols);
    for (size_t k = 0; k < ncols; ++k) {
        const jx::ExpandCol &pc = plan.cols[k];
        const DevColumn &src = srcs[k];
        DevColumn dst = src.dtype == NQE_BOOLEAN ? make_bool_column(ctx, M, pc.validity) : make_word_column(ctx, src.dtype, M, pc.validity);
        ec.by_pos[k] = pc.by_pos ? 1 : 0;
        ec.from_probe[k] = pc.from_probe ? 1 : 0;
        ec.src[k] = src.values ? src.values->ptr : nullptr;
        ec.src_valid[k] = src.valid();
        ec.dtype[k] = src.dtype;
        ec.null_word[k] = pc.null_word;
        if (src.dtype == NQE_BOOLEAN) {
            bool_bytes[k] = dev_alloc(ctx, size_t(M) + 8);
            ec.dst_bool_bytes[k] = (uint8_t *)bool_bytes[k]->ptr;
        } else {
            ec.dst_words[k] = (uint64_t *)dst.values->ptr;
        }
        if (pc.validity) {
            valid_bytes[k] = dev_alloc(ctx, size_t(M) + 8);
            ec.dst_valid_bytes[k] = (uint8_t *)valid_bytes[k]->ptr;
        }
        dsts[k] = std::move(dst);
    }
    if (n && M) {
        auto k = mode.null_extend ? (plan.plain ? outer_write_kernel<true> : outer_write_kernel<false>) : (plan.plain ? probe_write_kernel<true> : probe_write_kernel<false>);
        launch(ctx, mode.write_label, k, dim3(grid), dim3(JT_BLOCK), 0, (const uint64_t *)pmeta->ptr, n, (const uint64_t *)offs->ptr,
               jt->perm ? (const uint32_t *)jt->perm->ptr : (const uint32_t *)nullptr, jt->direct ? 1 : 0, ec);
    }
    for (size_t k = 0; k < ncols; ++k) {
        const int slot = plan.cols[k].out_slot;
        if (bool_bytes[k]) pack_bytes_to_bits(ctx, (const uint8_t *)bool_bytes[k]->ptr, M, (uint64_t *)dsts[k].values->ptr);
        if (valid_bytes[k]) pack_bytes_to_bits(ctx, (const uint8_t *)valid_bytes[k]->ptr, M, (uint64_t *)dsts[k].validity->ptr);
        if (slot >= 0) out->cols[size_t(slot)] = dsts[k];
        else if (slot == jx::SLOT_OUTER_POS) outer_pos = dsts[k];
        else inner_pos = dsts[k];
    }
    for (size_t c = 0; c < nleft; ++c)
        if (jt->left_cols[c].dtype == NQE_UTF8) out->cols[c] = take_utf8(ctx, jt->left_cols[c], (const int64_t *)outer_pos.words(), M, has_null);
    for (size_t c = 0; c < right->cols.size(); ++c)
        if (right->cols[c].dtype == NQE_UTF8) out->cols[nleft + c] = take_utf8(ctx, right->cols[c], (const int64_t *)inner_pos.words(), M, false);
    if (mode.null_extend) count_nulls_exact(ctx, out);
}
// `rk`: the probe key as the lookups take it (encoded_probe_key), `rk_orig`: the caller's column
std::unique_ptr<nqe_table> probe_expand(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key, const DevColumn &rk, const DevColumn &rk_orig,
                                        const ExpandMode &mode) {
    const int64_t n = right->rows;
    const int64_t ntiles = (n + JT_ROWS - 1) / JT_ROWS;
    BufRef pmeta = dev_alloc(ctx, size_t(n) * 8 + 8);
    BufRef counts = dev_alloc(ctx, size_t(ntiles + 1) * 4);
    BufRef offs = dev_alloc(ctx, size_t(ntiles + 1) * 8);
    BufRef misses;
    if (mode.null_extend) misses = dev_alloc_zero(ctx, 8);
    const int grid = int(std::max<int64_t>(1, std::min<int64_t>(ntiles, int64_t(ctx->num_cus) * 8)));
    if (n && !mode.null_extend) {
        launch(ctx, mode.count_label, probe_count_kernel, dim3(grid), dim3(JT_BLOCK), 0, rk.words(), n, lookup_of(jt), (uint64_t *)pmeta->ptr, (uint32_t *)counts->ptr, ctx->d_flags);
    } else if (n) {
        auto k = mode.keep_probe ? (mode.marks ? outer_count_kernel<true, true> : outer_count_kernel<true, false>)
                                 : (mode.marks ? outer_count_kernel<false, true> : outer_count_kernel<false, false>);
        launch(ctx, mode.count_label, k, dim3(grid), dim3(JT_BLOCK), 0, rk.words(), n, lookup_of(jt), (uint64_t *)pmeta->ptr, (uint32_t *)counts->ptr, mode.marks,
               (unsigned long long *)misses->ptr, ctx->d_flags);
    }
    exclusive_scan_u32_to_u64(ctx, (const uint32_t *)counts->ptr, (uint64_t *)offs->ptr, ntiles);
    const int64_t M = int64_t(read_scalar(ctx, (const uint64_t *)offs->ptr + ntiles));
    const bool has_null = mode.keep_probe && read_scalar(ctx, (const unsigned long long *)misses->ptr) != 0ull;
    {
        int f[NQE_NUM_FLAGS];
        flags_read(ctx, f);
        if (f[NQE_FLAG_TABLE_FULL]) fail(NQE_ERR_OUT_OF_MEMORY, "join output of one probe tile exceeds 2^32 rows");
    }
    auto out = std::make_unique<nqe_table>();
    out->ctx = ctx;
    out->rows = M;
    // the kernel's columns.  A Utf8 column goes through a row-number column (the kernel emits outer_pos / inner_pos) and the Utf8
    // `take`; a plain integer build key is taken from the probe side (the key of a match is bit-identical on both sides), and where
    // that makes the two key columns of the output identical they are ONE buffer, as in the unique-key forms: a column less to write
    const DevColumn &lk = jt->left_cols[size_t(jt->left_key)];
    jx::ExpandSides sides;
    for (size_t c = 0; c < jt->left_cols.size(); ++c) {
        jx::SideCol sc;
        sc.dtype = jt->left_cols[c].dtype;
        sc.validity = jt->left_cols[c].validity != nullptr;
        sc.sorted_copy = c < jt->sorted_cols.size() && jt->sorted_cols[c] != nullptr;
        sides.left.push_back(sc);
    }
    for (auto &c : right->cols) {
        jx::SideCol sc;
        sc.dtype = c.dtype;
        sc.validity = c.validity != nullptr;
        sides.right.push_back(sc);
    }
    sides.left_key = jt->left_key;
    sides.right_key = right_key;
    sides.left_rows = jt->left_rows;
    sides.right_rows = n;
    sides.direct = jt->direct;
    sides.keys_shareable = share_key_column(lk, rk_orig);
    sides.null_extend = mode.null_extend;
    sides.has_null = has_null;
    const jx::ExpandPlan plan = jx::plan_expand(sides);
    if (plan.cols.size() > size_t(MAX_JOIN_COLS)) fail(NQE_ERR_NOT_SUPPORTED, "join output wider than 32 columns");
    std::vector<DevColumn> srcs(plan.cols.size());
    for (size_t k = 0; k < plan.cols.size(); ++k) {
        const jx::ExpandCol &pc = plan.cols[k];
        DevColumn &s = srcs[k];
        if (pc.source == jx::SRC_LEFT) {
            s = jt->left_cols[size_t(pc.index)];
            if (pc.by_pos) s.values = jt->sorted_cols[size_t(pc.index)];
        } else if (pc.source == jx::SRC_RIGHT) {
            s = right->cols[size_t(pc.index)];
        } else if (pc.source == jx::SRC_PROBE_KEY) {
            s = as_build_key(rk);
            s.dtype = pc.dtype;
        } else {
            s = rowid_column(ctx, pc.source == jx::SRC_LEFT_ROWID ? jt->left_rows : n);
        }
    }
    write_matches(ctx, jt, right, mode, has_null, M, pmeta, offs, grid, plan, srcs, out.get());
    if (plan.key_shared) {
        out->cols[size_t(jt->left_key)] = out->cols[jt->left_cols.size() + size_t(right_key)];
        out->cols[size_t(jt->left_key)].dtype = lk.dtype;
    }
    sync(ctx); // the temporaries above are released on return; keep the stream drained for simplicity
    return out;
}
// the inner entry: duplicate build keys (probe_table has checked the arguments)
std::unique_ptr<nqe_table> probe_duplicates(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key, const DevColumn &rk, const DevColumn &rk_orig) {
    return probe_expand(ctx, jt, right, right_key, rk, rk_orig, ExpandMode{false, false, nullptr, "join_probe_count", "join_probe_write"});
}
// the outer entry.  `marks`: the bitmap of nqe_join_marks, or null
std::unique_ptr<nqe_table> probe_outer(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key, bool keep_probe, uint32_t *marks) {
    if (right_key < 0 || size_t(right_key) >= right->cols.size()) fail(NQE_ERR_LOGICAL, "ColumnExpr must has name or idx");
    const DevColumn &rk_orig = right->cols[size_t(right_key)];
    check_key_types(jt->key_dtype, rk_orig.dtype);
    if (jt->left_cols.size() + right->cols.size() > size_t(MAX_JOIN_COLS)) fail(NQE_ERR_NOT_SUPPORTED, "join output wider than 32 columns");
    if (keep_probe && jt->left_rows > int64_t(OUTER_NULL_START)) fail(NQE_ERR_NOT_SUPPORTED, "outer join: a build side of 2^32 rows collides with the no-match mark");
    DevColumn rk_codes;
    const DevColumn &rk = encoded_probe_key(ctx, jt, rk_orig, rk_codes);
    return probe_expand(ctx, jt, right, right_key, rk, rk_orig, ExpandMode{true, keep_probe, marks, "join_outer_count", "join_outer_write"});
}

// exact null counts of the nullable columns of `out` (count_set_bits_kernel per column, one read-back for all of them); declared in
// nqe_internal.hpp (set_ops.hip calls it too): true when it waited for the stream
} // namespace
bool count_nulls_exact(nqe_ctx *ctx, nqe_table *out, const char *label) {
    std::vector<size_t> which;
    for (size_t c = 0; c < out->cols.size(); ++c)
        if (out->cols[c].validity && out->cols[c].null_count < 0) which.push_back(c);
    if (which.empty()) return false;
    if (out->rows == 0) {
        for (size_t c : which) out->cols[c].null_count = 0;
        return false;
    }
    BufRef set = dev_alloc_zero(ctx, which.size() * 8);
    for (size_t k = 0; k < which.size(); ++k)
        launch(ctx, label, count_set_bits_kernel, dim3(stream_grid(ctx, (out->rows + 63) / 64, 256)), dim3(256), 0,
               (const uint64_t *)out->cols[which[k]].validity->ptr, out->rows, (unsigned long long *)set->ptr + k);
    std::vector<unsigned long long> h(which.size());
    NQE_HIP_CHECK(hipMemcpyAsync(h.data(), set->ptr, which.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    sync(ctx);
    for (size_t k = 0; k < which.size(); ++k) out->cols[which[k]].null_count = out->rows - int64_t(h[k]);
    return true;
}
namespace {
// m rows of NULL: zero words / false bits / zero-length strings under an all-zero validity buffer (none at 0 rows: no NULL-extended row)
DevColumn null_column(nqe_ctx *ctx, int dtype, int64_t m) {
    DevColumn c;
    c.dtype = dtype;
    c.length = m;
    if (dtype == NQE_UTF8) {
        c.values = dev_alloc_zero(ctx, size_t(m + 1) * 4 + 8);
        c.data = dev_alloc(ctx, 8);
    } else if (dtype == NQE_BOOLEAN) {
        c.values = dev_alloc_zero(ctx, bitmap_alloc_bytes(m));
    } else {
        c.values = dev_alloc_zero(ctx, size_t(m) * 8);
    }
    if (m) {
        c.validity = dev_alloc_zero(ctx, bitmap_alloc_bytes(m));
        c.null_count = m;
    }
    return c;
}
// the build rows whose bit is set (anti: not set), in ascending build row: KEEP mask over the build rows (marked_build_kernel) →
// compaction of the visible left columns.  What else the output holds, and its null counts, are the caller's
std::unique_ptr<nqe_table> compact_marked_build(nqe_ctx *ctx, const nqe_join_table *jt, const uint32_t *marks, bool anti, const char *label) {
    const int64_t n = jt->left_rows;
    DevColumn codes;
    const uint64_t *bkeys = nullptr;
    if (!jt->direct) { // duplicate keys: the row's own key finds the bit its key group shares
        const DevColumn &kc = jt->left_cols[size_t(jt->left_key)];
        bkeys = encoded_probe_key(ctx, jt, kc, codes).words();
    }
    BufRef counts;
    KeepMask km = new_keep_mask(ctx, n, &counts);
    if (km.ntiles)
        launch(ctx, label, anti ? marked_build_kernel<true> : marked_build_kernel<false>, dim3(stream_grid(ctx, km.ntiles, 4)), dim3(256), 0, bkeys, n, km.ntiles, lookup_of(jt), marks,
               (uint64_t *)km.keep->ptr, (uint32_t *)counts->ptr);
    km = finish_mask(ctx, km, counts); // (waits for the stream: the codes may go)
    auto out = std::make_unique<nqe_table>();
    out->ctx = ctx;
    out->rows = km.total;
    const size_t visible = jt->left_cols.size() - (jt->keys ? 1 : 0); // (the hidden code column of a join on several keys, the last one, is not gathered)
    for (size_t c = 0; c < visible; ++c) out->cols.push_back(compact_column(ctx, jt->left_cols[c], km));
    return out;
}
// the outer joins' build-preserving side: the build rows whose bit is not set, every right column NULL
std::unique_ptr<nqe_table> unmatched_build(nqe_ctx *ctx, const nqe_join_table *jt, const uint32_t *marks, const int32_t *right_dtypes, int num_right) {
    if (jt->left_cols.size() + size_t(num_right) > size_t(MAX_JOIN_COLS)) fail(NQE_ERR_NOT_SUPPORTED, "join output wider than 32 columns");
    auto out = compact_marked_build(ctx, jt, marks, true, "join_outer_unmatched");
    for (int k = 0; k < num_right; ++k) out->cols.push_back(null_column(ctx, right_dtypes[k], out->rows));
    count_nulls_exact(ctx, out.get());
    sync(ctx);
    return out;
}

// ---- semi and anti joins (quirk Q22): which probe rows have a partner (SEMI) or none (ANTI), and the same question for the build rows
// through the marks.  One keep-mask pass (semi_keep_kernel) and the selection's compaction over the caller's own columns: no build
// column is read or written, no per-row word exists.  The existence form follows the build form (the map at the top of this file):
//   build_unique_dense with dense_full                      → RANGE  (a comparison, no memory access beyond the key)
//   build_unique_dense / build_sorted_dense with `presence` → BITMAP (one bit per key)
//   other dense tables (no payload copies, duplicate keys), and every pass over a dense table that marks → LOOKUP (dense[d] != 0; with marks lookup_meta)
//   hashed tables, wave-cooperatively (semi_keep_coop_kernel): the packed {key, payload} words where the build made them → PACKED, its
//   16-byte pairs → PAIRS, else — and for every pass that marks — the {key, meta} slots → COOP.  NQE_SEMI_NO_COOP=1 (a diagnostic switch,
//   read per call) sends hashed tables through LOOKUP's per-lane probe_one instead: same result (profiles/semi_join has the A/B).
template <int FORM, bool NULLS, bool MARKS> void launch_semi_keep(nqe_ctx *ctx, const char *label, bool anti, bool want_out, dim3 grid, const uint64_t *rk, int64_t n, int64_t ntiles,
                                                                 const Lookup &L, const uint32_t *presence, const SemiValid &sv, uint32_t *marks, uint64_t *keep, uint32_t *counts) {
    if constexpr (MARKS) {
        if (!want_out) return launch(ctx, label, semi_keep_kernel<FORM, false, NULLS, true, false>, grid, dim3(256), 0, rk, n, ntiles, L, presence, sv, marks, keep, counts);
    }
    if (anti) launch(ctx, label, semi_keep_kernel<FORM, true, NULLS, MARKS, true>, grid, dim3(256), 0, rk, n, ntiles, L, presence, sv, marks, keep, counts);
    else launch(ctx, label, semi_keep_kernel<FORM, false, NULLS, MARKS, true>, grid, dim3(256), 0, rk, n, ntiles, L, presence, sv, marks, keep, counts);
}
template <int TABLE, bool NULLS, bool MARKS> void launch_semi_coop(nqe_ctx *ctx, const char *label, bool anti, bool want_out, dim3 grid, const uint64_t *rk, int64_t n, int64_t ntiles,
                                                                  const SemiHashed &H, const SemiValid &sv, uint32_t *marks, uint64_t *keep, uint32_t *counts) {
    if constexpr (MARKS) {
        if (!want_out) return launch(ctx, label, semi_keep_coop_kernel<TABLE, false, NULLS, true, false>, grid, dim3(256), 0, rk, n, ntiles, H, sv, marks, keep, counts);
    }
    if (anti) launch(ctx, label, semi_keep_coop_kernel<TABLE, true, NULLS, MARKS, true>, grid, dim3(256), 0, rk, n, ntiles, H, sv, marks, keep, counts);
    else launch(ctx, label, semi_keep_coop_kernel<TABLE, false, NULLS, MARKS, true>, grid, dim3(256), 0, rk, n, ntiles, H, sv, marks, keep, counts);
}
// `right_with_key`: the caller's columns (the first `out_cols`) and, as its last column, the key to look up — the key column itself, or
// the code column of a join on several keys.  `key_valid`: the validity bitmaps of the probe key columns when NULL keys match nothing
// (null otherwise).  Returns null for the mark-only pass (`want_out` false).
std::unique_ptr<nqe_table> probe_semi(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right_with_key, size_t out_cols, bool anti, const SemiValid *key_valid,
                                      uint32_t *marks, bool want_out) {
    DevColumn rk_codes;
    const DevColumn &rk = encoded_probe_key(ctx, jt, right_with_key->cols.back(), rk_codes);
    const int64_t n = right_with_key->rows;
    BufRef counts;
    KeepMask km;
    if (want_out) km = new_keep_mask(ctx, n, &counts);
    const int64_t ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    SemiValid sv;
    std::memset(&sv, 0, sizeof(sv));
    bool nulls = false;
    if (key_valid)
        for (int j = 0; j < NQE_MAX_JOIN_KEYS; ++j) {
            sv.v[j] = key_valid->v[j];
            nulls = nulls || sv.v[j] != nullptr;
        }
    const bool hashed = !jt->dense && getenv("NQE_SEMI_NO_COOP") == nullptr;
    const int table = (marks || !jt->slotsp) ? SEMI_SLOTS : (jt->pp.pbits ? SEMI_PACKED : SEMI_PAIRS);
    const int form = hashed ? -1 : (marks ? SEMI_LOOKUP : (jt->dense_full ? SEMI_RANGE : (jt->presence ? SEMI_BITMAP : SEMI_LOOKUP)));
    const char *label = hashed ? (table == SEMI_SLOTS ? "join_semi_keep_coop" : (table == SEMI_PACKED ? "join_semi_keep_packed" : "join_semi_keep_pairs"))
                               : (form == SEMI_RANGE ? "join_semi_keep_range" : (form == SEMI_BITMAP ? "join_semi_keep_bitmap" : "join_semi_keep_lookup"));
    if (getenv("NQE_DEBUG"))
        fprintf(stderr, "[nqe] join semi: n=%lld %s anti=%d nulls=%d marks=%d out=%d\n", (long long)n, label, int(anti), int(nulls), int(marks != nullptr), int(want_out));
    if (ntiles) {
        const dim3 grid(stream_grid(ctx, ntiles, 4));
        const Lookup L = lookup_of(jt);
        const uint32_t *pp = jt->presence ? (const uint32_t *)jt->presence->ptr : (const uint32_t *)nullptr;
        uint64_t *kp = want_out ? (uint64_t *)km.keep->ptr : (uint64_t *)nullptr;
        uint32_t *cp = want_out ? (uint32_t *)counts->ptr : (uint32_t *)nullptr;
        SemiHashed H;
        std::memset(&H, 0, sizeof(H));
        if (hashed) { // (a dense table built without sorting has no hash table at all)
            H.tab = (const ulonglong2 *)(table == SEMI_SLOTS ? jt->slots->ptr : jt->slotsp->ptr);
            H.cap = jt->cap;
            H.shift = jt->shift;
            H.filler = jt->filler;
            H.pp = jt->pp;
        }
#define NQE_SEMI(FORM, MARKS)                                                                                                                   \
    (nulls ? launch_semi_keep<FORM, true, MARKS>(ctx, label, anti, want_out, grid, rk.words(), n, ntiles, L, pp, sv, marks, kp, cp)             \
           : launch_semi_keep<FORM, false, MARKS>(ctx, label, anti, want_out, grid, rk.words(), n, ntiles, L, pp, sv, marks, kp, cp))
#define NQE_SEMI_COOP(TABLE, MARKS)                                                                                                             \
    (nulls ? launch_semi_coop<TABLE, true, MARKS>(ctx, label, anti, want_out, grid, rk.words(), n, ntiles, H, sv, marks, kp, cp)                \
           : launch_semi_coop<TABLE, false, MARKS>(ctx, label, anti, want_out, grid, rk.words(), n, ntiles, H, sv, marks, kp, cp))
        if (hashed && marks) NQE_SEMI_COOP(SEMI_SLOTS, true);
        else if (hashed && table == SEMI_SLOTS) NQE_SEMI_COOP(SEMI_SLOTS, false);
        else if (hashed && table == SEMI_PACKED) NQE_SEMI_COOP(SEMI_PACKED, false);
        else if (hashed) NQE_SEMI_COOP(SEMI_PAIRS, false);
        else if (marks) NQE_SEMI(SEMI_LOOKUP, true);
        else if (form == SEMI_RANGE) NQE_SEMI(SEMI_RANGE, false);
        else if (form == SEMI_BITMAP) NQE_SEMI(SEMI_BITMAP, false);
        else NQE_SEMI(SEMI_LOOKUP, false);
#undef NQE_SEMI
#undef NQE_SEMI_COOP
    }
    if (!want_out) {
        sync(ctx); // the probe codes are released on return
        return nullptr;
    }
    km = finish_mask(ctx, km, counts);
    auto out = std::make_unique<nqe_table>();
    out->ctx = ctx;
    out->rows = km.total;
    for (size_t c = 0; c < out_cols; ++c) out->cols.push_back(compact_column(ctx, right_with_key->cols[c], km));
    count_nulls_exact(ctx, out.get(), "join_semi_null_count");
    sync(ctx);
    return out;
}
// the semi / anti joins' build side: the visible left columns and nothing else
std::unique_ptr<nqe_table> marked_build(nqe_ctx *ctx, const nqe_join_table *jt, const uint32_t *marks, bool anti) {
    auto out = compact_marked_build(ctx, jt, marks, anti, "join_semi_marked");
    count_nulls_exact(ctx, out.get(), "join_semi_null_count");
    sync(ctx);
    return out;
}

std::unique_ptr<nqe_table> probe_table(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right, int right_key) {
    if (right_key < 0 || size_t(right_key) >= right->cols.size()) fail(NQE_ERR_LOGICAL, "ColumnExpr must has name or idx");
    const DevColumn &rk_orig = right->cols[size_t(right_key)];
    check_key_types(jt->key_dtype, rk_orig.dtype);
    DevColumn rk_codes;
    const DevColumn &rk = encoded_probe_key(ctx, jt, rk_orig, rk_codes);
    if (jt->left_cols.size() + right->cols.size() > size_t(MAX_JOIN_COLS)) fail(NQE_ERR_NOT_SUPPORTED, "join output wider than 32 columns");
    bool right_plain = true;
    for (auto &c : right->cols) right_plain = right_plain && is_plain_word(c);
    if (jt->dense_payload && right_plain) return probe_dense_payload(ctx, jt, right, right_key, rk);
    if (jt->direct) return probe_unique(ctx, jt, right, right_key, rk, right_plain);
    return probe_duplicates(ctx, jt, right, right_key, rk, rk_orig);
}

// a table built on several keys is probed through nqe_hash_join_probe_keys alone: its key is a code column the caller never sees
void refuse_tuple_table(const nqe_join_table *jt, const char *who) {
    if (jt->keys) fail(NQE_ERR_INVALID_ARGUMENT, std::string(who) + ": the join table was built on several keys (nqe_hash_join_probe_keys probes it)");
}
bool foreign_marks(nqe_ctx *ctx, const nqe_join_table *build, const nqe_join_marks *marks) {
    return marks->ctx != ctx || marks->table != build || marks->rows != build->left_rows;
}
void check_outer_args(nqe_ctx *ctx, const nqe_join_table *build, uint32_t flags, const nqe_join_marks *marks) {
    if (flags & ~NQE_JOIN_KEEP_PROBE) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_outer: unknown flag bits");
    if (marks && foreign_marks(ctx, build, marks)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_outer: the marks belong to another join table or context");
}

} // namespace

// ---- the doors of join_keys.hip (join_keys_state.hpp)
void join_check_key_types(int ldt, int rdt) { check_key_types(ldt, rdt); }
nqe_join_table *join_build_coded(nqe_ctx *ctx, const nqe_table *left_with_code, std::shared_ptr<const JoinKeysState> keys) {
    flags_reset(ctx);
    std::unique_ptr<nqe_join_table> jt = build_table(ctx, left_with_code, int(left_with_code->cols.size()) - 1);
    jt->keys = std::move(keys);
    return jt.release();
}
const JoinKeysState *join_table_keys(const nqe_join_table *jt) { return jt->keys.get(); }
size_t join_table_columns(const nqe_join_table *jt) { return jt->left_cols.size(); }
void join_check_outer_args(nqe_ctx *ctx, const nqe_join_table *jt, uint32_t flags, const nqe_join_marks *marks) { check_outer_args(ctx, jt, flags, marks); }
nqe_table *join_probe_coded(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right_with_code, uint32_t flags, nqe_join_marks *marks) {
    const int key = int(right_with_code->cols.size()) - 1;
    flags_reset(ctx);
    if (flags == 0 && !marks) return probe_table(ctx, jt, right_with_code, key).release();
    return probe_outer(ctx, jt, right_with_code, key, (flags & NQE_JOIN_KEEP_PROBE) != 0, marks ? (uint32_t *)marks->bits->ptr : (uint32_t *)nullptr).release();
}
void join_check_semi_args(nqe_ctx *ctx, const nqe_join_table *jt, uint32_t flags, const nqe_join_marks *marks) {
    if (flags & ~(NQE_SEMI_ANTI | NQE_SEMI_NULL_KEY_UNMATCHED)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_semi: unknown flag bits");
    if (marks && foreign_marks(ctx, jt, marks)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_semi: the marks belong to another join table or context");
}
const DevColumn &join_table_key_column(const nqe_join_table *jt) { return jt->left_cols[size_t(jt->left_key)]; }
nqe_table *join_semi_coded(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right_with_key, size_t out_cols, uint32_t flags, const uint8_t *const *key_valid,
                           nqe_join_marks *marks, bool want_out) {
    SemiValid sv;
    std::memset(&sv, 0, sizeof(sv));
    if (key_valid)
        for (int j = 0; j < NQE_MAX_JOIN_KEYS; ++j) sv.v[j] = key_valid[j];
    flags_reset(ctx);
    return probe_semi(ctx, jt, right_with_key, out_cols, (flags & NQE_SEMI_ANTI) != 0, key_valid ? &sv : nullptr, marks ? (uint32_t *)marks->bits->ptr : (uint32_t *)nullptr, want_out)
        .release();
}

} // namespace nqe

using namespace nqe;

extern "C" {

nqe_status nqe_hash_join_build(nqe_ctx *ctx, const nqe_table *left, int32_t left_key, nqe_join_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !left || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    flags_reset(ctx);
    *out = build_table(ctx, left, left_key).release();
    NQE_API_END()
}

nqe_status nqe_hash_join_probe(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, int32_t right_key,
                               nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !right || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    refuse_tuple_table(build, "nqe_hash_join_probe");
    flags_reset(ctx);
    *out = probe_table(ctx, build, right, right_key).release();
    NQE_API_END()
}

nqe_status nqe_join_table_release(nqe_join_table *jt) {
    delete jt;
    return NQE_OK;
}

nqe_status nqe_join_marks_create(nqe_ctx *ctx, const nqe_join_table *build, nqe_join_marks **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !out || build->ctx != ctx) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    auto m = std::make_unique<nqe_join_marks>();
    m->ctx = ctx;
    m->table = build;
    m->rows = build->left_rows;
    m->bits = dev_alloc_zero(ctx, size_t((build->left_rows + 31) / 32) * 4 + 8);
    *out = m.release();
    NQE_API_END()
}

nqe_status nqe_join_marks_release(nqe_join_marks *marks) {
    delete marks;
    return NQE_OK;
}

nqe_status nqe_hash_join_probe_outer(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, int32_t right_key, uint32_t flags,
                                     nqe_join_marks *marks, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !right || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    refuse_tuple_table(build, "nqe_hash_join_probe_outer");
    check_outer_args(ctx, build, flags, marks);
    flags_reset(ctx);
    *out = probe_outer(ctx, build, right, right_key, (flags & NQE_JOIN_KEEP_PROBE) != 0, marks ? (uint32_t *)marks->bits->ptr : (uint32_t *)nullptr).release();
    NQE_API_END()
}

nqe_status nqe_hash_join_unmatched_build(nqe_ctx *ctx, const nqe_join_table *build, const nqe_join_marks *marks, const int32_t *right_dtypes,
                                         int32_t num_right, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (!marks) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_unmatched_build: marks are required");
    if (foreign_marks(ctx, build, marks)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_unmatched_build: the marks belong to another join table or context");
    if (num_right < 0 || (num_right > 0 && !right_dtypes)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_unmatched_build: bad right_dtypes");
    for (int32_t k = 0; k < num_right; ++k) {
        if (right_dtypes[k] < NQE_NULLTYPE || right_dtypes[k] > NQE_UTF8) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_unmatched_build: a dtype outside nqe_dtype");
        if (right_dtypes[k] == NQE_NULLTYPE) fail(NQE_ERR_NOT_SUPPORTED, "nqe_hash_join_unmatched_build: no column of DataType::Null");
    }
    flags_reset(ctx);
    *out = unmatched_build(ctx, build, (const uint32_t *)marks->bits->ptr, right_dtypes, num_right).release();
    NQE_API_END()
}

nqe_status nqe_hash_join_marked_build(nqe_ctx *ctx, const nqe_join_table *build, const nqe_join_marks *marks, uint32_t flags, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (!marks) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_marked_build: marks are required");
    if (flags & ~NQE_SEMI_ANTI) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_marked_build: unknown flag bits");
    if (foreign_marks(ctx, build, marks)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_marked_build: the marks belong to another join table or context");
    flags_reset(ctx);
    *out = marked_build(ctx, build, (const uint32_t *)marks->bits->ptr, (flags & NQE_SEMI_ANTI) != 0).release();
    NQE_API_END()
}

nqe_status nqe_hash_join_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, int32_t left_key,
                                 int32_t right_key, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !left || !right || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (left_key < 0 || right_key < 0) // empty `on` (hash_join.rs:125-129)
        fail(NQE_ERR_PLAN, "Inner Join on Conditions can't not be empty");
    flags_reset(ctx);
    std::unique_ptr<nqe_join_table> jt = build_table(ctx, left, left_key);
    *out = probe_table(ctx, jt.get(), right, right_key).release();
    NQE_API_END()
}

} // extern "C"

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::iota_u32_kernel);
