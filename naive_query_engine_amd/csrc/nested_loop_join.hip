// nested_loop_join.hip — NestedLoopJoin::execute for one batch pair (reference: src/physical_plan/nested_loop_join.rs:110-175), quirk Q17.
//
// The reference walks `for x in left { for y in right }` and appends (x, y) where both keys are valid and equal, then takes every
// column of both sides by the two position lists.  Here: L·R key comparisons on the device, output in the same (x, y) order.
//
//   nlj_count   grid over (outer tile of 1024 rows × inner chunk): a workgroup stages its chunk's keys in LDS 2048 at a time (plus one
//               validity bit per key when the inner key column has a bitmap), every lane holds FOUR outer keys in registers and walks
//               the staged keys in ascending y — all lanes read the same 16 bytes (an LDS broadcast, two keys per read, eight
//               comparisons per read) — and leaves counts[x·C + c]
//   scan        exclusive 64-bit scan of the counts in row-major (x, c) order (sort.hip); its total is the call's host wait
//   nlj_emit    the same walk; a lane writes its matches from offsets[x·C + c] on: ascending y inside a cell, cells in (x, c) order,
//               so the positions come out sorted by (x, y)
//   take        context.hip's take_column for every column of both sides (validity preserved)
//
// C, the chunks per outer row: as many as it takes to put NLJ_WG_PER_CU workgroups on every CU when the outer side alone has too few
// tiles, and never more than the inner side has LDS fills: C = min(ceil(R / 2048), max(1, ceil(NLJ_WG_PER_CU · CUs / tiles))).  The
// count matrix has L·C <= L + 1024 · NLJ_WG_PER_CU · CUs entries (2^20 on 256 CUs) of 4 bytes, its scan as many of 8.
//
// Keys are one 8-byte word per row: Int64 / UInt64 compare the words, Float64 compares as doubles (NaN ≠ NaN, −0.0 = 0.0), Utf8 keys
// are first encoded to representative-row codes (strings.hip) and then compared as integers; NULL is decided by the key columns' own
// bitmaps.  Everything is written with ordinary vector stores.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "device_utils.hpp"
#include "nqe_internal.hpp"

namespace nqe {

namespace {

constexpr int NLJ_THREADS = 256;
constexpr int NLJ_KPL = 4;                           // outer keys per lane
constexpr int64_t NLJ_TILE = NLJ_THREADS * NLJ_KPL;  // outer rows per workgroup
constexpr int NLJ_LDS_KEYS = 2048;                   // inner keys per LDS fill (16 KiB)
constexpr int NLJ_GROUP = 8;                         // inner keys per unrolled step (four 16-byte reads)
constexpr int NLJ_WG_PER_CU = 4;
constexpr int64_t NLJ_MAX_GRID = int64_t(1) << 20;   // cells beyond it are grid-strided

typedef uint64_t nlj_u64x2 __attribute__((ext_vector_type(2)));

struct NljArgs {
    const uint64_t *lkeys;
    const uint8_t *lvalid; // null: every outer key is valid
    int64_t L;
    const uint64_t *rkeys;
    const uint8_t *rvalid;
    int64_t R;
    int64_t C, chunk_len, tiles; // chunk_len is a multiple of NLJ_LDS_KEYS
    uint32_t *counts;            // [L · C]                 (count pass)
    const uint64_t *offsets;     // [L · C + 1]             (emit pass)
    int64_t *x_pos, *y_pos;      // [total]
};

template <bool F64> __device__ __forceinline__ bool nlj_eq(uint64_t a, uint64_t b) {
    if (F64) return __longlong_as_double((long long)a) == __longlong_as_double((long long)b);
    return a == b;
}

// RNULL: the inner key column has a validity bitmap.  EMIT: write positions instead of counting.
template <bool F64, bool RNULL, bool EMIT> __global__ void __launch_bounds__(NLJ_THREADS) nlj_kernel(NljArgs a) {
    __shared__ __attribute__((aligned(16))) uint64_t skeys[NLJ_LDS_KEYS];
    __shared__ uint64_t smask[NLJ_LDS_KEYS / 64];
    const int64_t ncells = a.tiles * a.C;
    for (int64_t cell = blockIdx.x; cell < ncells; cell += gridDim.x) {
        const int64_t tile = cell / a.C, c = cell - tile * a.C;
        uint64_t xk[NLJ_KPL];
        int64_t xrow[NLJ_KPL];
        bool act[NLJ_KPL];
        uint32_t cnt[NLJ_KPL]; // matches of the cell (a chunk is capped below 2^32 keys)
        uint64_t acc[NLJ_KPL]; // emit: the next output position
#pragma unroll
        for (int k = 0; k < NLJ_KPL; ++k) {
            xrow[k] = tile * NLJ_TILE + int64_t(k) * NLJ_THREADS + threadIdx.x;
            act[k] = xrow[k] < a.L && (!a.lvalid || get_bit(a.lvalid, xrow[k]));
            xk[k] = act[k] ? a.lkeys[xrow[k]] : 0;
            cnt[k] = 0;
            acc[k] = EMIT && xrow[k] < a.L ? a.offsets[xrow[k] * a.C + c] : 0;
        }
        const int64_t y_begin = c * a.chunk_len, y_end = min(a.R, y_begin + a.chunk_len);
        for (int64_t y0 = y_begin; y0 < y_end; y0 += NLJ_LDS_KEYS) {
            const int n = int(min(int64_t(NLJ_LDS_KEYS), y_end - y0));
            __syncthreads(); // the previous fill has been read
            for (int i = threadIdx.x; i < NLJ_LDS_KEYS; i += NLJ_THREADS) {
                const bool in = i < n;
                skeys[i] = in ? a.rkeys[y0 + i] : 0;
                if (RNULL) { // 64 consecutive keys per wave and step: one mask word
                    const uint64_t w = __ballot(in && get_bit(a.rvalid, y0 + i));
                    if (lane_id() == 0) smask[i >> 6] = w;
                }
            }
            __syncthreads();
            const int full = RNULL ? 0 : n / NLJ_GROUP, groups = (n + NLJ_GROUP - 1) / NLJ_GROUP;
            const nlj_u64x2 *s2 = reinterpret_cast<const nlj_u64x2 *>(skeys);
            if (!EMIT && !RNULL) {
                // whole groups of valid keys: compare and add
                for (int g = 0; g < full; ++g) {
                    uint64_t kk[NLJ_GROUP];
#pragma unroll
                    for (int p = 0; p < NLJ_GROUP / 2; ++p) {
                        const nlj_u64x2 v = s2[g * (NLJ_GROUP / 2) + p];
                        kk[2 * p] = v.x;
                        kk[2 * p + 1] = v.y;
                    }
#pragma unroll
                    for (int k = 0; k < NLJ_KPL; ++k)
#pragma unroll
                        for (int j = 0; j < NLJ_GROUP; ++j) cnt[k] += nlj_eq<F64>(xk[k], kk[j]) ? 1u : 0u;
                }
            }
            // groups with a mask (NULL inner keys, the ragged last group) and the emit pass: a match bit per key of the group
            for (int g = (!EMIT && !RNULL) ? full : 0; g < groups; ++g) {
                uint64_t kk[NLJ_GROUP];
#pragma unroll
                for (int p = 0; p < NLJ_GROUP / 2; ++p) {
                    const nlj_u64x2 v = s2[g * (NLJ_GROUP / 2) + p];
                    kk[2 * p] = v.x;
                    kk[2 * p + 1] = v.y;
                }
                uint32_t ok; // which keys of the group exist and are valid (the same for every lane)
                if (RNULL) ok = uint32_t(smask[g >> 3] >> ((g & 7) * NLJ_GROUP)) & 0xffu;
                else ok = g < n / NLJ_GROUP ? 0xffu : (1u << (n % NLJ_GROUP)) - 1u;
#pragma unroll
                for (int k = 0; k < NLJ_KPL; ++k) {
                    uint32_t bits = 0;
#pragma unroll
                    for (int j = 0; j < NLJ_GROUP; ++j) bits |= nlj_eq<F64>(xk[k], kk[j]) ? (1u << j) : 0u;
                    bits &= ok;
                    if (!EMIT) {
                        cnt[k] += uint32_t(__popc(bits));
                    } else if (bits && act[k]) {
                        const int64_t yb = y0 + int64_t(g) * NLJ_GROUP;
                        while (bits) {
                            const int j = __ffs(int(bits)) - 1;
                            bits &= bits - 1;
                            a.x_pos[acc[k]] = xrow[k];
                            a.y_pos[acc[k]] = yb + j;
                            ++acc[k];
                        }
                    }
                }
            }
        }
        if (!EMIT) {
#pragma unroll
            for (int k = 0; k < NLJ_KPL; ++k)
                if (xrow[k] < a.L) a.counts[xrow[k] * a.C + c] = act[k] ? cnt[k] : 0u;
        }
    }
}

// out[col] += Σ_j len(src[pos[j]]) over valid slots: the byte size of a Utf8 output column before it is allocated
struct NljUtf8Len {
    const int32_t *off;
    const uint8_t *valid;
    const int64_t *pos;
};
constexpr int NLJ_MAX_UTF8 = 32;
struct NljUtf8Args {
    NljUtf8Len c[NLJ_MAX_UTF8];
    int64_t m;
    unsigned long long *out;
};
__global__ void __launch_bounds__(NLJ_THREADS) nlj_utf8_bytes_kernel(NljUtf8Args a) {
    const NljUtf8Len c = a.c[blockIdx.y];
    unsigned long long sum = 0;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < a.m; j += stride) {
        const int64_t i = c.pos[j];
        if (!c.valid || get_bit(c.valid, i)) sum += uint64_t(c.off[i + 1] - c.off[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane_id() == 0 && sum) atomicAdd(a.out + blockIdx.y, sum);
}

template <bool EMIT> void nlj_launch(nqe_ctx *ctx, bool f64, bool rnull, unsigned grid, const NljArgs &a) {
    const char *name = EMIT ? "nlj_emit" : "nlj_count";
    auto k = f64 ? (rnull ? nlj_kernel<true, true, EMIT> : nlj_kernel<true, false, EMIT>) : (rnull ? nlj_kernel<false, true, EMIT> : nlj_kernel<false, false, EMIT>);
    launch(ctx, name, k, dim3(grid), dim3(NLJ_THREADS), 0, a);
}

[[noreturn]] void fail_too_large(const char *what) { fail(NQE_ERR_OUT_OF_MEMORY, std::string("nested loop join: ") + what + " overflows int64"); }

// bytes of an output column of `m` rows without its Utf8 payload
int64_t column_bytes(const DevColumn &c, int64_t m) {
    int64_t b = 0, v = 0;
    if (is_word_type(c.dtype)) {
        if (__builtin_mul_overflow(m, int64_t(8), &b)) fail_too_large("a column's byte size");
    } else if (c.dtype == NQE_UTF8) {
        if (__builtin_add_overflow(m, int64_t(1), &b) || __builtin_mul_overflow(b, int64_t(4), &b)) fail_too_large("a column's byte size");
    } else {
        b = m / 8 + 8;
    }
    if (c.validity) v = m / 8 + 8;
    if (__builtin_add_overflow(b, v, &b)) fail_too_large("a column's byte size");
    return b;
}

} // namespace

} // namespace nqe

using namespace nqe;

nqe_status nqe_nested_loop_join_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, int32_t left_key, int32_t right_key,
                                        nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !left || !right || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (left_key < 0 || size_t(left_key) >= left->cols.size() || right_key < 0 || size_t(right_key) >= right->cols.size())
        fail(NQE_ERR_NOT_SUPPORTED, "nested loop join: key column index out of range");
    const DevColumn &lk = left->cols[size_t(left_key)], &rk = right->cols[size_t(right_key)];
    // the reference's order: the data types are compared first (:118-124), then the match arms (:128-155)
    if (lk.dtype != rk.dtype) fail(NQE_ERR_PLAN, "Join on left and right data type should be same");
    if (!(is_word_type(lk.dtype) || lk.dtype == NQE_UTF8))
        fail(NQE_ERR_NOT_SUPPORTED, "nested loop join: keys of this type are not implemented (nested_loop_join.rs panics: unimplemented!())");
    const int64_t L = left->rows, R = right->rows;

    int64_t total = 0;
    int64_t C = 1, chunk_len = NLJ_LDS_KEYS;
    const int64_t tiles = (L + NLJ_TILE - 1) / NLJ_TILE;
    BufRef offsets;
    NljArgs a;
    std::memset(&a, 0, sizeof(a));
    DevColumn lcodes, rcodes; // Utf8 keys: the code columns live until the emit pass has run
    bool f64 = false;
    unsigned grid = 1;
    if (L > 0 && R > 0) {
        const DevColumn *lkc = &lk, *rkc = &rk;
        if (lk.dtype == NQE_UTF8) {
            Utf8Dict dict;
            lcodes = utf8_encode_build(ctx, lk, &dict);
            rcodes = utf8_encode_probe(ctx, rk, dict);
            lkc = &lcodes;
            rkc = &rcodes;
        }
        f64 = lk.dtype == NQE_FLOAT64;
        // C (see the head of the file); a chunk stays below 2^31 keys so that a cell's count fits 32 bits
        const int64_t fills = (R + NLJ_LDS_KEYS - 1) / NLJ_LDS_KEYS;
        const int64_t want = (int64_t(ctx->num_cus) * NLJ_WG_PER_CU + tiles - 1) / tiles;
        C = std::max<int64_t>(1, std::min(fills, want));
        C = std::max(C, (R >> 31) + 1);
        chunk_len = ((R + C - 1) / C + NLJ_LDS_KEYS - 1) / NLJ_LDS_KEYS * NLJ_LDS_KEYS;
        C = (R + chunk_len - 1) / chunk_len;
        int64_t cells = 0, cbytes = 0;
        if (__builtin_mul_overflow(L, C, &cells) || __builtin_mul_overflow(cells + 1, int64_t(12), &cbytes)) fail_too_large("the count matrix");
        a.lkeys = lkc->words();
        a.lvalid = lk.valid();
        a.L = L;
        a.rkeys = rkc->words();
        a.rvalid = rk.valid();
        a.R = R;
        a.C = C;
        a.chunk_len = chunk_len;
        a.tiles = tiles;
        BufRef counts = dev_alloc(ctx, size_t(cells) * 4);
        offsets = dev_alloc(ctx, size_t(cells + 1) * 8);
        a.counts = static_cast<uint32_t *>(counts->ptr);
        grid = unsigned(std::min<int64_t>(tiles * C, NLJ_MAX_GRID));
        nlj_launch<false>(ctx, f64, a.rvalid != nullptr, grid, a);
        exclusive_scan_u32_to_u64(ctx, a.counts, static_cast<uint64_t *>(offsets->ptr), cells);
        const uint64_t t = read_scalar(ctx, static_cast<const uint64_t *>(offsets->ptr) + cells);
        if (t > uint64_t(INT64_MAX)) fail_too_large("the match count");
        total = int64_t(t);
    }

    // sizes, before anything of the output's size is allocated: the two position lists and every column (Utf8 payloads excepted: they
    // need the positions, and are checked below before they are allocated)
    int64_t need = 0;
    if (__builtin_mul_overflow(total, int64_t(16), &need)) fail_too_large("the position lists");
    for (const nqe_table *t : {left, right})
        for (const DevColumn &c : t->cols)
            if (__builtin_add_overflow(need, column_bytes(c, total), &need)) fail_too_large("the output's byte size");
    size_t free_b = 0, total_b = 0;
    NQE_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (uint64_t(need) > uint64_t(total_b))
        fail(NQE_ERR_OUT_OF_MEMORY, "nested loop join: " + std::to_string(total) + " matches need " + std::to_string(need) + " bytes, the device has " + std::to_string(total_b));

    BufRef x_pos = dev_alloc(ctx, size_t(total) * 8 + 8), y_pos = dev_alloc(ctx, size_t(total) * 8 + 8);
    if (total > 0) {
        a.offsets = static_cast<const uint64_t *>(offsets->ptr);
        a.x_pos = static_cast<int64_t *>(x_pos->ptr);
        a.y_pos = static_cast<int64_t *>(y_pos->ptr);
        nlj_launch<true>(ctx, f64, a.rvalid != nullptr, grid, a);
    }
    offsets.reset();

    // Utf8 output columns: their byte sizes from the positions; more than int32 offsets address is refused (arrow's take would overflow)
    if (total > 0) {
        NljUtf8Args ua;
        std::memset(&ua, 0, sizeof(ua));
        ua.m = total;
        std::vector<unsigned long long> sizes;
        auto flush = [&](int n) {
            if (n == 0) return;
            BufRef d = dev_alloc_zero(ctx, size_t(n) * 8);
            ua.out = static_cast<unsigned long long *>(d->ptr);
            launch(ctx, "nlj_utf8_bytes", nlj_utf8_bytes_kernel, dim3(unsigned(stream_grid(ctx, total, NLJ_THREADS, 4)), unsigned(n)), dim3(NLJ_THREADS), 0, ua);
            std::vector<unsigned long long> h(size_t(n), 0);
            NQE_HIP_CHECK(hipMemcpyAsync(h.data(), d->ptr, size_t(n) * 8, hipMemcpyDeviceToHost, ctx->stream));
            sync(ctx);
            sizes.insert(sizes.end(), h.begin(), h.end());
        };
        int n = 0;
        for (int side = 0; side < 2; ++side)
            for (const DevColumn &c : (side ? right : left)->cols) {
                if (c.dtype != NQE_UTF8) continue;
                ua.c[n++] = NljUtf8Len{static_cast<const int32_t *>(c.values->ptr), c.valid(), static_cast<const int64_t *>((side ? y_pos : x_pos)->ptr)};
                if (n == NLJ_MAX_UTF8) {
                    flush(n);
                    n = 0;
                }
            }
        flush(n);
        for (unsigned long long b : sizes)
            if (b > uint64_t(INT32_MAX))
                fail(NQE_ERR_NOT_SUPPORTED, "nested loop join: a Utf8 output column holds " + std::to_string(b) + " bytes, more than int32 offsets address");
    }

    auto t = std::make_unique<nqe_table>();
    t->ctx = ctx;
    t->rows = total;
    for (const DevColumn &c : left->cols) t->cols.push_back(take_column(ctx, c, static_cast<const int64_t *>(x_pos->ptr), total));
    x_pos.reset(); // (stream-ordered: the takes above still read it; the block goes back to the pool for the right side's columns)
    for (const DevColumn &c : right->cols) t->cols.push_back(take_column(ctx, c, static_cast<const int64_t *>(y_pos->ptr), total));
    *out = t.release();
    NQE_API_END()
}

// No NQE_MODULE_PROBE here: this unit's code object is loaded by the first nested loop join of a process (a few milliseconds, once), not
// by nqe_ctx_create.  Loading it up front moved the device allocations of every other query and cost the headline aggregate 1.3 % of
// its kernel time in alternating runs against the parent (profiles/nested_loop_join/README.md).
