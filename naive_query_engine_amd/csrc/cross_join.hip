// cross_join.hip — CrossJoin::execute for one batch pair (reference: src/physical_plan/cross_join.rs:55-185), quirk Q15.
//
// The reference fills a left column with `for _ in 0..R { for k in 0..L }` and a right column with `for _ in 0..L { for k in 0..R }`,
// so output row j takes left[j % L] and right[j % R]: every output column is a periodic tile of one input column (a Cartesian
// product only when gcd(L, R) = 1).  Nothing is hashed, scanned or indexed; the kernels below write the N = L·R output rows from the
// closed form, and the roofline is the card's store rate.
//
//   cross_join_words        every 8-byte column of both sides in ONE launch (blockIdx.y = column), two rows per lane per 16-byte store
//   cross_join_utf8_offsets every Utf8 column's int32 offsets in one launch: out_off[j] = (j / P)·B + off[j % P] − off[0]
//   cross_join_utf8_bytes   every Utf8 column's payload in one launch: the byte range [off[0], off[P]) tiled N / P times
//
// No per-row 64-bit division: a workgroup takes a contiguous chunk of rows and divides its first row by the period once; a lane then
// walks (quotient, remainder) forward with adds and one conditional subtract (steps prepared on the host).  Validity is dropped (the
// reference builds its outputs from a Vec): word outputs are the raw slots, Utf8 outputs the bytes between a slot's offsets.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "device_utils.hpp"
#include "nqe_internal.hpp"

namespace nqe {

namespace {

constexpr int CJ_THREADS = 256;
constexpr int CJ_ITERS = 8;                                          // 16-byte stores per lane and chunk
constexpr int64_t CJ_WORD_STEP = 2 * CJ_THREADS;                     // rows a workgroup writes per iteration (two per lane)
constexpr int64_t CJ_WORD_CHUNK = CJ_WORD_STEP * CJ_ITERS;           // 4096 rows
constexpr int64_t CJ_OFF_STEP = 4 * CJ_THREADS;                      // int32 offsets: four per lane
constexpr int64_t CJ_OFF_CHUNK = CJ_OFF_STEP * CJ_ITERS;
constexpr int64_t CJ_BYTE_STEP = 16 * CJ_THREADS;                    // payload bytes: sixteen per lane
constexpr int64_t CJ_BYTE_CHUNK = CJ_BYTE_STEP * CJ_ITERS;
constexpr int CJ_MAX_WORD_COLS = 64;                                 // descriptors per launch (kernel arguments: 2 KiB)
constexpr int CJ_MAX_UTF8_COLS = 32;
constexpr int64_t CJ_MAX_GRID_X = 1 << 16;                           // chunks beyond it are grid-strided

typedef uint64_t cj_u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t cj_u32x4 __attribute__((ext_vector_type(4)));

struct CjWordCol {
    const uint64_t *src;
    uint64_t *dst;
    int64_t period; // L for a left column, R for a right one
    int64_t step;   // CJ_WORD_STEP % period
};
struct CjWordArgs {
    CjWordCol c[CJ_MAX_WORD_COLS];
    int64_t n;
};

struct CjUtf8Col {
    const int32_t *off; // input offsets [period + 1]
    const uint8_t *src; // input bytes (offsets index them directly)
    int32_t *dst_off;   // [n + 1]
    uint8_t *dst;       // [bytes rounded up to 16]
    int64_t period;
    int64_t off_step, off_qstep;   // CJ_OFF_STEP % / / period
    int64_t tile;                  // B = off[P] − off[0]
    int64_t bytes;                 // B · (n / P)
    int64_t byte_step;             // CJ_BYTE_STEP % B
    int32_t off0, pad;
};
struct CjUtf8Args {
    CjUtf8Col c[CJ_MAX_UTF8_COLS];
    int64_t n;
};

// first position of a lane: (base + d) mod p, with base < p and d < span; one conditional subtract when p >= span, else a 32-bit
// remainder of d (p < span fits 32 bits)
__device__ __forceinline__ void cj_first(int64_t base, uint32_t d, int64_t p, int64_t span, int64_t *r, int64_t *q) {
    int64_t rr, qq;
    if (p >= span) {
        rr = base + d;
        qq = 0;
    } else {
        const uint32_t p32 = uint32_t(p);
        qq = d / p32;
        rr = base + (d - uint32_t(qq) * p32);
    }
    if (rr >= p) {
        rr -= p;
        ++qq;
    }
    *r = rr;
    *q = qq;
}

template <bool NT> __device__ __forceinline__ void cj_store2(uint64_t *p, uint64_t a, uint64_t b) {
    cj_u64x2 v = {a, b};
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<cj_u64x2 *>(p));
    else *reinterpret_cast<cj_u64x2 *>(p) = v;
}
template <bool NT> __device__ __forceinline__ void cj_store4(uint32_t *p, cj_u32x4 v) {
    if (NT) __builtin_nontemporal_store(v, reinterpret_cast<cj_u32x4 *>(p));
    else *reinterpret_cast<cj_u32x4 *>(p) = v;
}

// out[j] = src[j % period] for every 8-byte column of the batch pair
template <bool NT> __global__ void __launch_bounds__(CJ_THREADS) cross_join_words_kernel(CjWordArgs a) {
    const CjWordCol c = a.c[blockIdx.y];
    const int64_t n = a.n, p = c.period;
    const int64_t nchunks = (n + CJ_WORD_CHUNK - 1) / CJ_WORD_CHUNK;
    const uint32_t d = 2u * threadIdx.x;
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int64_t start = ch * CJ_WORD_CHUNK;
        int64_t r, q;
        cj_first(start % p, d, p, CJ_WORD_STEP, &r, &q);
        int64_t j = start + d;
#pragma unroll
        for (int it = 0; it < CJ_ITERS; ++it, j += CJ_WORD_STEP) {
            const int64_t r1 = r + 1 == p ? 0 : r + 1;
            const uint64_t v0 = c.src[r], v1 = c.src[r1];
            if (j + 1 < n) cj_store2<NT>(c.dst + j, v0, v1);
            else if (j < n) c.dst[j] = v0; // the scalar tail (odd n)
            r += c.step;
            if (r >= p) r -= p;
        }
    }
}

// out_off[j] = (j / P)·B + off[j % P] − off[0] for j in [0, n] (j = n: r = 0, q = n / P, the total), four per lane
template <bool NT> __global__ void __launch_bounds__(CJ_THREADS) cross_join_utf8_offsets_kernel(CjUtf8Args a) {
    const CjUtf8Col c = a.c[blockIdx.y];
    const int64_t m = a.n + 1, p = c.period;
    const int64_t nchunks = (m + CJ_OFF_CHUNK - 1) / CJ_OFF_CHUNK;
    const uint32_t d = 4u * threadIdx.x;
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int64_t start = ch * CJ_OFF_CHUNK;
        const int64_t q0 = start / p;
        int64_t r, q;
        cj_first(start - q0 * p, d, p, CJ_OFF_STEP, &r, &q);
        q += q0;
        int64_t j = start + d;
#pragma unroll
        for (int it = 0; it < CJ_ITERS; ++it, j += CJ_OFF_STEP) {
            if (j < m) {
                int32_t v[4];
                int64_t rr = r, qq = q;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = int32_t(qq * c.tile + int64_t(c.off[rr] - c.off0));
                    if (++rr == p) {
                        rr = 0;
                        ++qq;
                    }
                }
                if (j + 3 < m) cj_store4<NT>(reinterpret_cast<uint32_t *>(c.dst_off + j), cj_u32x4{uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3])});
                else
                    for (int k = 0; k < 4 && j + k < m; ++k) c.dst_off[j + k] = v[k]; // the scalar tail
            }
            r += c.off_step;
            q += c.off_qstep;
            if (r >= p) {
                r -= p;
                ++q;
            }
        }
    }
}

__device__ __forceinline__ uint64_t cj_load_u64_unaligned(const uint8_t *p) {
    typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
    return *reinterpret_cast<const u64_unaligned *>(p);
}

// dst[k] = src[off0 + k % B] for k < bytes, sixteen bytes per lane (the buffer is padded to whole 16-byte units)
template <bool NT> __global__ void __launch_bounds__(CJ_THREADS) cross_join_utf8_bytes_kernel(CjUtf8Args a) {
    const CjUtf8Col c = a.c[blockIdx.y];
    const int64_t total = c.bytes, b = c.tile;
    if (total == 0) return;
    const uint8_t *src = c.src + c.off0;
    const int64_t nchunks = (total + CJ_BYTE_CHUNK - 1) / CJ_BYTE_CHUNK;
    const uint32_t d = 16u * threadIdx.x;
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int64_t start = ch * CJ_BYTE_CHUNK;
        int64_t s, unused;
        cj_first(start % b, d, b, CJ_BYTE_STEP, &s, &unused);
        int64_t k = start + d;
#pragma unroll 2
        for (int it = 0; it < CJ_ITERS; ++it, k += CJ_BYTE_STEP) {
            if (k < total) {
                uint64_t w0, w1;
                if (s + 16 <= b) { // no wrap inside these sixteen bytes
                    w0 = cj_load_u64_unaligned(src + s);
                    w1 = cj_load_u64_unaligned(src + s + 8);
                } else {
                    w0 = w1 = 0;
                    int64_t ss = s;
                    for (int i = 0; i < 16; ++i) {
                        const uint64_t byte = src[ss];
                        if (i < 8) w0 |= byte << (8 * i);
                        else w1 |= byte << (8 * (i - 8));
                        if (++ss == b) ss = 0;
                    }
                }
                cj_store2<NT>(reinterpret_cast<uint64_t *>(c.dst + k), w0, w1);
            }
            s += c.byte_step;
            if (s >= b) s -= b;
        }
    }
}

inline int64_t grid_x(int64_t chunks) { return std::max<int64_t>(1, std::min<int64_t>(chunks, CJ_MAX_GRID_X)); }

// NQE_CROSS_JOIN_STORES=plain|nt (read per call): the store flavour of the three kernels, for A/B runs (tools/probe_cross_join.py)
bool nontemporal_stores() {
    const char *e = getenv("NQE_CROSS_JOIN_STORES");
    if (e && !strcmp(e, "nt")) return true;
    if (e && !strcmp(e, "plain")) return false;
    return false; // the default: plain stores (CrossJoin)
}

void fail_too_large(const char *what) { fail(NQE_ERR_OUT_OF_MEMORY, std::string("cross join: ") + what + " overflows int64"); }

} // namespace

} // namespace nqe

using namespace nqe;

nqe_status nqe_cross_join_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !left || !right || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    // per column type, whatever the row counts: the reference's `_ => unimplemented!()` (cross_join.rs:118, :172)
    for (const nqe_table *t : {left, right})
        for (const DevColumn &c : t->cols)
            if (!(is_word_type(c.dtype) || c.dtype == NQE_UTF8))
                fail(NQE_ERR_NOT_SUPPORTED, "cross join: Boolean columns are not implemented (cross_join.rs panics: unimplemented!())");
    const int64_t L = left->rows, R = right->rows;
    int64_t n = 0;
    if (__builtin_mul_overflow(L, R, &n)) fail_too_large("the row count L * R");
    int64_t word_bytes = 0;
    if (__builtin_mul_overflow(n, int64_t(8), &word_bytes)) fail_too_large("a column's byte size");

    // every output column: its source, its period (L or R) and whether it tiles more than once
    struct Src {
        const DevColumn *c;
        int64_t period;
        bool tiled;
    };
    std::vector<Src> srcs;
    for (const DevColumn &c : left->cols) srcs.push_back({&c, L, R != 1});
    for (const DevColumn &c : right->cols) srcs.push_back({&c, R, L != 1});

    // Utf8: the first and last offset of every column, read back together (one synchronisation for the call)
    std::vector<int32_t> ends;
    for (const Src &s : srcs)
        if (s.c->dtype == NQE_UTF8) ends.insert(ends.end(), {0, 0});
    if (n > 0 && !ends.empty()) {
        size_t k = 0;
        for (const Src &s : srcs) {
            if (s.c->dtype != NQE_UTF8) continue;
            const int32_t *off = static_cast<const int32_t *>(s.c->values->ptr);
            NQE_HIP_CHECK(hipMemcpyAsync(&ends[k], off, 4, hipMemcpyDeviceToHost, ctx->stream));
            NQE_HIP_CHECK(hipMemcpyAsync(&ends[k + 1], off + s.period, 4, hipMemcpyDeviceToHost, ctx->stream));
            k += 2;
        }
        sync(ctx);
    }
    // sizes, overflow-checked, before anything is allocated or launched
    int64_t total = 0;
    std::vector<int64_t> utf8_bytes;
    for (size_t i = 0, k = 0; i < srcs.size(); ++i) {
        int64_t col_bytes = word_bytes;
        if (srcs[i].c->dtype == NQE_UTF8) {
            const int64_t b = n > 0 ? int64_t(ends[k + 1]) - int64_t(ends[k]) : 0;
            if (b < 0) fail(NQE_ERR_ARROW, "cross join: Utf8 offsets decrease");
            k += 2;
            int64_t bytes = 0;
            if (n > 0 && __builtin_mul_overflow(b, n / srcs[i].period, &bytes)) bytes = INT64_MAX;
            // the output's int32 offsets cannot address more (the reference panics building its StringArray)
            if (bytes > int64_t(INT32_MAX))
                fail(NQE_ERR_NOT_SUPPORTED, "cross join: a Utf8 output column holds " + std::to_string(bytes) + " bytes, more than int32 offsets address");
            utf8_bytes.push_back(bytes);
            if (__builtin_mul_overflow(n + 1, int64_t(4), &col_bytes) || __builtin_add_overflow(col_bytes, bytes, &col_bytes))
                fail_too_large("a column's byte size");
        }
        if (__builtin_add_overflow(total, col_bytes, &total)) fail_too_large("the output's byte size");
    }
    size_t free_b = 0, total_b = 0;
    NQE_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (uint64_t(total) > uint64_t(total_b))
        fail(NQE_ERR_OUT_OF_MEMORY, "cross join: the output needs " + std::to_string(total) + " bytes, the device has " + std::to_string(total_b));

    const bool nt = nontemporal_stores();
    auto t = std::make_unique<nqe_table>();
    t->ctx = ctx;
    t->rows = n;
    CjWordArgs wa;
    std::memset(&wa, 0, sizeof(wa));
    wa.n = n;
    int nw = 0;
    auto flush_words = [&]() {
        if (nw == 0) return;
        const dim3 grid(unsigned(grid_x((n + CJ_WORD_CHUNK - 1) / CJ_WORD_CHUNK)), unsigned(nw));
        launch(ctx, "cross_join_words", nt ? cross_join_words_kernel<true> : cross_join_words_kernel<false>, grid, dim3(CJ_THREADS), 0, wa);
        nw = 0;
    };
    CjUtf8Args ua;
    std::memset(&ua, 0, sizeof(ua));
    ua.n = n;
    int nu = 0;
    int64_t max_bytes = 0;
    auto flush_utf8 = [&]() {
        if (nu == 0) return;
        const dim3 g_off(unsigned(grid_x((n + 1 + CJ_OFF_CHUNK - 1) / CJ_OFF_CHUNK)), unsigned(nu));
        launch(ctx, "cross_join_utf8_offsets", nt ? cross_join_utf8_offsets_kernel<true> : cross_join_utf8_offsets_kernel<false>, g_off, dim3(CJ_THREADS), 0, ua);
        if (max_bytes > 0) {
            const dim3 g_b(unsigned(grid_x((max_bytes + CJ_BYTE_CHUNK - 1) / CJ_BYTE_CHUNK)), unsigned(nu));
            launch(ctx, "cross_join_utf8_bytes", nt ? cross_join_utf8_bytes_kernel<true> : cross_join_utf8_bytes_kernel<false>, g_b, dim3(CJ_THREADS), 0, ua);
        }
        nu = 0;
        max_bytes = 0;
    };
    size_t ui = 0, ek = 0;
    for (const Src &s : srcs) {
        const DevColumn &c = *s.c;
        DevColumn o;
        o.dtype = c.dtype;
        o.length = n;
        o.null_count = 0; // built from a Vec: no validity bitmap (cross_join.rs:81, :160)
        if (is_word_type(c.dtype)) {
            if (!s.tiled && buf_shareable(c.values)) {
                o.values = c.values; // one tile: the input's own slots, without its validity
            } else {
                o.values = dev_alloc(ctx, size_t(word_bytes));
                if (n > 0) {
                    wa.c[nw++] = CjWordCol{c.words(), static_cast<uint64_t *>(o.values->ptr), s.period, CJ_WORD_STEP % s.period};
                    if (nw == CJ_MAX_WORD_COLS) flush_words();
                }
            }
        } else { // Utf8
            const int64_t bytes = utf8_bytes[ui++];
            o.values = dev_alloc(ctx, size_t(n + 1) * 4);
            o.data = dev_alloc(ctx, size_t((bytes + 15) / 16 * 16));
            o.data_length = bytes;
            if (n == 0) {
                NQE_HIP_CHECK(hipMemsetAsync(o.values->ptr, 0, 4, ctx->stream));
            } else {
                CjUtf8Col &u = ua.c[nu++];
                u.off = static_cast<const int32_t *>(c.values->ptr);
                u.src = c.data ? static_cast<const uint8_t *>(c.data->ptr) : nullptr;
                u.dst_off = static_cast<int32_t *>(o.values->ptr);
                u.dst = static_cast<uint8_t *>(o.data->ptr);
                u.period = s.period;
                u.off_step = CJ_OFF_STEP % s.period;
                u.off_qstep = CJ_OFF_STEP / s.period;
                u.off0 = ends[ek];
                u.tile = int64_t(ends[ek + 1]) - int64_t(ends[ek]);
                u.bytes = bytes;
                u.byte_step = u.tile > 0 ? CJ_BYTE_STEP % u.tile : 0;
                max_bytes = std::max(max_bytes, bytes);
                if (nu == CJ_MAX_UTF8_COLS) flush_utf8();
            }
            ek += 2;
        }
        t->cols.push_back(std::move(o));
    }
    flush_words();
    flush_utf8();
    *out = t.release();
    NQE_API_END()
}

NQE_MODULE_PROBE(nqe::cross_join_words_kernel<false>);
