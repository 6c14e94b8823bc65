// conditional_kernels.hpp — the kernels of the conditional and NULL-handling functions (quirk Q28: NQE_EXPR_CONDITIONAL), gfx950, wave 64,
// grid-stride, 256-thread workgroups.  What they compute per row is conditional_parts.hpp's; here is only how the work is spread over lanes.
//
//   cond_words         COALESCE / NULLIF / IF over 8-byte words, four rows per lane (rows chunk + r * 64 + lane): one coalesced 8-byte load per
//                      column operand and row (a literal is a scalar), one 8-byte store, and — in the instances whose form can be NULL —
//                      the validity word of 64 rows by one ballot, stored by lane 0.  NULLIF's compare is in the same pass.
//   cond_bits          everything whose result and value operands are bitmaps: NOT, IS_NULL, IS_NOT_NULL, and COALESCE / NULLIF / IF over
//                      Boolean.  A lane per 64-row word, pure word logic, the last word masked to the row count.  The bitmaps are read as
//                      bytes (a borrowed bitmap ends at ceil(n / 8) and need not be 8-byte aligned).
//   cond_str_lengths   Utf8, a lane per row: the source the row's bytes come from (a byte per row), its length, the validity word by
//                      ballot, the 64-bit byte total by one atomic per wave (never on the value path)
//   cond_str_copy      2^LG lanes per result row copy its bytes in 8-byte words from the source chosen for it
//
// Every instance is picked by template parameters (the function, "has validity"); no by-value argument is indexed at run time.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "conditional_parts.hpp"
#include "device_utils.hpp"
#include "string_args_kernels.hpp" // str_bit_at, wave_add_to, str_u64_unaligned

namespace nqe {
namespace {

__device__ __forceinline__ bool cond_valid_at(const Operand &o, int64_t j) { return o.is_lit ? !o.lit_null : str_bit_at(o.valid, j); }

// out[row] = F(c, a, b) over 8-byte words; `c` is IF's Boolean condition (a bitmap or a literal), unused by the other functions.  The
// stack machine's access pattern (expr_kernels.hpp: expr_tree_kernel): a wave walks chunks of 64 x COND_ROWS rows, a lane owns the rows
// chunk + r * 64 + lane — every access a coalesced 512-byte wave access, every ballot one bitmap word — and the loads of a chunk are
// issued back to back before anything is consumed.  Words stream through once: nontemporal loads and stores.
constexpr int COND_ROWS = 4;
template <int F, bool HAS_VALID>
__global__ void __launch_bounds__(256) cond_words_kernel(Operand c, Operand a, Operand b, int f64, int64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ out_valid) {
    constexpr int R = COND_ROWS;
    const int lane = lane_id();
    const int64_t n_chunks = (n + 64 * R - 1) / (64 * R);
    const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const uint64_t *aw = static_cast<const uint64_t *>(a.values), *bw = static_cast<const uint64_t *>(b.values);
    const uint8_t *cbits = static_cast<const uint8_t *>(c.values);
    for (int64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
        const int64_t row0 = chunk * (64 * R) + lane;
        // every load of the chunk is issued before anything is consumed; rows are clamped to n - 1 so that no load is predicated
        int64_t rc[R];
        uint64_t x[R], y[R];
        uint32_t ab[R], bb[R], cb[R], cvb[R]; // the bytes that hold the rows' validity and condition bits (0xff: a literal, or no bitmap)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            rc[r] = row0 + r * 64 < n ? row0 + r * 64 : n - 1;
            x[r] = a.is_lit ? a.lit : __builtin_nontemporal_load(aw + rc[r]);
            y[r] = b.is_lit ? b.lit : __builtin_nontemporal_load(bw + rc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ab[r] = (a.is_lit || !a.valid) ? 0xffu : a.valid[rc[r] >> 3];
            bb[r] = (b.is_lit || !b.valid) ? 0xffu : b.valid[rc[r] >> 3];
            cb[r] = cvb[r] = 0xffu;
            if constexpr (F == cond::IF) {
                if (!c.is_lit) cb[r] = cbits[rc[r] >> 3];
                if (!c.is_lit && c.valid) cvb[r] = c.valid[rc[r] >> 3];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = row0 + r * 64;
            if (row - lane >= n) break; // wave-uniform: this 64-row word is past the end (every lane of the wave takes part in the ballot)
            const bool in = row < n;
            const int sh = int(rc[r]) & 7;
            const bool av = in && (a.is_lit ? !a.lit_null : ((ab[r] >> sh) & 1u) != 0), bv = in && (b.is_lit ? !b.lit_null : ((bb[r] >> sh) & 1u) != 0);
            bool c_true = false;
            if constexpr (F == cond::IF) c_true = in && (c.is_lit ? (!c.lit_null && c.lit != 0) : ((cb[r] & cvb[r]) >> sh) & 1u);
            const cond::Word w = cond::select_word<F>(f64 != 0, c_true, x[r], av, y[r], bv);
            if (in) __builtin_nontemporal_store(w.word, out + row);
            if constexpr (HAS_VALID) {
                const uint64_t v = __ballot(w.valid);
                if (lane == 0) out_valid[row >> 6] = v;
            }
        }
    }
}

// word w of an n-row bitmap read as bytes (null: all ones); bits beyond n are whatever the last byte holds — the caller masks the result
__device__ __forceinline__ uint64_t cond_bitmap_word(const uint8_t *bm, int64_t w, int64_t n) {
    if (!bm) return ~0ull;
    const int64_t bytes = (n + 7) >> 3, first = 8 * w;
    uint64_t word = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (first + k < bytes) word |= uint64_t(bm[first + k]) << (8 * k);
    return word;
}
__device__ __forceinline__ uint64_t cond_value_word(const Operand &o, int64_t w, int64_t n) {
    return o.is_lit ? (o.lit ? ~0ull : 0ull) : cond_bitmap_word(static_cast<const uint8_t *>(o.values), w, n);
}
__device__ __forceinline__ uint64_t cond_valid_word(const Operand &o, int64_t w, int64_t n) { return o.is_lit ? (o.lit_null ? 0ull : ~0ull) : cond_bitmap_word(o.valid, w, n); }

// 64 rows per lane.  IS_NULL / IS_NOT_NULL read a's validity alone (a.values may be of any dtype and is not touched).
template <int F, bool HAS_VALID>
__global__ void __launch_bounds__(256) cond_bits_kernel(Operand c, Operand a, Operand b, int64_t n, uint64_t *__restrict__ out, uint64_t *__restrict__ out_valid) {
    const int64_t words = (n + 63) >> 6;
    for (int64_t w = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < words; w += int64_t(gridDim.x) * blockDim.x) {
        uint64_t cb = 0, cv = 0, ab = 0, bb = 0, bv = 0;
        const uint64_t av = cond_valid_word(a, w, n);
        if constexpr (F == cond::IF) {
            cb = cond_value_word(c, w, n);
            cv = cond_valid_word(c, w, n);
        }
        if constexpr (F != cond::IS_NULL && F != cond::IS_NOT_NULL) ab = cond_value_word(a, w, n);
        if constexpr (F >= cond::COALESCE) {
            bb = cond_value_word(b, w, n);
            bv = cond_valid_word(b, w, n);
        }
        const cond::Bits r = cond::masked(cond::select_bits<F>(cb, cv, ab, av, bb, bv), cond::tail_mask(n, w));
        out[w] = r.value;
        if constexpr (HAS_VALID) out_valid[w] = r.valid;
    }
}

// a Utf8 operand: offsets, bytes, validity bytes (null: no NULLs)
struct CondStr {
    const int32_t *off;
    const uint8_t *data;
    const uint8_t *valid;
};

// Row j takes a where the condition holds, else b: the condition is bit j of c_bits AND bit j of c_valid (null pointers: ones).
// pick[j] = the source, lens[j] = its length (lens[n] = 0 for the scan), *total += the lengths, out_valid (or null) = the validity words.
__global__ void __launch_bounds__(256) cond_str_lengths_kernel(const uint8_t *c_bits, const uint8_t *c_valid, CondStr a, CondStr b, int64_t n, uint8_t *__restrict__ pick,
                                                               uint32_t *__restrict__ lens, uint64_t *__restrict__ out_valid, unsigned long long *total) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, n_pad = (n + 63) / 64 * 64, tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (tid == 0) lens[n] = 0;
    unsigned long long acc = 0;
    for (int64_t j = tid; j < n_pad; j += stride) {
        uint8_t from = cond::FROM_NONE;
        if (j < n) {
            from = cond::pick_source(str_bit_at(c_bits, j) && str_bit_at(c_valid, j), str_bit_at(a.valid, j), str_bit_at(b.valid, j));
            const int32_t *off = from == cond::FROM_B ? b.off : a.off;
            const uint32_t len = from == cond::FROM_NONE ? 0u : uint32_t(off[j + 1] - off[j]);
            pick[j] = from;
            lens[j] = len;
            acc += len;
        }
        if (out_valid) { // (uniform over the grid)
            const uint64_t v = __ballot(from != cond::FROM_NONE);
            if (lane_id() == 0) out_valid[j >> 6] = v;
        }
    }
    wave_add_to(acc, total);
}

template <int LG>
__global__ void __launch_bounds__(256) cond_str_copy_kernel(CondStr a, CondStr b, const uint8_t *__restrict__ pick, const uint32_t *__restrict__ out_off, uint8_t *__restrict__ out,
                                                            int64_t n) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        if (j >= n) continue;
        const uint32_t d = out_off[j], olen = out_off[j + 1] - d;
        if (olen == 0) continue; // a NULL row or an empty string
        const bool from_b = pick[j] == cond::FROM_B;
        const uint8_t *p = (from_b ? b.data : a.data) + (from_b ? b.off : a.off)[j];
        uint8_t *q = out + d;
        const uint32_t nw = olen >> 3;
        for (uint32_t w = sub; w < nw; w += G) *reinterpret_cast<str_u64_unaligned *>(q + 8u * w) = *reinterpret_cast<const str_u64_unaligned *>(p + 8u * w);
        for (uint32_t k = (nw << 3) + sub; k < olen; k += G) q[k] = p[k];
    }
}

} // namespace
} // namespace nqe
