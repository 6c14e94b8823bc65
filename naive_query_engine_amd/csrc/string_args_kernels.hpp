// string_args_kernels.hpp — the kernels of the string functions with arguments (quirk Q26: NQE_EXPR_STRING_ARGS), gfx950, wave 64,
// grid-stride.  What they compute per string is string_args_parts.hpp's; here is only how the work is spread over lanes.
//
//   str_substr_bounds    2^LG lanes per string walk it in chunks of G 8-byte words: popcount of each word's non-continuation mask, an
//                        ordered prefix over the group carried from chunk to chunk; the lane whose word holds the window's first or
//                        last character finds the byte; the group stops at the chunk that holds the window's end.  Kept lengths and
//                        starts go where str_trim_bounds puts them: str_trim_copy (string_fn_kernels.hpp) moves the bytes.
//   str_repeat_lengths   a lane per row: the saturating length, and the 64-bit total by one atomic per wave
//   str_repeat_copy      2^LG lanes per OUTPUT row stride over its 8-byte words, source index modulo the string's length
//   str_replace_same     |to| == |from|: G positions per chunk, a candidate test per lane, the group's ballot resolved greedily; every
//                        byte is written where it was read
//   str_replace_count    the same walk; lengths and the 64-bit total
//   str_replace_emit     the same walk again: the matches in front of every byte place it, and every match's lane writes `to`
//   str_args_validity    the AND of up to three validity bitmaps, a word per lane, and the number of valid rows
//
// Unlike Q25's kernels these read validity: a NULL row has length 0 (str_replace_same, which shares the operand's offsets, cannot and
// does not).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_utils.hpp"
#include "string_args_parts.hpp"
#include "string_fn_kernels.hpp"

namespace nqe {
namespace {

// an Int64 argument: a column (with its validity bytes, or null) or, when `values` is null, the literal
struct StrArgView {
    const int64_t *values;
    const uint8_t *valid;
    int64_t lit;
};
__device__ __forceinline__ int64_t str_arg_at(const StrArgView &a, int64_t j) { return a.values ? a.values[j] : a.lit; }
// (str_bit_at, wave_add_to: device_utils.hpp)

// the bits of a wave's ballot that belong to this lane's group of 2^LG lanes, bit b = lane b of the group
template <int LG> __device__ __forceinline__ uint64_t group_ballot(bool pred, uint32_t grp) {
    const uint64_t b = __ballot(pred);
    if constexpr (LG == 6) return b;
    else return (b >> (grp << LG)) & ((1ull << (1 << LG)) - 1ull);
}

template <int LG>
__global__ void __launch_bounds__(256) str_substr_bounds_kernel(const int32_t *off, const uint8_t *src, const uint8_t *s_valid, StrArgView start, StrArgView count, int64_t n,
                                                                uint32_t *lens, uint32_t *starts) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[n] = 0;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) { // (j0 is the wave's: every lane takes part in the shuffles)
        const int64_t j = j0 + grp;
        uint32_t len = 0;
        const uint8_t *p = src;
        uint64_t lo = 0, hi = 0;
        bool more = false; // the group's: the window's end lies behind the chunks read so far
        if (j < n && str_bit_at(s_valid, j) && str_bit_at(start.valid, j) && str_bit_at(count.valid, j)) {
            const int32_t so = off[j];
            len = uint32_t(off[j + 1] - so);
            p = src + so;
            more = strargs::substr_window(str_arg_at(start, j), str_arg_at(count, j), &lo, &hi) && len > 0;
        }
        const bool live = more;
        uint32_t pos_lo = 0xFFFFFFFFu, pos_hi = 0xFFFFFFFFu; // where characters lo and hi begin, in the lane that finds them
        uint64_t before = 0;                                  // non-continuation bytes in front of the chunk (the group's)
        for (uint32_t c0 = 0; __any(more); c0 += 8u * G) {
            const uint32_t b0 = c0 + 8u * sub;
            uint64_t mask = 0;
            if (more && b0 < len) {
                const uint32_t left = len - b0;
                const uint64_t w = left >= 8 ? *reinterpret_cast<const str_u64_unaligned *>(p + b0) : strargs::tail_word(p + b0, left);
                mask = strfn::noncontinuation_mask(w);
            }
            const uint32_t own = uint32_t(__builtin_popcountll(mask));
            uint32_t incl = own;
#pragma unroll
            for (int d = 1; d < G; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, G);
                if (sub >= uint32_t(d)) incl += up;
            }
            const uint32_t chunk_total = __shfl(incl, G - 1, G);
            if (more) {
                const uint64_t mine = before + (incl - own);
                uint32_t k = strargs::kth_in_word(mask, mine, lo);
                if (k < 8) pos_lo = b0 + k;
                k = strargs::kth_in_word(mask, mine, hi);
                if (k < 8) pos_hi = b0 + k;
                before += chunk_total;
                more = before < hi && uint64_t(c0) + 8u * G < len;
            }
        }
#pragma unroll
        for (int d = G >> 1; d > 0; d >>= 1) {
            const uint32_t ol = __shfl_xor(pos_lo, d, 64), oh = __shfl_xor(pos_hi, d, 64);
            pos_lo = ol < pos_lo ? ol : pos_lo;
            pos_hi = oh < pos_hi ? oh : pos_hi;
        }
        if (j < n && sub == 0) {
            uint32_t first = 0, end = 0;
            if (live) strargs::substr_combine(lo, pos_lo < len ? pos_lo : len, pos_hi < len ? pos_hi : len, &first, &end);
            lens[j] = end - first;
            starts[j] = first;
        }
    }
}

// lens[j] = the row's length clamped to 32 bits (the scan reads it only when the total fits), *total += the 64-bit lengths
__global__ void __launch_bounds__(256) str_repeat_lengths_kernel(const int32_t *off, const uint8_t *s_valid, StrArgView times, int64_t n, uint32_t *lens, unsigned long long *total) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    if (tid == 0) lens[n] = 0;
    unsigned long long acc = 0;
    for (int64_t j = tid; j < n; j += stride) {
        uint64_t r = 0;
        if (str_bit_at(s_valid, j) && str_bit_at(times.valid, j)) r = strargs::repeat_length(uint32_t(off[j + 1] - off[j]), str_arg_at(times, j));
        lens[j] = r < 0xFFFFFFFFull ? uint32_t(r) : 0xFFFFFFFFu;
        acc += r;
    }
    wave_add_to(acc, total);
}

template <int LG>
__global__ void __launch_bounds__(256) str_repeat_copy_kernel(const int32_t *src_off, const uint8_t *src, const uint32_t *out_off, uint8_t *out, int64_t n) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        if (j >= n) continue;
        const uint32_t d = out_off[j], olen = out_off[j + 1] - d;
        if (olen == 0) continue; // a NULL row, an empty string or no copies
        const int32_t so = src_off[j];
        const uint32_t slen = uint32_t(src_off[j + 1] - so), nw = olen >> 3;
        const uint8_t *p = src + so;
        uint8_t *q = out + d;
        for (uint32_t w = sub; w < nw; w += G) {
            uint32_t r = (8u * w) % slen;
            uint64_t v = 0;
            if (r + 8 <= slen)
                v = *reinterpret_cast<const str_u64_unaligned *>(p + r);
            else
                for (uint32_t k = 0; k < 8; ++k) {
                    v |= uint64_t(p[r]) << (8 * k);
                    if (++r == slen) r = 0;
                }
            *reinterpret_cast<str_u64_unaligned *>(q + 8u * w) = v;
        }
        for (uint32_t b = (nw << 3) + sub; b < olen; b += G) q[b] = p[b % slen];
    }
}

// |to| == |from| = m: the result has the operand's offsets, so validity is not read and no length is written
template <int LG>
__global__ void __launch_bounds__(256) str_replace_same_kernel(const int32_t *off, const uint8_t *src, const uint8_t *from, const uint8_t *to, uint32_t m, int bordered,
                                                               uint8_t *dst, int64_t n) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) { // (j0 is the wave's: every lane takes part in the ballots)
        const int64_t j = j0 + grp;
        uint32_t len = 0;
        const uint8_t *p = src;
        uint8_t *q = dst;
        if (j < n) {
            const int32_t so = off[j];
            len = uint32_t(off[j + 1] - so);
            p = src + so;
            q = dst + so;
        }
        uint32_t next_free = 0;
        for (uint32_t c0 = 0; __any(c0 < len); c0 += G) {
            const uint32_t i = c0 + sub;
            const uint64_t cand = group_ballot<LG>(c0 < len && strargs::is_candidate(p, len, i, from, m), grp);
            const uint32_t nf_before = next_free;
            const uint64_t taken = strargs::resolve_matches(cand, c0, m, bordered != 0, &next_free);
            if (i < len) {
                const strargs::Placement pl = strargs::place_byte(taken, c0, sub, 0, nf_before, m, m);
                q[i] = pl.is_start ? to[0] : pl.covered ? to[pl.within] : p[i];
            }
        }
    }
}

template <int LG>
__global__ void __launch_bounds__(256) str_replace_count_kernel(const int32_t *off, const uint8_t *src, const uint8_t *s_valid, const uint8_t *from, uint32_t m, uint32_t t,
                                                                int bordered, int64_t n, uint32_t *lens, unsigned long long *total) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[n] = 0;
    unsigned long long acc = 0;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        uint32_t len = 0;
        const uint8_t *p = src;
        if (j < n && str_bit_at(s_valid, j)) {
            const int32_t so = off[j];
            len = uint32_t(off[j + 1] - so);
            p = src + so;
        }
        uint32_t next_free = 0;
        uint64_t matches = 0;
        for (uint32_t c0 = 0; __any(c0 < len); c0 += G) {
            const uint64_t cand = group_ballot<LG>(c0 < len && strargs::is_candidate(p, len, c0 + sub, from, m), grp);
            matches += uint64_t(__builtin_popcountll(strargs::resolve_matches(cand, c0, m, bordered != 0, &next_free)));
        }
        if (j < n && sub == 0) {
            const uint64_t r = strargs::replaced_length(len, matches, m, t);
            lens[j] = r < 0xFFFFFFFFull ? uint32_t(r) : 0xFFFFFFFFu;
            acc += r;
        }
    }
    wave_add_to(acc, total);
}

template <int LG>
__global__ void __launch_bounds__(256) str_replace_emit_kernel(const int32_t *off, const uint8_t *src, const uint8_t *s_valid, const uint8_t *from, const uint8_t *to, uint32_t m,
                                                               uint32_t t, int bordered, const uint32_t *out_off, uint8_t *out, int64_t n) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        uint32_t len = 0;
        const uint8_t *p = src;
        uint8_t *q = out;
        if (j < n && str_bit_at(s_valid, j)) {
            const int32_t so = off[j];
            len = uint32_t(off[j + 1] - so);
            p = src + so;
            q = out + out_off[j];
        }
        uint32_t next_free = 0;
        uint64_t matches = 0;
        for (uint32_t c0 = 0; __any(c0 < len); c0 += G) {
            const uint32_t i = c0 + sub;
            const uint64_t cand = group_ballot<LG>(c0 < len && strargs::is_candidate(p, len, i, from, m), grp);
            const uint32_t nf_before = next_free;
            const uint64_t taken = strargs::resolve_matches(cand, c0, m, bordered != 0, &next_free);
            if (i < len) {
                const strargs::Placement pl = strargs::place_byte(taken, c0, sub, matches, nf_before, m, t);
                if (pl.is_start)
                    for (uint32_t k = 0; k < t; ++k) q[pl.out + k] = to[k];
                else if (!pl.covered)
                    q[pl.out] = p[i];
            }
            matches += uint64_t(__builtin_popcountll(taken));
        }
    }
}

// out = v0 & v1 & v2 over the first n bits (a null pointer: all ones), the bits behind n zero; *valid_rows += the set bits
__global__ void __launch_bounds__(256) str_args_validity_kernel(const uint8_t *v0, const uint8_t *v1, const uint8_t *v2, int64_t n, uint64_t *out, unsigned long long *valid_rows) {
    const int64_t words = (n + 63) >> 6;
    unsigned long long acc = 0;
    for (int64_t w = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < words; w += int64_t(gridDim.x) * blockDim.x) {
        uint64_t word = 0;
        for (int k = 0; k < 8; ++k) {
            const int64_t byte = 8 * w + k, bit0 = 8 * byte;
            if (bit0 >= n) break;
            uint32_t b = 0xFFu;
            if (v0) b &= v0[byte];
            if (v1) b &= v1[byte];
            if (v2) b &= v2[byte];
            if (n - bit0 < 8) b &= (1u << (n - bit0)) - 1u;
            word |= uint64_t(b) << (8 * k);
        }
        out[w] = word;
        acc += (unsigned long long)__builtin_popcountll(word);
    }
    wave_add_to(acc, valid_rows);
}

} // namespace
} // namespace nqe
