// string_fn_kernels.hpp — the kernels of the string functions (quirk Q25: NQE_EXPR_STRING), gfx950, wave 64, grid-stride.  What they
// compute per byte and per string is string_fn_parts.hpp's; here is only how the work is spread over lanes.
//
//   str_case         a byte stream: 16 bytes per lane over the aligned body, bytes for the head and the tail
//   str_reverse      2^LG lanes per string; every lane strides over the string and stores byte i where REVERSE puts it (a word of
//                    single-byte units in one byte-swapped piece)
//   str_length       2^LG lanes per string; 8-byte words plus a byte tail, popcount of the non-continuation mask, reduced over the group
//   str_trim_bounds  2^LG lanes per string scan inwards from both ends; the kept length goes to the future offsets, the start to a column
//   str_trim_copy    2^LG lanes per string; 8-byte words plus a byte tail from src_off[i] + start[i]
//
// None of them reads validity: the bytes between a slot's two offsets are transformed whatever the slot's validity bit says.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_utils.hpp"
#include "string_fn_parts.hpp"

namespace nqe {
namespace {

// (str_u64_unaligned: device_utils.hpp)

// `head` bytes precede the first 16-byte boundary of src AND of dst (the host places dst at src's misalignment), head <= nbytes
template <bool UPPER>
__global__ void __launch_bounds__(256) str_case_kernel(const uint8_t *src, uint8_t *dst, int64_t nbytes, int64_t head) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t body = (nbytes - head) >> 4;
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(src + head);
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(dst + head);
    for (int64_t i = tid; i < body; i += stride) {
        ulonglong2 v = s[i];
        v.x = strfn::case_word(v.x, UPPER);
        v.y = strfn::case_word(v.y, UPPER);
        d[i] = v;
    }
    // fewer than 32 bytes in all: the head, then the tail behind the body
    const int64_t tail0 = head + (body << 4), edge = head + (nbytes - tail0);
    for (int64_t i = tid; i < edge; i += stride) {
        const int64_t b = i < head ? i : tail0 + (i - head);
        dst[b] = strfn::case_byte(src[b], UPPER);
    }
}

// 2^LG lanes per string, 64 >> LG strings per wave and step (the grouping of utf8_take_copy_kernel); the output has the input's offsets
template <int LG>
__global__ void __launch_bounds__(256) str_reverse_kernel(const int32_t *off, const uint8_t *src, uint8_t *dst, int64_t n) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        if (j >= n) continue;
        const int32_t so = off[j];
        const uint32_t len = uint32_t(off[j + 1] - so);
        const uint8_t *p = src + so;
        uint8_t *q = dst + so;
        // 8-byte words first: a word of single-byte units (ASCII, and no continuation byte behind it) is stored byte-swapped in one piece;
        // any other word, and the tail, byte by byte (at a byte a lane reads p[i-6 .. i+3] at most, and nothing outside the string)
        const uint32_t nw = len >> 3;
        for (uint32_t w = sub; w < nw; w += G) {
            const uint32_t i = 8 * w;
            const uint64_t v = *reinterpret_cast<const str_u64_unaligned *>(p + i);
            if (strfn::is_single_byte_units_word(v, i + 8 < len ? p[i + 8] : uint8_t(0)))
                *reinterpret_cast<str_u64_unaligned *>(q + (len - 8 - i)) = strfn::reverse_word(v);
            else
                for (uint32_t k = 0; k < 8; ++k) q[strfn::reverse_dest(p, len, i + k)] = p[i + k];
        }
        for (uint32_t b = (nw << 3) + sub; b < len; b += G) q[strfn::reverse_dest(p, len, b)] = p[b];
    }
}

template <int LG>
__global__ void __launch_bounds__(256) str_length_kernel(const int32_t *off, const uint8_t *src, int64_t n, int64_t *out) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) { // (j0 is the wave's: every lane takes part in the reduction)
        const int64_t j = j0 + grp;
        uint32_t count = 0;
        if (j < n) {
            const int32_t so = off[j];
            const uint32_t len = uint32_t(off[j + 1] - so), nw = len >> 3;
            const uint8_t *p = src + so;
            for (uint32_t w = sub; w < nw; w += G) count += strfn::noncontinuation_count(*reinterpret_cast<const str_u64_unaligned *>(p + 8 * w));
            for (uint32_t b = (nw << 3) + sub; b < len; b += G) count += strfn::is_continuation(p[b]) ? 0u : 1u;
        }
#pragma unroll
        for (int d = G >> 1; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
        if (j < n && sub == 0) out[j] = int64_t(count);
    }
}

// lens[j] = kept bytes of string j (the exclusive scan turns them into the output's offsets; lens[n] = 0 receives the total),
// starts[j] = the first kept byte, relative to the string's own start
template <int LG>
__global__ void __launch_bounds__(256) str_trim_bounds_kernel(const int32_t *off, const uint8_t *src, int64_t n, int mode, uint32_t *lens, uint32_t *starts) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    if (blockIdx.x == 0 && threadIdx.x == 0) lens[n] = 0;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        uint32_t len = 0, front = 0xFFFFFFFFu, back = 0;
        if (j < n) {
            const int32_t so = off[j];
            len = uint32_t(off[j + 1] - so);
            const uint8_t *p = src + so;
            if (mode & strfn::TRIM_FRONT) front = strfn::trim_front_scan(p, len, sub, G);
            if (mode & strfn::TRIM_BACK) back = strfn::trim_back_scan(p, len, sub, G);
        }
#pragma unroll
        for (int d = G >> 1; d > 0; d >>= 1) {
            const uint32_t of = __shfl_xor(front, d, 64), ob = __shfl_xor(back, d, 64);
            front = of < front ? of : front;
            back = ob > back ? ob : back;
        }
        if (j < n && sub == 0) {
            uint32_t first, end;
            strfn::trim_combine(mode, len, front, back, &first, &end);
            lens[j] = end - first;
            starts[j] = first;
        }
    }
}

template <int LG>
__global__ void __launch_bounds__(256) str_trim_copy_kernel(const int32_t *src_off, const uint8_t *src, const uint32_t *starts, const uint32_t *out_off, uint8_t *out, int64_t n) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t sub = uint32_t(lane_id()) & uint32_t(G - 1), grp = uint32_t(lane_id()) >> LG;
    for (int64_t j0 = wave * PER_WAVE; j0 < n; j0 += waves * PER_WAVE) {
        const int64_t j = j0 + grp;
        if (j >= n) continue;
        const uint8_t *p = src + src_off[j] + starts[j];
        const uint32_t d = out_off[j], len = out_off[j + 1] - d, nw = len >> 3;
        uint8_t *q = out + d;
        for (uint32_t w = sub; w < nw; w += G) *reinterpret_cast<str_u64_unaligned *>(q + 8 * w) = *reinterpret_cast<const str_u64_unaligned *>(p + 8 * w);
        for (uint32_t b = (nw << 3) + sub; b < len; b += G) q[b] = p[b];
    }
}

} // namespace
} // namespace nqe
