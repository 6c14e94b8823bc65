// cast_kernels.hpp — the kernels of a cast (quirk Q29: NQE_EXPR_CAST), gfx950, wave 64, grid-stride, 256-thread workgroups.  What a row
// becomes is cast_parts.hpp's; here is only how the work is spread over lanes.  The operand is always a column (the host expands literals).
//
//   cast_fixed         between the 8-byte word types and Boolean, one streaming launch.  A wave walks chunks of 64 x CAST_ROWS rows, a lane
//                      owns the rows chunk + r * 64 + lane (cond_words' and the stack machine's pattern): a word operand is one coalesced
//                      8-byte load per row, a Boolean operand the byte that holds the row's bit; a word result is one 8-byte store, a
//                      Boolean result the ballot of 64 rows stored by lane 0, and so is the validity word — (operand valid) AND (conversion
//                      representable) — where the result carries a buffer of its own.  Nothing is read back.  The Boolean casts take this
//                      form and not a lane per 64-row bitmap word: that lane would read or write 64 consecutive 8-byte words, a 512-byte
//                      stride between neighbouring lanes, on the side that carries 64 times the bytes.
//   cast_parse         Utf8 to a word type or Boolean, a lane per row: the parser runs over the bytes between the slot's two offsets; the
//                      validity word by ballot (always: every parse can fail).
//   cast_text_lengths  Int64 / UInt64 / Boolean to Utf8, a lane per row: the text's length (0 under a NULL) and the 64-bit byte total by
//                      one atomic per wave.
//   cast_text_write    a lane per row forms the text in three registers and stores it in 8-byte words where whole ones fit.
//
// Every instance is picked by template parameters (the two types); no by-value argument is indexed at run time.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cast_parts.hpp"
#include "device_utils.hpp" // str_bit_at, wave_add_to, str_u64_unaligned

namespace nqe {
namespace {

constexpr int CAST_ROWS = 4;    // rows per lane and chunk of cast_fixed: a workgroup's four waves cover CAST_BLOCK_ROWS rows per trip
constexpr int CAST_BLOCK_ROWS = 256 * CAST_ROWS;
constexpr int CAST_LANE_ROWS = 256; // rows a workgroup of the lane-per-row kernels covers per trip

// `values`: words, or the packed bits of a Boolean operand; `out`: words, or the bitmap words of a Boolean result; `out_valid`: null when
// the result carries the operand's validity buffer (or none).  n >= 1.
template <int FROM, int TO>
__global__ void __launch_bounds__(256) cast_fixed_kernel(const void *__restrict__ values, const uint8_t *__restrict__ valid, int64_t n, uint64_t *__restrict__ out,
                                                         uint64_t *__restrict__ out_valid) {
    constexpr int R = CAST_ROWS;
    const int lane = lane_id();
    const int64_t n_chunks = (n + 64 * R - 1) / (64 * R);
    const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const uint64_t *words = static_cast<const uint64_t *>(values);
    const uint8_t *bits = static_cast<const uint8_t *>(values);
    for (int64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
        const int64_t row0 = chunk * (64 * R) + lane;
        // every load of the chunk is issued before anything is consumed; rows are clamped to n - 1 so that no load is predicated
        int64_t rc[R];
        uint64_t x[R];
        uint32_t vb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            rc[r] = row0 + r * 64 < n ? row0 + r * 64 : n - 1;
            if constexpr (FROM == cast::BOOLEAN) x[r] = bits[rc[r] >> 3];
            else x[r] = __builtin_nontemporal_load(words + rc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) vb[r] = valid ? valid[rc[r] >> 3] : 0xffu;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = row0 + r * 64;
            if (row - lane >= n) break; // wave-uniform: this 64-row word is past the end (every lane of the wave takes part in the ballots)
            const bool in = row < n;
            const int sh = int(rc[r]) & 7;
            const cast::Word c = cast::convert<FROM, TO>(FROM == cast::BOOLEAN ? (x[r] >> sh) & 1ull : x[r]);
            const cast::Word w = cast::made(c.word, in && ((vb[r] >> sh) & 1u) != 0 && c.valid);
            if constexpr (TO == cast::BOOLEAN) {
                const uint64_t b = __ballot(w.word != 0);
                if (lane == 0) out[row >> 6] = b;
            } else {
                if (in) __builtin_nontemporal_store(w.word, out + row);
            }
            if (out_valid) { // (uniform over the grid)
                const uint64_t v = __ballot(w.valid);
                if (lane == 0) out_valid[row >> 6] = v;
            }
        }
    }
}

// out (words, or bitmap words for Boolean) and out_valid from the parse of every slot; a NULL slot is not read
template <int TO>
__global__ void __launch_bounds__(256) cast_parse_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ data, const uint8_t *__restrict__ valid, int64_t n,
                                                         uint64_t *__restrict__ out, uint64_t *__restrict__ out_valid) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, n_pad = (n + 63) / 64 * 64;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n_pad; j += stride) {
        cast::Word w{0, false};
        if (j < n && str_bit_at(valid, j)) {
            const int32_t o = off[j];
            w = cast::parse<TO>(reinterpret_cast<const char *>(data) + o, int(off[j + 1] - o));
        }
        if constexpr (TO == cast::BOOLEAN) {
            const uint64_t b = __ballot(w.word != 0);
            if (lane_id() == 0) out[j >> 6] = b;
        } else {
            if (j < n) out[j] = w.word;
        }
        const uint64_t v = __ballot(w.valid);
        if (lane_id() == 0) out_valid[j >> 6] = v;
    }
}

__device__ __forceinline__ uint64_t cast_value_at(const void *values, bool boolean, int64_t j) {
    return boolean ? uint64_t(get_bit(static_cast<const uint8_t *>(values), j)) : static_cast<const uint64_t *>(values)[j];
}

// lens[j] = the bytes of row j's text (0 under a NULL), lens[n] = 0 for the scan, *total += the lengths
template <int FROM>
__global__ void __launch_bounds__(256) cast_text_lengths_kernel(const void *__restrict__ values, const uint8_t *__restrict__ valid, int64_t n, uint32_t *__restrict__ lens,
                                                                unsigned long long *total) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (tid == 0) lens[n] = 0;
    unsigned long long acc = 0;
    for (int64_t j = tid; j < n; j += stride) {
        const uint32_t len = str_bit_at(valid, j) ? uint32_t(cast::text_length<FROM>(cast_value_at(values, FROM == cast::BOOLEAN, j))) : 0u;
        lens[j] = len;
        acc += len;
    }
    wave_add_to(acc, total); // (every lane of the wave arrives here: the loop holds no wave operation)
}

// row j's text at out + out_off[j]; a row of no bytes is a NULL row (every text has at least one byte)
template <int FROM>
__global__ void __launch_bounds__(256) cast_text_write_kernel(const void *__restrict__ values, const uint32_t *__restrict__ out_off, uint8_t *__restrict__ out, int64_t n) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint32_t d = out_off[j], olen = out_off[j + 1] - d;
        if (olen == 0) continue;
        const cast::Text t = cast::text_of<FROM>(cast_value_at(values, FROM == cast::BOOLEAN, j));
        uint8_t *q = out + d;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (8u * i + 8u <= olen) *reinterpret_cast<str_u64_unaligned *>(q + 8 * i) = t.w[i];
            else
                for (uint32_t k = 8u * i; k < olen; ++k) q[k] = uint8_t(t.w[i] >> (8u * (k & 7u)));
        }
    }
}

} // namespace
} // namespace nqe
