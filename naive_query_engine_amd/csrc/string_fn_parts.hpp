// string_fn_parts.hpp — the per-string and per-byte rules of the string functions (quirk Q25: NQE_EXPR_STRING) and nothing else: the trim
// range of a byte range, the case map of one byte and of an 8-byte word, where a unit of REVERSE starts and where a byte goes, and the
// non-continuation count of a word.  Everything is defined on bytes; nothing here knows of validity, offsets or columns.
// Plain C++17, `__host__ __device__` under hipcc: string_fn_kernels.hpp calls exactly these functions, and tests/cpp/test_string_fn.cpp
// includes this header alone and runs them against a sequential reference of its own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define NQE_STR_HD __host__ __device__ __forceinline__
#else
#define NQE_STR_HD inline
#endif

namespace nqe {
namespace strfn {

constexpr uint64_t ONES = 0x0101010101010101ull, HIGH = 0x8080808080808080ull;

// ---- TRIM / LTRIM / RTRIM: byte 0x20 and no other (SQL's and DataFusion's default; tab, newline, U+00A0, U+3000 stay)
enum TrimMode : int { TRIM_FRONT = 1, TRIM_BACK = 2, TRIM_BOTH = 3 };
NQE_STR_HD bool is_trim_byte(uint8_t b) { return b == 0x20; }
// Lane `lane` of `lanes` looks at bytes lane, lane + lanes, … from the front: the first of them that is kept, or `len`.  The minimum over
// the lanes is the first kept byte of the string.
NQE_STR_HD uint32_t trim_front_scan(const uint8_t *p, uint32_t len, uint32_t lane, uint32_t lanes) {
    uint32_t i = lane;
    while (i < len && is_trim_byte(p[i])) i += lanes;
    return i < len ? i : len;
}
// The same from the back (bytes len-1-lane, len-1-lane-lanes, …): one past the last of them that is kept, or 0.  The maximum over the
// lanes is one past the last kept byte.
NQE_STR_HD uint32_t trim_back_scan(const uint8_t *p, uint32_t len, uint32_t lane, uint32_t lanes) {
    int64_t i = int64_t(len) - 1 - int64_t(lane);
    while (i >= 0 && is_trim_byte(p[i])) i -= int64_t(lanes);
    return i >= 0 ? uint32_t(i) + 1 : 0u;
}
// The kept range [first, end) from the two scans' minimum and maximum; a side the mode leaves alone keeps its end of the string, and a
// string of only trimmed bytes is the empty range at `first`.
NQE_STR_HD void trim_combine(int mode, uint32_t len, uint32_t front_min, uint32_t back_max, uint32_t *first, uint32_t *end) {
    uint32_t f = (mode & TRIM_FRONT) ? front_min : 0u, e = (mode & TRIM_BACK) ? back_max : len;
    if (e < f) e = f;
    *first = f;
    *end = e;
}
// one thread's whole answer
NQE_STR_HD void trim_range(const uint8_t *p, uint32_t len, int mode, uint32_t *first, uint32_t *end) {
    trim_combine(mode, len, (mode & TRIM_FRONT) ? trim_front_scan(p, len, 0, 1) : 0u, (mode & TRIM_BACK) ? trim_back_scan(p, len, 0, 1) : len, first, end);
}

// ---- LOWER / UPPER: ASCII only, A-Z <-> a-z, every other byte (all of a multi-byte sequence's) unchanged
NQE_STR_HD uint8_t case_byte(uint8_t b, bool upper) {
    const uint8_t lo = upper ? 'a' : 'A', hi = upper ? 'z' : 'Z';
    return (b >= lo && b <= hi) ? uint8_t(b ^ 0x20) : b;
}
// Eight bytes at once, branch-free: the range test runs on the low seven bits of every byte (no sum reaches bit 8, so no byte carries
// into its neighbour), bytes with bit 7 set are masked out, and the surviving 0x80 marks become the 0x20 to flip.
NQE_STR_HD uint64_t case_word(uint64_t w, bool upper) {
    const uint64_t lo = upper ? 'a' : 'A', hi = upper ? 'z' : 'Z';
    const uint64_t low7 = w & ~HIGH;
    const uint64_t ge_lo = low7 + (0x80 - lo) * ONES;      // bit 7: low7 >= lo
    const uint64_t gt_hi = low7 + (0x80 - (hi + 1)) * ONES; // bit 7: low7 > hi
    const uint64_t m = ge_lo & ~gt_hi & ~w & HIGH;
    return w ^ (m >> 2);
}

// ---- CHARACTER_LENGTH: the bytes that are no continuation byte (10xxxxxx)
NQE_STR_HD bool is_continuation(uint8_t b) { return (b & 0xC0) == 0x80; }
// 0x80 in every byte of `w` that is no continuation byte
NQE_STR_HD uint64_t noncontinuation_mask(uint64_t w) { return ~(w & ~(w << 1)) & HIGH; } // (w << 1: bit 6 of a byte lands on its own bit 7)
NQE_STR_HD uint32_t noncontinuation_count(uint64_t w) { return uint32_t(__builtin_popcountll(noncontinuation_mask(w))); }

// ---- REVERSE: the order of units is reversed, the bytes of a unit keep theirs.  Byte i starts a unit iff i == 0, or it is no continuation
// byte, or bytes i-1, i-2 and i-3 all exist and are continuation bytes: units are 1-4 bytes long, and on valid UTF-8 exactly the code points.
NQE_STR_HD bool is_unit_start(const uint8_t *p, uint32_t len, uint32_t i) {
    (void)len;
    if (i == 0 || !is_continuation(p[i])) return true;
    return i >= 3 && is_continuation(p[i - 1]) && is_continuation(p[i - 2]) && is_continuation(p[i - 3]);
}
// where byte i of the string goes: reads p[i-6 .. i+3] at most, and nothing outside [0, len)
NQE_STR_HD uint32_t reverse_dest(const uint8_t *p, uint32_t len, uint32_t i) {
    uint32_t s = i, e = i + 1;
    while (!is_unit_start(p, len, s)) --s;              // at most 3 steps: byte 0 starts a unit, and no unit is longer than 4
    while (e < len && !is_unit_start(p, len, e)) ++e;   // likewise
    return len - e + (i - s);
}
// Eight bytes at once: when none of the word's bytes has bit 7 set and the byte behind the word (`next`; pass 0 at the string's end) is no
// continuation byte, every byte of the word is a unit of its own, so byte i + k goes to len - 1 - (i + k): the word, byte-swapped, at
// len - 8 - i.  Any other word goes byte by byte through reverse_dest.
NQE_STR_HD bool is_single_byte_units_word(uint64_t w, uint8_t next) { return (w & HIGH) == 0 && !is_continuation(next); }
NQE_STR_HD uint64_t reverse_word(uint64_t w) { return __builtin_bswap64(w); }

} // namespace strfn
} // namespace nqe
