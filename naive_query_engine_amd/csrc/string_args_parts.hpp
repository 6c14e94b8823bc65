// string_args_parts.hpp — the per-string rules of the string functions with arguments (quirk Q26: NQE_EXPR_STRING_ARGS) and nothing else:
// SUBSTR's window and where its k-th character starts, REPEAT's and REPLACE's saturating lengths, whether a pattern has a border, the
// candidate test, the greedy resolution of one chunk's candidates and where a byte of a chunk goes.  Everything is defined on bytes;
// nothing here knows of validity, offsets or columns.
// Plain C++17, `__host__ __device__` under hipcc: string_args_kernels.hpp calls exactly these functions, and tests/cpp/test_string_args.cpp
// includes this header alone and runs them — one thread's whole answer and the lane-by-lane walk — against a reference of its own.
#pragma once

#include <cstdint>

#include "string_fn_parts.hpp"

namespace nqe {
namespace strargs {

// A row's byte count is clamped here.  Anything above 2^31-1 already overflows the int32 offsets, and 2^31 rows of 2^32 still sum
// without wrapping in 64 bits: the total is exact whenever it matters and never wraps.
constexpr uint64_t ROW_CAP = 1ull << 32;
constexpr uint64_t MAX_TOTAL = 0x7FFFFFFFull; // the largest data buffer int32 offsets address

// ---- SUBSTR(s, start, len): the bytes j with max(start, 1) <= c(j) < start + len, where c(j) = max(1, non-continuation bytes in s[0..j])
// The window in character numbers, [lo, hi): false when no character number lies in it (len <= 0, or start + len <= 1).  The sum
// saturates at INT64_MAX (start > 0 and len > 0 are the only way to overflow).
NQE_STR_HD bool substr_window(int64_t start, int64_t len, uint64_t *lo, uint64_t *hi) {
    if (len <= 0) return false;
    int64_t h;
    if (__builtin_add_overflow(start, len, &h)) h = INT64_MAX;
    if (h <= 1) return false;
    *lo = start < 1 ? 1u : uint64_t(start);
    *hi = uint64_t(h);
    return true; // (len > 0: lo < hi — or both saturated at INT64_MAX, a window no character number lies in)
}
// The byte (0-7) of a word at which its r-th (1-based) marked byte lies; `mask` has 0x80 in every marked byte and at least r of them.
NQE_STR_HD uint32_t nth_marked_byte(uint64_t mask, uint32_t r) {
    for (uint32_t k = 1; k < r; ++k) mask &= mask - 1;
    return uint32_t(__builtin_ctzll(mask)) >> 3;
}
// A word of which `before` non-continuation bytes of the string lie in front: the byte of the word that is the string's k-th
// non-continuation byte (1-based), or 8 when that byte is not in this word.
NQE_STR_HD uint32_t kth_in_word(uint64_t mask, uint64_t before, uint64_t k) {
    const uint64_t here = uint64_t(__builtin_popcountll(mask));
    return (k > before && k - before <= here) ? nth_marked_byte(mask, uint32_t(k - before)) : 8u;
}
// The last, partial word of a string (nbytes < 8), read byte by byte — nothing behind the string is touched — and filled up with
// continuation bytes, which no count sees.
NQE_STR_HD uint64_t tail_word(const uint8_t *p, uint32_t nbytes) {
    uint64_t w = 0x8080808080808080ull;
    for (uint32_t k = 0; k < nbytes; ++k) w = (w & ~(0xFFull << (8 * k))) | (uint64_t(p[k]) << (8 * k));
    return w;
}
// the position of the string's k-th non-continuation byte (1-based), or len: where character number k >= 2 begins
NQE_STR_HD uint32_t nth_noncontinuation(const uint8_t *p, uint32_t len, uint64_t k) {
    uint64_t seen = 0;
    for (uint32_t j = 0; j < len; ++j)
        if (!strfn::is_continuation(p[j]) && ++seen == k) return j;
    return len;
}
// The kept range [first, end) from the positions of the window's two characters: character 1 begins at byte 0 whatever the bytes are
// (continuation bytes at the very front belong to it).  `pos_lo` / `pos_hi`: nth_noncontinuation of lo / hi.
NQE_STR_HD void substr_combine(uint64_t lo, uint32_t pos_lo, uint32_t pos_hi, uint32_t *first, uint32_t *end) {
    *first = lo <= 1 ? 0u : pos_lo;
    *end = pos_hi < *first ? *first : pos_hi;
}
// one thread's whole answer; the empty result is [0, 0)
NQE_STR_HD void substr_range(const uint8_t *p, uint32_t len, int64_t start, int64_t count, uint32_t *first, uint32_t *end) {
    uint64_t lo, hi;
    *first = *end = 0;
    if (!substr_window(start, count, &lo, &hi)) return;
    substr_combine(lo, lo <= 1 ? 0u : nth_noncontinuation(p, len, lo), nth_noncontinuation(p, len, hi), first, end);
    if (*first >= len) *first = *end = 0; // (a start past the end)
}

// ---- REPEAT(s, n): max(n, 0) copies.  The length saturates at ROW_CAP.
NQE_STR_HD uint64_t repeat_length(uint32_t len, int64_t n) {
    if (n <= 0 || len == 0) return 0;
    if (uint64_t(n) >= ROW_CAP) return ROW_CAP;
    const uint64_t prod = uint64_t(len) * uint64_t(n); // both below 2^32
    return prod < ROW_CAP ? prod : ROW_CAP;
}

// ---- REPLACE(s, from, to), |from| = m >= 1, |to| = t
// Has the pattern a border: a proper, non-empty prefix that is also its suffix?  Two occurrences can overlap only if it has; for a
// border-free pattern every occurrence is a match of the greedy left-to-right search.
NQE_STR_HD bool has_border(const uint8_t *from, uint32_t m) {
    for (uint32_t b = 1; b < m; ++b) {
        uint32_t k = 0;
        while (k < b && from[k] == from[m - b + k]) ++k;
        if (k == b) return true;
    }
    return false;
}
// Does `from` occur at byte i of the string?  Reads at most m bytes and nothing at or behind the string's end.
NQE_STR_HD bool is_candidate(const uint8_t *p, uint32_t len, uint32_t i, const uint8_t *from, uint32_t m) {
    if (i >= len || len - i < m) return false;
    for (uint32_t k = 0; k < m; ++k)
        if (p[i + k] != from[k]) return false;
    return true;
}
// One chunk of up to 64 positions starting at byte chunk0: bit b of `cand` says that the pattern occurs at chunk0 + b.  Returns the
// occurrences the greedy search takes — those at or behind *next_free, the end of the match before — and moves *next_free behind the
// chunk's last match.  Without a border no two candidates overlap and all of them are taken.
NQE_STR_HD uint64_t resolve_matches(uint64_t cand, uint32_t chunk0, uint32_t m, bool bordered, uint32_t *next_free) {
    uint64_t taken = cand;
    if (bordered) {
        uint32_t nf = *next_free;
        taken = 0;
        for (uint64_t c = cand; c; c &= c - 1) {
            const uint32_t b = uint32_t(__builtin_ctzll(c));
            if (chunk0 + b >= nf) {
                taken |= 1ull << b;
                nf = chunk0 + b + m;
            }
        }
    }
    if (taken) *next_free = chunk0 + (63u - uint32_t(__builtin_clzll(taken))) + m;
    return taken;
}
// the result's length from the number of matches; saturates at ROW_CAP (matches * m <= len, and matches, t < 2^31: no 64-bit overflow)
NQE_STR_HD uint64_t replaced_length(uint32_t len, uint64_t matches, uint32_t m, uint32_t t) {
    const uint64_t r = uint64_t(len) - matches * m + matches * t;
    return r < ROW_CAP ? r : ROW_CAP;
}
// What becomes of byte chunk0 + b, given the chunk's matches, the matches in front of the chunk and the end of the last of them
struct Placement {
    bool is_start; // a match begins here: the bytes of `to` go to `out`
    bool covered;  // inside a match that began earlier: the byte goes nowhere (under |to| == |from|: it becomes to[within])
    uint32_t within; // covered: the byte's index within its match
    uint64_t out;  // the result position of this byte, or of the copy of `to` that replaces the match beginning here
};
NQE_STR_HD Placement place_byte(uint64_t taken, uint32_t chunk0, uint32_t b, uint64_t matches_before_chunk, uint32_t next_free_before_chunk, uint32_t m, uint32_t t) {
    const uint64_t low = b ? taken & (~0ull >> (64 - b)) : 0ull;
    const uint32_t i = chunk0 + b;
    const uint32_t last_end = low ? chunk0 + (63u - uint32_t(__builtin_clzll(low))) + m : next_free_before_chunk;
    const uint64_t before = matches_before_chunk + uint64_t(__builtin_popcountll(low));
    Placement r;
    r.is_start = (taken >> b) & 1;
    r.covered = !r.is_start && i < last_end;
    r.within = r.covered ? i - (last_end - m) : 0u;
    r.out = uint64_t(i) - before * m + before * t;
    return r;
}

} // namespace strargs
} // namespace nqe
