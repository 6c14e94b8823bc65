// string_match_parts.hpp — the per-string rules of string matching (quirk Q27: NQE_EXPR_STRING_MATCH) and nothing else: the folded byte,
// where the character that starts at a byte ends, whether a segment of the pattern matches at a byte and where that match ends, and the
// same walk backwards from the string's end.  Everything is defined on bytes; nothing here knows of validity, offsets or columns.
// Plain C++17, `__host__ __device__` under hipcc: string_match_kernels.hpp calls exactly these functions, and tests/cpp/test_string_match.cpp
// includes this header alone and runs them — one thread's whole answer and the chunked walk — against a matcher of its own.
//
// A segment is a run of elements between two ANYs: `el[k]` is element k's literal byte (already folded for ILIKE), `one[k]` != 0 makes
// it ONE.  Characters are Q26's: byte j has the number c(j) = max(1, non-continuation bytes in s[0..j]).  `lead` is the number of
// continuation bytes at the very front of the string (they belong to character 1): a byte i starts a character iff i == 0, or it is no
// continuation byte and i > lead.
//
// The greedy strategy the kernels and match_one_thread follow: the first segment is tested at 0 when the pattern does not begin with
// ANY; the last one is walked backwards from the string's end when it does not end with ANY; every other segment takes its leftmost
// match at or behind the cursor, which moves to that match's end.  That is exact: the end of a segment's match is monotone in its start
// (a literal advances one byte, "the next character start" is monotone), so the leftmost match ends no later than any other.
#pragma once

#include <cstdint>

#include "string_fn_parts.hpp"

namespace nqe {
namespace strmatch {

template <bool FOLD> NQE_STR_HD uint8_t folded(uint8_t b) {
    if constexpr (FOLD) return strfn::case_byte(b, false);
    else return b;
}

// the continuation bytes at the very front (len when the string holds nothing else)
NQE_STR_HD uint32_t leading_continuations(const uint8_t *p, uint32_t len) {
    uint32_t k = 0;
    while (k < len && strfn::is_continuation(p[k])) ++k;
    return k;
}
NQE_STR_HD bool is_char_start(const uint8_t *p, uint32_t lead, uint32_t i) { return i == 0 || (i > lead && !strfn::is_continuation(p[i])); }
// the end of the character that starts at byte i < len (is_char_start(i)): the next character start, or len
NQE_STR_HD uint32_t char_end(const uint8_t *p, uint32_t len, uint32_t lead, uint32_t i) {
    uint32_t e = i + 1;
    if (i == 0 && lead > 0) e = lead < len ? lead + 1 : len; // character 1 owns the leading continuation bytes and the byte behind them
    while (e < len && strfn::is_continuation(p[e])) ++e;
    return e;
}

// Does the segment match with its first element at byte i?  The end of the match (one past its last byte), or -1.  Reads nothing at or
// behind p[len].
template <bool FOLD>
NQE_STR_HD int32_t match_at(const uint8_t *p, uint32_t len, uint32_t lead, uint32_t i, const uint8_t *el, const uint8_t *one, uint32_t m, bool has_one) {
    if (i > len || len - i < m) return -1; // every element needs a byte
    if (!has_one) {
        for (uint32_t k = 0; k < m; ++k)
            if (folded<FOLD>(p[i + k]) != el[k]) return -1;
        return int32_t(i + m);
    }
    uint32_t pos = i;
    for (uint32_t k = 0; k < m; ++k) {
        if (pos >= len) return -1;
        if (one[k]) {
            if (!is_char_start(p, lead, pos)) return -1;
            pos = char_end(p, len, lead, pos);
        } else {
            if (folded<FOLD>(p[pos]) != el[k]) return -1;
            ++pos;
        }
    }
    return int32_t(pos);
}

// The same walk backwards: does the segment match with its last element ending at the string's end?  The start of the match, or -1.
template <bool FOLD>
NQE_STR_HD int32_t match_back(const uint8_t *p, uint32_t len, uint32_t lead, const uint8_t *el, const uint8_t *one, uint32_t m) {
    if (len < m) return -1;
    uint32_t e = len;
    for (uint32_t k = m; k-- > 0;) {
        if (e == 0) return -1;
        if (one[k]) {
            if (e < len && !is_char_start(p, lead, e)) return -1; // the piece must end where a character ends
            uint32_t s = e - 1;
            while (s > 0 && !is_char_start(p, lead, s)) --s;
            e = s;
        } else {
            if (folded<FOLD>(p[e - 1]) != el[k]) return -1;
            --e;
        }
    }
    return int32_t(e);
}

// A segment of at most 8 literal bytes as one masked word (`seg_word`: its bytes, little-endian, `seg_mask`: 0xFF in each of them).  A lane
// holds the 16 bytes of the string from byte i in w0 and w1 (what lies behind the string's end is anything) and tests the 8 positions
// i .. i + 7: bit k of the result says that the segment occurs at i + k and ends at or before `bs` (<= the string's length, so every byte
// compared is the string's own).
NQE_STR_HD uint32_t word_candidates(uint64_t w0, uint64_t w1, uint64_t seg_word, uint64_t seg_mask, uint32_t i, uint32_t seg_len, uint32_t bs) {
    uint32_t bits = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        const uint64_t window = k ? (w0 >> (8 * k)) | (w1 << (64 - 8 * k)) : w0;
        if ((window & seg_mask) == seg_word && i + k + seg_len <= bs) bits |= 1u << k;
    }
    return bits;
}
NQE_STR_HD bool is_word_segment(uint32_t seg_len, uint32_t seg_ones) { return seg_ones == 0 && seg_len <= 8; }
NQE_STR_HD uint64_t word_mask(uint32_t seg_len) { return seg_len >= 8 ? ~0ull : (1ull << (8 * seg_len)) - 1ull; }

// what the walk needs of a compiled pattern (string_match_plan.hpp's Compiled, as pointers)
struct SegView {
    uint32_t off, len, ones, pad;
};
struct Pattern {
    const uint8_t *el, *one;
    const SegView *segs;
    uint32_t nseg, min_bytes;
    int32_t anchored_front, anchored_back, has_any, negate;
    int32_t has_one; // some element is ONE (where none is, no rule looks at `lead`)
};

// The walk's fixed part, the same for every lane of a group: the anchored segments.  Sets the range [*first, *last] of the segments
// still to be searched for, the cursor and the limit `*bs` no searched match may end behind.  False: the string cannot match.
// With `*decided` the answer is final (the pattern holds no ANY, or too few bytes).
template <bool FOLD>
NQE_STR_HD bool walk_begin(const Pattern &P, const uint8_t *p, uint32_t len, uint32_t lead, uint32_t *first, int32_t *last, uint32_t *cur, uint32_t *bs, bool *decided) {
    *decided = true;
    *first = 0;
    *last = int32_t(P.nseg) - 1;
    *cur = 0;
    *bs = len;
    if (len < P.min_bytes) return false;
    if (!P.has_any) { // one segment at most, anchored at both ends
        if (P.nseg == 0) return len == 0;
        const SegView s = P.segs[0];
        return match_at<FOLD>(p, len, lead, 0, P.el + s.off, P.one + s.off, s.len, s.ones != 0) == int32_t(len);
    }
    if (P.anchored_front && P.nseg > 0) {
        const SegView s = P.segs[0];
        const int32_t e = match_at<FOLD>(p, len, lead, 0, P.el + s.off, P.one + s.off, s.len, s.ones != 0);
        if (e < 0) return false;
        *cur = uint32_t(e);
        *first = 1;
    }
    if (P.anchored_back && *last >= int32_t(*first)) {
        const SegView s = P.segs[*last];
        const int32_t b = match_back<FOLD>(p, len, lead, P.el + s.off, P.one + s.off, s.len);
        if (b < 0 || uint32_t(b) < *cur) return false;
        *bs = uint32_t(b);
        *last -= 1;
    }
    *decided = int32_t(*first) > *last; // nothing left to search for: the anchors fit
    return true;
}

// One thread's whole answer: the greedy walk, position by position.  *pos is where the LAST searched segment matched (STRPOS).
template <bool FOLD> NQE_STR_HD bool match_one_thread(const Pattern &P, const uint8_t *p, uint32_t len, uint32_t *pos) {
    const uint32_t lead = leading_continuations(p, len);
    uint32_t first, cur, bs;
    int32_t last;
    bool decided;
    *pos = 0;
    if (!walk_begin<FOLD>(P, p, len, lead, &first, &last, &cur, &bs, &decided)) return false;
    if (decided) return true;
    for (int32_t k = int32_t(first); k <= last; ++k) {
        const SegView s = P.segs[k];
        int32_t e = -1;
        uint32_t i = cur;
        for (; i + s.len <= bs; ++i) {
            e = match_at<FOLD>(p, len, lead, i, P.el + s.off, P.one + s.off, s.len, s.ones != 0);
            if (e >= 0 && uint32_t(e) <= bs) break;
            e = -1;
        }
        if (e < 0) return false;
        *pos = i;
        cur = uint32_t(e);
    }
    return true;
}

// STRPOS's character number of byte j: c(j) = max(1, non-continuation bytes in s[0..j])
NQE_STR_HD uint64_t char_number(const uint8_t *p, uint32_t j) {
    uint64_t c = 0;
    for (uint32_t k = 0; k <= j; ++k) c += strfn::is_continuation(p[k]) ? 0u : 1u;
    return c ? c : 1u;
}

} // namespace strmatch
} // namespace nqe
