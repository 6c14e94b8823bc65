// string_match_plan.hpp — the host side of an NQE_EXPR_STRING_MATCH node (quirk Q27): the pattern literal compiled into what the kernels
// of string_match_kernels.hpp walk.  A LIKE / ILIKE pattern becomes its elements (a literal byte, or ONE), cut at every ANY into
// segments; STARTS_WITH / ENDS_WITH / CONTAINS / STRPOS take the literal verbatim as one segment.  The FORM says which kernel serves the
// pattern and how: the anchored forms compare a prefix and / or a suffix and never search.
// Plain C++17, no HIP: tests/cpp/test_string_match_plan.cpp compiles this header (and expr_plan.hpp) alone.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nqe.h"

namespace nqe {
namespace strmatch {

enum Form : int {
    FORM_ALWAYS = 0,        // `%`, and an empty STARTS_WITH / ENDS_WITH / CONTAINS literal: true for every string
    FORM_EQUAL = 1,         // no ANY, no ONE: the string is the literal
    FORM_PREFIX = 2,        // lit%
    FORM_SUFFIX = 3,        // %lit
    FORM_PREFIX_SUFFIX = 4, // lit%lit
    FORM_CONTAINS = 5,      // %lit%, without ONE
    FORM_GENERAL = 6        // everything else: the greedy walk over the segments
};

// a maximal run of elements between two ANYs (never empty)
struct Segment {
    uint32_t off, len; // its elements: [off, off + len) of `elems` and `ones`
    uint32_t ones;     // how many of them are ONE
    uint32_t pad;
};

struct Compiled {
    std::string elems;             // one byte per element: the literal's byte (folded for ILIKE), 0 for ONE
    std::string ones;              // one byte per element: 1 for ONE, else 0
    std::vector<Segment> segs;
    bool anchored_front = true;    // the pattern does not begin with ANY: the first segment starts at byte 0
    bool anchored_back = true;     // the pattern does not end with ANY: the last segment ends at the string's end
    bool has_any = false;
    bool fold = false;             // ILIKE: the string's bytes are folded before they are compared
    bool negate = false;           // NOT_LIKE / NOT_ILIKE
    uint32_t min_bytes = 0;        // every element needs at least one byte: a shorter string cannot match
    int form = FORM_ALWAYS;
};

inline uint8_t fold_byte(uint8_t b) { return (b >= 'A' && b <= 'Z') ? uint8_t(b | 0x20) : b; }
inline bool is_like(int op) { return op >= NQE_MATCH_LIKE && op <= NQE_MATCH_NOT_ILIKE; }

inline Compiled compile(int op, const std::string &pattern) {
    Compiled c;
    c.fold = op == NQE_MATCH_ILIKE || op == NQE_MATCH_NOT_ILIKE;
    c.negate = op == NQE_MATCH_NOT_LIKE || op == NQE_MATCH_NOT_ILIKE;
    bool open = false; // the segment being filled
    bool last_any = false, first = true;
    auto element = [&](uint8_t byte, bool one) {
        if (!open) {
            c.segs.push_back(Segment{uint32_t(c.elems.size()), 0, 0, 0});
            open = true;
        }
        c.elems.push_back(char(one ? 0 : (c.fold ? fold_byte(byte) : byte)));
        c.ones.push_back(char(one ? 1 : 0));
        ++c.segs.back().len;
        c.segs.back().ones += one ? 1u : 0u;
        last_any = false;
        first = false;
    };
    if (is_like(op)) {
        for (size_t i = 0; i < pattern.size(); ++i) {
            const uint8_t b = uint8_t(pattern[i]);
            if (b == '\\' && i + 1 < pattern.size()) element(uint8_t(pattern[++i]), false);
            else if (b == '%') {
                if (first) c.anchored_front = false;
                c.has_any = true;
                open = false;
                last_any = true;
                first = false;
            } else if (b == '_') element(0, true);
            else element(b, false); // (a `\` that ends the pattern included)
        }
        c.anchored_back = !last_any;
    } else {
        for (char ch : pattern) element(uint8_t(ch), false);
        // the verbatim operators as the LIKE they are: lit%, %lit, %lit% (STRPOS searches like CONTAINS)
        c.anchored_front = op == NQE_MATCH_STARTS_WITH;
        c.anchored_back = op == NQE_MATCH_ENDS_WITH;
        c.has_any = true;
    }
    c.min_bytes = uint32_t(c.elems.size());
    const size_t ns = c.segs.size();
    bool any_one = false;
    for (const Segment &s : c.segs) any_one = any_one || s.ones != 0;
    if (ns == 0) c.form = c.has_any ? FORM_ALWAYS : FORM_EQUAL; // `%`, an empty verbatim literal — or the empty pattern: only the empty string
    else if (any_one) c.form = FORM_GENERAL;
    else if (!c.has_any) c.form = FORM_EQUAL;
    else if (ns == 1 && c.anchored_front && !c.anchored_back) c.form = FORM_PREFIX;
    else if (ns == 1 && !c.anchored_front && c.anchored_back) c.form = FORM_SUFFIX;
    else if (ns == 1 && !c.anchored_front && !c.anchored_back) c.form = FORM_CONTAINS;
    else if (ns == 2 && c.anchored_front && c.anchored_back) c.form = FORM_PREFIX_SUFFIX;
    else c.form = FORM_GENERAL;
    return c;
}

} // namespace strmatch
} // namespace nqe
