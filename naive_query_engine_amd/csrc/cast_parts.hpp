// cast_parts.hpp — the per-row rules of a cast (quirk Q29: NQE_EXPR_CAST) and nothing else: what one value of one type becomes in another.
// The rules are arrow's cast with safe = true, restated (include/nqe.h): a conversion that cannot represent the value is NULL, never an
// error and never a wrapped value; under a NULL the word is 0.  Nothing here knows of columns, offsets or validity buffers.
// Plain C++17, `__host__ __device__` under hipcc: cast_kernels.hpp calls exactly these functions, and tests/cpp/test_cast.cpp includes this
// header alone and decides every rule against a restatement of its own.
//
// The string parsers of Int64, Float64 and Boolean are the CSV reader's (csv_parse.hpp: parse_i64, parse_f64, parse_bool), called on the
// bytes between a slot's two offsets, untrimmed.  The UInt64 parser is this header's: the CSV reader infers no UInt64 column.
#pragma once

#include <cstdint>

#include "csv_parse.hpp"

namespace nqe {
namespace cast {

// the types, numbered as nqe_dtype numbers them (cast.hip checks that)
constexpr int BOOLEAN = 1, INT64 = 2, UINT64 = 3, FLOAT64 = 4, UTF8 = 5;

struct Word {
    uint64_t word; // a Boolean result: 0 or 1
    bool valid;
};
NQE_HD Word made(uint64_t w, bool valid) { return Word{valid ? w : 0ull, valid}; }

NQE_HD double as_f64(uint64_t w) {
    double d;
    __builtin_memcpy(&d, &w, 8);
    return d;
}
NQE_HD uint64_t f64_bits(double d) {
    uint64_t w;
    __builtin_memcpy(&w, &d, 8);
    return w;
}

// can the cast from -> to give NULL for a valid operand?  (its result then always carries a validity buffer)
NQE_HD bool fallible(int from, int to) {
    if (from == to) return false;
    if (from == UTF8) return true;
    if (from == INT64) return to == UINT64;
    if (from == UINT64) return to == INT64;
    if (from == FLOAT64) return to == INT64 || to == UINT64;
    return false;
}

// Float64 -> Int64: NULL iff NaN, x < -2^63 or x >= 2^63 (the test comes first: the conversion of anything else is defined)
NQE_HD Word f64_to_i64(double x) {
    if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) return Word{0, false};
    return Word{uint64_t(int64_t(x)), true};
}
// Float64 -> UInt64: NULL iff NaN, x <= -1.0 or x >= 2^64; (-1, 0] truncates to 0
NQE_HD Word f64_to_u64(double x) {
    if (!(x > -1.0 && x < 18446744073709551616.0)) return Word{0, false};
    return Word{x <= 0.0 ? 0ull : uint64_t(x), true};
}

// one valid value of a word type or Boolean (0 / 1) to a word type or Boolean; FROM != TO, neither Utf8
template <int FROM, int TO> NQE_HD Word convert(uint64_t w) {
    static_assert(FROM != TO && FROM >= BOOLEAN && FROM <= FLOAT64 && TO >= BOOLEAN && TO <= FLOAT64, "a cast between two different fixed-width types");
    if constexpr (TO == BOOLEAN) { // v != 0: NaN is true, -0.0 is false
        if constexpr (FROM == FLOAT64) return Word{as_f64(w) != 0.0 ? 1ull : 0ull, true};
        else return Word{w != 0 ? 1ull : 0ull, true};
    } else if constexpr (FROM == BOOLEAN) {
        if constexpr (TO == FLOAT64) return Word{f64_bits(w ? 1.0 : 0.0), true};
        else return Word{w ? 1ull : 0ull, true};
    } else if constexpr (FROM == INT64) {
        if constexpr (TO == UINT64) return made(w, int64_t(w) >= 0);
        else return Word{f64_bits(double(int64_t(w))), true}; // the nearest binary64, ties to even
    } else if constexpr (FROM == UINT64) {
        if constexpr (TO == INT64) return made(w, (w >> 63) == 0);
        else return Word{f64_bits(double(w)), true};
    } else {
        if constexpr (TO == INT64) return f64_to_i64(as_f64(w));
        else return f64_to_u64(as_f64(w));
    }
}

// [+]digits+, no other characters; false above 2^64-1 and on any `-` (`-0` included)
NQE_HD bool parse_u64(const char *s, int len, uint64_t *out) {
    int i = 0;
    if (i < len && s[i] == '+') ++i;
    if (i >= len) return false;
    uint64_t v = 0;
    for (; i < len; ++i) {
        if (!csvp::is_digit(s[i])) return false;
        const uint64_t d = uint64_t(s[i] - '0');
        if (v > (0xffffffffffffffffull - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

// the bytes of one Utf8 slot to a word type or Boolean (0 / 1); whatever the parser rejects is NULL
template <int TO> NQE_HD Word parse(const char *s, int len) {
    static_assert(TO >= BOOLEAN && TO <= FLOAT64, "a cast of Utf8 to a fixed-width type");
    if constexpr (TO == INT64) {
        int64_t v = 0;
        return csvp::parse_i64(s, len, &v) ? Word{uint64_t(v), true} : Word{0, false};
    } else if constexpr (TO == UINT64) {
        uint64_t v = 0;
        return parse_u64(s, len, &v) ? Word{v, true} : Word{0, false};
    } else if constexpr (TO == FLOAT64) {
        double d = 0.0;
        return csvp::parse_f64(s, len, &d) ? Word{f64_bits(d), true} : Word{0, false};
    } else {
        bool b = false;
        return csvp::parse_bool(s, len, &b) ? Word{b ? 1ull : 0ull, true} : Word{0, false};
    }
}

// ---- to Utf8: the shortest decimal of an integer, `true` / `false` of a Boolean
constexpr int MAX_TEXT = 20; // INT64_MIN, and 2^64-1

// decimal digits of v: 1 .. 20
NQE_HD int digit_count(uint64_t v) {
    int n = 1;
    while (v >= 10000) {
        v /= 10000;
        n += 4;
    }
    return n + (v >= 1000 ? 3 : v >= 100 ? 2 : v >= 10 ? 1 : 0);
}
// the magnitude of an Int64 word (INT64_MIN: 2^63)
NQE_HD uint64_t magnitude(uint64_t w) { return int64_t(w) < 0 ? 0ull - w : w; }

template <int FROM> NQE_HD int text_length(uint64_t w) {
    static_assert(FROM == BOOLEAN || FROM == INT64 || FROM == UINT64, "a cast to Utf8 of Boolean, Int64 or UInt64");
    if constexpr (FROM == BOOLEAN) return w ? 4 : 5;
    else if constexpr (FROM == INT64) return digit_count(magnitude(w)) + (int64_t(w) < 0 ? 1 : 0);
    else return digit_count(w);
}

// The text of a value as three 8-byte words, byte k of the text = byte (k & 7) of words[k >> 3] (little endian: the order of memory):
// the digits are formed from the last one back, in registers, and stored by the caller in 8-byte words where whole ones fit.
struct Text {
    uint64_t w[3];
    int len;
};
template <int FROM> NQE_HD Text text_of(uint64_t v) {
    Text t{{0, 0, 0}, text_length<FROM>(v)};
    if constexpr (FROM == BOOLEAN) {
        t.w[0] = v ? 0x65757274ull /* "true" */ : 0x65736c6166ull /* "false" */;
    } else {
        const bool neg = FROM == INT64 && int64_t(v) < 0;
        uint64_t m = FROM == INT64 ? magnitude(v) : v;
        uint64_t w0 = 0, w1 = 0, w2 = 0; // named, not indexed: a register array indexed at run time would go to scratch memory
        for (int k = t.len - 1; k >= (neg ? 1 : 0); --k) {
            const uint64_t c = uint64_t('0' + m % 10) << (8 * (k & 7));
            m /= 10;
            if (k < 8) w0 |= c;
            else if (k < 16) w1 |= c;
            else w2 |= c;
        }
        if (neg) w0 |= uint64_t('-');
        t.w[0] = w0;
        t.w[1] = w1;
        t.w[2] = w2;
    }
    return t;
}
// the text written to `out` (t.len bytes), byte by byte: the host form, and the kernels' tail
NQE_HD int write_text(const Text &t, char *out) {
    for (int k = 0; k < t.len; ++k) out[k] = char((t.w[k >> 3] >> (8 * (k & 7))) & 0xff);
    return t.len;
}

} // namespace cast
} // namespace nqe
