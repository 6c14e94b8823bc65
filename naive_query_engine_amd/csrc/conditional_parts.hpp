// conditional_parts.hpp — the per-row rules of the conditional and NULL-handling functions (quirk Q28: NQE_EXPR_CONDITIONAL) and nothing
// else: what NOT, IS_NULL, IS_NOT_NULL, COALESCE, NULLIF and IF make of one row's values and validity.  Two forms of every rule: over one
// 8-byte word per operand with its validity as a bool (Int64, UInt64, Float64), and over 64 rows at once, a word of value bits and a word
// of validity bits per operand (Boolean operands, and everything that reads validity alone).  Nothing here knows of columns or offsets.
// Plain C++17, `__host__ __device__` under hipcc: conditional_kernels.hpp calls exactly these functions, and tests/cpp/test_conditional.cpp
// includes this header alone and decides every combination against a restatement of its own.
//
// The definitions (include/nqe.h): COALESCE(a, b) is a where a is valid, else b.  IF(c, t, e) is t where c is valid and true, e where c is
// false or NULL.  NULLIF(a, b) is IF(a = b, NULL, a) with `=` NQE_OP_EQ: a NULL a or b makes the compare NULL, so the row is a; Float64
// compares as IEEE does (NaN equals nothing, -0.0 equals +0.0), every other type by its bits.  Under a NULL result the value is 0.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define NQE_COND_HD __host__ __device__ __forceinline__
#else
#define NQE_COND_HD inline
#endif

namespace nqe {
namespace cond {

// the functions, numbered as nqe_cond_operator numbers them (conditional.hip checks that)
constexpr int NOT = 0, IS_NULL = 1, IS_NOT_NULL = 2, COALESCE = 3, NULLIF = 4, IF = 5;

// ---- one row, 8-byte words
struct Word {
    uint64_t word;
    bool valid;
};
NQE_COND_HD Word made(uint64_t w, bool valid) { return Word{valid ? w : 0ull, valid}; }

// NQE_OP_EQ on two valid words
NQE_COND_HD bool words_equal(bool f64, uint64_t x, uint64_t y) {
    if (!f64) return x == y;
    double a, b;
    __builtin_memcpy(&a, &x, 8);
    __builtin_memcpy(&b, &y, 8);
    return a == b;
}
NQE_COND_HD Word coalesce_word(uint64_t a, bool av, uint64_t b, bool bv) { return made(av ? a : b, av || bv); }
// c_true: the condition is valid AND true
NQE_COND_HD Word if_word(bool c_true, uint64_t t, bool tv, uint64_t e, bool ev) { return made(c_true ? t : e, c_true ? tv : ev); }
NQE_COND_HD Word nullif_word(bool f64, uint64_t a, bool av, uint64_t b, bool bv) { return made(a, av && !(bv && words_equal(f64, a, b))); }
template <int F> NQE_COND_HD Word select_word(bool f64, bool c_true, uint64_t a, bool av, uint64_t b, bool bv) {
    if constexpr (F == COALESCE) return coalesce_word(a, av, b, bv);
    else if constexpr (F == NULLIF) return nullif_word(f64, a, av, b, bv);
    else return if_word(c_true, a, av, b, bv);
}

// ---- 64 rows: bit k of `value` and of `valid` is row k's (an operand without validity: valid = all ones)
struct Bits {
    uint64_t value, valid;
};
NQE_COND_HD Bits made_bits(uint64_t value, uint64_t valid) { return Bits{value & valid, valid}; }
NQE_COND_HD Bits not_bits(uint64_t b, uint64_t bv) { return made_bits(~b, bv); }
NQE_COND_HD Bits is_null_bits(uint64_t xv) { return Bits{~xv, ~0ull}; }
NQE_COND_HD Bits is_not_null_bits(uint64_t xv) { return Bits{xv, ~0ull}; }
NQE_COND_HD Bits coalesce_bits(uint64_t a, uint64_t av, uint64_t b, uint64_t bv) { return made_bits((a & av) | (b & ~av), av | bv); }
NQE_COND_HD Bits if_bits(uint64_t c, uint64_t cv, uint64_t t, uint64_t tv, uint64_t e, uint64_t ev) {
    const uint64_t pick = c & cv;
    return made_bits((t & pick) | (e & ~pick), (tv & pick) | (ev & ~pick));
}
NQE_COND_HD Bits nullif_bits(uint64_t a, uint64_t av, uint64_t b, uint64_t bv) { return made_bits(a, av & ~(bv & ~(a ^ b))); }
// c, cv: IF's condition; a, av / b, bv: the one operand of the one-operand forms (a), a and b, or t and e
template <int F> NQE_COND_HD Bits select_bits(uint64_t c, uint64_t cv, uint64_t a, uint64_t av, uint64_t b, uint64_t bv) {
    if constexpr (F == NOT) return not_bits(a, av);
    else if constexpr (F == IS_NULL) return is_null_bits(av);
    else if constexpr (F == IS_NOT_NULL) return is_not_null_bits(av);
    else if constexpr (F == COALESCE) return coalesce_bits(a, av, b, bv);
    else if constexpr (F == NULLIF) return nullif_bits(a, av, b, bv);
    else return if_bits(c, cv, a, av, b, bv);
}
// the bits of bitmap word w that are rows of an n-row column: what a stored value or validity word is ANDed with
NQE_COND_HD uint64_t tail_mask(int64_t n, int64_t w) {
    const int64_t left = n - 64 * w;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
}
NQE_COND_HD Bits masked(Bits r, uint64_t mask) { return Bits{r.value & mask, r.valid & mask}; }

// ---- Utf8: which operand a result row's bytes come from
constexpr uint8_t FROM_A = 0, FROM_B = 1, FROM_NONE = 2; // FROM_NONE: the row is NULL, and empty
// c_true: IF's condition valid and true (COALESCE(a, b) is IF(a is valid, a, b); NULLIF(a, b) is IF(a = b, NULL, a))
NQE_COND_HD uint8_t pick_source(bool c_true, bool av, bool bv) { return c_true ? (av ? FROM_A : FROM_NONE) : (bv ? FROM_B : FROM_NONE); }

} // namespace cond
} // namespace nqe
