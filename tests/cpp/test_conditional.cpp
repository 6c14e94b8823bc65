// The per-row rules of the conditional and NULL-handling functions (naive_query_engine_amd/csrc/conditional_parts.hpp, quirk Q28) on the
// CPU, every combination decided against a straight restatement of include/nqe.h.  Includes that header alone.
//   words:  each operand NULL or valid x the condition true, false or NULL x equal or unequal values, for integers and for Float64
//           (NaN, -0.0 / +0.0, infinities)
//   bits:   all 2^k assignments of one bit position of the k input words, at bit positions 0, 1, 62 and 63, and whole random words
//           against the word rules bit by bit; the tail mask at 0, 1, 63, 64, 65, 127, 128 rows
//   Utf8:   the source of a row for every combination
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_conditional.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "conditional_parts.hpp"

using namespace nqe::cond;

static int failures = 0;
static long checked = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++checked;                                                               \
        if (!(cond)) {                                                           \
            if (++failures <= 40) std::printf("%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

static uint64_t bits_of(double d) { uint64_t w; std::memcpy(&w, &d, 8); return w; }

// ---- the restatement: an optional value per operand
struct Opt {
    bool valid;
    uint64_t w;
};
static bool same(const Word &r, const Opt &want) { return r.valid == want.valid && r.word == (want.valid ? want.w : 0ull); }
static bool ref_equal(bool f64, uint64_t x, uint64_t y) {
    if (!f64) return x == y;
    double a, b;
    std::memcpy(&a, &x, 8);
    std::memcpy(&b, &y, 8);
    if (std::isnan(a) || std::isnan(b)) return false;
    return a == b; // (-0.0 == +0.0)
}
static Opt ref_coalesce(Opt a, Opt b) { return a.valid ? a : b; }
// c: 0 false, 1 true, 2 NULL
static Opt ref_if(int c, Opt t, Opt e) { return c == 1 ? t : e; }
static Opt ref_nullif(bool f64, Opt a, Opt b) {
    const int eq = (a.valid && b.valid) ? (ref_equal(f64, a.w, b.w) ? 1 : 0) : 2; // a = b: NULL when either is
    return ref_if(eq, Opt{false, 0}, a);
}

static void test_words() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const uint64_t ints[] = {0, 1, 7, 0x8000000000000000ull, 0x7fffffffffffffffull, ~0ull};
    const uint64_t floats[] = {bits_of(0.0), bits_of(-0.0), bits_of(1.5), bits_of(-1.5), bits_of(nan), bits_of(-nan), bits_of(inf), bits_of(-inf), 0x7ff8000000000001ull};
    for (int f64 = 0; f64 < 2; ++f64) {
        const uint64_t *vals = f64 ? floats : ints;
        const int nv = f64 ? int(sizeof(floats) / 8) : int(sizeof(ints) / 8);
        for (int i = 0; i < nv; ++i)
            for (int k = 0; k < nv; ++k)
                for (int av = 0; av < 2; ++av)
                    for (int bv = 0; bv < 2; ++bv) {
                        const Opt a{av != 0, vals[i]}, b{bv != 0, vals[k]};
                        CHECK(same(coalesce_word(a.w, a.valid, b.w, b.valid), ref_coalesce(a, b)));
                        CHECK(same(select_word<COALESCE>(f64 != 0, false, a.w, a.valid, b.w, b.valid), ref_coalesce(a, b)));
                        CHECK(same(nullif_word(f64 != 0, a.w, a.valid, b.w, b.valid), ref_nullif(f64 != 0, a, b)));
                        CHECK(same(select_word<NULLIF>(f64 != 0, true, a.w, a.valid, b.w, b.valid), ref_nullif(f64 != 0, a, b)));
                        for (int c = 0; c < 3; ++c) { // false, true, NULL: the kernels pass "valid and true"
                            CHECK(same(if_word(c == 1, a.w, a.valid, b.w, b.valid), ref_if(c, a, b)));
                            CHECK(same(select_word<IF>(f64 != 0, c == 1, a.w, a.valid, b.w, b.valid), ref_if(c, a, b)));
                        }
                        // nullif(a, b) is if(a = b, NULL, a)
                        const bool eq_true = a.valid && b.valid && words_equal(f64 != 0, a.w, b.w);
                        const Word viaif = if_word(eq_true, 0, false, a.w, a.valid), direct = nullif_word(f64 != 0, a.w, a.valid, b.w, b.valid);
                        CHECK(viaif.valid == direct.valid && viaif.word == direct.word);
                    }
    }
    // the rule taken from NQE_OP_EQ, by hand
    CHECK(!nullif_word(true, bits_of(-0.0), true, bits_of(0.0), true).valid);                                   // -0.0 = +0.0: NULL
    CHECK(nullif_word(true, bits_of(nan), true, bits_of(nan), true).valid);                                     // NaN = NaN is false: NaN stays
    CHECK(nullif_word(true, bits_of(nan), true, bits_of(nan), true).word == bits_of(nan));
    CHECK(!nullif_word(true, bits_of(inf), true, bits_of(inf), true).valid && nullif_word(true, bits_of(inf), true, bits_of(-inf), true).valid);
    CHECK(nullif_word(false, bits_of(-0.0), true, bits_of(0.0), true).valid);                                   // as integers the two words differ
    CHECK(!nullif_word(false, 0x8000000000000000ull, true, 0x8000000000000000ull, true).valid);
}

// ---- bits: bit p of every result must be the word rule applied to bit p of every input
static Opt bit_opt(uint64_t value, uint64_t valid, int p) { return Opt{((valid >> p) & 1) != 0, (value >> p) & 1}; }
static bool bit_same(const Bits &r, int p, const Opt &want) {
    const bool v = (r.valid >> p) & 1, b = (r.value >> p) & 1;
    return v == want.valid && b == (want.valid ? want.w != 0 : false);
}
static void check_position(uint64_t c, uint64_t cv, uint64_t a, uint64_t av, uint64_t b, uint64_t bv, int p) {
    const Opt A = bit_opt(a, av, p), B = bit_opt(b, bv, p), C = bit_opt(c, cv, p);
    CHECK(bit_same(not_bits(a, av), p, Opt{A.valid, uint64_t(!A.w)}));
    CHECK(bit_same(is_null_bits(av), p, Opt{true, uint64_t(!A.valid)}));
    CHECK(bit_same(is_not_null_bits(av), p, Opt{true, uint64_t(A.valid)}));
    CHECK(bit_same(coalesce_bits(a, av, b, bv), p, ref_coalesce(A, B)));
    CHECK(bit_same(nullif_bits(a, av, b, bv), p, ref_nullif(false, A, B)));
    CHECK(bit_same(if_bits(c, cv, a, av, b, bv), p, ref_if(C.valid ? int(C.w) : 2, A, B)));
    CHECK(bit_same(select_bits<NOT>(c, cv, a, av, b, bv), p, Opt{A.valid, uint64_t(!A.w)}));
    CHECK(bit_same(select_bits<IS_NULL>(c, cv, a, av, b, bv), p, Opt{true, uint64_t(!A.valid)}));
    CHECK(bit_same(select_bits<IS_NOT_NULL>(c, cv, a, av, b, bv), p, Opt{true, uint64_t(A.valid)}));
    CHECK(bit_same(select_bits<COALESCE>(c, cv, a, av, b, bv), p, ref_coalesce(A, B)));
    CHECK(bit_same(select_bits<NULLIF>(c, cv, a, av, b, bv), p, ref_nullif(false, A, B)));
    CHECK(bit_same(select_bits<IF>(c, cv, a, av, b, bv), p, ref_if(C.valid ? int(C.w) : 2, A, B)));
}

static void test_bits() {
    // all 2^6 assignments of one bit position, the other 63 positions all zeros and all ones
    for (int p : {0, 1, 31, 62, 63})
        for (int asg = 0; asg < 64; ++asg)
            for (uint64_t others : {0ull, ~0ull}) {
                uint64_t w[6];
                for (int k = 0; k < 6; ++k) w[k] = (others & ~(1ull << p)) | (uint64_t((asg >> k) & 1) << p);
                check_position(w[0], w[1], w[2], w[3], w[4], w[5], p);
                for (int q : {0, 17, 63})
                    if (q != p) check_position(w[0], w[1], w[2], w[3], w[4], w[5], q);
            }
    // whole words of a fixed pseudo-random sequence, every position
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int round = 0; round < 200; ++round) {
        const uint64_t c = next(), cv = next() | next(), a = next(), av = next() | next(), b = next(), bv = next() | next();
        for (int p = 0; p < 64; ++p) check_position(c, cv, a, av, b, bv, p);
        // the value bit under a NULL is 0, whatever the operands hold there
        for (const Bits &r : {not_bits(a, av), coalesce_bits(a, av, b, bv), nullif_bits(a, av, b, bv), if_bits(c, cv, a, av, b, bv)}) CHECK((r.value & ~r.valid) == 0);
    }
    // the tail: rows 64w .. n-1 of word w
    const int64_t rows[] = {0, 1, 63, 64, 65, 127, 128, 129};
    for (int64_t n : rows)
        for (int64_t w = 0; w < 3; ++w) {
            uint64_t want = 0;
            for (int p = 0; p < 64; ++p)
                if (64 * w + p < n) want |= 1ull << p;
            CHECK(tail_mask(n, w) == want);
            const Bits m = masked(Bits{~0ull, ~0ull}, tail_mask(n, w)); // is_null of an all-NULL column, is_not_null of one without NULLs
            CHECK(m.value == want && m.valid == want);
        }
    CHECK(tail_mask(1, 0) == 1ull && tail_mask(63, 0) == 0x7fffffffffffffffull && tail_mask(64, 0) == ~0ull && tail_mask(64, 1) == 0ull);
}

static void test_sources() {
    for (int c = 0; c < 2; ++c)
        for (int av = 0; av < 2; ++av)
            for (int bv = 0; bv < 2; ++bv) {
                const uint8_t want = c ? (av ? FROM_A : FROM_NONE) : (bv ? FROM_B : FROM_NONE);
                CHECK(pick_source(c != 0, av != 0, bv != 0) == want);
            }
    // coalesce(a, b) = if(a is valid, a, b): never FROM_NONE while either is valid
    for (int av = 0; av < 2; ++av)
        for (int bv = 0; bv < 2; ++bv) CHECK((pick_source(av != 0, av != 0, bv != 0) == FROM_NONE) == (!av && !bv));
    CHECK(NOT == 0 && IS_NULL == 1 && IS_NOT_NULL == 2 && COALESCE == 3 && NULLIF == 4 && IF == 5);
}

int main() {
    test_words();
    test_bits();
    test_sources();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("conditional ok: %ld checks\n", checked);
    return 0;
}
