// The per-row rules of a cast (naive_query_engine_amd/csrc/cast_parts.hpp, quirk Q29) on the CPU: includes that header alone and decides
// every rule against a restatement of its own — the float -> integer casts by "is the truncated value representable" in 80-bit long double,
// the integer -> float casts by a hand-made round-half-even, the parsers by tables of edge strings and glibc's strtod, the texts by printf.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_cast.cpp && ./a.out
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "cast_parts.hpp"

using namespace nqe;
using cast::Word;

static int failures = 0;
static long checks = 0;
#define CHECK(...)                                                               \
    do {                                                                         \
        ++checks;                                                                \
        if (!(__VA_ARGS__)) {                                                          \
            if (++failures <= 40) std::printf("%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #__VA_ARGS__); \
        }                                                                        \
    } while (0)

static_assert(sizeof(long double) >= 10 && std::numeric_limits<long double>::digits >= 64, "the restatement needs a 64-bit significand");

static uint64_t bits_of(double d) { uint64_t w; std::memcpy(&w, &d, 8); return w; }
static double f64_of(uint64_t w) { double d; std::memcpy(&d, &w, 8); return d; }
static bool same(Word a, Word b) { return a.valid == b.valid && a.word == b.word; }

// ---- the restatement: Float64 -> integer is NULL iff the value truncated toward zero is not a value of the target
static Word expect_f64_to_i64(double x) {
    if (std::isnan(x) || std::isinf(x)) return {0, false};
    const long double t = std::trunc((long double)x);
    if (t < -9223372036854775808.0L || t > 9223372036854775807.0L) return {0, false};
    return {uint64_t(int64_t(t)), true};
}
static Word expect_f64_to_u64(double x) {
    if (std::isnan(x) || std::isinf(x)) return {0, false};
    const long double t = std::trunc((long double)x);
    if (t < 0.0L || t > 18446744073709551615.0L) return {0, false};
    return {uint64_t(t), true};
}
// the nearest binary64 of an unsigned integer, ties to even, by hand
static double expect_u64_to_f64(uint64_t v) {
    if (v < (1ull << 53)) return double(int64_t(v));
    int len = 64;
    while (!(v >> (len - 1))) --len;
    const int shift = len - 53;
    uint64_t q = v >> shift;
    const uint64_t rem = v & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    return std::ldexp(double(int64_t(q)), shift); // q <= 2^53: exact
}
static double expect_i64_to_f64(int64_t v) { return v < 0 ? -expect_u64_to_f64(0ull - uint64_t(v)) : expect_u64_to_f64(uint64_t(v)); }

static std::vector<double> float_edges() {
    std::vector<double> xs;
    const double inf = std::numeric_limits<double>::infinity();
    for (double b : {9223372036854775808.0, -9223372036854775808.0, 18446744073709551616.0, -1.0, 1.0, 0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, 1e15, -1e15, 9007199254740993.0, 1e19, 1e20, -1e19, 1e300, -1e300}) {
        xs.push_back(b);
        xs.push_back(std::nextafter(b, inf));
        xs.push_back(std::nextafter(b, -inf));
    }
    for (double b : {inf, -inf, std::numeric_limits<double>::quiet_NaN(), -std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min(),
                     std::numeric_limits<double>::min(), std::numeric_limits<double>::max(), std::numeric_limits<double>::lowest(), 4.9e-324, 2.2e-308})
        xs.push_back(b);
    return xs;
}

static void test_float_to_integer() {
    for (double x : float_edges()) {
        CHECK(same(cast::convert<cast::FLOAT64, cast::INT64>(bits_of(x)), expect_f64_to_i64(x)));
        CHECK(same(cast::convert<cast::FLOAT64, cast::UINT64>(bits_of(x)), expect_f64_to_u64(x)));
    }
    // the table's own words
    const double inf = std::numeric_limits<double>::infinity();
    const double two63 = 9223372036854775808.0, two64 = 18446744073709551616.0;
    CHECK(!cast::f64_to_i64(two63).valid && cast::f64_to_i64(std::nextafter(two63, 0.0)).valid && int64_t(cast::f64_to_i64(std::nextafter(two63, 0.0)).word) == INT64_MAX - 1023);
    CHECK(cast::f64_to_i64(-two63).valid && int64_t(cast::f64_to_i64(-two63).word) == INT64_MIN && !cast::f64_to_i64(std::nextafter(-two63, -inf)).valid);
    CHECK(!cast::f64_to_u64(two64).valid && cast::f64_to_u64(std::nextafter(two64, 0.0)).word == UINT64_MAX - 2047);
    CHECK(!cast::f64_to_u64(-1.0).valid && cast::f64_to_u64(std::nextafter(-1.0, 0.0)).valid && cast::f64_to_u64(std::nextafter(-1.0, 0.0)).word == 0);
    CHECK(cast::f64_to_u64(-0.5).valid && cast::f64_to_u64(-0.5).word == 0 && cast::f64_to_u64(-0.0).valid && cast::f64_to_u64(-0.0).word == 0);
    CHECK(int64_t(cast::f64_to_i64(-1.5).word) == -1 && int64_t(cast::f64_to_i64(2.5).word) == 2 && int64_t(cast::f64_to_i64(-0.5).word) == 0);
    CHECK(!cast::f64_to_i64(std::nan("")).valid && !cast::f64_to_u64(std::nan("")).valid && !cast::f64_to_i64(inf).valid && !cast::f64_to_u64(-inf).valid);
    CHECK(cast::f64_to_i64(std::nan("")).word == 0 && cast::f64_to_u64(two64).word == 0); // zeros under a NULL
}

static void test_integer_to_float_and_back() {
    std::vector<uint64_t> us = {0, 1, 2, (1ull << 53) - 1, 1ull << 53, (1ull << 53) + 1, (1ull << 53) + 2, (1ull << 53) + 3, (1ull << 54) + 2, (1ull << 54) + 6, (1ull << 63) - 1, 1ull << 63, (1ull << 63) + 1,
                                (1ull << 63) + 1024, (1ull << 63) + 1025, (1ull << 63) + 3072, UINT64_MAX, UINT64_MAX - 1};
    for (uint64_t d = 0; d <= 4200; ++d) us.push_back(UINT64_MAX - d); // the ties around 2^64 - 1024 and 2^64 - 3072, each with its neighbours
    for (uint64_t d = 0; d <= 1100; ++d) us.push_back(uint64_t(INT64_MAX) - d); // and 2^63 - 512 for Int64
    for (uint64_t v : us) {
        CHECK(same(cast::convert<cast::UINT64, cast::FLOAT64>(v), Word{bits_of(expect_u64_to_f64(v)), true}));
        CHECK(same(cast::convert<cast::INT64, cast::FLOAT64>(v), Word{bits_of(expect_i64_to_f64(int64_t(v))), true}));
        CHECK(same(cast::convert<cast::INT64, cast::FLOAT64>(0ull - v), Word{bits_of(expect_i64_to_f64(int64_t(0ull - v))), true}));
        CHECK(same(cast::convert<cast::INT64, cast::UINT64>(v), Word{int64_t(v) < 0 ? 0 : v, int64_t(v) >= 0}));
        CHECK(same(cast::convert<cast::UINT64, cast::INT64>(v), Word{v > uint64_t(INT64_MAX) ? 0 : v, v <= uint64_t(INT64_MAX)}));
    }
    CHECK(f64_of(cast::convert<cast::UINT64, cast::FLOAT64>((1ull << 53) + 1).word) == 9007199254740992.0);
    CHECK(f64_of(cast::convert<cast::UINT64, cast::FLOAT64>(UINT64_MAX).word) == 18446744073709551616.0);
    CHECK(f64_of(cast::convert<cast::UINT64, cast::FLOAT64>(UINT64_MAX - 1023).word) == 18446744073709551616.0);          // 2^64 - 1024: the tie goes to the even 2^64
    CHECK(f64_of(cast::convert<cast::UINT64, cast::FLOAT64>(UINT64_MAX - 1024).word) == 18446744073709549568.0);          // 2^64 - 1025: down to 2^64 - 2048
    CHECK(f64_of(cast::convert<cast::UINT64, cast::FLOAT64>(UINT64_MAX - 3071).word) == 18446744073709547520.0);          // 2^64 - 3072: the tie goes to the even 2^64 - 4096
    CHECK(f64_of(cast::convert<cast::INT64, cast::FLOAT64>(uint64_t(INT64_MAX)).word) == 9223372036854775808.0);
    CHECK(f64_of(cast::convert<cast::INT64, cast::FLOAT64>(uint64_t(INT64_MIN)).word) == -9223372036854775808.0);
    CHECK(same(cast::convert<cast::INT64, cast::UINT64>(uint64_t(-1)), Word{0, false}) && same(cast::convert<cast::UINT64, cast::INT64>(1ull << 63), Word{0, false}));
}

static void test_boolean() {
    for (uint64_t b : std::vector<uint64_t>{0, 1}) {
        CHECK(same(cast::convert<cast::BOOLEAN, cast::INT64>(b), Word{b, true}) && same(cast::convert<cast::BOOLEAN, cast::UINT64>(b), Word{b, true}));
        CHECK(same(cast::convert<cast::BOOLEAN, cast::FLOAT64>(b), Word{bits_of(b ? 1.0 : 0.0), true}));
    }
    for (uint64_t v : std::vector<uint64_t>{0, 1, 2, uint64_t(-1), 1ull << 63, 1ull << 32}) {
        CHECK(same(cast::convert<cast::INT64, cast::BOOLEAN>(v), Word{v != 0, true}) && same(cast::convert<cast::UINT64, cast::BOOLEAN>(v), Word{v != 0, true}));
    }
    for (double x : float_edges()) CHECK(same(cast::convert<cast::FLOAT64, cast::BOOLEAN>(bits_of(x)), Word{(x != 0.0) ? 1ull : 0ull, true}));
    CHECK(cast::convert<cast::FLOAT64, cast::BOOLEAN>(bits_of(std::nan(""))).word == 1); // NaN is true
    CHECK(cast::convert<cast::FLOAT64, cast::BOOLEAN>(bits_of(-0.0)).word == 0);         // -0.0 is false
    CHECK(cast::convert<cast::INT64, cast::BOOLEAN>(1ull << 63).word == 1);              // (not "the low bits")
}

static void test_fallible() {
    using namespace cast;
    for (int from = BOOLEAN; from <= UTF8; ++from)
        for (int to = BOOLEAN; to <= UTF8; ++to) {
            const bool expect = from != to && (from == UTF8 || (from == INT64 && to == UINT64) || (from == UINT64 && to == INT64) || (from == FLOAT64 && (to == INT64 || to == UINT64)));
            CHECK(fallible(from, to) == expect);
        }
}

template <int TO> static Word parsed(const std::string &s) { return cast::parse<TO>(s.data(), int(s.size())); }

static void test_integer_parsers() {
    struct I { const char *s; bool ok; int64_t v; };
    const I is[] = {{"0", true, 0}, {"7", true, 7}, {"-7", true, -7}, {"+7", true, 7}, {"007", true, 7}, {"-0", true, 0}, {"+0", true, 0},
                    {"9223372036854775807", true, INT64_MAX}, {"9223372036854775808", false, 0}, {"+9223372036854775807", true, INT64_MAX},
                    {"-9223372036854775808", true, INT64_MIN}, {"-9223372036854775809", false, 0}, {"00000000000000000000009223372036854775807", true, INT64_MAX},
                    {"18446744073709551615", false, 0}, {"99999999999999999999", false, 0}, {"", false, 0}, {"+", false, 0}, {"-", false, 0}, {"+-1", false, 0}, {"--1", false, 0},
                    {" 1", false, 0}, {"1 ", false, 0}, {" ", false, 0}, {"1e3", false, 0}, {"1.0", false, 0}, {"1.", false, 0}, {".1", false, 0}, {"0x10", false, 0}, {"1_000", false, 0},
                    {"12a", false, 0}, {"a12", false, 0}, {"1+", false, 0}, {"nan", false, 0}, {"true", false, 0}};
    for (const I &c : is) CHECK(same(parsed<cast::INT64>(c.s), Word{uint64_t(c.v), c.ok}));
    struct U { const char *s; bool ok; uint64_t v; };
    const U us[] = {{"0", true, 0}, {"7", true, 7}, {"+7", true, 7}, {"007", true, 7}, {"+0", true, 0}, {"-0", false, 0}, {"-7", false, 0}, {"-", false, 0}, {"+", false, 0}, {"", false, 0},
                    {"18446744073709551615", true, UINT64_MAX}, {"18446744073709551616", false, 0}, {"+18446744073709551615", true, UINT64_MAX}, {"18446744073709551620", false, 0},
                    {"28446744073709551615", false, 0}, {"184467440737095516150", false, 0}, {"000000000018446744073709551615", true, UINT64_MAX}, {"9223372036854775808", true, 1ull << 63},
                    {"99999999999999999999", false, 0}, {"++1", false, 0}, {"+-1", false, 0}, {" 1", false, 0}, {"1 ", false, 0}, {"1e3", false, 0}, {"1.0", false, 0}, {"1-", false, 0}, {"12a", false, 0}};
    for (const U &c : us) CHECK(same(parsed<cast::UINT64>(c.s), Word{c.v, c.ok}));
    // a string with a NUL inside is bytes like any other
    CHECK(!parsed<cast::INT64>(std::string("1\0" "2", 3)).valid && !parsed<cast::UINT64>(std::string("1\0", 2)).valid);
    // every power of ten and its neighbours, both parsers against printf
    uint64_t p = 1;
    for (int k = 0; k < 20; ++k, p *= 10)
        for (uint64_t v : {p - 1, p, p + 1}) {
            char buf[32];
            std::snprintf(buf, sizeof buf, "%" PRIu64, v);
            CHECK(same(parsed<cast::UINT64>(buf), Word{v, true}));
            CHECK(same(parsed<cast::INT64>(buf), Word{v <= uint64_t(INT64_MAX) ? v : 0, v <= uint64_t(INT64_MAX)}));
        }
}

static void test_bool_and_float_parsers() {
    for (const char *s : {"true", "TRUE", "True", "tRuE"}) CHECK(same(parsed<cast::BOOLEAN>(s), Word{1, true}));
    for (const char *s : {"false", "FALSE", "False"}) CHECK(same(parsed<cast::BOOLEAN>(s), Word{0, true}));
    for (const char *s : {"", "1", "0", "t", "f", "yes", "no", " true", "true ", "truee", "fals"}) CHECK(same(parsed<cast::BOOLEAN>(s), Word{0, false}));
    std::vector<std::string> good = {"0", "-0", "0.0", "-0.0", "1", "1.5", "-1.5", "+1.5", "1.", ".5", "-.5", "1e3", "1E3", "1e+3", "1e-3", "1.25e2", "123456789012345678", "1234567890123456789",
                                     "12345678901234567890", "9007199254740993", "9007199254740992.5", "9007199254740993.0000000000000000000001", "0.1", "0.2", "0.3", "1e22", "1e23", "8.5e22",
                                     "1e308", "1.7976931348623157e308", "1.7976931348623159e308", "1e309", "-1e309", "2.2250738585072014e-308", "2.2250738585072011e-308", "4.9e-324", "2.4703282292062327e-324",
                                     "2.4703282292062328e-324", "1e-400", "0e999999", "1e400", "123456789.123456789e-5", "00001.5000", "9223372036854775807", "9223372036854775808", "18446744073709551615", "18446744073709551616"};
    std::string forty = "1234567890123456789012345678901234567890", four_hundred;
    for (int k = 0; k < 400; ++k) four_hundred += char('1' + (k * 7) % 9);
    good.push_back(forty);
    good.push_back("0." + forty);
    good.push_back(forty + "e-20");
    good.push_back(four_hundred);
    good.push_back("0." + four_hundred);
    good.push_back(four_hundred.substr(0, 200) + "." + four_hundred.substr(200));
    good.push_back(four_hundred + "e-391");
    good.push_back("9007199254740993" + std::string(384, '0') + "e-384");            // a tie at 400 digits: to even
    good.push_back("9007199254740993" + std::string(383, '0') + "1e-384");           // one digit past the tie: up
    for (const std::string &s : good) {
        const double ref = std::strtod(s.c_str(), nullptr);
        const Word w = parsed<cast::FLOAT64>(s);
        CHECK(w.valid && w.word == bits_of(ref));
    }
    for (const char *s : {"nan", "NaN", "NAN", "+nan", "-nan"}) CHECK(parsed<cast::FLOAT64>(s).valid && std::isnan(f64_of(parsed<cast::FLOAT64>(s).word)));
    for (const char *s : {"inf", "Inf", "INF", "+inf", "infinity", "Infinity", "+INFINITY"}) CHECK(same(parsed<cast::FLOAT64>(s), Word{bits_of(std::numeric_limits<double>::infinity()), true}));
    for (const char *s : {"-inf", "-Infinity"}) CHECK(same(parsed<cast::FLOAT64>(s), Word{bits_of(-std::numeric_limits<double>::infinity()), true}));
    for (const char *s : {"", " ", "+", "-", ".", "e", "e5", "1e", "1e+", "1e-", ".e1", "1.2.3", "1..", " 1.5", "1.5 ", "1,5", "1.5f", "0x1p3", "infinit", "in", "nanx", "na", "--1", "+-1", "1e5.5", "1 e5", "abc", "1d3"})
        CHECK(same(parsed<cast::FLOAT64>(s), Word{0, false}));
}

static void test_texts() {
    // every digit count from 1 to 20: 10^(k-1) is the first value of k digits, 10^k - 1 the last
    uint64_t p = 1;
    for (int k = 1; k <= 20; ++k) {
        CHECK(cast::digit_count(p) == k);
        CHECK(cast::digit_count(p + (p > 1 ? 1 : 0)) == k);
        const uint64_t last = k < 20 ? p * 10 - 1 : UINT64_MAX;
        CHECK(cast::digit_count(last) == k);
        if (k < 20) p *= 10;
    }
    CHECK(cast::digit_count(0) == 1 && cast::digit_count(9) == 1 && cast::digit_count(UINT64_MAX) == 20 && cast::MAX_TEXT == 20);
    std::vector<uint64_t> vs = {0, 1, 9, 10, 11, 99, 100, 12345678, 123456789, 1234567890123456ull, 12345678901234567ull, uint64_t(INT64_MAX), uint64_t(INT64_MIN), uint64_t(INT64_MIN) + 1, UINT64_MAX, UINT64_MAX - 1,
                                uint64_t(-1), uint64_t(-9), uint64_t(-10), uint64_t(-1234567), uint64_t(-12345678), uint64_t(-123456789012345ll), uint64_t(-1234567890123456ll)};
    p = 1;
    for (int k = 0; k < 20; ++k, p *= 10)
        for (uint64_t v : std::vector<uint64_t>{p - 1, p, p + 1, 0 - p, 0 - (p - 1), 0 - (p + 1)}) vs.push_back(v);
    for (uint64_t v : vs) {
        char ref[32], got[32];
        int n = std::snprintf(ref, sizeof ref, "%" PRId64, int64_t(v));
        cast::Text t = cast::text_of<cast::INT64>(v);
        CHECK(t.len == n && cast::text_length<cast::INT64>(v) == n && cast::write_text(t, got) == n && std::string(got, size_t(n)) == std::string(ref, size_t(n)));
        n = std::snprintf(ref, sizeof ref, "%" PRIu64, v);
        t = cast::text_of<cast::UINT64>(v);
        CHECK(t.len == n && cast::text_length<cast::UINT64>(v) == n && cast::write_text(t, got) == n && std::string(got, size_t(n)) == std::string(ref, size_t(n)));
        // and back
        CHECK(same(cast::parse<cast::UINT64>(got, n), Word{v, true}));
    }
    CHECK(cast::text_length<cast::INT64>(uint64_t(INT64_MIN)) == 20);
    char got[8];
    CHECK(cast::write_text(cast::text_of<cast::BOOLEAN>(1), got) == 4 && std::string(got, 4) == "true");
    CHECK(cast::write_text(cast::text_of<cast::BOOLEAN>(0), got) == 5 && std::string(got, 5) == "false");
}

int main() {
    test_float_to_integer();
    test_integer_to_float_and_back();
    test_boolean();
    test_fallible();
    test_integer_parsers();
    test_bool_and_float_parsers();
    test_texts();
    if (failures) {
        std::printf("%d failure(s) of %ld checks\n", failures, checks);
        return 1;
    }
    std::printf("cast ok: %ld checks\n", checks);
    return 0;
}
