// The host analysis of DISTINCT and the set operators (csrc/set_ops_plan.hpp, quirk Q24) on the CPU: this file includes that header
// alone.  The argument checks in their order, the capacity rule, the canonical words, the NULL tag, the instantiation choice.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "set_ops_plan.hpp"

using namespace nqe;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static int code_of(const std::function<void()> &f) {
    try {
        f();
    } catch (const Error &e) {
        return e.code;
    }
    return NQE_OK;
}

static uint64_t bits_of(double d) {
    uint64_t w;
    std::memcpy(&w, &d, 8);
    return w;
}

int main() {
    const int five[5] = {NQE_INT64, NQE_UINT64, NQE_FLOAT64, NQE_BOOLEAN, NQE_UTF8};
    const int32_t k01[2] = {0, 1}, k00[2] = {0, 0}, k05[2] = {0, 5}, kneg[1] = {-1};

    // ---- nqe_distinct_execute: the checks in their order
    auto distinct = [&](bool ctx, bool in, bool out, const int *dt, int32_t nc, int64_t rows, const int32_t *cols, int32_t num) {
        return code_of([&] { setop::plan_distinct(ctx, in, out, dt, nc, rows, cols, num); });
    };
    CHECK(distinct(true, true, true, five, 5, 10, k01, 2) == NQE_OK);
    CHECK(distinct(false, true, true, five, 5, 10, k01, 2) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(distinct(true, false, true, five, 5, 10, k01, 2) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(distinct(true, true, false, five, 5, 10, k01, 2) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(distinct(true, true, true, five, 5, 10, nullptr, 2) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(distinct(true, true, true, five, 5, 10, nullptr, 40) == NQE_ERR_INVALID_ARGUMENT); // (1) before (3)
    CHECK(distinct(true, true, true, five, 5, 10, k01, -1) == NQE_ERR_NOT_SUPPORTED);
    CHECK(distinct(true, true, true, five, 5, 10, nullptr, -1) == NQE_ERR_NOT_SUPPORTED);
    CHECK(distinct(true, true, true, five, 5, 10, k05, 2) == NQE_ERR_NOT_SUPPORTED);
    CHECK(distinct(true, true, true, five, 5, 10, kneg, 1) == NQE_ERR_NOT_SUPPORTED);
    CHECK(distinct(true, true, true, five, 5, 10, k00, 2) == NQE_ERR_NOT_SUPPORTED);
    {
        std::vector<int> wide(40, NQE_INT64);
        std::vector<int32_t> all(40);
        for (int i = 0; i < 40; ++i) all[size_t(i)] = i;
        CHECK(distinct(true, true, true, wide.data(), 40, 10, all.data(), 33) == NQE_ERR_NOT_SUPPORTED);
        CHECK(distinct(true, true, true, wide.data(), 40, 10, all.data(), 32) == NQE_OK);
        CHECK(distinct(true, true, true, wide.data(), 40, 10, nullptr, 0) == NQE_ERR_NOT_SUPPORTED); // every column: 40 keys
        CHECK(distinct(true, true, true, wide.data(), 32, 10, nullptr, 0) == NQE_OK);
    }
    CHECK(distinct(true, true, true, five, 5, (int64_t(1) << 31) - 1, k01, 2) == NQE_OK);
    CHECK(distinct(true, true, true, five, 5, int64_t(1) << 31, k01, 2) == NQE_ERR_NOT_SUPPORTED);
    CHECK(distinct(true, true, true, five, 5, int64_t(1) << 31, k05, 2) == NQE_ERR_NOT_SUPPORTED);
    CHECK(distinct(true, true, true, five, 0, 0, nullptr, 0) == NQE_ERR_PLAN); // zero columns with zero keys
    CHECK(distinct(true, true, true, five, 5, 10, k01, 0) == NQE_ERR_PLAN);    // an empty key list that is not "every column"
    {
        const std::vector<int32_t> all = setop::plan_distinct(true, true, true, five, 5, 0, nullptr, 0);
        CHECK(all.size() == 5 && all[0] == 0 && all[4] == 4);
        const int null_typed[2] = {NQE_INT64, NQE_NULLTYPE};
        CHECK(distinct(true, true, true, null_typed, 2, 10, k01, 2) == NQE_ERR_NOT_SUPPORTED);
        CHECK(distinct(true, true, true, null_typed, 2, 10, k01, 1) == NQE_OK); // a payload column may be anything
    }

    // ---- nqe_set_op_execute
    auto set_op = [&](bool ctx, bool l, bool r, bool out, int32_t op, const int *ld, int32_t lc, int64_t lr, const int *rd, int32_t rc, int64_t rr) {
        return code_of([&] { setop::plan_set_op(ctx, l, r, out, op, ld, lc, lr, rd, rc, rr); });
    };
    const int other[5] = {NQE_INT64, NQE_INT64, NQE_FLOAT64, NQE_UTF8, NQE_UTF8};
    CHECK(set_op(true, true, true, true, NQE_SET_UNION, five, 5, 3, five, 5, 4) == NQE_OK);
    CHECK(set_op(false, true, true, true, NQE_SET_UNION, five, 5, 3, five, 5, 4) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(set_op(true, false, true, true, NQE_SET_UNION, five, 5, 3, five, 5, 4) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(set_op(true, true, false, true, NQE_SET_UNION, five, 5, 3, five, 5, 4) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(set_op(true, true, true, false, NQE_SET_UNION, five, 5, 3, five, 5, 4) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(set_op(true, true, true, true, 3, five, 5, 3, five, 5, 4) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(set_op(true, true, true, true, -1, five, 5, 3, five, 4, 4) == NQE_ERR_INVALID_ARGUMENT); // (1) before (2)
    CHECK(set_op(true, true, true, true, NQE_SET_EXCEPT, five, 5, 3, five, 4, 4) == NQE_ERR_PLAN);
    CHECK(set_op(true, true, true, true, NQE_SET_EXCEPT, five, 5, 3, other, 5, 4) == NQE_ERR_PLAN);
    {
        std::string msg;
        try {
            setop::plan_set_op(true, true, true, true, NQE_SET_UNION, five, 5, 3, other, 5, 4);
        } catch (const Error &e) {
            msg = e.msg;
        }
        CHECK(msg.find("column 1 ") != std::string::npos); // the FIRST differing dtype in column order
        std::vector<int> wide(33, NQE_INT64), wide2(33, NQE_INT64);
        wide2[32] = NQE_UTF8;
        CHECK(set_op(true, true, true, true, NQE_SET_UNION, wide.data(), 33, 3, wide.data(), 33, 4) == NQE_ERR_NOT_SUPPORTED);
        CHECK(set_op(true, true, true, true, NQE_SET_UNION, wide.data(), 33, 3, wide2.data(), 33, 4) == NQE_ERR_PLAN); // (2) before (3)
        CHECK(set_op(true, true, true, true, NQE_SET_UNION, wide.data(), 33, int64_t(1) << 31, wide.data(), 33, 4) == NQE_ERR_NOT_SUPPORTED);
    }
    CHECK(set_op(true, true, true, true, NQE_SET_INTERSECT, five, 0, 0, five, 0, 0) == NQE_ERR_PLAN);
    const int64_t big = int64_t(1) << 31;
    CHECK(set_op(true, true, true, true, NQE_SET_INTERSECT, five, 5, big, five, 5, 1) == NQE_ERR_NOT_SUPPORTED);
    CHECK(set_op(true, true, true, true, NQE_SET_INTERSECT, five, 5, big - 1, five, 5, big * 4) == NQE_OK); // the probed side has no limit
    CHECK(set_op(true, true, true, true, NQE_SET_EXCEPT, five, 5, 1, five, 5, big) == NQE_OK);
    CHECK(set_op(true, true, true, true, NQE_SET_UNION, five, 5, big / 2, five, 5, big / 2) == NQE_ERR_NOT_SUPPORTED); // UNION inserts both
    CHECK(set_op(true, true, true, true, NQE_SET_UNION, five, 5, big / 2, five, 5, big / 2 - 1) == NQE_OK);

    // ---- the capacity rule: the power of two >= 2 n (at least 2), and the shift that takes the top log2(cap) bits
    CHECK(setop::table_capacity(0) == 2 && setop::table_capacity(1) == 2 && setop::table_capacity(2) == 4 && setop::table_capacity(3) == 8);
    for (int k = 1; k < 31; ++k) {
        const int64_t n = int64_t(1) << k;
        CHECK(setop::table_capacity(n) == uint64_t(2 * n));
        CHECK(setop::table_capacity(n + 1) == uint64_t(4 * n));
        CHECK(setop::table_capacity(n - 1) == uint64_t(n == 2 ? 2 : 2 * n));
    }
    CHECK(setop::table_capacity(64) == 128 && setop::table_shift(128) == 57 && setop::table_shift(2) == 63);
    CHECK(setop::table_capacity(big - 1) == uint64_t(1) << 32 && setop::table_shift(uint64_t(1) << 32) == 32);
    for (uint64_t h : {uint64_t(0), ~uint64_t(0), uint64_t(0x123456789abcdefull)}) CHECK(setop::home_slot(h, setop::table_shift(128)) < 128);

    // ---- more than 2^30 rows: cap is 2^32, the mask is all ones and EVERY u32 is a slot index — the bit pattern of EMPTY included, so
    // the kernels report "found" apart from the slot and keep no sentinel among slot indices (EMPTY marks ROW values, rows < 2^31)
    {
        const uint64_t cap = setop::table_capacity((int64_t(1) << 30) + 1);
        CHECK(cap == uint64_t(1) << 32 && uint32_t(cap - 1) == 0xFFFFFFFFu && setop::table_shift(cap) == 32);
        uint64_t inv = setop::GOLD; // the inverse of GOLD modulo 2^64 (Newton: the correct bits double per step)
        for (int i = 0; i < 6; ++i) inv *= 2 - setop::GOLD * inv;
        CHECK(setop::GOLD * inv == 1);
        CHECK(setop::home_slot(0xFFFFFFFF00000000ull * inv, 32) == 0xFFFFFFFFu); // reachable, and equal to EMPTY's pattern
        CHECK(setop::home_slot(0xFFFFFFFF00000000ull * inv, 32) == setop::EMPTY);
        CHECK(setop::home_slot(0, 32) == 0 && setop::home_slot(0x0000000100000000ull * inv, 32) == 1);
        CHECK(((0xFFFFFFFFu + 1u) & uint32_t(cap - 1)) == 0u); // the probe wraps from the last slot to slot 0
        CHECK(setop::MAX_INSERT_ROWS - 1 < int64_t(setop::EMPTY)); // every row index is below EMPTY: `first` and the representative keep their sentinel
        CHECK(setop::table_capacity(int64_t(1) << 30) == uint64_t(1) << 31 && setop::table_shift(uint64_t(1) << 31) == 33);
        for (uint64_t h : {uint64_t(0), ~uint64_t(0), uint64_t(0x123456789abcdefull)}) CHECK(uint64_t(setop::home_slot(h, 33)) < (uint64_t(1) << 31));
    }

    // ---- canonical words
    CHECK(setop::canonical_f64(bits_of(-0.0)) == setop::canonical_f64(bits_of(0.0)));
    CHECK(setop::canonical_f64(bits_of(0.0)) == 0);
    const uint64_t nans[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xfff0000000000001ull, 0x7fffffffffffffffull, 0xffffffffffffffffull, 0x7ff8000000001234ull};
    for (uint64_t w : nans) CHECK(setop::canonical_f64(w) == setop::CANON_NAN);
    for (double d : {1.5, -1.5, 5e-324, -5e-324, std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), 1.7976931348623157e308})
        CHECK(setop::canonical_f64(bits_of(d)) == bits_of(d)); // every other value keeps its word: +inf and -inf are not NaN
    CHECK(setop::canonical_f64(bits_of(std::numeric_limits<double>::infinity())) != setop::CANON_NAN);

    // ---- the NULL tag is not what 0 or "" feed the hash; the hash is mixed per key
    const uint8_t none[1] = {0};
    CHECK(setop::NULL_TAG != 0 && setop::NULL_TAG != setop::fnv1a64_bytes(none, 0));
    CHECK(setop::hash_step(setop::hash_start(), setop::NULL_TAG) != setop::hash_step(setop::hash_start(), 0));
    CHECK(setop::hash_step(setop::hash_start(), setop::NULL_TAG) != setop::hash_step(setop::hash_start(), setop::fnv1a64_bytes(none, 0)));
    CHECK(setop::hash_step(setop::hash_step(setop::hash_start(), 1), 2) != setop::hash_step(setop::hash_step(setop::hash_start(), 2), 1));
    const uint8_t text[] = "abcdefghijklmnopq";
    CHECK(setop::fnv1a64_bytes(text, 8) != setop::fnv1a64_bytes(text, 9) && setop::fnv1a64_bytes(text, 16) != setop::fnv1a64_bytes(text, 17));
    CHECK(setop::fnv1a64_bytes(text, 3) == setop::fnv1a64_bytes(text, 3) && setop::fnv1a64_bytes(text, 0) == setop::fnv1a64_bytes(text + 5, 0));
    CHECK(setop::bytes_same(text, text, 17) && !setop::bytes_same(text, text + 1, 9) && setop::bytes_same(text, text + 3, 0));

    // ---- the instantiation: WORDS<K> for 1..4 non-nullable Int64 / UInt64 keys, GENERAL for everything else
    {
        const int dt[7] = {NQE_INT64, NQE_UINT64, NQE_INT64, NQE_UINT64, NQE_INT64, NQE_FLOAT64, NQE_INT64};
        const bool nullable[7] = {false, false, false, false, false, false, true};
        const int32_t keys[5] = {0, 1, 2, 3, 4}, with_float[2] = {0, 5}, with_nullable[2] = {6, 0}, one_nullable[1] = {6};
        for (int k = 1; k <= 4; ++k) {
            const setop::Instance i = setop::choose_instance(dt, nullable, keys, k);
            CHECK(i.form == setop::FORM_WORDS && i.k == k);
        }
        CHECK(setop::choose_instance(dt, nullable, keys, 5).form == setop::FORM_GENERAL);
        CHECK(setop::choose_instance(dt, nullable, with_float, 2).form == setop::FORM_GENERAL);
        CHECK(setop::choose_instance(dt, nullable, with_nullable, 2).form == setop::FORM_GENERAL);
        CHECK(setop::choose_instance(dt, nullable, one_nullable, 1).form == setop::FORM_GENERAL);
        CHECK(setop::choose_instance(dt, nullable, keys, 0).form == setop::FORM_GENERAL);
    }

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("set ops plan ok\n");
    return 0;
}
