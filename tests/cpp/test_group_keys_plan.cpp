// test_group_keys_plan.cpp — the host plan of GROUP BY on several keys (naive_query_engine_amd/csrc/group_keys_plan.hpp, quirk Q20): spans,
// mixed-radix strides and the packed / dictionary decision, on the CPU.  The model is independent of the header: tuples are compared as
// tuples (signed or unsigned per key), codes as integers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "group_keys_plan.hpp"

using namespace nqe::gk;

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

static KeyRange range_i64(int64_t lo, int64_t hi) { return KeyRange{uint64_t(lo) ^ SIGN, uint64_t(hi) ^ SIGN, true}; }
static KeyRange range_u64(uint64_t lo, uint64_t hi) { return KeyRange{lo, hi, false}; }

// the model's order of two key words of one column
static int cmp_key(uint64_t a, uint64_t b, bool is_signed) {
    if (is_signed) return int64_t(a) < int64_t(b) ? -1 : int64_t(a) > int64_t(b) ? 1 : 0;
    return a < b ? -1 : a > b ? 1 : 0;
}
static int cmp_tuple(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, const std::vector<KeyRange> &r) {
    for (size_t i = 0; i < a.size(); ++i)
        if (int c = cmp_key(a[i], b[i], r[i].is_signed)) return c;
    return 0;
}

static void test_limit() {
    // a product of exactly 2^62 packs; 2^62 + 1 does not
    KeyRange a[2] = {range_i64(0, (int64_t(1) << 31) - 1), range_u64(0, (uint64_t(1) << 31) - 1)};
    PackPlan p = plan_pack(a, 2);
    CHECK(p.packed && p.total == PACK_LIMIT && p.stride[1] == 1 && p.stride[0] == (uint64_t(1) << 31) && p.span[0] == (uint64_t(1) << 31));
    KeyRange one[1] = {range_u64(5, 5 + PACK_LIMIT - 1)};
    p = plan_pack(one, 1);
    CHECK(p.packed && p.total == PACK_LIMIT && p.min[0] == 5);
    KeyRange over[2] = {range_u64(0, PACK_LIMIT), range_i64(7, 7)}; // span 2^62 + 1, times 1
    CHECK(!plan_pack(over, 2).packed);
    KeyRange over2[2] = {range_i64(0, (int64_t(1) << 31) - 1), range_u64(0, uint64_t(1) << 31)}; // 2^31 * (2^31 + 1)
    CHECK(!plan_pack(over2, 2).packed);
    // a product that would WRAP to something small: 2^33 * 2^33 = 2^66 = 4 (mod 2^64)
    KeyRange wrap[2] = {range_u64(0, (uint64_t(1) << 33) - 1), range_u64(0, (uint64_t(1) << 33) - 1)};
    CHECK(!plan_pack(wrap, 2).packed);
}

static void test_wide_and_edges() {
    KeyRange all[1] = {range_i64(INT64_MIN, INT64_MAX)}; // one key spanning all of Int64: the span does not fit a word
    CHECK(!plan_pack(all, 1).packed);
    KeyRange all2[2] = {range_i64(1, 2), range_u64(0, ~uint64_t(0))};
    CHECK(!plan_pack(all2, 2).packed);
    // UInt64 minima above 2^63, a negative Int64 minimum
    KeyRange hi[2] = {range_u64(SIGN + 10, SIGN + 13), range_i64(-5, 4)};
    PackPlan p = plan_pack(hi, 2);
    CHECK(p.packed && p.min[0] == SIGN + 10 && p.span[0] == 4 && p.min[1] == uint64_t(int64_t(-5)) && p.span[1] == 10 && p.stride[0] == 10 && p.total == 40);
    uint64_t t[2] = {SIGN + 13, uint64_t(int64_t(4))}, back[2];
    CHECK(pack_tuple(p, t) == 39);
    decode_tuple(p, 39, back);
    CHECK(back[0] == t[0] && back[1] == t[1]);
    // a range that straddles the signed / unsigned seam of its type
    KeyRange seam[2] = {range_i64(-2, 1), range_u64(SIGN - 1, SIGN + 1)};
    p = plan_pack(seam, 2);
    CHECK(p.packed && p.span[0] == 4 && p.span[1] == 3 && p.total == 12);
    // span 1 everywhere
    KeyRange ones[3] = {range_i64(7, 7), range_u64(9, 9), range_i64(INT64_MIN, INT64_MIN)};
    p = plan_pack(ones, 3);
    CHECK(p.packed && p.total == 1 && p.stride[0] == 1 && p.stride[2] == 1);
    uint64_t t3[3] = {7, 9, uint64_t(INT64_MIN)}, b3[3];
    CHECK(pack_tuple(p, t3) == 0);
    decode_tuple(p, 0, b3);
    CHECK(b3[0] == 7 && b3[1] == 9 && b3[2] == uint64_t(INT64_MIN));
    // a column without a valid row (lo > hi): any digit serves
    KeyRange none[2] = {KeyRange{~uint64_t(0), 0, true}, range_u64(3, 6)};
    p = plan_pack(none, 2);
    CHECK(p.packed && p.span[0] == 1 && p.total == 4);
    // 8 keys: 2^7 values each is 2^56, 2^8 each is 2^64
    KeyRange k8[MAX_KEYS], k8wide[MAX_KEYS];
    for (int i = 0; i < MAX_KEYS; ++i) {
        k8[i] = (i & 1) ? range_u64(100, 227) : range_i64(-64, 63);
        k8wide[i] = range_u64(0, 255);
    }
    p = plan_pack(k8, MAX_KEYS);
    CHECK(p.packed && p.total == (uint64_t(1) << 56) && p.stride[0] == (uint64_t(1) << 49) && p.stride[MAX_KEYS - 1] == 1);
    CHECK(!plan_pack(k8wide, MAX_KEYS).packed);
}

// decode(pack(t)) == t and order preservation over random tuples
static void test_round_trip(std::mt19937_64 &rng, int k) {
    std::vector<KeyRange> r(static_cast<size_t>(k));
    std::vector<uint64_t> lo(static_cast<size_t>(k)), span(static_cast<size_t>(k));
    for (int i = 0; i < k; ++i) {
        const bool sg = rng() & 1;
        span[size_t(i)] = 1 + rng() % (k <= 3 ? 1000 : 50);
        const uint64_t base = rng() % 3 == 0 ? rng() : uint64_t(int64_t(rng() % 200) - 100);
        // the smallest value in the key's own order, kept clear of the type's upper end
        uint64_t ord = (base ^ (sg ? SIGN : 0));
        if (ord > ~uint64_t(0) - span[size_t(i)]) ord -= span[size_t(i)];
        lo[size_t(i)] = ord;
        r[size_t(i)] = KeyRange{ord, ord + span[size_t(i)] - 1, sg};
    }
    const PackPlan p = plan_pack(r.data(), k);
    CHECK(p.packed);
    if (!p.packed) return;
    std::vector<std::vector<uint64_t>> tuples;
    std::vector<uint64_t> codes;
    for (int n = 0; n < 400; ++n) {
        std::vector<uint64_t> t(static_cast<size_t>(k));
        for (int i = 0; i < k; ++i) {
            const uint64_t d = n == 0 ? 0 : n == 1 ? span[size_t(i)] - 1 : rng() % span[size_t(i)];
            t[size_t(i)] = (lo[size_t(i)] + d) ^ (r[size_t(i)].is_signed ? SIGN : 0);
        }
        const uint64_t code = pack_tuple(p, t.data());
        CHECK(code < p.total);
        std::vector<uint64_t> back(static_cast<size_t>(k));
        decode_tuple(p, code, back.data());
        CHECK(back == t);
        tuples.push_back(t);
        codes.push_back(code);
    }
    CHECK(codes[0] == 0 && codes[1] == p.total - 1); // the smallest and the largest tuple
    for (size_t a = 0; a < tuples.size(); ++a)
        for (size_t b = a + 1; b < tuples.size(); b += 7) {
            const int ct = cmp_tuple(tuples[a], tuples[b], r), cc = codes[a] < codes[b] ? -1 : codes[a] > codes[b] ? 1 : 0;
            CHECK(ct == cc);
        }
}

int main() {
    test_limit();
    test_wide_and_edges();
    std::mt19937_64 rng(20);
    for (int rep = 0; rep < 40; ++rep)
        for (int k : {1, 2, 3, 8}) test_round_trip(rng, k);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("group keys plan ok\n");
    return 0;
}
