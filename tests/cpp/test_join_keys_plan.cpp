// test_join_keys_plan.cpp — the probe-side plan of the join on several keys (naive_query_engine_amd/csrc/join_keys_plan.hpp, quirk Q21), on
// the CPU: probe_digit_in_range against a brute-force comparison in the key's own order — Int64 and UInt64, ranges that touch INT64_MIN,
// INT64_MAX, 0 and UINT64_MAX, keys one below the minimum and one above the maximum, span 1 — and the code of a probe tuple against
// pack_tuple / JOIN_KEYS_NO_MATCH.
#include <cstdio>
#include <random>
#include <vector>

#include "join_keys_plan.hpp"

using namespace nqe::gk;
using namespace nqe::jk;

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

static KeyRange range_of(uint64_t lo, uint64_t hi, bool is_signed) { return KeyRange{lo ^ order_flip(is_signed), hi ^ order_flip(is_signed), is_signed}; }

// the model: min <= key <= max in the key's own order
static bool inside(uint64_t key, uint64_t lo, uint64_t hi, bool is_signed) {
    if (is_signed) return int64_t(lo) <= int64_t(key) && int64_t(key) <= int64_t(hi);
    return lo <= key && key <= hi;
}

// one range [lo, hi] (raw words) of one key, probed with the words around its ends, around every break of either order, and at random
static void check_range(uint64_t lo, uint64_t hi, bool is_signed, std::mt19937_64 &rng) {
    KeyRange r[1] = {range_of(lo, hi, is_signed)};
    const PackPlan p = plan_pack(r, 1);
    if (!p.packed) { // the range is all 2^64 words (or wider than 2^62): the dictionary's, not ours
        CHECK(p.span[0] == 0 || p.span[0] > PACK_LIMIT);
        return;
    }
    CHECK(p.min[0] == lo && p.span[0] == hi - lo + 1);
    std::vector<uint64_t> keys = {lo, hi, lo - 1, hi + 1, lo + 1, hi - 1, 0, 1, ~0ull, ~0ull - 1, SIGN, SIGN - 1, SIGN + 1, lo + (hi - lo) / 2};
    for (int i = 0; i < 64; ++i) keys.push_back(rng());
    for (int i = 0; i < 64; ++i) keys.push_back(lo + rng() % p.span[0]);
    for (uint64_t key : keys) {
        uint64_t d = 0;
        const bool in = probe_digit_in_range(key, p.min[0], p.span[0], &d);
        CHECK(in == inside(key, lo, hi, is_signed));
        CHECK(d == key - lo);
        const int64_t code = probe_tuple(p, &key);
        CHECK(in ? (code >= 0 && uint64_t(code) == pack_tuple(p, &key) && uint64_t(code) < p.total) : code == JOIN_KEYS_NO_MATCH);
    }
}

static void test_ranges() {
    std::mt19937_64 rng(21);
    const uint64_t I64_MIN = SIGN, I64_MAX = SIGN - 1, U64_MAX = ~0ull;
    // Int64: at the minimum, at the maximum, across zero, span 1 at every special word
    check_range(I64_MIN, I64_MIN + 9, true, rng);
    check_range(I64_MAX - 9, I64_MAX, true, rng);
    check_range(uint64_t(-5), 5, true, rng);
    check_range(uint64_t(-1), 0, true, rng);
    for (uint64_t w : {I64_MIN, I64_MAX, uint64_t(0), uint64_t(-1), uint64_t(1)}) check_range(w, w, true, rng);
    check_range(I64_MIN, I64_MIN + (PACK_LIMIT - 1), true, rng); // the widest range that packs
    check_range(I64_MIN, I64_MAX, true, rng);                     // all of Int64: not packed
    // UInt64: at 0, at the maximum, across 2^63 (where the signed order breaks), span 1
    check_range(0, 9, false, rng);
    check_range(U64_MAX - 9, U64_MAX, false, rng);
    check_range(SIGN - 5, SIGN + 5, false, rng);
    for (uint64_t w : {uint64_t(0), U64_MAX, SIGN, SIGN - 1}) check_range(w, w, false, rng);
    check_range(U64_MAX - (PACK_LIMIT - 1), U64_MAX, false, rng);
    check_range(0, U64_MAX, false, rng);
    // random ranges of random widths, both orders
    for (int t = 0; t < 2000; ++t) {
        const bool is_signed = t & 1;
        const uint64_t width = rng() >> (2 + rng() % 62); // < 2^62
        const uint64_t lo_order = width ? rng() % (U64_MAX - width + 1) : rng(), lo = lo_order ^ order_flip(is_signed);
        check_range(lo, lo + width, is_signed, rng);
    }
}

// tuples: an in-range probe tuple gets pack_tuple's code, a tuple with any key one outside its range gets JOIN_KEYS_NO_MATCH
static void test_tuples() {
    std::mt19937_64 rng(22);
    for (int t = 0; t < 500; ++t) {
        const int k = 2 + int(rng() % 7);
        KeyRange r[nqe::jk::MAX_KEYS];
        uint64_t lo[nqe::jk::MAX_KEYS], hi[nqe::jk::MAX_KEYS];
        bool sg[nqe::jk::MAX_KEYS];
        for (int i = 0; i < k; ++i) {
            sg[i] = rng() & 1;
            const uint64_t width = rng() % 100;
            const uint64_t lo_order = rng() % 3 == 0 ? (rng() & 1 ? 0 : ~0ull - width) : rng() % (~0ull - width);
            lo[i] = lo_order ^ order_flip(sg[i]);
            hi[i] = lo[i] + width;
            r[i] = range_of(lo[i], hi[i], sg[i]);
        }
        const PackPlan p = plan_pack(r, k);
        if (!p.packed) continue; // (eight keys of up to 100 values pack: 100^8 < 2^62)
        uint64_t keys[nqe::jk::MAX_KEYS];
        for (int i = 0; i < k; ++i) keys[i] = lo[i] + rng() % p.span[i];
        const int64_t code = probe_tuple(p, keys);
        CHECK(code >= 0 && uint64_t(code) == pack_tuple(p, keys) && uint64_t(code) < p.total);
        uint64_t back[nqe::jk::MAX_KEYS];
        decode_tuple(p, uint64_t(code), back);
        for (int i = 0; i < k; ++i) CHECK(back[i] == keys[i]);
        for (int i = 0; i < k; ++i)
            for (uint64_t out : {lo[i] - 1, hi[i] + 1}) {
                if (inside(out, lo[i], hi[i], sg[i])) continue; // (a range that ends at the order's end: its neighbour wrapped inside — never with width < 2^64 - 1, kept for safety)
                const uint64_t keep = keys[i];
                keys[i] = out;
                CHECK(probe_tuple(p, keys) == JOIN_KEYS_NO_MATCH);
                keys[i] = keep;
            }
    }
    // the plan of an empty build side: nothing is in range
    const PackPlan e = empty_build_plan(3);
    const uint64_t any[3] = {0, ~0ull, SIGN};
    CHECK(e.packed && probe_tuple(e, any) == JOIN_KEYS_NO_MATCH);
}

int main() {
    test_ranges();
    test_tuples();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("join keys plan ok\n");
    return 0;
}
