// join_keys_plan.hpp — the join on several keys (quirk Q21): how a PROBE row's key tuple becomes a code in the code space the build side
// fixed (group_keys_plan.hpp: PackPlan, measured over the build key columns).  Plain C++17, no HIP: tests/cpp/test_join_keys_plan.cpp
// compiles it alone.
//
// The build codes are pack_tuple's, in [0, total) with total <= 2^62.  A probe tuple the build side has never seen must get a code that
// equals none of them: JOIN_KEYS_NO_MATCH = -1 for a tuple with a key outside its build range; a tuple inside every range gets
// pack_tuple's code, which is the code of the equal build tuple if there is one (the packing is injective on the box of the ranges).
#pragma once

#include "group_keys_plan.hpp"

namespace nqe {
namespace jk {

constexpr int MAX_KEYS = gk::MAX_KEYS; // NQE_MAX_JOIN_KEYS
constexpr int64_t JOIN_KEYS_NO_MATCH = -1;

// *digit = key - min (wrapping); true iff min <= key <= max in the key's own order, where span = max - min + 1 in [1, 2^64).
//
// Why ONE unsigned test is exact, for Int64 and UInt64 alike: x -> x - min is a bijection of the 2^64 words.  The `span` keys min,
// min + 1, ..., max are consecutive words (a range that does not wrap in the key's own order does not pass the order's break — between
// INT64_MAX and INT64_MIN, or between UINT64_MAX and 0 — so stepping by +1 on the raw words walks it), and they land on 0, 1, ...,
// span - 1.  Every other word therefore lands on a value >= span: a key below min wraps to at least 2^64 - (number of words below
// min) >= span, a key above max gives key - min > max - min.
NQE_GK_HD inline bool probe_digit_in_range(uint64_t key, uint64_t min, uint64_t span, uint64_t *digit) {
    *digit = key - min;
    return *digit < span;
}

// the code of one probe tuple under the build side's plan (what join_keys_pack_probe_kernel computes per row)
inline int64_t probe_tuple(const gk::PackPlan &p, const uint64_t *keys) {
    uint64_t code = 0;
    bool in = true;
    for (int i = 0; i < p.k; ++i) {
        uint64_t d;
        in = probe_digit_in_range(keys[i], p.min[i], p.span[i], &d) && in;
        code += d * p.stride[i];
    }
    return in ? int64_t(code) : JOIN_KEYS_NO_MATCH;
}

// the plan of an EMPTY build side: span 0 everywhere, so no digit is in range and every probe tuple is JOIN_KEYS_NO_MATCH
inline gk::PackPlan empty_build_plan(int k) {
    gk::PackPlan p;
    p.k = k;
    p.packed = true;
    for (int i = 0; i < k; ++i) p.min[i] = p.span[i] = p.stride[i] = 0;
    return p;
}

} // namespace jk
} // namespace nqe
