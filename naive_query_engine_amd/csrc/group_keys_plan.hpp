// group_keys_plan.hpp — GROUP BY on several keys (quirk Q20): how a tuple of integer keys becomes ONE Int64 code per row, decided on the
// host from the measured value range of every key column.  Plain C++17, no HIP: tests/cpp/test_group_keys_plan.cpp compiles it alone.
//
//   span_i   = max_i - min_i + 1 over the valid rows of key i (signed for Int64, unsigned for UInt64; the difference of the raw words is
//              the same in both orders)
//   stride_i = span_{i+1} * ... * span_{k-1}: mixed radix, key 0 most significant
//   code     = sum (key_i - min_i) * stride_i, in [0, product of the spans)
//
// Every digit preserves its key's order, so ascending code is ascending tuple order and the aggregate's sorted output needs no sort.
// The packed path is taken iff the product of the spans is at most 2^62 (the codes are non-negative Int64 with room to spare); the
// product is formed with a checked multiplication, never wrapped.  Anything else — a key spanning all of Int64, eight wide keys —
// takes the tuple dictionary (group_keys.hip).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define NQE_GK_HD __host__ __device__
#else
#define NQE_GK_HD
#endif

namespace nqe {
namespace gk {

constexpr int MAX_KEYS = 8; // NQE_MAX_GROUP_KEYS
constexpr uint64_t PACK_LIMIT = uint64_t(1) << 62;
constexpr uint64_t SIGN = uint64_t(1) << 63;

// the XOR that maps a key word to an unsigned word of the same order
inline uint64_t order_flip(bool is_signed) { return is_signed ? SIGN : 0; }

// what the ranges kernel leaves per key, as ORDER words (word ^ order_flip): lo > hi when the column has no valid row
struct KeyRange {
    uint64_t lo, hi;
    bool is_signed;
};

struct PackPlan {
    int k = 0;
    bool packed = false;     // false: the dictionary path (the fields below are then unspecified)
    uint64_t min[MAX_KEYS];  // raw key word of the smallest value
    uint64_t span[MAX_KEYS]; // >= 1
    uint64_t stride[MAX_KEYS];
    uint64_t total = 0;      // product of the spans = one past the largest code
};

// a * b <= limit, without wrapping (a, b >= 1)
inline bool mul_within(uint64_t a, uint64_t b, uint64_t limit, uint64_t *out) {
    if (a > limit / b) return false;
    *out = a * b;
    return true;
}

inline PackPlan plan_pack(const KeyRange *r, int k) {
    PackPlan p;
    p.k = k;
    for (int i = 0; i < k; ++i) {
        if (r[i].lo > r[i].hi) { // no valid row: every tuple is dropped, any digit serves
            p.min[i] = 0;
            p.span[i] = 1;
            continue;
        }
        p.min[i] = r[i].lo ^ order_flip(r[i].is_signed);
        p.span[i] = r[i].hi - r[i].lo + 1; // 0: the key spans all 2^64 values
        if (p.span[i] == 0) return p;
    }
    uint64_t prod = 1;
    for (int i = k - 1; i >= 0; --i) {
        p.stride[i] = prod;
        if (!mul_within(prod, p.span[i], PACK_LIMIT, &prod)) return p;
    }
    p.total = prod;
    p.packed = true;
    return p;
}

// the arithmetic of the pack and decode kernels (wrapping subtraction: min is the smallest key in the key's own order)
NQE_GK_HD inline uint64_t pack_digit(uint64_t key, uint64_t min, uint64_t stride) { return (key - min) * stride; }
NQE_GK_HD inline uint64_t decode_digit(uint64_t code, uint64_t min, uint64_t span, uint64_t stride) { return (code / stride) % span + min; }

inline uint64_t pack_tuple(const PackPlan &p, const uint64_t *keys) {
    uint64_t code = 0;
    for (int i = 0; i < p.k; ++i) code += pack_digit(keys[i], p.min[i], p.stride[i]);
    return code;
}
inline void decode_tuple(const PackPlan &p, uint64_t code, uint64_t *keys) {
    for (int i = 0; i < p.k; ++i) keys[i] = decode_digit(code, p.min[i], p.span[i], p.stride[i]);
}

} // namespace gk
} // namespace nqe
