// set_ops_plan.hpp — the host analysis of DISTINCT and the set operators (quirk Q24, set_ops.hip): the argument checks in the order
// include/nqe.h states them, the capacity rule of the set table, which kernel instantiation a key list takes, and — shared with the
// kernels, which is why they are here — the canonical words the hash reads and the hash itself.
// Plain C++17, no HIP and no nqe_table: a table is seen as its column dtypes, which of them hold a NULL, and its row count, so
// tests/cpp/test_set_ops_plan.cpp compiles this header alone, and a test can construct keys that collide.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nqe.h"
#include "nqe_error.hpp"

#if defined(__HIPCC__)
#define NQE_SET_HD __host__ __device__ inline
#else
#define NQE_SET_HD inline
#endif

namespace nqe {

namespace setop {

constexpr int MAX_WORD_KEYS = 4;                          // the WORDS instantiation: 1..4 non-nullable Int64 / UInt64 keys
constexpr int64_t MAX_INSERT_ROWS = int64_t(1) << 31;     // rows of the inserted table: fewer than this (slot values are u32 rows)
constexpr uint32_t EMPTY = 0xFFFFFFFFu;                   // a slot without a representative; also "no row yet" of `first`
constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ull;
constexpr uint64_t NULL_TAG = 0x6E756C6CA5A5F00Dull;      // what a NULL feeds the hash, whatever lies under it
constexpr uint64_t CANON_NAN = 0x7FF8000000000000ull;     // the one NaN every NaN hashes and compares as

// ---- canonical words: equal under Q24's tuple equality <=> equal canonical words
NQE_SET_HD uint64_t canonical_f64(uint64_t w) {
    if ((w & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return CANON_NAN; // every NaN payload, either sign
    return w == 0x8000000000000000ull ? 0ull : w;                              // -0.0 = +0.0
}
NQE_SET_HD uint64_t load_u64_bytes(const uint8_t *p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}
NQE_SET_HD uint64_t tail_bytes(const uint8_t *p, int32_t n) { // n < 8 bytes, little-endian; nothing beyond them is read
    uint64_t w = 0;
    for (int32_t i = 0; i < n; ++i) w |= uint64_t(p[i]) << (8 * i);
    return w;
}
// utf8_bytes.hpp's fnv1a64, callable on the host as well
NQE_SET_HD uint64_t fnv1a64_bytes(const uint8_t *p, int32_t len) {
    uint64_t h = 0xcbf29ce484222325ull ^ uint64_t(uint32_t(len));
    int32_t i = 0;
    for (; i + 8 <= len; i += 8) {
        h ^= load_u64_bytes(p + i);
        h *= 0x9FB21C651E98DF25ull;
        h ^= h >> 29;
    }
    if (i < len) {
        h ^= tail_bytes(p + i, len - i);
        h *= 0x9FB21C651E98DF25ull;
        h ^= h >> 29;
    }
    return h * 0x100000001b3ull;
}
NQE_SET_HD bool bytes_same(const uint8_t *a, const uint8_t *b, int32_t len) {
    int32_t i = 0;
    for (; i + 8 <= len; i += 8)
        if (load_u64_bytes(a + i) != load_u64_bytes(b + i)) return false;
    return i == len || tail_bytes(a + i, len - i) == tail_bytes(b + i, len - i);
}

// ---- the hash: mixed per key, so that (1, 2) and (2, 1) part ways (group_keys_dict_kernel's scheme)
NQE_SET_HD uint64_t mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}
NQE_SET_HD uint64_t hash_start() { return GOLD; }
NQE_SET_HD uint64_t hash_step(uint64_t h, uint64_t canonical_word) { return mix(h ^ canonical_word); }
// the slot a probe starts at: the top log2(cap) bits
NQE_SET_HD uint32_t home_slot(uint64_t h, int shift) { return uint32_t((h * GOLD) >> shift); }

// ---- the capacity rule: the smallest power of two >= 2 n, at least 2 (n < 2^31, so cap <= 2^32 and cap - 1 is a u32 mask)
inline uint64_t table_capacity(int64_t n) {
    uint64_t cap = 2;
    while (cap < 2 * uint64_t(n)) cap <<= 1;
    return cap;
}
inline int table_shift(uint64_t cap) {
    int log2 = 0;
    while ((uint64_t(1) << log2) < cap) ++log2;
    return 64 - log2;
}

// ---- which instantiation of set_insert / set_find a key list takes
enum Form : int { FORM_GENERAL = 0, FORM_WORDS = 1 };
struct Instance {
    int form = FORM_GENERAL;
    int k = 0; // FORM_WORDS: the number of keys, 1..MAX_WORD_KEYS
};
// `nullable[c]`: column c holds at least one NULL (a validity buffer of all ones does not count)
inline Instance choose_instance(const int *dtypes, const bool *nullable, const int32_t *keys, int32_t num_keys) {
    Instance r;
    if (num_keys < 1 || num_keys > MAX_WORD_KEYS) return r;
    for (int32_t k = 0; k < num_keys; ++k) {
        const int dt = dtypes[keys[k]];
        if (!(dt == NQE_INT64 || dt == NQE_UINT64) || nullable[keys[k]]) return r;
    }
    r.form = FORM_WORDS;
    r.k = num_keys;
    return r;
}

inline bool key_dtype_ok(int dt) { return dt == NQE_BOOLEAN || dt == NQE_INT64 || dt == NQE_UINT64 || dt == NQE_FLOAT64 || dt == NQE_UTF8; }

// What nqe_distinct_execute refuses, in the order of include/nqe.h; launches and allocates nothing.  Returns the key columns
// (num_cols == 0 with cols == NULL: every column).
inline std::vector<int32_t> plan_distinct(bool ctx_ok, bool in_ok, bool out_ok, const int *dtypes, int32_t table_cols, int64_t rows, const int32_t *cols, int32_t num_cols) {
    if (!ctx_ok || !in_ok || !out_ok || (num_cols > 0 && !cols)) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    const bool all = num_cols == 0 && !cols;
    const int64_t nkeys = all ? table_cols : num_cols;
    if (num_cols < 0 || nkeys > NQE_MAX_SET_KEYS) fail(NQE_ERR_NOT_SUPPORTED, "distinct: at most " + std::to_string(NQE_MAX_SET_KEYS) + " key columns per call");
    std::vector<int32_t> keys;
    for (int32_t k = 0; k < int32_t(nkeys); ++k) {
        const int32_t c = all ? k : cols[k];
        if (c < 0 || c >= table_cols) fail(NQE_ERR_NOT_SUPPORTED, "distinct: key column index out of range");
        for (int32_t seen : keys)
            if (seen == c) fail(NQE_ERR_NOT_SUPPORTED, "distinct: key column " + std::to_string(c) + " given twice");
        keys.push_back(c);
    }
    for (int32_t c : keys)
        if (!key_dtype_ok(dtypes[c])) fail(NQE_ERR_NOT_SUPPORTED, "distinct: keys of this type are not implemented");
    if (keys.empty()) fail(NQE_ERR_PLAN, "distinct: no key columns (a table without columns, or an empty key list)");
    if (rows >= MAX_INSERT_ROWS) fail(NQE_ERR_NOT_SUPPORTED, "distinct: " + std::to_string(rows) + " rows, the set table handles fewer than 2^31");
    return keys;
}

// What nqe_set_op_execute refuses, in the order of include/nqe.h; every column is a key
inline std::vector<int32_t> plan_set_op(bool ctx_ok, bool left_ok, bool right_ok, bool out_ok, int32_t op, const int *left_dtypes, int32_t left_cols, int64_t left_rows,
                                        const int *right_dtypes, int32_t right_cols, int64_t right_rows) {
    if (!ctx_ok || !left_ok || !right_ok || !out_ok) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (op < NQE_SET_UNION || op > NQE_SET_EXCEPT) fail(NQE_ERR_INVALID_ARGUMENT, "set operation: unknown operator");
    if (left_cols != right_cols)
        fail(NQE_ERR_PLAN, "set operation: the tables have " + std::to_string(left_cols) + " and " + std::to_string(right_cols) + " columns");
    for (int32_t c = 0; c < left_cols; ++c)
        if (left_dtypes[c] != right_dtypes[c]) fail(NQE_ERR_PLAN, "set operation: column " + std::to_string(c) + " differs in type between the tables");
    if (left_cols > NQE_MAX_SET_KEYS) fail(NQE_ERR_NOT_SUPPORTED, "set operation: at most " + std::to_string(NQE_MAX_SET_KEYS) + " columns per table");
    std::vector<int32_t> keys;
    for (int32_t c = 0; c < left_cols; ++c) {
        if (!key_dtype_ok(left_dtypes[c])) fail(NQE_ERR_NOT_SUPPORTED, "set operation: columns of this type are not implemented");
        keys.push_back(c);
    }
    if (keys.empty()) fail(NQE_ERR_PLAN, "set operation: tables without columns");
    const int64_t inserted = op == NQE_SET_UNION ? left_rows + right_rows : left_rows;
    if (inserted >= MAX_INSERT_ROWS) fail(NQE_ERR_NOT_SUPPORTED, "set operation: " + std::to_string(inserted) + " rows to insert, the set table handles fewer than 2^31");
    return keys;
}

} // namespace setop

} // namespace nqe
