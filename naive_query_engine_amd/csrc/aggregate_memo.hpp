// aggregate_memo.hpp — what a context remembers of a grouped aggregate's query shape between executions (nqe_ctx::agg_memo, keyed by
// AggRun::hint_key: a hash of everything that decides which kernels the query takes).  Plain C++17, no HIP: tests/cpp/test_aggregate_memo.cpp
// compiles it alone.
//
// Everything here is a STARTING POINT only: every tier checks what it is given (a key outside a remembered range, an overfull table)
// and the ladder of aggregate.hip moves on from there, so a stale or lost entry costs an abandoned attempt, never a wrong result.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>

namespace nqe {

// the tier an execution starts in
enum class AggStart : uint8_t {
    Unknown,        // nothing recorded: the first execution samples the keys
    Streaming,      // one workgroup table per workgroup (recorded, so the next execution does not sample again)
    TwoSubsets,     // the streaming kernel with two key subsets
    SlabFirstParts, // partitioned, slab form, the first (smaller) partition count
    SlabAllParts,   // partitioned, slab form, PARTS partitions
    ExactForm,      // partitioned, exact form (a slab overflowed or did not fit)
};

struct AggMemo {
    AggStart start = AggStart::Unknown;
    bool key32_failed = false;         // a group key beyond int32 met the 12-byte tuples: 16-byte tuples
    bool no_three_column_pass = false; // more groups than the three-column instance's table holds: passes of one and two
    bool tiny_rejected = false;        // the register kernel met a key outside [0, m)
    // the value range of a plain integer key column (sampled or measured; span 0: wider than 2^64 - 1 values, or no rows)
    bool key_range_known = false;
    int64_t key_min = 0;
    uint64_t key_span = 0;
    // the range the key-range partitions are cut from: that of the query's groups, as a tail measured it
    enum class PartRange : uint8_t { Unknown, Never, Known }; // Never: a remembered range stopped holding, or its intervals were lopsided
    PartRange part_range = PartRange::Unknown;
    int64_t part_min = 0;
    uint64_t part_span = 0;

    // nothing that steers the start is known: the key sample runs (the partition range and tiny_rejected do not count)
    bool first_execution() const { return start == AggStart::Unknown && !key_range_known; }

    // a tier overflowed (or the key sample picked one): the next execution starts in `s`.  Replaces the start AND both flags — a site that
    // carries key32_failed over passes it, and none carries no_three_column_pass over
    void remember_start(AggStart s, bool key32) {
        start = s;
        key32_failed = key32;
        no_three_column_pass = false;
    }
    // the key sample found one workgroup table enough: recorded unless a start is already there (a later overflow overwrites it)
    void remember_sampled_streaming() {
        if (start == AggStart::Unknown) start = AggStart::Streaming;
    }
    // the three-column instance overflowed: streaming, in passes of one and two (key32_failed is not carried over)
    void remember_no_three_column_pass() {
        remember_start(AggStart::Streaming, false);
        no_three_column_pass = true;
    }
    void remember_tiny_rejected() { tiny_rejected = true; }
    void remember_key_range(int64_t min, uint64_t span) {
        key_range_known = true;
        key_min = min;
        key_span = span;
    }
    void forget_key_range() { key_range_known = false; } // (and nothing else)
    void remember_part_range(int64_t min, uint64_t span) {
        part_range = PartRange::Known;
        part_min = min;
        part_span = span;
    }
    void never_range_partition_again() { part_range = PartRange::Never; }
};

// query shape -> memo, at most MAX_SHAPES of them: a NEW shape arriving at a full table clears it first
class AggMemoTable {
public:
    static constexpr size_t MAX_SHAPES = 256;
    AggMemo *find(uint64_t shape) {
        auto it = map_.find(shape);
        return it == map_.end() ? nullptr : &it->second;
    }
    AggMemo &entry(uint64_t shape) {
        auto it = map_.find(shape);
        if (it != map_.end()) return it->second;
        if (map_.size() >= MAX_SHAPES) map_.clear();
        return map_[shape];
    }
    size_t size() const { return map_.size(); }

private:
    std::map<uint64_t, AggMemo> map_;
};

} // namespace nqe
