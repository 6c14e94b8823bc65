// The aggregate's plan memo on the CPU: aggregate_memo.hpp alone (no HIP).  tests/test_cpp_aggregate_memo.py builds and runs this.
#include "aggregate_memo.hpp"

#include <cstdio>
#include <cstdlib>

using namespace nqe;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

int main() {
    {   // a fresh key is "first execution"; a recorded "streaming" start is not; neither is a known key range
        AggMemoTable t;
        CHECK(t.find(7) == nullptr);
        AggMemo &m = t.entry(7);
        CHECK(m.first_execution());
        CHECK(m.start == AggStart::Unknown && !m.key32_failed && !m.no_three_column_pass && !m.tiny_rejected);
        m.remember_sampled_streaming();
        CHECK(m.start == AggStart::Streaming);
        CHECK(!m.first_execution());
        AggMemo &r = t.entry(8);
        r.remember_key_range(-5, 0);
        CHECK(!r.first_execution());
        // … the partition range and tiny_rejected do not count
        AggMemo &p = t.entry(9);
        p.remember_part_range(3, 40);
        p.remember_tiny_rejected();
        CHECK(p.first_execution());
        CHECK(t.size() == 3 && t.find(7) == &m);
    }
    {   // the no-overwrite write leaves an existing start (and its flags) alone
        AggMemo m;
        m.remember_start(AggStart::SlabAllParts, true);
        m.remember_sampled_streaming();
        CHECK(m.start == AggStart::SlabAllParts && m.key32_failed);
    }
    {   // a start replaces both flags: key32_failed as passed, no_three_column_pass dropped
        AggMemo m;
        m.remember_no_three_column_pass();
        CHECK(m.start == AggStart::Streaming && m.no_three_column_pass && !m.key32_failed);
        m.remember_start(AggStart::TwoSubsets, true);
        CHECK(m.start == AggStart::TwoSubsets && m.key32_failed && !m.no_three_column_pass);
        m.remember_no_three_column_pass();
        CHECK(!m.key32_failed && m.no_three_column_pass);
        m.remember_start(AggStart::ExactForm, false);
        CHECK(m.start == AggStart::ExactForm && !m.key32_failed && !m.no_three_column_pass);
    }
    {   // erasing the key range keeps the rest
        AggMemo m;
        m.remember_start(AggStart::SlabFirstParts, true);
        m.remember_key_range(-1000, 6000);
        m.remember_part_range(11, 42000);
        m.remember_tiny_rejected();
        CHECK(m.key_range_known && m.key_min == -1000 && m.key_span == 6000);
        m.forget_key_range();
        CHECK(!m.key_range_known);
        CHECK(m.start == AggStart::SlabFirstParts && m.key32_failed && m.tiny_rejected);
        CHECK(m.part_range == AggMemo::PartRange::Known && m.part_min == 11 && m.part_span == 42000);
        CHECK(!m.first_execution()); // (a start is recorded)
    }
    {   // the partition range's three states survive a round trip through the table
        AggMemoTable t;
        CHECK(t.entry(1).part_range == AggMemo::PartRange::Unknown);
        t.entry(2).remember_part_range(INT64_MIN, UINT64_MAX);
        t.entry(3).never_range_partition_again();
        CHECK(t.find(1)->part_range == AggMemo::PartRange::Unknown);
        CHECK(t.find(2)->part_range == AggMemo::PartRange::Known && t.find(2)->part_min == INT64_MIN && t.find(2)->part_span == UINT64_MAX);
        CHECK(t.find(3)->part_range == AggMemo::PartRange::Never);
        t.entry(2).never_range_partition_again();
        CHECK(t.find(2)->part_range == AggMemo::PartRange::Never);
        t.entry(3).remember_part_range(5, 6);
        CHECK(t.find(3)->part_range == AggMemo::PartRange::Known && t.find(3)->part_min == 5 && t.find(3)->part_span == 6);
    }
    {   // the 257th distinct key clears the table and the first 256 are gone; a known key at a full table clears nothing
        AggMemoTable t;
        for (uint64_t k = 1; k <= AggMemoTable::MAX_SHAPES; ++k) t.entry(k * 0x9E3779B97F4A7C15ull).remember_start(AggStart::TwoSubsets, false);
        CHECK(t.size() == 256);
        t.entry(5 * 0x9E3779B97F4A7C15ull).remember_tiny_rejected();
        CHECK(t.size() == 256 && t.find(0x9E3779B97F4A7C15ull)->start == AggStart::TwoSubsets);
        AggMemo &n = t.entry(12345);
        CHECK(n.first_execution());
        CHECK(t.size() == 1);
        for (uint64_t k = 1; k <= AggMemoTable::MAX_SHAPES; ++k) CHECK(t.find(k * 0x9E3779B97F4A7C15ull) == nullptr);
        CHECK(t.find(12345) == &n);
    }
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("aggregate memo ok");
    return 0;
}
