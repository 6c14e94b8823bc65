// The dynamic-LDS layouts of the partitioned aggregate's kernels (aggregate_partition_layout.hpp, included alone) on the CPU: for every
// shape the host can produce, the fields do not overlap and are aligned for their widest access, bytes() is what the host used to
// compute by hand (the formulas of aggregate.hip before the layouts had a description, written out below as the expectation), and the
// shapes the host launches fit the 160 KB of LDS a workgroup can have.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aggregate_partition_layout.hpp"

using namespace nqe::agg;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s: ", #cond);            \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            if (++failures > 20) std::exit(1);            \
        }                                                 \
    } while (0)

constexpr size_t LDS_PER_WORKGROUP = size_t(160) << 10;
constexpr int PARTS = 512;       // counters per array of the exact and the slab scatter (aggregate_common.hpp: PARTS)
constexpr int AGG_BLOCK = 1024;  // their workgroup size

template <class L> static void check_fields(const L &l, const char *what, long a, long b, long c) {
    std::vector<LdsField> f;
    for (int i = 0; i < L::NFIELDS; ++i) f.push_back(l.field(i));
    for (const LdsField &x : f) CHECK(x.offset % x.align == 0, "%s(%ld, %ld, %ld): offset %zu, alignment %zu", what, a, b, c, x.offset, x.align);
    std::sort(f.begin(), f.end(), [](const LdsField &x, const LdsField &y) { return x.offset < y.offset; });
    for (size_t i = 0; i + 1 < f.size(); ++i)
        CHECK(f[i].offset + f[i].bytes <= f[i + 1].offset, "%s(%ld, %ld, %ld): [%zu, +%zu) runs into %zu", what, a, b, c, f[i].offset, f[i].bytes, f[i + 1].offset);
    CHECK(f.back().offset + f.back().bytes <= l.bytes(), "%s(%ld, %ld, %ld): the last field ends at %zu, bytes() %zu", what, a, b, c, f.back().offset + f.back().bytes, l.bytes());
}

int main() {
    // ---- exact scatter and the sub-partition stage: value columns 1..2, rows per thread 4 and 8
    for (int nv = 1; nv <= 2; ++nv) {
        CHECK(ExactScatterLayout::rows_per_thread(nv) == (nv == 1 ? 8 : 4), "nv %d", nv);
        for (int rpt : {4, 8}) {
            const size_t sc_rows = size_t(AGG_BLOCK) * rpt;
            const ExactScatterLayout e(int(sc_rows), nv, PARTS);
            check_fields(e, "exact scatter", long(sc_rows), nv, PARTS);
            CHECK(e.bytes() == sc_rows * 8 * size_t(1 + nv) + size_t(PARTS) * (8 + 4 + 4), "exact scatter rows %zu nv %d: %zu", sc_rows, nv, e.bytes());
            const SubStageLayout s(int(sc_rows), nv);
            check_fields(s, "sub-partition stage", long(sc_rows), nv, 0);
            CHECK(s.bytes() == sc_rows * 8 * size_t(1 + nv), "sub-partition stage rows %zu nv %d: %zu", sc_rows, nv, s.bytes());
            if (rpt == ExactScatterLayout::rows_per_thread(nv)) { // what the host launches
                CHECK(e.bytes() <= LDS_PER_WORKGROUP, "exact scatter nv %d: %zu bytes", nv, e.bytes());
                CHECK(s.bytes() <= LDS_PER_WORKGROUP, "sub-partition stage nv %d: %zu bytes", nv, s.bytes());
            }
        }
    }
    // ---- slab scatter (16- and 24-byte tuples): the tuples are moved with 128-bit accesses, so the stage is 16-byte aligned
    for (int nv = 1; nv <= 2; ++nv)
        for (int rpt : {4, 8}) {
            const size_t tile_rows = size_t(AGG_BLOCK) * rpt, tw = size_t(1 + nv);
            const SlabScatterLayout l(int(tile_rows), nv, PARTS);
            check_fields(l, "slab scatter", long(tile_rows), nv, PARTS);
            CHECK(l.field(0).align == 16 && l.stup() % 16 == 0, "slab scatter: the tuple stage");
            CHECK(l.bytes() == tile_rows * 8 * tw + size_t(PARTS) * 12, "slab scatter rows %zu nv %d: %zu", tile_rows, nv, l.bytes());
            // (8 rows per thread only with one value column: slab_scatter_rows_per_thread, aggregate_common.hpp)
            if (rpt == 4 || nv == 1) CHECK(l.bytes() <= LDS_PER_WORKGROUP, "slab scatter rows %zu nv %d: %zu bytes", tile_rows, nv, l.bytes());
        }
    // ---- two-stream (SoA) scatter: partitions 2^4..2^9, 512 and 1024 threads, 4 and 8 rows per thread
    for (int parts_log2 = 4; parts_log2 <= 9; ++parts_log2)
        for (int threads : {512, 1024})
            for (int rpt : {4, 8}) {
                const size_t tile_rows = size_t(threads) * rpt, sparts = size_t(1) << parts_log2;
                const SoaScatterLayout l(int(tile_rows), parts_log2);
                check_fields(l, "SoA scatter", long(tile_rows), parts_log2, 0);
                CHECK(SoaScatterLayout::block_log2(parts_log2) == (parts_log2 <= 8 ? 4 : 3), "parts_log2 %d", parts_log2);
                const size_t sc_carry = sparts << (parts_log2 <= 8 ? 4 : 3);
                CHECK(l.bytes() == (tile_rows + sc_carry) * 12 + sparts * 20 + (tile_rows / 8 + sparts) * 2 + 16, "SoA scatter rows %zu parts_log2 %d: %zu", tile_rows,
                      parts_log2, l.bytes());
                // the kernel reads stage and carry through ONE index: each carry buffer starts where its stage ends
                CHECK(l.cval() == l.sval() + tile_rows * 8 && l.ckey() == l.skey() + tile_rows * 4, "SoA scatter rows %zu parts_log2 %d: carry behind stage", tile_rows, parts_log2);
                CHECK(l.bytes() <= LDS_PER_WORKGROUP, "SoA scatter rows %zu parts_log2 %d: %zu bytes", tile_rows, parts_log2, l.bytes());
            }
    // ---- key-range table: 1..5120 slots (RANGE_TIER_MAX_SLOTS)
    for (uint32_t slots = 1; slots <= 5120; ++slots) {
        const RangeTableLayout l(slots);
        check_fields(l, "range table", long(slots), 0, 0);
        CHECK(l.bytes() == size_t(28) * size_t(slots) + 16, "range table %u slots: %zu", slots, l.bytes());
        CHECK(l.bytes() <= LDS_PER_WORKGROUP, "range table %u slots: %zu bytes", slots, l.bytes());
    }
    if (failures) return 1;
    std::printf("partition layout ok\n");
    return 0;
}
