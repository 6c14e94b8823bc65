// aggregate_partition_layout.hpp — the dynamic-LDS layouts of the partitioned aggregate's kernels (aggregate_partition.hip), each
// described ONCE: the kernel carves its `smem` through the description, the host (aggregate.hip) passes its bytes() to the launch.
// Plain C++17 without any other header of the project (tests/cpp/test_partition_layout.cpp includes this file alone); every member
// is constexpr, so the same text serves host and device code.  Offsets are in bytes from the start of `smem` (16-byte aligned).
#pragma once
#include <cstddef>
#include <cstdint>

namespace nqe {
namespace agg {

struct LdsField {
    size_t offset, bytes, align; // align: what the widest access to the field needs
};

// agg_partition_scatter_kernel: the tile's keys and values by partition, then per partition the workgroup's global write cursor, the
// tile's tuple count and its exclusive scan.  `parts`: counters per array (PARTS)
struct ExactScatterLayout {
    size_t rows, nv, parts;
    constexpr ExactScatterLayout(int rows_per_tile, int value_columns, int parts_) : rows(size_t(rows_per_tile)), nv(size_t(value_columns)), parts(size_t(parts_)) {}
    static constexpr int rows_per_thread(int value_columns) { return value_columns == 1 ? 8 : 4; } // 8192 (one value column) / 4096 (two) rows per tile
    constexpr size_t skey() const { return 0; }                        // uint64 [rows]
    constexpr size_t sval() const { return rows * 8; }                 // uint64 [nv][rows]
    constexpr size_t gcur() const { return sval() + nv * rows * 8; }   // uint64 [parts]
    constexpr size_t tcnt() const { return gcur() + parts * 8; }       // uint32 [parts]
    constexpr size_t tstart() const { return tcnt() + parts * 4; }     // uint32 [parts]
    constexpr size_t bytes() const { return tstart() + parts * 4; }
    static constexpr int NFIELDS = 5;
    constexpr LdsField field(int i) const {
        return i == 0 ? LdsField{skey(), rows * 8, 8} : i == 1 ? LdsField{sval(), nv * rows * 8, 8} : i == 2 ? LdsField{gcur(), parts * 8, 8}
             : i == 3 ? LdsField{tcnt(), parts * 4, 4} : LdsField{tstart(), parts * 4, 4};
    }
};

// agg_subpartition_kernel: the stage alone (its SUB counters are static LDS)
struct SubStageLayout {
    size_t rows, nv;
    constexpr SubStageLayout(int rows_per_tile, int value_columns) : rows(size_t(rows_per_tile)), nv(size_t(value_columns)) {}
    constexpr size_t skey() const { return 0; }          // uint64 [rows]
    constexpr size_t sval() const { return rows * 8; }   // uint64 [nv][rows]
    constexpr size_t bytes() const { return sval() + nv * rows * 8; }
    static constexpr int NFIELDS = 2;
    constexpr LdsField field(int i) const { return i == 0 ? LdsField{skey(), rows * 8, 8} : LdsField{sval(), nv * rows * 8, 8}; }
};

// agg_slab_scatter_kernel: the tile's tuples of (1 + nv) words by partition (16-byte tuples move as one 128-bit access), then per
// partition the tuples this workgroup has written, the tile's count and its exclusive scan
struct SlabScatterLayout {
    size_t rows, tw, parts;
    constexpr SlabScatterLayout(int rows_per_tile, int value_columns, int parts_) : rows(size_t(rows_per_tile)), tw(size_t(1 + value_columns)), parts(size_t(parts_)) {}
    constexpr size_t stup() const { return 0; }                      // uint64 [rows][tw]
    constexpr size_t gcur() const { return rows * tw * 8; }          // uint32 [parts]
    constexpr size_t tcnt() const { return gcur() + parts * 4; }     // uint32 [parts]
    constexpr size_t tstart() const { return tcnt() + parts * 4; }   // uint32 [parts]
    constexpr size_t bytes() const { return tstart() + parts * 4; }
    static constexpr int NFIELDS = 4;
    constexpr LdsField field(int i) const {
        return i == 0 ? LdsField{stup(), rows * tw * 8, 16} : i == 1 ? LdsField{gcur(), parts * 4, 4} : i == 2 ? LdsField{tcnt(), parts * 4, 4}
                                                                                                        : LdsField{tstart(), parts * 4, 4};
    }
};

// agg_slab_scatter_soa_kernel: stage [rows] and carry [parts x block] of values, the same of 32-bit keys — each carry buffer RIGHT BEHIND
// its stage (the kernel addresses both through one index) —, five counters per partition, the owner map of the blocks a tile completes.
// The layout follows the partition count of the run.
struct SoaScatterLayout {
    size_t rows, parts, carry;
    constexpr SoaScatterLayout(int rows_per_tile, int parts_log2) : rows(size_t(rows_per_tile)), parts(size_t(1) << parts_log2), carry((size_t(1) << parts_log2) << block_log2(parts_log2)) {}
    static constexpr int block_log2(int parts_log2) { return parts_log2 <= 8 ? 4 : 3; } // tuples per block: 16 (8 with 512 partitions)
    constexpr size_t sval() const { return 0; }                        // uint64 [rows]
    constexpr size_t cval() const { return rows * 8; }                 // uint64 [carry]
    constexpr size_t skey() const { return cval() + carry * 8; }       // uint32 [rows]
    constexpr size_t ckey() const { return skey() + rows * 4; }        // uint32 [carry]
    constexpr size_t gblk() const { return ckey() + carry * 4; }       // uint32 [parts] blocks this workgroup has written
    constexpr size_t ccnt() const { return gblk() + parts * 4; }       // uint32 [parts] tuples in the carry buffer
    constexpr size_t tcnt() const { return ccnt() + parts * 4; }       // uint32 [parts] tuples of this tile
    constexpr size_t tstart() const { return tcnt() + parts * 4; }     // uint32 [parts] exclusive scan of tcnt
    constexpr size_t bstart() const { return tstart() + parts * 4; }   // uint32 [parts] exclusive scan of the blocks this tile completes
    constexpr size_t bown() const { return bstart() + parts * 4; }     // uint16 [rows / 8 + parts] partition of each such block
    constexpr size_t bown_entries() const { return rows / 8 + parts; }
    constexpr size_t bytes() const { return bown() + bown_entries() * 2 + 16; }
    static constexpr int NFIELDS = 10;
    constexpr LdsField field(int i) const {
        return i == 0 ? LdsField{sval(), rows * 8, 8} : i == 1 ? LdsField{cval(), carry * 8, 8} : i == 2 ? LdsField{skey(), rows * 4, 4}
             : i == 3 ? LdsField{ckey(), carry * 4, 4} : i == 4 ? LdsField{gblk(), parts * 4, 4} : i == 5 ? LdsField{ccnt(), parts * 4, 4}
             : i == 6 ? LdsField{tcnt(), parts * 4, 4} : i == 7 ? LdsField{tstart(), parts * 4, 4} : i == 8 ? LdsField{bstart(), parts * 4, 4}
                                                                                                         : LdsField{bown(), bown_entries() * 2, 2};
    }
};

// agg_slab_segments_direct_kernel, agg_range_segments_kernel: the table of one key-range partition, addressed by (key - range_min) >>
// parts_log2 — sums, mins and maxs as doubles, counts (NaN mark in the top bit): 28 bytes per slot
struct RangeTableLayout {
    size_t slots;
    constexpr explicit RangeTableLayout(uint32_t slots_) : slots(slots_) {}
    constexpr size_t lsum() const { return 0; }            // double [slots]
    constexpr size_t lmn() const { return slots * 8; }     // double [slots]
    constexpr size_t lmx() const { return slots * 16; }    // double [slots]
    constexpr size_t lcnt() const { return slots * 24; }   // uint32 [slots]
    constexpr size_t bytes() const { return lcnt() + slots * 4 + 16; }
    static constexpr int NFIELDS = 4;
    constexpr LdsField field(int i) const {
        return i == 0 ? LdsField{lsum(), slots * 8, 8} : i == 1 ? LdsField{lmn(), slots * 8, 8} : i == 2 ? LdsField{lmx(), slots * 8, 8} : LdsField{lcnt(), slots * 4, 4};
    }
};

} // namespace agg
} // namespace nqe
