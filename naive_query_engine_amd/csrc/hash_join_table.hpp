// hash_join_table.hpp — the join table (nqe_join_table), the constants of its layouts and the argument blocks of the join's kernels.
// Included once, by hash_join.hip (through the two kernel headers); which build form fills which field is mapped in hash_join.hip.
#pragma once
#include "device_utils.hpp"
#include "join_keys_state.hpp"
#include "nqe_internal.hpp"

namespace nqe {

namespace {

constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ull;
constexpr int JT_ROWS = 4096; // probe tile
constexpr int JT_BLOCK = 256;
constexpr int JT_ITERS = JT_ROWS / JT_BLOCK;
constexpr int MAX_JOIN_COLS = JOIN_MAX_COLS;
constexpr int UNIQUE_MAX_PROBE = 128; // longest probe sequence of the sort-free inserts (beyond it: the sort-based build)
constexpr int PW_TILE = 1024; // probe rows per tile (= JT_ROWS / 4); tile_offsets are per JT_ROWS, so 4 sub-tiles share one base
// 16 rows per lane in flight: the kernel is bound by the latency of its gathers, and memory-level parallelism per wave
// beats occupancy (A/B on one box, C4: 4 rows/lane (70 VGPRs, 7 waves/SIMD) 1.53 ms, 8 (116, 4) 1.33 ms, 16 (210, 2)
// 1.24 ms, 32 (256, 1) 1.31 ms)
constexpr int FUSED_WRITE_ROWS = 16;
// the partitioned dense build (hash_join_build_kernels.hpp: part_build_*)
constexpr int PB_BLOCK = 1024;
constexpr int PB_MAX_PARTS = 1024;
constexpr int PB_XCDS = 8;
constexpr int PB_CHUNK = 2048;      // tuples a workgroup of the place pass takes from a partition's cursor at a time
constexpr int PB_SPLIT_TILE = 4096; // tuples per tile of the second scatter
constexpr int PB_FILL_LOG2 = 13, PB_FILL_KEYS = 1 << PB_FILL_LOG2; // keys of a fine bin: 4 + 8 bytes of LDS each
constexpr int PB_FINE_LOG2_MAX = 6;                                 // at most 64 fine bins per partition: partition = key >> (PB_FILL_LOG2 + fine_log2), fine_log2 = pb.shift - PB_FILL_LOG2 (the host picks it: see plan_partitions)
constexpr int PB_MAX_FINE = 32768;                                  // bins in all: 128 KB of LDS in the count pass (2.7 x 10^8 keys)

// Every probe sequence starts at the first slot of the key's 8-slot bucket = one 128-byte line (capacities are multiples of 64):
// inserts fill a bucket from its start, a lookup that reads the whole line has seen every candidate unless the bucket is full.
__device__ __forceinline__ uint32_t home_slot(uint64_t key, int shift) { return uint32_t((key * GOLD) >> shift) & ~7u; }

struct MinMaxCols {
    const uint64_t *src[MAX_JOIN_COLS];
    uint64_t flip[MAX_JOIN_COLS];
};
struct DensePayload {
    int32_t n;
    int32_t pad;
    const uint64_t *src[MAX_JOIN_COLS];
    void *dst[MAX_JOIN_COLS];
    uint64_t base[MAX_JOIN_COLS];
    int32_t packed[MAX_JOIN_COLS]; // 1: dst holds uint32 (value - base); 2..25: that many BITS per entry (value - base < 2^packed)
};
struct PartBuild {
    const uint64_t *keys;
    int64_t n;
    uint64_t dmin;
    int32_t shift; // partition = (key - dmin) >> shift
    int32_t parts;
    int64_t chunk; // rows per workgroup of the count / scatter passes (a multiple of the tile)
    int32_t W;     // workgroups of the count / scatter passes
    int32_t nc;    // payload words per tuple
    const uint64_t *src[MAX_JOIN_COLS];
};
// the packed form of the {key, payload} table (nqe_join_table::pp; pbits == 0: the 16-byte form)
struct PackedPairs {
    uint64_t kmin, kspan, pbase;
    uint32_t nb;   // buckets of 16 slots
    int32_t pbits; // payload bits (the low ones)
};
constexpr int PACKED_BUCKET = 16;
__device__ __forceinline__ uint32_t packed_home(uint64_t key, uint32_t nb) { return uint32_t((uint64_t(uint32_t((key * GOLD) >> 32)) * nb) >> 32); }

struct Lookup {
    const ulonglong2 *slots; // hash table (16-byte slots)
    uint32_t cap;
    int32_t shift;
    const uint32_t *dense;   // direct-address table or null
    const uint32_t *ustart;
    uint64_t dense_min, dense_span;
    int32_t direct;
    int32_t pad;
};
struct FusedCols {
    int32_t n;
    int32_t pad;
    int32_t kind[MAX_JOIN_COLS];        // 0: probe-side column (coalesced copy), 1: build key (= probe key), 2: build payload (gather),
                                        // 3: build payload packed as uint32 offsets from base[] (gather), 4: as bits[]-bit offsets
    const uint64_t *src[MAX_JOIN_COLS]; // kind 0: probe column; kind 2/3: key-ordered build column
    uint64_t *dst[MAX_JOIN_COLS];
    uint64_t base[MAX_JOIN_COLS];
    int32_t bits[MAX_JOIN_COLS]; // kind 4: bits per entry
};
// the columns of the expand-and-write pass (expand_write: probe_write_kernel / outer_write_kernel), filled from
// hash_join_expand_plan.hpp's list.  from_probe and null_word are the outer entry's: the inner instances never read them.
struct ExpandCols {
    int32_t n;
    int32_t n_left;
    int32_t need_perm; // some left column is addressed by build row (else: all by position in the sorted row list)
    int32_t pad;
    int32_t by_pos[MAX_JOIN_COLS]; // left column k: src is the `perm`-ordered copy, addressed by start + match number
    // left column k is the build key, taken from the PROBE key column at the probe row (the key of a match is bit-identical on both
    // sides: a coalesced read instead of a random gather); a NULL-extended row still gets null_word and validity 0
    int32_t from_probe[MAX_JOIN_COLS];
    int32_t dtype[MAX_JOIN_COLS];
    const void *src[MAX_JOIN_COLS];
    const uint8_t *src_valid[MAX_JOIN_COLS];
    uint64_t null_word[MAX_JOIN_COLS]; // the word a NULL-extended row holds (0; -1 for a row-number column that feeds take_utf8)
    uint64_t *dst_words[MAX_JOIN_COLS];
    uint8_t *dst_bool_bytes[MAX_JOIN_COLS];
    uint8_t *dst_valid_bytes[MAX_JOIN_COLS];
};

} // namespace

} // namespace nqe

struct nqe_join_table {
    nqe_ctx *ctx = nullptr;
    std::vector<nqe::DevColumn> left_cols; // shared buffers of the build side ("self.data")
    int64_t left_rows = 0;
    int key_dtype = NQE_INT64;
    nqe::BufRef slots; // ulonglong2[cap]
    nqe::BufRef perm;  // uint32[left_rows], build rows sorted by (key, row)
    // duplicate build keys: plain 8-byte payload columns re-laid out in `perm` order, so that the matches of one probe row — consecutive
    // entries of the sorted row list — are ADJACENT words (one line per probe row instead of two dependent random reads per
    // output row: perm[...] then the column; PMC showed 20 GB of traffic for 4.8 GB algorithmic on the 4-rows-per-key join)
    std::vector<nqe::BufRef> sorted_cols; // per left column, null where none
    uint32_t cap = 0;
    int shift = 0;
    bool direct = false; // all build keys unique: slot.y>>32 is the build row itself
    // a probe that found a key outside a gap-free build key range: later probes of this table take the two-pass form at once
    mutable bool all_match_failed = false;
    // dense build keys (max-min+1 <= 4n): direct-address table instead of hashing.
    //   unique keys:   dense[key-min] = build row + 1
    //   duplicate keys: dense[key-min] = unique-key index + 1 → (ustart[u], ustart[u+1]-ustart[u])
    // INVARIANT of `dense`, `presence` and `dense_cols`: only entries / bits at positions < dense_span are defined.  Every reader
    // tests key - dense_min < dense_span first; entries and bits at positions >= dense_span and the pad bytes behind them are never
    // read, and after the two-level partitioned build (which writes every entry itself instead of zeroing the tables) they are
    // UNDEFINED.  `presence` is sized differently by the two builds: the sort-free one allocates whole 64-entry groups
    // ((span + 63) / 64 * 8 bytes, written pairwise by dense_finish / part_build_fill), the sort-based one (span + 31) / 32 words.
    int left_key = 0;
    nqe::BufRef dense;   // uint32[span]
    nqe::BufRef ustart;  // uint32[U+1]
    uint64_t dense_min = 0, dense_span = 0; // span = number of entries (0: not dense)
    // unique + dense keys + plain 8-byte payload: payload columns re-laid out by (key - min) so that a probe
    // needs ONE random access per gathered value and no build-row lookup at all
    nqe::BufRef presence;                 // uint32 bitmap over [0, span)
    std::vector<nqe::BufRef> dense_cols;  // per left column (null for the key column)
    // Int64/UInt64 payloads whose value range fits 32 bits are stored as uint32 offsets from their minimum (frame of
    // reference): the gather target halves, so more of it stays in the 4 MB per-XCD L2 (the probe is gather-bound)
    std::vector<int> dense_packed;        // dense_cols[ci] holds value - dense_base[ci] as 1: uint32, 2..25: that many bits per entry
    std::vector<uint64_t> dense_base;
    bool dense_payload = false;
    bool dense_full = false; // every key of the dense range occurs
    // unique hashed keys whose build side has exactly one plain payload column: a second table of 16-byte slots {key, payload} — a
    // probe gets key check and payload with ONE random access (beyond the 4 MB per-XCD L2 that access IS the cost: 5.3e10/s
    // whatever the element size — tools/micro_bench.hip).  Empty slots hold `filler`, a value that is not a build key.
    nqe::BufRef slotsp;
    uint64_t filler = 0;
    int pis_col = -1; // the left column carried in the slot
    // … in 8-byte slots when key and payload fit one word together: (key - pp.kmin) << pp.pbits | (payload - pp.pbase), empty = all
    // ones (key bits + payload bits <= 63), 16-slot = 128-byte buckets, pp.nb of them (not a power of two: load ~0.6) — 10^6 keys
    // of a 2^40 domain with a 20-bit payload: 13 MB instead of 32, so more of the probe's line fetches stay in the 4 MB per-XCD L2
    nqe::PackedPairs pp{}; // pbits == 0: the 16-byte form
    // Utf8 join keys: the build strings are encoded to representative-row codes (strings.hip)
    nqe::Utf8Dict dict;
    // a join on several keys (quirk Q21, join_keys.hip): the last of left_cols is the hidden code column this table is keyed by, and
    // this is what turns a probe tuple into a code; null for a table built on one key
    std::shared_ptr<const nqe::JoinKeysState> keys;
};
