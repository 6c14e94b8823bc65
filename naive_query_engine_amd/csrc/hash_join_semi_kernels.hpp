// hash_join_semi_kernels.hpp — the device side of the semi and anti hash joins (quirk Q22; included once, by hash_join.hip, after
// hash_join_outer_kernels.hpp): a probe whose output per row is ONE BIT — the KEEP mask of the compaction kernels — and the pass over
// the build rows that the marks have (SEMI) or have not (ANTI) seen match.  No per-row word is written anywhere: no build row, no
// (start, count).
#pragma once
#include "hash_join_outer_kernels.hpp"

namespace nqe {

namespace {

// how semi_keep_kernel decides that a probe key has a partner
enum SemiForm {
    SEMI_RANGE = 0,  // dense_full tables: key - dense_min < dense_span, no memory access beyond the key
    SEMI_BITMAP = 1, // tables with `presence`: one bit per key of the range (a gather target 32x smaller than `dense`)
    SEMI_LOOKUP = 2, // every table: dense[d] != 0 (no ustart reads) or the hash table's probe_one; with marks, lookup_meta
};

// the validity bitmaps of the probe key columns (NQE_SEMI_NULL_KEY_UNMATCHED): null = all valid.  The bitmaps may be the caller's own
// device memory, ceil(n / 8) bytes at any alignment: a lane reads the byte of its own row (the 64 rows of a wave share 8 bytes, one
// request), never a word that could reach past the end
struct SemiValid {
    const uint8_t *v[NQE_MAX_JOIN_KEYS];
};

// One wave per 4096-row tile, eight keys per lane in flight before the first lookup (probe_unique_kernel's shape); per 64 rows one
// ballot word of the keep mask, per tile one count.
// ANTI:  keeps the rows WITHOUT a partner.  The inversion is part of the lane's own predicate, under row < n: the bits of the rows past
//        the end stay 0 (a ballot inverted afterwards would set them, and the compaction would emit rows that do not exist).
// NULLS: a row with a NULL at any key position matches nothing — its hit is cleared before the polarity applies and before any mark.
// MARKS: a hit sets bit `start` of `marks` exactly as the count pass (expand_count) does (a plain read first, then atomicOr); needs the start,
//        so it always goes through lookup_meta.
// KEEP:  off for the mark-only pass: no keep word, no count.
template <int FORM, bool ANTI, bool NULLS, bool MARKS, bool KEEP>
__global__ void __launch_bounds__(256) semi_keep_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, Lookup L, const uint32_t *presence, SemiValid sv,
                                                        uint32_t *marks, uint64_t *keep, uint32_t *tile_counts) {
    static_assert(!MARKS || FORM == SEMI_LOOKUP, "marks need the start of the match: the lookup form");
    static_assert(KEEP || MARKS, "a pass that neither keeps nor marks does nothing");
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles; tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
#pragma unroll 2
        for (int k0 = 0; k0 < TILE_WORDS; k0 += 8) {
            uint64_t key[8], meta[8];
            bool hit[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int64_t row = row0 + int64_t(k0 + k) * 64 + lane_id();
                key[k] = __builtin_nontemporal_load(&rkeys[row < last ? row : last]); // (a row past the end looks the last key up: in bounds, and masked below)
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint64_t d = key[k] - L.dense_min;
                meta[k] = 0;
                if (MARKS) {
                    meta[k] = lookup_meta(L, key[k]);
                    hit[k] = meta[k] != 0ull;
                } else if (FORM == SEMI_RANGE) {
                    hit[k] = d < L.dense_span;
                } else if (FORM == SEMI_BITMAP) {
                    hit[k] = d < L.dense_span && ((presence[d >> 5] >> (d & 31)) & 1u); // (only bits below dense_span are defined)
                } else if (L.dense) {
                    hit[k] = d < L.dense_span && L.dense[d] != 0u;
                } else {
                    hit[k] = probe_one(L.slots, L.cap, L.shift, key[k]) != 0ull;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int64_t row = row0 + int64_t(k0 + k) * 64 + lane_id();
                bool h = row < n && hit[k];
                if (NULLS && row < n) {
#pragma unroll
                    for (int j = 0; j < NQE_MAX_JOIN_KEYS; ++j)
                        if (sv.v[j]) h = h && get_bit(sv.v[j], row);
                }
                if (MARKS && h) {
                    const uint32_t s = uint32_t(meta[k] >> 32), bit = 1u << (s & 31u);
                    uint32_t *w = marks + (s >> 5);
                    if (!(*w & bit)) atomicOr(w, bit);
                }
                if (KEEP) {
                    const bool kept = row < n && (ANTI ? !h : h);
                    const uint64_t kw = __ballot(kept);
                    if (row0 + int64_t(k0 + k) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0 + k] = kw;
                    total += __popcll(kw);
                }
            }
        }
        if (KEEP && lane_id() == 0) tile_counts[tile] = total;
    }
}

// ---- hashed tables, wave-cooperatively (probe_unique_coop_kernel / probe_pairs_kernel / probe_packed_kernel without their per-row
// outputs): a wave looks its 64 keys up in 8 sub-steps of 8 keys; lane (g, i) loads slot i of the bucket — one 128-byte line — of
// sub-step key g, the loads of all 8 sub-steps in flight together, and a ballot finds the match.  Per-lane probing (probe_one) fetches
// the same line per key but walks it with dependent, divergent loads: 3.32 ms per 10^8 keys of bench.py's c4_sparse against 1.36 ms for the
// packed words (profiles/semi_join; the PAIRS and SLOTS forms were not measured at that size — their inner-join twins were, see there).
// EVERY lane of the wave calls these, with the key of its own row.
enum SemiTable {
    SEMI_SLOTS = 0,  // `slots`: {key, start << 32 | count}, 8-slot buckets, empty = meta 0; every hashed table has it, and it gives the start
    SEMI_PAIRS = 1,  // `slotsp` as {key, payload} pairs, empty = key `filler`
    SEMI_PACKED = 2, // `slotsp` as 8-byte words (key - kmin) << pbits | payload, 16-slot buckets, empty = all ones: the smallest table
};
struct SemiHashed {
    const ulonglong2 *tab;
    uint32_t cap;
    int32_t shift;
    uint64_t filler;
    PackedPairs pp;
};
// meta of `key` (0: absent)
__device__ __forceinline__ uint64_t coop_find_slots(const ulonglong2 *__restrict__ tab, uint32_t cap, int shift, uint64_t key) {
    const int my_t = lane_id() >> 3, my_g = lane_id() & 7;
    uint64_t kg[8];
    ulonglong2 s[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        kg[t] = (uint64_t)__shfl((unsigned long long)key, t * 8 + (lane_id() >> 3), 64);
        s[t] = tab[home_slot(kg[t], shift) + uint32_t(lane_id() & 7)];
    }
    uint64_t meta = 0;
    bool settled = false;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint64_t m = __ballot(s[t].y != 0ull && s[t].x == kg[t]), f = __ballot(s[t].y == 0ull);
        const uint32_t mb = uint32_t(m >> (8 * my_g)) & 0xFFu, fb = uint32_t(f >> (8 * my_g)) & 0xFFu;
        const int src = 8 * my_g + (mb ? __ffs(int(mb)) - 1 : 0);
        const uint64_t mt = (uint64_t)__shfl((unsigned long long)s[t].y, src, 64);
        if (t == my_t) {
            meta = mb ? mt : 0ull;
            settled = mb != 0 || fb != 0;
        }
    }
    if (!settled) { // a full bucket without the key: the following buckets, a whole bucket per round trip
        uint32_t sl = (home_slot(key, shift) + 8u) & (cap - 1);
        bool done = false;
        for (uint32_t p = 8; p < cap && !done; p += 8) {
            ulonglong2 c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = tab[sl + uint32_t(i)];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (done) continue;
                if (c[i].y == 0ull) done = true;
                else if (c[i].x == key) { meta = c[i].y; done = true; }
            }
            sl = (sl + 8u) & (cap - 1);
        }
    }
    return meta;
}
__device__ __forceinline__ bool coop_find_pairs(const ulonglong2 *__restrict__ tab, uint32_t cap, int shift, uint64_t filler, uint64_t key) {
    const int my_t = lane_id() >> 3, my_g = lane_id() & 7;
    uint64_t kg[8];
    ulonglong2 s[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        kg[t] = (uint64_t)__shfl((unsigned long long)key, t * 8 + (lane_id() >> 3), 64);
        s[t] = tab[home_slot(kg[t], shift) + uint32_t(lane_id() & 7)];
    }
    bool hit = false, settled = false;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint64_t m = __ballot(s[t].x == kg[t]), f = __ballot(s[t].x == filler);
        const uint32_t mb = uint32_t(m >> (8 * my_g)) & 0xFFu, fb = uint32_t(f >> (8 * my_g)) & 0xFFu;
        if (t == my_t) {
            hit = mb != 0;
            settled = hit || fb != 0;
        }
    }
    if (!settled) {
        uint32_t sl = (home_slot(key, shift) + 8u) & (cap - 1);
        bool done = false;
        for (int hop = 0; hop < 2 * UNIQUE_MAX_PROBE / 8 && !done; ++hop) {
            ulonglong2 c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = tab[sl + uint32_t(i)];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (done) continue;
                if (c[i].x == key) { hit = true; done = true; }
                else if (c[i].x == filler) done = true;
            }
            sl = (sl + 8u) & (cap - 1);
        }
    }
    return hit && key != filler; // (the filler is not a build key: it would match an empty slot)
}
__device__ __forceinline__ bool coop_find_packed(const ulonglong2 *__restrict__ tab, const PackedPairs &pp, uint64_t key) {
    const int my_t = lane_id() >> 3, my_g = lane_id() & 7;
    const uint64_t kd = key - pp.kmin;
    uint64_t kdg[8];
    ulonglong2 s[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint64_t kg = (uint64_t)__shfl((unsigned long long)key, t * 8 + (lane_id() >> 3), 64);
        kdg[t] = kg - pp.kmin;
        s[t] = tab[packed_home(kg, pp.nb) * (PACKED_BUCKET / 2) + uint32_t(lane_id() & 7)];
    }
    bool hit = false, settled = false;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint64_t m = __ballot((s[t].x >> pp.pbits) == kdg[t] || (s[t].y >> pp.pbits) == kdg[t]), f = __ballot(s[t].x == ~0ull || s[t].y == ~0ull);
        const uint32_t mb = uint32_t(m >> (8 * my_g)) & 0xFFu, fb = uint32_t(f >> (8 * my_g)) & 0xFFu;
        if (t == my_t) {
            hit = mb != 0;
            settled = hit || fb != 0;
        }
    }
    if (!settled) {
        uint32_t b = packed_home(key, pp.nb) + 1;
        bool done = false;
        for (int hop = 0; hop < 2 * UNIQUE_MAX_PROBE / PACKED_BUCKET && !done; ++hop) {
            if (b == pp.nb) b = 0;
            ulonglong2 w[PACKED_BUCKET / 2];
#pragma unroll
            for (int i = 0; i < PACKED_BUCKET / 2; ++i) w[i] = tab[size_t(b) * (PACKED_BUCKET / 2) + i];
#pragma unroll
            for (int i = 0; i < PACKED_BUCKET / 2; ++i) {
                if (done) continue;
                if ((w[i].x >> pp.pbits) == kd) { hit = true; done = true; }
                else if (w[i].x == ~0ull) done = true;
                else if ((w[i].y >> pp.pbits) == kd) { hit = true; done = true; }
                else if (w[i].y == ~0ull) done = true;
            }
            ++b;
        }
    }
    return hit && kd <= pp.kspan; // (a key outside the build range shifts to bits no stored word has — except the empty word's)
}
// semi_keep_kernel for hashed tables: the same keep mask, counts, NULL rule, marks and tail handling, one 64-row word per step
template <int TABLE, bool ANTI, bool NULLS, bool MARKS, bool KEEP>
__global__ void __launch_bounds__(256) semi_keep_coop_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, SemiHashed H, SemiValid sv, uint32_t *marks, uint64_t *keep,
                                                             uint32_t *tile_counts) {
    static_assert(!MARKS || TABLE == SEMI_SLOTS, "marks need the start of the match: the {key, meta} table");
    static_assert(KEEP || MARKS, "a pass that neither keeps nor marks does nothing");
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles; tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k0 = 0; k0 < TILE_WORDS; ++k0) {
            const int64_t row = row0 + int64_t(k0) * 64 + lane_id();
            const uint64_t key = __builtin_nontemporal_load(&rkeys[row < last ? row : last]);
            uint64_t meta = 0;
            bool h;
            if (TABLE == SEMI_SLOTS) {
                meta = coop_find_slots(H.tab, H.cap, H.shift, key);
                h = meta != 0ull;
            } else if (TABLE == SEMI_PAIRS) {
                h = coop_find_pairs(H.tab, H.cap, H.shift, H.filler, key);
            } else {
                h = coop_find_packed(H.tab, H.pp, key);
            }
            h = h && row < n;
            if (NULLS && row < n) {
#pragma unroll
                for (int j = 0; j < NQE_MAX_JOIN_KEYS; ++j)
                    if (sv.v[j]) h = h && get_bit(sv.v[j], row);
            }
            if (MARKS && h) {
                const uint32_t s = uint32_t(meta >> 32), bit = 1u << (s & 31u);
                uint32_t *w = marks + (s >> 5);
                if (!(*w & bit)) atomicOr(w, bit);
            }
            if (KEEP) {
                const bool kept = row < n && (ANTI ? !h : h);
                const uint64_t kw = __ballot(kept);
                if (row0 + int64_t(k0) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0] = kw;
                total += __popcll(kw);
            }
        }
        if (KEEP && lane_id() == 0) tile_counts[tile] = total;
    }
}

// the build rows whose bit is set (SEMI) or not (ANTI), as the KEEP mask of the compaction kernels (wave per 4096-row tile); <true> is
// also the outer join's pass over the build rows that no probe batch matched (label join_outer_unmatched).  direct tables test bit r;
// duplicate-key tables look the row's own key up (bkeys: the build key column — for Utf8 keys re-encoded through the table's
// dictionary) and test bit `start`, the bit every row of that key shares.
template <bool ANTI>
__global__ void __launch_bounds__(256) marked_build_kernel(const uint64_t *bkeys, int64_t n, int64_t ntiles, Lookup L, const uint32_t *marks, uint64_t *keep,
                                                           uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles; tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k = 0; k < TILE_WORDS; ++k) {
            const int64_t row = row0 + int64_t(k) * 64 + lane_id();
            bool kept = false;
            if (row < n) {
                const uint32_t s = L.direct ? uint32_t(row) : uint32_t(lookup_meta(L, bkeys[row]) >> 32);
                const bool marked = (marks[s >> 5] >> (s & 31u)) & 1u;
                kept = ANTI ? !marked : marked;
            }
            const uint64_t kw = __ballot(kept);
            if (row0 + int64_t(k) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k] = kw;
            total += __popcll(kw);
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

} // namespace

} // namespace nqe
