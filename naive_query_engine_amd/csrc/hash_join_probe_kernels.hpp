// hash_join_probe_kernels.hpp — the device side of the join's probe (included once, by hash_join.hip, after
// hash_join_build_kernels.hpp: probe_one lives there): the lookups of the unique-key forms, the presence pass and the fused write of
// the dense-payload form, and the two passes of the expand path — expand_count / expand_write, the one body each behind the inner
// entries here (probe_count_kernel, probe_write_kernel: the duplicate-key form) and the outer entries of hash_join_outer_kernels.hpp.
#pragma once
#include "hash_join_build_kernels.hpp"

namespace nqe {

namespace {

// (start<<32 | count) of `key`, 0 when absent. direct ⇒ start is the build row itself.
__device__ __forceinline__ uint64_t lookup_meta(const Lookup &L, uint64_t key) {
    if (L.dense) {
        uint64_t d = key - L.dense_min;
        if (d >= L.dense_span) return 0ull;
        uint32_t e = L.dense[d];
        if (e == 0) return 0ull;
        if (L.direct) return (uint64_t(e - 1) << 32) | 1ull;
        uint32_t st = L.ustart[e - 1];
        return (uint64_t(st) << 32) | uint64_t(L.ustart[e] - st);
    }
    return probe_one(L.slots, L.cap, L.shift, key);
}

// Unique build keys: one lookup per probe row → match bitmap (the KEEP mask of the compaction
// kernels), 4-byte build row per probe row, per-tile match counts.  Wave per 4096-row tile.
__global__ void __launch_bounds__(256) probe_unique_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, Lookup L, uint64_t *keep,
                                                           uint32_t *bidx, uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles;
         tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        // (issuing the first probe of 16 keys before examining any was measured slower, 2.41 -> 2.63 ms: the hashed probe is
        // bound by line fetches — 10^8 x 128 B at ≈5 TB/s — not by latency, and the extra registers cost occupancy)
#pragma unroll 2
        for (int k0 = 0; k0 < TILE_WORDS; k0 += 8) {
            uint64_t key[8], meta[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int64_t row = row0 + int64_t(k0 + k) * 64 + lane_id();
                key[k] = rkeys[row < last ? row : last];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) meta[k] = lookup_meta(L, key[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int64_t row = row0 + int64_t(k0 + k) * 64 + lane_id();
                bool hit = row < n && meta[k] != 0ull;
                uint64_t kw = __ballot(hit);
                if (row < n) bidx[row] = uint32_t(meta[k] >> 32);
                if (row0 + int64_t(k0 + k) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0 + k] = kw;
                total += __popcll(kw);
            }
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

// the same for hashed tables, wave-cooperatively (see probe_pairs_kernel): 8 lanes read the 8 slots of a key's bucket — one
// coalesced line per key, the loads of 8 sub-steps in flight together — and a ballot finds the match
__global__ void __launch_bounds__(256) probe_unique_coop_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, const ulonglong2 *tab, uint32_t cap, int shift,
                                                                uint64_t *keep, uint32_t *bidx, uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    const int my_t = lane_id() >> 3, my_g = lane_id() & 7;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles;
         tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k0 = 0; k0 < TILE_WORDS; ++k0) {
            const int64_t row = row0 + int64_t(k0) * 64 + lane_id();
            const uint64_t key = __builtin_nontemporal_load(&rkeys[row < last ? row : last]);
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
            if (!settled) { // a full bucket without the key: the following buckets, a whole bucket per round trip (see probe_pairs_kernel)
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
            const bool hit = row < n && meta != 0ull;
            const uint64_t kw = __ballot(hit);
            if (row < n) bidx[row] = uint32_t(meta >> 32);
            if (row0 + int64_t(k0) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0] = kw;
            total += __popcll(kw);
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

// pass 1: match bitmap + per-tile counts (no build-row output).
// MODE 0: every key of [min, min+span) is present → a range check, no memory access at all;
// MODE 1: presence bitmap staged in LDS (span/8 bytes ≤ 128 KB: random LDS reads instead of one L2
//         request per probe row); MODE 2: presence bitmap read from global memory.
template <int MODE>
__global__ void __launch_bounds__(1024) probe_presence_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, const uint32_t *presence,
                                                              uint64_t dmin, uint64_t span, uint64_t *keep, uint32_t *tile_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *lp = reinterpret_cast<uint32_t *>(smem);
    if (MODE == 1) {
        const uint32_t words = uint32_t((span + 31) / 32);
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) lp[i] = presence[i];
        __syncthreads();
    }
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles;
         tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
#pragma unroll 2
        for (int k0 = 0; k0 < TILE_WORDS; k0 += 8) {
            uint64_t key[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int64_t row = row0 + int64_t(k0 + k) * 64 + lane_id();
                key[k] = __builtin_nontemporal_load(&rkeys[row < last ? row : last]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int64_t row = row0 + int64_t(k0 + k) * 64 + lane_id();
                uint64_t d = key[k] - dmin;
                bool hit = row < n && d < span;
                if (MODE == 1) hit = hit && ((lp[d >> 5] >> (d & 31)) & 1u);
                if (MODE == 2) hit = hit && ((presence[d >> 5] >> (d & 31)) & 1u);
                uint64_t kw = __ballot(hit);
                if (row0 + int64_t(k0 + k) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0 + k] = kw;
                total += __popcll(kw);
            }
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

// pass 2: one read of the probe keys, every output column written in probe order
// `bidx` null: a build payload is addressed by key - dmin (key-ordered dense columns); non-null: by the build row recorded
// per probe row by probe_unique_kernel (hashed unique keys), gathered from the build columns themselves.
// IDENT (the optimistic form of a PK-FK join, see probe): no keep bitmap and no offsets — every probe row is taken to match, output row =
// probe row; a key outside [dmin, dmin + span) raises *miss and the host discards the output.
template <int FW_B, bool IDENT = false> // FW_B: rows per lane in flight
__global__ void __launch_bounds__(256) join_fused_write_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, const uint64_t *keep,
                                                               const uint64_t *tile_offsets, uint64_t dmin, const uint32_t *bidx, FusedCols fc,
                                                               uint64_t span, int *miss) {
    const int waves_per_block = blockDim.x / 64;
    const int64_t nwords = (n + 63) / 64;
    const int64_t last = n - 1;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles;
         tile += int64_t(gridDim.x) * waves_per_block) {
        int64_t w = tile * TILE_WORDS + lane_id();
        uint64_t my_word = 0;
        uint32_t tot = 0, my_off = 0;
        uint64_t base = 0;
        if (IDENT) {
            // some wave (or the sampling kernel ahead of this one) found a foreign key without its primary key: the host discards the
            // output, so stop writing it (checked once per 4096-row tile; the flag only ever goes from 0 to 1)
            if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(miss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return;
        }
        if (!IDENT) {
            my_word = w < nwords ? keep[w] : 0;
            my_off = wave_exclusive_scan(uint32_t(__popcll(my_word)), tot);
            if (tot == 0) continue; // no probe row of this tile matched (wave-uniform): nothing of it is read again
            base = tile_offsets[tile];
        }
        for (int k0 = 0; k0 < TILE_WORDS; k0 += FW_B) {
            uint64_t key[FW_B];
            uint32_t pos[FW_B]; // position inside the tile's output range
            uint32_t kept = 0;
#pragma unroll
            for (int k = 0; k < FW_B; ++k) {
                int64_t row = (tile * TILE_WORDS + k0 + k) * 64 + lane_id();
                key[k] = __builtin_nontemporal_load(&rkeys[row < last ? row : last]); // streamed once: keep L2 for the gather
            }
            if (IDENT) {
                bool bad = false;
#pragma unroll
                for (int k = 0; k < FW_B; ++k) {
                    const int64_t row = (tile * TILE_WORDS + k0 + k) * 64 + lane_id();
                    const bool in = row < n;
                    const bool ok = key[k] - dmin < span;
                    bad = bad || (in && !ok);
                    pos[k] = uint32_t(row - tile * TILE_ROWS);
                    kept |= uint32_t(in && ok) << k;
                }
                if (bad) *miss = 1; // plain store of a constant
                base = uint64_t(tile) * TILE_ROWS;
            } else {
#pragma unroll
                for (int k = 0; k < FW_B; ++k) {
                    uint64_t word = bcast64(my_word, k0 + k);
                    pos[k] = bcast32(my_off, k0 + k) + __popcll(word & lanemask_lt());
                    kept |= uint32_t((word >> lane_id()) & 1) << k;
                }
            }
            uint64_t gix[FW_B]; // gather index of a build payload
#pragma unroll
            for (int k = 0; k < FW_B; ++k) {
                if (bidx) {
                    int64_t row = (tile * TILE_WORDS + k0 + k) * 64 + lane_id();
                    gix[k] = bidx[row < last ? row : last];
                } else gix[k] = key[k] - dmin;
            }
            for (int c = 0; c < fc.n; ++c) {
                const uint64_t *__restrict__ src = fc.src[c];
                uint64_t *__restrict__ dst = fc.dst[c] + base;
                const int kind = fc.kind[c];
                uint64_t v[FW_B];
                if (kind == 0) {
#pragma unroll
                    for (int k = 0; k < FW_B; ++k) {
                        int64_t row = (tile * TILE_WORDS + k0 + k) * 64 + lane_id();
                        v[k] = __builtin_nontemporal_load(&src[row < last ? row : last]);
                    }
                } else if (kind == 1) {
#pragma unroll
                    for (int k = 0; k < FW_B; ++k) v[k] = key[k];
                } else if (kind == 2) {
#pragma unroll
                    for (int k = 0; k < FW_B; ++k) v[k] = src[(kept >> k) & 1 ? gix[k] : 0];
                } else if (kind == 3) {
                    const uint32_t *__restrict__ src32 = reinterpret_cast<const uint32_t *>(src);
                    const uint64_t b0 = fc.base[c];
#pragma unroll
                    for (int k = 0; k < FW_B; ++k) v[k] = b0 + src32[(kept >> k) & 1 ? gix[k] : 0];
                } else { // kind 4: `bits` per entry (<= 25): one unaligned 4-byte load holds the entry wherever it starts (the table is padded)
                    const uint8_t *__restrict__ src8 = reinterpret_cast<const uint8_t *>(src);
                    const uint64_t b0 = fc.base[c];
                    const uint32_t nb = uint32_t(fc.bits[c]), mask = (1u << nb) - 1u;
#pragma unroll
                    for (int k = 0; k < FW_B; ++k) {
                        const uint64_t bit = ((kept >> k) & 1 ? gix[k] : 0) * nb;
                        uint32_t x;
                        __builtin_memcpy(&x, src8 + (bit >> 3), 4);
                        v[k] = b0 + ((x >> (uint32_t(bit) & 7u)) & mask);
                    }
                }
#pragma unroll
                for (int k = 0; k < FW_B; ++k)
                    if ((kept >> k) & 1) __builtin_nontemporal_store(v[k], &dst[pos[k]]);
            }
        }
    }
}

// ahead of the optimistic one-pass probe: 2^16 probe keys spread evenly over the column, tested against the primary key's range.  A
// foreign key column that misses on any noticeable fraction of its rows is caught here in ~10 µs — the one-pass kernel behind
// it then leaves at once (it reads the flag before its first tile) instead of writing an output the host would discard
__global__ void __launch_bounds__(256) join_sample_range_kernel(const uint64_t *rkeys, int64_t n, uint64_t dmin, uint64_t span, int *miss) {
    const int64_t samples = int64_t(gridDim.x) * blockDim.x;
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t row = n <= samples ? i : int64_t((__int128)(i) * n / samples);
    const bool bad = row < n && !(rkeys[row < n ? row : n - 1] - dmin < span);
    if (__ballot(bad) && lane_id() == 0) *miss = 1;
}

// ---- unique hashed keys with ONE plain payload column: the lookup IS the gather.  Pass 1 of the two-pass probe looks every
// probe key up in the {key, payload} table (one random 16-byte access) and writes the payload word per probe row next to the
// match bitmap; the payload is then just another probe-side column that pass 2 (join_fused_write_kernel) streams and compacts —
// no build-row list, no second random access per row (the {key, row} form gathers every payload column by build row in pass 2).
// (A single-pass probe — decoupled look-back over per-tile counts, flat or hierarchical, publish-early / consume-a-tile-later —
// was built and measured: the fused kernel runs C4 in 1.00-1.08 ms with the placement given, 1.4-1.6 ms with any of the
// look-back variants: with 8 XCDs every publish / poll is a 2-5 µs fabric round trip per 512-1024-row tile and pollers eat the
// bandwidth the gathers need.  Two passes without inter-workgroup traffic are faster here.)
// Wave-cooperative probing: the table is read in 8-slot buckets = one 128-byte line.  A wave looks up its 64 keys in 8 sub-steps
// of 8 keys: lane (g, i) loads slot i of the bucket of sub-step key g — one coalesced line per key, all 8 sub-steps' loads in
// flight together — and a ballot finds the slot that matches.  Per-lane probing fetches the same one line per key but then walks
// collisions with dependent, divergent loads (2.4-3.0 ms per 1e8 keys against 1.6 ms for the bare random reads).
__global__ void __launch_bounds__(256) probe_pairs_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, const ulonglong2 *tab, uint32_t cap, int shift,
                                                          uint64_t filler, uint64_t *keep, uint64_t *payload, uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    const int my_t = lane_id() >> 3, my_g = lane_id() & 7; // this lane owns key my_g of sub-step my_t; as a loader it reads slot my_g... of group lane>>3
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles;
         tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k0 = 0; k0 < TILE_WORDS; ++k0) {
            const int64_t row = row0 + int64_t(k0) * 64 + lane_id();
            const uint64_t key = __builtin_nontemporal_load(&rkeys[row < last ? row : last]);
            uint64_t kg[8];
            ulonglong2 s[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) { // sub-step t serves the keys of lanes 8t .. 8t+7; this lane loads for key group lane >> 3
                kg[t] = (uint64_t)__shfl((unsigned long long)key, t * 8 + (lane_id() >> 3), 64);
                const uint32_t bucket = home_slot(kg[t], shift);
                s[t] = tab[bucket + uint32_t(lane_id() & 7)];
            }
            uint64_t pay = 0;
            bool hit = false, settled = false;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint64_t m = __ballot(s[t].x == kg[t]), f = __ballot(s[t].x == filler);
                const uint32_t mb = uint32_t(m >> (8 * my_g)) & 0xFFu, fb = uint32_t(f >> (8 * my_g)) & 0xFFu; // the bucket of this lane's own key, if t is its sub-step
                const int src = 8 * my_g + (mb ? __ffs(int(mb)) - 1 : 0);
                const uint64_t pl = (uint64_t)__shfl((unsigned long long)s[t].y, src, 64);
                if (t == my_t) {
                    hit = mb != 0;
                    pay = pl;
                    settled = hit || fb != 0; // found, or the bucket has a free slot: the key is not in the table
                }
            }
            if (!settled) { // a full bucket without the key — the following buckets, alone, a whole bucket (eight loads issued together) per round trip
                uint32_t sl = (home_slot(key, shift) + 8u) & (cap - 1);
                bool done = false;
                for (int hop = 0; hop < 2 * UNIQUE_MAX_PROBE / 8 && !done; ++hop) {
                    ulonglong2 c[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) c[i] = tab[sl + uint32_t(i)]; // (buckets are 8-slot aligned, cap is a multiple of 8)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (done) continue;
                        if (c[i].x == key) { hit = true; pay = c[i].y; done = true; }
                        else if (c[i].x == filler) done = true;
                    }
                    sl = (sl + 8u) & (cap - 1);
                }
            }
            hit = hit && row < n && key != filler;
            const uint64_t kw = __ballot(hit);
            if (row < n) __builtin_nontemporal_store(hit ? pay : 0ull, &payload[row]);
            if (row0 + int64_t(k0) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0] = kw;
            total += __popcll(kw);
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

// the same over the packed table: a bucket is 16 eight-byte slots = the same one line, lane (g, i) loads slots 2i and 2i + 1
__global__ void __launch_bounds__(256) probe_packed_kernel(const uint64_t *rkeys, int64_t n, int64_t ntiles, const ulonglong2 *tab, PackedPairs pp, uint64_t *keep,
                                                           uint64_t *payload, uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    const int64_t last = n - 1;
    const int my_t = lane_id() >> 3, my_g = lane_id() & 7;
    const uint64_t pmask = (1ull << pp.pbits) - 1ull;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles;
         tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k0 = 0; k0 < TILE_WORDS; ++k0) {
            const int64_t row = row0 + int64_t(k0) * 64 + lane_id();
            const uint64_t key = __builtin_nontemporal_load(&rkeys[row < last ? row : last]);
            const uint64_t kd = key - pp.kmin;
            uint64_t kdg[8];
            ulonglong2 s[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint64_t kg = (uint64_t)__shfl((unsigned long long)key, t * 8 + (lane_id() >> 3), 64);
                kdg[t] = kg - pp.kmin;
                s[t] = tab[packed_home(kg, pp.nb) * (PACKED_BUCKET / 2) + uint32_t(lane_id() & 7)];
            }
            uint64_t pay = 0;
            bool hit = false, settled = false;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const bool mx = (s[t].x >> pp.pbits) == kdg[t], my = (s[t].y >> pp.pbits) == kdg[t];
                const uint64_t m = __ballot(mx || my), f = __ballot(s[t].x == ~0ull || s[t].y == ~0ull);
                const uint32_t mb = uint32_t(m >> (8 * my_g)) & 0xFFu, fb = uint32_t(f >> (8 * my_g)) & 0xFFu;
                const int src = 8 * my_g + (mb ? __ffs(int(mb)) - 1 : 0);
                const uint64_t pl = (uint64_t)__shfl((unsigned long long)(mx ? s[t].x : s[t].y), src, 64);
                if (t == my_t) {
                    hit = mb != 0;
                    pay = pl;
                    settled = hit || fb != 0;
                }
            }
            if (!settled) { // a full bucket without the key (2-4 % of the buckets at load 0.6): the following buckets, alone — a whole bucket
                // per round trip (its eight 16-byte loads issued together, then examined in slot order): walking slot by slot made a
                // probe side of mostly absent keys twice as slow as one that matches (a wave waits for its slowest lane)
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
                        if ((w[i].x >> pp.pbits) == kd) { hit = true; pay = w[i].x; done = true; }
                        else if (w[i].x == ~0ull) done = true;
                        else if ((w[i].y >> pp.pbits) == kd) { hit = true; pay = w[i].y; done = true; }
                        else if (w[i].y == ~0ull) done = true;
                    }
                    ++b;
                }
            }
            hit = hit && row < n && kd <= pp.kspan; // (a key outside the build range shifts to bits no stored word has — except the empty word's)
            const uint64_t kw = __ballot(hit);
            if (row < n) __builtin_nontemporal_store(hit ? pp.pbase + (pay & pmask) : 0ull, &payload[row]);
            if (row0 + int64_t(k0) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k0] = kw;
            total += __popcll(kw);
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

// ---- the count → scan → expand-and-write path (hash_join.hip: probe_expand).  ONE body per pass; its entries are the inner probe of a
// duplicate-key table (probe_count_kernel, probe_write_kernel) and the outer probe (hash_join_outer_kernels.hpp).

// `start` recorded for a probe row without a match (count 1): build rows and positions in the sorted row list are < 2^32 - 1 —
// build_table refuses 2^32 rows and more, and the outer probe refuses the one size (2^32 rows) at which the last row would collide
constexpr uint32_t OUTER_NULL_START = 0xFFFFFFFFu;

// pass 1: one table lookup per probe row; records meta (start << 32 | count) and per-tile totals.  The outer entry's additions:
// KEEP_PROBE: a miss counts 1 and records OUTER_NULL_START (the write pass emits one row with every left column NULL); the misses
//             are summed into *misses (one atomic per 4096-row tile that has any): the host decides from it whether the left
//             columns of this batch get a validity buffer.
// MARKS:      a hit sets bit `start` of `marks` (direct: the build row; duplicate keys: the key's first position in the sorted row
//             list — every row of the key shares it).  One atomic per matching probe row, behind a plain read that skips it when
//             the bit is already set: a foreign key hits each primary key ~100 times, and bits only ever go from 0 to 1 (a stale
//             0 costs one redundant atomic, nothing else).
template <bool KEEP_PROBE, bool MARKS>
__device__ __forceinline__ void expand_count(const uint64_t *rkeys, int64_t n, Lookup L, uint64_t *pmeta, uint32_t *tile_counts, uint32_t *marks,
                                             unsigned long long *misses, int *flags) {
    __shared__ uint64_t wave_tot[JT_BLOCK / 64];
    __shared__ uint32_t wave_miss[JT_BLOCK / 64];
    for (int64_t tile = blockIdx.x; tile * JT_ROWS < n; tile += gridDim.x) {
        uint64_t keys[JT_ITERS];
#pragma unroll
        for (int it = 0; it < JT_ITERS; ++it) {
            int64_t i = tile * JT_ROWS + int64_t(it) * JT_BLOCK + threadIdx.x;
            keys[it] = i < n ? rkeys[i] : 0;
        }
        uint64_t local = 0;
        uint32_t miss = 0;
#pragma unroll
        for (int it = 0; it < JT_ITERS; ++it) {
            int64_t i = tile * JT_ROWS + int64_t(it) * JT_BLOCK + threadIdx.x;
            if (i < n) {
                uint64_t m = lookup_meta(L, keys[it]);
                if (m != 0ull) {
                    if (MARKS) {
                        const uint32_t s = uint32_t(m >> 32), bit = 1u << (s & 31u);
                        uint32_t *w = marks + (s >> 5);
                        if (!(*w & bit)) atomicOr(w, bit);
                    }
                } else if (KEEP_PROBE) {
                    m = (uint64_t(OUTER_NULL_START) << 32) | 1ull;
                    ++miss;
                }
                pmeta[i] = m;
                local += m & 0xFFFFFFFFull;
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            local += __shfl_down((unsigned long long)local, d, 64);
            if (KEEP_PROBE) miss += __shfl_down(miss, d, 64);
        }
        if (lane_id() == 0) {
            wave_tot[threadIdx.x / 64] = local;
            wave_miss[threadIdx.x / 64] = miss;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0, tm = 0;
            for (int w = 0; w < JT_BLOCK / 64; ++w) t += wave_tot[w], tm += wave_miss[w];
            if (t > 0xFFFFFFFFull) {
                atomicOr(&flags[NQE_FLAG_TABLE_FULL], 1);
                t = 0;
            }
            tile_counts[tile] = uint32_t(t);
            if (KEEP_PROBE && tm) atomicAdd(misses, (unsigned long long)tm);
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(JT_BLOCK) probe_count_kernel(const uint64_t *rkeys, int64_t n, Lookup L, uint64_t *pmeta,
                                                               uint32_t *tile_counts, int *flags) {
    expand_count<false, false>(rkeys, n, L, pmeta, tile_counts, nullptr, nullptr, flags);
}

// pass 2, output-driven ("load-balanced expansion"): a tile of probe rows is scanned in LDS; lane j of the
// workgroup then produces OUTPUT row base+j: its probe row is found by binary search in the tile's offsets,
// its match number m = j - offset[row], its build row = perm[start + m].  Consecutive lanes write consecutive
// output rows of every column (coalesced), probe-row-major with ascending build row inside a probe row —
// exactly the order of the reference's outer_pos/inner_pos (hash_join.rs:86-101).
// PLAIN: every source column is a plain 8-byte column without validity written as words (C4 with duplicate build keys: the whole
// output): no dtype dispatch, validity test or byte-array branches in the per-column loop
// NULL_EXTEND (the outer entry): a probe row whose recorded start is OUTER_NULL_START emits one row whose left columns hold null_word
// (0) / a false bit and validity byte 0; a left column's validity is source validity AND matched; a from_probe left column is read at
// the probe row.  Nothing of the build side is read for such a row (the build side may be empty), and on PLAIN a left column may
// still have a validity byte array (it has one when the batch contains a NULL-extended row).  Without NULL_EXTEND every live row is a
// hit and all of this folds away: the PLAIN instance loads unconditionally (dead lanes read source row 0 — the host grants PLAIN only
// when no source is empty) and stores behind live[q] alone.
template <bool PLAIN, bool NULL_EXTEND>
__device__ __forceinline__ void expand_write(const uint64_t *pmeta, int64_t n, const uint64_t *tile_offsets, const uint32_t *perm, int direct, const ExpandCols &ec) {
    __shared__ uint32_t off[PW_TILE + 1];
    __shared__ uint32_t startv[PW_TILE];
    __shared__ uint32_t wave_tot[JT_BLOCK / 64];
    constexpr int RPT = PW_TILE / JT_BLOCK; // probe rows per thread
    for (int64_t tile = blockIdx.x; tile * JT_ROWS < n; tile += gridDim.x) {
        uint64_t out_base = tile_offsets[tile];
        for (int sub = 0; sub < JT_ROWS / PW_TILE; ++sub) {
            const int64_t row0 = tile * JT_ROWS + int64_t(sub) * PW_TILE;
            if (row0 >= n) break;
            // ---- exclusive scan of the match counts of this sub-tile (thread t owns RPT consecutive probe rows)
            uint32_t cnt[RPT], local = 0;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                int64_t i = row0 + int64_t(threadIdx.x) * RPT + r;
                uint64_t m = i < n ? pmeta[i] : 0ull;
                cnt[r] = uint32_t(m & 0xFFFFFFFFull);
                startv[threadIdx.x * RPT + r] = uint32_t(m >> 32);
                local += cnt[r];
            }
            uint32_t wtot;
            uint32_t ex = wave_exclusive_scan(local, wtot);
            if (lane_id() == 63) wave_tot[threadIdx.x / 64] = wtot;
            __syncthreads();
            uint32_t pre = 0, total = 0;
            for (int w = 0; w < JT_BLOCK / 64; ++w) {
                if (w < int(threadIdx.x) / 64) pre += wave_tot[w];
                total += wave_tot[w];
            }
            uint32_t run = pre + ex;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                off[threadIdx.x * RPT + r] = run;
                run += cnt[r];
            }
            if (threadIdx.x == 0) off[PW_TILE] = total;
            __syncthreads();
            // ---- one lane per output row.  The lanes are shifted by the output position's offset inside its 128-byte line, so that every
            // wave's 64 consecutive words are four whole lines (round 5: a non-temporal store of a partial line is the costliest store there is)
            // (64-bit positions: one sub-tile may expand to 2^31 output rows and more — only the whole tile is bounded, at 2^32)
            const int64_t head = int64_t(out_base & 15);
            for (int64_t j0 = -head; j0 < int64_t(total); j0 += JT_BLOCK * 4) {
                uint32_t prow[4], brow[4], bpos[4];
                bool live[4], hit[4]; // hit: a live row that has a build row (not NULL-extended)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t js = j0 + q * JT_BLOCK + int64_t(threadIdx.x);
                    live[q] = js >= 0 && js < int64_t(total);
                    uint32_t lo = 0, hi = PW_TILE; // largest lo with off[lo] <= j
                    const uint32_t jj = live[q] ? uint32_t(js) : 0;
#pragma unroll
                    for (int step = 0; step < 10; ++step) {
                        uint32_t mid = (lo + hi) >> 1;
                        bool go = off[mid] <= jj;
                        lo = go ? mid : lo;
                        hi = go ? hi : mid;
                    }
                    prow[q] = lo;
                    const uint32_t st = startv[lo], mth = jj - off[lo];
                    hit[q] = live[q] && (!NULL_EXTEND || st != OUTER_NULL_START);
                    bpos[q] = hit[q] ? st + mth : 0u;
                    brow[q] = hit[q] ? (direct ? st : (ec.need_perm ? perm[st + mth] : 0u)) : 0u;
                }
                for (int c = 0; c < ec.n; ++c) {
                    const bool left = c < ec.n_left;
                    const void *src = ec.src[c];
                    const bool by_pos = ec.by_pos[c] != 0, from_probe = NULL_EXTEND && ec.from_probe[c] != 0;
                    if (PLAIN) {
                        uint8_t *__restrict__ vb = NULL_EXTEND ? ec.dst_valid_bytes[c] : nullptr;
                        const uint64_t *__restrict__ sw = static_cast<const uint64_t *>(src);
                        uint64_t *__restrict__ dw = ec.dst_words[c];
                        const uint64_t nw = NULL_EXTEND ? ec.null_word[c] : 0ull;
                        uint64_t v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (!NULL_EXTEND) v[q] = sw[left ? int64_t(by_pos ? bpos[q] : brow[q]) : (live[q] ? row0 + prow[q] : int64_t(0))]; // (dead lanes read row 0)
                            else if (left) v[q] = hit[q] ? sw[from_probe ? row0 + prow[q] : int64_t(by_pos ? bpos[q] : brow[q])] : nw;
                            else v[q] = live[q] ? sw[row0 + prow[q]] : 0ull;
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (!live[q]) continue;
                            const uint64_t pos = out_base + uint64_t(j0 + q * JT_BLOCK + int64_t(threadIdx.x));
                            __builtin_nontemporal_store(v[q], &dw[pos]);
                            if (NULL_EXTEND && vb) vb[pos] = hit[q] ? 1 : 0;
                        }
                        continue;
                    }
                    const uint8_t *sv = ec.src_valid[c];
                    const int dt = ec.dtype[c];
                    uint8_t *__restrict__ vb = ec.dst_valid_bytes[c];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (!live[q]) continue;
                        const uint64_t pos = out_base + uint64_t(j0 + q * JT_BLOCK + int64_t(threadIdx.x));
                        bool ok = false;
                        uint64_t v = NULL_EXTEND ? ec.null_word[c] : 0ull;
                        if (!left || hit[q]) {
                            const int64_t srow = left && !from_probe ? int64_t(by_pos ? bpos[q] : brow[q]) : row0 + prow[q];
                            ok = sv ? get_bit(sv, srow) : true;
                            v = load_word(src, dt, srow); // (the word under a NULL is read and dropped: no branch around the load)
                            v = ok ? v : 0ull;
                        }
                        if (ec.dst_words[c]) ec.dst_words[c][pos] = v;
                        if (ec.dst_bool_bytes[c]) ec.dst_bool_bytes[c][pos] = (ok && v) ? 1 : 0;
                        if (vb) vb[pos] = ok ? 1 : 0;
                    }
                }
            }
            out_base += total;
            __syncthreads();
        }
    }
}
// (8 waves per SIMD, as before the positions became 64-bit: the general instance would otherwise take two scalar registers too many)
template <bool PLAIN>
__global__ void __launch_bounds__(JT_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) probe_write_kernel(const uint64_t *pmeta, int64_t n, const uint64_t *tile_offsets,
                                                               const uint32_t *perm, int direct, ExpandCols ec) {
    expand_write<PLAIN, false>(pmeta, n, tile_offsets, perm, direct, ec);
}

} // namespace

} // namespace nqe
