// hash_join_outer_kernels.hpp — the device side of the outer hash joins (quirk Q19; included once, by hash_join.hip, after
// hash_join_probe_kernels.hpp: lookup_meta lives there): the count pass that keeps unmatched probe rows and marks matched build
// rows, the output-driven write pass with NULL-extended rows, and the pass over the build rows that never matched.  One general
// path over every build form (lookup_of is complete for all of them); the inner join's kernels are not touched.
#pragma once
#include "hash_join_probe_kernels.hpp"

namespace nqe {

namespace {

// `start` recorded for a probe row without a match (count 1): build rows and positions in the sorted row list are < 2^32 - 1 —
// build_table refuses 2^32 rows and more, and the outer probe refuses the one size (2^32 rows) at which the last row would collide
constexpr uint32_t OUTER_NULL_START = 0xFFFFFFFFu;

// the columns of outer_write_kernel: JoinCols + the word a NULL-extended row holds (0; -1 for a row-number column that feeds take_utf8)
struct OuterCols {
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
    uint64_t null_word[MAX_JOIN_COLS];
    uint64_t *dst_words[MAX_JOIN_COLS];
    uint8_t *dst_bool_bytes[MAX_JOIN_COLS];
    uint8_t *dst_valid_bytes[MAX_JOIN_COLS];
};

// pass 1 of the outer probe: probe_count_kernel with two additions.
// KEEP_PROBE: a miss counts 1 and records OUTER_NULL_START (the write pass emits one row with every left column NULL); the misses
//             are summed into *misses (one atomic per 4096-row tile that has any): the host decides from it whether the left
//             columns of this batch get a validity buffer.
// MARKS:      a hit sets bit `start` of `marks` (direct: the build row; duplicate keys: the key's first position in the sorted row
//             list — every row of the key shares it).  One atomic per matching probe row, behind a plain read that skips it when
//             the bit is already set: a foreign key hits each primary key ~100 times, and bits only ever go from 0 to 1 (a stale
//             0 costs one redundant atomic, nothing else).
template <bool KEEP_PROBE, bool MARKS>
__global__ void __launch_bounds__(JT_BLOCK) outer_count_kernel(const uint64_t *rkeys, int64_t n, Lookup L, uint64_t *pmeta, uint32_t *tile_counts,
                                                               uint32_t *marks, unsigned long long *misses, int *flags) {
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

// pass 2 of the outer probe: the load-balanced expansion of probe_write_kernel (LDS scan of the sub-tile's counts, a binary search
// per output row, lanes shifted so that waves store whole 128-byte lines) with NULL-extended rows: a probe row whose recorded
// start is OUTER_NULL_START emits one row whose left columns hold null_word (0) / a false bit and validity byte 0; a left column's
// validity is source validity AND matched.  Nothing of the build side is read for such a row (the build side may be empty).
// PLAIN: every source column is a plain 8-byte column without validity written as words; a left column may still have a
// validity byte array (it has one when the batch contains a NULL-extended row).
template <bool PLAIN>
__global__ void __launch_bounds__(JT_BLOCK) outer_write_kernel(const uint64_t *pmeta, int64_t n, const uint64_t *tile_offsets, const uint32_t *perm, int direct,
                                                               OuterCols oc) {
    __shared__ uint32_t off[PW_TILE + 1];
    __shared__ uint32_t startv[PW_TILE];
    __shared__ uint32_t wave_tot[JT_BLOCK / 64];
    constexpr int RPT = PW_TILE / JT_BLOCK; // probe rows per thread
    for (int64_t tile = blockIdx.x; tile * JT_ROWS < n; tile += gridDim.x) {
        uint64_t out_base = tile_offsets[tile];
        for (int sub = 0; sub < JT_ROWS / PW_TILE; ++sub) {
            const int64_t row0 = tile * JT_ROWS + int64_t(sub) * PW_TILE;
            if (row0 >= n) break;
            // ---- exclusive scan of the counts of this sub-tile (thread t owns RPT consecutive probe rows)
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
            // ---- one lane per output row, shifted by the output position's offset inside its 128-byte line
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
                    hit[q] = live[q] && st != OUTER_NULL_START;
                    bpos[q] = hit[q] ? st + mth : 0u;
                    brow[q] = hit[q] ? (direct ? st : (oc.need_perm ? perm[st + mth] : 0u)) : 0u;
                }
                for (int c = 0; c < oc.n; ++c) {
                    const bool left = c < oc.n_left;
                    const void *src = oc.src[c];
                    const bool by_pos = oc.by_pos[c] != 0, from_probe = oc.from_probe[c] != 0;
                    uint8_t *__restrict__ vb = oc.dst_valid_bytes[c];
                    if (PLAIN) {
                        const uint64_t *__restrict__ sw = static_cast<const uint64_t *>(src);
                        uint64_t *__restrict__ dw = oc.dst_words[c];
                        const uint64_t nw = oc.null_word[c];
                        uint64_t v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (left) v[q] = hit[q] ? sw[from_probe ? row0 + prow[q] : int64_t(by_pos ? bpos[q] : brow[q])] : nw;
                            else v[q] = live[q] ? sw[row0 + prow[q]] : 0ull;
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (!live[q]) continue;
                            const uint64_t pos = out_base + uint64_t(int64_t(j0) + q * JT_BLOCK + int64_t(threadIdx.x));
                            __builtin_nontemporal_store(v[q], &dw[pos]);
                            if (vb) vb[pos] = hit[q] ? 1 : 0;
                        }
                        continue;
                    }
                    const uint8_t *sv = oc.src_valid[c];
                    const int dt = oc.dtype[c];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (!live[q]) continue;
                        const uint64_t pos = out_base + uint64_t(int64_t(j0) + q * JT_BLOCK + int64_t(threadIdx.x));
                        bool ok = false;
                        uint64_t v = oc.null_word[c];
                        if (!left || hit[q]) {
                            const int64_t srow = left && !from_probe ? int64_t(by_pos ? bpos[q] : brow[q]) : row0 + prow[q];
                            ok = sv ? get_bit(sv, srow) : true;
                            v = ok ? load_word(src, dt, srow) : 0ull;
                        }
                        if (oc.dst_words[c]) oc.dst_words[c][pos] = v;
                        if (oc.dst_bool_bytes[c]) oc.dst_bool_bytes[c][pos] = (ok && v) ? 1 : 0;
                        if (vb) vb[pos] = ok ? 1 : 0;
                    }
                }
            }
            out_base += total;
            __syncthreads();
        }
    }
}

// the build rows that no probe batch matched, as the KEEP mask of the compaction kernels (wave per 4096-row tile).  direct tables
// test bit r; duplicate-key tables look the row's own key up (bkeys: the build key column — for Utf8 keys re-encoded through the
// table's dictionary) and test bit `start`, the bit every row of that key shares.
__global__ void __launch_bounds__(256) unmatched_build_kernel(const uint64_t *bkeys, int64_t n, int64_t ntiles, Lookup L, const uint32_t *marks, uint64_t *keep,
                                                              uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles; tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k = 0; k < TILE_WORDS; ++k) {
            const int64_t row = row0 + int64_t(k) * 64 + lane_id();
            bool unmatched = false;
            if (row < n) {
                const uint32_t s = L.direct ? uint32_t(row) : uint32_t(lookup_meta(L, bkeys[row]) >> 32);
                unmatched = !((marks[s >> 5] >> (s & 31u)) & 1u);
            }
            const uint64_t kw = __ballot(unmatched);
            if (row0 + int64_t(k) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k] = kw;
            total += __popcll(kw);
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

// set bits among the first n_rows bits of a bitmap of whole 64-bit words, added to *out (one atomic per wave): the exact null count
// of an output column is n_rows minus this
__global__ void __launch_bounds__(256) count_set_bits_kernel(const uint64_t *words, int64_t n_rows, unsigned long long *out) {
    const int64_t nwords = (n_rows + 63) / 64;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long local = 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nwords; i += stride) {
        uint64_t w = words[i];
        if (i == nwords - 1 && (n_rows & 63)) w &= (1ull << (n_rows & 63)) - 1ull;
        local += (unsigned long long)__popcll(w);
    }
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if (lane_id() == 0 && local) atomicAdd(out, local);
}

} // namespace

} // namespace nqe
