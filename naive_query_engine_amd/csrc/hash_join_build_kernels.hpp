// hash_join_build_kernels.hpp — the device side of the join's build (included once, by hash_join.hip, after hash_join_table.hpp):
// the sort-based build's run heads and inserts, the range measurement, the dense forms (one-kernel, scatter + finish, partitioned
// in one and two levels), the hashed forms ({key, row}, {key, payload}, packed) and the payload copies of the sort-based build.
#pragma once
#include "hash_join_table.hpp"

namespace nqe {

namespace {

__global__ void iota_u32_kernel(uint32_t *out, int64_t n) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = uint32_t(i);
}

// flags[j] = 1 iff sorted key j starts a run; flags[n] = 0 (so the exclusive scan leaves the total there)
__global__ void mark_heads_kernel(const uint64_t *skeys, int64_t n, uint32_t *flags) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j <= n; j += stride)
        flags[j] = (j < n && (j == 0 || skeys[j] != skeys[j - 1])) ? 1u : 0u;
}

// ustart[u] = position of the u-th run head in the sorted order; ustart[U] = n
__global__ void fill_ustart_kernel(const uint32_t *flags, const uint64_t *offs, int64_t n, uint32_t U, uint32_t *ustart) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j <= n; j += stride) {
        if (j == n) ustart[U] = uint32_t(n);
        else if (flags[j]) ustart[offs[j]] = uint32_t(j);
    }
}

// inserts every unique key: claims a slot by CAS on the meta word (0 = empty), then stores the key
__global__ void insert_unique_kernel(const uint64_t *skeys, const uint32_t *ustart, const uint32_t *perm, uint32_t U,
                                     ulonglong2 *slots, uint32_t cap, int shift, int direct) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; u < int64_t(U); u += stride) {
        uint32_t j = ustart[u];
        uint64_t key = skeys[j];
        uint64_t count = uint64_t(ustart[u + 1] - j);
        uint64_t start = direct ? uint64_t(perm[j]) : uint64_t(j);
        uint64_t meta = (start << 32) | count;
        uint32_t slot = home_slot(key, shift);
        for (;;) {
            unsigned long long old = atomicCAS((unsigned long long *)&slots[slot].y, 0ull, (unsigned long long)meta);
            if (old == 0ull) {
                slots[slot].x = key;
                break;
            }
            slot = (slot + 1) & (cap - 1);
        }
    }
}

__device__ __forceinline__ uint64_t probe_one(const ulonglong2 *__restrict__ slots, uint32_t cap, int shift, uint64_t key) {
    uint32_t slot = home_slot(key, shift);
    for (uint32_t p = 0; p < cap; ++p) {
        ulonglong2 s = slots[slot];
        if (s.y == 0ull) return 0ull;
        if (s.x == key) return s.y;
        slot = (slot + 1) & (cap - 1);
    }
    return 0ull;
}

// ---- sort-free build for unique keys (the common case: a dimension table's primary key).  Uniqueness is established by the
// build itself: a second occupant of a dense slot / a second slot with the same key raises *dup and the host falls back to the
// sort-based build below, which handles duplicates (and their ascending-build-row order).
// unsigned min / max of (value ^ flip) over up to MAX_JOIN_COLS columns in one launch: blockIdx.y = column; one atomic pair per
// workgroup (per wave it was 16 K same-address atomics at ~12 ns each = 0.2 ms of a 1e6-row build)
typedef unsigned long long nt_u64x2 __attribute__((ext_vector_type(2))); // (what __builtin_nontemporal_load takes for a 16-byte access)
// `descents` (column 0 = the key only): the number of rows whose key is below its predecessor's — a build side in (nearly) ascending
// key order, the usual shape of a dimension table, writes and gathers coalesced whatever its size
__global__ void __launch_bounds__(256) minmax_cols_kernel(MinMaxCols mc, int64_t n, unsigned long long *mins, unsigned long long *maxs, unsigned long long *descents) {
    __shared__ uint64_t smn[4], smx[4];
    const int c = blockIdx.y;
    const uint64_t *__restrict__ v = mc.src[c];
    const uint64_t flip = mc.flip[c];
    uint64_t mn = ~0ull, mx = 0;
    uint32_t desc = 0;
    // four independent loads in flight per thread (one at a time read 1.6 GB of a 10^8-row build side at 3.2 TB/s: 0.50 ms of the build)
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, last = n - 1;
    const bool want_desc = c == 0 && descents != nullptr;
    // 16-byte-aligned columns (the library's own always are): PAIRS of words in 16-byte non-temporal loads, four in flight — the word before
    // a pair (the descent test across pairs) is the lane below's second word; lane 0 reads it
    const int64_t npairs = (reinterpret_cast<uintptr_t>(v) & 15) == 0 ? n / 2 : 0;
    for (int64_t p0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p0 - threadIdx.x % 64 < npairs; p0 += 4 * stride) { // (whole waves stay in the loop: shuffles)
        nt_u64x2 x[4];
        uint64_t before[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * stride, pc = p < npairs ? p : npairs - 1;
            x[u] = __builtin_nontemporal_load(reinterpret_cast<const nt_u64x2 *>(v) + pc);
            before[u] = (want_desc && lane_id() == 0 && pc > 0) ? v[2 * pc - 1] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t p = p0 + u * stride;
            const uint64_t a = x[u].x ^ flip, b = x[u].y ^ flip;
            uint64_t prev = __shfl_up((unsigned long long)b, 1, 64); // (the lane below holds the pair before this one: consecutive lanes, consecutive pairs)
            if (lane_id() == 0) prev = before[u] ^ flip;
            if (p >= npairs) continue;
            mn = a < mn ? a : mn;
            mn = b < mn ? b : mn;
            mx = a > mx ? a : mx;
            mx = b > mx ? b : mx;
            if (want_desc) desc += (a > b ? 1u : 0u) + ((p > 0 && prev > a) ? 1u : 0u);
        }
    }
    // (the rest: an odd last word, or the whole column when it is not 16-byte aligned)
    for (int64_t i0 = 2 * npairs + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * stride) {
        uint64_t x[4], p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride, ic = i < last ? i : last;
            x[u] = v[ic] ^ flip;
            p[u] = want_desc ? (v[ic > 0 ? ic - 1 : 0] ^ flip) : 0; // (the neighbour's word is in the line just read)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * stride;
            if (i >= n) break;
            mn = x[u] < mn ? x[u] : mn;
            mx = x[u] > mx ? x[u] : mx;
            if (want_desc && i > 0 && p[u] > x[u]) ++desc;
        }
    }
    // (one atomic per WORKGROUP: random keys make every wave count descents, and same-address device atomics retire one at a time —
    // a pair per wave was ~0.1 ms of a 10^8-row build's min/max pass)
    __shared__ uint32_t sdesc[4];
    if (want_desc) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) desc += __shfl_down(desc, d, 64);
        if (lane_id() == 0) sdesc[threadIdx.x / 64] = desc;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t a = __shfl_down((unsigned long long)mn, d, 64), b = __shfl_down((unsigned long long)mx, d, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane_id() == 0) smn[threadIdx.x / 64] = mn, smx[threadIdx.x / 64] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mn = smn[w] < mn ? smn[w] : mn;
            mx = smx[w] > mx ? smx[w] : mx;
        }
        atomicMin(&mins[c], (unsigned long long)mn);
        atomicMax(&maxs[c], (unsigned long long)mx);
        if (want_desc) {
            const uint32_t dsum = sdesc[0] + sdesc[1] + sdesc[2] + sdesc[3];
            if (dsum) atomicAdd(descents, (unsigned long long)dsum);
        }
    }
}
__global__ void __launch_bounds__(256) dense_unique_build_kernel(const uint64_t *keys, int64_t n, uint64_t dmin, uint32_t *dense, uint32_t *presence,
                                                                 DensePayload dp, int *dup) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t d = keys[r] - dmin;
        const uint32_t bit = 1u << (d & 31);
        const uint32_t old = atomicOr(&presence[d >> 5], bit);
        if (old & bit) {
            *dup = 1; // plain store of a constant: every writer agrees
            continue;
        }
        dense[d] = uint32_t(r) + 1u;
        for (int c = 0; c < dp.n; ++c) {
            const uint64_t v = dp.src[c][r];
            if (dp.packed[c] >= 2) {
                // `packed` bits per entry (<= 25), entry d at bit d * packed of a zeroed table: neighbours share words, so the bits are
                // OR-ed in (at most two aligned words per entry)
                const uint64_t bit = d * uint64_t(dp.packed[c]);
                const uint64_t o = uint64_t(uint32_t(v - dp.base[c])) << (bit & 31);
                uint32_t *w = static_cast<uint32_t *>(dp.dst[c]) + (bit >> 5);
                atomicOr(w, uint32_t(o));
                if (o >> 32) atomicOr(w + 1, uint32_t(o >> 32));
            } else if (dp.packed[c]) static_cast<uint32_t *>(dp.dst[c])[d] = uint32_t(v - dp.base[c]);
            else static_cast<uint64_t *>(dp.dst[c])[d] = v;
        }
    }
}
// The same build WITHOUT device-scope atomics (they run at a flat ~2.4x10^10/s on this chip whatever the table size: two to three per
// row made a 10^8-row build 9.8 ms, a 10^7-row one 1.2 ms).  Pass A scatters row numbers with plain stores — of several rows with
// one key any one wins.  Pass B walks the table in KEY order, 64 entries per wave: the presence words are ballots, the number of
// occupied entries (== rows ⇔ the keys are unique) one atomic per workgroup, and the payload columns are GATHERED by the stored
// row (random reads, which the chip serves at 5-10x10^10/s) and written in whole coalesced words — bit-packed entries are
// assembled in LDS, a wave's 64 entries being exactly 2 x bits words.
__global__ void __launch_bounds__(256) dense_scatter_rows_kernel(const uint64_t *keys, int64_t n, uint64_t dmin, uint32_t *dense) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) dense[keys[r] - dmin] = uint32_t(r) + 1u;
}
// `kord` (the partitioned build below): the entries arrive as key-ordered records of `twp` words {row + 1, payload words…} — the row
// table is written from them here, and the payloads are read from the record of entry d, not gathered by row.
// WHOLE (kord with records of two or four words): a record is read in 16-byte loads — a wave's loads then cover its 1 or 2 KB of records
// once; word-by-word non-temporal loads at a 16-byte stride fetched every line once per word
template <bool WHOLE>
__global__ void __launch_bounds__(256) dense_finish_kernel(uint32_t *dense, uint64_t span, uint32_t *presence, DensePayload dp, unsigned long long *occupied,
                                                           const uint64_t *kord, int twp) {
    __shared__ uint32_t pack[4][2 * 25];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const uint64_t ngroups = (span + 63) / 64;
    uint32_t mine = 0;
    for (uint64_t g = uint64_t(blockIdx.x) * 4 + wave; g < ngroups; g += uint64_t(gridDim.x) * 4) {
        const uint64_t d = g * 64 + lane;
        uint32_t e = 0;
        nt_u64x2 r0 = {0ull, 0ull}, r1 = r0;
        constexpr bool whole = WHOLE;
        if (d < span) {
            if (whole) {
                r0 = __builtin_nontemporal_load(reinterpret_cast<const nt_u64x2 *>(kord + d * uint64_t(twp)));
                if (twp == 4) r1 = __builtin_nontemporal_load(reinterpret_cast<const nt_u64x2 *>(kord + d * uint64_t(twp) + 2));
                dense[d] = e = uint32_t(r0.x);
            } else if (kord) dense[d] = e = uint32_t(__builtin_nontemporal_load(&kord[d * uint64_t(twp)]));
            else e = dense[d];
        }
        const bool present = e != 0;
        const uint64_t m = __ballot(present);
        mine += __popcll(m);
        // presence: bit d of 32-bit words — this wave's 64 entries are words 2g and 2g + 1 (the bitmap is allocated in whole pairs)
        if (presence && lane < 2 && 2 * g + lane < (span + 31) / 32) presence[2 * g + lane] = uint32_t(m >> (32 * lane));
        for (int c = 0; c < dp.n; ++c) {
            const uint64_t v = !present ? dp.base[c]
                               : whole  ? (c == 0 ? r0.y : (c == 1 ? r1.x : r1.y)) // (twp 2: one payload word; twp 4: up to three)
                               : kord   ? __builtin_nontemporal_load(&kord[d * uint64_t(twp) + 1 + c])
                                        : dp.src[c][e - 1];
            const int nb = dp.packed[c];
            if (nb >= 2) {
                if (lane < 2 * nb) pack[wave][lane] = 0;
                __builtin_amdgcn_wave_barrier();
                const uint32_t bit = uint32_t(lane) * uint32_t(nb);
                const uint64_t o = uint64_t(uint32_t(v - dp.base[c])) << (bit & 31);
                atomicOr(&pack[wave][bit >> 5], uint32_t(o));
                if (o >> 32) atomicOr(&pack[wave][(bit >> 5) + 1], uint32_t(o >> 32));
                __builtin_amdgcn_wave_barrier();
                // entry d at bit d * nb: the wave's first entry starts word 2 * nb * g
                if (lane < 2 * nb) static_cast<uint32_t *>(dp.dst[c])[g * uint64_t(2 * nb) + lane] = pack[wave][lane];
                __builtin_amdgcn_wave_barrier();
            } else if (d < span) {
                if (nb) static_cast<uint32_t *>(dp.dst[c])[d] = uint32_t(v - dp.base[c]);
                else static_cast<uint64_t *>(dp.dst[c])[d] = v;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64); // (every lane of a wave holds the same count: lane 0's sum counts it 64 times)
    if (lane == 0 && mine) atomicAdd(occupied, (unsigned long long)(mine / 64));
}
// ---- Partitioned dense build (builds of >= 2^25 rows).  A table of gigabytes takes neither form above: random 4-byte stores and
// gathers over that range run at a fraction of the chip's line rate (22 ms per 10^8 rows), the atomics at their flat
// 2.4x10^10/s (10-11 ms).  Here the rows are first PARTITIONED BY KEY RANGE — tuples {key - min | row, payload words} in one
// stream; count, scan, then per 8192-row tile a counting sort in LDS so that a partition's tuples leave as one run — into
// slices of the table that fit one XCD's L2 (<= 3 MB of table per partition).  The second pass then scatters partition by
// partition: the workgroups of one XCD (blockIdx % 8) walk the same partitions together, their random stores land in an
// L2-resident slice and leave it as whole lines.  Payload words travel with the tuple (no gather by build row afterwards);
// dense_finish_kernel packs them from the key-ordered copies and counts the occupied entries (== rows <=> unique keys).
__global__ void __launch_bounds__(PB_BLOCK) part_build_count_kernel(PartBuild pb, uint32_t *counts) {
    __shared__ uint32_t hist[PB_MAX_PARTS];
    for (int p = threadIdx.x; p < PB_MAX_PARTS; p += blockDim.x) hist[p] = 0;
    __syncthreads();
    const int64_t lo = int64_t(blockIdx.x) * pb.chunk;
    const int64_t hi = lo + pb.chunk < pb.n ? lo + pb.chunk : pb.n;
    for (int64_t r0 = lo + threadIdx.x; r0 < hi; r0 += 4 * int64_t(blockDim.x)) { // (four loads in flight per thread)
        uint64_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = r0 + u * int64_t(blockDim.x);
            k[u] = __builtin_nontemporal_load(&pb.keys[r < hi ? r : hi - 1]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r0 + u * int64_t(blockDim.x) < hi) atomicAdd(&hist[uint32_t((k[u] - pb.dmin) >> pb.shift)], 1u);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < pb.parts; p += blockDim.x) counts[size_t(p) * size_t(pb.W) + blockIdx.x] = hist[p];
}
// offsets[p * W + w] (exclusive scan of the counts): where workgroup w's tuples of partition p start in the tuple stream
template <int RPT>
__global__ void __launch_bounds__(PB_BLOCK) part_build_scatter_kernel(PartBuild pb, const uint64_t *offsets, uint64_t *tuples) {
    constexpr int ROWS = PB_BLOCK * RPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int TW = 1 + pb.nc;
    uint64_t *stup = reinterpret_cast<uint64_t *>(smem);                          // [ROWS][TW]
    uint32_t *gcur = reinterpret_cast<uint32_t *>(stup + size_t(ROWS) * size_t(TW)); // [PB_MAX_PARTS] next tuple of (partition, this workgroup)
    uint32_t *tcnt = gcur + PB_MAX_PARTS;                                         // tuples of this tile per partition
    uint32_t *tstart = tcnt + PB_MAX_PARTS;                                       // tile-local exclusive scan
    __shared__ uint32_t wave_tot[PB_BLOCK / 64];
    const int parts = pb.parts;
    for (int p = threadIdx.x; p < PB_MAX_PARTS; p += blockDim.x) {
        gcur[p] = p < parts ? uint32_t(offsets[size_t(p) * size_t(pb.W) + blockIdx.x]) : 0u; // (rows < 2^32)
        tcnt[p] = 0;
    }
    __syncthreads();
    const int64_t lo = int64_t(blockIdx.x) * pb.chunk;
    const int64_t hi = lo + pb.chunk < pb.n ? lo + pb.chunk : pb.n;
    for (int64_t base = lo; base < hi; base += ROWS) {
        uint32_t d[RPT], rank[RPT];
        bool ok[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const int64_t row = base + int64_t(u) * PB_BLOCK + threadIdx.x;
            ok[u] = row < hi;
            d[u] = ok[u] ? uint32_t(__builtin_nontemporal_load(&pb.keys[row]) - pb.dmin) : 0u;
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) rank[u] = ok[u] ? atomicAdd(&tcnt[d[u] >> pb.shift], 1u) : 0u;
        __syncthreads();
        const uint32_t c = tcnt[threadIdx.x]; // PB_MAX_PARTS == PB_BLOCK: one counter per thread
        uint32_t wt;
        const uint32_t ex = wave_exclusive_scan(c, wt);
        if (lane_id() == 63) wave_tot[threadIdx.x / 64] = wt;
        __syncthreads();
        uint32_t pre = 0, tile_total = 0;
        for (int w = 0; w < PB_BLOCK / 64; ++w) {
            if (w < int(threadIdx.x) / 64) pre += wave_tot[w];
            tile_total += wave_tot[w];
        }
        tstart[threadIdx.x] = pre + ex;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            if (!ok[u]) continue;
            const int64_t row = base + int64_t(u) * PB_BLOCK + threadIdx.x;
            const uint32_t i = tstart[d[u] >> pb.shift] + rank[u];
            stup[size_t(i) * TW] = (uint64_t(d[u]) << 32) | uint64_t(uint32_t(row));
            for (int cc = 0; cc < pb.nc; ++cc) stup[size_t(i) * TW + 1 + cc] = __builtin_nontemporal_load(&pb.src[cc][row]);
        }
        __syncthreads();
        if (TW == 2) {
            for (uint32_t i = threadIdx.x; i < tile_total; i += PB_BLOCK) {
                const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(&stup[size_t(i) * 2]);
                const uint32_t p = uint32_t(t.x >> 32) >> pb.shift;
                *reinterpret_cast<ulonglong2 *>(&tuples[(size_t(gcur[p]) + (i - tstart[p])) * 2]) = t;
            }
        } else {
            // word e of the tile's sorted tuples: consecutive lanes write consecutive words, across tuple boundaries
            const uint32_t words = tile_total * uint32_t(TW);
            for (uint32_t e = threadIdx.x; e < words; e += PB_BLOCK) {
                const uint32_t i = e / uint32_t(TW), k = e - i * uint32_t(TW);
                const uint32_t p = uint32_t(stup[size_t(i) * TW] >> 32) >> pb.shift;
                tuples[(size_t(gcur[p]) + (i - tstart[p])) * size_t(TW) + k] = stup[e];
            }
        }
        __syncthreads();
        gcur[threadIdx.x] += tcnt[threadIdx.x];
        tcnt[threadIdx.x] = 0;
        __syncthreads();
    }
}
// The same scatter for key-only builds and one payload word (NC = 0 / 1: the shapes of the two-level form), with the tile's words in
// REGISTERS from the start — the payload word was requested only after two barriers, its whole latency in front of the staging — and
// the NEXT tile's words requested as soon as this tile's are staged: they arrive during the copy-out.  (One 1024-thread workgroup per
// CU holds the LDS: nothing else overlaps its phases.)
template <int NC>
__global__ void __launch_bounds__(PB_BLOCK) part_build_scatter1_kernel(PartBuild pb, const uint64_t *offsets, uint64_t *tuples) {
    constexpr int RPT = 8, ROWS = PB_BLOCK * RPT, TW = 1 + NC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t *stup = reinterpret_cast<uint64_t *>(smem);                          // [ROWS][TW]
    uint32_t *gcur = reinterpret_cast<uint32_t *>(stup + size_t(ROWS) * size_t(TW)); // [PB_MAX_PARTS] next tuple of (partition, this workgroup)
    uint32_t *tcnt = gcur + PB_MAX_PARTS;
    uint32_t *tstart = tcnt + PB_MAX_PARTS;
    __shared__ uint32_t wave_tot[PB_BLOCK / 64];
    const int parts = pb.parts;
    for (int p = threadIdx.x; p < PB_MAX_PARTS; p += blockDim.x) {
        gcur[p] = p < parts ? uint32_t(offsets[size_t(p) * size_t(pb.W) + blockIdx.x]) : 0u; // (rows < 2^32)
        tcnt[p] = 0;
    }
    __syncthreads();
    const int64_t lo = int64_t(blockIdx.x) * pb.chunk;
    const int64_t hi = lo + pb.chunk < pb.n ? lo + pb.chunk : pb.n;
    const uint64_t *__restrict__ keys = pb.keys;
    const uint64_t *__restrict__ pay = NC ? pb.src[0] : pb.keys;
    uint64_t kw[RPT], pw[NC ? RPT : 1];
    auto load = [&](int64_t base) {
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            int64_t row = base + int64_t(u) * PB_BLOCK + threadIdx.x;
            row = row < hi ? row : hi - 1; // clamp: unconditional, in-bounds (lo < hi)
            kw[u] = __builtin_nontemporal_load(&keys[row]);
            if (NC) pw[NC ? u : 0] = __builtin_nontemporal_load(&pay[row]);
        }
    };
    if (lo < hi) load(lo);
    for (int64_t base = lo; base < hi; base += ROWS) {
        uint32_t d[RPT], rank[RPT];
        bool ok[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            ok[u] = base + int64_t(u) * PB_BLOCK + threadIdx.x < hi;
            d[u] = uint32_t(kw[u] - pb.dmin);
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) rank[u] = ok[u] ? atomicAdd(&tcnt[d[u] >> pb.shift], 1u) : 0u;
        __syncthreads();
        const uint32_t c = tcnt[threadIdx.x]; // PB_MAX_PARTS == PB_BLOCK: one counter per thread
        uint32_t wt;
        const uint32_t ex = wave_exclusive_scan(c, wt);
        if (lane_id() == 63) wave_tot[threadIdx.x / 64] = wt;
        __syncthreads();
        uint32_t pre = 0, tile_total = 0;
        for (int w = 0; w < PB_BLOCK / 64; ++w) {
            if (w < int(threadIdx.x) / 64) pre += wave_tot[w];
            tile_total += wave_tot[w];
        }
        tstart[threadIdx.x] = pre + ex;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            if (!ok[u]) continue;
            const uint32_t row = uint32_t(base + int64_t(u) * PB_BLOCK + threadIdx.x);
            const uint32_t i = tstart[d[u] >> pb.shift] + rank[u];
            const uint64_t x = (uint64_t(d[u]) << 32) | uint64_t(row);
            if (NC) *reinterpret_cast<ulonglong2 *>(&stup[size_t(i) * 2]) = make_ulonglong2(x, pw[NC ? u : 0]);
            else stup[i] = x;
        }
        if (base + ROWS < hi) load(base + ROWS); // (workgroup-uniform) the next tile's words fly during the copy-out
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < tile_total; i += PB_BLOCK) {
            if (NC) {
                const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(&stup[size_t(i) * 2]);
                const uint32_t p = uint32_t(t.x >> 32) >> pb.shift;
                *reinterpret_cast<ulonglong2 *>(&tuples[(size_t(gcur[p]) + (i - tstart[p])) * 2]) = t;
            } else {
                const uint64_t t = stup[i];
                const uint32_t p = uint32_t(t >> 32) >> pb.shift;
                tuples[size_t(gcur[p]) + (i - tstart[p])] = t;
            }
        }
        __syncthreads();
        gcur[threadIdx.x] += tcnt[threadIdx.x];
        tcnt[threadIdx.x] = 0;
        __syncthreads();
    }
}
// pass 2: the workgroups of XCD x (HW_REG_XCC_ID — a performance matter only) take the partitions p = x, x + 8, … one after the other,
// sharing each 2048 tuples at a time through the partition's cursor; afterwards every workgroup sweeps all cursors once and takes
// what is left (nothing, when the hardware numbers its XCDs 0 … 7), so every tuple is placed whatever the mapping.
__device__ __forceinline__ uint32_t xcc_id() {
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 15u;
}
// Key-only build sides store the row number into `dense`; with payload words the whole entry goes into a key-ordered record of
// twp = 2 * ceil((1 + nc) / 2) words in 16-byte stores (random stores cost per store, not per byte: 6-8x10^10/s whatever the slice).
__global__ void __launch_bounds__(256) part_build_place_kernel(PartBuild pb, const uint64_t *offsets, const uint64_t *tuples, uint32_t *dense, uint64_t *kord,
                                                               int twp, uint32_t *cursor, int by_block, uint32_t chunk) {
    __shared__ uint32_t got;
    __shared__ int left;
    const int x = by_block ? int(blockIdx.x % PB_XCDS) : int(xcc_id() % PB_XCDS);
    const int TW = 1 + pb.nc;
    for (int sweep = 0; sweep < 2; ++sweep) {
        if (sweep) { // anything left?  (all cursors looked at together; normally nothing is)
            if (threadIdx.x == 0) left = 0;
            __syncthreads();
            for (int p = threadIdx.x; p < pb.parts; p += 256)
                if (offsets[size_t(p) * size_t(pb.W)] + __hip_atomic_load(&cursor[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < offsets[size_t(p + 1) * size_t(pb.W)]) left = 1;
            __syncthreads();
            if (!left) break; // (workgroup-uniform)
        }
        for (int p = sweep ? 0 : x; p < pb.parts; p += sweep ? 1 : PB_XCDS) {
            const uint64_t s = offsets[size_t(p) * size_t(pb.W)], e = offsets[size_t(p + 1) * size_t(pb.W)]; // (offsets[parts * W] = rows)
            for (;;) {
                if (threadIdx.x == 0) got = atomicAdd(&cursor[p], chunk);
                __syncthreads();
                const uint64_t c0 = s + got;
                __syncthreads();
                if (c0 >= e) break;
                const uint64_t c1 = c0 + chunk < e ? c0 + chunk : e;
                for (uint64_t i = c0 + threadIdx.x; i < c1; i += 256) {
                    if (kord && TW == 2) { // {key - min | row, payload}: one 16-byte load, one 16-byte store
                        const nt_u64x2 t = __builtin_nontemporal_load(reinterpret_cast<const nt_u64x2 *>(tuples + i * 2));
                        *reinterpret_cast<ulonglong2 *>(kord + uint64_t(uint32_t(t.x >> 32)) * 2) = make_ulonglong2(uint64_t(uint32_t(t.x) + 1u), t.y);
                        continue;
                    }
                    const uint64_t w0 = __builtin_nontemporal_load(&tuples[i * TW]);
                    const uint32_t d = uint32_t(w0 >> 32);
                    if (!kord) {
                        dense[d] = uint32_t(w0) + 1u;
                        continue;
                    }
                    uint64_t *rec = kord + uint64_t(d) * uint64_t(twp);
                    uint64_t a = uint64_t(uint32_t(w0) + 1u);
                    for (int k = 0; k < twp; k += 2) {
                        const uint64_t b = k + 1 < TW ? __builtin_nontemporal_load(&tuples[i * TW + k + 1]) : 0ull;
                        *reinterpret_cast<ulonglong2 *>(rec + k) = make_ulonglong2(a, b);
                        a = k + 2 < TW ? __builtin_nontemporal_load(&tuples[i * TW + k + 2]) : 0ull;
                    }
                }
            }
        }
    }
}
// ---- Two-level form of the partitioned build (round 6): what the place pass pays for is one scattered 16-byte store per row —
// 1.9 ms per 10^8 rows whatever its slice size, workgroup count or cursor chunk (profiles/r05/sweep_build_place.txt), plus a zeroed
// 16-byte record per key written and read back (memset 0.3 + finish 0.6 ms).  Here every store is coalesced: the count pass takes a
// FINE histogram (up to 64 bins per partition, each PB_FILL_KEYS keys wide: fine_count), so that after the usual scatter into
// partitions a second one — ONE workgroup per partition, a counting sort of 4096-tuple tiles in LDS, runs of a hundred tuples
// (part_build_split_kernel) — leaves the tuples grouped by fine bin; a fine bin's keys then fit a workgroup's LDS, where its entries
// are laid out in key order and leave as whole lines of the FINAL tables (row table, presence words, the packed payload column:
// part_build_fill_kernel) — no key-ordered records, no finish pass.  Key-only builds and builds with one payload word.
// count pass: this workgroup's rows per FINE bin in LDS; the partition counts of the scatter's offsets are sums of 2^fine_log2 of them, and the
// workgroup's fine histogram goes to finehist[w][bin] (added up by part_build_fine_offsets_kernel)
__global__ void __launch_bounds__(PB_BLOCK) part_build_count_fine_kernel(PartBuild pb, uint32_t *counts, uint32_t *finehist, int bins) {
    extern __shared__ uint32_t fhist[];
    for (int b = threadIdx.x; b < bins; b += blockDim.x) fhist[b] = 0;
    __syncthreads();
    const int64_t lo = int64_t(blockIdx.x) * pb.chunk;
    const int64_t hi = lo + pb.chunk < pb.n ? lo + pb.chunk : pb.n;
    for (int64_t r0 = lo + threadIdx.x; r0 < hi; r0 += 4 * int64_t(blockDim.x)) { // (four loads in flight per thread)
        uint64_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t r = r0 + u * int64_t(blockDim.x);
            k[u] = __builtin_nontemporal_load(&pb.keys[r < hi ? r : hi - 1]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r0 + u * int64_t(blockDim.x) < hi) atomicAdd(&fhist[uint32_t((k[u] - pb.dmin) >> PB_FILL_LOG2)], 1u);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < pb.parts; p += blockDim.x) {
        uint32_t c = 0;
        const int fl = pb.shift - PB_FILL_LOG2;
        for (int f = 0; f < (1 << fl); ++f) c += (p << fl) + f < bins ? fhist[(p << fl) + f] : 0u;
        counts[size_t(p) * size_t(pb.W) + blockIdx.x] = c;
    }
    for (int b = threadIdx.x; b < bins; b += blockDim.x) finehist[size_t(blockIdx.x) * size_t(bins) + b] = fhist[b];
}
// fine_start[b]: where fine bin b's tuples start in the twice-partitioned stream = its partition's start (offsets[p * W], the scatter's
// scan) + the bins of the partition before it.  One workgroup per partition (thread = bin x an eighth of the count workgroups);
// fine_start[bins] = rows.
__global__ void __launch_bounds__(256) part_build_fine_offsets_kernel(const uint32_t *finehist, int W, int bins, int parts, int fine_log2, const uint64_t *offsets, uint64_t *fine_start) {
    const int F = 1 << fine_log2;
    __shared__ uint32_t part[256]; // [256 / F][F]
    const int p = blockIdx.x, f = threadIdx.x % F, q = threadIdx.x / F, b = (p << fine_log2) + f;
    uint32_t c = 0;
    if (b < bins)
        for (int w = q; w < W; w += 256 / F) c += finehist[size_t(w) * size_t(bins) + b];
    part[q * F + f] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t at = offsets[size_t(p) * size_t(W)];
        for (int ff = 0; ff < F && (p << fine_log2) + ff < bins; ++ff) {
            fine_start[(p << fine_log2) + ff] = at;
            for (int qq = 0; qq < 256 / F; ++qq) at += part[qq * F + ff];
        }
        if (p == parts - 1) fine_start[bins] = at;
    }
}
// second scatter: workgroup p sorts partition p's tuples (offsets[p * W] .. offsets[(p + 1) * W) of `tuples`) by fine bin into `out`
// (same positions overall: the partition's range, its bins in order).  Per 4096-tuple tile: rank per bin (LDS atomic), the bins'
// starts inside the tile, tuples staged in LDS by bin, copy-out in runs — the only writer of its range, so the cursors are its own.
template <int NC>
__global__ void __launch_bounds__(PB_BLOCK) part_build_split_kernel(PartBuild pb, const uint64_t *offsets, const uint64_t *fine_start, int bins, const uint64_t *tuples, uint64_t *out) {
    constexpr int FMAX = 1 << PB_FINE_LOG2_MAX, RPT = PB_SPLIT_TILE / PB_BLOCK;
    const int fine_log2 = pb.shift - PB_FILL_LOG2, F = 1 << fine_log2;
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_smem[];
    uint64_t *stage = reinterpret_cast<uint64_t *>(pb_smem); // [PB_SPLIT_TILE][1 + NC]
    __shared__ uint32_t tcnt[FMAX], tstart[FMAX + 1];
    __shared__ uint64_t cur[FMAX];
    for (int p = blockIdx.x; p < pb.parts; p += gridDim.x) {
        const uint64_t s = offsets[size_t(p) * size_t(pb.W)], e = offsets[size_t(p + 1) * size_t(pb.W)];
        __syncthreads(); // (the previous partition's cursors are done with)
        if (int(threadIdx.x) < F) {
            const int b = (p << fine_log2) + int(threadIdx.x);
            cur[threadIdx.x] = b < bins ? fine_start[b] : e;
            tcnt[threadIdx.x] = 0;
        }
        __syncthreads();
        uint64_t x[RPT], y[NC ? RPT : 1];
        auto load = [&](uint64_t base) { // (the partition is not empty: s < e)
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const uint64_t i = base + uint64_t(u) * PB_BLOCK + threadIdx.x, ic = i < e ? i : e - 1;
                if (NC) {
                    const nt_u64x2 t = __builtin_nontemporal_load(reinterpret_cast<const nt_u64x2 *>(tuples + ic * 2));
                    x[u] = t.x;
                    y[NC ? u : 0] = t.y;
                } else
                    x[u] = __builtin_nontemporal_load(&tuples[ic]);
            }
        };
        if (s < e) load(s);
        for (uint64_t base = s; base < e; base += PB_SPLIT_TILE) {
            uint32_t f[RPT], rank[RPT];
            bool ok[RPT];
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                ok[u] = base + uint64_t(u) * PB_BLOCK + threadIdx.x < e;
                f[u] = (uint32_t(x[u] >> 32) >> PB_FILL_LOG2) & uint32_t(F - 1);
            }
#pragma unroll
            for (int u = 0; u < RPT; ++u) rank[u] = ok[u] ? atomicAdd(&tcnt[f[u]], 1u) : 0u;
            __syncthreads();
            if (threadIdx.x < 64) { // F <= 64 counters: one wave scans them
                const uint32_t c = int(threadIdx.x) < F ? tcnt[threadIdx.x] : 0u;
                uint32_t tot;
                const uint32_t ex = wave_exclusive_scan(c, tot);
                if (int(threadIdx.x) < F) tstart[threadIdx.x] = ex;
                if (threadIdx.x == 0) tstart[F] = tot;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                if (!ok[u]) continue;
                const uint32_t i = tstart[f[u]] + rank[u];
                if (NC) *reinterpret_cast<ulonglong2 *>(&stage[size_t(i) * 2]) = make_ulonglong2(x[u], y[NC ? u : 0]);
                else stage[i] = x[u];
            }
            if (base + PB_SPLIT_TILE < e) load(base + PB_SPLIT_TILE); // (workgroup-uniform) the next tile flies during the copy-out
            __syncthreads();
            const uint32_t total = tstart[F];
            for (uint32_t i = threadIdx.x; i < total; i += PB_BLOCK) {
                if (NC) {
                    const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(&stage[size_t(i) * 2]);
                    const uint32_t fb = (uint32_t(t.x >> 32) >> PB_FILL_LOG2) & uint32_t(F - 1);
                    *reinterpret_cast<ulonglong2 *>(&out[(cur[fb] + (i - tstart[fb])) * 2]) = t;
                } else {
                    const uint64_t t = stage[i];
                    const uint32_t fb = (uint32_t(t >> 32) >> PB_FILL_LOG2) & uint32_t(F - 1);
                    out[cur[fb] + (i - tstart[fb])] = t;
                }
            }
            __syncthreads();
            if (int(threadIdx.x) < F) {
                cur[threadIdx.x] += tcnt[threadIdx.x];
                tcnt[threadIdx.x] = 0;
            }
            __syncthreads();
        }
    }
}
// one key-ordered group of 64 table entries (a wave): the row table, the presence words, the payload column of entry d in the form the
// join table keeps it (DensePayload::packed) — dense_finish_kernel's stores.  e: row + 1 (0: no such key), v: the payload word
__device__ __forceinline__ void dense_store_group(uint32_t *dense, uint32_t *presence, const DensePayload &dp, uint32_t (*pack)[2 * 25], int wave, int lane, uint64_t g, uint64_t span,
                                                  uint32_t e, uint64_t v) {
    const uint64_t d = g * 64 + uint64_t(lane);
    if (d < span) dense[d] = e;
    const bool present = e != 0;
    const uint64_t m = __ballot(present);
    if (presence && lane < 2 && 2 * g + lane < (span + 31) / 32) presence[2 * g + lane] = uint32_t(m >> (32 * lane));
    if (dp.n == 0) return;
    if (!present) v = dp.base[0];
    const int nb = dp.packed[0];
    if (nb >= 2) {
        if (lane < 2 * nb) pack[wave][lane] = 0;
        __builtin_amdgcn_wave_barrier();
        const uint32_t bit = uint32_t(lane) * uint32_t(nb);
        const uint64_t o = uint64_t(uint32_t(v - dp.base[0])) << (bit & 31);
        atomicOr(&pack[wave][bit >> 5], uint32_t(o));
        if (o >> 32) atomicOr(&pack[wave][(bit >> 5) + 1], uint32_t(o >> 32));
        __builtin_amdgcn_wave_barrier();
        if (lane < 2 * nb) static_cast<uint32_t *>(dp.dst[0])[g * uint64_t(2 * nb) + lane] = pack[wave][lane];
        __builtin_amdgcn_wave_barrier();
    } else if (d < span) {
        if (nb) static_cast<uint32_t *>(dp.dst[0])[d] = uint32_t(v - dp.base[0]);
        else static_cast<uint64_t *>(dp.dst[0])[d] = v;
    }
}
// fill: a workgroup takes fine bins (fine_start[b] .. fine_start[b + 1) of the twice-partitioned tuples = the keys [b, b + 1) <<
// PB_FILL_LOG2), lays their entries out in key order in LDS (a key met twice: one of its rows stays — the occupied count then
// falls short of the rows, and the caller takes the sort-based build) and writes the final tables in whole groups of 64 entries.
template <int NC>
__global__ void __launch_bounds__(PB_BLOCK) part_build_fill_kernel(const uint64_t *fine_start, int bins, const uint64_t *tuples, uint64_t span, uint32_t *dense, uint32_t *presence, DensePayload dp,
                                                                   unsigned long long *occupied) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pb_smem[];
    uint64_t *lv = reinterpret_cast<uint64_t *>(pb_smem);                              // [NC ? PB_FILL_KEYS : 0] payload words
    uint32_t *le = reinterpret_cast<uint32_t *>(lv + (NC ? PB_FILL_KEYS : 0));         // [PB_FILL_KEYS] row + 1
    __shared__ uint32_t pack[PB_BLOCK / 64][2 * 25];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    uint32_t mine = 0;
    for (int b = blockIdx.x; b < bins; b += gridDim.x) {
        __syncthreads(); // (the previous bin's entries have left)
        for (int i = threadIdx.x; i < PB_FILL_KEYS; i += PB_BLOCK) le[i] = 0;
        __syncthreads();
        const uint64_t s = fine_start[b], e = fine_start[b + 1];
        const uint32_t d0 = uint32_t(b) << PB_FILL_LOG2;
        for (uint64_t i0 = s + threadIdx.x; i0 < e; i0 += 4 * uint64_t(PB_BLOCK)) { // (four loads in flight per thread)
            uint64_t x[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t i = i0 + uint64_t(u) * PB_BLOCK, ic = i < e ? i : e - 1;
                if (NC) {
                    const nt_u64x2 t = __builtin_nontemporal_load(reinterpret_cast<const nt_u64x2 *>(tuples + ic * 2));
                    x[u] = t.x;
                    y[u] = t.y;
                } else {
                    x[u] = __builtin_nontemporal_load(&tuples[ic]);
                    y[u] = 0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i0 + uint64_t(u) * PB_BLOCK >= e) continue;
                const uint32_t sl = (uint32_t(x[u] >> 32) - d0) & uint32_t(PB_FILL_KEYS - 1);
                le[sl] = uint32_t(x[u]) + 1u;
                if (NC) lv[NC ? sl : 0] = y[u];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < PB_FILL_KEYS; i += PB_BLOCK) { // (whole waves: i - lane is a multiple of 64)
            const uint64_t g = (uint64_t(d0) + uint64_t(i)) >> 6;
            if (g * 64 >= span) break; // (wave-uniform: the table ends inside the last bin)
            const uint32_t ent = le[i];
            mine += ent != 0 ? 1u : 0u;
            dense_store_group(dense, presence, dp, pack, wave, lane, g, span, ent, NC ? lv[NC ? i : 0] : 0ull);
        }
    }
    // occupied entries: one atomic per workgroup
    __shared__ uint32_t wsum[PB_BLOCK / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < PB_BLOCK / 64; ++w) t += wsum[w];
        if (t) atomicAdd(occupied, t);
    }
}
// claims the first free slot of the probe sequence for every row (no key comparison: equal keys simply occupy several slots),
// then writes the key (and the 32-byte companion slot at the same index)
__global__ void __launch_bounds__(256) hashed_insert_rows_kernel(const uint64_t *keys, int64_t n, ulonglong2 *slots, uint32_t cap, int shift, int *dup) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t key = keys[r];
        const unsigned long long meta = ((unsigned long long)r << 32) | 1ull;
        uint32_t slot = home_slot(key, shift);
        // bounded walk: with unique keys at load <= 1/2 a sequence this long does not occur; many equal keys (which the sort-based
        // build handles) would otherwise turn the insert into O(n^2)
        bool placed = false;
        for (int p = 0; p < UNIQUE_MAX_PROBE; ++p) {
            if (atomicCAS((unsigned long long *)&slots[slot].y, 0ull, meta) == 0ull) {
                placed = true;
                break;
            }
            slot = (slot + 1) & (cap - 1);
        }
        if (!placed) {
            *dup = 1;
            continue;
        }
        slots[slot].x = key;
    }
}
// the {key, payload} table: empty slots hold `filler` (not a build key), so the key word itself is claimed by CAS — and an equal
// key already in place IS a duplicate
__global__ void __launch_bounds__(256) fill_pairs_kernel(ulonglong2 *t, uint32_t cap, uint64_t filler) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) t[i] = make_ulonglong2(filler, 0ull);
}
__global__ void __launch_bounds__(256) hashed_insert_pairs_kernel(const uint64_t *keys, const uint64_t *payload, int64_t n, ulonglong2 *t, uint32_t cap, int shift,
                                                                  uint64_t filler, int *dup) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t key = keys[r];
        uint32_t slot = home_slot(key, shift);
        bool placed = false;
        for (int p = 0; p < UNIQUE_MAX_PROBE; ++p) {
            const unsigned long long old = atomicCAS((unsigned long long *)&t[slot].x, (unsigned long long)filler, (unsigned long long)key);
            if (old == filler) {
                t[slot].y = payload[r];
                placed = true;
                break;
            }
            if (old == key) break; // the same key twice
            slot = (slot + 1) & (cap - 1);
        }
        if (!placed) *dup = 1;
    }
}
__global__ void __launch_bounds__(256) packed_insert_kernel(const uint64_t *keys, const uint64_t *payload, int64_t n, unsigned long long *tab, PackedPairs pp, int *dup) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const uint32_t total = pp.nb * PACKED_BUCKET;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t key = keys[r], kd = key - pp.kmin;
        const unsigned long long w = (kd << pp.pbits) | (payload[r] - pp.pbase);
        uint32_t slot = packed_home(key, pp.nb) * PACKED_BUCKET;
        bool placed = false;
        for (int p = 0; p < UNIQUE_MAX_PROBE; ++p) {
            const unsigned long long old = atomicCAS(&tab[slot], ~0ull, w);
            if (old == ~0ull) {
                placed = true;
                break;
            }
            if ((old >> pp.pbits) == kd) break; // the same key twice
            slot = slot + 1 == total ? 0 : slot + 1;
        }
        if (!placed) *dup = 1;
    }
}
// after the insert kernel has completed: does any row's probe sequence hold its key twice?
__global__ void __launch_bounds__(256) hashed_check_unique_kernel(const uint64_t *keys, int64_t n, const ulonglong2 *slots, uint32_t cap, int shift, int *dup) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t key = keys[r];
        uint32_t slot = home_slot(key, shift);
        for (int p = 0; p < 2 * UNIQUE_MAX_PROBE; ++p) {
            const ulonglong2 s = slots[slot];
            if (s.y == 0ull) break;
            if (s.x == key && uint32_t(s.y >> 32) != uint32_t(r)) {
                *dup = 1;
                break;
            }
            slot = (slot + 1) & (cap - 1);
        }
    }
}

__global__ void fill_dense_kernel(const uint64_t *skeys, const uint32_t *ustart, const uint32_t *perm, uint32_t U, uint64_t dmin,
                                  uint32_t *dense, int direct) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; u < int64_t(U); u += stride) {
        uint32_t j = ustart[u];
        dense[skeys[j] - dmin] = direct ? perm[j] + 1u : uint32_t(u) + 1u;
    }
}

// ---- unique + dense + plain payload: fused probe
__global__ void scatter_dense_payload_kernel(const uint64_t *keys, int64_t n, uint64_t dmin, const uint64_t *src, uint64_t *dst,
                                             uint32_t *presence) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        uint64_t d = keys[r] - dmin;
        if (dst) dst[d] = src[r];
        if (presence) atomicOr(&presence[d >> 5], 1u << (d & 31));
    }
}

// unsigned min / max of (value ^ flip) over a column (flip = sign bit for Int64 → order as signed)
__global__ void __launch_bounds__(256) minmax_u64_kernel(const uint64_t *v, int64_t n, uint64_t flip, unsigned long long *out_min, unsigned long long *out_max) {
    uint64_t mn = ~0ull, mx = 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
        const uint64_t x = v[i] ^ flip;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t a = __shfl_down(mn, d, 64), b = __shfl_down(mx, d, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane_id() == 0) {
        atomicMin(out_min, (unsigned long long)mn);
        atomicMax(out_max, (unsigned long long)mx);
    }
}
__global__ void scatter_dense_payload32_kernel(const uint64_t *keys, int64_t n, uint64_t dmin, const uint64_t *src, uint64_t base, uint32_t *dst,
                                               uint32_t *presence) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        uint64_t d = keys[r] - dmin;
        dst[d] = uint32_t(src[r] - base);
        if (presence) atomicOr(&presence[d >> 5], 1u << (d & 31));
    }
}

// dst[i] = src[perm[i]]: a payload column in sorted-row order (build side, once)
__global__ void __launch_bounds__(256) permute_words_kernel(const uint64_t *src, const uint32_t *perm, int64_t n, uint64_t *dst) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) dst[i] = src[perm[i]];
}

} // namespace

} // namespace nqe
