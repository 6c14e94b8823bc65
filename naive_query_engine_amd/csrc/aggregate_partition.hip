// aggregate_partition.hip — partitioned aggregation for more distinct keys than a workgroup's LDS table holds.
// More distinct keys than a workgroup's LDS table holds would turn every row into device-scope atomics, and
// those run at a flat ≈2.4e10 ops/s on MI355X whatever the scope, table size or layout (tools/atomics_bench.hip):
// 100 M rows took 17-20 ms at 4 K…1 M groups versus 0.6 ms at 1 K.  Instead the passing rows are hash-partitioned
// (count → scan → scatter of (key, values) tuples, PARTS partitions so that a workgroup's open write lines stay L2
// resident) and each partition — whose distinct keys now fit an LDS table — is aggregated by one workgroup.
#include "aggregate_partition_parts.hpp"

namespace nqe {
namespace agg {
namespace {

// The count pass of the exact form: how many passing rows of workgroup w's chunk fall into each partition (counts[p][w]).  It reads the
// key and predicate words only, never a value column.
template <int PRED, int KEY>
__global__ void __launch_bounds__(AGG_BLOCK) agg_partition_kernel(AggArgs a, FastPred fp, PartArgs pa) {
    __shared__ uint32_t cnt[PARTS];
    for (int p = threadIdx.x; p < PARTS; p += blockDim.x) cnt[p] = 0;
    __syncthreads();
    const RowSource<PRED, 0> src(a, pa.chunk);
    for (int64_t base = src.lo; base < src.hi; base += int64_t(AGG_BLOCK) * AGG_U) {
        RowRegs<PRED, 0, AGG_U> r;
        src.template load<AGG_U, AGG_BLOCK>(fp, r, base);
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            const bool pass = src.passes(a, fp, r, u, base + int64_t(u) * AGG_BLOCK + threadIdx.x);
            const uint64_t key = src.template key<KEY>(a, r.kw[u]);
            if (!pass) continue;
            atomicAdd(&cnt[hash_partition(key, PARTS_LOG2)], 1u);
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < PARTS; p += blockDim.x) pa.counts[size_t(p) * gridDim.x + blockIdx.x] = cnt[p];
}

// (The counting-sort tile below — stage by rank, copy out by cursor, advance the cursors — is written out here AND in
// agg_subpartition_kernel: as a shared function it cost instances of this kernel 10 VGPRs and a step of occupancy,
// profiles/partition_refactor/README.md.)
// Scatter pass with LDS write-combining: a tile of SC_ROWS rows is counting-sorted by partition inside LDS
// (rank = LDS atomic on a per-tile counter, tile-local exclusive scan), then copied out so that consecutive lanes
// write consecutive tuples of the same partition (runs of SC_ROWS/PARTS tuples → full 128-B lines instead of
// 8-byte stores sprayed over 512 streams: 2.4 ms → see DESIGN.md for the measured effect).
template <int PRED, int KEY, int NVT>
__global__ void __launch_bounds__(AGG_BLOCK) agg_partition_scatter_kernel(AggArgs a, FastPred fp, PartArgs pa) {
    constexpr int RPT = ExactScatterLayout::rows_per_thread(NVT); // rows per thread per tile
    constexpr int SC_ROWS = AGG_BLOCK * RPT;                       // 8192 (one value column) / 4096 (two)
    constexpr ExactScatterLayout L(SC_ROWS, NVT, PARTS);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t *skey = reinterpret_cast<uint64_t *>(smem + L.skey());
    uint64_t *sval = reinterpret_cast<uint64_t *>(smem + L.sval());
    uint64_t *gcur = reinterpret_cast<uint64_t *>(smem + L.gcur());     // global write cursor of this workgroup
    uint32_t *tcnt = reinterpret_cast<uint32_t *>(smem + L.tcnt());     // tuples of this tile per partition
    uint32_t *tstart = reinterpret_cast<uint32_t *>(smem + L.tstart()); // tile-local exclusive scan
    __shared__ uint32_t wave_tot[AGG_BLOCK / 64];
    for (int p = threadIdx.x; p < PARTS; p += blockDim.x) {
        gcur[p] = pa.offsets[size_t(p) * gridDim.x + blockIdx.x];
        tcnt[p] = 0;
    }
    __syncthreads();
    const RowSource<PRED, NVT> src(a, pa.chunk);
    for (int64_t base = src.lo; base < src.hi; base += SC_ROWS) {
        uint64_t key[RPT], vw[NVT][RPT];
        uint32_t part[RPT], rank[RPT];
        bool pass[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const int64_t row = base + int64_t(u) * AGG_BLOCK + threadIdx.x;
            const RowWords<NVT> w = src.load_row(fp, row);
#pragma unroll
            for (int j = 0; j < NVT; ++j) vw[j][u] = w.vw[j];
            pass[u] = src.passes(a, fp, w.kw, w.pw, row);
            key[u] = src.template key<KEY>(a, w.kw);
            part[u] = hash_partition(key[u], PARTS_LOG2);
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) rank[u] = pass[u] ? atomicAdd(&tcnt[part[u]], 1u) : 0u;
        __syncthreads();
        const uint32_t tile_total = tile_scan(tcnt, tstart, wave_tot, PARTS);
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            if (!pass[u]) continue;
            uint32_t i = tstart[part[u]] + rank[u];
            skey[i] = key[u];
#pragma unroll
            for (int j = 0; j < NVT; ++j) sval[j * SC_ROWS + i] = vw[j][u];
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < tile_total; i += blockDim.x) {
            uint64_t k = skey[i];
            uint32_t p = hash_partition(k, PARTS_LOG2);
            uint64_t dest = gcur[p] + (i - tstart[p]);
            pa.out_key[dest] = k;
#pragma unroll
            for (int j = 0; j < NVT; ++j) pa.out_val[j][dest] = sval[j * SC_ROWS + i];
        }
        __syncthreads();
        if (threadIdx.x < PARTS) {
            gcur[threadIdx.x] += tcnt[threadIdx.x];
            tcnt[threadIdx.x] = 0;
        }
        __syncthreads();
    }
}

// Second partitioning level: workgroup p splits parent partition p (a contiguous tuple range) into SUB sub-partitions
// by the next SUB_LOG2 hash bits — count, tile-local scan, then the same LDS-sorted scatter as level 1.  The output
// occupies the same global range as the input partition, so no cross-workgroup scan is needed.
template <int NVT>
__global__ void __launch_bounds__(AGG_BLOCK) agg_subpartition_kernel(const uint64_t *offsets, int64_t off_stride, const uint64_t *in_key,
                                                                     const uint64_t *in_v0, const uint64_t *in_v1, uint64_t *out_key,
                                                                     uint64_t *out_v0, uint64_t *out_v1, uint64_t *sub_offsets) {
    constexpr int RPT = ExactScatterLayout::rows_per_thread(NVT);
    constexpr int SC_ROWS = AGG_BLOCK * RPT;
    constexpr SubStageLayout L(SC_ROWS, NVT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t *skey = reinterpret_cast<uint64_t *>(smem + L.skey());
    uint64_t *sval = reinterpret_cast<uint64_t *>(smem + L.sval());
    __shared__ uint64_t gcur[SUB];
    __shared__ uint32_t tcnt[SUB], tstart[SUB], total_cnt[SUB];
    const uint64_t *__restrict__ inv[2] = {in_v0, in_v1};
    uint64_t *outv[2] = {out_v0, out_v1};
    auto sub_of = [](uint64_t k) { return uint32_t(((k * GOLD) << PARTS_LOG2) >> (64 - SUB_LOG2)); }; // the next SUB_LOG2 hash bits
    for (int p = blockIdx.x; p < PARTS; p += gridDim.x) {
        const int64_t lo = int64_t(offsets[int64_t(p) * off_stride]), hi = int64_t(offsets[int64_t(p + 1) * off_stride]);
        __syncthreads();
        if (threadIdx.x < SUB) total_cnt[threadIdx.x] = 0, tcnt[threadIdx.x] = 0;
        __syncthreads();
        // ---- count
        for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&total_cnt[sub_of(in_key[i])], 1u);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t run = uint64_t(lo);
            for (int sp = 0; sp < SUB; ++sp) {
                gcur[sp] = run;
                sub_offsets[int64_t(p) * SUB + sp] = run;
                run += total_cnt[sp];
            }
            if (p == PARTS - 1) sub_offsets[int64_t(PARTS) * SUB] = run;
        }
        __syncthreads();
        // ---- scatter, tile by tile, sorted in LDS first
        for (int64_t base = lo; base < hi; base += SC_ROWS) {
            uint64_t key[RPT], vw[NVT][RPT];
            uint32_t part[RPT], rank[RPT];
            bool pass[RPT];
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                int64_t row = base + int64_t(u) * AGG_BLOCK + threadIdx.x;
                pass[u] = row < hi;
                int64_t rc = pass[u] ? row : hi - 1;
                key[u] = in_key[rc];
#pragma unroll
                for (int j = 0; j < NVT; ++j) vw[j][u] = inv[j][rc];
                part[u] = sub_of(key[u]);
            }
#pragma unroll
            for (int u = 0; u < RPT; ++u) rank[u] = pass[u] ? atomicAdd(&tcnt[part[u]], 1u) : 0u;
            __syncthreads();
            if (threadIdx.x < 64) { // SUB == 64: one wave scans the tile counters
                uint32_t c = tcnt[threadIdx.x], wt;
                tstart[threadIdx.x] = wave_exclusive_scan(c, wt);
            }
            __syncthreads();
            uint32_t tile_total = tstart[SUB - 1] + tcnt[SUB - 1];
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                if (!pass[u]) continue;
                uint32_t i = tstart[part[u]] + rank[u];
                skey[i] = key[u];
#pragma unroll
                for (int j = 0; j < NVT; ++j) sval[j * SC_ROWS + i] = vw[j][u];
            }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < tile_total; i += blockDim.x) {
                uint64_t k = skey[i];
                uint32_t sp = sub_of(k);
                uint64_t dest = gcur[sp] + (i - tstart[sp]);
                out_key[dest] = k;
#pragma unroll
                for (int j = 0; j < NVT; ++j) outv[j][dest] = sval[j * SC_ROWS + i];
            }
            __syncthreads();
            if (threadIdx.x < SUB) {
                gcur[threadIdx.x] += tcnt[threadIdx.x];
                tcnt[threadIdx.x] = 0;
            }
            __syncthreads();
        }
    }
}

// seg_full_flag (agg_segments_kernel, agg_slab_segments_kernel: the partition has more distinct keys than the workgroup table) is read and
// written as an LDS word (ds_read / ds_write): through a generic `volatile int *` the accesses were FLAT loads, each followed by
// s_waitcnt vmcnt(0) — on every first-probe miss the wave waited for the tuples it had just prefetched
#define SEG_FULL() __hip_atomic_load(&seg_full_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define SEG_FULL_SET() __hip_atomic_store(&seg_full_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

// one workgroup per partition (grid-stride over partitions): plain (key, values) tuples → LDS table → global table.
// The LDS slot uses the hash bits BELOW the partition bits (all keys of a partition share the top PARTS_LOG2 bits).
template <int NVT, bool VF64>
__global__ void __launch_bounds__(AGG_BLOCK) agg_segments_kernel(AggArgs a, const uint64_t *seg_offsets, int64_t seg_stride, int nsegs, int part_bits,
                                                                 int signal_level2, const uint64_t *keys,
                                                                 const uint64_t *v0, const uint64_t *v1, GroupTable g, int *flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const HashedTable<NVT> tab(smem, uint32_t(a.lds_cap));
    const uint32_t cap = tab.cap, slots = tab.slots;
    double *const lsum = tab.lsum;
    uint64_t *const lmn = tab.lmn, *const lmx = tab.lmx;
    uint32_t *const lcnt = tab.lcnt;
    const uint64_t *__restrict__ valp[2] = {v0, v1};
    int vdt[NVT];
#pragma unroll
    for (int j = 0; j < NVT; ++j) vdt[j] = a.val[j].dtype;
    __shared__ int seg_full_flag;
    for (int seg = blockIdx.x; seg < nsegs; seg += gridDim.x) {
        __syncthreads();
        if (signal_level2 && __hip_atomic_load(&flags[NQE_FLAG_NEED_LEVEL2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        if (threadIdx.x == 0) seg_full_flag = 0;
        tab.init();
        __syncthreads();
        const int64_t lo = int64_t(seg_offsets[int64_t(seg) * seg_stride]), hi = int64_t(seg_offsets[int64_t(seg + 1) * seg_stride]);
        for (int64_t base = lo; base < hi; base += int64_t(AGG_BLOCK) * AGG_U) {
            uint64_t kw[AGG_U], vw[NVT][AGG_U];
#pragma unroll
            for (int u = 0; u < AGG_U; ++u) {
                int64_t row = base + int64_t(u) * AGG_BLOCK + threadIdx.x;
                row = row < hi - 1 ? row : hi - 1;
                kw[u] = keys[row];
#pragma unroll
                for (int j = 0; j < NVT; ++j) vw[j][u] = valp[j][row];
            }
#pragma unroll
            for (int u = 0; u < AGG_U; ++u) {
                int64_t row = base + int64_t(u) * AGG_BLOCK + threadIdx.x;
                if (row >= hi) continue;
                const uint64_t key = kw[u];
                // tuples of a partition arrive in no particular order: no run cache, one table update per row
                int slot;
                if (key == EMPTY_KEY) { tab.lkeys[cap] = 0; slot = int(cap); }
                else if (SEG_FULL()) slot = -1; // this partition has more distinct keys than the table: spill the rest
                else slot = tab.find_or_insert(key, part_bits, a.lds_shift);
                if (slot < 0 && !SEG_FULL()) {
                    SEG_FULL_SET();
                    if (signal_level2) atomicOr(&flags[NQE_FLAG_NEED_LEVEL2], 1); // the host re-partitions one level deeper
                }
                if (slot < 0 && signal_level2) continue;                              // result will be discarded
                if (slot < 0 && g.dense_count) {                                      // no hash table to spill to: the host falls back
                    atomicOr(&flags[NQE_FLAG_DENSE_OVERFLOW], 1);
                    continue;
                }
                int64_t gslot = slot < 0 ? global_find_or_insert(g, key, flags) : 0; // partition larger than the table: spill
#pragma unroll
                for (int j = 0; j < NVT; ++j) {
                    double x = VF64 ? u2d(vw[j][u]) : word_as_f64(vw[j][u], vdt[j]);
                    bool isn = x != x;
                    uint64_t xo = f64_to_ord(x);
                    if (slot >= 0) {
                        uint32_t o = uint32_t(j) * slots + uint32_t(slot);
                        atomicAdd(&lcnt[o], 1u);
                        if (isn) atomicOr(&lcnt[o], NAN_BIT);
                        unsafeAtomicAdd(&lsum[o], x);
                        if (!isn) {
                            if (xo < lmn[o]) atomicMin((unsigned long long *)&lmn[o], (unsigned long long)xo);
                            if (xo > lmx[o]) atomicMax((unsigned long long *)&lmx[o], (unsigned long long)xo);
                        }
                    } else if (gslot >= 0) {
                        global_update(g, gslot, a.v0 + j, 1, x, true, xo, xo, !isn, isn);
                    }
                }
            }
        }
        __syncthreads();
        if (g.dense_count) emit_dense(tab, g, a.v0, flags);
        else tab.flush_to_global(g, a.v0, flags);
    }
}

// ------------------------------------------------------------------ slab form: no count pass, software-pipelined scatter
// One workgroup per chunk of rows.  Per tile: fused predicate + key → partition → rank (LDS atomic on the tile's counter) →
// tile-local scan → tuples written to LDS at their sorted position → copied out so that consecutive lanes write consecutive
// tuples of one partition into THIS workgroup's slab of it.  The next tile's words are requested before the copy-out, so the
// loads overlap the LDS phases and the stores (one workgroup per CU fits — 136 KB of LDS — and the unpipelined form spent
// 22 µs per 8192-row tile where the CU's share of HBM needs 13).
// (Tuples of 16 or 24 bytes — a 64-bit key, or two value columns.  One value column under a key that fits 32 bits takes the two-stream
// whole-block form: agg_slab_scatter_soa_kernel below.)
#ifdef NQE_SLAB_PROFILE
// diagnostic build (tools/probe_slab_phases.py): shader-clock time of thread 0 of every scatter workgroup per phase of a tile
__device__ unsigned long long nqe_slab_prof[8];
#define SLAB_STAMP(i)                                   \
    do {                                                \
        if (threadIdx.x == 0) {                         \
            const unsigned long long now_ = clock64();  \
            prof_acc[i] += now_ - prof_t;               \
            prof_t = now_;                              \
        }                                               \
    } while (0)
#else
#define SLAB_STAMP(i) do { } while (0)
#endif
template <int PRED, int KEY, int NVT>
__global__ void __launch_bounds__(AGG_BLOCK) agg_slab_scatter_kernel(AggArgs a, FastPred fp, SlabArgs sa, int *flags) {
    constexpr int RPT = slab_scatter_rows_per_thread(PRED, KEY, NVT);
    constexpr int SC_ROWS = AGG_BLOCK * RPT;
    constexpr int TW = 1 + NVT; // words per tuple
    constexpr SlabScatterLayout L(SC_ROWS, NVT, PARTS);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t *stup = reinterpret_cast<uint64_t *>(smem + L.stup());     // [SC_ROWS][TW]
    uint32_t *gcur = reinterpret_cast<uint32_t *>(smem + L.gcur());     // tuples this workgroup has written per partition
    uint32_t *tcnt = reinterpret_cast<uint32_t *>(smem + L.tcnt());     // tuples of this tile per partition
    uint32_t *tstart = reinterpret_cast<uint32_t *>(smem + L.tstart()); // tile-local exclusive scan
    __shared__ uint32_t wave_tot[AGG_BLOCK / 64];
    const int parts_log2 = sa.parts_log2, parts = 1 << parts_log2; // <= PARTS (the LDS counters are sized for PARTS)
    for (int p = threadIdx.x; p < PARTS; p += blockDim.x) {
        gcur[p] = 0;
        tcnt[p] = 0;
    }
    __syncthreads();
    const RowSource<PRED, NVT> src(a, sa.chunk);
    const int64_t lo = src.lo, hi = src.hi;
    const uint32_t cap = uint32_t(sa.cap);
    typedef RowRegs<PRED, NVT, RPT> Regs;
    auto load = [&](Regs &r, int64_t base) { src.template load<RPT, AGG_BLOCK>(fp, r, base); };
#ifdef NQE_SLAB_PROFILE
    unsigned long long prof_acc[6] = {0, 0, 0, 0, 0, 0}, prof_t = clock64();
#endif
    auto tile = [&](const Regs &r, Regs &next, int64_t base) {
        uint64_t key[RPT];
        uint32_t part[RPT], rank[RPT];
        bool pass[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            pass[u] = src.passes(a, fp, r, u, base + int64_t(u) * AGG_BLOCK + threadIdx.x);
            key[u] = src.template key<KEY>(a, r.kw[u]);
            part[u] = hash_partition(key[u], parts_log2);
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) rank[u] = pass[u] ? atomicAdd(&tcnt[part[u]], 1u) : 0u;
        __syncthreads();
        SLAB_STAMP(0); // wait for the tile's words, key / partition, rank atomics
        const uint32_t tile_total = tile_scan(tcnt, tstart, wave_tot, parts);
        SLAB_STAMP(1); // scan of the tile's counters
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            if (!pass[u]) continue;
            const uint32_t i = tstart[part[u]] + rank[u];
            if (TW == 2) {
                *reinterpret_cast<ulonglong2 *>(&stup[size_t(i) * 2]) = make_ulonglong2(key[u], r.vw[0][u]);
            } else {
                stup[size_t(i) * TW] = key[u];
#pragma unroll
                for (int j = 0; j < NVT; ++j) stup[size_t(i) * TW + 1 + j] = r.vw[j][u];
            }
        }
        if (base + SC_ROWS < hi) load(next, base + SC_ROWS); // workgroup-uniform: the next tile's words fly during the copy-out
        __syncthreads();
        SLAB_STAMP(2); // tuples to LDS, next tile's loads issued
        for (uint32_t i = threadIdx.x; i < tile_total; i += blockDim.x) {
            uint64_t k, v0 = 0, v1 = 0;
            if (TW == 2) {
                const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(&stup[size_t(i) * 2]);
                k = t.x;
                v0 = t.y;
            } else {
                k = stup[size_t(i) * TW];
                v0 = stup[size_t(i) * TW + 1];
                if (NVT > 1) v1 = stup[size_t(i) * TW + 2];
            }
            const uint32_t p = hash_partition(k, parts_log2);
            const uint32_t at = gcur[p] + (i - tstart[p]);
            if (at < cap) {
                uint64_t *dst = sa.slabs + ((size_t(blockIdx.x) * size_t(parts) + p) * size_t(cap) + at) * TW;
                if (TW == 2) {
                    *reinterpret_cast<ulonglong2 *>(dst) = make_ulonglong2(k, v0);
                } else {
                    dst[0] = k;
                    dst[1] = v0;
                    if (NVT > 1) dst[2] = v1;
                }
            } else {
                atomicOr(&flags[NQE_FLAG_SLAB_OVERFLOW], 1); // skewed keys: the host redoes the query with exact partition sizes
            }
        }
        __syncthreads();
        SLAB_STAMP(3); // copy-out
        if (int(threadIdx.x) < parts) {
            gcur[threadIdx.x] += tcnt[threadIdx.x];
            tcnt[threadIdx.x] = 0;
        }
        __syncthreads();
        SLAB_STAMP(4); // cursors
    };
    if (lo < hi) {
        Regs A, B;
        load(A, lo);
        for (int64_t base = lo; base < hi; base += 2 * int64_t(SC_ROWS)) {
            tile(A, B, base);
            if (base + SC_ROWS >= hi) break;
            tile(B, A, base + SC_ROWS);
        }
    }
    for (int p = threadIdx.x; p < parts; p += blockDim.x) sa.fill[size_t(p) * size_t(sa.W) + blockIdx.x] = gcur[p] < cap ? gcur[p] : cap;
#ifdef NQE_SLAB_PROFILE
    if (threadIdx.x == 0) {
        for (int i = 0; i < 5; ++i) atomicAdd(&nqe_slab_prof[i], prof_acc[i]);
        atomicAdd(&nqe_slab_prof[7], 1ull);
    }
#endif
}

// ------------------------------------------------------------------ the K32 scatter with WHOLE-LINE stores (round 5)
// tools/scatter_bench.hip: what the 12-byte-record scatter above pays for is not its 256 streams but the shape of its stores — runs
// of ~32 records that start and end anywhere, plain stores (a non-temporal store of a PARTIAL line is far worse: 1.1 ms), 0.70-0.83 ms
// per 10^8 rows at 256 partitions where separate value / key streams written in whole aligned lines with non-temporal stores take
// 0.57.  So the slab of (workgroup, partition) is two arrays — cap 8-byte values, then (behind every slab's values) cap 4-byte keys —
// and a slab only ever receives whole BLOCKS of 16 tuples (8 with 512 partitions): one 128-byte line of values + 64 bytes of keys per
// block, written by 16 consecutive lanes.  What a tile leaves over per partition (< 16 tuples) waits in an LDS carry buffer and leads
// the partition's next block.  Per tile: rank the rows per partition (LDS atomic), scan the counts and the block counts, stage the
// tuples by partition, copy out whole blocks — a block's tuples come from the carry buffer first, then from the stage — move the
// leftovers to the carry buffer, advance the cursors.  The last, partial block of every partition is written when the chunk ends.
// (Run length no longer matters — every store is a whole block — so neither does the tile size; the tile stays 8 rows per thread where
// the registers allow two tiles in flight.)  Key as stored: key - range_min under key-range partitions, else the key's low 32 bits
// (a key outside int32 raises NQE_FLAG_KEY32_OVERFLOW as before).
// THREADS: 512 (two workgroups per CU: their barrier phases overlap, as the staged compaction's do) or 1024.  The LDS layout follows the
// partition count of the run: stage [THREADS x RPT], carry [parts x block], five counters per partition, the block owner map.
template <int PRED, int KEY, int THREADS>
__global__ void __launch_bounds__(THREADS) agg_slab_scatter_soa_kernel(AggArgs a, FastPred fp, SlabArgs sa, int *flags) {
    constexpr int RPT = SOA_RPT;
    constexpr int SC_ROWS = THREADS * RPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int parts_log2 = sa.parts_log2, parts = 1 << parts_log2;
    const SoaScatterLayout L(SC_ROWS, parts_log2);
    const int blk_log2 = SoaScatterLayout::block_log2(parts_log2), blk = 1 << blk_log2;
    uint64_t *sval = reinterpret_cast<uint64_t *>(smem + L.sval());     // [SC_ROWS] the tile's values by partition
    uint64_t *cval = reinterpret_cast<uint64_t *>(smem + L.cval());     // [carry]
    uint32_t *skey = reinterpret_cast<uint32_t *>(smem + L.skey());     // [SC_ROWS]
    uint32_t *ckey = reinterpret_cast<uint32_t *>(smem + L.ckey());     // [carry]
    uint32_t *gblk = reinterpret_cast<uint32_t *>(smem + L.gblk());     // [parts] blocks this workgroup has written per partition
    uint32_t *ccnt = reinterpret_cast<uint32_t *>(smem + L.ccnt());     // [parts] tuples in the carry buffer
    uint32_t *tcnt = reinterpret_cast<uint32_t *>(smem + L.tcnt());     // [parts] tuples of this tile
    uint32_t *tstart = reinterpret_cast<uint32_t *>(smem + L.tstart()); // [parts] tile-local exclusive scan of tcnt
    uint32_t *bstart = reinterpret_cast<uint32_t *>(smem + L.bstart()); // [parts] exclusive scan of the blocks this tile completes
    uint16_t *bown = reinterpret_cast<uint16_t *>(smem + L.bown());     // [SC_ROWS / 8 + parts] partition of each such block
    __shared__ uint32_t wave_tot[2][THREADS / 64];
    const bool range_part = sa.range_span != 0;
    for (int p = threadIdx.x; p < parts; p += blockDim.x) gblk[p] = ccnt[p] = tcnt[p] = 0;
    __syncthreads();
    const RowSource<PRED, 1> src(a, sa.chunk);
    const int64_t lo = src.lo, hi = src.hi;
    const uint32_t cap = uint32_t(sa.cap);
    // this workgroup's slabs: values of (w, p) at vbase + p * cap, keys at kbase + p * cap
    uint64_t *__restrict__ vbase = sa.slabs + size_t(blockIdx.x) * size_t(parts) * size_t(cap);
    uint32_t *__restrict__ kbase = reinterpret_cast<uint32_t *>(sa.slabs + size_t(sa.W) * size_t(parts) * size_t(cap)) + size_t(blockIdx.x) * size_t(parts) * size_t(cap);
    typedef RowRegs<PRED, 1, RPT> Regs;
    auto load = [&](Regs &r, int64_t base) { src.template load<RPT, THREADS>(fp, r, base); };
    // tuple j of partition p's pending sequence: the carried tuples first, then the tile's
    // (one index into sval / skey — the carry buffers lie right behind the stages: a selected POINTER sends the pointers to scratch memory)
    auto pending = [&](uint32_t p, uint32_t j, uint32_t cc, uint64_t &v, uint32_t &k) {
        const uint32_t i = j < cc ? uint32_t(SC_ROWS) + (p << blk_log2) + j : tstart[p] + (j - cc);
        v = sval[i];
        k = skey[i];
    };
    auto tile = [&](const Regs &r, Regs &next, int64_t base) {
        uint32_t k32[RPT], part[RPT], rank[RPT];
        bool pass[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            bool ok = src.passes(a, fp, r, u, base + int64_t(u) * THREADS + threadIdx.x);
            const uint64_t key = src.template key<KEY>(a, r.kw[u]);
            if (range_part) { // (wave-uniform choice) a key outside the range: the host redoes the query hashed
                const uint64_t d = key - uint64_t(sa.range_min);
                if (ok && d >= sa.range_span) {
                    atomicOr(&flags[NQE_FLAG_OOB], 1);
                    ok = false;
                }
                part[u] = range_partition(d, parts_log2);
                k32[u] = uint32_t(d);
            } else {
                part[u] = hash_partition(key, parts_log2);
                k32[u] = uint32_t(key);
                if (ok && int64_t(int32_t(uint32_t(key))) != int64_t(key)) atomicOr(&flags[NQE_FLAG_KEY32_OVERFLOW], 1);
            }
            pass[u] = ok;
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) rank[u] = pass[u] ? atomicAdd(&tcnt[part[u]], 1u) : 0u;
        __syncthreads();
        // threads 0..parts-1: exclusive scans of the tile's counts and of the blocks the tile completes
        uint32_t c = 0, nb = 0;
        if (int(threadIdx.x) < parts) {
            c = tcnt[threadIdx.x];
            nb = (ccnt[threadIdx.x] + c) >> blk_log2;
        }
        uint32_t wt0, wt1;
        const uint32_t ex0 = wave_exclusive_scan(c, wt0), ex1 = wave_exclusive_scan(nb, wt1);
        if (lane_id() == 63) {
            wave_tot[0][threadIdx.x / 64] = wt0;
            wave_tot[1][threadIdx.x / 64] = wt1;
        }
        __syncthreads();
        uint32_t nblocks = 0;
        {
            uint32_t pre0 = 0, pre1 = 0;
            for (int w = 0; w < THREADS / 64; ++w) {
                if (w < int(threadIdx.x) / 64) {
                    pre0 += wave_tot[0][w];
                    pre1 += wave_tot[1][w];
                }
                nblocks += wave_tot[1][w];
            }
            if (int(threadIdx.x) < parts) {
                tstart[threadIdx.x] = pre0 + ex0;
                bstart[threadIdx.x] = pre1 + ex1;
                for (uint32_t b = 0; b < nb; ++b) bown[pre1 + ex1 + b] = uint16_t(threadIdx.x);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            if (!pass[u]) continue;
            const uint32_t i = tstart[part[u]] + rank[u];
            sval[i] = r.vw[0][u];
            skey[i] = k32[u];
        }
        if (base + SC_ROWS < hi) load(next, base + SC_ROWS); // workgroup-uniform: the next tile's words fly during the copy-out
        __syncthreads();
        // whole blocks: 2^blk_log2 consecutive lanes write one block — a 128-byte line of values and 64 bytes of keys
        for (uint32_t t = threadIdx.x; t < (nblocks << blk_log2); t += blockDim.x) {
            const uint32_t b = t >> blk_log2, l = t & uint32_t(blk - 1), p = bown[b];
            const uint32_t j = ((b - bstart[p]) << blk_log2) + l, at = (gblk[p] << blk_log2) + j;
            uint64_t v;
            uint32_t k;
            pending(p, j, ccnt[p], v, k);
            if (at < cap) {
                __builtin_nontemporal_store(v, vbase + size_t(p) * cap + at);
                __builtin_nontemporal_store(k, kbase + size_t(p) * cap + at);
            } else
                atomicOr(&flags[NQE_FLAG_SLAB_OVERFLOW], 1); // skewed keys: the host redoes the query with exact partition sizes
        }
        __syncthreads();
        // leftovers to the carry buffer (a partition that completed a block consumed its carry: the leftovers are the tile's own)
        for (uint32_t t = threadIdx.x; t < uint32_t(parts << blk_log2); t += blockDim.x) {
            const uint32_t p = t >> blk_log2, l = t & uint32_t(blk - 1);
            const uint32_t cc = ccnt[p], tot = cc + tcnt[p], nbp = tot >> blk_log2, rem = tot & uint32_t(blk - 1);
            const uint32_t j = (nbp << blk_log2) + l;
            if (l < rem && j >= cc) {
                uint64_t v;
                uint32_t k;
                pending(p, j, cc, v, k);
                cval[(p << blk_log2) + l] = v;
                ckey[(p << blk_log2) + l] = k;
            }
        }
        __syncthreads();
        if (int(threadIdx.x) < parts) {
            const uint32_t tot = ccnt[threadIdx.x] + tcnt[threadIdx.x];
            gblk[threadIdx.x] += tot >> blk_log2;
            ccnt[threadIdx.x] = tot & uint32_t(blk - 1);
            tcnt[threadIdx.x] = 0;
        }
        __syncthreads();
    };
    if (lo < hi) {
        Regs A, B;
        load(A, lo);
        for (int64_t base = lo; base < hi; base += 2 * int64_t(SC_ROWS)) {
            tile(A, B, base);
            if (base + SC_ROWS >= hi) break;
            tile(B, A, base + SC_ROWS);
        }
    }
    // the last, partial block of every partition; the fill counts
    for (uint32_t t = threadIdx.x; t < uint32_t(parts << blk_log2); t += blockDim.x) {
        const uint32_t p = t >> blk_log2, l = t & uint32_t(blk - 1), at = (gblk[p] << blk_log2) + l;
        if (l < ccnt[p]) {
            if (at < cap) {
                vbase[size_t(p) * cap + at] = cval[(p << blk_log2) + l];
                kbase[size_t(p) * cap + at] = ckey[(p << blk_log2) + l];
            } else
                atomicOr(&flags[NQE_FLAG_SLAB_OVERFLOW], 1);
        }
    }
    for (int p = threadIdx.x; p < parts; p += blockDim.x) {
        const uint32_t n = (gblk[p] << blk_log2) + ccnt[p];
        sa.fill[size_t(p) * size_t(sa.W) + blockIdx.x] = n < cap ? n : cap;
    }
}

// one workgroup per partition (grid-stride); its waves take the partition's slabs round-robin and stream their tuples, four
// per lane per step, into the workgroup's LDS table with the batched update of the fast kernel (all first probes, then all
// min/max reads of the step in flight together — tuples of a partition arrive in no particular order, every row is an update).
template <int NVT, bool VF64, bool K32 = false>
__global__ void __launch_bounds__(AGG_BLOCK) agg_slab_segments_kernel(AggArgs a, SlabArgs sa, GroupTable g, int *flags) {
    constexpr int SU = 4; // tuples per lane per step
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const HashedTable<NVT> tab(smem, uint32_t(a.lds_cap));
    const uint32_t cap = tab.cap, slots = tab.slots;
    uint64_t *const lkeys = tab.lkeys;
    double *const lsum = tab.lsum;
    uint64_t *const lmn = tab.lmn, *const lmx = tab.lmx;
    uint32_t *const lcnt = tab.lcnt;
    int vdt[NVT];
#pragma unroll
    for (int j = 0; j < NVT; ++j) vdt[j] = a.val[j].dtype;
    __shared__ int seg_full_flag;
    const int wave = int(threadIdx.x) / 64, nwaves = AGG_BLOCK / 64;
    const int parts_log2 = sa.parts_log2, parts = 1 << parts_log2;
    for (int p = blockIdx.x; p < parts; p += gridDim.x) {
        __syncthreads();
        if (__hip_atomic_load(&flags[NQE_FLAG_NEED_LEVEL2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        if (threadIdx.x == 0) seg_full_flag = 0;
        tab.init();
        __syncthreads();
        const int nl = (sa.W - wave + nwaves - 1) / nwaves; // slabs of this wave: w = wave, wave + 16, ... (<= 64: W <= 1024)
        auto update = [&](const SlabStep<NVT, K32, SU> &st) {
            uint64_t skey[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) skey[u] = K32 ? uint64_t(int64_t(st.k32[K32 ? u : 0])) : st.key[K32 ? 0 : u];
            // ---- slots: every first probe issued before any is examined
            uint32_t s0[SU];
            uint64_t k0[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                s0[u] = tab.home(skey[u], parts_log2, a.lds_shift);
                k0[u] = lkeys[s0[u]];
            }
            int slot[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                slot[u] = -1;
                if (!st.live[u]) continue;
                const uint64_t key = skey[u];
                if (key == EMPTY_KEY) {
                    lkeys[cap] = 0;
                    slot[u] = int(cap);
                } else if (k0[u] == key) {
                    slot[u] = int(s0[u]);
                } else if (!SEG_FULL()) {
                    slot[u] = tab.probe(s0[u], key);
                }
                if (slot[u] < 0 && !SEG_FULL()) { // more distinct keys than the table: the host partitions one level deeper (exact form)
                    SEG_FULL_SET();
                    atomicOr(&flags[NQE_FLAG_NEED_LEVEL2], 1);
                }
            }
            // ---- read-before-atomic, the step's rows in flight together
            uint64_t cmn[NVT][SU], cmx[NVT][SU];
#pragma unroll
            for (int j = 0; j < NVT; ++j) {
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    const uint32_t o = uint32_t(j) * slots + uint32_t(slot[u] < 0 ? 0 : slot[u]);
                    cmn[j][u] = lmn[o];
                    cmx[j][u] = lmx[o];
                }
            }
#pragma unroll
            for (int j = 0; j < NVT; ++j) {
#pragma unroll
                for (int u = 0; u < SU; ++u) {
                    if (slot[u] < 0) continue;
                    const double x = VF64 ? u2d(st.vw[j][u]) : word_as_f64(st.vw[j][u], vdt[j]);
                    const bool isn = x != x;
                    const uint64_t xo = f64_to_ord(x);
                    const uint32_t o = uint32_t(j) * slots + uint32_t(slot[u]);
                    atomicAdd(&lcnt[o], 1u);
                    unsafeAtomicAdd(&lsum[o], x);
                    if (isn) atomicOr(&lcnt[o], NAN_BIT);
                    else {
                        if (xo < cmn[j][u]) atomicMin((unsigned long long *)&lmn[o], (unsigned long long)xo);
                        if (xo > cmx[j][u]) atomicMax((unsigned long long *)&lmx[o], (unsigned long long)xo);
                    }
                }
            }
        };
        stream_slabs<NVT, K32, SU>(sa, p, nl, [&](int l) { return wave + l * nwaves; }, update);
        __syncthreads();
        if (SEG_FULL()) break; // result discarded
        if (g.dense_count) emit_dense(tab, g, a.v0, flags);
        else tab.flush_to_global(g, a.v0, flags);
    }
}

// Key-range partitions (SlabArgs::range_span != 0; one value column, 12-byte tuples): the table of partition p is addressed by
// (key - range_min) >> parts_log2 — no hash, no probe sequence, no key words, no overflow; the key of a slot is rebuilt from (p, slot);
// min / max are doubles behind ordered compares (native LDS f64 atomics).  The hashed kernel above spends ~75 instructions
// per tuple (64-bit multiply, probe, compare, ordered-integer min / max); this one a dozen.  Same tuple stream (a wave's slabs as one
// sequence of 256-tuple steps, the next step requested before the current one is processed), same dense output.
template <bool VF64>
__global__ void __launch_bounds__(AGG_BLOCK) agg_slab_segments_direct_kernel(AggArgs a, SlabArgs sa, GroupTable g, int *flags) {
    constexpr int SU = DIRECT_SU; // tuples per lane per step
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    RangeTable tab(smem, sa);
    const int vdt = a.val[0].dtype;
    const int wave = int(threadIdx.x) / 64, nwaves = AGG_BLOCK / 64;
    const int parts = 1 << sa.parts_log2;
    for (int p = blockIdx.x; p < parts; p += gridDim.x) {
        __syncthreads();
        tab.init();
        __syncthreads();
        const int nl = (sa.W - wave + nwaves - 1) / nwaves; // slabs of this wave (<= 64: W <= 1024)
        stream_slabs<1, true, SU>(sa, p, nl, [&](int l) { return wave + l * nwaves; }, [&](const SlabStep<1, true, SU> &st) { tab.template update<VF64>(st, vdt); });
        __syncthreads();
        tab.p = p;
        emit_dense(tab, g, a.v0, flags);
    }
}

// The range tier's second kernel (aggregate_common.hpp: RangeRec): workgroup (p, q) = blockIdx / Q, blockIdx % Q streams the slabs
// w = q, q + Q, q + 2Q, ... of partition p into its LDS table (agg_slab_segments_direct_kernel's tuple stream and update) and writes
// the whole table to tab[(p * Q + q) * W + slot].
template <bool VF64>
__global__ void __launch_bounds__(AGG_BLOCK) agg_range_segments_kernel(AggArgs a, SlabArgs sa, int Q, RangeRec *__restrict__ tab_out) {
    constexpr int SU = DIRECT_SU; // tuples per lane per step
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RangeTable tab(smem, sa);
    const uint32_t W = tab.W;
    const int vdt = a.val[0].dtype;
    const int wave = int(threadIdx.x) / 64, nwaves = AGG_BLOCK / 64;
    const int p = int(blockIdx.x) / Q, q = int(blockIdx.x) % Q;
    tab.init();
    __syncthreads();
    const int nq = (sa.W - q + Q - 1) / Q;               // slabs of this workgroup: w = q + Q * j, j < nq
    const int nl = nq > wave ? (nq - wave + nwaves - 1) / nwaves : 0; // ... of this wave: j = wave + l * nwaves (<= 64: W <= 1024)
    stream_slabs<1, true, SU>(sa, p, nl, [&](int l) { return q + Q * (wave + l * nwaves); }, [&](const SlabStep<1, true, SU> &st) { tab.template update<VF64>(st, vdt); });
    __syncthreads();
    RangeRec *__restrict__ mine = tab_out + size_t(blockIdx.x) * size_t(W);
    for (uint32_t s = threadIdx.x; s < W; s += blockDim.x) {
        RangeRec r;
        r.sum = tab.lsum[s];
        r.mn = tab.lmn[s];
        r.mx = tab.lmx[s];
        r.cnt = uint64_t(tab.lcnt[s] & ~NAN_BIT) | ((tab.lcnt[s] & NAN_BIT) ? NAN_BIT64 : 0ull); // (one workgroup's rows of a pass: below 2^31)
        mine[s] = r;
    }
}

// ------------------------------------------------------------------ pickers
// every (pred, key) picker goes through here: f(PRED, KEY) with the two as integral constants
template <int I> using Int = std::integral_constant<int, I>;
template <class F> auto with_pred_key(int pred, int key, F f) {
    auto with_key = [&](auto P) {
        switch (key) {
        case 0: return f(P, Int<0>());
        case 1: return f(P, Int<1>());
        case 2: return f(P, Int<2>());
        default: return f(P, Int<3>());
        }
    };
    switch (pred) {
    case 0: return with_key(Int<0>());
    case 1: return with_key(Int<1>());
    case 2: return with_key(Int<2>());
    default: return with_key(Int<3>());
    }
}

} // namespace

PartKernel pick_part_kernel(int pred, int key) {
    return with_pred_key(pred, key, [](auto P, auto K) -> PartKernel { return agg_partition_kernel<decltype(P)::value, decltype(K)::value>; });
}
PartKernel pick_scatter_kernel(int pred, int key, int nv) {
    return with_pred_key(pred, key, [&](auto P, auto K) -> PartKernel {
        constexpr int PR = decltype(P)::value, KE = decltype(K)::value;
        return nv == 1 ? agg_partition_scatter_kernel<PR, KE, 1> : agg_partition_scatter_kernel<PR, KE, 2>;
    });
}
SlabScatterKernel pick_slab_scatter_kernel(int pred, int key, int nv, bool k32) {
    return with_pred_key(pred, key, [&](auto P, auto K) -> SlabScatterKernel {
        constexpr int PR = decltype(P)::value, KE = decltype(K)::value;
        if (nv == 1 && k32) return agg_slab_scatter_soa_kernel<PR, KE, SOA_THREADS>; // (two workgroups per CU: aggregate_common.hpp)
        return nv == 1 ? agg_slab_scatter_kernel<PR, KE, 1> : agg_slab_scatter_kernel<PR, KE, 2>;
    });
}
SlabSegmentsKernel pick_slab_segments_kernel(int nv, bool vf64, bool k32) {
    if (nv == 1 && k32) return vf64 ? agg_slab_segments_kernel<1, true, true> : agg_slab_segments_kernel<1, false, true>;
    return nv == 1 ? (vf64 ? agg_slab_segments_kernel<1, true> : agg_slab_segments_kernel<1, false>)
                   : (vf64 ? agg_slab_segments_kernel<2, true> : agg_slab_segments_kernel<2, false>);
}
RangeSegmentsKernel pick_range_segments_kernel(bool vf64) { return vf64 ? agg_range_segments_kernel<true> : agg_range_segments_kernel<false>; }
SlabSegmentsKernel pick_slab_segments_direct_kernel(bool vf64) { return vf64 ? agg_slab_segments_direct_kernel<true> : agg_slab_segments_direct_kernel<false>; }
SubpartitionKernel pick_subpartition_kernel(int nv) { return nv == 1 ? agg_subpartition_kernel<1> : agg_subpartition_kernel<2>; }
SegmentsKernel pick_segments_kernel(int nv, bool vf64) {
    return nv == 1 ? (vf64 ? agg_segments_kernel<1, true> : agg_segments_kernel<1, false>) : (vf64 ? agg_segments_kernel<2, true> : agg_segments_kernel<2, false>);
}

} // namespace agg
} // namespace nqe

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE((nqe::agg::agg_slab_segments_kernel<1, true, false>));

#ifdef NQE_SLAB_PROFILE
extern "C" void nqe_debug_slab_profile(unsigned long long *out) { // reads and clears the phase clocks
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(nqe::agg::nqe_slab_prof), sizeof(z));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(nqe::agg::nqe_slab_prof), z, sizeof(z));
}
#endif
