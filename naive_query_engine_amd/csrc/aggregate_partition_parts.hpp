// aggregate_partition_parts.hpp — the mechanisms the partitioned aggregate's kernels share, each defined once (included by
// aggregate_partition.hip alone): the row source of the count / scatter kernels, the tile-local scan of the scatters, the
// workgroup tables of the second-stage kernels (hashed and key-range) with their dense output, and the slab tuple stream.
// The dynamic-LDS layouts are aggregate_partition_layout.hpp's.
#pragma once
#include "aggregate_common.hpp"

namespace nqe {
namespace agg {
namespace {

__device__ __forceinline__ uint32_t hash_partition(uint64_t key, int parts_log2) { return uint32_t((key * GOLD) >> (64 - parts_log2)); }

// ------------------------------------------------------------------ row source (count and scatter kernels)
// the words of one row: key, predicate (PRED >= 2: a column of its own) and NVT value columns
template <int NVT> struct RowWords {
    uint64_t kw, pw, vw[NVT ? NVT : 1];
};
// ... of a register tile, RPT rows per thread
template <int PRED, int NVT, int RPT> struct RowRegs {
    uint64_t kw[RPT], pw[PRED >= 2 ? RPT : 1], vw[NVT ? NVT : 1][RPT];
};

// The input columns of workgroup `blockIdx.x`'s chunk of rows [lo, hi).  PRED: 0 none, 1 a range test of the key column's word, 2 a
// range test of another column (FastPred says how its word is found and cut), 3 an interpreted chain over another column's word
// (host-vetted: cannot fault).  KEY: inline_key's.
template <int PRED, int NVT> struct RowSource {
    const uint64_t *__restrict__ keyp, *__restrict__ predp, *__restrict__ valp[NVT ? NVT : 1];
    uint64_t key_mask;
    OpAux key_aux;
    bool key_signed;
    int64_t lo, hi, last;

    __device__ __forceinline__ RowSource(const AggArgs &a, int64_t chunk) {
        keyp = static_cast<const uint64_t *>(a.key_src.values);
        predp = static_cast<const uint64_t *>(PRED >= 2 ? a.pred_src.values : a.key_src.values);
#pragma unroll
        for (int j = 0; j < NVT; ++j) valp[j] = static_cast<const uint64_t *>(a.val[j].values);
        key_mask = a.key.aux[0].abs_lit - 1;
        key_aux = a.key.aux[0];
        key_signed = a.key.op_dtype[0] == NQE_INT64;
        lo = int64_t(blockIdx.x) * chunk;
        hi = lo + chunk < a.n ? lo + chunk : a.n;
        last = a.n - 1;
    }
    // the words of row `row`, clamped to the last row: unconditional, in-bounds, non-temporal (pw: PRED >= 2 only)
    __device__ __forceinline__ RowWords<NVT> load_row(const FastPred &fp, int64_t row) const {
        RowWords<NVT> w;
        row = row < last ? row : last;
        w.kw = __builtin_nontemporal_load(&keyp[row]);
        w.pw = PRED == 2 ? __builtin_nontemporal_load(&predp[row >> fp.row_shift]) : (PRED == 3 ? __builtin_nontemporal_load(&predp[row]) : 0);
#pragma unroll
        for (int j = 0; j < NVT; ++j) w.vw[j] = __builtin_nontemporal_load(&valp[j][row]);
        return w;
    }
    // a whole tile: rows base + u * THREADS + threadIdx.x
    template <int RPT, int THREADS> __device__ __forceinline__ void load(const FastPred &fp, RowRegs<PRED, NVT, RPT> &r, int64_t base) const {
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const RowWords<NVT> w = load_row(fp, base + int64_t(u) * THREADS + threadIdx.x);
            r.kw[u] = w.kw;
            r.pw[PRED >= 2 ? u : 0] = w.pw;
#pragma unroll
            for (int j = 0; j < NVT; ++j) r.vw[j][u] = w.vw[j];
        }
    }
    // row `row`, whose key and predicate words are kw and pw, lies in the chunk and passes the predicate
    __device__ __forceinline__ bool passes(const AggArgs &a, const FastPred &fp, uint64_t kw, uint64_t pw, int64_t row) const {
        bool ok = row < hi;
        if (PRED == 3) ok = ok && eval_simple<false>(a.pred, pw, false, nullptr) != 0;
        else if (PRED == 2) ok = ok && range_pass(fp, pred_extract(fp, pw, row < last ? row : last));
        else if (PRED == 1) ok = ok && range_pass(fp, kw);
        return ok;
    }
    template <int RPT> __device__ __forceinline__ bool passes(const AggArgs &a, const FastPred &fp, const RowRegs<PRED, NVT, RPT> &r, int u, int64_t row) const {
        return passes(a, fp, r.kw[u], r.pw[PRED >= 2 ? u : 0], row);
    }
    template <int KEY> __device__ __forceinline__ uint64_t key(const AggArgs &a, uint64_t kw) const { return inline_key<KEY>(a.key, kw, key_mask, key_aux, key_signed); }
};

// ------------------------------------------------------------------ tile-local scan
// exclusive scan of the tile's per-partition counters by threads 0..parts-1 (parts <= PARTS) into tstart; returns the tile's total.
// wave_tot: PARTS / 64 words of LDS.  Every thread of the workgroup calls it (two barriers).
__device__ __forceinline__ uint32_t tile_scan(const uint32_t *tcnt, uint32_t *tstart, uint32_t *wave_tot, int parts) {
    uint32_t c = int(threadIdx.x) < parts ? tcnt[threadIdx.x] : 0u, wt;
    uint32_t ex = wave_exclusive_scan(c, wt);
    if (lane_id() == 63) wave_tot[threadIdx.x / 64] = wt;
    __syncthreads();
    if (int(threadIdx.x) < parts) {
        uint32_t pre = 0;
        for (int w = 0; w < int(threadIdx.x) / 64; ++w) pre += wave_tot[w];
        tstart[threadIdx.x] = pre + ex;
    }
    uint32_t tile_total = 0;
    for (int w = 0; w < PARTS / 64; ++w) tile_total += wave_tot[w];
    __syncthreads();
    return tile_total;
}

// ------------------------------------------------------------------ dense output of a workgroup table
// Count the table's groups, reserve [base, base + n) of the global table with ONE atomic, write them at their rank.  T: nslots(),
// occupied(s), key_of(s), and per value column j < T::NV the state at(j, s) -> cnt / sum / ord_mn / ord_mx.  Every thread calls it.
template <class T> __device__ __forceinline__ void emit_dense(const T &t, const GroupTable &g, int v0, int *flags) {
    __shared__ uint32_t wave_tot[AGG_BLOCK / 64];
    __shared__ uint32_t dense_base;
    const uint32_t n = t.nslots();
    uint32_t mine = 0;
    for (uint32_t s = threadIdx.x; s < n; s += blockDim.x) mine += t.occupied(s) ? 1u : 0u;
    uint32_t wtot;
    const uint32_t wexcl = wave_exclusive_scan(mine, wtot);
    if (lane_id() == 0) wave_tot[threadIdx.x / 64] = wtot;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < AGG_BLOCK / 64; ++w) { uint32_t c = wave_tot[w]; wave_tot[w] = tot; tot += c; }
        dense_base = tot ? atomicAdd(g.dense_count, tot) : 0u;
    }
    __syncthreads();
    uint32_t pos = dense_base + wave_tot[threadIdx.x / 64] + wexcl;
    const size_t gstride = size_t(g.cap) + 1;
    for (uint32_t s = threadIdx.x; s < n; s += blockDim.x) {
        if (!t.occupied(s)) continue;
        if (pos < g.cap) {
            g.keys[pos] = t.key_of(s);
#pragma unroll
            for (int j = 0; j < T::NV; ++j) {
                const uint32_t o = t.at(j, s);
                const uint32_t c = t.lcnt[o];
                const size_t go = size_t(v0 + j) * gstride + pos;
                g.cnt[go] = uint64_t(c & ~NAN_BIT);
                g.sum[go] = t.lsum[o];
                g.mn[go] = t.ord_mn(o);
                g.mx[go] = t.ord_mx(o);
                g.nan[go] = (c & NAN_BIT) ? 1u : 0u;
            }
        } else atomicOr(&flags[NQE_FLAG_DENSE_OVERFLOW], 1);
        ++pos;
    }
}

// ------------------------------------------------------------------ hashed workgroup table
// `cap` slots (a power of two) + slot [cap] for EMPTY_KEY itself; per value column sums, ordered mins / maxs, counts (NaN mark in the top
// bit).  The slot of a key uses the hash bits BELOW the partition bits: all keys of a partition share the top ones.
template <int NVT> struct HashedTable {
    static constexpr int NV = NVT;
    uint32_t cap, slots;
    uint64_t *lkeys;
    double *lsum;
    uint64_t *lmn, *lmx;
    uint32_t *lcnt;
    __device__ __forceinline__ HashedTable(unsigned char *smem, uint32_t cap_) : cap(cap_), slots(cap_ + 1) {
        lkeys = reinterpret_cast<uint64_t *>(smem);
        lsum = reinterpret_cast<double *>(lkeys + slots);
        lmn = reinterpret_cast<uint64_t *>(lsum + NVT * slots);
        lmx = lmn + NVT * slots;
        lcnt = reinterpret_cast<uint32_t *>(lmx + NVT * slots);
    }
    __device__ __forceinline__ void init() const {
        const uint64_t ORD_MAX = f64_to_ord(DBL_MAX), ORD_MIN = f64_to_ord(-DBL_MAX);
        for (uint32_t s = threadIdx.x; s < slots; s += blockDim.x) {
            lkeys[s] = EMPTY_KEY;
#pragma unroll
            for (int j = 0; j < NVT; ++j) {
                lsum[j * slots + s] = 0.0;
                lmn[j * slots + s] = ORD_MAX;
                lmx[j * slots + s] = ORD_MIN;
                lcnt[j * slots + s] = 0;
            }
        }
    }
    __device__ __forceinline__ uint32_t home(uint64_t key, int part_bits, int shift) const { return uint32_t(((key * GOLD) << part_bits) >> shift); }
    // the slot of `key` (not EMPTY_KEY), claimed if new, within 32 probes from `sl`; -1: the partition has more distinct keys than the table
    __device__ __forceinline__ int probe(uint32_t sl, uint64_t key) const {
        int slot = -1;
        for (int probe = 0; probe < 32; ++probe) {
            uint64_t k = lkeys[sl];
            if (k == key) { slot = int(sl); break; }
            if (k == EMPTY_KEY) {
                uint64_t old = atomicCAS((unsigned long long *)&lkeys[sl], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
                if (old == EMPTY_KEY || old == key) { slot = int(sl); break; }
            }
            sl = (sl + 1) & (cap - 1);
        }
        return slot;
    }
    __device__ __forceinline__ int find_or_insert(uint64_t key, int part_bits, int shift) const { return probe(home(key, part_bits, shift), key); }
    // every group into the global hashed table
    __device__ __forceinline__ void flush_to_global(const GroupTable &g, int v0, int *flags) const {
        for (uint32_t s = threadIdx.x; s < slots; s += blockDim.x) {
            uint64_t k = lkeys[s];
            if (k == EMPTY_KEY) continue;
            uint64_t key = (s == cap) ? EMPTY_KEY : k;
            int64_t gslot = global_find_or_insert(g, key, flags);
            if (gslot < 0) continue;
#pragma unroll
            for (int j = 0; j < NVT; ++j) {
                uint32_t o = uint32_t(j) * slots + s;
                uint32_t c = lcnt[o];
                global_update(g, gslot, v0 + j, uint64_t(c & ~NAN_BIT), lsum[o], true, lmn[o], lmx[o], true, (c & NAN_BIT) != 0);
            }
        }
    }
    // emit_dense's view
    __device__ __forceinline__ uint32_t nslots() const { return slots; }
    __device__ __forceinline__ bool occupied(uint32_t s) const { return lkeys[s] != EMPTY_KEY; }
    __device__ __forceinline__ uint64_t key_of(uint32_t s) const { return s == cap ? EMPTY_KEY : lkeys[s]; }
    __device__ __forceinline__ uint32_t at(int j, uint32_t s) const { return uint32_t(j) * slots + s; }
    __device__ __forceinline__ uint64_t ord_mn(uint32_t o) const { return lmn[o]; }
    __device__ __forceinline__ uint64_t ord_mx(uint32_t o) const { return lmx[o]; }
};

// ------------------------------------------------------------------ slab tuple stream
// SU tuples per lane of a 64-lane step.  K32 (one value column): the 12-byte two-array tuple; its key stays AS LOADED — widening it in
// fetch would make the fetch wait for its own loads
template <int NVT, bool K32, int SU> struct SlabStep {
    uint64_t key[K32 ? 1 : SU], vw[NVT][SU];
    int32_t k32[K32 ? SU : 1];
    bool live[SU];
};

// A wave streams partition p's tuples out of its nl slabs slab_of(0), slab_of(1), ... (nl <= 64; slab (w, p) holds sa.fill[p][w] tuples)
// as ONE flat sequence of 64 x SU-tuple steps, the next step's tuples requested before update(step) processes the current one (a slab is
// ~750 tuples = 3 steps; walking the slabs one at a time exposed the fill-count load and the first tuple load of every slab: 16
// dependent round trips per wave per partition).  Tuple formats: (1 + NVT) 64-bit words in one stream (16 bytes as one 128-bit load),
// or K32's two arrays — cap 8-byte values per slab, then (behind every slab's values) cap 4-byte keys: agg_slab_scatter_soa_kernel.
template <int NVT, bool K32, int SU, class SlabOf, class Update>
__device__ __forceinline__ void stream_slabs(const SlabArgs &sa, int p, int nl, SlabOf slab_of, Update update) {
    constexpr int TW = 1 + NVT;
    typedef SlabStep<NVT, K32, SU> Step;
    const int parts = 1 << sa.parts_log2;
    const uint32_t myfill = lane_id() < nl ? sa.fill[size_t(p) * size_t(sa.W) + size_t(slab_of(lane_id()))] : 0u;
    int cl = 0;       // current slab (index into the wave's list), wave-uniform
    uint32_t ci0 = 0; // first tuple of the current step
    auto seek = [&](int &l, uint32_t &i0) { // first position at or after (l, i0) that holds tuples; l == nl: none
        while (l < nl && i0 >= uint32_t(__builtin_amdgcn_readlane(int(myfill), l))) {
            ++l;
            i0 = 0;
        }
    };
    // `on` false: a dummy step (every tuple dead) over a position known to hold tuples — the prefetch of the step past the last is
    // issued unconditionally, because a conditional fetch makes the step's registers a phi and the copies that resolve it sit
    // right behind the loads (s_waitcnt vmcnt(0) before the CURRENT step is processed: no prefetch at all; seen in the ISA)
    auto fetch = [&](Step &st, int l, uint32_t i0, bool on) {
        const uint32_t f = uint32_t(__builtin_amdgcn_readlane(int(myfill), l));
        const size_t sbase = (size_t(slab_of(l)) * size_t(parts) + size_t(p)) * size_t(sa.cap); // first tuple of slab (w, p)
        const uint64_t *__restrict__ slab = sa.slabs + sbase * (K32 ? 1 : TW);
        const uint32_t *__restrict__ skeys = reinterpret_cast<const uint32_t *>(sa.slabs + size_t(sa.W) * size_t(parts) * size_t(sa.cap)) + sbase; // (K32)
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            const uint32_t i = i0 + uint32_t(u) * 64 + uint32_t(lane_id());
            st.live[u] = on && i < f;
            const uint32_t ic = i < f ? i : f - 1;
            if (K32) {
                st.k32[K32 ? u : 0] = int32_t(__builtin_nontemporal_load(skeys + ic));
                st.vw[0][u] = __builtin_nontemporal_load(slab + ic);
            } else if (TW == 2) {
                typedef unsigned long long v2u64 __attribute__((ext_vector_type(2)));
                const v2u64 t = __builtin_nontemporal_load(reinterpret_cast<const v2u64 *>(&slab[size_t(ic) * 2]));
                st.key[K32 ? 0 : u] = t.x;
                st.vw[0][u] = t.y;
            } else {
                st.key[K32 ? 0 : u] = slab[size_t(ic) * TW];
#pragma unroll
                for (int j = 0; j < NVT; ++j) st.vw[j][u] = slab[size_t(ic) * TW + 1 + j];
            }
        }
    };
    seek(cl, ci0);
    if (cl < nl) {
        const int fl = cl;
        const uint32_t fi0 = ci0;
        Step A, B;
        fetch(A, cl, ci0, true);
        for (;;) {
            int nlx = cl;
            uint32_t ni0 = ci0 + 64 * SU;
            seek(nlx, ni0);
            const bool more_b = nlx < nl;
            fetch(B, more_b ? nlx : fl, more_b ? ni0 : fi0, more_b);
            update(A);
            if (!more_b) break;
            cl = nlx;
            ci0 = ni0 + 64 * SU;
            seek(cl, ci0);
            const bool more_a = cl < nl;
            fetch(A, more_a ? cl : fl, more_a ? ci0 : fi0, more_a);
            update(B);
            if (!more_a) break;
        }
    }
}

// ------------------------------------------------------------------ key-range table
// The table of key-range partition p (SlabArgs::range_span != 0; one value column, 12-byte tuples holding key - range_min), addressed
// by the tuple's key >> parts_log2 — no hash, no probe sequence, no key words, no overflow; min / max are doubles behind ordered compares
// (native LDS f64 atomics).  W slots (<= 5120: the host checks); a slot is occupied when its count is not zero.
struct RangeTable {
    static constexpr int NV = 1;
    uint32_t W;
    double *lsum, *lmn, *lmx;
    uint32_t *lcnt;
    // (emit_dense rebuilds the key of a slot from these)
    int p, parts_log2;
    int64_t range_min;
    __device__ __forceinline__ RangeTable(unsigned char *smem, const SlabArgs &sa)
        : W(uint32_t((sa.range_span + (uint64_t(1) << sa.parts_log2) - 1) >> sa.parts_log2)), p(0), parts_log2(sa.parts_log2), range_min(sa.range_min) {
        const RangeTableLayout L(W);
        lsum = reinterpret_cast<double *>(smem + L.lsum());
        lmn = reinterpret_cast<double *>(smem + L.lmn());
        lmx = reinterpret_cast<double *>(smem + L.lmx());
        lcnt = reinterpret_cast<uint32_t *>(smem + L.lcnt());
    }
    __device__ __forceinline__ void init() const {
        for (uint32_t s = threadIdx.x; s < W; s += blockDim.x) {
            lsum[s] = 0.0;
            lmn[s] = DBL_MAX;
            lmx[s] = -DBL_MAX;
            lcnt[s] = 0;
        }
    }
    // a step's tuples, the min / max reads of all of them in flight together before the atomics
    template <bool VF64, int SU> __device__ __forceinline__ void update(const SlabStep<1, true, SU> &st, int vdt) const {
        uint32_t slot[SU];
        double x[SU], cmn[SU], cmx[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            slot[u] = st.live[u] ? uint32_t(st.k32[u]) >> parts_log2 : 0u; // the tuple holds key - range_min (< span: the scatter checked the range, so slot < W)
            x[u] = VF64 ? u2d(st.vw[0][u]) : word_as_f64(st.vw[0][u], vdt);
            cmn[u] = lmn[slot[u]];
            cmx[u] = lmx[slot[u]];
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
            if (!st.live[u]) continue;
            atomicAdd(&lcnt[slot[u]], 1u);
            unsafeAtomicAdd(&lsum[slot[u]], x[u]);
            if (x[u] != x[u]) atomicOr(&lcnt[slot[u]], NAN_BIT);
            else {
                if (x[u] < cmn[u]) unsafeAtomicMin(&lmn[slot[u]], x[u]);
                if (x[u] > cmx[u]) unsafeAtomicMax(&lmx[slot[u]], x[u]);
            }
        }
    }
    // emit_dense's view
    __device__ __forceinline__ uint32_t nslots() const { return W; }
    __device__ __forceinline__ bool occupied(uint32_t s) const { return lcnt[s] != 0; }
    __device__ __forceinline__ uint64_t key_of(uint32_t s) const {
        const int parts = 1 << parts_log2;
        return uint64_t(range_min + int64_t((uint64_t(s) << parts_log2) | uint64_t((uint32_t(p) ^ range_scramble(s, parts_log2)) & uint32_t(parts - 1))));
    }
    __device__ __forceinline__ uint32_t at(int, uint32_t s) const { return s; }
    __device__ __forceinline__ uint64_t ord_mn(uint32_t o) const { return f64_to_ord(lmn[o]); }
    __device__ __forceinline__ uint64_t ord_mx(uint32_t o) const { return f64_to_ord(lmx[o]); }
};

} // namespace
} // namespace agg
} // namespace nqe
