// window_kernels.hpp — the kernels of the window operator (window.hip; the host analysis: window_plan.hpp).
//
// Everything runs over the SORTED order (position i holds input row perm[i]).  A tile is WIN_TILE = 4096 consecutive positions, one
// workgroup of 256 threads, 16 consecutive positions per thread: a thread's piece of a bitmap is one uint16, its piece of the gathered
// value column 128 bytes read with 16-byte loads.  Both scans have the same three-launch shape — reduce every tile to a carry, scan the
// carries in ONE workgroup, rescan every tile with its carry-in — so kernel boundaries are the only synchronisation between workgroups:
// nothing here waits on a word another workgroup writes.
#pragma once

#include "device_utils.hpp"
#include "window_plan.hpp"

namespace nqe {
namespace {

constexpr double WIN_F64_MAX = 1.7976931348623157e308;

// ---- one workgroup's exclusive scan of one state per thread, in thread order.  S gives identity(), combine(earlier, later), up(s, d), and
// its combine is associative.  `lds`: WIN_THREADS / 64 states.  *total: the combination of all WIN_THREADS states, in every thread.
template <typename S> __device__ __forceinline__ S win_block_exclusive(const S &v, S *lds, S *total) {
    S x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const S y = S::up(x, d);
        if (lane_id() >= d) x = S::combine(y, x);
    }
    const int wave = int(threadIdx.x) >> 6;
    if (lane_id() == 63) lds[wave] = x;
    S excl = S::up(x, 1);
    if (lane_id() == 0) excl = S::identity();
    __syncthreads();
    S pre = S::identity(), tot = S::identity();
#pragma unroll
    for (int w = 0; w < WIN_THREADS / 64; ++w) {
        const S t = lds[w];
        if (w < wave) pre = S::combine(pre, t);
        tot = S::combine(tot, t);
    }
    __syncthreads(); // `lds` may be written again
    *total = tot;
    return S::combine(pre, excl);
}

// the bits of positions [base, base + 16) of a bitmap, those at or beyond n cleared (null bitmap: all ones)
__device__ __forceinline__ uint32_t win_bits16(const uint16_t *bm16, int64_t base, int64_t n) {
    const int64_t left = n - base;
    const uint32_t mask = left >= WIN_ITEMS ? 0xffffu : left <= 0 ? 0u : ((1u << int(left)) - 1u);
    return (bm16 ? uint32_t(bm16[base >> 4]) : 0xffffu) & mask;
}

// =============================================================================================== win_bounds
struct WinKeyCol {
    const uint64_t *words; // Int64 / UInt64 / Float64
    const uint8_t *bits;   // Boolean
    const int32_t *off;    // Utf8
    const uint8_t *data;
    const uint8_t *valid;  // null: no NULLs
    int dtype;
};
struct WinBoundsArgs {
    WinKeyCol key[2 * NQE_MAX_WINDOW_KEYS]; // the partition keys, then the order keys
    int num_partition, num_keys;
    const uint32_t *perm; // null: the identity
    int64_t n;
    uint64_t *part_start, *peer_start; // bitmaps over positions
};

// Float64 ties as OrderedFloat: every NaN one value, -0.0 as +0.0
__device__ __forceinline__ uint64_t win_f64_tie(uint64_t w) {
    if ((w & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return 0x7ff8000000000000ull;
    return w == 0x8000000000000000ull ? 0 : w;
}

// do rows r and q tie on this key?  Whether a NULL is present is decided first: NULL ties with NULL, whatever lies under it
__device__ __forceinline__ bool win_key_ties(const WinKeyCol &c, int64_t r, int64_t q) {
    if (c.valid) {
        const bool vr = get_bit(c.valid, r), vq = get_bit(c.valid, q);
        if (!vr || !vq) return vr == vq;
    }
    if (c.dtype == NQE_FLOAT64) return win_f64_tie(c.words[r]) == win_f64_tie(c.words[q]);
    if (c.dtype == NQE_BOOLEAN) return get_bit(c.bits, r) == get_bit(c.bits, q);
    if (c.dtype == NQE_UTF8) {
        const int64_t br = c.off[r], bq = c.off[q], len = int64_t(c.off[r + 1]) - br;
        if (len != int64_t(c.off[q + 1]) - bq) return false;
        for (int64_t j = 0; j < len; ++j)
            if (c.data[br + j] != c.data[bq + j]) return false;
        return true;
    }
    return c.words[r] == c.words[q];
}

// one thread per sorted position i: row perm[i] against row perm[i - 1] on every key; a wave writes one word of each bitmap
__global__ void __launch_bounds__(WIN_THREADS) win_bounds_kernel(WinBoundsArgs a) {
    const int64_t nwords = (a.n + 63) / 64;
    const int64_t waves = int64_t(gridDim.x) * (WIN_THREADS / 64);
    for (int64_t w = int64_t(blockIdx.x) * (WIN_THREADS / 64) + (int(threadIdx.x) >> 6); w < nwords; w += waves) { // (wave-uniform)
        const int64_t i = w * 64 + lane_id();
        bool part = false, peer = false;
        if (i < a.n) {
            if (i == 0) {
                part = peer = true;
            } else {
                const int64_t r = a.perm ? int64_t(a.perm[i]) : i, q = a.perm ? int64_t(a.perm[i - 1]) : i - 1;
                for (int k = 0; k < a.num_keys; ++k) {
                    if (!win_key_ties(a.key[k], r, q)) {
                        part = k < a.num_partition;
                        peer = true;
                        break;
                    }
                }
            }
        }
        const uint64_t bp = __ballot(part), be = __ballot(peer);
        if (lane_id() == 0) {
            a.part_start[w] = bp;
            a.peer_start[w] = be;
        }
    }
}

// =============================================================================================== positions from the bitmaps
// forward: the last partition start and the last peer start at or before a position (position 0 starts both, so 0 stands for "none
// yet"), and the number of peer starts so far
struct WinFwd {
    uint32_t part_first, peer_first, peers;
    static __device__ __forceinline__ WinFwd identity() { return WinFwd{0, 0, 0}; }
    static __device__ __forceinline__ WinFwd combine(const WinFwd &a, const WinFwd &b) {
        return WinFwd{max(a.part_first, b.part_first), max(a.peer_first, b.peer_first), a.peers + b.peers};
    }
    static __device__ __forceinline__ WinFwd up(const WinFwd &s, int d) {
        return WinFwd{__shfl_up(s.part_first, d, 64), __shfl_up(s.peer_first, d, 64), __shfl_up(s.peers, d, 64)};
    }
};
// backward (the same scan run from the other end): the nearest partition start and peer start AFTER a position; ~0 for "none"
struct WinBwd {
    uint32_t part_next, peer_next;
    static __device__ __forceinline__ WinBwd identity() { return WinBwd{~0u, ~0u}; }
    static __device__ __forceinline__ WinBwd combine(const WinBwd &a, const WinBwd &b) {
        return WinBwd{min(a.part_next, b.part_next), min(a.peer_next, b.peer_next)};
    }
    static __device__ __forceinline__ WinBwd up(const WinBwd &s, int d) { return WinBwd{__shfl_up(s.part_next, d, 64), __shfl_up(s.peer_next, d, 64)}; }
};
struct WinPosCarry {
    WinFwd fwd; // of tile t: after the carry scan, the state before the tile's first position
    WinBwd bwd; // after the carry scan, the state behind the tile's last position
};

struct WinPosArgs {
    const uint16_t *part_start, *peer_start;
    int64_t n, tiles;
    WinPosCarry *carry; // [tiles]; null with a single tile
    uint32_t *part_first, *peer_first, *peers, *peer_last, *part_last; // each [padded rows] or null: not wanted
};

__device__ __forceinline__ WinFwd win_fwd_of(uint32_t pbits, uint32_t ebits, int64_t base) {
    WinFwd s = WinFwd::identity();
    if (pbits) s.part_first = uint32_t(base) + (31 - __clz(int(pbits)));
    if (ebits) s.peer_first = uint32_t(base) + (31 - __clz(int(ebits)));
    s.peers = uint32_t(__popc(ebits));
    return s;
}
__device__ __forceinline__ WinBwd win_bwd_of(uint32_t pbits, uint32_t ebits, int64_t base) {
    WinBwd s = WinBwd::identity();
    if (pbits) s.part_next = uint32_t(base) + uint32_t(__ffs(int(pbits)) - 1);
    if (ebits) s.peer_next = uint32_t(base) + uint32_t(__ffs(int(ebits)) - 1);
    return s;
}

// the forward scan walks a tile's 16-position pieces in thread order, the backward scan in the opposite order
__global__ void __launch_bounds__(WIN_THREADS) win_pos_reduce_kernel(WinPosArgs a) {
    __shared__ WinFwd lf[WIN_THREADS / 64];
    __shared__ WinBwd lb[WIN_THREADS / 64];
    const int64_t tile0 = int64_t(blockIdx.x) * WIN_TILE;
    const int64_t fbase = tile0 + int64_t(threadIdx.x) * WIN_ITEMS, bbase = tile0 + int64_t(WIN_THREADS - 1 - threadIdx.x) * WIN_ITEMS;
    WinFwd ft;
    WinBwd bt;
    (void)win_block_exclusive(win_fwd_of(win_bits16(a.part_start, fbase, a.n), win_bits16(a.peer_start, fbase, a.n), fbase), lf, &ft);
    (void)win_block_exclusive(win_bwd_of(win_bits16(a.part_start, bbase, a.n), win_bits16(a.peer_start, bbase, a.n), bbase), lb, &bt);
    if (threadIdx.x == 0) a.carry[blockIdx.x] = WinPosCarry{ft, bt};
}

// ONE workgroup: the tiles' carries scanned forward (fwd) and from the last tile back (bwd), WIN_THREADS at a time
__global__ void __launch_bounds__(WIN_THREADS) win_pos_carry_kernel(WinPosArgs a) {
    __shared__ WinFwd lf[WIN_THREADS / 64];
    __shared__ WinBwd lb[WIN_THREADS / 64];
    WinFwd frun = WinFwd::identity();
    WinBwd brun = WinBwd::identity();
    for (int64_t c0 = 0; c0 < a.tiles; c0 += WIN_THREADS) { // (uniform over the workgroup)
        const int64_t f = c0 + threadIdx.x, b = a.tiles - 1 - f;
        const bool in = f < a.tiles;
        WinFwd ft;
        WinBwd bt;
        const WinFwd fe = win_block_exclusive(in ? a.carry[f].fwd : WinFwd::identity(), lf, &ft);
        const WinBwd be = win_block_exclusive(in ? a.carry[b].bwd : WinBwd::identity(), lb, &bt);
        if (in) {
            a.carry[f].fwd = WinFwd::combine(frun, fe);
            a.carry[b].bwd = WinBwd::combine(brun, be);
        }
        frun = WinFwd::combine(frun, ft);
        brun = WinBwd::combine(brun, bt);
    }
}

__device__ __forceinline__ void win_store16(uint32_t *dst, int64_t base, const uint32_t (&v)[WIN_ITEMS]) {
    uint4 *d = reinterpret_cast<uint4 *>(dst + base);
#pragma unroll
    for (int k = 0; k < WIN_ITEMS / 4; ++k) d[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}

__global__ void __launch_bounds__(WIN_THREADS) win_pos_apply_kernel(WinPosArgs a) {
    __shared__ WinFwd lf[WIN_THREADS / 64];
    __shared__ WinBwd lb[WIN_THREADS / 64];
    const int64_t tile0 = int64_t(blockIdx.x) * WIN_TILE;
    const uint32_t last = uint32_t(a.n - 1);
    uint32_t v[WIN_ITEMS];
    if (a.part_first || a.peer_first || a.peers) { // (kernel arguments: uniform)
        const int64_t base = tile0 + int64_t(threadIdx.x) * WIN_ITEMS;
        const uint32_t pbits = win_bits16(a.part_start, base, a.n), ebits = win_bits16(a.peer_start, base, a.n);
        WinFwd tot;
        WinFwd s = win_block_exclusive(win_fwd_of(pbits, ebits, base), lf, &tot);
        if (a.carry) s = WinFwd::combine(a.carry[blockIdx.x].fwd, s);
        uint32_t pf[WIN_ITEMS], ef[WIN_ITEMS];
#pragma unroll
        for (int k = 0; k < WIN_ITEMS; ++k) {
            if ((pbits >> k) & 1) s.part_first = uint32_t(base) + k;
            if ((ebits >> k) & 1) s.peer_first = uint32_t(base) + k, ++s.peers;
            pf[k] = s.part_first, ef[k] = s.peer_first, v[k] = s.peers;
        }
        if (a.part_first) win_store16(a.part_first, base, pf);
        if (a.peer_first) win_store16(a.peer_first, base, ef);
        if (a.peers) win_store16(a.peers, base, v);
    }
    if (a.peer_last || a.part_last) {
        const int64_t base = tile0 + int64_t(WIN_THREADS - 1 - threadIdx.x) * WIN_ITEMS;
        const uint32_t pbits = win_bits16(a.part_start, base, a.n), ebits = win_bits16(a.peer_start, base, a.n);
        WinBwd tot;
        WinBwd s = win_block_exclusive(win_bwd_of(pbits, ebits, base), lb, &tot);
        if (a.carry) s = WinBwd::combine(a.carry[blockIdx.x].bwd, s);
        uint32_t pl[WIN_ITEMS];
#pragma unroll
        for (int k = WIN_ITEMS - 1; k >= 0; --k) { // s: the nearest starts after position base + k (none: the order's last position ends both)
            pl[k] = s.part_next == ~0u ? last : s.part_next - 1;
            v[k] = s.peer_next == ~0u ? last : s.peer_next - 1;
            if ((pbits >> k) & 1) s.part_next = uint32_t(base) + k;
            if ((ebits >> k) & 1) s.peer_next = uint32_t(base) + k;
        }
        if (a.part_last) win_store16(a.part_last, base, pl);
        if (a.peer_last) win_store16(a.peer_last, base, v);
    }
}

// =============================================================================================== win_gather
// x[i] = the value of row perm[i] as f64 (Q10: every value is converted first), and its valid bit — one word per wave
__global__ void __launch_bounds__(WIN_THREADS) win_gather_kernel(const uint64_t *words, const uint8_t *valid, int dtype, const uint32_t *perm, int64_t n, double *x,
                                                                 uint64_t *valid_sorted) {
    const int64_t nwords = (n + 63) / 64;
    const int64_t waves = int64_t(gridDim.x) * (WIN_THREADS / 64);
    for (int64_t w = int64_t(blockIdx.x) * (WIN_THREADS / 64) + (int(threadIdx.x) >> 6); w < nwords; w += waves) { // (wave-uniform)
        const int64_t i = w * 64 + lane_id();
        bool ok = false;
        if (i < n) {
            const int64_t r = perm ? int64_t(perm[i]) : i;
            ok = !valid || get_bit(valid, r);
            x[i] = word_as_f64(words[r], dtype);
        }
        const uint64_t b = __ballot(ok);
        if (valid_sorted && lane_id() == 0) valid_sorted[w] = b;
    }
}

// =============================================================================================== win_scan: the segmented scan
// The state of a run of positions: did it see a partition start, and Q10's aggregates over its rows AFTER the last start it saw (over
// all its rows when it saw none).  combine(a, b), a before b, restarts at b when b saw a start — a true segmented scan: nothing of an
// earlier partition ever reaches a later one, neither an infinity nor a rounding error.
//   sum    f64 addition; a NULL adds 0.0                         count  valid rows (u32: fewer than 2^32 rows)
//   min    starts at f64::MAX, a NaN is skipped                   max    starts at f64::MIN, a NaN stays
template <int OPS> struct WinVal {
    uint32_t flag, count;
    double sum, mn, mx;
    static __device__ __forceinline__ WinVal identity() { return WinVal{0, 0, 0.0, WIN_F64_MAX, -WIN_F64_MAX}; }
    static __device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? u2d(0x7ff8000000000000ull) : fmax(a, b); }
    static __device__ __forceinline__ WinVal combine(const WinVal &a, const WinVal &b) {
        WinVal r = identity();
        r.flag = a.flag | b.flag;
        if (OPS & WIN_OP_COUNT) r.count = b.flag ? b.count : a.count + b.count;
        if (OPS & WIN_OP_SUM) r.sum = b.flag ? b.sum : a.sum + b.sum;
        if (OPS & WIN_OP_MIN) r.mn = b.flag ? b.mn : fmin(a.mn, b.mn); // (neither is ever NaN)
        if (OPS & WIN_OP_MAX) r.mx = b.flag ? b.mx : nan_max(a.mx, b.mx);
        return r;
    }
    static __device__ __forceinline__ WinVal up(const WinVal &s, int d) {
        WinVal r = identity();
        r.flag = __shfl_up(s.flag, d, 64);
        if (OPS & WIN_OP_COUNT) r.count = __shfl_up(s.count, d, 64);
        if (OPS & WIN_OP_SUM) r.sum = __shfl_up(s.sum, d, 64);
        if (OPS & WIN_OP_MIN) r.mn = __shfl_up(s.mn, d, 64);
        if (OPS & WIN_OP_MAX) r.mx = __shfl_up(s.mx, d, 64);
        return r;
    }
    // one row: its value, whether it is valid, whether its position starts a partition
    static __device__ __forceinline__ WinVal of(double v, bool ok, bool start) {
        WinVal r = identity();
        r.flag = start ? 1u : 0u;
        if (ok) {
            r.count = 1;
            r.sum = v;
            if (v == v) r.mn = fmin(v, WIN_F64_MAX);
            r.mx = v != v ? v : fmax(v, -WIN_F64_MAX);
        }
        return r;
    }
};

struct WinScanArgs {
    const double *x;           // [padded rows] the gathered column
    const uint16_t *valid;     // its valid bits; null: no NULLs
    const uint16_t *part_start;
    int64_t n, tiles;
    void *carry;               // WinVal<OPS>[tiles]; null with a single tile
    double *sum, *mn, *mx;     // [padded rows] the state at every position, per operator of OPS
    uint32_t *count;
};

// a thread's 16 rows (16-byte loads) folded from `s` on; KEEP: the state at every row is kept in out[]
template <int OPS, bool KEEP>
__device__ __forceinline__ WinVal<OPS> win_fold16(const WinScanArgs &a, int64_t base, WinVal<OPS> s, WinVal<OPS> *out) {
    const uint32_t vbits = win_bits16(a.valid, base, a.n), sbits = win_bits16(a.part_start, base, a.n);
    const double2 *src = reinterpret_cast<const double2 *>(a.x + base);
    double v[WIN_ITEMS];
#pragma unroll
    for (int k = 0; k < WIN_ITEMS / 2; ++k) {
        const double2 t = src[k];
        v[2 * k] = t.x, v[2 * k + 1] = t.y;
    }
#pragma unroll
    for (int k = 0; k < WIN_ITEMS; ++k) {
        s = WinVal<OPS>::combine(s, WinVal<OPS>::of(v[k], (vbits >> k) & 1, (sbits >> k) & 1));
        if (KEEP) out[k] = s;
    }
    return s;
}

// one workgroup per tile: the tile's carry — flag seen, and the state after the last flag
template <int OPS> __global__ void __launch_bounds__(WIN_THREADS) win_scan_reduce_kernel(WinScanArgs a) {
    __shared__ WinVal<OPS> lds[WIN_THREADS / 64];
    const int64_t base = int64_t(blockIdx.x) * WIN_TILE + int64_t(threadIdx.x) * WIN_ITEMS;
    WinVal<OPS> total;
    (void)win_block_exclusive(win_fold16<OPS, false>(a, base, WinVal<OPS>::identity(), nullptr), lds, &total);
    if (threadIdx.x == 0) static_cast<WinVal<OPS> *>(a.carry)[blockIdx.x] = total;
}

// ONE workgroup scans the tile carries, WIN_THREADS at a time: carry[t] becomes the state before tile t's first row
template <int OPS> __global__ void __launch_bounds__(WIN_THREADS) win_scan_carry_kernel(WinScanArgs a) {
    __shared__ WinVal<OPS> lds[WIN_THREADS / 64];
    WinVal<OPS> *carry = static_cast<WinVal<OPS> *>(a.carry);
    WinVal<OPS> run = WinVal<OPS>::identity();
    for (int64_t c0 = 0; c0 < a.tiles; c0 += WIN_THREADS) { // (uniform over the workgroup)
        const int64_t t = c0 + threadIdx.x;
        WinVal<OPS> total;
        const WinVal<OPS> e = win_block_exclusive(t < a.tiles ? carry[t] : WinVal<OPS>::identity(), lds, &total);
        if (t < a.tiles) carry[t] = WinVal<OPS>::combine(run, e);
        run = WinVal<OPS>::combine(run, total);
    }
}

// every tile again, from its carry-in: the state at every position, one array per operator
template <int OPS> __global__ void __launch_bounds__(WIN_THREADS) win_scan_apply_kernel(WinScanArgs a) {
    __shared__ WinVal<OPS> lds[WIN_THREADS / 64];
    const int64_t base = int64_t(blockIdx.x) * WIN_TILE + int64_t(threadIdx.x) * WIN_ITEMS;
    WinVal<OPS> total;
    WinVal<OPS> s = win_block_exclusive(win_fold16<OPS, false>(a, base, WinVal<OPS>::identity(), nullptr), lds, &total);
    if (a.carry) s = WinVal<OPS>::combine(static_cast<const WinVal<OPS> *>(a.carry)[blockIdx.x], s);
    WinVal<OPS> st[WIN_ITEMS];
    (void)win_fold16<OPS, true>(a, base, s, st);
    if (OPS & WIN_OP_SUM) {
        double2 *d = reinterpret_cast<double2 *>(a.sum + base);
#pragma unroll
        for (int k = 0; k < WIN_ITEMS / 2; ++k) d[k] = make_double2(st[2 * k].sum, st[2 * k + 1].sum);
    }
    if (OPS & WIN_OP_MIN) {
        double2 *d = reinterpret_cast<double2 *>(a.mn + base);
#pragma unroll
        for (int k = 0; k < WIN_ITEMS / 2; ++k) d[k] = make_double2(st[2 * k].mn, st[2 * k + 1].mn);
    }
    if (OPS & WIN_OP_MAX) {
        double2 *d = reinterpret_cast<double2 *>(a.mx + base);
#pragma unroll
        for (int k = 0; k < WIN_ITEMS / 2; ++k) d[k] = make_double2(st[2 * k].mx, st[2 * k + 1].mx);
    }
    if (OPS & WIN_OP_COUNT) {
        uint4 *d = reinterpret_cast<uint4 *>(a.count + base);
#pragma unroll
        for (int k = 0; k < WIN_ITEMS / 4; ++k) d[k] = make_uint4(st[4 * k].count, st[4 * k + 1].count, st[4 * k + 2].count, st[4 * k + 3].count);
    }
}

// =============================================================================================== win_emit
struct WinEmitFunc {
    int func, frame, slot; // slot: the value column's index in WinEmitArgs::val
    void *out;             // [n] uint64_t (ranking, count) or double, in INPUT order
};
struct WinEmitVal {
    const double *sum, *mn, *mx;
    const uint32_t *count;
};
struct WinEmitArgs {
    WinEmitFunc f[NQE_MAX_WINDOW_FUNCS];
    WinEmitVal val[NQE_MAX_WINDOW_FUNCS];
    int num_funcs;
    const uint32_t *perm; // null: the identity
    const uint32_t *part_first, *peer_first, *peers, *peer_last, *part_last; // null: not needed
    int64_t n;
};

// one thread per sorted position: every function's value, stored to row perm[i] of its column — the operator's only scatter.  (Position-major:
// a function-major loop, all workgroups writing one column at a time, measured no faster — profiles/window/README.md.)
__global__ void __launch_bounds__(WIN_THREADS) win_emit_kernel(WinEmitArgs a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const int64_t row = a.perm ? int64_t(a.perm[i]) : i;
        const uint32_t part_first = a.part_first ? a.part_first[i] : 0, peer_first = a.peer_first ? a.peer_first[i] : 0;
        const int64_t peer_last = a.peer_last ? int64_t(a.peer_last[i]) : i, part_last = a.part_last ? int64_t(a.part_last[i]) : i;
        for (int k = 0; k < a.num_funcs; ++k) { // (kernel arguments: uniform)
            const WinEmitFunc &f = a.f[k];
            if (f.func <= NQE_WIN_DENSE_RANK) {
                uint64_t r;
                if (f.func == NQE_WIN_ROW_NUMBER) r = uint64_t(i) - part_first + 1;
                else if (f.func == NQE_WIN_RANK) r = uint64_t(peer_first) - part_first + 1;
                else r = uint64_t(a.peers[i] - a.peers[part_first]) + 1;
                static_cast<uint64_t *>(f.out)[row] = r;
                continue;
            }
            const int64_t p = f.frame == NQE_FRAME_ROWS ? i : f.frame == NQE_FRAME_RANGE ? peer_last : part_last;
            const WinEmitVal &v = a.val[f.slot];
            if (f.func == NQE_WIN_COUNT) static_cast<uint64_t *>(f.out)[row] = uint64_t(v.count[p]);
            else if (f.func == NQE_WIN_SUM) static_cast<double *>(f.out)[row] = v.sum[p];
            else if (f.func == NQE_WIN_MIN) static_cast<double *>(f.out)[row] = v.mn[p];
            else if (f.func == NQE_WIN_MAX) static_cast<double *>(f.out)[row] = v.mx[p];
            else static_cast<double *>(f.out)[row] = v.sum[p] / double(v.count[p]); // avg.rs: the count as u32
        }
    }
}

} // namespace
} // namespace nqe
