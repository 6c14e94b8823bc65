// window_ex_kernels.hpp — the kernels nqe_window_execute_ex adds to those of window_kernels.hpp (window.hip; the host analysis and the
// position arithmetic: window_ex_plan.hpp).
//
// A bounded frame is never a difference of prefixes.  Per (value column, width w) two segmented scans run — both through the EXISTING
// forward machinery win_scan_*<OPS>, which restarts wherever its flag bitmap has a bit:
//   pre      over the gathered column, flags = partition starts | positions with p % w == 0                          (win_flags)
//   suf      over the REVERSED gathered column (win_reverse: x_rev[j] = x[n - 1 - j], valid bits likewise), flags in reversed positions
//            = partition ends | positions with p % w == w - 1; suf[p] is that scan's state at n - 1 - p
// and win_emit_frame combines at most two states that lie inside the row's frame (win_frame_pieces).  The backward scan is the forward
// scan over a reversed copy: no new scan kernel, no new instance of an old one.
#pragma once

#include "window_ex_plan.hpp"
#include "window_kernels.hpp"

namespace nqe {
namespace {

// =============================================================================================== win_flags
// One thread per position j, a wave writes one word of each bitmap.  fwd bit j: position j starts a partition or a block of w;
// rev bit j: position p = n - 1 - j ends a partition or a block of w.  w == 0: no blocks.  Either bitmap may be null.
__global__ void __launch_bounds__(WIN_THREADS) win_flags_kernel(const uint8_t *part_start, int64_t n, uint32_t w, uint64_t *fwd, uint64_t *rev) {
    const int64_t nwords = (n + 63) / 64;
    const int64_t waves = int64_t(gridDim.x) * (WIN_THREADS / 64);
    for (int64_t word = int64_t(blockIdx.x) * (WIN_THREADS / 64) + (int(threadIdx.x) >> 6); word < nwords; word += waves) { // (wave-uniform)
        const int64_t j = word * 64 + lane_id();
        bool f = false, r = false;
        if (j < n) {
            f = get_bit(part_start, j) || (w && uint32_t(j) % w == 0);
            const int64_t p = n - 1 - j;
            r = p == n - 1 || get_bit(part_start, p + 1) || (w && uint32_t(p) % w == w - 1);
        }
        const uint64_t bf = __ballot(f), br = __ballot(r);
        if (lane_id() == 0) {
            if (fwd) fwd[word] = bf;
            if (rev) rev[word] = br;
        }
    }
}

// =============================================================================================== win_reverse
// x_rev[j] = x[n - 1 - j] and the valid bits likewise (valid null: none are written); both streams are read and written in whole lines
__global__ void __launch_bounds__(WIN_THREADS) win_reverse_kernel(const double *x, const uint8_t *valid, int64_t n, double *x_rev, uint64_t *valid_rev) {
    const int64_t nwords = (n + 63) / 64;
    const int64_t waves = int64_t(gridDim.x) * (WIN_THREADS / 64);
    for (int64_t word = int64_t(blockIdx.x) * (WIN_THREADS / 64) + (int(threadIdx.x) >> 6); word < nwords; word += waves) { // (wave-uniform)
        const int64_t j = word * 64 + lane_id();
        bool ok = false;
        if (j < n) {
            const int64_t p = n - 1 - j;
            x_rev[j] = x[p];
            ok = !valid || get_bit(valid, p);
        }
        const uint64_t b = __ballot(ok);
        if (valid_rev && lane_id() == 0) valid_rev[word] = b;
    }
}

// =============================================================================================== win_emit_frame
// the aggregates over half-unbounded and bounded ROWS BETWEEN frames
struct WinFrameFunc {
    int func, cls;        // NQE_WINX_COUNT .. NQE_WINX_AVG; WinFrameClass
    uint32_t w;           // WIN_FC_BOUNDED: the block width
    int64_t start, end;   // the clamped offsets
    WinEmitVal pre, suf;  // states by position / by REVERSED position (n - 1 - p); the class decides which are read
    void *out;            // [n] uint64_t (count) or double, in INPUT order
};
struct WinFrameArgs {
    WinFrameFunc f[NQE_MAX_WINDOW_FUNCS];
    int num_funcs;
    const uint32_t *perm; // null: the identity
    const uint32_t *part_first, *part_last;
    int64_t n;
};

// one thread per sorted position: per function the one or two states of its frame's pieces, combined as WinVal combines them
__global__ void __launch_bounds__(WIN_THREADS) win_emit_frame_kernel(WinFrameArgs a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const int64_t row = a.perm ? int64_t(a.perm[i]) : i;
        const uint32_t pf = a.part_first[i], pl = a.part_last[i];
        for (int k = 0; k < a.num_funcs; ++k) { // (kernel arguments: uniform)
            const WinFrameFunc &f = a.f[k];
            const WinPieces p = win_frame_pieces(f.cls, f.start, f.end, f.w, uint32_t(i), pf, pl);
            const bool pre = p.kind == WIN_PIECE_BOTH || p.kind == WIN_PIECE_PRE, suf = p.kind == WIN_PIECE_BOTH || p.kind == WIN_PIECE_SUF;
            const int64_t ip = int64_t(p.b), is = a.n - 1 - int64_t(p.a);
            const bool want_count = f.func == NQE_WINX_COUNT || f.func == NQE_WINX_AVG, want_sum = f.func == NQE_WINX_SUM || f.func == NQE_WINX_AVG;
            uint32_t count = 0;
            double sum = 0.0;
            if (want_count) count = (pre ? f.pre.count[ip] : 0u) + (suf ? f.suf.count[is] : 0u);
            if (want_sum) sum = pre && suf ? f.suf.sum[is] + f.pre.sum[ip] : pre ? f.pre.sum[ip] : suf ? f.suf.sum[is] : 0.0;
            if (f.func == NQE_WINX_COUNT) static_cast<uint64_t *>(f.out)[row] = uint64_t(count);
            else if (f.func == NQE_WINX_SUM) static_cast<double *>(f.out)[row] = sum;
            else if (f.func == NQE_WINX_AVG) static_cast<double *>(f.out)[row] = sum / double(count); // avg.rs: the count as u32
            else if (f.func == NQE_WINX_MIN) static_cast<double *>(f.out)[row] = fmin(pre ? f.pre.mn[ip] : WIN_F64_MAX, suf ? f.suf.mn[is] : WIN_F64_MAX); // (neither is ever NaN)
            else static_cast<double *>(f.out)[row] = WinVal<WIN_OP_MAX>::nan_max(pre ? f.pre.mx[ip] : -WIN_F64_MAX, suf ? f.suf.mx[is] : -WIN_F64_MAX);
        }
    }
}

// =============================================================================================== win_inverse / win_emit_value
// pos[perm[i]] = i: the sorted position of every input row (one word per thread; perm is a permutation, so no word is written twice)
__global__ void __launch_bounds__(WIN_THREADS) win_inverse_kernel(const uint32_t *perm, int64_t n, uint32_t *pos) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) pos[perm[i]] = uint32_t(i);
}

struct WinValueFunc {
    int func, cls, frame, has_default; // NQE_WINX_LAG .. NQE_WINX_NTILE; FIRST / LAST: the frame's class and, for WIN_FC_OLD, which frame
    int64_t start, end, param;         // the clamped frame offsets; k (LAG / LEAD) or b (NTILE)
    uint64_t default_word;
    const uint64_t *words;             // the argument column, in input order
    const uint8_t *valid;              // null: no NULLs
    uint64_t *out;                     // [n] in INPUT order
    uint64_t *out_valid;               // one word per 64 rows; null for NTILE
    unsigned long long *nulls;         // the column's NULL count is added here
};
struct WinValueArgs {
    WinValueFunc f[NQE_MAX_WINDOW_FUNCS];
    int num_funcs;
    const uint32_t *perm, *pos; // null: the identity (both)
    const uint32_t *part_first, *part_last, *peer_last; // peer_last null: no FIRST / LAST over RANGE
    int64_t n;
};

// One thread per INPUT row r, a wave owns 64 consecutive rows and therefore one whole validity word of every output column: the word
// is the wave's ballot, stored once — no word is ever read back or shared between waves.  The thread finds its sorted position, the
// source position of every function, and reads the source row through the permutation; the value stores are coalesced.
__global__ void __launch_bounds__(WIN_THREADS) win_emit_value_kernel(WinValueArgs a) {
    const int64_t nwords = (a.n + 63) / 64;
    const int64_t waves = int64_t(gridDim.x) * (WIN_THREADS / 64);
    for (int64_t word = int64_t(blockIdx.x) * (WIN_THREADS / 64) + (int(threadIdx.x) >> 6); word < nwords; word += waves) { // (wave-uniform)
        const int64_t r = word * 64 + lane_id();
        const bool in = r < a.n;
        uint32_t i = 0, pf = 0, pl = 0;
        if (in) {
            i = a.pos ? a.pos[r] : uint32_t(r);
            pf = a.part_first[i], pl = a.part_last[i];
        }
        for (int k = 0; k < a.num_funcs; ++k) { // (kernel arguments: uniform)
            const WinValueFunc &f = a.f[k];
            if (f.func == NQE_WINX_NTILE) {
                if (in) f.out[r] = win_ntile_bucket(i - pf, pl - pf + 1, uint32_t(f.param));
                continue;
            }
            bool ok = false;
            if (in) {
                int64_t src = -1; // the source's sorted position; -1: none
                bool use_default = false;
                if (f.func == NQE_WINX_LAG) {
                    src = int64_t(i) - f.param;
                    if (src < int64_t(pf)) src = -1, use_default = f.has_default != 0;
                } else if (f.func == NQE_WINX_LEAD) {
                    src = int64_t(i) + f.param;
                    if (src > int64_t(pl)) src = -1, use_default = f.has_default != 0;
                } else if (f.cls == WIN_FC_OLD) {
                    const uint32_t last = f.frame == NQE_FRAMEX_ROWS ? i : f.frame == NQE_FRAMEX_RANGE ? a.peer_last[i] : pl;
                    src = f.func == NQE_WINX_FIRST_VALUE ? int64_t(pf) : int64_t(last);
                } else {
                    const WinPieces p = win_frame_pieces(f.cls, f.start, f.end, 1u, i, pf, pl); // (only a and b are read: any width will do)
                    if (p.kind != WIN_PIECE_EMPTY) src = f.func == NQE_WINX_FIRST_VALUE ? int64_t(p.a) : int64_t(p.b);
                }
                uint64_t v = 0;
                if (src >= 0) {
                    const int64_t q = a.perm ? int64_t(a.perm[src]) : src;
                    ok = !f.valid || get_bit(f.valid, q);
                    if (ok) v = f.words[q];
                } else if (use_default) {
                    ok = true;
                    v = f.default_word;
                }
                f.out[r] = v;
            }
            const uint64_t b = __ballot(ok);
            if (lane_id() == 0) {
                f.out_valid[word] = b;
                const int64_t left = a.n - word * 64;
                const int rows = left >= 64 ? 64 : int(left);
                const int nulls = rows - __popcll(b);
                if (nulls) atomicAdd(f.nulls, (unsigned long long)nulls);
            }
        }
    }
}

} // namespace
} // namespace nqe
