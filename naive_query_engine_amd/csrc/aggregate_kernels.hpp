// aggregate_kernels.hpp — the kernels of aggregate.hip's own translation unit: the general grouped kernel (any key / predicate shape the
// streaming kernels of aggregate_fast_kernel.hpp do not take), the un-grouped kernels and their fold, with the pickers that map run-time
// shapes to template instances.  Included by aggregate.hip alone, inside its anonymous namespace (after `using namespace agg;`).
#pragma once

// ------------------------------------------------------------------ grouped kernel
// History: with the 64-bit software divide inlined for predicate and key in each of the 4 unrolled rows the first
// version of this kernel was 30k instructions long and instruction-fetch bound (2.2 TB/s).  Now literal divisors use
// shift/mask or a magic multiply and only column÷column reaches the out-of-line divmod_general, so the general
// SimpleExpr evaluator is inlined again; the common shapes are still specialised:
//   PRED: 0 none | 1 `col cmp lit` (literal on either side, normalised on the host) | 2 Boolean bitmap
//         | 3 any other SimpleExpr
//   KEY : 0 plain column | 1 `col % ±2^k` | 2 any other SimpleExpr
//   PLAIN: every streamed source is an 8-byte column without a validity bitmap (no bitmap loads)
__device__ __forceinline__ bool cmp_lit(int op, int dt, uint64_t a, uint64_t b) {
    bool lt, eq;
    if (dt == NQE_INT64) { lt = (long long)a < (long long)b; eq = a == b; }
    else if (dt == NQE_FLOAT64) { double x = u2d(a), y = u2d(b); lt = x < y; eq = x == y; if (x != x || y != y) return op == NQE_OP_NOT_EQ; }
    else { lt = a < b; eq = a == b; }
    return op == NQE_OP_EQ ? eq : op == NQE_OP_NOT_EQ ? !eq : op == NQE_OP_LT ? lt : op == NQE_OP_LT_EQ ? (lt || eq)
           : op == NQE_OP_GT ? !(lt || eq) : !lt;
}

template <int PRED, int KEY, bool PLAIN>
__global__ void __launch_bounds__(AGG_BLOCK) agg_grouped_kernel(AggArgs a, GroupTable g, int *flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t cap = uint32_t(a.lds_cap);
    const uint32_t slots = cap + 1;
    uint64_t *lkeys = reinterpret_cast<uint64_t *>(smem);
    const uint32_t nvl = a.nv > 0 ? uint32_t(a.nv) : 1u;                 // value columns of THIS pass
    double *lsum = reinterpret_cast<double *>(lkeys + slots);            // [nvl][slots]
    uint64_t *lmn = reinterpret_cast<uint64_t *>(lsum + nvl * slots);    // [nvl][slots]
    uint64_t *lmx = lmn + nvl * slots;                                   // [nvl][slots]
    uint32_t *lcnt = reinterpret_cast<uint32_t *>(lmx + nvl * slots);    // [nvl][slots]
    const uint64_t ORD_MAX = f64_to_ord(DBL_MAX), ORD_MIN = f64_to_ord(-DBL_MAX);
    __shared__ int lds_full_flag;
    volatile int *lds_full = &lds_full_flag;
    if (threadIdx.x == 0) lds_full_flag = 0;

    for (uint32_t s = threadIdx.x; s < slots; s += blockDim.x) {
        lkeys[s] = EMPTY_KEY;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (uint32_t(j) >= nvl) continue;
            lsum[j * slots + s] = 0.0;
            lmn[j * slots + s] = ORD_MAX;
            lmx[j * slots + s] = ORD_MIN;
            lcnt[j * slots + s] = 0;
        }
    }
    __syncthreads();

    // Per-thread run cache.  All rows a thread visits are congruent modulo blockDim (row = base + u*blockDim +
    // tid with base a multiple of blockDim*AGG_U), so for clustered keys — and for `id % m` over a row-number id
    // whenever m divides blockDim — consecutive rows of a thread carry the SAME key.  They are accumulated in
    // registers and written to the workgroup table only when the key changes (one flush per run instead of four
    // LDS atomics per row).  Random keys flush every row.
    bool full = false; // register copy of lds_full_flag (set by own failures, refreshed per tile)
    bool run_live = false;
    uint64_t run_key = 0;
    uint32_t rcnt[NV];
    double rsum[NV];
    uint64_t rmn[NV], rmx[NV];
    bool rnan[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        rcnt[j] = 0; rsum[j] = 0.0; rmn[j] = ORD_MAX; rmx[j] = ORD_MIN; rnan[j] = false;
    }
    auto flush_run = [&]() {
        // once this workgroup's table has rejected a key, later keys skip it: any split of the updates between
        // the LDS table and the global table is correct (the merge is additive), and a full table costs 48 probes
        int slot = full ? -1 : lds_find_or_insert(lkeys, run_key, cap, a.lds_shift);
        if (slot < 0 && !full) {
            full = true;
            *lds_full = 1;
        }
        int64_t gslot = slot < 0 ? global_find_or_insert(g, run_key, flags) : 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (j >= a.nv) continue;
            if (slot >= 0) {
                uint32_t o = uint32_t(j) * slots + uint32_t(slot);
                if (rcnt[j]) atomicAdd(&lcnt[o], rcnt[j]); // < 2^31 rows per workgroup, bit 31 is the NaN flag
                if (rnan[j]) atomicOr(&lcnt[o], NAN_BIT);
                if (a.need_sum[j] && rcnt[j]) unsafeAtomicAdd(&lsum[o], rsum[j]);
                if (a.need_minmax[j]) {
                    // read-before-atomic: once a group holds a few rows almost no run improves its extremes, and
                    // an LDS read costs a small fraction of a 64-bit LDS atomic.  A stale read only causes a
                    // redundant (still correct) atomic.
                    if (rmn[j] < lmn[o]) atomicMin((unsigned long long *)&lmn[o], (unsigned long long)rmn[j]);
                    if (rmx[j] > lmx[o]) atomicMax((unsigned long long *)&lmx[o], (unsigned long long)rmx[j]);
                }
            } else if (gslot >= 0) {
                global_update(g, gslot, a.v0 + j, rcnt[j], rsum[j], a.need_sum[j] != 0, rmn[j], rmx[j], a.need_minmax[j] != 0,
                              rnan[j]);
            }
            rcnt[j] = 0; rsum[j] = 0.0; rmn[j] = ORD_MAX; rmx[j] = ORD_MIN; rnan[j] = false;
        }
    };

    const uint64_t *keyp = static_cast<const uint64_t *>(a.key_src.values);
    const uint64_t *predp = static_cast<const uint64_t *>(a.pred_src.values);
    const int pred_op = a.pred.op[0], pred_dt = a.pred.op_dtype[0];
    const uint64_t pred_lit = a.pred.lit[0];
    const uint64_t key_mask = a.key.aux[0].abs_lit - 1;
    const bool key_signed = a.key.op_dtype[0] == NQE_INT64;

    const int64_t step = int64_t(blockDim.x) * AGG_U;
    for (int64_t base = int64_t(blockIdx.x) * step; base < a.n; base += int64_t(gridDim.x) * step) {
        if (__hip_atomic_load(&flags[NQE_FLAG_TABLE_FULL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break; // host retries
        full = full || *lds_full != 0;
        uint64_t kw[AGG_U], pw[AGG_U], vw[NV][AGG_U];
        // ---- load phase: every referenced word of this iteration is requested before any use
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            int64_t row = base + int64_t(u) * blockDim.x + threadIdx.x;
            bool in = row < a.n;
            if (PLAIN) {
                kw[u] = in ? keyp[row] : 0;
                pw[u] = ((PRED == 1 || PRED == 3) && in && !a.pred_shares_key) ? predp[row] : 0;
            } else {
                kw[u] = in ? load_word(a.key_src.values, a.key_src.dtype, row) : 0;
                pw[u] = ((PRED == 1 || PRED == 3) && in && !a.pred_shares_key) ? load_word(a.pred_src.values, a.pred_src.dtype, row) : 0;
            }
#pragma unroll
            for (int j = 0; j < NV; ++j)
                vw[j][u] = (in && j < a.nv && a.val[j].values && !a.val_shares_key[j])
                               ? static_cast<const uint64_t *>(a.val[j].values)[row]
                               : 0;
        }
        // ---- compute phase
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            int64_t row = base + int64_t(u) * blockDim.x + threadIdx.x;
            bool pass = row < a.n;
            if (PRED == 1 || PRED == 3) {
                bool ok = pass && (PLAIN || row_valid(a.pred_src, row));
                uint64_t w = a.pred_shares_key ? kw[u] : pw[u];
                if (PRED == 1) pass = ok && cmp_lit(pred_op, pred_dt, w, pred_lit);
                else pass = ok && eval_simple(a.pred, w, ok, flags) != 0;
            } else if (PRED == 2) {
                pass = pass && get_bit(static_cast<const uint8_t *>(a.pred_src.values), row) && row_valid(a.pred_src, row);
            }
            bool kok = pass && (PLAIN || row_valid(a.key_src, row));
            uint64_t key;
            if (KEY == 0) key = kw[u];
            else if (KEY == 1) {
                uint64_t x = kw[u];
                bool neg = key_signed && (long long)x < 0;
                uint64_t ur = (neg ? 0ull - x : x) & key_mask;
                key = neg ? 0ull - ur : ur;
            } else key = eval_simple(a.key, kw[u], kok, flags);
            pass = kok;
            if (!pass) continue;
            if (!run_live || key != run_key) {
                if (run_live) flush_run();
                run_key = key;
                run_live = true;
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if (j >= a.nv) continue;
                if (!PLAIN && !row_valid(a.val[j], row)) continue;
                rcnt[j] += 1;
                if (a.need_sum[j] || a.need_minmax[j]) {
                    double x = word_as_f64(a.val_shares_key[j] ? kw[u] : vw[j][u], a.val[j].dtype);
                    rsum[j] += x;
                    if (x != x) rnan[j] = true;
                    else {
                        uint64_t xo = f64_to_ord(x);
                        rmn[j] = xo < rmn[j] ? xo : rmn[j];
                        rmx[j] = xo > rmx[j] ? xo : rmx[j];
                    }
                }
            }
        }
    }
    if (run_live) flush_run();
    __syncthreads();
    // ---- merge this workgroup's table into the global one
    for (uint32_t s = threadIdx.x; s < slots; s += blockDim.x) {
        uint64_t k = lkeys[s];
        if (k == EMPTY_KEY) continue;
        uint64_t key = (s == cap) ? EMPTY_KEY : k;
        int64_t gslot = global_find_or_insert(g, key, flags);
        if (gslot < 0) continue;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (j >= a.nv) continue;
            uint32_t o = uint32_t(j) * slots + s;
            uint32_t c = lcnt[o];
            global_update(g, gslot, a.v0 + j, uint64_t(c & ~NAN_BIT), lsum[o], a.need_sum[j] != 0, lmn[o], lmx[o],
                          a.need_minmax[j] != 0, (c & NAN_BIT) != 0);
        }
    }
}

using GroupedKernel = void (*)(AggArgs, GroupTable, int *);
template <int PRED, int KEY> GroupedKernel pick_plain(bool plain) {
    return plain ? agg_grouped_kernel<PRED, KEY, true> : agg_grouped_kernel<PRED, KEY, false>;
}
template <int PRED> GroupedKernel pick_key(int key, bool plain) {
    switch (key) {
    case 0: return pick_plain<PRED, 0>(plain);
    case 1: return pick_plain<PRED, 1>(plain);
    default: return pick_plain<PRED, 2>(plain);
    }
}
GroupedKernel pick_grouped_kernel(int pred, int key, bool plain) {
    switch (pred) {
    case 0: return pick_key<0>(key, plain);
    case 1: return pick_key<1>(key, plain);
    case 2: return pick_key<2>(key, plain);
    default: return pick_key<3>(key, plain);
    }
}

// ------------------------------------------------------------------ un-grouped kernel
struct Partial {
    uint64_t cnt;
    double sum;
    double mn, mx;
    uint32_t nan;
    uint32_t pad;
};

__device__ __forceinline__ double shfl_down_f64(double v, int d) { return __shfl_down(v, d, 64); }

__global__ void __launch_bounds__(AGG_BLOCK) agg_ungrouped_kernel(AggArgs a, Partial *partials, int *flags) {
    uint64_t cnt[NV];
    double sum[NV], mn[NV], mx[NV];
    uint32_t nanf[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        cnt[j] = 0; sum[j] = 0.0; mn[j] = DBL_MAX; mx[j] = -DBL_MAX; nanf[j] = 0;
    }
    const int64_t step = int64_t(blockDim.x) * AGG_U;
    for (int64_t base = int64_t(blockIdx.x) * step; base < a.n; base += int64_t(gridDim.x) * step) {
        uint64_t pw[AGG_U], vw[NV][AGG_U];
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            int64_t row = base + int64_t(u) * blockDim.x + threadIdx.x;
            bool in = row < a.n;
            pw[u] = (in && a.pred_mode == 1) ? load_word(a.pred_src.values, a.pred_src.dtype, row) : 0;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                vw[j][u] = (in && j < a.nv && a.val[j].values) ? static_cast<const uint64_t *>(a.val[j].values)[row] : 0;
        }
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            int64_t row = base + int64_t(u) * blockDim.x + threadIdx.x;
            bool pass = row < a.n;
            if (a.pred_mode == 1) {
                bool ok = pass && row_valid(a.pred_src, row);
                pass = ok && eval_simple(a.pred, pw[u], ok, flags) != 0;
            } else if (a.pred_mode == 2) {
                pass = pass && get_bit(static_cast<const uint8_t *>(a.pred_src.values), row) && row_valid(a.pred_src, row);
            }
            if (!pass) continue;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if (j >= a.nv || !row_valid(a.val[j], row)) continue;
                cnt[j] += 1;
                if (a.need_sum[j] || a.need_minmax[j]) {
                    double x = word_as_f64(vw[j][u], a.val[j].dtype);
                    sum[j] += x;
                    if (x != x) nanf[j] = 1;
                    else {
                        mn[j] = x < mn[j] ? x : mn[j];
                        mx[j] = x > mx[j] ? x : mx[j];
                    }
                }
            }
        }
    }
    __shared__ Partial wave_part[AGG_BLOCK / 64][NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        for (int d = 32; d > 0; d >>= 1) {
            cnt[j] += __shfl_down((unsigned long long)cnt[j], d, 64);
            sum[j] += shfl_down_f64(sum[j], d);
            double omn = shfl_down_f64(mn[j], d), omx = shfl_down_f64(mx[j], d);
            mn[j] = omn < mn[j] ? omn : mn[j];
            mx[j] = omx > mx[j] ? omx : mx[j];
            nanf[j] |= __shfl_down(nanf[j], d, 64);
        }
        if (lane_id() == 0) {
            Partial p{cnt[j], sum[j], mn[j], mx[j], nanf[j], 0};
            wave_part[threadIdx.x / 64][j] = p;
        }
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        int j = threadIdx.x;
        Partial t{0, 0.0, DBL_MAX, -DBL_MAX, 0, 0};
        for (int w = 0; w < int(blockDim.x) / 64; ++w) { // fixed order: deterministic
            const Partial &p = wave_part[w][j];
            t.cnt += p.cnt; t.sum += p.sum;
            t.mn = p.mn < t.mn ? p.mn : t.mn;
            t.mx = p.mx > t.mx ? p.mx : t.mx;
            t.nan |= p.nan;
        }
        partials[size_t(blockIdx.x) * NV + j] = t;
    }
}

// un-grouped fast path: plain 8-byte columns, optional integer range predicate on one column.
// PRED: 0 none, 1 predicate column is value column 0 (one load serves both), 2 a separate column.
template <int PRED, int NVT, bool VF64, bool VNULL>
__global__ void __launch_bounds__(AGG_BLOCK) agg_ungrouped_fast_kernel(AggArgs a, FastPred fp, Partial *partials) {
    uint64_t cnt[NVT];
    double sum[NVT], mn[NVT], mx[NVT];
    bool nanf[NVT];
#pragma unroll
    for (int j = 0; j < NVT; ++j) {
        cnt[j] = 0; sum[j] = 0.0; mn[j] = DBL_MAX; mx[j] = -DBL_MAX; nanf[j] = false;
    }
    const uint64_t *__restrict__ predp = static_cast<const uint64_t *>(a.pred_src.values);
    const uint64_t *__restrict__ valp[NVT];
    const uint64_t *__restrict__ vvalid[NVT]; // VNULL: word-readable validity bitmaps, null = all valid
    const uint64_t *__restrict__ pvalid = reinterpret_cast<const uint64_t *>(PRED != 0 ? a.pred_src.valid : nullptr);
    int vdt[NVT];
#pragma unroll
    for (int j = 0; j < NVT; ++j) {
        valp[j] = static_cast<const uint64_t *>(a.val[j].values);
        vvalid[j] = reinterpret_cast<const uint64_t *>(a.val[j].valid);
        vdt[j] = a.val[j].dtype;
    }
    const int64_t n = a.n, last = a.n - 1;
    struct Tile {
        uint64_t pw[AGG_U], vw[NVT][AGG_U];
        uint64_t vv[VNULL ? NVT : 1][AGG_U], pv[VNULL ? AGG_U : 1];
    };
    auto load_tile = [&](Tile &t, int64_t base) {
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            int64_t row = base + int64_t(u) * AGG_BLOCK + threadIdx.x;
            row = row < last ? row : last;
            if (PRED == 2) t.pw[u] = __builtin_nontemporal_load(&predp[row >> fp.row_shift]);
#pragma unroll
            for (int j = 0; j < NVT; ++j) t.vw[j][u] = __builtin_nontemporal_load(&valp[j][row]);
            if (VNULL) {
#pragma unroll
                for (int j = 0; j < NVT; ++j) t.vv[j][u] = vvalid[j] ? vvalid[j][row >> 6] : ~0ull;
                t.pv[u] = pvalid ? pvalid[row >> 6] : ~0ull;
            }
        }
    };
    auto process_tile = [&](const Tile &t, int64_t base) {
#pragma unroll
        for (int u = 0; u < AGG_U; ++u) {
            int64_t row = base + int64_t(u) * AGG_BLOCK + threadIdx.x;
            bool pass = row < n;
            if (PRED != 0) pass = pass && range_pass(fp, PRED == 1 ? t.vw[0][u] : pred_extract(fp, t.pw[u], row));
            if (VNULL) pass = pass && ((t.pv[u] >> (row & 63)) & 1ull); // a NULL predicate's row is all-NULL: contributes nothing
            if (!pass) continue;
#pragma unroll
            for (int j = 0; j < NVT; ++j) {
                double x = VF64 ? u2d(t.vw[j][u]) : word_as_f64(t.vw[j][u], vdt[j]);
                if (VNULL && !((t.vv[j][u] >> (row & 63)) & 1ull)) continue; // NULL value: not counted (Q10)
                cnt[j] += 1;
                sum[j] += x;
                nanf[j] = nanf[j] || (x != x);
                mn[j] = fmin(mn[j], x);
                mx[j] = fmax(mx[j], x);
            }
        }
    };
    const int64_t step = int64_t(AGG_BLOCK) * AGG_U;
    const int64_t stride = int64_t(gridDim.x) * step;
    int64_t base = int64_t(blockIdx.x) * step;
    if (base < n) {
        Tile A, B;
        load_tile(A, base);
        for (;;) {
            load_tile(B, base + stride);
            process_tile(A, base);
            base += stride;
            if (base >= n) break;
            load_tile(A, base + stride);
            process_tile(B, base);
            base += stride;
            if (base >= n) break;
        }
    }
    __shared__ Partial wave_part[AGG_BLOCK / 64][NV];
#pragma unroll
    for (int j = 0; j < NVT; ++j) {
        uint32_t nf = nanf[j] ? 1u : 0u;
        for (int d = 32; d > 0; d >>= 1) {
            cnt[j] += __shfl_down((unsigned long long)cnt[j], d, 64);
            sum[j] += shfl_down_f64(sum[j], d);
            double omn = shfl_down_f64(mn[j], d), omx = shfl_down_f64(mx[j], d);
            mn[j] = omn < mn[j] ? omn : mn[j];
            mx[j] = omx > mx[j] ? omx : mx[j];
            nf |= __shfl_down(nf, d, 64);
        }
        if (lane_id() == 0) {
            Partial p{cnt[j], sum[j], mn[j], mx[j], nf, 0};
            wave_part[threadIdx.x / 64][j] = p;
        }
    }
    __syncthreads();
    if (threadIdx.x < NVT) {
        int j = threadIdx.x;
        Partial t{0, 0.0, DBL_MAX, -DBL_MAX, 0, 0};
        for (int w = 0; w < AGG_BLOCK / 64; ++w) {
            const Partial &p = wave_part[w][j];
            t.cnt += p.cnt; t.sum += p.sum;
            t.mn = p.mn < t.mn ? p.mn : t.mn;
            t.mx = p.mx > t.mx ? p.mx : t.mx;
            t.nan |= p.nan;
        }
        partials[size_t(blockIdx.x) * NV + j] = t;
    }
}

using UngroupedFastKernel = void (*)(AggArgs, FastPred, Partial *);
template <int PRED, bool VNULL> UngroupedFastKernel pick_ungrouped_fast_nv(int nv, bool vf64) {
    if (nv == 1) return vf64 ? agg_ungrouped_fast_kernel<PRED, 1, true, VNULL> : agg_ungrouped_fast_kernel<PRED, 1, false, VNULL>;
    return vf64 ? agg_ungrouped_fast_kernel<PRED, 2, true, VNULL> : agg_ungrouped_fast_kernel<PRED, 2, false, VNULL>;
}
template <bool VNULL> UngroupedFastKernel pick_ungrouped_fast_pred(int pred, int nv, bool vf64) {
    return pred == 0 ? pick_ungrouped_fast_nv<0, VNULL>(nv, vf64) : pred == 1 ? pick_ungrouped_fast_nv<1, VNULL>(nv, vf64) : pick_ungrouped_fast_nv<2, VNULL>(nv, vf64);
}
UngroupedFastKernel pick_ungrouped_fast(int pred, int nv, bool vf64, bool vnull) {
    return vnull ? pick_ungrouped_fast_pred<true>(pred, nv, vf64) : pick_ungrouped_fast_pred<false>(pred, nv, vf64);
}

__global__ void agg_ungrouped_fold_kernel(const Partial *partials, int nblocks, int nv, int v0, GroupTable g) {
    int j = threadIdx.x;
    if (j >= nv) return;
    Partial t{0, 0.0, DBL_MAX, -DBL_MAX, 0, 0};
    for (int b = 0; b < nblocks; ++b) {
        const Partial &p = partials[size_t(b) * NV + j];
        t.cnt += p.cnt; t.sum += p.sum;
        t.mn = p.mn < t.mn ? p.mn : t.mn;
        t.mx = p.mx > t.mx ? p.mx : t.mx;
        t.nan |= p.nan;
    }
    size_t o = size_t(v0 + j) * (size_t(g.cap) + 1);
    g.cnt[o] += t.cnt;
    g.sum[o] += t.sum;
    uint64_t omn = f64_to_ord(t.mn), omx = f64_to_ord(t.mx);
    if (omn < g.mn[o]) g.mn[o] = omn;
    if (omx > g.mx[o]) g.mx[o] = omx;
    g.nan[o] |= t.nan;
}
