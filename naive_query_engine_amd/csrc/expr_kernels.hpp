// expr_kernels.hpp — the device code of expr.hip (included by it alone): the node-at-a-time kernels (one per binary or unary node, and the
// literal fill) and the stack machine that runs a whole ExProgram (expr_plan.hpp) in one pass, plain and behind a selection.
#pragma once

#include "device_utils.hpp"
#include "expr_plan.hpp"

namespace nqe {
namespace {

// ------------------------------------------------------------------ kernels (their operands: device_utils.hpp, Operand)

// out = a op b, 64 consecutive rows per wave so that ballots form the packed result words.
// bool_out: result is Boolean (compare / and / or) → packed into out_bits.
__global__ void __launch_bounds__(256) binary_kernel(Operand a, Operand b, int op, int dt, OpAux aux, int64_t n,
                                                     uint64_t *out_words, uint64_t *out_bits, uint64_t *out_valid,
                                                     int *flags) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t n_pad = (n + 63) / 64 * 64;
    const bool logic = op == NQE_OP_AND || op == NQE_OP_OR;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n_pad; j += stride) {
        const bool in = j < n;
        bool av = in && (a.is_lit ? !a.lit_null : (a.valid ? get_bit(a.valid, j) : true));
        bool bv = in && (b.is_lit ? !b.lit_null : (b.valid ? get_bit(b.valid, j) : true));
        uint64_t x = a.is_lit ? a.lit : (in ? load_word(a.values, dt, j) : 0);
        uint64_t y = b.is_lit ? b.lit : (in ? load_word(b.values, dt, j) : 0);
        bool ok;
        uint64_t r;
        if (logic) {
            // and_kleene / or_kleene
            bool lb = av && x, rb = bv && y;
            if (op == NQE_OP_AND) {
                ok = (av && bv) || (av && !lb) || (bv && !rb);
                r = ok && lb && rb;
            } else {
                ok = (av && bv) || lb || rb;
                r = ok && (lb || rb);
            }
        } else {
            ok = av && bv;
            r = in ? apply_binary(op, dt, x, y, aux, ok, flags) : 0;
        }
        if (out_words) {
            if (in) out_words[j] = ok ? r : 0;
        } else {
            uint64_t w = __ballot(ok && r);
            if (lane_id() == 0) out_bits[j >> 6] = w;
        }
        if (out_valid) {
            uint64_t v = __ballot(ok);
            if (lane_id() == 0) out_valid[j >> 6] = v;
        }
    }
}

// out = f(in) over Float64 words, one kernel per UNARY node of the node-at-a-time form (arity::unary, unary.rs:28-29): validity is
// not touched (the output column shares the operand's bitmap), so NULL slots are mapped like any other.  Two rows per lane through
// 16-byte accesses over the first `pairs` row pairs (the host passes 0 when either buffer is not 16-byte aligned), the rest one row
// per lane (one load in flight per lane: more of them, or more waves per CU, measured slower — see the launch site).  F is a
// template parameter: the abs instance is an `and` between a load and a store.
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
template <int F>
__global__ void __launch_bounds__(256) unary_f64_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, int64_t pairs, int64_t n) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, first = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const u64x2 *in2 = reinterpret_cast<const u64x2 *>(in);
    u64x2 *out2 = reinterpret_cast<u64x2 *>(out);
    for (int64_t j = first; j < pairs; j += stride) {
        u64x2 v = __builtin_nontemporal_load(in2 + j);
        v.x = apply_unary<F>(v.x);
        v.y = apply_unary<F>(v.y);
        __builtin_nontemporal_store(v, out2 + j);
    }
    for (int64_t j = 2 * pairs + first; j < n; j += stride) out[j] = apply_unary<F>(in[j]);
}

__global__ void fill_words_kernel(uint64_t *out, uint64_t v, int64_t n) {
    int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < n; j += stride) out[j] = v;
}

// ------------------------------------------------------------------ fused whole-tree evaluation
// A tree of binary and unary nodes is evaluated in ONE pass by a small stack machine: one instruction per BINARY or
// UNARY node (post-order), whose operands are a literal (SGPR broadcast), a pre-loaded column word, or the top of a
// register-resident stack of intermediate results.  A unary instruction (op = EX_OP_UNARY + nqe_unary_operator, b_src =
// EX_NONE) has the one operand a_src and replaces the top of the stack when that operand is the stack (depth unchanged),
// or pushes (depth + 1).  Control flow is wave-uniform (the program lives in the kernel arguments).
// Reads each referenced column once and writes the result once — no temporaries (the reference / arrow materialise one
// full column per node plus one per literal).
//
// Each wave walks 256-row chunks; a lane owns EX_ROWS rows (chunk + r*64 + lane: every access is a coalesced 512-byte
// wave access and a ballot is one bitmap word).  All column loads of a chunk are issued back to back before anything is
// consumed; the interpretive overhead (scalar instruction fetch, op/dtype branch chain) is paid once per EX_ROWS rows and
// the next instruction is fetched while the current one executes.  The stack keeps its top at level 0 by register moves:
// `stack op x` (the common left-deep shape) moves nothing.
// (the program — ExProgram, ExInstr, ExSrc and the EX_* limits — is defined in expr_plan.hpp, where build_program fills it)
template <int OP, int DT> struct OpTag { static constexpr int op = OP, dt = DT; };
// wave-uniform (op, dtype) → compile-time constants.  Boolean operands compare like UInt64 words (0/1).
template <class F> __device__ __forceinline__ void dispatch_binary(int op, int dt, F &&f) {
#define NQE_DISPATCH_OP(O)                                                                                                       \
    case O:                                                                                                                      \
        if (dt == NQE_INT64) f(OpTag<O, NQE_INT64>{});                                                                           \
        else if (dt == NQE_FLOAT64) f(OpTag<O, NQE_FLOAT64>{});                                                                  \
        else f(OpTag<O, NQE_UINT64>{});                                                                                          \
        break;
    switch (op) {
        NQE_DISPATCH_OP(NQE_OP_EQ) NQE_DISPATCH_OP(NQE_OP_NOT_EQ) NQE_DISPATCH_OP(NQE_OP_LT) NQE_DISPATCH_OP(NQE_OP_LT_EQ)
        NQE_DISPATCH_OP(NQE_OP_GT) NQE_DISPATCH_OP(NQE_OP_GT_EQ) NQE_DISPATCH_OP(NQE_OP_PLUS) NQE_DISPATCH_OP(NQE_OP_MINUS)
        NQE_DISPATCH_OP(NQE_OP_MULTIPLY) NQE_DISPATCH_OP(NQE_OP_DIVIDE)
    default: // NQE_OP_MODULOS
        if (dt == NQE_INT64) f(OpTag<NQE_OP_MODULOS, NQE_INT64>{});
        else if (dt == NQE_FLOAT64) f(OpTag<NQE_OP_MODULOS, NQE_FLOAT64>{});
        else f(OpTag<NQE_OP_MODULOS, NQE_UINT64>{});
        break;
    }
#undef NQE_DISPATCH_OP
}

__device__ __forceinline__ void ex_combine(const ExInstr &in, uint64_t &a, bool &av, uint64_t b, bool bv, int *flags) {
    if (in.op == NQE_OP_AND || in.op == NQE_OP_OR) { // and_kleene / or_kleene
        bool lb = av && a, rb = bv && b, ok, r;
        if (in.op == NQE_OP_AND) { ok = (av && bv) || (av && !lb) || (bv && !rb); r = ok && lb && rb; }
        else { ok = (av && bv) || lb || rb; r = ok && (lb || rb); }
        a = r ? 1ull : 0ull;
        av = ok;
    } else {
        bool ok = av && bv;
        a = apply_binary(in.op, in.dt, a, b, in.aux, ok, flags);
        av = ok;
    }
}

// Loads the EX_ROWS rows a lane owns (row0 + r*64) of every program column; `inm` = rows that exist / are wanted.
// NULLS = false: no column has a validity bitmap and no literal is NULL, so every mask equals `inm` and none is computed
// (the kernel is VALU-issue bound once the program has a few instructions; mask bookkeeping is ~40% of it).
template <bool NULLS, int NC, int R = EX_ROWS>
__device__ __forceinline__ void ex_load(const ExProgram &P, int64_t row0, int64_t n, uint32_t inm, uint64_t (&cw)[NC][R], uint32_t (&cvm)[NC]) {
    // issue every load of the chunk (rows clamped to n-1 so that no load is predicated), then consume
    int64_t rc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rc[r] = min(row0 + r * 64, n - 1);
    uint32_t vbyte[NC][R];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int r = 0; r < R; ++r) { cw[c][r] = 0; vbyte[c][r] = 0xffu; }
        if (c < P.ncols) {
            if (P.col_dtype[c] == NQE_BOOLEAN) {
#pragma unroll
                for (int r = 0; r < R; ++r) cw[c][r] = static_cast<const uint8_t *>(P.col_values[c])[rc[r] >> 3];
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) cw[c][r] = __builtin_nontemporal_load(static_cast<const uint64_t *>(P.col_values[c]) + rc[r]);
            }
            if (NULLS && P.col_valid[c]) {
#pragma unroll
                for (int r = 0; r < R; ++r) vbyte[c][r] = P.col_valid[c][rc[r] >> 3];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        cvm[c] = inm;
        if (c < P.ncols) {
            if (P.col_dtype[c] == NQE_BOOLEAN) {
#pragma unroll
                for (int r = 0; r < R; ++r) cw[c][r] = (cw[c][r] >> (int(rc[r]) & 7)) & 1ull;
            }
            if (NULLS && P.col_valid[c]) {
                uint32_t m = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) m |= ((vbyte[c][r] >> (int(rc[r]) & 7)) & 1u) << r;
                cvm[c] = m & inm;
            }
        }
    }
}

// Runs the program on the loaded rows; the result words are left in res[], the returned mask holds their validity.
// TRIG = false: the program holds no sin / cos step (the host checks), so that instance carries no transcendental code and
// keeps the register budget of a purely arithmetic machine.
template <bool NULLS, int NC, int R = EX_ROWS, bool TRIG = false>
__device__ __forceinline__ uint32_t ex_run(const ExProgram &P, const uint64_t (&cw)[NC][R], const uint32_t (&cvm)[NC],
                                           uint32_t inm, uint32_t litm, uint64_t (&res)[R], int *flags) {
    // ---- run the program
    uint64_t s[EX_MAX_DEPTH][R];
    uint32_t vm[EX_MAX_DEPTH];
#pragma unroll
    for (int d = 0; d < EX_MAX_DEPTH; ++d) {
        vm[d] = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) s[d][r] = 0;
    }
    ExInstr cur = P.ins[0];
    for (int pc = 0; pc < P.n; ++pc) {
        const ExInstr nxt = P.ins[pc + 1 < P.n ? pc + 1 : pc]; // in flight while `cur` executes
        const bool a_st = cur.a_src == EX_STACK, b_st = cur.b_src == EX_STACK;
        const int ac = cur.a_src - EX_COL, bc = cur.b_src - EX_COL;
        // Operand fetch and stack update are wave-uniform BRANCHES around plain register moves: a select costs VALU
        // issue slots per row, a scalar branch does not, and the budget to stay HBM-bound is ~130 VALU instructions per
        // 64 rows for the whole program.  Everything is copied by value with constant indices (a conditional over array
        // lvalues would turn the stack into a dynamically indexed private array, i.e. scratch memory).
        uint64_t a[R], b[R];
        uint32_t am, bm;
        if (a_st) {
            if (b_st) {
                am = vm[1];
#pragma unroll
                for (int r = 0; r < R; ++r) a[r] = s[1][r];
            } else {
                am = vm[0];
#pragma unroll
                for (int r = 0; r < R; ++r) a[r] = s[0][r];
            }
        } else if (ac < 0) {
            am = cur.a_src == EX_LIT ? litm : 0u;
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = cur.lit_a;
        } else if (ac == 0) {
            am = cvm[0];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = cw[0][r];
        } else if (NC <= 2 || ac == 1) {
            am = cvm[1];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = cw[1][r];
        } else if (ac == 2) {
            am = cvm[NC > 2 ? 2 : 0];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = cw[NC > 2 ? 2 : 0][r];
        } else {
            am = cvm[NC > 2 ? 3 : 0];
#pragma unroll
            for (int r = 0; r < R; ++r) a[r] = cw[NC > 2 ? 3 : 0][r];
        }
        if (b_st) {
            bm = vm[0];
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = s[0][r];
        } else if (bc < 0) {
            bm = cur.b_src == EX_LIT ? litm : 0u;
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = cur.lit_b;
        } else if (bc == 0) {
            bm = cvm[0];
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = cw[0][r];
        } else if (NC <= 2 || bc == 1) {
            bm = cvm[1];
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = cw[1][r];
        } else if (bc == 2) {
            bm = cvm[NC > 2 ? 2 : 0];
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = cw[NC > 2 ? 2 : 0][r];
        } else {
            bm = cvm[NC > 2 ? 3 : 0];
#pragma unroll
            for (int r = 0; r < R; ++r) b[r] = cw[NC > 2 ? 3 : 0][r];
        }
        uint32_t m;
        if (cur.op >= EX_OP_UNARY) { // one operand (b is unused): the value is mapped, the validity passes through
            m = NULLS ? am : inm;
            const int f = cur.op - EX_OP_UNARY;
            if (f == NQE_UNARY_ABS) {
#pragma unroll
                for (int r = 0; r < R; ++r) a[r] = apply_unary<NQE_UNARY_ABS>(a[r]);
            } else if (TRIG) {
                if (f == NQE_UNARY_SIN) {
#pragma unroll
                    for (int r = 0; r < R; ++r) a[r] = apply_unary<NQE_UNARY_SIN>(a[r]);
                } else { // Cos, and Tan (quirk Q16)
#pragma unroll
                    for (int r = 0; r < R; ++r) a[r] = apply_unary<NQE_UNARY_COS>(a[r]);
                }
            }
        } else if (cur.op == NQE_OP_AND || cur.op == NQE_OP_OR) {
            if (NULLS) { // and_kleene / or_kleene
                m = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    bool av = (am >> r) & 1u;
                    ex_combine(cur, a[r], av, b[r], (bm >> r) & 1u, flags);
                    m |= (av ? 1u : 0u) << r;
                }
            } else {
                m = inm;
                if (cur.op == NQE_OP_AND) {
#pragma unroll
                    for (int r = 0; r < R; ++r) a[r] &= b[r];
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r) a[r] |= b[r];
                }
            }
        } else {
            m = NULLS ? (am & bm) : inm;
            // one uniform op/dtype decision per instruction (not per row): the body is instantiated with constants
            dispatch_binary(cur.op, cur.dt, [&](auto tag) {
#pragma unroll
                for (int r = 0; r < R; ++r) a[r] = apply_binary(tag.op, tag.dt, a[r], b[r], cur.aux, (m >> r) & 1u, flags);
            });
        }
        if (a_st && b_st) { // pop 2, push 1 (a unary step over the stack: neither branch — the top is replaced in place)
            vm[1] = vm[2];
#pragma unroll
            for (int r = 0; r < R; ++r) s[1][r] = s[2][r];
        } else if (!a_st && !b_st) { // push
            vm[2] = vm[1];
            vm[1] = vm[0];
#pragma unroll
            for (int r = 0; r < R; ++r) { s[2][r] = s[1][r]; s[1][r] = s[0][r]; }
        }
        vm[0] = m;
#pragma unroll
        for (int r = 0; r < R; ++r) s[0][r] = a[r];
        cur = nxt;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) res[r] = s[0][r];
    return vm[0];
}

// R rows per lane: the dispatch of an instruction (scalar work) is paid once per R x 64 rows; 4 by default (8 halves the scalar work
// but takes 176 VGPRs — see the launch site)
template <bool NULLS, int NC, int R = EX_ROWS, bool TRIG = false>
__global__ void __launch_bounds__(256) expr_tree_kernel(ExProgram P, int64_t n, uint64_t *out_words, uint64_t *out_bits, uint64_t *out_valid,
                                                        int *flags) {
    const int lane = lane_id();
    const int64_t n_chunks = (n + 64 * R - 1) / (64 * R);
    const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, n_waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t chunk = wave; chunk < n_chunks; chunk += n_waves) {
        const int64_t row0 = chunk * (64 * R) + lane;
        uint32_t inm = 0; // one bit per owned row
#pragma unroll
        for (int r = 0; r < R; ++r) inm |= (row0 + r * 64 < n ? 1u : 0u) << r;
        uint64_t cw[NC][R], res[R];
        uint32_t cvm[NC];
        ex_load<NULLS, NC, R>(P, row0, n, inm, cw, cvm);
        const uint32_t vm = ex_run<NULLS, NC, R, TRIG>(P, cw, cvm, inm, inm, res, flags);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = row0 + r * 64;
            const bool ok = (vm >> r) & 1u;
            if (row - lane >= n) break; // wave-uniform: this 64-row word is past the end
            if (out_words) {
                if (row < n) __builtin_nontemporal_store(ok ? res[r] : 0ull, out_words + row);
            } else {
                uint64_t w = __ballot(ok && res[r]);
                if (lane == 0) out_bits[row >> 6] = w;
            }
            if (out_valid) {
                uint64_t w = __ballot(ok);
                if (lane == 0) out_valid[row >> 6] = w;
            }
        }
    }
}

// The same machine behind a selection: one wave per 4096-row tile of the keep bitmap (word k of the tile in lane k, as in
// compact_kernel); only the rows the filter emits are evaluated as valid (a dropped row can never raise DivideByZero,
// as in the reference where the projection runs on the filtered batch), 256-row chunks without any kept row are not even
// loaded, and results go straight to their compacted position.  A NULL predicate emits a NULL row (quirk Q4).
template <bool NULLS, int NC, bool TRIG = false>
__global__ void __launch_bounds__(256) expr_tree_compact_kernel(ExProgram P, const uint64_t *keep, const uint64_t *pvalid,
                                                                const uint64_t *tile_offsets, int64_t n, int64_t ntiles, uint64_t *out_words,
                                                                uint8_t *out_bool_bytes, uint8_t *out_valid_bytes, int *flags) {
    constexpr int R = EX_ROWS;
    const int lane = lane_id();
    const int waves_per_block = blockDim.x / 64;
    const int64_t nwords = (n + 63) / 64;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles; tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t w = tile * TILE_WORDS + lane;
        const uint64_t my_word = w < nwords ? keep[w] : 0;
        const uint64_t my_pv = (pvalid && w < nwords) ? pvalid[w] : ~0ull;
        uint32_t tot;
        const uint32_t my_off = wave_exclusive_scan(uint32_t(__popcll(my_word)), tot);
        if (tot == 0) continue;
        const uint64_t base = tile_offsets[tile];
        for (int k0 = 0; k0 < TILE_WORDS; k0 += R) {
            uint64_t kw[R];
            // inm: emitted rows whose predicate was valid (column values count); litm: every emitted row — a row emitted for
            // a NULL predicate is all-NULL in the reference's filtered batch, but literals are still valid there
            // (NULL OR true = true), found by the differential fuzzer
            uint32_t inm = 0, litm = 0, anyk = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                kw[r] = bcast64(my_word, k0 + r);
                anyk |= kw[r] != 0 ? 1u : 0u;
                litm |= uint32_t((kw[r] >> lane) & 1ull) << r;
                inm |= uint32_t(((kw[r] & bcast64(my_pv, k0 + r)) >> lane) & 1ull) << r;
            }
            if (!anyk) continue; // wave-uniform
            const int64_t row0 = (tile * TILE_WORDS + k0) * 64 + lane;
            uint64_t cw[NC][R], res[R];
            uint32_t cvm[NC];
            ex_load<NULLS, NC>(P, row0, n, inm, cw, cvm);
            const uint32_t vm = ex_run<NULLS, NC, R, TRIG>(P, cw, cvm, inm, litm, res, flags);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if ((kw[r] >> lane) & 1ull) {
                    const bool ok = (vm >> r) & 1u;
                    const uint64_t pos = base + bcast32(my_off, k0 + r) + __popcll(kw[r] & lanemask_lt());
                    if (out_words) __builtin_nontemporal_store(ok ? res[r] : 0ull, out_words + pos);
                    if (out_bool_bytes) out_bool_bytes[pos] = (ok && res[r]) ? 1 : 0;
                    if (out_valid_bytes) out_valid_bytes[pos] = ok ? 1 : 0;
                }
            }
        }
    }
}

} // namespace
} // namespace nqe
