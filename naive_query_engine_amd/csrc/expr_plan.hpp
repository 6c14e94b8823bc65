// expr_plan.hpp — the host side of expressions: the tree parser and type checker, the recognisers of the shapes that consumer kernels
// fuse (SimpleExpr, FastPred, ConjPred, TreePred: expr_shapes.hpp) and the builder of the stack machine's program (ExProgram, run by
// expr_kernels.hpp and restated as source by expr_jit.hpp).  They decide which kernel a query takes and with what constants.
// Plain C++17, no HIP and no nqe_table: the input is seen through ExprView, so tests/cpp/test_expr_plan.cpp compiles this header alone.
//
// The types live directly in nqe's unnamed namespace (the kernels of the one including unit take ExProgram by value); the functions in
// `plan` below it — nqe_internal.hpp declares some of them over nqe_table under the same names, which expr.hip forwards here.
#pragma once

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "expr_shapes.hpp"
#include "nqe_error.hpp"

namespace nqe {
namespace {

// what the functions here see of an input table: per column its dtype, values pointer, validity pointer and length
struct ExprView {
    struct Col {
        int dtype = NQE_NULLTYPE;
        bool has_values = false; // the column holds a values buffer (whose address may still be null: a borrowed column of no rows)
        const void *values = nullptr;
        const uint8_t *valid = nullptr; // null: no NULLs
        int64_t length = 0;
    };
    std::vector<Col> cols;
};

struct Node {
    int kind = 0, op = 0, column = 0, dtype = 0;
    bool lit_null = false;
    uint64_t lit = 0;
    std::string lit_str;       // Utf8 literal
    int left = -1, right = -1; // children (indices into the node vector); a UNARY node's operand is `left`
    int third = -1;            // a STRING_ARGS node's last argument (SUBSTR's len, REPLACE's to): left = s, right = the first argument;
                               // a CONDITIONAL node: left = the first operand (NOT's b, IS_NULL's x, a, IF's c), right = b or t, third = IF's e
    int out_dtype = NQE_NULLTYPE;
};

bool is_compare(int op) { return op >= NQE_OP_EQ && op <= NQE_OP_GT_EQ; }
bool is_logic(int op) { return op == NQE_OP_AND || op == NQE_OP_OR; }
bool is_arith(int op) { return op >= NQE_OP_PLUS && op <= NQE_OP_MODULOS; }
bool is_string_node(int kind) { return kind == NQE_EXPR_STRING || kind == NQE_EXPR_STRING_ARGS || kind == NQE_EXPR_STRING_MATCH; } // Q25, Q26 and Q27: evaluated node at a time
bool is_node_at_a_time(int kind) { return is_string_node(kind) || kind == NQE_EXPR_CONDITIONAL || kind == NQE_EXPR_CAST; } // Q25-Q27, Q28's conditional node and Q29's cast: no step of the stack machine
bool is_op_node(int kind) { return kind == NQE_EXPR_BINARY || kind == NQE_EXPR_UNARY || is_node_at_a_time(kind); } // a node with operands: a step of a program
// the values a CONDITIONAL node's function pops (quirk Q28); 0: `op` is outside nqe_cond_operator
int cond_arity(int op) { return op < NQE_COND_NOT || op > NQE_COND_IF ? 0 : op <= NQE_COND_IS_NOT_NULL ? 1 : op == NQE_COND_IF ? 3 : 2; }

// ------------------------------------------------------------------ fused whole-tree evaluation: the stack machine's program
// One instruction per BINARY or UNARY node (post-order), whose operands are a literal, a column word (slot k of the program's distinct
// columns), or the top of a stack of intermediate results, at most EX_MAX_DEPTH deep.  A unary instruction (op = EX_OP_UNARY +
// nqe_unary_operator, b_src = EX_NONE) has the one operand a_src and replaces the top of the stack when that operand is the stack (depth
// unchanged), or pushes (depth + 1).  How the machine runs it: expr_kernels.hpp.
constexpr int EX_MAX_INSTR = 16, EX_MAX_COLS = 4, EX_MAX_DEPTH = 3, EX_ROWS = 4;
enum ExSrc : int32_t { EX_STACK = 0, EX_LIT = 1, EX_LIT_NULL = 2, EX_NONE = 3 /* b_src of a unary instruction */, EX_COL = 4 /* + slot */ };
constexpr int32_t EX_OP_UNARY = 32; // ExInstr::op of a unary instruction: EX_OP_UNARY + nqe_unary_operator (above every nqe_operator)
struct ExInstr {
    int32_t op, dt;       // operator (binary: nqe_operator; unary: EX_OP_UNARY + nqe_unary_operator), operand dtype
    int32_t a_src, b_src; // ExSrc
    uint64_t lit_a, lit_b;
    OpAux aux;            // host-prepared divisor constants when b is a literal
};
struct ExProgram {
    int32_t n, ncols;
    ExInstr ins[EX_MAX_INSTR];
    const void *col_values[EX_MAX_COLS];
    const uint8_t *col_valid[EX_MAX_COLS];
    int32_t col_dtype[EX_MAX_COLS];
};

// The distinct columns — (values, valid, dtype) — that a program, or the programs of one specialised kernel, read: slot k is the k-th
// column met.  The policy comes with each call: how many slots the consumer has, and whether it takes only 8-byte columns without NULLs.
constexpr int SLOT_MAX = 8;
struct SlotTable {
    int n = 0;
    const void *values[SLOT_MAX] = {};
    const uint8_t *valid[SLOT_MAX] = {};
    int32_t dtype[SLOT_MAX] = {};
    void store(ExProgram *P) const { // as a program's own columns
        P->ncols = n;
        for (int k = 0; k < n; ++k) { P->col_values[k] = values[k]; P->col_valid[k] = valid[k]; P->col_dtype[k] = dtype[k]; }
    }
    // the column's slot, appended when it is new; -1: no slot left, or a nullable / bit-packed column where only plain words are taken
    int slot_of(const void *v, const uint8_t *vd, int dt, int capacity, bool plain_words_only = false) {
        if (plain_words_only && (vd || !is_word_type(dt))) return -1;
        for (int k = 0; k < n; ++k)
            if (values[k] == v && valid[k] == vd && dtype[k] == dt) return k;
        if (n == capacity) return -1;
        values[n] = v;
        valid[n] = vd;
        dtype[n] = dt;
        return n++;
    }
    // rewrites the column operands of P (numbered by P's own columns) to this table's slots; false: a column found no slot, or P holds
    // a NULL literal the consumer refuses.  used_mask collects the slots P reads.
    bool renumber(ExProgram &P, int capacity, bool plain_words_only, uint32_t *used_mask = nullptr, bool refuse_null_literal = false) {
        for (int i = 0; i < P.n; ++i) {
            ExInstr &I = P.ins[i];
            for (int32_t *src : {&I.a_src, &I.b_src}) {
                if (refuse_null_literal && *src == EX_LIT_NULL) return false;
                if (*src < EX_COL) continue;
                const int k = *src - EX_COL, u = slot_of(P.col_values[k], P.col_valid[k], P.col_dtype[k], capacity, plain_words_only);
                if (u < 0) return false;
                *src = EX_COL + u;
                if (used_mask) *used_mask |= 1u << u;
            }
        }
        return true;
    }
};

namespace plan {

// builds the tree and type-checks it exactly where binary.rs and unary.rs do
std::vector<Node> parse(const ExprView &in, const nqe_expr_node *nodes, int n, int *root) {
    if (!nodes || n <= 0) fail(NQE_ERR_INVALID_ARGUMENT, "empty expression");
    std::vector<Node> t;
    std::vector<int> st;
    for (int i = 0; i < n; ++i) {
        const nqe_expr_node &nd = nodes[i];
        Node x;
        x.kind = nd.kind;
        if (nd.kind == NQE_EXPR_COLUMN) {
            if (nd.column < 0 || size_t(nd.column) >= in.cols.size())
                fail(NQE_ERR_NOT_SUPPORTED, "column index out of range (RecordBatch::column panics)");
            x.column = nd.column;
            x.out_dtype = in.cols[size_t(nd.column)].dtype;
        } else if (nd.kind == NQE_EXPR_LITERAL) {
            x.dtype = nd.dtype;
            x.lit_null = nd.is_null != 0 || nd.dtype == NQE_NULLTYPE;
            x.lit = nd.dtype == NQE_BOOLEAN ? uint64_t(nd.value.boolean != 0) : nd.value.u64;
            x.out_dtype = nd.dtype;
            if (nd.dtype == NQE_UTF8) {
                x.lit = 0;
                if (!x.lit_null) {
                    if (nd.utf8_length < 0 || (nd.utf8_length > 0 && !nd.value.utf8)) fail(NQE_ERR_INVALID_ARGUMENT, "Utf8 literal without bytes");
                    x.lit_str.assign(nd.value.utf8 ? nd.value.utf8 : "", size_t(nd.utf8_length));
                }
            }
        } else if (nd.kind == NQE_EXPR_BINARY) {
            if (st.size() < 2) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            x.right = st.back(); st.pop_back();
            x.left = st.back(); st.pop_back();
            x.op = nd.op;
            int ldt = t[size_t(x.left)].out_dtype, rdt = t[size_t(x.right)].out_dtype;
            if (ldt != rdt) // binary.rs:114-119
                fail(NQE_ERR_INTERVAL, "Cannot evaluate binary expression with types " + std::to_string(ldt) + " and " +
                                           std::to_string(rdt));
            if (is_compare(x.op)) {
                if (ldt == NQE_NULLTYPE) fail(NQE_ERR_ARROW, "comparison on Null arrays is not supported");
                x.out_dtype = NQE_BOOLEAN;
            } else if (is_logic(x.op)) {
                if (ldt != NQE_BOOLEAN) // binary_op! (binary.rs:32-42)
                    fail(NQE_ERR_INTERVAL, "Cannot evaluate binary expression And/Or with non-Boolean types");
                x.out_dtype = NQE_BOOLEAN;
            } else if (is_arith(x.op)) {
                if (!is_word_type(ldt)) // arithemic_op! `_ => unimplemented!()` (binary.rs:85)
                    fail(NQE_ERR_NOT_SUPPORTED, "arithmetic on this type is unimplemented!() (binary.rs:85)");
                x.out_dtype = ldt;
            } else {
                fail(NQE_ERR_INVALID_ARGUMENT, "unknown operator");
            }
        } else if (nd.kind == NQE_EXPR_UNARY) { // unary.rs:85-108
            if (st.empty()) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            x.left = st.back(); st.pop_back();
            x.op = nd.op;
            if (x.op < NQE_UNARY_ABS || x.op > NQE_UNARY_SUBSTR) fail(NQE_ERR_INVALID_ARGUMENT, "unknown unary operator");
            if (x.op > NQE_UNARY_TAN) fail(NQE_ERR_NOT_SUPPORTED, "the string functions are todo!() (unary.rs:97-106)");
            if (t[size_t(x.left)].out_dtype != NQE_FLOAT64) // unary_arith_op! `_ => unimplemented!()` (unary.rs:41)
                fail(NQE_ERR_NOT_SUPPORTED, "unary math functions on this type are unimplemented!() (unary.rs:41)");
            x.out_dtype = NQE_FLOAT64;
        } else if (nd.kind == NQE_EXPR_STRING) { // quirk Q25: the string functions, given a body (string_fn.hip)
            if (st.empty()) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            x.left = st.back(); st.pop_back();
            x.op = nd.op;
            if (x.op < NQE_UNARY_ABS || x.op > NQE_UNARY_SUBSTR) fail(NQE_ERR_INVALID_ARGUMENT, "unknown string function");
            if (x.op <= NQE_UNARY_TAN) fail(NQE_ERR_INVALID_ARGUMENT, "a math function under a string node (it belongs under NQE_EXPR_UNARY)");
            if (x.op == NQE_UNARY_REPEAT || x.op == NQE_UNARY_REPLACE || x.op == NQE_UNARY_SUBSTR)
                fail(NQE_ERR_NOT_SUPPORTED, "repeat / replace / substr need arguments a one-operand node cannot carry");
            if (t[size_t(x.left)].out_dtype != NQE_UTF8) fail(NQE_ERR_NOT_SUPPORTED, "a string function over an operand that is not Utf8");
            x.out_dtype = x.op == NQE_UNARY_CHARACTER_LENGTH ? NQE_INT64 : NQE_UTF8;
        } else if (nd.kind == NQE_EXPR_STRING_ARGS) { // quirk Q26: substr / repeat / replace (string_args.hip)
            x.op = nd.op;
            if (x.op < NQE_UNARY_ABS || x.op > NQE_UNARY_SUBSTR) fail(NQE_ERR_INVALID_ARGUMENT, "unknown string function");
            if (x.op != NQE_UNARY_REPEAT && x.op != NQE_UNARY_REPLACE && x.op != NQE_UNARY_SUBSTR)
                fail(NQE_ERR_INVALID_ARGUMENT, "a function without arguments under a string-arguments node (it belongs under NQE_EXPR_UNARY or NQE_EXPR_STRING)");
            const size_t pops = x.op == NQE_UNARY_REPEAT ? 2 : 3;
            if (st.size() < pops) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            if (pops == 3) { x.third = st.back(); st.pop_back(); }
            x.right = st.back(); st.pop_back();
            x.left = st.back(); st.pop_back();
            if (t[size_t(x.left)].out_dtype != NQE_UTF8) fail(NQE_ERR_NOT_SUPPORTED, "a string function over an operand that is not Utf8");
            for (int a : {x.right, x.third}) {
                if (a < 0) continue;
                const Node &arg = t[size_t(a)];
                if (x.op == NQE_UNARY_REPLACE) {
                    if (arg.kind != NQE_EXPR_LITERAL || arg.dtype != NQE_UTF8) fail(NQE_ERR_NOT_SUPPORTED, "replace takes Utf8 literals for `from` and `to`");
                } else if (arg.out_dtype != NQE_INT64)
                    fail(NQE_ERR_NOT_SUPPORTED, "substr / repeat take Int64 arguments");
            }
            x.out_dtype = NQE_UTF8;
        } else if (nd.kind == NQE_EXPR_STRING_MATCH) { // quirk Q27: like / ilike / starts_with / ends_with / contains / strpos (string_match.hip)
            x.op = nd.op;
            if (x.op < NQE_MATCH_LIKE || x.op > NQE_MATCH_STRPOS) fail(NQE_ERR_INVALID_ARGUMENT, "unknown match operator");
            if (st.size() < 2) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            x.right = st.back(); st.pop_back();
            x.left = st.back(); st.pop_back();
            if (t[size_t(x.left)].out_dtype != NQE_UTF8) fail(NQE_ERR_NOT_SUPPORTED, "a string match over an operand that is not Utf8");
            const Node &pat = t[size_t(x.right)];
            if (pat.kind != NQE_EXPR_LITERAL || pat.dtype != NQE_UTF8) fail(NQE_ERR_NOT_SUPPORTED, "a string match takes a Utf8 literal for the pattern");
            if (pat.lit_str.size() > size_t(NQE_MAX_MATCH_PATTERN)) fail(NQE_ERR_NOT_SUPPORTED, "a pattern of more than NQE_MAX_MATCH_PATTERN bytes");
            x.out_dtype = x.op == NQE_MATCH_STRPOS ? NQE_INT64 : NQE_BOOLEAN;
        } else if (nd.kind == NQE_EXPR_CONDITIONAL) { // quirk Q28: not / is_null / is_not_null / coalesce / nullif / if (conditional.hip)
            if (nd.column < 1 || nd.column > 3) fail(NQE_ERR_INVALID_ARGUMENT, "a conditional node pops one to three values (its `column` field)");
            x.op = nd.op;
            const int pops = cond_arity(x.op);
            if (pops == 0) fail(NQE_ERR_INVALID_ARGUMENT, "unknown conditional operator");
            if (nd.column != pops) fail(NQE_ERR_INVALID_ARGUMENT, "a conditional node whose `column` field is not its function's arity");
            if (st.size() < size_t(pops)) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            if (pops == 3) { x.third = st.back(); st.pop_back(); }
            if (pops >= 2) { x.right = st.back(); st.pop_back(); }
            x.left = st.back(); st.pop_back();
            for (int a : {x.left, x.right, x.third})
                if (a >= 0 && t[size_t(a)].out_dtype == NQE_NULLTYPE) fail(NQE_ERR_NOT_SUPPORTED, "Null-typed arrays are not supported on the device path");
            const int first = t[size_t(x.left)].out_dtype;
            if ((x.op == NQE_COND_NOT || x.op == NQE_COND_IF) && first != NQE_BOOLEAN)
                fail(NQE_ERR_INTERVAL, "Cannot evaluate Not / If with a non-Boolean condition");
            if (pops >= 2) {
                const int adt = t[size_t(pops == 3 ? x.right : x.left)].out_dtype, bdt = t[size_t(pops == 3 ? x.third : x.right)].out_dtype;
                if (adt != bdt) fail(NQE_ERR_INTERVAL, "Cannot evaluate conditional expression with types " + std::to_string(adt) + " and " + std::to_string(bdt));
                x.out_dtype = adt;
            } else
                x.out_dtype = NQE_BOOLEAN;
        } else if (nd.kind == NQE_EXPR_CAST) { // quirk Q29: `x CAST`, the target in `dtype` (cast.hip)
            if (nd.dtype < NQE_BOOLEAN || nd.dtype > NQE_UTF8) fail(NQE_ERR_INVALID_ARGUMENT, "a cast node whose `dtype` field is not a target type (Boolean .. Utf8)");
            if (st.empty()) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
            x.left = st.back(); st.pop_back();
            x.dtype = nd.dtype;
            const int from = t[size_t(x.left)].out_dtype;
            if (from == NQE_NULLTYPE) fail(NQE_ERR_NOT_SUPPORTED, "Null-typed arrays are not supported on the device path");
            if (from == NQE_FLOAT64 && nd.dtype == NQE_UTF8) fail(NQE_ERR_NOT_SUPPORTED, "a cast of Float64 to Utf8 (shortest-round-trip digits) is not supported");
            x.out_dtype = nd.dtype;
        } else {
            fail(NQE_ERR_INVALID_ARGUMENT, "unknown expression node kind");
        }
        t.push_back(x);
        st.push_back(int(t.size()) - 1);
    }
    if (st.size() != 1) fail(NQE_ERR_INVALID_ARGUMENT, "malformed expression");
    *root = st[0];
    return t;
}

OpAux make_aux(int op, int dt, uint64_t lit) {
    OpAux a;
    a.pow2_shift = -1;
    a.more = -1;
    a.abs_lit = 0;
    a.magic = 0;
    if (op == NQE_OP_DIVIDE && dt == NQE_FLOAT64) {
        // x / ±2^k  ==  x * ±2^-k bit for bit (scaling by a power of two is exact; where the quotient is subnormal both round the same
        // real number): a multiplication instead of the ~40-instruction Float64 division — when 2^k and 2^-k are both normal
        const uint64_t mant = lit & 0x000fffffffffffffull, ex = (lit >> 52) & 0x7ff;
        if (mant == 0 && ex >= 2 && ex <= 2044) {
            a.more = -2;
            a.magic = (lit & 0x8000000000000000ull) | ((2046 - ex) << 52);
        }
        return a;
    }
    if ((op == NQE_OP_DIVIDE || op == NQE_OP_MODULOS) && (dt == NQE_INT64 || dt == NQE_UINT64) && lit != 0) {
        uint64_t ab = lit;
        if (dt == NQE_INT64 && int64_t(lit) < 0) ab = 0ull - lit;
        a.abs_lit = ab;
        if ((ab & (ab - 1)) == 0) {
            int s = 0;
            while ((ab >> s) != 1) ++s;
            a.pow2_shift = s;
        } else {
            // unsigned 64-bit division by an invariant divisor (Granlund–Montgomery, the branch-free "add"
            // form): magic = floor(2^(64+L) / d) * 2 + adjustment + 1 with L = floor(log2 d)
            int L = 63;
            while (!((ab >> L) & 1)) --L;
            unsigned __int128 num = (unsigned __int128)1 << (64 + L);
            uint64_t pm = uint64_t(num / ab);
            uint64_t rem = uint64_t(num % ab);
            pm += pm;
            uint64_t twice = rem + rem;
            if (twice >= ab || twice < rem) pm += 1;
            a.magic = pm + 1;
            a.more = L;
        }
    }
    return a;
}

// col [op lit]{0,SIMPLE_MAX_OPS}
bool match_simple(const std::vector<Node> &t, int i, SimpleExpr *s) {
    const Node &x = t[size_t(i)];
    if (x.kind == NQE_EXPR_COLUMN) {
        std::memset(s, 0, sizeof(*s));
        s->col = x.column;
        s->src_dtype = x.out_dtype;
        s->out_dtype = x.out_dtype;
        for (int k = 0; k < SIMPLE_MAX_OPS; ++k) s->aux[k].pow2_shift = s->aux[k].more = -1;
        return true; // a bare column of any type (Utf8 included) passes through
    }
    if (x.kind != NQE_EXPR_BINARY || is_logic(x.op)) return false; // (a UNARY, STRING, STRING_MATCH or CONDITIONAL step anywhere below ends the chain here too)
    const Node &l = t[size_t(x.left)], &r = t[size_t(x.right)];
    bool lit_left;
    int sub;
    const Node *litn;
    if (r.kind == NQE_EXPR_LITERAL && !r.lit_null && l.kind != NQE_EXPR_LITERAL) {
        lit_left = false; sub = x.left; litn = &r;
    } else if (l.kind == NQE_EXPR_LITERAL && !l.lit_null && r.kind != NQE_EXPR_LITERAL) {
        lit_left = true; sub = x.right; litn = &l;
    } else {
        return false;
    }
    if (litn->dtype == NQE_UTF8) return false; // string compares have their own kernel
    if (!match_simple(t, sub, s) || s->nops >= SIMPLE_MAX_OPS) return false;
    int k = s->nops++;
    s->op[k] = x.op;
    s->lit_left[k] = lit_left ? 1 : 0;
    s->op_dtype[k] = litn->dtype;
    s->lit[k] = litn->lit;
    s->aux[k] = lit_left ? make_aux(0, 0, 0) : make_aux(x.op, litn->dtype, litn->lit);
    s->out_dtype = x.out_dtype;
    return true;
}

// builds the stack program; false when the tree does not fit the machine (then: node-at-a-time)
bool build_program(const ExprView &in, const std::vector<Node> &t, int root, ExProgram *P, bool *needs_valid) {
    std::memset(P, 0, sizeof(*P));
    if (getenv("NQE_NO_EXPR_TREE")) return false; // diagnostics (A/B, parity tests): every tree node-at-a-time
    std::vector<int> order; // BINARY and UNARY nodes, post-order
    std::vector<std::pair<int, bool>> st = {{root, false}};
    while (!st.empty()) {
        auto [i, done] = st.back();
        st.pop_back();
        const Node &x = t[size_t(i)];
        if (!is_op_node(x.kind)) continue;
        if (is_node_at_a_time(x.kind)) return false; // the machine works on 8-byte words and has no select: a tree that holds a string or conditional node goes node at a time
        if (done) { order.push_back(i); continue; }
        st.push_back({i, true});
        if (x.kind == NQE_EXPR_BINARY) st.push_back({x.right, false});
        st.push_back({x.left, false});
    }
    if (int(order.size()) > EX_MAX_INSTR || order.empty()) return false;
    *needs_valid = false;
    bool fits = true;
    SlotTable slots;
    auto operand = [&](int idx, int32_t *src, uint64_t *lit) {
        const Node &x = t[size_t(idx)];
        if (is_op_node(x.kind)) { *src = EX_STACK; return; }
        if (x.kind == NQE_EXPR_LITERAL) {
            if (x.dtype == NQE_UTF8) { fits = false; return; }
            *src = x.lit_null ? EX_LIT_NULL : EX_LIT;
            *lit = x.lit;
            *needs_valid |= x.lit_null;
            return;
        }
        const ExprView::Col &c = in.cols[size_t(x.column)];
        if (!(is_word_type(c.dtype) || c.dtype == NQE_BOOLEAN)) { fits = false; return; }
        const int slot = slots.slot_of(c.values, c.valid, c.dtype, EX_MAX_COLS);
        if (slot < 0) { fits = false; return; }
        *src = EX_COL + slot;
        *needs_valid |= c.valid != nullptr;
    };
    int depth = 0;
    for (int i : order) {
        const Node &x = t[size_t(i)];
        ExInstr &I = P->ins[P->n++];
        I.dt = t[size_t(x.left)].out_dtype;
        I.aux.pow2_shift = I.aux.more = -1;
        operand(x.left, &I.a_src, &I.lit_a);
        if (x.kind == NQE_EXPR_UNARY) { // the one-operand form: replaces the top of the stack, or pushes
            I.op = EX_OP_UNARY + x.op;
            I.b_src = EX_NONE;
            if (!fits) return false;
            depth += 1 - int(I.a_src == EX_STACK);
            if (depth > EX_MAX_DEPTH) return false;
            continue;
        }
        I.op = x.op;
        operand(x.right, &I.b_src, &I.lit_b);
        if (!fits) return false;
        if (I.b_src == EX_LIT) I.aux = make_aux(x.op, I.dt, I.lit_b);
        depth += 1 - int(I.a_src == EX_STACK) - int(I.b_src == EX_STACK);
        if (depth > EX_MAX_DEPTH) return false;
    }
    slots.store(P);
    return true;
}

// does the program hold a sin / cos step (the TRIG instances of the interpreting kernels)?
bool program_has_trig(const ExProgram &P) {
    for (int i = 0; i < P.n; ++i)
        if (P.ins[i].op > EX_OP_UNARY + NQE_UNARY_ABS) return true;
    return false;
}

// What a caller asks of a tree before it takes its program
enum ProgramReq : unsigned {
    REQ_BINARY_ROOT = 1, // the root is a BINARY node (a unary root or a bare column / literal is not this consumer's)
    REQ_BOOLEAN = 2,     // the tree is a predicate
    REQ_NOT_BOOLEAN = 4, // the tree yields words
    REQ_NO_NULLS = 8,    // no nullable column and no NULL literal
};
struct ExprProgram {
    std::vector<Node> tree;
    int root = -1;
    ExProgram P;
    bool needs_valid = false; // some column carries validity or some literal is NULL
    const Node &top() const { return tree[size_t(root)]; }
};
// Parses and type-checks `nodes` (raising what parse raises: e->tree and e->root are set whenever it returns) and builds the tree's
// program; false: the root is no operator node, `req` is not met, or the tree does not fit the machine.
bool program_of(const ExprView &in, const nqe_expr_node *nodes, int n, unsigned req, ExprProgram *e) {
    e->tree = parse(in, nodes, n, &e->root);
    const Node &rt = e->top();
    if (!is_op_node(rt.kind) || ((req & REQ_BINARY_ROOT) && rt.kind != NQE_EXPR_BINARY)) return false;
    if (((req & REQ_BOOLEAN) && rt.out_dtype != NQE_BOOLEAN) || ((req & REQ_NOT_BOOLEAN) && rt.out_dtype == NQE_BOOLEAN)) return false;
    return build_program(in, e->tree, e->root, &e->P, &e->needs_valid) && !((req & REQ_NO_NULLS) && e->needs_valid);
}

// `x op lit` (x Int64/UInt64) → range test. Returns false if the shape is not covered.
bool make_fast_pred(const SimpleExpr &pe, FastPred *fp) {
    if (pe.nops != 1 || pe.op[0] > NQE_OP_GT_EQ) return false;
    if (pe.src_dtype != NQE_INT64 && pe.src_dtype != NQE_UINT64 && pe.src_dtype != NQE_FLOAT64) return false;
    static const int flip_op[6] = {NQE_OP_EQ, NQE_OP_NOT_EQ, NQE_OP_GT, NQE_OP_GT_EQ, NQE_OP_LT, NQE_OP_LT_EQ};
    int op = pe.lit_left[0] ? flip_op[pe.op[0]] : pe.op[0]; // lit op x  ≡  x op' lit
    const int64_t MIN = INT64_MIN, MAX = INT64_MAX;
    fp->negate = 0;
    fp->pad = 0;
    fp->row_shift = 0;
    fp->bit_mask = 0;
    fp->val_mask = ~0ull;
    fp->fmask = 0;
    if (pe.src_dtype == NQE_FLOAT64) {
        // IEEE compares as an integer range over the order-preserving image ord(x) = x ^ ((x >> 63) & 0x7fff…f) (signed):
        // every NaN maps beyond ord(±inf), so a range inside [ord(-inf), ord(+inf)] is false for NaN, and the negated
        // range (!=) is true for NaN — exactly arrow's lt/gt/eq/neq on Float64.  ±0 compare equal: the bound uses
        // whichever zero makes the range include / exclude both.
        fp->flip = 0;
        fp->fmask = 0x7fffffffffffffffull;
        auto ord = [](double d) {
            uint64_t b;
            std::memcpy(&b, &d, 8);
            return int64_t(b ^ (uint64_t(int64_t(b) >> 63) & 0x7fffffffffffffffull));
        };
        double c;
        std::memcpy(&c, &pe.lit[0], 8);
        const int64_t NINF = ord(-HUGE_VAL), PINF = ord(HUGE_VAL);
        if (c != c) { // NaN literal: every compare is false, != is true
            fp->lo = 1; fp->hi = 0;
            fp->negate = op == NQE_OP_NOT_EQ ? 1 : 0;
            return true;
        }
        const int64_t c_lo = ord(c == 0.0 ? -0.0 : c), c_hi = ord(c == 0.0 ? 0.0 : c); // image of {x : x == c}
        switch (op) {
        case NQE_OP_EQ: fp->lo = c_lo; fp->hi = c_hi; break;
        case NQE_OP_NOT_EQ: fp->lo = c_lo; fp->hi = c_hi; fp->negate = 1; break;
        case NQE_OP_LT: fp->lo = NINF; fp->hi = c_lo - 1; break;   // c = -inf: empty (hi < lo)
        case NQE_OP_LT_EQ: fp->lo = NINF; fp->hi = c_hi; break;
        case NQE_OP_GT: fp->lo = c_hi + 1; fp->hi = PINF; break;   // c = +inf: empty
        default: fp->lo = c_lo; fp->hi = PINF; break;
        }
        return true;
    }
    fp->flip = pe.src_dtype == NQE_UINT64 ? 0x8000000000000000ull : 0ull;
    const int64_t L = int64_t(pe.lit[0] ^ fp->flip);
    switch (op) {
    case NQE_OP_EQ: fp->lo = L; fp->hi = L; break;
    case NQE_OP_NOT_EQ: fp->lo = L; fp->hi = L; fp->negate = 1; break;
    case NQE_OP_LT: if (L == MIN) { fp->lo = 1; fp->hi = 0; } else { fp->lo = MIN; fp->hi = L - 1; } break; // (x < MIN: empty)
    case NQE_OP_LT_EQ: fp->lo = MIN; fp->hi = L; break;
    case NQE_OP_GT: if (L == MAX) { fp->lo = 1; fp->hi = 0; } else { fp->lo = L + 1; fp->hi = MAX; } break;
    default: fp->lo = L; fp->hi = MAX; break;
    }
    return true;
}

FastPred bitmap_fast_pred() {
    FastPred fp{};
    fp.lo = fp.hi = 1;
    fp.row_shift = 6;
    fp.bit_mask = 63;
    fp.val_mask = 1;
    fp.fmask = 0;
    return fp;
}


ExprInfo analyze_expr(const ExprView &in, const nqe_expr_node *nodes, int n) {
    int root;
    std::vector<Node> t = parse(in, nodes, n, &root);
    ExprInfo info;
    info.out_dtype = t[size_t(root)].out_dtype;
    info.simple = match_simple(t, root, &info.s);
    for (const Node &x : t) {
        if (x.kind != NQE_EXPR_BINARY || (x.op != NQE_OP_DIVIDE && x.op != NQE_OP_MODULOS)) continue;
        const Node &r = t[size_t(x.right)];
        const bool safe_literal = r.kind == NQE_EXPR_LITERAL && !r.lit_null &&
                                  (r.dtype == NQE_FLOAT64 ? r.lit != 0 && r.lit != 0x8000000000000000ull : r.lit != 0 && r.lit != ~0ull);
        if (!safe_literal) info.may_fault = true;
    }
    return info;
}

// Any nesting of `and` / `or` over ONE to CONJ_MAX tests, a test being `col cmp lit` (either side) or `(col arith lit) cmp lit` with a
// fault-free arithmetic step (`id % 3 = 0`, `v * 2.0 > 100.0`, `100 - w >= 7`), over non-null Int64/UInt64/Float64 columns (cols[]
// names the tested column of every test; which loaded word of a row serves a test — ConjTest::src — is the consumer's business).
// A pure and-list / or-list of plain range tests keeps the straight-line form (general = 0); everything else is evaluated through
// the truth table of the and/or structure.  Nodes are in postfix order.
bool match_conj(const ExprView &in, const nqe_expr_node *nodes, int n, ConjPred *out, int *cols) {
    constexpr int MAXN = 8 * CONJ_MAX;
    if (n < 3 || n > MAXN || nodes[n - 1].kind != NQE_EXPR_BINARY) return false;
    // first node of the subtree that ends at node i
    int start[MAXN], stack[MAXN], sp = 0;
    for (int i = 0; i < n; ++i) {
        if (nodes[i].kind == NQE_EXPR_UNARY || is_node_at_a_time(nodes[i].kind)) return false; // (a test is `col [arith lit] cmp lit`: no one-operand step; such trees go through expr_tree_kernel, or node at a time)
        if (nodes[i].kind == NQE_EXPR_BINARY) {
            if (sp < 2) return false;
            sp -= 2;
            start[i] = stack[sp];
        } else
            start[i] = i;
        stack[sp++] = start[i];
    }
    if (sp != 1) return false;
    std::memset(out, 0, sizeof(*out));
    // leaves = maximal subtrees that are not and/or nodes, left to right
    int leaf_of[MAXN]; // node -> leaf number when the node is a leaf's root
    int leaves[CONJ_MAX], nl = 0;
    bool plain_list = true;
    const int root_op = nodes[n - 1].op;
    {
        int todo[MAXN], nt = 0;
        todo[nt++] = n - 1;
        int rev[CONJ_MAX], nr = 0;
        while (nt) {
            const int i = todo[--nt];
            if (nodes[i].kind == NQE_EXPR_BINARY && (nodes[i].op == NQE_OP_AND || nodes[i].op == NQE_OP_OR)) {
                if (nodes[i].op != root_op) plain_list = false;
                todo[nt++] = start[i - 1] - 1; // left operand's root (examined after the right one: leaves come out right to left)
                todo[nt++] = i - 1;
            } else {
                if (nr == CONJ_MAX) return false;
                rev[nr++] = i;
            }
        }
        for (int k = 0; k < nr; ++k) leaves[nl++] = rev[nr - 1 - k];
    }
    if (nl < 1) return false;
    if (root_op != NQE_OP_AND && root_op != NQE_OP_OR) plain_list = false; // a single test (with an arithmetic step, or it would be a SimpleExpr)
    bool any_pre = false;
    for (int t = 0; t < nl; ++t) {
        const int i = leaves[t];
        leaf_of[i] = t;
        const nqe_expr_node *leaf = nodes + start[i];
        const int len = i - start[i] + 1;
        if (len != 3 && len != 5) return false;
        ExprInfo li;
        try {
            li = analyze_expr(in, leaf, len);
        } catch (...) {
            return false; // whatever the leaf's problem is, the tree as a whole reports it
        }
        if (!li.simple || li.out_dtype != NQE_BOOLEAN || li.may_fault) return false;
        const ExprView::Col &c = in.cols[size_t(li.s.col)];
        if (!is_word_type(c.dtype) || c.valid || !c.has_values) return false;
        ConjTest &T = out->t[t];
        SimpleExpr cmp = li.s; // the comparison alone, over the type it compares
        if (li.s.nops == 2) {
            const int op = li.s.op[0], dt = li.s.op_dtype[0];
            if (op < NQE_OP_PLUS || op > NQE_OP_MODULOS) return false;
            if (dt == NQE_FLOAT64 && op == NQE_OP_MODULOS) return false;
            if ((op == NQE_OP_DIVIDE || op == NQE_OP_MODULOS) && li.s.lit_left[0]) return false; // (analyze_expr: may_fault — kept explicit)
            T.pre = op;
            T.pre_dt = dt;
            T.pre_rev = li.s.lit_left[0];
            T.pre_lit = li.s.lit[0];
            T.pre_aux = li.s.aux[0];
            any_pre = true;
            cmp.nops = 1;
            cmp.op[0] = li.s.op[1];
            cmp.lit_left[0] = li.s.lit_left[1];
            cmp.op_dtype[0] = li.s.op_dtype[1];
            cmp.lit[0] = li.s.lit[1];
            cmp.src_dtype = li.s.op_dtype[1];
        } else if (li.s.nops != 1)
            return false;
        FastPred fp{};
        if (!plan::make_fast_pred(cmp, &fp)) return false; // (qualified: nqe_internal.hpp declares the forward of the same name)
        cols[t] = li.s.col;
        T.lo = fp.lo;
        T.hi = fp.hi;
        T.flip = fp.flip;
        T.fmask = fp.fmask;
        T.negate = fp.negate;
    }
    out->n = nl;
    if (plain_list && !any_pre && nl >= 2) {
        out->is_or = root_op == NQE_OP_OR ? 1 : 0;
        return true;
    }
    if (nl == 1 && !any_pre) return false; // a bare compare: the SimpleExpr paths are leaner
    // truth table: evaluate the and/or structure for every assignment of the tests
    out->general = 1;
    for (uint32_t asg = 0; asg < (1u << nl); ++asg) {
        bool val[MAXN];
        int vs = 0;
        // postfix walk over the and/or skeleton: a leaf's subtree contributes its assigned value at its root
        for (int i = 0; i < n; ++i) {
            bool is_leaf_root = false;
            for (int t = 0; t < nl; ++t) is_leaf_root = is_leaf_root || leaves[t] == i;
            if (is_leaf_root) {
                val[vs++] = (asg >> leaf_of[i]) & 1u;
                continue;
            }
            bool inside = false; // a node strictly inside some leaf's subtree
            for (int t = 0; t < nl; ++t) inside = inside || (i >= start[leaves[t]] && i < leaves[t]);
            if (inside) continue;
            // an and/or node of the skeleton
            const bool rv = val[--vs], lv = val[--vs];
            val[vs++] = nodes[i].op == NQE_OP_AND ? (lv && rv) : (lv || rv);
        }
        if (val[0]) out->truth |= 1u << asg;
    }
    return true;
}

bool match_tree_pred(const ExprView &in, const nqe_expr_node *nodes, int n, TreePred *out) {
    std::memset(out, 0, sizeof(*out));
    ExprProgram e;
    try {
        if (!program_of(in, nodes, n, REQ_BINARY_ROOT | REQ_BOOLEAN | REQ_NO_NULLS, &e)) return false;
    } catch (...) {
        return false; // the operator's own analysis reports the problem
    }
    const ExProgram &P = e.P;
    if (P.n > TREE_MAX_INSTR || P.ncols > TREE_MAX_COLS) return false;
    // typed stacks (see tree_pred_eval): one VALUE register, three BOOLEAN levels; normal forms x ∈ {stack, word}, y ∈ {literal,
    // stack, word}, lit_a = 1: the operands are swapped back before the operation
    int vdepth = 0, bdepth = 0;
    for (int i = 0; i < P.n; ++i) {
        const ExInstr &I = P.ins[i];
        if (I.a_src == EX_LIT_NULL || I.b_src == EX_LIT_NULL) return false;
        if (I.op >= EX_OP_UNARY) return false; // (TreeInstr has no one-operand form: the predicate goes through expr_tree_kernel)
        TreeInstr &T = out->ins[i];
        T.op = I.op;
        T.dt = I.dt;
        T.lit_a = 0;
        T.lit_b = 0;
        T.aux = I.aux;
        auto src = [](int s) { return s >= EX_COL ? int(TS_W0) + (s - EX_COL) : (s == EX_LIT ? int(TS_LIT) : int(TS_STACK)); };
        if (I.op == NQE_OP_AND || I.op == NQE_OP_OR) {
            if (I.a_src != EX_STACK || I.b_src != EX_STACK) return false; // a Boolean literal or column as an operand: not this machine's
            if (bdepth < 2) return false;
            --bdepth;
            T.a_src = T.b_src = TS_STACK;
            continue;
        }
        if (I.dt == NQE_BOOLEAN) return false; // comparing Booleans
        if (I.a_src == EX_LIT && I.b_src == EX_LIT) return false;
        int xs = src(I.a_src), ys = src(I.b_src);
        uint64_t lit = I.lit_b;
        bool rev = false;
        if (xs == TS_LIT) { // literal on the left: swap, and remember it for the operators that are not commutative
            xs = ys;
            ys = TS_LIT;
            lit = I.lit_a;
            rev = I.op != NQE_OP_PLUS && I.op != NQE_OP_MULTIPLY && I.op != NQE_OP_EQ && I.op != NQE_OP_NOT_EQ;
            T.aux.pow2_shift = T.aux.more = -1;
        }
        if (I.op == NQE_OP_DIVIDE || I.op == NQE_OP_MODULOS) {
            // no fault may be possible: the kernel has no flag path for the predicate
            if (ys != TS_LIT || rev) return false;
            if (I.dt == NQE_FLOAT64 ? (lit == 0 || lit == 0x8000000000000000ull) : (lit == 0 || lit == ~0ull)) return false;
        }
        const int pops = int(xs == TS_STACK) + int(ys == TS_STACK);
        if (pops > vdepth) return false;
        vdepth -= pops;
        if (I.op <= NQE_OP_GT_EQ) {
            if (++bdepth > 3) return false;
        } else if (++vdepth > 1)
            return false; // two arithmetic subtrees alive at once
        T.a_src = xs;
        T.b_src = ys;
        T.lit_a = rev ? 1 : 0;
        T.lit_b = lit;
    }
    if (vdepth != 0 || bdepth != 1) return false;
    for (int c = 0; c < P.ncols; ++c) {
        if (!is_word_type(P.col_dtype[c])) return false;
        out->col[c] = -1;
        for (size_t k = 0; k < in.cols.size(); ++k)
            if (in.cols[k].has_values && in.cols[k].values == P.col_values[c] && in.cols[k].dtype == P.col_dtype[c] && !in.cols[k].valid) out->col[c] = int(k);
        if (out->col[c] < 0) return false;
    }
    out->n = P.n;
    out->ncols = P.ncols;
    return true;
}

} // namespace plan
} // namespace
} // namespace nqe
