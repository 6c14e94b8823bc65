// expr_shapes.hpp — what the consumers of expressions are handed: the shapes expr_plan.hpp recognises in a tree, as plain structs that
// the consuming kernels (selection, aggregation) take BY VALUE — their layouts are part of those kernels' argument lists.
// Plain C++17, no HIP; nqe_internal.hpp includes it, so every unit sees these declarations.
#pragma once

#include <cstdint>

#include "../../include/nqe.h"

namespace nqe {

inline bool is_word_type(int dt) { return dt == NQE_INT64 || dt == NQE_UINT64 || dt == NQE_FLOAT64; }

struct OpAux {          // host-precomputed helpers for `x / lit`, `x % lit`
    int32_t pow2_shift; // >= 0: |lit| is 2^shift
    int32_t more;       // >= 0: |lit| is not a power of two: q = (((n - mulhi(magic,n)) >> 1) + mulhi(magic,n)) >> more
    uint64_t abs_lit;
    uint64_t magic;
};

// col [op lit]{0,4}: the expression shapes fused into the consumer kernels (literal on either side of every step)
constexpr int SIMPLE_MAX_OPS = 4;
struct SimpleExpr {
    int32_t col;       // index into the INPUT table
    int32_t src_dtype; // dtype of the column
    int32_t out_dtype;
    int32_t nops;
    int32_t op[SIMPLE_MAX_OPS];
    int32_t lit_left[SIMPLE_MAX_OPS]; // 1: lit op v
    int32_t op_dtype[SIMPLE_MAX_OPS]; // operand dtype of step k
    uint64_t lit[SIMPLE_MAX_OPS];
    OpAux aux[SIMPLE_MAX_OPS];
};

// `x op lit` over an Int64/UInt64 column rewritten as  lo <= (x ^ flip) <= hi  (xor negate)
struct FastPred {
    int64_t lo, hi;
    uint64_t flip;
    int32_t negate;
    // where the tested word of row r comes from: word column → src[r]; Boolean bitmap → (src[r >> 6] >> (r & 63)) & 1
    int32_t row_shift; // 0 | 6
    int32_t bit_mask;  // 0 | 63
    int32_t pad;
    uint64_t val_mask; // ~0 | 1
    // Float64 operands: x ^= (x >> 63 arithmetic) & fmask with fmask = 0x7fff…f maps IEEE doubles to signed integers in
    // the same order (negative values reversed); NaNs land beyond ±inf and are excluded by [lo, hi].  0 for integers.
    uint64_t fmask;
};
// `A and B [and C [and D]]` / the same with `or`: up to four range tests `col cmp lit` over non-null 8-byte columns — a WHERE
// clause's usual shape — tested per row inside the consuming kernel (the aggregate's streaming kernel when the columns are its key
// column, its first value column and at most one more; the selection's keep-mask kernel over up to four columns) instead of
// through a materialised Boolean column (one more pass over the predicate's columns)
constexpr int CONJ_MAX = 4;
struct ConjTest {
    int64_t lo, hi;
    uint64_t flip;  // sign bit for UInt64 operands
    uint64_t fmask; // Float64 operands: order map (see FastPred::fmask), 0 for integers
    int32_t negate;
    int32_t src;    // which loaded word of the row (aggregate: 0 key column, 1 first value column, 2 the predicate column;
                    // selection: the column's slot among the distinct tested columns)
    // one fault-free arithmetic step on the word ahead of the range test — `id % 3 = 0`, `v * 2.0 > 100.0`, `100 - w >= 7`:
    // pre = 0: none; else the nqe_operator (PLUS … MODULOS) over operands of type pre_dt, the literal on the right unless pre_rev
    int32_t pre, pre_dt, pre_rev, pad;
    uint64_t pre_lit;
    OpAux pre_aux;
};
struct ConjPred {
    ConjTest t[CONJ_MAX];
    int32_t n;       // tests
    int32_t is_or;   // (lists only)
    int32_t need_pw; // aggregate: some test reads the predicate column (src == 2)
    // general = 0: an and-list / or-list of plain range tests (the straight-line form).  general = 1: ANY nesting of and / or over
    // the tests, some of them with an arithmetic step: the tests' outcomes index the truth table (bit i of `truth`: the predicate's
    // value when test k's outcome is bit k of i)
    int32_t general;
    uint32_t truth;
    int32_t pad;
};
// Any other fault-free predicate tree over at most three non-null 8-byte columns (`v < 20 or id % 3 = 0`, `a + b > c`, …): a
// register stack machine runs it per row INSIDE the consuming kernel (the aggregate's streaming kernel: the tested columns are
// its key column, its first value column and at most one more) instead of a pass that materialises a Boolean column.  One
// instruction per BINARY node, post-order; operands: the stack (depth <= 2), a literal, or one of the row's loaded words.
constexpr int TREE_MAX_INSTR = 12, TREE_MAX_COLS = 3;
enum TreeSrc : int32_t { TS_STACK = 0, TS_LIT = 1, TS_W0 = 4 /* + word slot */ };
struct TreeInstr {
    int32_t op, dt;       // operator, operand dtype
    int32_t a_src, b_src; // TreeSrc
    uint64_t lit_a, lit_b;
    OpAux aux;            // host-prepared divisor constants when b is a literal
};
struct TreePred {
    int32_t n, ncols;
    TreeInstr ins[TREE_MAX_INSTR];
    int32_t col[TREE_MAX_COLS]; // table column behind word slot k of the program as built (the consumer renumbers the slots)
};

struct ExprInfo {
    int out_dtype = NQE_NULLTYPE;
    bool simple = false;
    SimpleExpr s{};
    // true when evaluating it can raise a device error flag (a divide/modulus whose divisor is not a literal other than
    // 0 and -1): only then does an operator need the flag read-back, which is a stream synchronisation
    bool may_fault = false;
};

} // namespace nqe
