// NQE_EXPR_STRING (quirk Q25) through the host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp) on the CPU: every error
// of the node in the order include/nqe.h states, the result dtypes, nesting, and that no tree with a string step anywhere reaches the
// stack machine or a fused shape — while an unchanged tree still builds.  Includes that header alone.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_string_expr_plan.cpp && ./a.out
#include <cstdio>

#include "expr_plan.hpp"

using namespace nqe;
using N = nqe_expr_node;
using E = std::vector<N>;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            if (++failures <= 40) std::printf("%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

enum { ID, V, S, B, U, NCOLS };
static char buffers[NCOLS][8];
static ExprView make_view() {
    const int dt[NCOLS] = {NQE_INT64, NQE_FLOAT64, NQE_UTF8, NQE_BOOLEAN, NQE_UINT64};
    ExprView v;
    for (int c = 0; c < NCOLS; ++c) v.cols.push_back({dt[c], true, buffers[c], nullptr, 100});
    return v;
}
static const ExprView view = make_view();

static N node(int kind) { N n; std::memset(&n, 0, sizeof(n)); n.kind = kind; return n; }
static E col(int c) { N n = node(NQE_EXPR_COLUMN); n.column = c; return {n}; }
static E i64(int64_t v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_INT64; n.value.i64 = v; return {n}; }
static E utf8(const char *s) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_UTF8; n.value.utf8 = s; n.utf8_length = int32_t(std::strlen(s)); return {n}; }
static E null_of(int dt) { N n = node(NQE_EXPR_LITERAL); n.dtype = dt; n.is_null = 1; return {n}; }
static E bin(E l, int op, const E &r) { l.insert(l.end(), r.begin(), r.end()); N n = node(NQE_EXPR_BINARY); n.op = op; l.push_back(n); return l; }
static E un(int f, E e) { N n = node(NQE_EXPR_UNARY); n.op = f; e.push_back(n); return e; }
static E str(int f, E e) { N n = node(NQE_EXPR_STRING); n.op = f; e.push_back(n); return e; }

static int parse_error(const E &e) {
    int root;
    try {
        plan::parse(view, e.data(), int(e.size()), &root);
    } catch (const Error &err) {
        return err.code;
    }
    return NQE_OK;
}
static int dtype_of(const E &e) {
    int root;
    const std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
    return t[size_t(root)].out_dtype;
}
static bool builds(const E &e) {
    int root;
    const std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
    ExProgram P;
    bool needs_valid = false;
    return plan::build_program(view, t, root, &P, &needs_valid);
}
static bool simple(const E &e) { return plan::analyze_expr(view, e.data(), int(e.size())).simple; }

static const int STRING_FNS[7] = {NQE_UNARY_TRIM, NQE_UNARY_LTRIM, NQE_UNARY_RTRIM, NQE_UNARY_CHARACTER_LENGTH, NQE_UNARY_LOWER, NQE_UNARY_UPPER, NQE_UNARY_REVERSE};

static void test_errors_in_their_order() {
    // nothing on the stack comes first: whatever the op says
    for (int op : {int(NQE_UNARY_TRIM), 99, -1, int(NQE_UNARY_ABS), int(NQE_UNARY_SUBSTR)}) {
        N s = node(NQE_EXPR_STRING);
        s.op = op;
        CHECK(parse_error({s}) == NQE_ERR_INVALID_ARGUMENT);
    }
    // op outside 0..13, whatever the operand's type
    for (int op : {14, -1, 1000})
        for (int c : {S, ID}) CHECK(parse_error(str(op, col(c))) == NQE_ERR_INVALID_ARGUMENT);
    // a math function: InvalidArgument, also over the Float64 it takes under a UNARY node and over a non-Utf8 operand
    for (int op = NQE_UNARY_ABS; op <= NQE_UNARY_TAN; ++op)
        for (int c : {S, V, ID}) CHECK(parse_error(str(op, col(c))) == NQE_ERR_INVALID_ARGUMENT);
    // repeat / replace / substr: NotSupported (before the operand's type is looked at: the status is the same, so only the order above shows)
    for (int op : {int(NQE_UNARY_REPEAT), int(NQE_UNARY_REPLACE), int(NQE_UNARY_SUBSTR)})
        for (int c : {S, ID}) CHECK(parse_error(str(op, col(c))) == NQE_ERR_NOT_SUPPORTED);
    // an operand that is not Utf8
    for (int op : STRING_FNS) {
        for (int c : {ID, V, B, U}) CHECK(parse_error(str(op, col(c))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(str(op, i64(3))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(str(op, null_of(NQE_NULLTYPE))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(str(op, col(S))) == NQE_OK);
        CHECK(parse_error(str(op, utf8("abc"))) == NQE_OK);
        CHECK(parse_error(str(op, null_of(NQE_UTF8))) == NQE_OK);
    }
    // what was there stays: a UNARY node over a string function, unknown kinds
    for (int op = NQE_UNARY_TRIM; op <= NQE_UNARY_SUBSTR; ++op) CHECK(parse_error(un(op, col(S))) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error({node(7)}) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error({node(5)}) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error({node(-1)}) == NQE_ERR_INVALID_ARGUMENT);
}

static void test_dtypes_and_nesting() {
    for (int op : STRING_FNS) CHECK(dtype_of(str(op, col(S))) == (op == NQE_UNARY_CHARACTER_LENGTH ? NQE_INT64 : NQE_UTF8));
    CHECK(dtype_of(str(NQE_UNARY_LOWER, str(NQE_UNARY_TRIM, col(S)))) == NQE_UTF8);                       // lower(trim(s))
    CHECK(dtype_of(str(NQE_UNARY_CHARACTER_LENGTH, str(NQE_UNARY_REVERSE, col(S)))) == NQE_INT64);
    CHECK(parse_error(str(NQE_UNARY_TRIM, str(NQE_UNARY_CHARACTER_LENGTH, col(S)))) == NQE_ERR_NOT_SUPPORTED); // trim(an Int64)
    CHECK(dtype_of(bin(str(NQE_UNARY_LOWER, col(S)), NQE_OP_EQ, utf8("bob"))) == NQE_BOOLEAN);             // a Utf8 result feeds a Utf8 compare
    CHECK(dtype_of(bin(str(NQE_UNARY_LOWER, col(S)), NQE_OP_LT, str(NQE_UNARY_UPPER, col(S)))) == NQE_BOOLEAN);
    CHECK(parse_error(bin(str(NQE_UNARY_LOWER, col(S)), NQE_OP_EQ, i64(1))) == NQE_ERR_INTERVAL);
    CHECK(parse_error(bin(str(NQE_UNARY_LOWER, col(S)), NQE_OP_PLUS, utf8("x"))) == NQE_ERR_NOT_SUPPORTED); // arithmetic on Utf8, as ever
    CHECK(dtype_of(bin(str(NQE_UNARY_CHARACTER_LENGTH, col(S)), NQE_OP_MULTIPLY, i64(2))) == NQE_INT64);    // the length feeds Int64 arithmetic
    CHECK(dtype_of(bin(str(NQE_UNARY_CHARACTER_LENGTH, col(S)), NQE_OP_GT, col(ID))) == NQE_BOOLEAN);       // and compares
    CHECK(parse_error(bin(str(NQE_UNARY_CHARACTER_LENGTH, col(S)), NQE_OP_GT, col(U))) == NQE_ERR_INTERVAL);
    CHECK(parse_error(un(NQE_UNARY_ABS, str(NQE_UNARY_CHARACTER_LENGTH, col(S)))) == NQE_ERR_NOT_SUPPORTED); // abs(an Int64)
}

static void test_no_string_step_reaches_the_word_machines() {
    CHECK(is_op_node(NQE_EXPR_STRING) && is_op_node(NQE_EXPR_UNARY) && is_op_node(NQE_EXPR_BINARY) && !is_op_node(NQE_EXPR_COLUMN) && !is_op_node(NQE_EXPR_LITERAL));
    const E len = str(NQE_UNARY_CHARACTER_LENGTH, col(S));
    const E trees[] = {
        str(NQE_UNARY_TRIM, col(S)),                                                           // a bare root
        len,
        bin(str(NQE_UNARY_LOWER, col(S)), NQE_OP_EQ, utf8("bob")),
        bin(len, NQE_OP_MULTIPLY, i64(2)),                                                     // one word operator above the step
        bin(bin(len, NQE_OP_PLUS, i64(1)), NQE_OP_GT, i64(3)),                                 // character_length(s) + 1 > 3
        bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_GT, bin(i64(3), NQE_OP_MULTIPLY, len)),   // the step deep on the right
        bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(len, NQE_OP_GT, i64(3))),          // beside a fusable test
        bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(col(ID), NQE_OP_GT, len)),
    };
    for (const E &e : trees) {
        CHECK(parse_error(e) == NQE_OK);
        CHECK(!builds(e));
        CHECK(!simple(e));
        plan::ExprProgram p;
        CHECK(!plan::program_of(view, e.data(), int(e.size()), 0, &p));
        ConjPred conj;
        int cols[CONJ_MAX];
        CHECK(!plan::match_conj(view, e.data(), int(e.size()), &conj, cols));
        TreePred tp;
        CHECK(!plan::match_tree_pred(view, e.data(), int(e.size()), &tp));
    }
    // the same shapes without the step are the machines' as before
    CHECK(builds(bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_GT, i64(3))));
    CHECK(simple(bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_GT, i64(3))));
    CHECK(builds(bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(col(ID), NQE_OP_GT, i64(3)))));
    CHECK(builds(un(NQE_UNARY_ABS, bin(col(V), NQE_OP_MINUS, col(V)))));
    {
        const E e = bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(col(ID), NQE_OP_GT, i64(3)));
        ConjPred conj;
        int cols[CONJ_MAX];
        CHECK(plan::match_conj(view, e.data(), int(e.size()), &conj, cols));
    }
}

int main() {
    test_errors_in_their_order();
    test_dtypes_and_nesting();
    test_no_string_step_reaches_the_word_machines();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("string expr plan ok\n");
    return 0;
}
