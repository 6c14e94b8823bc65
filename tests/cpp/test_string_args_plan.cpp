// NQE_EXPR_STRING_ARGS (quirk Q26) through the host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp) on the CPU: the
// node's arity, every error in the order include/nqe.h states — one case for each precedence —, the typing of its result under compares
// and character_length, nesting, and that no tree that holds the node reaches the stack machine or a fused shape.  Includes that header
// alone.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_string_args_plan.cpp && ./a.out
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
static E u64(uint64_t v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_UINT64; n.value.u64 = v; return {n}; }
static E f64(double v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_FLOAT64; n.value.f64 = v; return {n}; }
static E utf8(const char *s) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_UTF8; n.value.utf8 = s; n.utf8_length = int32_t(std::strlen(s)); return {n}; }
static E null_of(int dt) { N n = node(NQE_EXPR_LITERAL); n.dtype = dt; n.is_null = 1; return {n}; }
static E bin(E l, int op, const E &r) { l.insert(l.end(), r.begin(), r.end()); N n = node(NQE_EXPR_BINARY); n.op = op; l.push_back(n); return l; }
static E str(int f, E e) { N n = node(NQE_EXPR_STRING); n.op = f; e.push_back(n); return e; }
// a STRING_ARGS node over the operands given, whatever their number
static E args(int f, std::vector<E> operands) {
    E e;
    for (const E &o : operands) e.insert(e.end(), o.begin(), o.end());
    N n = node(NQE_EXPR_STRING_ARGS);
    n.op = f;
    e.push_back(n);
    return e;
}
static E substr(const E &s, const E &a, const E &b) { return args(NQE_UNARY_SUBSTR, {s, a, b}); }
static E repeat(const E &s, const E &a) { return args(NQE_UNARY_REPEAT, {s, a}); }
static E replace(const E &s, const E &a, const E &b) { return args(NQE_UNARY_REPLACE, {s, a, b}); }

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

static void test_arity_and_children() {
    CHECK(NQE_EXPR_STRING_ARGS == 5);
    int root;
    E e = substr(col(S), i64(1), i64(2));
    std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 3 && t[3].left == 0 && t[3].right == 1 && t[3].third == 2 && t[3].out_dtype == NQE_UTF8); // the string deepest, the last argument on top
    e = replace(col(S), utf8("a"), utf8("bc"));
    t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 3 && t[3].left == 0 && t[t[3].right].lit_str == "a" && t[t[3].third].lit_str == "bc");
    e = repeat(col(S), col(ID));
    t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 2 && t[2].left == 0 && t[2].right == 1 && t[2].third == -1);
    // REPEAT pops two — the two on top: `s 1 2 REPEAT` repeats the Int64 `1`; with a string there a value stays behind and the tree is
    // malformed as any tree with two roots
    CHECK(parse_error(args(NQE_UNARY_REPEAT, {col(S), i64(1), i64(2)})) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(args(NQE_UNARY_REPEAT, {col(ID), col(S), i64(2)})) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error(args(NQE_UNARY_SUBSTR, {col(ID), col(S), i64(1), i64(2)})) == NQE_ERR_INVALID_ARGUMENT);
    // arguments of any Int64 form: a column, a literal, a NULL Int64 literal, a subtree
    const E len = str(NQE_UNARY_CHARACTER_LENGTH, col(S));
    for (const E &a : {col(ID), i64(-7), null_of(NQE_INT64), bin(len, NQE_OP_MINUS, i64(1)), bin(col(ID), NQE_OP_MODULOS, i64(3))}) {
        CHECK(parse_error(substr(col(S), a, i64(2))) == NQE_OK);
        CHECK(parse_error(substr(col(S), i64(1), a)) == NQE_OK);
        CHECK(parse_error(repeat(col(S), a)) == NQE_OK);
    }
    // `s` of any Utf8 form
    for (const E &s : {col(S), utf8("abc"), null_of(NQE_UTF8), str(NQE_UNARY_TRIM, col(S)), replace(col(S), utf8(" "), utf8("")), substr(col(S), i64(2), i64(INT64_MAX))}) {
        CHECK(dtype_of(substr(s, i64(1), i64(2))) == NQE_UTF8);
        CHECK(dtype_of(repeat(s, i64(3))) == NQE_UTF8);
        CHECK(dtype_of(replace(s, utf8("a"), null_of(NQE_UTF8))) == NQE_UTF8);
    }
}

static void test_errors_in_their_order() {
    // 1. op outside nqe_unary_operator: before everything, an empty stack included
    for (int op : {14, -1, 1000}) {
        CHECK(parse_error(args(op, {})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(ID), col(ID), col(ID)})) == NQE_ERR_INVALID_ARGUMENT); // (not NotSupported for the Int64 `s`)
    }
    // 2. a function without arguments: InvalidArgument, also with three well-typed operands and with a non-Utf8 `s` (4. would be NotSupported)
    for (int op = NQE_UNARY_ABS; op <= NQE_UNARY_SUBSTR; ++op) {
        if (op == NQE_UNARY_REPEAT || op == NQE_UNARY_REPLACE || op == NQE_UNARY_SUBSTR) continue;
        CHECK(parse_error(args(op, {})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(S)})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(S), i64(1), i64(2)})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(ID), f64(1), f64(2)})) == NQE_ERR_INVALID_ARGUMENT);
    }
    // 3. too few values: InvalidArgument although the one value there is no Utf8 (4.) and the arguments would be ill-typed (5., 6.)
    for (int op : {int(NQE_UNARY_SUBSTR), int(NQE_UNARY_REPLACE)}) {
        CHECK(parse_error(args(op, {})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(ID)})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(ID), f64(1)})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(args(op, {col(S), i64(1)})) == NQE_ERR_INVALID_ARGUMENT);
    }
    CHECK(parse_error(args(NQE_UNARY_REPEAT, {})) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error(args(NQE_UNARY_REPEAT, {col(ID)})) == NQE_ERR_INVALID_ARGUMENT);
    // 4. `s` not Utf8 (the status is 5.'s and 6.'s: only the order against 3. above shows)
    for (int c : {ID, V, B, U}) {
        CHECK(parse_error(substr(col(c), i64(1), i64(2))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(repeat(col(c), i64(1))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(replace(col(c), utf8("a"), utf8("b"))) == NQE_ERR_NOT_SUPPORTED);
    }
    CHECK(parse_error(substr(null_of(NQE_NULLTYPE), i64(1), i64(2))) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(repeat(str(NQE_UNARY_CHARACTER_LENGTH, col(S)), i64(2))) == NQE_ERR_NOT_SUPPORTED); // repeat(an Int64)
    // 5. a SUBSTR or REPEAT argument that is not Int64, in either place
    for (const E &bad : {col(U), col(V), col(B), col(S), u64(1), f64(1.0), utf8("1"), null_of(NQE_NULLTYPE), null_of(NQE_UINT64), null_of(NQE_UTF8),
                         bin(col(ID), NQE_OP_LT, i64(3)), str(NQE_UNARY_TRIM, col(S))}) {
        CHECK(parse_error(substr(col(S), bad, i64(2))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(substr(col(S), i64(1), bad)) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(repeat(col(S), bad)) == NQE_ERR_NOT_SUPPORTED);
    }
    // 6. a REPLACE argument that is not a Utf8 literal: a Utf8 column, a Utf8-valued node, literals of other types
    for (const E &bad : {col(S), str(NQE_UNARY_TRIM, col(S)), str(NQE_UNARY_LOWER, utf8("a")), i64(1), null_of(NQE_INT64), null_of(NQE_NULLTYPE), col(ID)}) {
        CHECK(parse_error(replace(col(S), bad, utf8("b"))) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(replace(col(S), utf8("a"), bad)) == NQE_ERR_NOT_SUPPORTED);
    }
    CHECK(parse_error(replace(col(S), utf8(""), utf8(""))) == NQE_OK);
    CHECK(parse_error(replace(col(S), null_of(NQE_UTF8), null_of(NQE_UTF8))) == NQE_OK);
    // an error below the node is raised where it is met, before the node's own
    CHECK(parse_error(substr(col(S), bin(col(ID), NQE_OP_PLUS, col(U)), f64(1))) == NQE_ERR_INTERVAL);
    // what was there stays: the STRING node refuses the three, a UNARY node over them is the reference's todo!()
    for (int op : {int(NQE_UNARY_REPEAT), int(NQE_UNARY_REPLACE), int(NQE_UNARY_SUBSTR)}) {
        CHECK(parse_error(str(op, col(S))) == NQE_ERR_NOT_SUPPORTED);
        E e = col(S);
        N u = node(NQE_EXPR_UNARY);
        u.op = op;
        e.push_back(u);
        CHECK(parse_error(e) == NQE_ERR_NOT_SUPPORTED);
    }
    CHECK(parse_error({node(5)}) == NQE_ERR_INVALID_ARGUMENT && parse_error({node(6)}) == NQE_ERR_INVALID_ARGUMENT && parse_error({node(7)}) == NQE_ERR_INVALID_ARGUMENT);
}

static void test_results_feed_compares_and_character_length() {
    CHECK(dtype_of(bin(substr(col(S), i64(1), i64(2)), NQE_OP_EQ, utf8("DE"))) == NQE_BOOLEAN);        // where substr(code, 1, 2) = 'DE'
    CHECK(dtype_of(bin(replace(col(S), utf8("-"), utf8(" ")), NQE_OP_LT, repeat(col(S), i64(2)))) == NQE_BOOLEAN);
    CHECK(dtype_of(str(NQE_UNARY_CHARACTER_LENGTH, replace(col(S), utf8(" "), utf8("")))) == NQE_INT64); // group by character_length(replace(s, ' ', ''))
    CHECK(dtype_of(bin(str(NQE_UNARY_CHARACTER_LENGTH, substr(col(S), i64(2), i64(INT64_MAX))), NQE_OP_PLUS, col(ID))) == NQE_INT64);
    CHECK(dtype_of(str(NQE_UNARY_UPPER, substr(col(S), col(ID), col(ID)))) == NQE_UTF8);
    CHECK(parse_error(bin(substr(col(S), i64(1), i64(2)), NQE_OP_EQ, i64(1))) == NQE_ERR_INTERVAL);
    CHECK(parse_error(bin(repeat(col(S), i64(2)), NQE_OP_PLUS, utf8("x"))) == NQE_ERR_NOT_SUPPORTED);   // arithmetic on Utf8, as ever
    // substr(s, character_length(s) - 1, 2): the argument is a subtree with a string step of its own
    CHECK(dtype_of(substr(col(S), bin(str(NQE_UNARY_CHARACTER_LENGTH, col(S)), NQE_OP_MINUS, i64(1)), i64(2))) == NQE_UTF8);
}

static void test_no_tree_with_the_node_reaches_the_word_machines() {
    CHECK(is_op_node(NQE_EXPR_STRING_ARGS) && is_string_node(NQE_EXPR_STRING_ARGS) && is_string_node(NQE_EXPR_STRING) && !is_string_node(NQE_EXPR_UNARY));
    const E len = str(NQE_UNARY_CHARACTER_LENGTH, substr(col(S), i64(1), i64(2)));
    const E trees[] = {
        substr(col(S), i64(1), i64(2)),
        repeat(col(S), col(ID)),
        replace(col(S), utf8("a"), utf8("b")),
        bin(substr(col(S), i64(1), i64(2)), NQE_OP_EQ, utf8("ab")),
        bin(len, NQE_OP_MULTIPLY, i64(2)),
        bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(len, NQE_OP_GT, i64(3))),
        bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_GT, bin(i64(3), NQE_OP_MULTIPLY, len)),
    };
    for (const E &e : trees) {
        CHECK(parse_error(e) == NQE_OK);
        int root;
        const std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
        ExProgram P;
        bool needs_valid = false;
        CHECK(!plan::build_program(view, t, root, &P, &needs_valid));
        CHECK(!plan::analyze_expr(view, e.data(), int(e.size())).simple);
        plan::ExprProgram p;
        CHECK(!plan::program_of(view, e.data(), int(e.size()), 0, &p));
        ConjPred conj;
        int cols[CONJ_MAX];
        CHECK(!plan::match_conj(view, e.data(), int(e.size()), &conj, cols));
        TreePred tp;
        CHECK(!plan::match_tree_pred(view, e.data(), int(e.size()), &tp));
    }
    // the same shape without the node is the machines' as before
    const E plain = bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(col(ID), NQE_OP_GT, i64(3)));
    int root;
    const std::vector<Node> t = plan::parse(view, plain.data(), int(plain.size()), &root);
    ExProgram P;
    bool needs_valid = false;
    CHECK(plan::build_program(view, t, root, &P, &needs_valid));
}

int main() {
    test_arity_and_children();
    test_errors_in_their_order();
    test_results_feed_compares_and_character_length();
    test_no_tree_with_the_node_reaches_the_word_machines();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("string args plan ok\n");
    return 0;
}
