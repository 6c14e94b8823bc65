// NQE_EXPR_STRING_MATCH (quirk Q27) through the host side (naive_query_engine_amd/csrc/expr_plan.hpp and string_match_plan.hpp) on the
// CPU: the node's errors in the order include/nqe.h states, kind 7 still unknown, the typing of its result, the compiled elements,
// segments and form of about thirty patterns, and that no tree that holds the node reaches the stack machine or a fused shape.
// Includes those two headers alone.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_string_match_plan.cpp && ./a.out
#include <cstdio>

#include "expr_plan.hpp"
#include "string_match_plan.hpp"

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
static E f64(double v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_FLOAT64; n.value.f64 = v; return {n}; }
static E utf8(const std::string &s) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_UTF8; n.value.utf8 = s.data(); n.utf8_length = int32_t(s.size()); return {n}; }
static E null_of(int dt) { N n = node(NQE_EXPR_LITERAL); n.dtype = dt; n.is_null = 1; return {n}; }
static E bin(E l, int op, const E &r) { l.insert(l.end(), r.begin(), r.end()); N n = node(NQE_EXPR_BINARY); n.op = op; l.push_back(n); return l; }
static E str(int f, E e) { N n = node(NQE_EXPR_STRING); n.op = f; e.push_back(n); return e; }
static E substr(const E &s, const E &a, const E &b) {
    E e = s;
    e.insert(e.end(), a.begin(), a.end());
    e.insert(e.end(), b.begin(), b.end());
    N n = node(NQE_EXPR_STRING_ARGS);
    n.op = NQE_UNARY_SUBSTR;
    e.push_back(n);
    return e;
}
// a STRING_MATCH node over the operands given, whatever their number
static E match(int op, std::vector<E> operands) {
    E e;
    for (const E &o : operands) e.insert(e.end(), o.begin(), o.end());
    N n = node(NQE_EXPR_STRING_MATCH);
    n.op = op;
    e.push_back(n);
    return e;
}

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

static void test_node_and_errors_in_their_order() {
    CHECK(NQE_EXPR_STRING_MATCH == 6 && NQE_MATCH_LIKE == 0 && NQE_MATCH_STRPOS == 7 && NQE_MAX_MATCH_PATTERN == 4096);
    int root;
    E e = match(NQE_MATCH_LIKE, {col(S), utf8("a%")});
    std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 2 && t[2].left == 0 && t[2].right == 1 && t[1].lit_str == "a%" && t[2].out_dtype == NQE_BOOLEAN); // the string deepest
    for (int op = NQE_MATCH_LIKE; op <= NQE_MATCH_STRPOS; ++op) {
        CHECK(dtype_of(match(op, {col(S), utf8("ab")})) == (op == NQE_MATCH_STRPOS ? NQE_INT64 : NQE_BOOLEAN));
        CHECK(parse_error(match(op, {col(S), null_of(NQE_UTF8)})) == NQE_OK); // a NULL Utf8 literal is a pattern
    }
    // 1. op outside nqe_match_operator: before the empty stack (2.) and the Int64 `s` (3.)
    for (int op : {8, 13, -1, 1000}) {
        CHECK(parse_error(match(op, {})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(match(op, {col(ID), col(ID), col(ID)})) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error(match(op, {col(ID), i64(1)})) == NQE_ERR_INVALID_ARGUMENT);
    }
    // 2. fewer than two values: before `s` (3.) and the pattern (4.)
    CHECK(parse_error(match(NQE_MATCH_LIKE, {})) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error(match(NQE_MATCH_STRPOS, {col(ID)})) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error(match(NQE_MATCH_CONTAINS, {col(S)})) == NQE_ERR_INVALID_ARGUMENT);
    // 3. `s` not Utf8 — also with a pattern that 4. would refuse
    for (const E &s : {col(ID), col(V), col(B), col(U), i64(3), null_of(NQE_NULLTYPE), str(NQE_UNARY_CHARACTER_LENGTH, col(S))}) {
        CHECK(parse_error(match(NQE_MATCH_LIKE, {s, utf8("a")})) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(match(NQE_MATCH_STRPOS, {s, col(ID)})) == NQE_ERR_NOT_SUPPORTED);
    }
    // 4. a pattern that is not a Utf8 literal: a column, a subtree, another dtype, a Null-typed literal
    for (const E &p : {col(S), str(NQE_UNARY_TRIM, col(S)), str(NQE_UNARY_LOWER, utf8("a")), col(ID), i64(1), null_of(NQE_NULLTYPE), null_of(NQE_INT64)})
        for (int op : {NQE_MATCH_LIKE, NQE_MATCH_NOT_ILIKE, NQE_MATCH_ENDS_WITH, NQE_MATCH_STRPOS}) CHECK(parse_error(match(op, {col(S), p})) == NQE_ERR_NOT_SUPPORTED);
    // 5. more than NQE_MAX_MATCH_PATTERN bytes
    const std::string most(4096, 'a'), more(4097, 'a');
    for (int op : {NQE_MATCH_LIKE, NQE_MATCH_CONTAINS, NQE_MATCH_STRPOS}) {
        CHECK(parse_error(match(op, {col(S), utf8(most)})) == NQE_OK);
        CHECK(parse_error(match(op, {col(S), utf8(more)})) == NQE_ERR_NOT_SUPPORTED);
        CHECK(parse_error(match(op, {col(ID), utf8(more)})) == NQE_ERR_NOT_SUPPORTED); // (3. and 5. give the same code)
    }
    // a third value stays behind: malformed as any tree with two roots
    CHECK(parse_error(match(NQE_MATCH_LIKE, {col(ID), col(S), utf8("a")})) == NQE_ERR_INVALID_ARGUMENT);
    // kind 7 is still unknown
    CHECK(parse_error({node(7)}) == NQE_ERR_INVALID_ARGUMENT);
    E seven = match(NQE_MATCH_LIKE, {col(S), utf8("a")});
    seven.back().kind = 7;
    CHECK(parse_error(seven) == NQE_ERR_INVALID_ARGUMENT);
    // `s` of any Utf8 form; the result feeds and / or, compares and arithmetic by its type
    for (const E &s : {col(S), utf8("abc"), null_of(NQE_UTF8), str(NQE_UNARY_LOWER, col(S)), substr(col(S), i64(1), i64(2))}) CHECK(dtype_of(match(NQE_MATCH_ILIKE, {s, utf8("a_")})) == NQE_BOOLEAN);
    CHECK(dtype_of(bin(match(NQE_MATCH_LIKE, {col(S), utf8("a%")}), NQE_OP_AND, bin(col(V), NQE_OP_GT, f64(0.0)))) == NQE_BOOLEAN); // where s like 'a%' and v > 0
    CHECK(dtype_of(bin(match(NQE_MATCH_STRPOS, {col(S), utf8("-")}), NQE_OP_PLUS, i64(1))) == NQE_INT64);
    CHECK(dtype_of(substr(col(S), bin(match(NQE_MATCH_STRPOS, {col(S), utf8("-")}), NQE_OP_PLUS, i64(1)), i64(INT64_MAX))) == NQE_UTF8);
    CHECK(parse_error(bin(match(NQE_MATCH_LIKE, {col(S), utf8("a")}), NQE_OP_PLUS, i64(1))) == NQE_ERR_INTERVAL);
}

struct Want {
    int op;
    const char *pattern;
    int form;
    const char *elems; // '\1' stands for ONE
    std::vector<uint32_t> seg_lens;
    bool front, back;
};

static void test_compiled_patterns() {
    using namespace strmatch;
    const int L = NQE_MATCH_LIKE, I = NQE_MATCH_ILIKE;
    const Want wants[] = {
        {L, "%", FORM_ALWAYS, "", {}, false, false},
        {L, "%%%", FORM_ALWAYS, "", {}, false, false},
        {L, "", FORM_EQUAL, "", {}, true, true},
        {L, "abc", FORM_EQUAL, "abc", {3}, true, true},
        {L, "ab%", FORM_PREFIX, "ab", {2}, true, false},
        {L, "%ab", FORM_SUFFIX, "ab", {2}, false, true},
        {L, "ab%yz", FORM_PREFIX_SUFFIX, "abyz", {2, 2}, true, true},
        {L, "ab%%yz", FORM_PREFIX_SUFFIX, "abyz", {2, 2}, true, true},
        {L, "%ab%", FORM_CONTAINS, "ab", {2}, false, false},
        {L, "%%ab%%", FORM_CONTAINS, "ab", {2}, false, false},
        {L, "_", FORM_GENERAL, "\1", {1}, true, true},
        {L, "___", FORM_GENERAL, "\1\1\1", {3}, true, true},
        {L, "%_%", FORM_GENERAL, "\1", {1}, false, false},
        {L, "a_c%", FORM_GENERAL, "a\1c", {3}, true, false},
        {L, "%a_", FORM_GENERAL, "a\1", {2}, false, true},
        {L, "a%b%c", FORM_GENERAL, "abc", {1, 1, 1}, true, true},
        {L, "%a%b%c%", FORM_GENERAL, "abc", {1, 1, 1}, false, false},
        {L, "%a%b", FORM_GENERAL, "ab", {1, 1}, false, true},
        {L, "a%b%", FORM_GENERAL, "ab", {1, 1}, true, false},
        {L, "\\%", FORM_EQUAL, "%", {1}, true, true},
        {L, "\\_%", FORM_PREFIX, "_", {1}, true, false},
        {L, "%\\\\", FORM_SUFFIX, "\\", {1}, false, true},
        {L, "\\a\\b", FORM_EQUAL, "ab", {2}, true, true},
        {L, "ab\\", FORM_EQUAL, "ab\\", {3}, true, true},   // a `\` that ends the pattern is a literal
        {L, "\\", FORM_EQUAL, "\\", {1}, true, true},
        {L, "%\\%%", FORM_CONTAINS, "%", {1}, false, false},
        {L, "a\\%%", FORM_PREFIX, "a%", {2}, true, false},
        {L, "AbC%", FORM_PREFIX, "AbC", {3}, true, false},
        {I, "AbC%", FORM_PREFIX, "abc", {3}, true, false}, // ILIKE folds the literal elements
        {I, "%[@Z`{\xc3\x89", FORM_SUFFIX, "[@z`{\xc3\x89", {7}, false, true}, // A-Z only
        {NQE_MATCH_NOT_ILIKE, "_Q%", FORM_GENERAL, "\1q", {2}, true, false},
        {NQE_MATCH_STARTS_WITH, "a%_\\", FORM_PREFIX, "a%_\\", {4}, true, false}, // verbatim: no wildcards, no escape
        {NQE_MATCH_ENDS_WITH, "%b", FORM_SUFFIX, "%b", {2}, false, true},
        {NQE_MATCH_CONTAINS, "_", FORM_CONTAINS, "_", {1}, false, false},
        {NQE_MATCH_STRPOS, "Ab", FORM_CONTAINS, "Ab", {2}, false, false},
        {NQE_MATCH_STARTS_WITH, "", FORM_ALWAYS, "", {}, true, false},
        {NQE_MATCH_CONTAINS, "", FORM_ALWAYS, "", {}, false, false},
    };
    for (const Want &w : wants) {
        const Compiled c = compile(w.op, w.pattern);
        std::string elems = c.elems;
        uint32_t ones = 0, seg_ones = 0, at = 0;
        for (size_t k = 0; k < elems.size(); ++k)
            if (c.ones[k]) { CHECK(elems[k] == 0); elems[k] = '\1'; ++ones; }
        bool ok = c.form == w.form && elems == w.elems && c.ones.size() == c.elems.size() && c.segs.size() == w.seg_lens.size() && c.min_bytes == c.elems.size();
        for (size_t k = 0; ok && k < c.segs.size(); ++k) {
            ok = c.segs[k].off == at && c.segs[k].len == w.seg_lens[k];
            at += c.segs[k].len;
            seg_ones += c.segs[k].ones;
        }
        ok = ok && seg_ones == ones && (c.segs.empty() || (c.anchored_front == w.front && c.anchored_back == w.back));
        ok = ok && c.fold == (w.op == NQE_MATCH_ILIKE || w.op == NQE_MATCH_NOT_ILIKE) && c.negate == (w.op == NQE_MATCH_NOT_LIKE || w.op == NQE_MATCH_NOT_ILIKE);
        if (!ok) std::printf("pattern '%s' (op %d): form %d, %zu segments\n", w.pattern, w.op, c.form, c.segs.size());
        CHECK(ok);
    }
    // the four anchored forms only without ONE
    for (const char *p : {"a_", "_a%", "%_a", "a_%_b"}) CHECK(compile(L, p).form == FORM_GENERAL);
    // 4096 bytes compile (the parser refuses 4097): alternating `%a` gives 2048 one-element segments
    std::string big;
    for (int k = 0; k < 2048; ++k) big += "%a";
    const Compiled c = compile(L, big);
    CHECK(c.form == FORM_GENERAL && c.segs.size() == 2048 && c.min_bytes == 2048 && !c.anchored_front && c.anchored_back);
    CHECK(compile(L, std::string(4096, 'a')).form == FORM_EQUAL && compile(L, std::string(4096, '_')).segs[0].ones == 4096);
}

static void test_no_tree_with_the_node_reaches_the_word_machines() {
    CHECK(is_op_node(NQE_EXPR_STRING_MATCH) && is_string_node(NQE_EXPR_STRING_MATCH) && is_string_node(NQE_EXPR_STRING_ARGS) && is_string_node(NQE_EXPR_STRING) && !is_string_node(7));
    const E like = match(NQE_MATCH_LIKE, {col(S), utf8("ab%")}), pos = match(NQE_MATCH_STRPOS, {col(S), utf8("-")});
    const E trees[] = {
        like,
        pos,
        bin(like, NQE_OP_AND, bin(col(ID), NQE_OP_GT, i64(0))),
        bin(bin(bin(col(ID), NQE_OP_MODULOS, i64(3)), NQE_OP_EQ, i64(0)), NQE_OP_OR, like),
        bin(pos, NQE_OP_GT, i64(0)),
        bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_GT, bin(i64(3), NQE_OP_MULTIPLY, pos)),
        bin(bin(col(ID), NQE_OP_LT, i64(5)), NQE_OP_AND, bin(pos, NQE_OP_GT, i64(3))),
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
    test_node_and_errors_in_their_order();
    test_compiled_patterns();
    test_no_tree_with_the_node_reaches_the_word_machines();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("string match plan ok\n");
    return 0;
}
