// NQE_EXPR_CONDITIONAL (quirk Q28) through the host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp) on the CPU: the
// node's seven errors, each shown to win over the later ones; the typing of every function over every dtype; nesting under and over
// BINARY, STRING, STRING_ARGS and STRING_MATCH nodes; that no tree that holds the node reaches the stack machine or a fused shape; a
// zeroed kind-7 node stays INVALID_ARGUMENT and kind 8 is unknown.  Includes that header alone.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_conditional_plan.cpp && ./a.out
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

enum { ID, V, S, B, U, ID2, V2, S2, B2, U2, NCOLS };
static char buffers[NCOLS][8];
static ExprView make_view() {
    const int dt[NCOLS] = {NQE_INT64, NQE_FLOAT64, NQE_UTF8, NQE_BOOLEAN, NQE_UINT64, NQE_INT64, NQE_FLOAT64, NQE_UTF8, NQE_BOOLEAN, NQE_UINT64};
    ExprView v;
    for (int c = 0; c < NCOLS; ++c) v.cols.push_back({dt[c], true, buffers[c], nullptr, 100});
    return v;
}
static const ExprView view = make_view();

static N node(int kind) { N n; std::memset(&n, 0, sizeof(n)); n.kind = kind; return n; }
static E col(int c) { N n = node(NQE_EXPR_COLUMN); n.column = c; return {n}; }
static E i64(int64_t v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_INT64; n.value.i64 = v; return {n}; }
static E f64(double v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_FLOAT64; n.value.f64 = v; return {n}; }
static E boolean(bool v) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_BOOLEAN; n.value.boolean = v; return {n}; }
static E utf8(const std::string &s) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_UTF8; n.value.utf8 = s.data(); n.utf8_length = int32_t(s.size()); return {n}; }
static E null_of(int dt) { N n = node(NQE_EXPR_LITERAL); n.dtype = dt; n.is_null = 1; return {n}; }
static E join(std::vector<E> parts, N last) {
    E e;
    for (const E &o : parts) e.insert(e.end(), o.begin(), o.end());
    e.push_back(last);
    return e;
}
static E bin(const E &l, int op, const E &r) { N n = node(NQE_EXPR_BINARY); n.op = op; return join({l, r}, n); }
static E unary(int f, const E &e) { N n = node(NQE_EXPR_UNARY); n.op = f; return join({e}, n); }
static E str(int f, const E &e) { N n = node(NQE_EXPR_STRING); n.op = f; return join({e}, n); }
static E substr(const E &s, const E &a, const E &b) { N n = node(NQE_EXPR_STRING_ARGS); n.op = NQE_UNARY_SUBSTR; return join({s, a, b}, n); }
static E like(const E &s, const std::string &p) { N n = node(NQE_EXPR_STRING_MATCH); n.op = NQE_MATCH_LIKE; return join({s, utf8(p)}, n); }
// a CONDITIONAL node over the operands given, whatever their number, with `column` = count (default: the number of operands)
static constexpr int ARITY = -1000;
static E cond(int op, std::vector<E> operands, int count = ARITY) {
    N n = node(NQE_EXPR_CONDITIONAL);
    n.op = op;
    n.column = count == ARITY ? int(operands.size()) : count;
    return join(std::move(operands), n);
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
static bool has_program(const E &e) {
    plan::ExprProgram p;
    return plan::program_of(view, e.data(), int(e.size()), 0, &p);
}

static const int INVALID = NQE_ERR_INVALID_ARGUMENT;

static void test_the_node() {
    CHECK(NQE_EXPR_CONDITIONAL == 7 && NQE_EXPR_STRING_MATCH == 6 && NQE_ABI_VERSION == 1);
    CHECK(NQE_COND_NOT == 0 && NQE_COND_IS_NULL == 1 && NQE_COND_IS_NOT_NULL == 2 && NQE_COND_COALESCE == 3 && NQE_COND_NULLIF == 4 && NQE_COND_IF == 5);
    for (int op = 0; op <= 5; ++op) CHECK(cond_arity(op) == (op <= 2 ? 1 : op == 5 ? 3 : 2));
    CHECK(cond_arity(-1) == 0 && cond_arity(6) == 0);
    CHECK(is_op_node(NQE_EXPR_CONDITIONAL) && is_node_at_a_time(NQE_EXPR_CONDITIONAL) && !is_string_node(NQE_EXPR_CONDITIONAL));
    int root;
    E e = cond(NQE_COND_IF, {col(B), col(ID), i64(0)});
    std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 3 && t[3].left == 0 && t[3].right == 1 && t[3].third == 2 && t[3].out_dtype == NQE_INT64); // the condition deepest, the else value on top
    e = cond(NQE_COND_COALESCE, {col(V), f64(0.0)});
    t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 2 && t[2].left == 0 && t[2].right == 1 && t[2].third == -1 && t[2].out_dtype == NQE_FLOAT64);
    e = cond(NQE_COND_IS_NULL, {col(S)});
    t = plan::parse(view, e.data(), int(e.size()), &root);
    CHECK(root == 1 && t[1].left == 0 && t[1].right == -1 && t[1].out_dtype == NQE_BOOLEAN);
}

static void test_errors_in_their_order() {
    // 1. `column` outside 1..3 — before the unknown op (2.), the empty stack (4.) and everything else; a zeroed kind-7 node is this
    CHECK(parse_error({node(7)}) == INVALID);
    for (int count : {0, -1, 4, 100}) {
        CHECK(parse_error(cond(99, {}, count)) == INVALID);
        CHECK(parse_error(cond(NQE_COND_NOT, {col(B)}, count)) == INVALID);
        CHECK(parse_error(cond(NQE_COND_IF, {col(B), col(ID), col(ID)}, count)) == INVALID);
        CHECK(parse_error(cond(NQE_COND_COALESCE, {null_of(NQE_NULLTYPE), col(ID)}, count)) == INVALID); // not 5.'s NOT_SUPPORTED
        CHECK(parse_error(cond(NQE_COND_NOT, {col(ID)}, count)) == INVALID);                             // not 6.'s INTERVAL
    }
    // 2. `op` outside nqe_cond_operator — before the arity (3.), the stack (4.) and the operands (5.-7.)
    for (int op : {6, 7, 13, -1, 1000})
        for (int count : {1, 2, 3}) {
            CHECK(parse_error(cond(op, {}, count)) == INVALID);
            CHECK(parse_error(cond(op, {null_of(NQE_NULLTYPE), col(ID), col(V)}, count)) == INVALID);
        }
    // 3. `column` differs from the arity — before the stack (4.) and the operands
    for (int op = 0; op <= 5; ++op)
        for (int count : {1, 2, 3}) {
            if (count == cond_arity(op)) continue;
            CHECK(parse_error(cond(op, {}, count)) == INVALID);
            CHECK(parse_error(cond(op, {col(B), col(ID), col(ID)}, count)) == INVALID);
            CHECK(parse_error(cond(op, {null_of(NQE_NULLTYPE), null_of(NQE_NULLTYPE), null_of(NQE_NULLTYPE)}, count)) == INVALID); // not 5.
            CHECK(parse_error(cond(op, {col(ID), col(V), col(S)}, count)) == INVALID);                                            // not 6. / 7.
        }
    // 4. fewer values than the node pops
    CHECK(parse_error(cond(NQE_COND_NOT, {}, 1)) == INVALID);
    CHECK(parse_error(cond(NQE_COND_COALESCE, {col(ID)}, 2)) == INVALID);
    CHECK(parse_error(cond(NQE_COND_NULLIF, {null_of(NQE_NULLTYPE)}, 2)) == INVALID); // not 5.
    CHECK(parse_error(cond(NQE_COND_IF, {col(ID), col(V)}, 3)) == INVALID);            // not 6. / 7.
    CHECK(parse_error(cond(NQE_COND_IF, {}, 3)) == INVALID);
    // 5. an operand of dtype NQE_NULLTYPE — before the non-Boolean condition (6.) and the mismatch (7.)
    CHECK(parse_error(cond(NQE_COND_NOT, {null_of(NQE_NULLTYPE)})) == NQE_ERR_NOT_SUPPORTED); // (6. would say INTERVAL: Null is not Boolean)
    CHECK(parse_error(cond(NQE_COND_IS_NULL, {null_of(NQE_NULLTYPE)})) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(cond(NQE_COND_IS_NOT_NULL, {null_of(NQE_NULLTYPE)})) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(cond(NQE_COND_COALESCE, {col(ID), null_of(NQE_NULLTYPE)})) == NQE_ERR_NOT_SUPPORTED); // (7. would say INTERVAL)
    CHECK(parse_error(cond(NQE_COND_NULLIF, {null_of(NQE_NULLTYPE), col(V)})) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(cond(NQE_COND_IF, {col(ID), null_of(NQE_NULLTYPE), col(V)})) == NQE_ERR_NOT_SUPPORTED); // (6. and 7. would both object)
    CHECK(parse_error(cond(NQE_COND_IF, {null_of(NQE_NULLTYPE), col(ID), col(ID)})) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(cond(NQE_COND_IF, {col(B), col(ID), null_of(NQE_NULLTYPE)})) == NQE_ERR_NOT_SUPPORTED);
    // 6. NOT's operand or IF's c not Boolean — before the mismatch (7.: the same code, so shown by a tree 7. would accept)
    for (const E &c : {col(ID), col(V), col(S), col(U), i64(1), utf8("t"), null_of(NQE_INT64)}) {
        CHECK(parse_error(cond(NQE_COND_NOT, {c})) == NQE_ERR_INTERVAL);
        CHECK(parse_error(cond(NQE_COND_IF, {c, col(ID), col(ID2)})) == NQE_ERR_INTERVAL);
        CHECK(parse_error(cond(NQE_COND_IF, {c, col(ID), col(V)})) == NQE_ERR_INTERVAL);
    }
    // 7. the two value operands differ
    const int dts[5] = {ID, V, S, B, U};
    for (int x : dts)
        for (int y : dts) {
            const int want = x == y ? NQE_OK : NQE_ERR_INTERVAL;
            CHECK(parse_error(cond(NQE_COND_COALESCE, {col(x), col(y)})) == want);
            CHECK(parse_error(cond(NQE_COND_NULLIF, {col(x), col(y)})) == want);
            CHECK(parse_error(cond(NQE_COND_IF, {col(B), col(x), col(y)})) == want);
        }
    CHECK(parse_error(cond(NQE_COND_COALESCE, {col(V), i64(0)})) == NQE_ERR_INTERVAL); // no coercion (Q6)
    CHECK(parse_error(cond(NQE_COND_IF, {col(B), col(S), null_of(NQE_INT64)})) == NQE_ERR_INTERVAL);
    // a value left behind: malformed as any tree with two roots
    CHECK(parse_error(cond(NQE_COND_NOT, {col(ID), col(B)}, 1)) == INVALID);
    // kind 8 is unknown, whatever its fields hold
    CHECK(parse_error({node(8)}) == INVALID);
    E eight = cond(NQE_COND_NOT, {col(B)});
    eight.back().kind = 8;
    CHECK(parse_error(eight) == INVALID);
}

static void test_typing_and_nesting() {
    const int cols[5] = {ID, V, S, B, U}, twins[5] = {ID2, V2, S2, B2, U2}, dts[5] = {NQE_INT64, NQE_FLOAT64, NQE_UTF8, NQE_BOOLEAN, NQE_UINT64};
    for (int k = 0; k < 5; ++k) {
        const E x = col(cols[k]), y = col(twins[k]), nul = null_of(dts[k]);
        CHECK(dtype_of(cond(NQE_COND_IS_NULL, {x})) == NQE_BOOLEAN && dtype_of(cond(NQE_COND_IS_NOT_NULL, {x})) == NQE_BOOLEAN);
        CHECK(dtype_of(cond(NQE_COND_IS_NULL, {nul})) == NQE_BOOLEAN);
        for (int op : {NQE_COND_COALESCE, NQE_COND_NULLIF}) {
            CHECK(dtype_of(cond(op, {x, y})) == dts[k]);
            CHECK(dtype_of(cond(op, {x, nul})) == dts[k] && dtype_of(cond(op, {nul, x})) == dts[k] && dtype_of(cond(op, {nul, nul})) == dts[k]);
        }
        CHECK(dtype_of(cond(NQE_COND_IF, {col(B), x, y})) == dts[k]);
        CHECK(dtype_of(cond(NQE_COND_IF, {boolean(true), x, nul})) == dts[k]);        // CASE without ELSE
        CHECK(dtype_of(cond(NQE_COND_IF, {null_of(NQE_BOOLEAN), nul, x})) == dts[k]); // a NULL Boolean literal is a condition
        // coalesce(a, b, c) = a b c COALESCE COALESCE; CASE WHEN c1 THEN x WHEN c2 THEN y ELSE z END = c1 x c2 y z IF IF
        CHECK(dtype_of(cond(NQE_COND_COALESCE, {x, cond(NQE_COND_COALESCE, {y, nul})})) == dts[k]);
        CHECK(dtype_of(cond(NQE_COND_IF, {col(B), x, cond(NQE_COND_IF, {col(B2), y, nul})})) == dts[k]);
    }
    CHECK(dtype_of(cond(NQE_COND_NOT, {col(B)})) == NQE_BOOLEAN && dtype_of(cond(NQE_COND_NOT, {boolean(false)})) == NQE_BOOLEAN);
    CHECK(dtype_of(cond(NQE_COND_NOT, {cond(NQE_COND_NOT, {col(B)})})) == NQE_BOOLEAN);
    // over BINARY, UNARY, STRING, STRING_ARGS and STRING_MATCH nodes
    const E gt = bin(col(V), NQE_OP_GT, f64(50.0));
    CHECK(dtype_of(cond(NQE_COND_IF, {gt, i64(1), i64(0)})) == NQE_INT64); // case when v > 50 then 1 else 0 end
    CHECK(dtype_of(cond(NQE_COND_NOT, {bin(like(col(S), "x%"), NQE_OP_AND, gt)})) == NQE_BOOLEAN); // where not (s like 'x%' and v > 50)
    CHECK(dtype_of(cond(NQE_COND_COALESCE, {unary(NQE_UNARY_ABS, col(V)), f64(0.0)})) == NQE_FLOAT64);
    CHECK(dtype_of(cond(NQE_COND_COALESCE, {str(NQE_UNARY_LOWER, col(S)), utf8("unknown")})) == NQE_UTF8);
    CHECK(dtype_of(cond(NQE_COND_NULLIF, {substr(col(S), i64(1), i64(3)), utf8("")})) == NQE_UTF8);
    CHECK(dtype_of(cond(NQE_COND_IF, {like(col(S), "a%"), col(S), col(S2)})) == NQE_UTF8);
    CHECK(dtype_of(cond(NQE_COND_IS_NULL, {str(NQE_UNARY_CHARACTER_LENGTH, col(S))})) == NQE_BOOLEAN);
    // under them
    CHECK(dtype_of(bin(cond(NQE_COND_COALESCE, {col(ID), i64(-1)}), NQE_OP_PLUS, i64(1))) == NQE_INT64);
    CHECK(dtype_of(bin(cond(NQE_COND_IS_NULL, {col(ID)}), NQE_OP_OR, cond(NQE_COND_NOT, {col(B)}))) == NQE_BOOLEAN);
    CHECK(dtype_of(unary(NQE_UNARY_SIN, cond(NQE_COND_COALESCE, {col(V), f64(0.0)}))) == NQE_FLOAT64);
    CHECK(dtype_of(str(NQE_UNARY_UPPER, cond(NQE_COND_COALESCE, {col(S), utf8("unknown")}))) == NQE_UTF8);
    CHECK(dtype_of(substr(cond(NQE_COND_IF, {col(B), col(S), col(S2)}), cond(NQE_COND_COALESCE, {col(ID), i64(1)}), i64(2))) == NQE_UTF8);
    CHECK(dtype_of(like(cond(NQE_COND_COALESCE, {col(S), utf8("")}), "a_")) == NQE_BOOLEAN);
    CHECK(parse_error(bin(cond(NQE_COND_IS_NULL, {col(ID)}), NQE_OP_PLUS, i64(1))) == NQE_ERR_INTERVAL); // Boolean + Int64
    CHECK(parse_error(str(NQE_UNARY_LOWER, cond(NQE_COND_COALESCE, {col(ID), i64(1)}))) == NQE_ERR_NOT_SUPPORTED);
}

static void test_no_program_and_no_fused_shape() {
    const E gt = bin(col(V), NQE_OP_GT, f64(50.0));
    const std::vector<E> trees = {
        cond(NQE_COND_NOT, {col(B)}),
        cond(NQE_COND_IS_NULL, {col(ID)}),
        cond(NQE_COND_COALESCE, {col(V), f64(0.0)}),
        cond(NQE_COND_IF, {gt, i64(1), i64(0)}),
        cond(NQE_COND_NOT, {bin(gt, NQE_OP_AND, bin(col(ID), NQE_OP_LT, i64(7)))}),
        bin(cond(NQE_COND_COALESCE, {col(ID), i64(-1)}), NQE_OP_PLUS, i64(1)),
        bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_MULTIPLY, cond(NQE_COND_NULLIF, {col(ID), i64(0)})),
        bin(gt, NQE_OP_AND, cond(NQE_COND_IS_NOT_NULL, {col(V)})),
        bin(gt, NQE_OP_AND, bin(cond(NQE_COND_COALESCE, {col(ID), i64(0)}), NQE_OP_LT, i64(7))),
        unary(NQE_UNARY_ABS, cond(NQE_COND_COALESCE, {col(V), f64(0.0)})),
        bin(unary(NQE_UNARY_ABS, cond(NQE_COND_COALESCE, {col(V), f64(0.0)})), NQE_OP_GT, f64(1.0)),
    };
    for (const E &e : trees) {
        CHECK(parse_error(e) == NQE_OK);
        CHECK(!has_program(e));
        plan::ExprProgram p;
        CHECK(!plan::program_of(view, e.data(), int(e.size()), plan::REQ_BINARY_ROOT | plan::REQ_BOOLEAN | plan::REQ_NO_NULLS, &p));
        const ExprInfo info = plan::analyze_expr(view, e.data(), int(e.size()));
        CHECK(!info.simple);
        ConjPred cp;
        int cols[CONJ_MAX];
        CHECK(!plan::match_conj(view, e.data(), int(e.size()), &cp, cols));
        TreePred tp;
        CHECK(!plan::match_tree_pred(view, e.data(), int(e.size()), &tp));
    }
    CHECK(has_program(bin(gt, NQE_OP_AND, bin(col(ID), NQE_OP_LT, i64(7))))); // the same tree without the node does fit
}

int main() {
    test_the_node();
    test_errors_in_their_order();
    test_typing_and_nesting();
    test_no_program_and_no_fused_shape();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("conditional plan ok\n");
    return 0;
}
