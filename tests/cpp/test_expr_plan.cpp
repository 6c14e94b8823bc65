// The host side of expressions (naive_query_engine_amd/csrc/expr_plan.hpp) on the CPU: the parser's errors, the divisor constants of
// make_aux, the range form of make_fast_pred, and what match_simple / match_conj / build_program / match_tree_pred accept, refuse and
// emit.  Includes that header alone; every expectation is computed here with native C++ arithmetic, never by the code under test.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_expr_plan.cpp && ./a.out
#include <cinttypes>
#include <cstdio>
#include <limits>
#include <random>

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

// ---- the input: what a table shows of itself
enum { ID, V, W, U, B, S, NI, X, Y, F2, Z, NCOLS };
static char buffers[NCOLS][8], ni_valid[8];
static ExprView make_view() {
    const int dt[NCOLS] = {NQE_INT64, NQE_FLOAT64, NQE_INT64, NQE_UINT64, NQE_BOOLEAN, NQE_UTF8, NQE_INT64, NQE_INT64, NQE_INT64, NQE_FLOAT64, NQE_INT64};
    ExprView v;
    for (int c = 0; c < NCOLS; ++c) v.cols.push_back({dt[c], true, buffers[c], c == NI ? reinterpret_cast<const uint8_t *>(ni_valid) : nullptr, 100});
    return v;
}
static const ExprView view = make_view();

// ---- postfix builders
static N node(int kind) { N n; std::memset(&n, 0, sizeof(n)); n.kind = kind; return n; }
static E col(int c) { N n = node(NQE_EXPR_COLUMN); n.column = c; return {n}; }
static E lit_bits(int dt, uint64_t w) { N n = node(NQE_EXPR_LITERAL); n.dtype = dt; n.value.u64 = w; return {n}; }
static E i64(int64_t v) { return lit_bits(NQE_INT64, uint64_t(v)); }
static uint64_t bits_of(double d) { uint64_t w; std::memcpy(&w, &d, 8); return w; }
static double double_of(uint64_t w) { double d; std::memcpy(&d, &w, 8); return d; }
static E f64(double d) { return lit_bits(NQE_FLOAT64, bits_of(d)); }
static E boolean(bool b) { return lit_bits(NQE_BOOLEAN, b ? 1 : 0); }
static E null_of(int dt) { N n = node(NQE_EXPR_LITERAL); n.dtype = dt; n.is_null = 1; return {n}; }
static E utf8(const char *s) { N n = node(NQE_EXPR_LITERAL); n.dtype = NQE_UTF8; n.value.utf8 = s; n.utf8_length = int32_t(std::strlen(s)); return {n}; }
static E bin(E l, int op, const E &r) { l.insert(l.end(), r.begin(), r.end()); N n = node(NQE_EXPR_BINARY); n.op = op; l.push_back(n); return l; }
static E un(int f, E e) { N n = node(NQE_EXPR_UNARY); n.op = f; e.push_back(n); return e; }

static int parse_error(const E &e, const ExprView &in = view) {
    int root;
    try {
        plan::parse(in, e.data(), int(e.size()), &root);
    } catch (const Error &err) {
        return err.code;
    }
    return NQE_OK;
}

// ---------------------------------------------------------------- parse: every error where it is raised
static void test_parse() {
    CHECK(parse_error(bin(col(ID), NQE_OP_PLUS, i64(1))) == NQE_OK);
    CHECK(parse_error(bin(col(ID), NQE_OP_PLUS, col(V))) == NQE_ERR_INTERVAL);           // mismatched operand types
    CHECK(parse_error(bin(col(ID), NQE_OP_LT, f64(1.0))) == NQE_ERR_INTERVAL);
    CHECK(parse_error(bin(col(ID), NQE_OP_AND, col(W))) == NQE_ERR_INTERVAL);            // and / or over non-Boolean
    CHECK(parse_error(bin(col(V), NQE_OP_OR, col(F2))) == NQE_ERR_INTERVAL);
    CHECK(parse_error(bin(col(B), NQE_OP_AND, boolean(true))) == NQE_OK);
    CHECK(parse_error(bin(col(B), NQE_OP_PLUS, col(B))) == NQE_ERR_NOT_SUPPORTED);       // arithmetic over Boolean, Utf8
    CHECK(parse_error(bin(col(S), NQE_OP_MODULOS, utf8("x"))) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(bin(col(S), NQE_OP_EQ, utf8("x"))) == NQE_OK);
    CHECK(parse_error(bin(null_of(NQE_NULLTYPE), NQE_OP_EQ, null_of(NQE_NULLTYPE))) == NQE_ERR_ARROW);
    CHECK(parse_error(un(NQE_UNARY_ABS, col(ID))) == NQE_ERR_NOT_SUPPORTED);             // unary over non-Float64
    CHECK(parse_error(un(NQE_UNARY_SIN, col(B))) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(un(NQE_UNARY_TAN, col(V))) == NQE_OK);
    for (int f = NQE_UNARY_TRIM; f <= NQE_UNARY_SUBSTR; ++f) CHECK(parse_error(un(f, col(V))) == NQE_ERR_NOT_SUPPORTED); // the string functions
    CHECK(parse_error(un(NQE_UNARY_SUBSTR + 1, col(V))) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error(un(-1, col(V))) == NQE_ERR_INVALID_ARGUMENT);
    CHECK(parse_error(col(NCOLS)) == NQE_ERR_NOT_SUPPORTED);                             // a column index out of range
    CHECK(parse_error(col(-1)) == NQE_ERR_NOT_SUPPORTED);
    CHECK(parse_error(bin(col(ID), 99, col(W))) == NQE_ERR_INVALID_ARGUMENT);            // unknown operator, unknown kind
    CHECK(parse_error({node(7)}) == NQE_ERR_INVALID_ARGUMENT);
    { // malformed postfix: an operator short of operands, two values left over, nothing at all
        E one = col(ID);
        N b = node(NQE_EXPR_BINARY);
        b.op = NQE_OP_PLUS;
        one.push_back(b);
        CHECK(parse_error(one) == NQE_ERR_INVALID_ARGUMENT);
        N u = node(NQE_EXPR_UNARY);
        CHECK(parse_error({u}) == NQE_ERR_INVALID_ARGUMENT);
        E two = col(ID);
        two.push_back(col(W)[0]);
        CHECK(parse_error(two) == NQE_ERR_INVALID_ARGUMENT);
        CHECK(parse_error({}) == NQE_ERR_INVALID_ARGUMENT);
    }
    { // a Utf8 literal that names bytes it does not have
        N n = node(NQE_EXPR_LITERAL);
        n.dtype = NQE_UTF8;
        n.utf8_length = 3;
        CHECK(parse_error({n}) == NQE_ERR_INVALID_ARGUMENT);
        n.utf8_length = -1;
        CHECK(parse_error({n}) == NQE_ERR_INVALID_ARGUMENT);
    }
}

// ---------------------------------------------------------------- make_aux: the quotient formula of OpAux against native / and %
static uint64_t mulhi(uint64_t a, uint64_t b) { return uint64_t(((unsigned __int128)a * b) >> 64); }
// |n| / |d| from the prepared constants, as OpAux's comment states it
static uint64_t quotient(uint64_t n, const OpAux &a) {
    if (a.pow2_shift >= 0) return n >> a.pow2_shift;
    const uint64_t q = mulhi(a.magic, n);
    return (((n - q) >> 1) + q) >> a.more;
}
static void test_make_aux() {
    const uint64_t P63 = 1ull << 63;
    std::vector<uint64_t> divisors = {1, 2, 3, 7, 10, 1000000000000000000ull, uint64_t(INT64_MAX), P63, ~0ull};
    for (int k = 1; k < 64; ++k) {
        divisors.push_back(1ull << k);
        divisors.push_back((1ull << k) - 1);
        divisors.push_back((1ull << k) + 1);
    }
    std::mt19937_64 rng(12345);
    std::vector<uint64_t> random_dividends;
    for (int i = 0; i < 300; ++i) random_dividends.push_back(rng());
    for (uint64_t d : divisors) {
        std::vector<uint64_t> dividends = {0, 1, d - 1, d, d + 1, (1ull << 32) - 1, (1ull << 32) + 1, P63 - 1, P63, ~0ull};
        dividends.insert(dividends.end(), random_dividends.begin(), random_dividends.end());
        for (int op : {NQE_OP_DIVIDE, NQE_OP_MODULOS}) {
            // UInt64
            const OpAux a = plan::make_aux(op, NQE_UINT64, d);
            CHECK(a.abs_lit == d && ((a.pow2_shift >= 0) != (a.more >= 0)));
            CHECK((a.pow2_shift >= 0) == ((d & (d - 1)) == 0));
            for (uint64_t n : dividends) {
                const uint64_t q = quotient(n, a);
                CHECK(q == n / d && n - q * a.abs_lit == n % d);
            }
            // Int64: the divisor and its negative, where they exist as Int64; the formula runs on magnitudes, the signs are C's
            for (int sign : {1, -1}) {
                if (d > P63 || (sign == 1 && d == P63)) continue;
                const int64_t y = sign == 1 ? int64_t(d) : int64_t(0ull - d);
                const OpAux s = plan::make_aux(op, NQE_INT64, uint64_t(y));
                CHECK(s.abs_lit == d);
                for (uint64_t n : dividends) {
                    const int64_t x = int64_t(n);
                    if (x == INT64_MIN && y == -1) continue; // (overflows natively: the kernels raise a flag instead)
                    const uint64_t ux = x < 0 ? 0ull - n : n, uq = quotient(ux, s), ur = ux - uq * s.abs_lit;
                    const int64_t q = int64_t(((x < 0) != (y < 0)) ? 0ull - uq : uq), r = int64_t(x < 0 ? 0ull - ur : ur);
                    CHECK(q == x / y && r == x % y);
                }
            }
        }
    }
    // nothing prepared for a zero divisor, a non-literal use (op 0), or another operator
    for (const OpAux &a : {plan::make_aux(NQE_OP_DIVIDE, NQE_INT64, 0), plan::make_aux(0, 0, 0), plan::make_aux(NQE_OP_PLUS, NQE_INT64, 8)}) CHECK(a.pow2_shift == -1 && a.more == -1);
    // Float64 `/ ±2^k`: the exact reciprocal for biased exponents 2..2044, nothing otherwise
    const double samples[] = {1.0, -3.5, 0.1, 1e300, 1e-300, 4.9406564584124654e-324, 1.7976931348623157e308, 0.0};
    for (uint64_t ex = 0; ex <= 2047; ++ex)
        for (uint64_t sign : {uint64_t(0), P63}) {
            const uint64_t lit = sign | (ex << 52);
            const OpAux a = plan::make_aux(NQE_OP_DIVIDE, NQE_FLOAT64, lit);
            CHECK((a.more == -2) == (ex >= 2 && ex <= 2044));
            CHECK(a.pow2_shift == -1);
            if (a.more != -2) continue;
            CHECK(double_of(a.magic) == 1.0 / double_of(lit));
            for (double x : samples) CHECK(bits_of(x * double_of(a.magic)) == bits_of(x / double_of(lit)));
        }
    for (double lit : {3.0, 0.1, 1.5, -6.0, 1.0000000000000002}) CHECK(plan::make_aux(NQE_OP_DIVIDE, NQE_FLOAT64, bits_of(lit)).more == -1); // a mantissa
    CHECK(plan::make_aux(NQE_OP_MODULOS, NQE_FLOAT64, bits_of(4.0)).more == -1);
}

// ---------------------------------------------------------------- make_fast_pred: the range form against the native compare
template <class T> static bool native(int op, T a, T b) {
    switch (op) {
    case NQE_OP_EQ: return a == b;
    case NQE_OP_NOT_EQ: return a != b;
    case NQE_OP_LT: return a < b;
    case NQE_OP_LT_EQ: return a <= b;
    case NQE_OP_GT: return a > b;
    default: return a >= b;
    }
}
static bool range_test(const FastPred &fp, uint64_t x) { // as documented on FastPred
    const uint64_t t = x ^ fp.flip ^ (uint64_t(int64_t(x) >> 63) & fp.fmask);
    const bool in = fp.lo <= int64_t(t) && int64_t(t) <= fp.hi;
    return in != (fp.negate != 0);
}
static void test_make_fast_pred() {
    const uint64_t TOP = 1ull << 63;
    const std::vector<uint64_t> ints = {uint64_t(INT64_MIN), uint64_t(INT64_MAX), 0, 1, ~0ull /* -1 */, TOP + 1, TOP - 2, 2, ~0ull - 1};
    const double DEN = 4.9406564584124654e-324, INF = std::numeric_limits<double>::infinity();
    std::vector<uint64_t> doubles;
    for (double d : {0.0, -0.0, DEN, -DEN, 1.0, -1.0, INF, -INF, 2.5, -1e300}) doubles.push_back(bits_of(d));
    const uint64_t nans[2] = {0x7ff8000000000000ull, 0xfff0000000000001ull};
    doubles.push_back(nans[0]);
    doubles.push_back(nans[1]);
    struct { int dt, column; const std::vector<uint64_t> *edge; } domains[3] = {{NQE_INT64, ID, &ints}, {NQE_UINT64, U, &ints}, {NQE_FLOAT64, V, &doubles}};
    for (const auto &dom : domains)
        for (int op = NQE_OP_EQ; op <= NQE_OP_GT_EQ; ++op)
            for (bool lit_left : {false, true})
                for (uint64_t lit : *dom.edge) {
                    const E e = lit_left ? bin(lit_bits(dom.dt, lit), op, col(dom.column)) : bin(col(dom.column), op, lit_bits(dom.dt, lit));
                    const ExprInfo info = plan::analyze_expr(view, e.data(), int(e.size()));
                    FastPred fp{};
                    CHECK(info.simple && info.s.col == dom.column && plan::make_fast_pred(info.s, &fp));
                    CHECK(fp.row_shift == 0 && fp.bit_mask == 0 && fp.val_mask == ~0ull);
                    for (uint64_t x : *dom.edge) {
                        bool want;
                        if (dom.dt == NQE_INT64) want = lit_left ? native(op, int64_t(lit), int64_t(x)) : native(op, int64_t(x), int64_t(lit));
                        else if (dom.dt == NQE_UINT64) want = lit_left ? native(op, lit, x) : native(op, x, lit);
                        else want = lit_left ? native(op, double_of(lit), double_of(x)) : native(op, double_of(x), double_of(lit));
                        CHECK(range_test(fp, x) == want);
                        if (dom.dt == NQE_FLOAT64 && (lit == nans[0] || lit == nans[1])) CHECK(range_test(fp, x) == (op == NQE_OP_NOT_EQ)); // a NaN literal
                    }
                }
    // the shapes it refuses still return false
    auto fast = [](const E &e) {
        const ExprInfo info = plan::analyze_expr(view, e.data(), int(e.size()));
        FastPred fp{};
        return info.simple && plan::make_fast_pred(info.s, &fp);
    };
    CHECK(fast(bin(col(ID), NQE_OP_LT, i64(5))));
    CHECK(!fast(bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_LT, i64(5)))); // two steps
    CHECK(!fast(bin(col(ID), NQE_OP_PLUS, i64(1))));                         // an arithmetic operator
    CHECK(!fast(bin(col(B), NQE_OP_EQ, boolean(true))));                     // a Boolean column
    CHECK(!fast(col(ID)));
    const FastPred bm = plan::bitmap_fast_pred();
    CHECK(bm.lo == 1 && bm.hi == 1 && bm.row_shift == 6 && bm.bit_mask == 63 && bm.val_mask == 1 && bm.fmask == 0 && bm.flip == 0 && bm.negate == 0);
}

// ---------------------------------------------------------------- match_simple (through analyze_expr)
static ExprInfo analyze(const E &e) { return plan::analyze_expr(view, e.data(), int(e.size())); }
static void test_match_simple() {
    const int ops[4] = {NQE_OP_PLUS, NQE_OP_MODULOS, NQE_OP_MULTIPLY, NQE_OP_LT};
    for (unsigned sides = 0; sides < 16; ++sides) { // bit k: the literal of step k is on the left
        E e = col(ID);
        for (int steps = 0; steps <= 5; ++steps) {
            if (steps) {
                const int k = steps - 1, op = k < 4 ? ops[k] : NQE_OP_EQ;
                const E lit = k < 4 ? i64(10 + k) : boolean(true); // (the fifth step compares the fourth step's Boolean)
                e = ((sides >> (k & 3)) & 1) ? bin(lit, op, e) : bin(e, op, lit);
            }
            const ExprInfo info = analyze(e);
            CHECK(info.simple == (steps <= SIMPLE_MAX_OPS)); // a fifth step is refused
            if (!info.simple) continue;
            CHECK(info.s.col == ID && info.s.src_dtype == NQE_INT64 && info.s.nops == steps);
            CHECK(info.s.out_dtype == (steps == 4 ? NQE_BOOLEAN : NQE_INT64) && info.out_dtype == info.s.out_dtype);
            for (int k = 0; k < steps; ++k) {
                const bool left = (sides >> k) & 1;
                CHECK(info.s.op[k] == ops[k] && info.s.lit_left[k] == (left ? 1 : 0) && info.s.lit[k] == uint64_t(10 + k) && info.s.op_dtype[k] == NQE_INT64);
                const OpAux want = left ? plan::make_aux(0, 0, 0) : plan::make_aux(ops[k], NQE_INT64, uint64_t(10 + k)); // divisor constants only for `x op lit`
                CHECK(std::memcmp(&info.s.aux[k], &want, sizeof(OpAux)) == 0);
            }
        }
    }
    CHECK(analyze(col(S)).simple && analyze(col(S)).s.nops == 0); // a bare column of any type
    CHECK(!analyze(bin(bin(col(ID), NQE_OP_LT, i64(1)), NQE_OP_AND, bin(col(ID), NQE_OP_GT, i64(0)))).simple); // and / or
    CHECK(!analyze(bin(col(B), NQE_OP_OR, boolean(true))).simple);
    CHECK(!analyze(bin(col(ID), NQE_OP_PLUS, null_of(NQE_INT64))).simple);                                     // a NULL literal
    CHECK(!analyze(bin(null_of(NQE_INT64), NQE_OP_PLUS, col(ID))).simple);
    CHECK(!analyze(bin(col(S), NQE_OP_EQ, utf8("x"))).simple);                                                 // a Utf8 literal
    CHECK(!analyze(bin(i64(3), NQE_OP_PLUS, i64(4))).simple);                                                  // a literal on both sides
    CHECK(!analyze(bin(col(ID), NQE_OP_PLUS, col(W))).simple);
    CHECK(!analyze(i64(3)).simple);
    // may_fault: a divisor that is not a literal other than 0 and -1
    CHECK(!analyze(bin(col(ID), NQE_OP_DIVIDE, i64(7))).may_fault && !analyze(bin(col(V), NQE_OP_MODULOS, f64(2.0))).may_fault);
    CHECK(analyze(bin(col(ID), NQE_OP_DIVIDE, i64(0))).may_fault && analyze(bin(col(ID), NQE_OP_MODULOS, i64(-1))).may_fault);
    CHECK(analyze(bin(col(V), NQE_OP_DIVIDE, f64(0.0))).may_fault && analyze(bin(col(V), NQE_OP_DIVIDE, f64(-0.0))).may_fault);
    CHECK(analyze(bin(i64(10), NQE_OP_DIVIDE, col(ID))).may_fault && analyze(bin(col(ID), NQE_OP_DIVIDE, null_of(NQE_INT64))).may_fault);
}

// ---------------------------------------------------------------- match_conj
struct Tree { // an and/or skeleton over leaves numbered left to right
    int leaf = -1, op = 0;
    std::vector<Tree> kids;
};
static std::vector<Tree> skeletons(int first, int n) { // every shape and every operator assignment over leaves first .. first + n - 1
    if (n == 1) { Tree t; t.leaf = first; return {t}; }
    std::vector<Tree> out;
    for (int k = 1; k < n; ++k)
        for (const Tree &l : skeletons(first, k))
            for (const Tree &r : skeletons(first + k, n - k))
                for (int op : {NQE_OP_AND, NQE_OP_OR}) { Tree t; t.op = op; t.kids = {l, r}; out.push_back(t); }
    return out;
}
static bool value_of(const Tree &t, unsigned assignment) {
    if (t.leaf >= 0) return (assignment >> t.leaf) & 1u;
    const bool l = value_of(t.kids[0], assignment), r = value_of(t.kids[1], assignment);
    return t.op == NQE_OP_AND ? (l && r) : (l || r);
}
static bool uniform(const Tree &t, int op) { return t.leaf >= 0 || (t.op == op && uniform(t.kids[0], op) && uniform(t.kids[1], op)); }
static const int LEAF_COLS[4] = {ID, W, X, Y};
static E expr_of(const Tree &t) { return t.leaf >= 0 ? bin(col(LEAF_COLS[t.leaf]), NQE_OP_LT, i64(10 + t.leaf)) : bin(expr_of(t.kids[0]), t.op, expr_of(t.kids[1])); }
static bool conj(const E &e, ConjPred *c, int *cols, const ExprView &in = view) { return plan::match_conj(in, e.data(), int(e.size()), c, cols); }
static void test_match_conj() {
    for (int n = 2; n <= 4; ++n)
        for (const Tree &t : skeletons(0, n)) {
            ConjPred c;
            int cols[CONJ_MAX] = {-1, -1, -1, -1};
            CHECK(conj(expr_of(t), &c, cols));
            CHECK(c.n == n);
            for (int k = 0; k < n; ++k) { // test k: `col < 10 + k` as a signed range
                CHECK(cols[k] == LEAF_COLS[k] && c.t[k].lo == INT64_MIN && c.t[k].hi == 9 + k && c.t[k].negate == 0 && c.t[k].flip == 0 && c.t[k].fmask == 0 && c.t[k].pre == 0);
            }
            if (uniform(t, t.op)) { // an and-list / or-list in any nesting: the straight-line form
                CHECK(c.general == 0 && c.is_or == (t.op == NQE_OP_OR ? 1 : 0));
            } else {
                CHECK(c.general == 1);
                for (unsigned a = 0; a < (1u << n); ++a) CHECK(((c.truth >> a) & 1u) == (value_of(t, a) ? 1u : 0u));
                CHECK((c.truth >> (1u << n)) == 0);
            }
        }
    { // leaves with an arithmetic step: `id % 3 = 0 and v * 2.0 > 100.0 and 100 - w >= 7`
        const E e = bin(bin(bin(bin(col(ID), NQE_OP_MODULOS, i64(3)), NQE_OP_EQ, i64(0)), NQE_OP_AND, bin(bin(col(V), NQE_OP_MULTIPLY, f64(2.0)), NQE_OP_GT, f64(100.0))), NQE_OP_AND,
                        bin(bin(i64(100), NQE_OP_MINUS, col(W)), NQE_OP_GT_EQ, i64(7)));
        ConjPred c;
        int cols[CONJ_MAX];
        CHECK(conj(e, &c, cols));
        CHECK(c.n == 3 && c.general == 1 && c.truth == 0x80u && cols[0] == ID && cols[1] == V && cols[2] == W);
        CHECK(c.t[0].pre == NQE_OP_MODULOS && c.t[0].pre_dt == NQE_INT64 && c.t[0].pre_rev == 0 && c.t[0].pre_lit == 3 && c.t[0].lo == 0 && c.t[0].hi == 0);
        const OpAux mod3 = plan::make_aux(NQE_OP_MODULOS, NQE_INT64, 3);
        CHECK(std::memcmp(&c.t[0].pre_aux, &mod3, sizeof(OpAux)) == 0);
        CHECK(c.t[1].pre == NQE_OP_MULTIPLY && c.t[1].pre_dt == NQE_FLOAT64 && c.t[1].pre_rev == 0 && c.t[1].pre_lit == bits_of(2.0) && c.t[1].fmask == 0x7fffffffffffffffull);
        CHECK(c.t[2].pre == NQE_OP_MINUS && c.t[2].pre_dt == NQE_INT64 && c.t[2].pre_rev == 1 && c.t[2].pre_lit == 100 && c.t[2].lo == 7 && c.t[2].hi == INT64_MAX);
        // a single test with an arithmetic step is taken (general form); a single plain compare is not
        CHECK(conj(bin(bin(col(ID), NQE_OP_MODULOS, i64(3)), NQE_OP_EQ, i64(0)), &c, cols) && c.n == 1 && c.general == 1 && c.truth == 2u);
    }
    ConjPred c;
    int cols[CONJ_MAX];
    const E plain = bin(col(ID), NQE_OP_LT, i64(10));
    CHECK(!conj(plain, &c, cols));                                                                    // a single plain compare
    E five = plain;
    for (int k = 0; k < 4; ++k) five = bin(five, NQE_OP_AND, plain);
    CHECK(!conj(five, &c, cols));                                                                     // a fifth leaf
    CHECK(!conj(bin(plain, NQE_OP_AND, bin(un(NQE_UNARY_ABS, col(V)), NQE_OP_LT, f64(1.0))), &c, cols)); // a unary node
    CHECK(!conj(bin(plain, NQE_OP_AND, bin(col(NI), NQE_OP_LT, i64(3))), &c, cols));                  // a nullable column
    CHECK(!conj(bin(plain, NQE_OP_AND, bin(bin(i64(10), NQE_OP_DIVIDE, col(W)), NQE_OP_GT, i64(1))), &c, cols)); // lit / col
    CHECK(!conj(bin(plain, NQE_OP_AND, bin(bin(col(V), NQE_OP_MODULOS, f64(2.0)), NQE_OP_GT, f64(1.0))), &c, cols)); // Float64 %
    CHECK(!conj(bin(plain, NQE_OP_AND, bin(col(ID), NQE_OP_LT, col(W))), &c, cols));                  // a leaf that is no `col cmp lit`
    CHECK(!conj(bin(plain, NQE_OP_AND, bin(col(ID), NQE_OP_PLUS, col(V))), &c, cols));                // a leaf that does not type-check
    CHECK(conj(bin(plain, NQE_OP_AND, bin(bin(col(V), NQE_OP_MULTIPLY, f64(2.0)), NQE_OP_GT, f64(1.0))), &c, cols));
}

// ---------------------------------------------------------------- build_program
static bool build(const E &e, ExProgram *P, bool *needs_valid) {
    int root;
    const std::vector<Node> t = plan::parse(view, e.data(), int(e.size()), &root);
    return plan::build_program(view, t, root, P, needs_valid);
}
static void test_build_program() {
    ExProgram P;
    bool nv = true;
    { // (id + 1) * (w - id): post-order, one slot per distinct column, `id` met twice takes one
        CHECK(build(bin(bin(col(ID), NQE_OP_PLUS, i64(1)), NQE_OP_MULTIPLY, bin(col(W), NQE_OP_MINUS, col(ID))), &P, &nv));
        CHECK(P.n == 3 && P.ncols == 2 && !nv);
        CHECK(P.col_values[0] == buffers[ID] && P.col_values[1] == buffers[W] && P.col_dtype[0] == NQE_INT64 && P.col_valid[0] == nullptr && P.col_valid[1] == nullptr);
        CHECK(P.ins[0].op == NQE_OP_PLUS && P.ins[0].dt == NQE_INT64 && P.ins[0].a_src == EX_COL + 0 && P.ins[0].b_src == EX_LIT && P.ins[0].lit_b == 1);
        CHECK(P.ins[1].op == NQE_OP_MINUS && P.ins[1].a_src == EX_COL + 1 && P.ins[1].b_src == EX_COL + 0);
        CHECK(P.ins[2].op == NQE_OP_MULTIPLY && P.ins[2].a_src == EX_STACK && P.ins[2].b_src == EX_STACK);
    }
    { // divisor constants ride with a literal on the right only
        CHECK(build(bin(bin(i64(100), NQE_OP_MODULOS, col(ID)), NQE_OP_MODULOS, i64(7)), &P, &nv));
        const OpAux none = plan::make_aux(0, 0, 0), mod7 = plan::make_aux(NQE_OP_MODULOS, NQE_INT64, 7);
        CHECK(P.n == 2 && P.ins[0].a_src == EX_LIT && P.ins[0].lit_a == 100 && P.ins[0].b_src == EX_COL + 0 && P.ins[0].aux.more == none.more && P.ins[0].aux.pow2_shift == none.pow2_shift);
        CHECK(P.ins[1].a_src == EX_STACK && P.ins[1].b_src == EX_LIT && std::memcmp(&P.ins[1].aux, &mod7, sizeof(OpAux)) == 0);
    }
    // the same buffer under another dtype or with a validity bitmap is another column: (values, valid, dtype) names a slot
    CHECK(build(bin(bin(col(ID), NQE_OP_PLUS, col(W)), NQE_OP_PLUS, bin(col(X), NQE_OP_PLUS, col(Y))), &P, &nv) && P.ncols == 4);
    CHECK(!build(bin(bin(bin(col(ID), NQE_OP_PLUS, col(W)), NQE_OP_PLUS, bin(col(X), NQE_OP_PLUS, col(Y))), NQE_OP_PLUS, col(Z)), &P, &nv)); // a fifth distinct column
    { // 16 instructions fit, a 17th does not
        E chain = col(ID);
        for (int k = 0; k < EX_MAX_INSTR; ++k) chain = bin(chain, NQE_OP_PLUS, i64(k));
        CHECK(build(chain, &P, &nv) && P.n == 16);
        CHECK(!build(bin(chain, NQE_OP_PLUS, i64(1)), &P, &nv));
    }
    { // the stack: three levels, not four; a unary step over the stack replaces its top, over a column it pushes
        const E s = bin(col(V), NQE_OP_PLUS, col(F2));
        CHECK(build(bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, s)), &P, &nv) && P.n == 5);
        CHECK(!build(bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, s))), &P, &nv));
        CHECK(build(bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, un(NQE_UNARY_ABS, s))), &P, &nv) && P.n == 6);
        CHECK(P.ins[3].op == EX_OP_UNARY + NQE_UNARY_ABS && P.ins[3].a_src == EX_STACK && P.ins[3].b_src == EX_NONE && P.ins[3].dt == NQE_FLOAT64);
        CHECK(build(bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, bin(un(NQE_UNARY_SIN, col(V)), NQE_OP_PLUS, f64(1.0)))), &P, &nv)); // the pushed sin(v) is the third level
        CHECK(P.ins[2].op == EX_OP_UNARY + NQE_UNARY_SIN && P.ins[2].a_src == EX_COL + 0 && plan::program_has_trig(P));
        CHECK(!build(bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, bin(s, NQE_OP_PLUS, un(NQE_UNARY_SIN, col(V))))), &P, &nv));      // … and a fourth here
        CHECK(build(un(NQE_UNARY_ABS, s), &P, &nv) && !plan::program_has_trig(P));
    }
    CHECK(!build(bin(col(S), NQE_OP_EQ, utf8("x")), &P, &nv));                // a Utf8 column, a Utf8 literal
    CHECK(!build(bin(utf8("y"), NQE_OP_EQ, utf8("x")), &P, &nv));
    CHECK(!build(col(ID), &P, &nv) && !build(i64(1), &P, &nv));               // no operator node: no program
    CHECK(build(bin(col(ID), NQE_OP_PLUS, i64(1)), &P, &nv) && !nv);
    CHECK(build(bin(col(ID), NQE_OP_PLUS, null_of(NQE_INT64)), &P, &nv) && nv && P.ins[0].b_src == EX_LIT_NULL); // needs_valid: a NULL literal, a nullable column
    CHECK(build(bin(col(NI), NQE_OP_PLUS, i64(1)), &P, &nv) && nv && P.col_valid[0] == reinterpret_cast<const uint8_t *>(ni_valid));
    CHECK(build(bin(col(B), NQE_OP_AND, bin(col(ID), NQE_OP_LT, i64(3))), &P, &nv) && P.col_dtype[1] == NQE_BOOLEAN && P.ins[1].a_src == EX_COL + 1 && P.ins[1].dt == NQE_BOOLEAN); // Boolean columns load (slots in post-order: `id` first)
    // program_of: the requirements
    plan::ExprProgram ep;
    auto prog = [&](const E &e, unsigned req) { return plan::program_of(view, e.data(), int(e.size()), req, &ep); };
    const E cmp = bin(col(ID), NQE_OP_LT, i64(3)), sum = bin(col(ID), NQE_OP_PLUS, i64(3)), absv = un(NQE_UNARY_ABS, bin(col(V), NQE_OP_PLUS, f64(1.0)));
    CHECK(prog(cmp, plan::REQ_BINARY_ROOT | plan::REQ_BOOLEAN | plan::REQ_NO_NULLS) && ep.top().out_dtype == NQE_BOOLEAN && ep.P.n == 1 && !ep.needs_valid);
    CHECK(!prog(sum, plan::REQ_BOOLEAN) && prog(sum, plan::REQ_NOT_BOOLEAN) && !prog(cmp, plan::REQ_NOT_BOOLEAN));
    CHECK(prog(absv, 0) && !prog(absv, plan::REQ_BINARY_ROOT));
    CHECK(prog(bin(col(NI), NQE_OP_LT, i64(3)), 0) && ep.needs_valid && !prog(bin(col(NI), NQE_OP_LT, i64(3)), plan::REQ_NO_NULLS));
    CHECK(!prog(col(ID), 0) && ep.top().kind == NQE_EXPR_COLUMN && ep.top().column == ID); // the parsed tree is there for the caller
    // the slot table's policies
    SlotTable slots;
    CHECK(slots.slot_of(buffers[ID], nullptr, NQE_INT64, 2) == 0 && slots.slot_of(buffers[W], nullptr, NQE_INT64, 2) == 1 && slots.slot_of(buffers[ID], nullptr, NQE_INT64, 2) == 0);
    CHECK(slots.slot_of(buffers[X], nullptr, NQE_INT64, 2) == -1 && slots.slot_of(buffers[X], nullptr, NQE_INT64, 3) == 2);
    CHECK(slots.slot_of(buffers[B], nullptr, NQE_BOOLEAN, 8, true) == -1 && slots.slot_of(buffers[NI], reinterpret_cast<const uint8_t *>(ni_valid), NQE_INT64, 8, true) == -1 && slots.n == 3);
    CHECK(build(bin(col(Y), NQE_OP_PLUS, bin(col(W), NQE_OP_PLUS, null_of(NQE_INT64))), &P, &nv));
    ExProgram Q = P;
    uint32_t used = 0;
    CHECK(!slots.renumber(Q, 8, true, &used, true)); // the NULL literal
    Q = P;
    CHECK(slots.renumber(Q, 8, true, &used, false) && used == ((1u << 1) | (1u << 3)) && Q.ins[0].a_src == EX_COL + 1 && Q.ins[1].a_src == EX_COL + 3 && slots.n == 4);
}

// ---------------------------------------------------------------- match_tree_pred
static bool tree(const E &e, TreePred *t, const ExprView &in = view) { return plan::match_tree_pred(in, e.data(), int(e.size()), t); }
static void test_match_tree_pred() {
    TreePred t;
    { // v < 20 or id % 3 = 0
        CHECK(tree(bin(bin(col(V), NQE_OP_LT, f64(20.0)), NQE_OP_OR, bin(bin(col(ID), NQE_OP_MODULOS, i64(3)), NQE_OP_EQ, i64(0))), &t));
        CHECK(t.n == 4 && t.ncols == 2 && t.col[0] == V && t.col[1] == ID);
        CHECK(t.ins[0].op == NQE_OP_LT && t.ins[0].dt == NQE_FLOAT64 && t.ins[0].a_src == TS_W0 && t.ins[0].b_src == TS_LIT && t.ins[0].lit_b == bits_of(20.0) && t.ins[0].lit_a == 0);
        CHECK(t.ins[1].op == NQE_OP_MODULOS && t.ins[1].a_src == TS_W0 + 1 && t.ins[1].b_src == TS_LIT && t.ins[1].lit_b == 3);
        const OpAux mod3 = plan::make_aux(NQE_OP_MODULOS, NQE_INT64, 3);
        CHECK(std::memcmp(&t.ins[1].aux, &mod3, sizeof(OpAux)) == 0);
        CHECK(t.ins[2].op == NQE_OP_EQ && t.ins[2].a_src == TS_STACK && t.ins[2].b_src == TS_LIT && t.ins[2].lit_b == 0);
        CHECK(t.ins[3].op == NQE_OP_OR && t.ins[3].a_src == TS_STACK && t.ins[3].b_src == TS_STACK);
    }
    CHECK(tree(bin(bin(col(ID), NQE_OP_PLUS, col(W)), NQE_OP_GT, col(X)), &t) && t.n == 2 && t.ncols == 3 && t.col[0] == ID && t.col[1] == W && t.col[2] == X); // a + b > c
    CHECK(t.ins[0].a_src == TS_W0 && t.ins[0].b_src == TS_W0 + 1 && t.ins[1].a_src == TS_STACK && t.ins[1].b_src == TS_W0 + 2);
    // a literal on the left swaps, and is remembered for the operators that are not commutative
    const int ops[] = {NQE_OP_EQ, NQE_OP_NOT_EQ, NQE_OP_LT, NQE_OP_LT_EQ, NQE_OP_GT, NQE_OP_GT_EQ};
    for (int op : ops) {
        CHECK(tree(bin(i64(5), op, col(ID)), &t) && t.n == 1 && t.ins[0].op == op && t.ins[0].a_src == TS_W0 && t.ins[0].b_src == TS_LIT && t.ins[0].lit_b == 5);
        CHECK(t.ins[0].lit_a == ((op == NQE_OP_EQ || op == NQE_OP_NOT_EQ) ? 0u : 1u));
    }
    for (int op : {NQE_OP_PLUS, NQE_OP_MINUS, NQE_OP_MULTIPLY}) {
        CHECK(tree(bin(bin(i64(5), op, col(ID)), NQE_OP_GT, i64(3)), &t) && t.n == 2 && t.ins[0].a_src == TS_W0 && t.ins[0].b_src == TS_LIT && t.ins[0].lit_b == 5);
        CHECK(t.ins[0].lit_a == (op == NQE_OP_MINUS ? 1u : 0u) && t.ins[0].aux.pow2_shift == -1 && t.ins[0].aux.more == -1);
    }
    const E lt = bin(col(ID), NQE_OP_LT, i64(3)), lt2 = bin(col(W), NQE_OP_LT, i64(4));
    CHECK(tree(bin(bin(lt, NQE_OP_OR, lt2), NQE_OP_AND, bin(lt2, NQE_OP_OR, lt)), &t)); // three Boolean levels
    CHECK(!tree(bin(col(ID), NQE_OP_LT, null_of(NQE_INT64)), &t));                                                  // a NULL literal
    CHECK(!tree(bin(un(NQE_UNARY_ABS, col(V)), NQE_OP_LT, f64(1.0)), &t));                                          // a unary step
    CHECK(!tree(bin(col(B), NQE_OP_AND, lt), &t) && !tree(bin(lt, NQE_OP_OR, boolean(true)), &t));                  // a Boolean column / literal under and / or
    CHECK(!tree(bin(lt, NQE_OP_EQ, lt2), &t));                                                                      // comparing Booleans
    CHECK(!tree(bin(bin(col(ID), NQE_OP_MODULOS, i64(0)), NQE_OP_EQ, i64(1)), &t));                                 // divisor 0, -1, +-0.0
    CHECK(!tree(bin(bin(col(ID), NQE_OP_DIVIDE, i64(-1)), NQE_OP_GT, i64(0)), &t));
    CHECK(!tree(bin(bin(col(V), NQE_OP_DIVIDE, f64(0.0)), NQE_OP_GT, f64(1.0)), &t) && !tree(bin(bin(col(V), NQE_OP_DIVIDE, f64(-0.0)), NQE_OP_GT, f64(1.0)), &t));
    CHECK(tree(bin(bin(col(V), NQE_OP_DIVIDE, f64(4.0)), NQE_OP_GT, f64(1.0)), &t) && tree(bin(bin(col(ID), NQE_OP_DIVIDE, i64(-2)), NQE_OP_GT, i64(0)), &t));
    CHECK(!tree(bin(bin(i64(10), NQE_OP_DIVIDE, col(ID)), NQE_OP_GT, i64(1)), &t));                                 // lit / col
    CHECK(!tree(bin(bin(col(ID), NQE_OP_DIVIDE, col(W)), NQE_OP_GT, i64(1)), &t));
    CHECK(!tree(bin(bin(col(ID), NQE_OP_PLUS, col(W)), NQE_OP_GT, bin(col(X), NQE_OP_PLUS, i64(1))), &t));          // two live arithmetic subtrees
    CHECK(!tree(bin(lt, NQE_OP_OR, bin(lt2, NQE_OP_OR, bin(lt, NQE_OP_OR, lt2))), &t));                             // four Boolean levels
    CHECK(!tree(bin(col(NI), NQE_OP_LT, i64(3)), &t));                                                              // a nullable column
    CHECK(!tree(bin(bin(bin(col(ID), NQE_OP_PLUS, col(W)), NQE_OP_PLUS, col(X)), NQE_OP_GT, col(Y)), &t));          // 4 columns
    CHECK(!tree(bin(col(ID), NQE_OP_PLUS, i64(1)), &t) && !tree(col(B), &t));                                       // not a predicate, no BINARY root
    CHECK(!tree(bin(col(ID), NQE_OP_LT, f64(1.0)), &t));                                                            // does not type-check: false, no throw
    E chain = col(ID);
    for (int k = 0; k < TREE_MAX_INSTR - 1; ++k) chain = bin(chain, NQE_OP_PLUS, i64(k));
    CHECK(tree(bin(chain, NQE_OP_GT, i64(0)), &t) && t.n == TREE_MAX_INSTR);
    CHECK(!tree(bin(bin(chain, NQE_OP_PLUS, i64(1)), NQE_OP_GT, i64(0)), &t));                                      // 13 instructions
}

int main() {
    test_parse();
    test_make_aux();
    test_make_fast_pred();
    test_match_simple();
    test_match_conj();
    test_build_program();
    test_match_tree_pred();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("expr plan ok\n");
    return 0;
}
