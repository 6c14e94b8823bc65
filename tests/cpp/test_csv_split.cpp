// CPU unit test of csrc/csv_split.hpp (the same code runs in the device kernels of csv.hip): the transition vectors of
// the quoting automaton, exhaustively over the four byte classes (newline, quote, delimiter, other).
//   1. csv_step against a transition table written out by hand from the csv crate's rules;
//   2. vec_compose is function composition (against the vector of the concatenated string, and entry by entry),
//      is associative, and VEC_ID is neutral on both sides, on every vector a chunk of <= 6 bytes can produce;
//   3. for every string of <= 8 bytes and every split of it into chunks of 1, 2 and 3 bytes, composing the chunk
//      vectors and reading entry ST_R gives the state of the sequential walk;
//   4. record starts and ends, counted chunk by chunk from the composed incoming states with the end-of-file rule of
//      csv_mark_kernel (the chunk that ends at n closes an open record), are equal in number and equal to the walk's.
// Built and run by tests/test_csv_host.py.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../naive_query_engine_amd/csrc/csv_split.hpp"

using namespace nqe::csv_split;

static long long checked = 0, failed = 0;
#define CHECK(cond, ...)                                                                                                                   \
    do {                                                                                                                                   \
        ++checked;                                                                                                                         \
        if (!(cond)) {                                                                                                                     \
            if (++failed < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); }                          \
        }                                                                                                                                  \
    } while (0)

static const uint8_t CLASSES[4] = {'\n', '"', ',', 'x'};
static const uint8_t DELIM = ',';

// the csv crate's reader, as a table: [state][class: newline, quote, delimiter, other]
//   R (record start): an empty line stays; a quote opens a quoted field; the delimiter ends an empty field
//   F (field start):  as R, but a newline ends the record
//   U (unquoted):     quotes are literal
//   Q (quoted):       only a quote matters
//   E (quote seen in Q): a second quote is an escaped pair (back to Q); anything else: the field goes on unquoted
static const uint32_t TABLE[5][4] = {
    {ST_R, ST_Q, ST_F, ST_U}, {ST_R, ST_Q, ST_F, ST_U}, {ST_R, ST_U, ST_F, ST_U}, {ST_Q, ST_E, ST_Q, ST_Q}, {ST_R, ST_Q, ST_F, ST_U},
};

static std::string printable(const std::string &s) {
    std::string o;
    for (char c : s) o += c == '\n' ? 'N' : c;
    return o;
}

static uint32_t walk(uint32_t st, const std::string &s, size_t lo, size_t hi, int *ns = nullptr, int *ne = nullptr) {
    for (size_t i = lo; i < hi; ++i) {
        bool a, b;
        st = csv_step(st, uint8_t(s[i]), DELIM, &a, &b);
        if (ns && a) ++*ns;
        if (ne && b) ++*ne;
    }
    return st;
}
// what csv_vec_kernel packs for one chunk
static uint32_t chunk_vec(const std::string &s, size_t lo, size_t hi) {
    uint32_t v = 0;
    for (uint32_t st = 0; st < 5; ++st) v |= walk(st, s, lo, hi) << (3 * st);
    return v;
}

static void strings_up_to(int maxlen, std::vector<std::string> &out) {
    out.push_back("");
    size_t lo = 0;
    for (int len = 1; len <= maxlen; ++len) {
        const size_t hi = out.size();
        for (size_t i = lo; i < hi; ++i)
            for (uint8_t c : CLASSES) out.push_back(out[i] + char(c));
        lo = hi;
    }
}

// every split of s[pos..) into chunks of 1, 2 and 3 bytes; `pre` = composed vector of s[0..pos), ns/ne = marks counted so far
static void splits(const std::string &s, size_t pos, uint32_t pre, int ns, int ne, uint32_t seq_state, int seq_ns, int seq_ne) {
    const size_t n = s.size();
    if (pos == n) {
        CHECK(vec_get(pre, ST_R) == seq_state, "'%s': chunked state %u, sequential %u", printable(s).c_str(), vec_get(pre, ST_R), seq_state);
        CHECK(ns == ne && ns == seq_ns && ne == seq_ne, "'%s': %d starts, %d ends (sequential %d / %d)", printable(s).c_str(), ns, ne, seq_ns, seq_ne);
        return;
    }
    for (size_t len = 1; len <= 3 && pos + len <= n; ++len) {
        const size_t hi = pos + len;
        int a = 0, b = 0;
        const uint32_t st = walk(vec_get(pre, ST_R), s, pos, hi, &a, &b); // csv_mark_kernel: incoming state = entry ST_R of the prefix
        if (hi == n && st != ST_R) ++b;                                   // the last record has no terminator
        splits(s, hi, vec_compose(pre, chunk_vec(s, pos, hi)), ns + a, ne + b, seq_state, seq_ns, seq_ne);
    }
}

int main() {
    // 1. csv_step against the table, with its record marks; '\r' behaves as '\n'
    for (uint32_t st = 0; st < 5; ++st)
        for (int k = 0; k < 4; ++k) {
            bool a, b;
            const uint32_t nx = csv_step(st, CLASSES[k], DELIM, &a, &b);
            CHECK(nx == TABLE[st][k], "step(%u, class %d) = %u, table %u", st, k, nx, TABLE[st][k]);
            CHECK(a == (st == ST_R && k != 0), "rec_start(%u, class %d)", st, k);
            CHECK(b == (k == 0 && (st == ST_F || st == ST_U || st == ST_E)), "rec_end(%u, class %d)", st, k);
            if (k == 0) {
                bool a2, b2;
                CHECK(csv_step(st, '\r', DELIM, &a2, &b2) == nx && a2 == a && b2 == b, "CR differs from LF in state %u", st);
            }
        }
    CHECK(is_nl('\n') && is_nl('\r') && !is_nl('"') && !is_nl(',') && !is_nl('x') && !is_nl(0), "is_nl");
    for (uint32_t st = 0; st < 5; ++st) CHECK(vec_get(VEC_ID, st) == st, "VEC_ID entry %u", st);

    // 2. the vectors of all chunks of <= 6 bytes, one representative string each
    std::vector<std::string> s6;
    strings_up_to(6, s6);
    std::map<uint32_t, std::string> reach;
    for (const std::string &s : s6) reach.emplace(chunk_vec(s, 0, s.size()), s);
    printf("%zu distinct vectors from %zu chunks\n", reach.size(), s6.size());
    CHECK(reach.count(VEC_ID) == 1, "the empty chunk gives the identity");
    for (const auto &x : reach) {
        CHECK(vec_compose(VEC_ID, x.first) == x.first, "VEC_ID is not left-neutral for %05o", x.first);
        CHECK(vec_compose(x.first, VEC_ID) == x.first, "VEC_ID is not right-neutral for %05o", x.first);
        for (const auto &y : reach) {
            const uint32_t xy = vec_compose(x.first, y.first);
            const std::string cat = x.second + y.second;
            CHECK(xy == chunk_vec(cat, 0, cat.size()), "compose('%s', '%s') is not the vector of the concatenation", printable(x.second).c_str(), printable(y.second).c_str());
            CHECK(xy < (1u << 15), "compose sets bits above entry 4");
            for (uint32_t st = 0; st < 5; ++st) {
                const uint32_t mid = walk(st, x.second, 0, x.second.size());
                CHECK(((xy >> (3 * st)) & 7u) == walk(mid, y.second, 0, y.second.size()), "entry %u of compose('%s', '%s')", st, printable(x.second).c_str(), printable(y.second).c_str());
            }
            for (const auto &z : reach)
                CHECK(vec_compose(xy, z.first) == vec_compose(x.first, vec_compose(y.first, z.first)), "not associative: %05o %05o %05o", x.first, y.first, z.first);
        }
    }
    // the same at string level for all pairs of chunks of <= 4 bytes (no representative in between)
    std::vector<std::string> s4;
    strings_up_to(4, s4);
    for (const std::string &x : s4)
        for (const std::string &y : s4) {
            const std::string cat = x + y;
            CHECK(vec_compose(chunk_vec(x, 0, x.size()), chunk_vec(y, 0, y.size())) == chunk_vec(cat, 0, cat.size()), "compose('%s', '%s')", printable(x).c_str(), printable(y).c_str());
        }

    // 3 + 4. every string of <= 8 bytes, every split into chunks of 1, 2 and 3 bytes
    std::vector<std::string> s8;
    strings_up_to(8, s8);
    for (const std::string &s : s8) {
        int ns = 0, ne = 0;
        const uint32_t st = walk(ST_R, s, 0, s.size(), &ns, &ne);
        if (!s.empty() && st != ST_R) ++ne;
        // the table's own walk, so that csv_step is not its own reference
        uint32_t ts = ST_R;
        for (char c : s) ts = TABLE[ts][c == '\n' ? 0 : c == '"' ? 1 : c == ',' ? 2 : 3];
        CHECK(ts == st, "'%s': csv_step walk %u, table walk %u", printable(s).c_str(), st, ts);
        splits(s, 0, VEC_ID, 0, 0, st, ns, ne);
    }
    printf("%lld checks, %lld failures\n", checked, failed);
    return failed ? 1 : 0;
}
