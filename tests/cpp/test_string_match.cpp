// The per-string rules of string matching (naive_query_engine_amd/csrc/string_match_parts.hpp, quirk Q27) on the CPU: that header alone,
// over every byte string of up to 6 bytes of a six-symbol alphabet (two letters, a continuation byte, a two-byte lead, `%` and `_`) and
// every pattern of a fixed list, against a matcher written here that shares nothing with the header (it tries every cut, and numbers the
// characters by c(j) itself).  Each string is decided three ways — by one thread, and chunked in groups of 4 and of 8 candidate positions
// the way str_match_scan walks (a position per lane, and 8 positions per lane out of two words for a segment of at most 8 literal bytes;
// longer strings take that walk past its first chunk) — and STRPOS's position and character number are checked for the segments without ONE.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_string_match.cpp && ./a.out
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "string_match_parts.hpp"

using namespace nqe;
using namespace nqe::strmatch;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            if (++failures <= 40) std::printf("%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

// ---- the reference: elements, character numbers, every cut
enum Kind { LIT, ANY, ONE };
struct Elem {
    Kind kind;
    uint8_t byte;
};
static std::vector<Elem> parse_like(const std::string &p) {
    std::vector<Elem> out;
    for (size_t i = 0; i < p.size(); ++i) {
        const uint8_t b = uint8_t(p[i]);
        if (b == '\\' && i + 1 < p.size()) out.push_back({LIT, uint8_t(p[++i])});
        else if (b == '%') { if (out.empty() || out.back().kind != ANY) out.push_back({ANY, 0}); }
        else if (b == '_') out.push_back({ONE, 0});
        else out.push_back({LIT, b});
    }
    return out;
}
static std::vector<uint64_t> char_numbers(const std::string &s) {
    std::vector<uint64_t> c;
    uint64_t seen = 0;
    for (char ch : s) {
        seen += (uint8_t(ch) & 0xC0) != 0x80;
        c.push_back(seen ? seen : 1);
    }
    return c;
}
static uint8_t lower(uint8_t b) { return (b >= 'A' && b <= 'Z') ? uint8_t(b + 0x20) : b; }
static bool ref_match(const std::string &s, const std::vector<uint64_t> &c, const std::vector<Elem> &els, size_t k, size_t i, bool fold) {
    if (k == els.size()) return i == s.size();
    const Elem &e = els[k];
    if (e.kind == ANY) {
        for (size_t j = i; j <= s.size(); ++j)
            if (ref_match(s, c, els, k + 1, j, fold)) return true;
        return false;
    }
    if (i >= s.size()) return false;
    if (e.kind == LIT) return (fold ? lower(uint8_t(s[i])) : uint8_t(s[i])) == (fold ? lower(e.byte) : e.byte) && ref_match(s, c, els, k + 1, i + 1, fold);
    // ONE: exactly the bytes {j : c(j) = c(i)}, so i must be the first of them
    if (i > 0 && c[i - 1] == c[i]) return false;
    size_t j = i;
    while (j < s.size() && c[j] == c[i]) ++j;
    return ref_match(s, c, els, k + 1, j, fold);
}

// ---- the pattern as the header takes it, built from the same elements
struct Built {
    std::vector<uint8_t> el, one;
    std::vector<SegView> segs;
    Pattern P;
};
static void build(const std::vector<Elem> &els, bool fold, Built *b) {
    b->el.clear(); b->one.clear(); b->segs.clear();
    bool open = false, has_any = false;
    for (const Elem &e : els) {
        if (e.kind == ANY) { open = false; has_any = true; continue; }
        if (!open) { b->segs.push_back({uint32_t(b->el.size()), 0, 0, 0}); open = true; }
        b->el.push_back(e.kind == ONE ? 0 : (fold ? lower(e.byte) : e.byte));
        b->one.push_back(e.kind == ONE ? 1 : 0);
        b->segs.back().len += 1;
        b->segs.back().ones += e.kind == ONE ? 1 : 0;
    }
    b->el.push_back(0); b->one.push_back(0); // (never empty: data() is a pointer)
    b->P.el = b->el.data();
    b->P.one = b->one.data();
    b->P.segs = b->segs.data();
    b->P.nseg = uint32_t(b->segs.size());
    b->P.min_bytes = uint32_t(b->el.size() - 1);
    b->P.anchored_front = els.empty() || els.front().kind != ANY;
    b->P.anchored_back = els.empty() || els.back().kind != ANY;
    b->P.has_any = has_any;
    b->P.negate = 0;
    b->P.has_one = 0;
    for (const SegView &sg : b->segs) b->P.has_one |= sg.ones != 0;
}

// ---- the chunked walk of str_match_scan: G lanes test G candidate positions from the cursor, the lowest set bit of their ballot wins
template <bool FOLD> static bool chunked(const Pattern &P, const uint8_t *p, uint32_t len, uint32_t G, uint32_t *pos) {
    const uint32_t lead = leading_continuations(p, len);
    uint32_t first, cur, bs;
    int32_t last;
    bool decided;
    *pos = 0;
    if (!walk_begin<FOLD>(P, p, len, lead, &first, &last, &cur, &bs, &decided)) return false;
    if (decided) return true;
    uint32_t c0 = cur;
    for (;;) {
        const SegView s = P.segs[first];
        if (is_word_segment(s.len, s.ones)) {
            // the word walk: lane `sub` holds the 16 bytes from c0 + 8 * sub and tests 8 positions, a chunk is 8 * G positions; what lies
            // behind the string's end in a loaded word is junk on purpose (0xEE here, 0x80 on the device: no candidate may look at it)
            const uint64_t mask = word_mask(s.len);
            uint64_t word = 0;
            for (uint32_t k = 0; k < s.len; ++k) word |= uint64_t(P.el[s.off + k]) << (8 * k);
            auto load = [&](uint32_t at) {
                uint64_t w = 0;
                for (uint32_t k = 0; k < 8; ++k) w |= uint64_t(at + k < len ? folded<FOLD>(p[at + k]) : uint8_t(0xEE)) << (8 * k);
                return w;
            };
            bool found = false;
            for (uint32_t sub = 0; sub < G && !found; ++sub) { // (ascending: the first lane with a bit set holds the leftmost candidate)
                const uint32_t i = c0 + 8 * sub;
                if (i + s.len > bs) continue;
                const uint32_t bits = word_candidates(load(i), i + 8 < len ? load(i + 8) : 0ull, word, mask, i, s.len, bs);
                if (bits) {
                    *pos = i + uint32_t(__builtin_ctz(bits));
                    cur = c0 = *pos + s.len;
                    found = true;
                }
            }
            if (found) {
                if (int32_t(++first) > last) return true;
            } else {
                c0 += 8 * G;
                if (c0 + s.len > bs) return false;
            }
            continue;
        }
        uint64_t cand = 0;
        int32_t ends[64];
        for (uint32_t sub = 0; sub < G; ++sub) {
            const uint32_t i = c0 + sub;
            int32_t e = -1;
            if (i + s.len <= bs) {
                e = match_at<FOLD>(p, len, lead, i, P.el + s.off, P.one + s.off, s.len, s.ones != 0);
                if (e >= 0 && uint32_t(e) > bs) e = -1;
            }
            ends[sub] = e;
            if (e >= 0) cand |= 1ull << sub;
        }
        if (cand) {
            const int b = __builtin_ctzll(cand);
            *pos = c0 + uint32_t(b);
            cur = c0 = uint32_t(ends[b]);
            if (int32_t(++first) > last) return true;
        } else {
            c0 += G;
            if (c0 + P.segs[first].len > bs) return false;
        }
    }
}

static const char *const PATTERNS[] = {"", "%", "a", "ab", "a%", "%a", "%ab", "ab%", "a%b", "ab%ba", "a%a", "%a%", "%ab%", "%\xc3\xa9%", "_", "__", "%_", "_%", "_%_", "%_%", "a_", "_a", "a_b",
                                       "%a_", "_a%", "%a%b%", "%a%b", "a%b%", "a%b%a", "%ab%ba%", "%a_b%", "%_a_%", "\\%", "\\_", "%\\%%", "\\_%", "%\\_", "%\xa9", "\xc3%", "%\xc3_", "_\xc3%",
                                       "%b_%a", "%aa%aa%", "%_\xa9", "\xa9_%", "%a%_", "_%_%_", "%\\_\\%%", "a\\", "%__a", "%\xa9%\xa9%"};
static const char *const FOLDED[] = {"A%", "%aB%", "_A%", "%B", "a%B%A"};
static const char ALPHABET[6] = {'a', 'b', '\xa9', '\xc3', '%', '_'};

static long checked = 0;
template <bool FOLD> static void check(const std::string &s, const std::vector<Elem> &els, const Built &b, const char *pattern) {
    // the string in a buffer of exactly its size: the sanitizer sees a read behind it
    std::vector<uint8_t> buf(s.begin(), s.end());
    buf.shrink_to_fit();
    const uint8_t *p = buf.empty() ? nullptr : buf.data();
    const uint32_t len = uint32_t(s.size());
    const bool want = ref_match(s, char_numbers(s), els, 0, 0, FOLD);
    uint32_t pos1, pos4, pos8;
    const bool one = match_one_thread<FOLD>(b.P, p, len, &pos1), by4 = chunked<FOLD>(b.P, p, len, 4, &pos4), by8 = chunked<FOLD>(b.P, p, len, 8, &pos8);
    if (one != want || by4 != want || by8 != want) {
        if (++failures <= 40) {
            std::printf("pattern '%s' over [", pattern);
            for (uint8_t c : buf) std::printf("%02x ", c);
            std::printf("]: want %d, one thread %d, by 4 %d, by 8 %d\n", want, one, by4, by8);
        }
    }
    // %lit% without ONE: the position is the leftmost occurrence's, and STRPOS's character number is c of that byte
    if (want && b.P.nseg == 1 && !b.P.anchored_front && !b.P.anchored_back && b.segs[0].ones == 0 && !FOLD) {
        const size_t at = s.find(std::string((const char *)b.el.data(), b.segs[0].len));
        CHECK(at == pos1 && at == pos4 && at == pos8);
        CHECK(char_number(p, pos1) == char_numbers(s)[at]);
    }
    ++checked;
}

int main() {
    // every string of up to 6 symbols
    std::vector<std::string> strings = {""};
    for (size_t from = 0, n = 1; n <= 6; ++n) {
        const size_t to = strings.size();
        for (size_t k = from; k < to; ++k)
            for (char ch : ALPHABET) strings.push_back(strings[k] + ch);
        from = to;
    }
    CHECK(strings.size() == 55987);
    Built b;
    for (const char *pat : PATTERNS) {
        const std::vector<Elem> els = parse_like(pat);
        build(els, false, &b);
        for (const std::string &s : strings) check<false>(s, els, b, pat);
    }
    // ILIKE: the strings' letters in upper case as well
    for (const char *pat : FOLDED) {
        const std::vector<Elem> els = parse_like(pat);
        build(els, true, &b);
        for (const std::string &s : strings) {
            if (s.size() > 5) break;
            check<true>(s, els, b, pat);
            std::string u = s;
            for (char &ch : u) ch = ch == 'a' ? 'A' : ch == 'b' ? 'B' : ch;
            check<true>(u, els, b, pat);
        }
    }
    // the word walk past its first chunk: strings of 8G-2 .. 8G+2 and 16G-1 .. 16G+1 bytes (G = 4 and 8) with the literal at every position
    for (const char *pat : {"%xy%", "%x%y%z%", "q%x%yz%", "%xy", "%x%yq", "%\xc3\xa9xy%"}) {
        const std::vector<Elem> els = parse_like(pat);
        build(els, false, &b);
        for (uint32_t G : {4u, 8u})
            for (uint32_t n : {8 * G - 2, 8 * G - 1, 8 * G, 8 * G + 1, 8 * G + 2, 16 * G - 1, 16 * G, 16 * G + 1}) {
                check<false>(std::string(n, 'q'), els, b, pat);
                for (uint32_t at = 0; at + 2 <= n; ++at) {
                    std::string s(n, 'q');
                    s[at] = 'x'; s[at + 1] = 'y';
                    check<false>(s, els, b, pat);
                    if (at + 3 <= n) { s[at + 2] = 'z'; check<false>(s, els, b, pat); }
                    if (at >= 4) { s[at - 1] = '\xa9'; s[at - 2] = '\xc3'; s[0] = 'x'; s[2] = 'y'; check<false>(s, els, b, pat); }
                }
            }
    }
    const uint8_t lead2[] = {0xa9, 0xa9, 'a', 0xa9, 'b'};
    CHECK(leading_continuations(lead2, 5) == 2 && is_char_start(lead2, 2, 0) && !is_char_start(lead2, 2, 2) && is_char_start(lead2, 2, 4));
    CHECK(char_end(lead2, 5, 2, 0) == 4 && char_end(lead2, 5, 2, 4) == 5 && char_end(lead2, 2, 2, 0) == 2);
    CHECK(folded<true>('A') == 'a' && folded<true>('Z') == 'z' && folded<true>('[') == '[' && folded<true>('@') == '@' && folded<true>(0xc9) == 0xc9 && folded<false>('A') == 'A');
    CHECK(char_number(lead2, 0) == 1 && char_number(lead2, 2) == 1 && char_number(lead2, 4) == 2);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("string match ok: %ld strings\n", checked);
    return 0;
}
