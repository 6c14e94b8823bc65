// The rules of the string functions with arguments (naive_query_engine_amd/csrc/string_args_parts.hpp, quirk Q26) on the CPU: this file
// includes that header alone and runs EVERY byte string of up to 7 bytes over the alphabet {0x20, 'A', 'z', 0xC3 (a lead byte), 0xA9 (a
// continuation byte), 0xF0} against a sequential reference written here from the rules in include/nqe.h:
//   SUBSTR   every start in [-2, 9] plus INT64_MAX and INT64_MIN, every len in {-1, 0, 1, 2, 8, INT64_MAX}: one thread's answer and the
//            lanes' walk (chunks of G words, the carried prefix, the early stop) against the literal c(j) rule;
//   REPLACE  every `from` of up to 3 bytes, `to` in {"", "x", "xyz"}: the chunked walk (candidates, greedy resolution with the carried
//            next free position, the placement of every byte) against a find-and-append loop, and has_border against whether any of
//            the strings holds two overlapping occurrences;
//   the saturating lengths at their edges.
// Longer random strings take the same walks over several chunks for every group size.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_string_args.cpp && ./a.out
#include "string_args_parts.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

using namespace nqe::strargs;
using Bytes = std::vector<uint8_t>;

static std::atomic<int> failures{0};
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                         \
    } while (0)

static const uint8_t ALPHABET[6] = {0x20, 'A', 'z', 0xC3, 0xA9, 0xF0};
static const int64_t STARTS[14] = {-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, INT64_MAX, INT64_MIN};
static const int64_t COUNTS[6] = {-1, 0, 1, 2, 8, INT64_MAX};

static bool same_bytes(const uint8_t *p, const Bytes &ref) { return ref.empty() || std::memcmp(p, ref.data(), ref.size()) == 0; }

// ---- the sequential reference
static bool ref_cont(uint8_t b) { return (b & 0xC0) == 0x80; }
// the kept bytes by the literal rule: max(start, 1) <= c(j) < start + len, the sum saturating; *contiguous: they form one range
static const Bytes &ref_substr(const uint8_t *s, uint32_t len, int64_t start, int64_t count, bool *contiguous) {
    __int128 hi = __int128(start) + __int128(count);
    if (hi > __int128(INT64_MAX)) hi = INT64_MAX;
    const __int128 lo = start < 1 ? 1 : start;
    static thread_local Bytes out; // (reused: this runs thirty million times)
    out.clear();
    int64_t seen = 0, last = -2;
    *contiguous = true;
    for (uint32_t j = 0; j < len; ++j) {
        if (!ref_cont(s[j])) ++seen;
        const int64_t c = seen < 1 ? 1 : seen;
        if (lo <= c && c < hi) {
            if (!out.empty() && last != int64_t(j) - 1) *contiguous = false;
            out.push_back(s[j]);
            last = j;
        }
    }
    return out;
}
struct Matches { // (eight in place, the rest on the heap: the short strings make a hundred million of these)
    uint32_t n = 0;
    uint32_t few[8];
    std::vector<uint32_t> more;
    void push_back(uint32_t p) {
        if (n < 8) few[n] = p;
        else more.push_back(p);
        ++n;
    }
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    uint32_t operator[](uint32_t k) const { return k < 8 ? few[k] : more[k - 8]; }
    bool operator==(const Matches &o) const {
        if (n != o.n) return false;
        for (uint32_t k = 0; k < n; ++k)
            if ((*this)[k] != o[k]) return false;
        return true;
    }
};
static Matches ref_matches(const uint8_t *s, uint32_t len, const Bytes &from) {
    Matches at;
    const uint32_t m = uint32_t(from.size());
    if (m == 0) return at;
    for (uint32_t i = 0; i + m <= len;) {
        if (std::memcmp(s + i, from.data(), m) == 0) {
            at.push_back(i);
            i += m;
        } else
            ++i;
    }
    return at;
}
static Bytes ref_replace(const uint8_t *s, uint32_t len, const Matches &at, uint32_t m, const Bytes &to) {
    Bytes out;
    uint32_t i = 0;
    for (uint32_t k = 0; k < at.n; ++k) {
        const uint32_t a = at[k];
        out.insert(out.end(), s + i, s + a);
        out.insert(out.end(), to.begin(), to.end());
        i = a + m;
    }
    out.insert(out.end(), s + i, s + len);
    return out;
}

// ---- the walks, lane by lane as the kernels take them (G lanes; the loops over `lane` are what a group does at once)
// str_substr_bounds: chunks of G words; returns the chunks read
static uint32_t walk_substr(const uint8_t *p, uint32_t len, int64_t start, int64_t count, uint32_t G, uint32_t *first, uint32_t *end) {
    uint64_t lo = 0, hi = 0;
    *first = *end = 0;
    if (!substr_window(start, count, &lo, &hi) || len == 0) return 0;
    uint32_t pos_lo = 0xFFFFFFFFu, pos_hi = 0xFFFFFFFFu, chunks = 0;
    uint64_t before = 0;
    bool more = true;
    for (uint32_t c0 = 0; more; c0 += 8 * G) {
        ++chunks;
        uint64_t prefix = 0; // the ordered prefix over the lanes
        for (uint32_t lane = 0; lane < G; ++lane) {
            const uint32_t b0 = c0 + 8 * lane;
            uint64_t mask = 0;
            if (b0 >= len + 8) break; // (the lanes further behind the end see the same empty mask: skipped to keep the test quick)
            if (b0 < len) {
                const uint32_t left = len - b0;
                uint64_t w;
                if (left >= 8) std::memcpy(&w, p + b0, 8);
                else w = tail_word(p + b0, left);
                mask = nqe::strfn::noncontinuation_mask(w);
            }
            const uint64_t mine = before + prefix;
            uint32_t k = kth_in_word(mask, mine, lo);
            if (k < 8 && b0 + k < pos_lo) pos_lo = b0 + k;
            k = kth_in_word(mask, mine, hi);
            if (k < 8 && b0 + k < pos_hi) pos_hi = b0 + k;
            prefix += uint64_t(__builtin_popcountll(mask));
        }
        before += prefix;
        more = before < hi && uint64_t(c0) + 8 * G < len;
    }
    substr_combine(lo, pos_lo < len ? pos_lo : len, pos_hi < len ? pos_hi : len, first, end);
    return chunks;
}
// the replace kernels' walk: chunks of G positions; the matches found, and (when `out`) every byte and every copy of `to` placed
static Matches walk_replace(const uint8_t *p, uint32_t len, const Bytes &from, const Bytes &to, uint32_t G, bool bordered, Bytes *out, bool same_length) {
    const uint32_t m = uint32_t(from.size()), t = uint32_t(to.size());
    Matches at;
    uint32_t next_free = 0;
    uint64_t matches = 0;
    for (uint32_t c0 = 0; c0 < len; c0 += G) {
        uint64_t cand = 0;
        for (uint32_t lane = 0; lane < G && c0 + lane <= len; ++lane) // (one lane behind the end, which must see no candidate; the others are the same)
            if (is_candidate(p, len, c0 + lane, from.data(), m)) cand |= 1ull << lane;
        const uint32_t nf_before = next_free;
        const uint64_t taken = resolve_matches(cand, c0, m, bordered, &next_free);
        for (uint32_t lane = 0; lane < G; ++lane) {
            const uint32_t i = c0 + lane;
            if (i >= len) break;
            if ((taken >> lane) & 1) at.push_back(i);
            if (!out) continue;
            const Placement pl = place_byte(taken, c0, lane, same_length ? 0 : matches, nf_before, m, same_length ? m : t);
            if (same_length) {
                (*out)[i] = pl.is_start ? to[0] : pl.covered ? to[pl.within] : p[i];
            } else if (pl.is_start) {
                for (uint32_t k = 0; k < t; ++k) {
                    CHECK(pl.out + k < out->size());
                    if (pl.out + k < out->size()) (*out)[size_t(pl.out) + k] = to[k];
                }
            } else if (!pl.covered) {
                CHECK(pl.out < out->size());
                if (pl.out < out->size()) (*out)[size_t(pl.out)] = p[i];
            }
        }
        matches += uint64_t(__builtin_popcountll(taken));
    }
    return at;
}

// ---- every `from` of up to 3 bytes
static std::vector<Bytes> all_patterns() {
    std::vector<Bytes> out;
    for (int n = 1; n <= 3; ++n) {
        int total = 1;
        for (int k = 0; k < n; ++k) total *= 6;
        for (int code = 0; code < total; ++code) {
            Bytes f;
            for (int k = 0, c = code; k < n; ++k, c /= 6) f.push_back(ALPHABET[c % 6]);
            out.push_back(f);
        }
    }
    return out;
}
static const std::vector<Bytes> PATTERNS = all_patterns();
static std::vector<std::atomic<char>> overlap_seen(PATTERNS.size());
static const Bytes TOS[3] = {Bytes{}, Bytes{'x'}, Bytes{'x', 'y', 'z'}};

static void check_substr(const uint8_t *p, uint32_t len) {
    for (int64_t start : STARTS)
        for (int64_t count : COUNTS) {
            bool contiguous;
            const Bytes &ref = ref_substr(p, len, start, count, &contiguous);
            CHECK(contiguous);
            uint32_t first, end;
            substr_range(p, len, start, count, &first, &end);
            CHECK(first <= end && end <= len && end - first == ref.size() && same_bytes(p + first, ref));
            for (uint32_t G : {4u, 64u}) {
                walk_substr(p, len, start, count, G, &first, &end);
                CHECK(first <= end && end <= len && end - first == ref.size() && same_bytes(p + first, ref));
            }
        }
}

static void check_replace(const uint8_t *p, uint32_t len, bool all_group_sizes) {
    for (size_t f = 0; f < PATTERNS.size(); ++f) {
        const Bytes &from = PATTERNS[f];
        const uint32_t m = uint32_t(from.size());
        const bool bordered = has_border(from.data(), m);
        const Matches ref_at = ref_matches(p, len, from);
        // two occurrences that overlap, anywhere in this string?
        for (uint32_t i = 0; i + m <= len && !overlap_seen[f]; ++i)
            for (uint32_t d = 1; d < m && i + d + m <= len; ++d)
                if (is_candidate(p, len, i, from.data(), m) && is_candidate(p, len, i + d, from.data(), m)) overlap_seen[f] = 1;
        for (uint32_t G : {4u, 8u, 16u, 32u, 64u}) {
            if (!all_group_sizes && G != 4u && G != 64u) continue;
            CHECK(walk_replace(p, len, from, TOS[0], G, bordered, nullptr, false) == ref_at);
            if (ref_at.empty() && len <= 7) continue; // (nothing is replaced: the placement is the identity — checked on the random strings)
            for (const Bytes &to : TOS) {
                const Bytes ref = ref_replace(p, len, ref_at, m, to);
                CHECK(replaced_length(len, ref_at.size(), m, uint32_t(to.size())) == ref.size());
                Bytes out(ref.size(), 0xEE);
                walk_replace(p, len, from, to, G, bordered, &out, false);
                CHECK(out == ref);
            }
            // |to| == |from|: every byte is written where it was read
            Bytes same_to(m);
            for (uint32_t k = 0; k < m; ++k) same_to[k] = uint8_t('1' + k);
            Bytes out(len, 0xEE);
            walk_replace(p, len, from, same_to, G, bordered, &out, true);
            CHECK(out == ref_replace(p, len, ref_at, m, same_to));
        }
    }
}

static std::atomic<uint64_t> strings_checked{0};
static void check_string(const Bytes &s, bool all_group_sizes) {
    const uint32_t len = uint32_t(s.size());
    // the functions must not read outside [0, len): the string sits between guard bytes that would change the answers if read — 'A's (a
    // character each; an occurrence of "A", "AA" or "AAA" across the end)
    Bytes guarded(len + 16, 'A');
    if (len) std::memcpy(guarded.data() + 8, s.data(), len);
    const uint8_t *p = guarded.data() + 8;
    check_substr(p, len);
    check_replace(p, len, all_group_sizes);
    ++strings_checked;
}

// (the strings are dealt out to a few threads: a third of a million strings x 258 patterns is half a minute on one)
static void test_every_short_string(int max_len) {
    const int workers = 8;
    std::vector<std::thread> pool;
    for (int w = 0; w < workers; ++w)
        pool.emplace_back([=]() {
            for (int n = 0; n <= max_len; ++n) {
                int total = 1;
                for (int k = 0; k < n; ++k) total *= 6;
                for (int code = w; code < total; code += workers) {
                    Bytes s;
                    for (int k = 0, c = code; k < n; ++k, c /= 6) s.push_back(ALPHABET[c % 6]);
                    check_string(s, false);
                }
            }
        });
    for (std::thread &t : pool) t.join();
    // has_border against what the strings showed: a pattern has a border iff two of its occurrences can overlap (a string of 2m - 1 <= 5 bytes shows it)
    if (max_len >= 5)
        for (size_t f = 0; f < PATTERNS.size(); ++f) CHECK(has_border(PATTERNS[f].data(), uint32_t(PATTERNS[f].size())) == (overlap_seen[f] != 0));
    CHECK(has_border((const uint8_t *)"aa", 2) && has_border((const uint8_t *)"aba", 3) && has_border((const uint8_t *)"abcab", 5));
    CHECK(!has_border((const uint8_t *)"a", 1) && !has_border((const uint8_t *)"ab", 2) && !has_border((const uint8_t *)"aab", 3) && !has_border((const uint8_t *)"abcd", 4));
}

// strings of several chunks for every group size, from the same alphabet with runs that make bordered patterns overlap
static void test_longer_strings() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int round = 0; round < 60; ++round) {
        const uint32_t len = uint32_t(next() % 700);
        Bytes s(len);
        for (uint32_t i = 0; i < len; ++i) s[i] = (next() % 3) ? ALPHABET[1 + (round % 2) * 2] : ALPHABET[next() % 6]; // mostly 'A' (or 0xC3)
        check_string(s, true);
        // the walk stops at the chunk that holds the window's end
        Bytes guarded(len + 16, 'A');
        if (len) std::memcpy(guarded.data() + 8, s.data(), len);
        for (uint32_t G : {4u, 8u, 16u, 32u, 64u}) {
            uint32_t first, end;
            for (int64_t start : {int64_t(1), int64_t(3), int64_t(40), int64_t(-5), int64_t(600)})
                for (int64_t count : {int64_t(2), int64_t(100), INT64_MAX, int64_t(0)}) {
                    bool contiguous;
                    const Bytes &ref = ref_substr(guarded.data() + 8, len, start, count, &contiguous);
                    const uint32_t chunks = walk_substr(guarded.data() + 8, len, start, count, G, &first, &end);
                    CHECK(contiguous && end - first == ref.size() && same_bytes(guarded.data() + 8 + first, ref));
                    // no chunk behind the one with the window's end byte (one more only when that byte is the next chunk's first)
                    if (count > 0 && count != INT64_MAX && len) CHECK(chunks <= end / (8 * G) + 1);
                }
        }
    }
    // "aa" over "a" * (2G + 1) and "aba" over "ababab...": the greedy carry across chunks
    for (uint32_t G : {4u, 8u, 16u, 32u, 64u}) {
        check_string(Bytes(2 * G + 1, 'A'), true);
        Bytes ab;
        for (uint32_t i = 0; i < 3 * G + 2; ++i) ab.push_back(i % 2 ? 'z' : 'A');
        check_string(ab, true);
    }
}

static void test_saturating_lengths() {
    const uint64_t I31 = 0x7FFFFFFFull;
    CHECK(repeat_length(1, int64_t(I31)) == I31 && repeat_length(1, int64_t(I31) + 1) == I31 + 1);
    CHECK(repeat_length(1024, 1 << 21) == I31 + 1 && repeat_length(1024, (1 << 21) - 1) == I31 + 1 - 1024);
    CHECK(repeat_length(7, 306783378) == 2147483646ull && repeat_length(7, 306783379) == 2147483653ull);
    CHECK(repeat_length(1024, int64_t(1) << 62) == ROW_CAP && repeat_length(1, int64_t(1) << 62) == ROW_CAP && repeat_length(1, INT64_MAX) == ROW_CAP);
    CHECK(repeat_length(uint32_t(I31), INT64_MAX) == ROW_CAP && repeat_length(uint32_t(I31), 2) == 2 * I31 && repeat_length(uint32_t(I31), 3) == ROW_CAP);
    CHECK(repeat_length(0, INT64_MAX) == 0 && repeat_length(5, 0) == 0 && repeat_length(5, -1) == 0 && repeat_length(5, INT64_MIN) == 0 && repeat_length(5, 1) == 5);
    CHECK(ROW_CAP > MAX_TOTAL && MAX_TOTAL == I31);
    CHECK(replaced_length(600, 600, 1, 4096) == 600ull * 4096 && replaced_length(600, 0, 1, 4096) == 600 && replaced_length(600, 600, 1, 0) == 0);
    CHECK(replaced_length(uint32_t(I31), I31, 1, uint32_t(I31)) == ROW_CAP && replaced_length(6, 2, 3, 1) == 2);
    uint64_t lo, hi;
    CHECK(substr_window(1, 2, &lo, &hi) && lo == 1 && hi == 3);
    CHECK(substr_window(-3, 5, &lo, &hi) && lo == 1 && hi == 2);
    CHECK(!substr_window(-3, 4, &lo, &hi) && !substr_window(5, 0, &lo, &hi) && !substr_window(5, -1, &lo, &hi) && !substr_window(INT64_MIN, INT64_MAX, &lo, &hi));
    CHECK(substr_window(INT64_MAX, INT64_MAX, &lo, &hi) && lo == uint64_t(INT64_MAX) && hi == uint64_t(INT64_MAX)); // saturated: no character number lies in it
    CHECK(substr_window(3, INT64_MAX, &lo, &hi) && lo == 3 && hi == uint64_t(INT64_MAX));
    CHECK(substr_window(INT64_MIN, INT64_MAX, &lo, &hi) == false);
    CHECK(substr_window(INT64_MIN + 3, INT64_MAX, &lo, &hi) && lo == 1 && hi == 2);
}

int main(int argc, char **argv) {
    const int max_len = argc > 1 ? std::atoi(argv[1]) : 7;
    test_saturating_lengths();
    test_longer_strings();
    test_every_short_string(max_len);
    if (failures) {
        std::printf("%d checks failed\n", failures.load());
        return 1;
    }
    std::printf("string args ok: %llu strings\n", (unsigned long long)strings_checked.load());
    return 0;
}
