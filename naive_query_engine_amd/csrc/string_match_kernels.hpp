// string_match_kernels.hpp — the kernels of string matching (quirk Q27: NQE_EXPR_STRING_MATCH), gfx950, wave 64, grid-stride.  What they
// compute per string is string_match_parts.hpp's; here is only how the work is spread over lanes and how the one BIT per row is stored:
// a wave owns 64 consecutive rows and one of its lanes stores their whole 64-bit value word — no atomic, no zero-fill, the bits behind
// the last row zero.  Validity is read (a NULL row's bit is 0, for the NOT forms too) and never written: the result carries the operand's.
//
//   str_match_anchor<FOLD>         EQUAL / PREFIX / SUFFIX / PREFIX_SUFFIX: a lane per row, 64 rows per step, one ballot.  The length test
//                                  first, then at most |prefix| + |suffix| bytes, 8 at a time; a prefix or suffix of at most 8 bytes is
//                                  one masked word that came with the kernel's arguments.
//   str_match_scan<LG, FOLD, POS>  CONTAINS / GENERAL / STRPOS: 2^LG lanes per string.  The anchored segments are walked by every lane of
//                                  the group alike; every other segment is searched for in chunks of candidate positions from the cursor,
//                                  the group's ballot giving the leftmost one, and the group stops at the chunk that decides the row.  A
//                                  segment of at most 8 literal bytes is one masked word: a lane loads two words of the string and tests 8
//                                  positions, a chunk is 8 * G positions.  Any other segment (ONE, longer): a position per lane, the walk
//                                  of string_match_parts.hpp, a chunk is G positions.  A wave takes its 64 rows in 2^LG steps of 64 >> LG and collects the row
//                                  bits before the one store.  POS (STRPOS): the non-continuation bytes up to the match are counted by the
//                                  group, 8 bytes per lane and step, and one lane per row writes the Int64.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_utils.hpp"
#include "string_args_kernels.hpp"
#include "string_match_parts.hpp"

namespace nqe {
namespace {

// a prefix and a suffix without ONE; the literal's bytes are `lit` (prefix, then suffix), and the first 8 of each came as words
struct StrAnchors {
    const uint8_t *lit;
    uint64_t pre_word, suf_word;
    uint32_t pre, suf;
    int32_t exact, negate; // exact: the string IS the prefix (EQUAL)
};

// the first `want` (1-8) bytes at p, the bytes above them zero; `avail` >= want bytes of the string lie at p
template <bool FOLD> __device__ __forceinline__ uint64_t str_low_bytes(const uint8_t *p, uint32_t want, uint32_t avail) {
    uint64_t w = avail >= 8 ? *reinterpret_cast<const str_u64_unaligned *>(p) : strargs::tail_word(p, want);
    if constexpr (FOLD) w = strfn::case_word(w, false);
    return want >= 8 ? w : w & ((1ull << (8 * want)) - 1ull);
}
// the 8 bytes of the string at byte i < len, the bytes behind its end continuation bytes (strargs::tail_word): nothing behind the string is read
template <bool FOLD> __device__ __forceinline__ uint64_t str_word_at(const uint8_t *p, uint32_t len, uint32_t i) {
    const uint32_t left = len - i;
    uint64_t w = left >= 8 ? *reinterpret_cast<const str_u64_unaligned *>(p + i) : strargs::tail_word(p + i, left);
    if constexpr (FOLD) w = strfn::case_word(w, false);
    return w;
}
// are the m bytes at p (of which `avail` >= m belong to the string) the literal's?  `word`: the literal's first min(m, 8) bytes
template <bool FOLD> __device__ __forceinline__ bool str_equals_literal(const uint8_t *p, uint32_t m, uint32_t avail, const uint8_t *lit, uint64_t word) {
    if (m <= 8) return m == 0 || str_low_bytes<FOLD>(p, m, avail) == word;
    for (uint32_t k = 0; k < m; k += 8) { // (the literal's buffer is padded: whole words may be read from it)
        const uint32_t left = m - k < 8 ? m - k : 8;
        uint64_t l = *reinterpret_cast<const str_u64_unaligned *>(lit + k);
        if (left < 8) l &= (1ull << (8 * left)) - 1ull;
        if (str_low_bytes<FOLD>(p + k, left, avail - k) != l) return false;
    }
    return true;
}

template <bool FOLD>
__global__ void __launch_bounds__(256) str_match_anchor_kernel(const int32_t *off, const uint8_t *src, const uint8_t *s_valid, StrAnchors a, int64_t n, uint64_t *out_bits) {
    const int64_t n_pad = (n + 63) / 64 * 64;
    for (int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; row < n_pad; row += int64_t(gridDim.x) * blockDim.x) { // (whole waves: 256 | stride)
        bool r = false;
        if (row < n && str_bit_at(s_valid, row)) {
            const int32_t so = off[row];
            const uint32_t len = uint32_t(off[row + 1] - so);
            bool hit = a.exact ? len == a.pre : len >= a.pre + a.suf;
            if (hit) {
                const uint8_t *p = src + so;
                hit = str_equals_literal<FOLD>(p, a.pre, len, a.lit, a.pre_word) && str_equals_literal<FOLD>(p + (len - a.suf), a.suf, a.suf, a.lit + a.pre, a.suf_word);
            }
            r = hit != (a.negate != 0);
        }
        const uint64_t wb = __ballot(r);
        if (lane_id() == 0) out_bits[row >> 6] = wb;
    }
}

template <int LG, bool FOLD, bool POS>
__global__ void __launch_bounds__(256) str_match_scan_kernel(const int32_t *off, const uint8_t *src, const uint8_t *s_valid, strmatch::Pattern P, int64_t n, uint64_t *out_bits,
                                                              int64_t *out_pos) {
    constexpr int G = 1 << LG, PER_WAVE = 64 >> LG;
    const int64_t waves = (int64_t(gridDim.x) * blockDim.x) >> 6, wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = uint32_t(lane_id()), sub = lane & uint32_t(G - 1), grp = lane >> LG;
    const int64_t blocks = (n + 63) >> 6;
    // A searched segment stays in registers until it is found: a segment of at most 8 literal bytes as ONE masked word, which a lane
    // compares at 8 positions out of the two words it loads.  The first segment any row searches for is the same for all rows and is
    // taken once, before the rows.
    struct Searched {
        strmatch::SegView seg;
        uint64_t word, mask;
        bool as_word;
    };
    auto segment = [&](uint32_t k) {
        Searched s{P.segs[k], 0, 0, false};
        s.as_word = strmatch::is_word_segment(s.seg.len, s.seg.ones);
        if (s.as_word) { // (the pattern's buffer is padded: a whole word may be read at any of its elements)
            s.mask = strmatch::word_mask(s.seg.len);
            s.word = *reinterpret_cast<const str_u64_unaligned *>(P.el + s.seg.off) & s.mask;
        }
        return s;
    };
    const uint32_t first_searched = P.anchored_front && P.nseg ? 1u : 0u; // (walk_begin's `first` where a search follows)
    const Searched initial = first_searched < P.nseg ? segment(first_searched) : Searched{{0, 0, 0, 0}, 0, 0, false};
    for (int64_t blk = wave; blk < blocks; blk += waves) { // (blk is the wave's: every lane takes part in the ballots)
        // lane r reads row r's validity bit and offsets — coalesced, once — and every step takes its rows' from the lanes that hold them
        const int64_t mine = (blk << 6) + lane;
        int32_t my_off = 0, my_end = 0;
        int my_live = 0;
        if (mine < n && str_bit_at(s_valid, mine)) {
            my_live = 1;
            my_off = off[mine];
            my_end = off[mine + 1];
        }
        unsigned long long acc = 0; // the group's row bits, bit s = step s
        for (int step = 0; step < G; ++step) {
            const int holder = step * PER_WAVE + int(grp);
            const int64_t j = (blk << 6) + holder;
            const int32_t so = __shfl(my_off, holder, 64), se = __shfl(my_end, holder, 64);
            const bool live = __shfl(my_live, holder, 64) != 0;
            uint32_t len = 0, lead = 0, first = 0, cur = 0, bs = 0, found_at = 0;
            int32_t last = -1;
            const uint8_t *p = src;
            bool hit = false, searching = false;
            if (live) {
                len = uint32_t(se - so);
                p = src + so;
                if (P.has_one) lead = strmatch::leading_continuations(p, len); // (no rule looks at it where the pattern holds no ONE)
                bool decided;
                hit = strmatch::walk_begin<FOLD>(P, p, len, lead, &first, &last, &cur, &bs, &decided);
                searching = hit && !decided;
            }
            uint32_t c0 = cur; // the chunk: candidate positions from c0 for segment `first`
            strmatch::SegView seg = initial.seg;
            uint64_t seg_word = initial.word, seg_mask = initial.mask;
            bool as_word = initial.as_word;
            auto take_segment = [&](uint32_t k) {
                const Searched s = segment(k);
                seg = s.seg;
                seg_word = s.word;
                seg_mask = s.mask;
                as_word = s.as_word;
            };
            while (__any(searching)) {
                int32_t e = -1;      // any other segment: the end of the match at c0 + sub
                uint32_t e_bits = 0; // a word segment: bit k = it occurs at c0 + 8 * sub + k
                if (searching) {
                    if (as_word) { // 8 candidate positions per lane out of two words: the chunk is 8 * G positions
                        const uint32_t i = c0 + 8u * sub;
                        if (i + seg.len <= bs) {
                            const uint64_t w0 = str_word_at<FOLD>(p, len, i), w1 = i + 8 < len ? str_word_at<FOLD>(p, len, i + 8) : 0ull;
                            e_bits = strmatch::word_candidates(w0, w1, seg_word, seg_mask, i, seg.len, bs);
                        }
                    } else {
                        const uint32_t i = c0 + sub;
                        if (i + seg.len <= bs) {
                            e = strmatch::match_at<FOLD>(p, len, lead, i, P.el + seg.off, P.one + seg.off, seg.len, seg.ones != 0);
                            if (e >= 0 && uint32_t(e) > bs) e = -1;
                        }
                    }
                }
                const uint64_t cand = group_ballot<LG>(e >= 0 || e_bits != 0, grp);
                const int b = cand ? __builtin_ctzll(cand) : 0;
                const int32_t end = __shfl(e, b, G);
                const uint32_t bits = __shfl(e_bits, b, G);
                if (searching) {
                    if (cand) { // the leftmost match: on to the next segment, from this match's end
                        found_at = as_word ? c0 + 8u * uint32_t(b) + uint32_t(__builtin_ctz(bits)) : c0 + uint32_t(b);
                        cur = c0 = as_word ? found_at + seg.len : uint32_t(end);
                        if (int32_t(++first) > last) searching = false;
                        else take_segment(first);
                    } else {
                        c0 += as_word ? 8u * G : uint32_t(G);
                        if (c0 + seg.len > bs) { // no room for the segment any more
                            searching = false;
                            hit = false;
                        }
                    }
                }
            }
            if constexpr (POS) {
                // the match's character number: the non-continuation bytes of p[0 .. found_at], at least 1 (an empty `sub`: 1)
                uint32_t count = 0;
                if (hit && P.nseg) {
                    const uint32_t nb = found_at + 1, nw = nb >> 3;
                    for (uint32_t w = sub; w < nw; w += G) count += strfn::noncontinuation_count(*reinterpret_cast<const str_u64_unaligned *>(p + 8 * w));
                    for (uint32_t k = (nw << 3) + sub; k < nb; k += G) count += strfn::is_continuation(p[k]) ? 0u : 1u;
                }
#pragma unroll
                for (int d = G >> 1; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
                if (j < n && sub == 0) out_pos[j] = hit ? int64_t(count ? count : 1u) : 0;
            } else {
                acc |= (unsigned long long)(live && (hit != (P.negate != 0))) << step;
            }
        }
        if constexpr (!POS) {
            // lane r takes row r's bit from the leader of group r % PER_WAVE, where it is bit r / PER_WAVE
            const unsigned long long theirs = __shfl(acc, int((lane & uint32_t(PER_WAVE - 1)) << LG), 64);
            const uint64_t word = __ballot((theirs >> (lane >> (6 - LG))) & 1ull);
            if (lane == 0) out_bits[blk] = word;
        }
    }
}

} // namespace
} // namespace nqe
