// The quoting automaton of the CSV record splitter and its transition vectors (host + device, header only, plain C++).
//
// csv.hip runs csv_step over every 64-byte chunk for all five start states at once, packs the five end states into one
// transition vector (5 x 3 bits) and composes the vectors in three levels (workgroup scan, scan over workgroup totals,
// block prefix with thread prefix).  The same code runs in the CPU unit test (tests/cpp/test_csv_split.cpp), which checks
// that vec_compose is function composition and that any chunking of a byte string ends in the sequential walk's state.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NQE_CSV_HD __host__ __device__ inline
#else
#define NQE_CSV_HD inline
#endif

namespace nqe {
namespace csv_split {

// quoting automaton of one record stream
enum : uint32_t { ST_R = 0 /* record start */, ST_F = 1 /* field start */, ST_U = 2 /* unquoted */, ST_Q = 3 /* quoted */, ST_E = 4 /* quote in quoted */ };
constexpr uint32_t VEC_ID = ST_R | (ST_F << 3) | (ST_U << 6) | (ST_Q << 9) | (ST_E << 12);

NQE_CSV_HD bool is_nl(uint8_t c) { return c == '\n' || c == '\r'; }

// next state; *rec_start: this byte opens a record; *rec_end: this byte (a terminator) closes one
NQE_CSV_HD uint32_t csv_step(uint32_t st, uint8_t c, uint8_t delim, bool *rec_start, bool *rec_end) {
    const bool nl = is_nl(c);
    *rec_start = st == ST_R && !nl;
    *rec_end = nl && (st == ST_F || st == ST_U || st == ST_E);
    switch (st) {
    case ST_R:
    case ST_F: return nl ? ST_R : c == '"' ? ST_Q : c == delim ? ST_F : ST_U;
    case ST_U: return nl ? ST_R : c == delim ? ST_F : ST_U;
    case ST_Q: return c == '"' ? ST_E : ST_Q;
    default: return c == '"' ? ST_Q : nl ? ST_R : c == delim ? ST_F : ST_U; // ST_E
    }
}
NQE_CSV_HD uint32_t vec_get(uint32_t v, uint32_t s) { return (v >> (3 * s)) & 7u; }
// (a then b)
NQE_CSV_HD uint32_t vec_compose(uint32_t a, uint32_t b) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t s = 0; s < 5; ++s) c |= vec_get(b, vec_get(a, s)) << (3 * s);
    return c;
}

} // namespace csv_split
} // namespace nqe
