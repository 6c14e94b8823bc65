// group_keys_kernels.hpp — the device side of GROUP BY on several keys (quirk Q20; the host side and the design are in group_keys.hip):
//
//   group_keys_ranges   min / max of every integer key column over its valid rows, as order words (word ^ sign flip for Int64)
//   group_keys_pack     code = sum (key_i - min_i) * stride_i per row, validity = AND of the keys' validity words
//   group_keys_decode   the G group codes back into k key columns
//   group_keys_dict     the tuple dictionary: code = representative row of the row's key tuple (open addressing, exact)
//
// The ranges and pack kernels are pure streaming: where every pointer is 16-byte aligned (VEC) a lane loads two rows at once, and
// several loads are in flight per lane before the first is used.
#pragma once

#include "device_utils.hpp"
#include "group_keys_plan.hpp"
#include "utf8_bytes.hpp"

namespace nqe {

namespace {

constexpr int GK_THREADS = 256;
constexpr int GK_UNROLL = 4; // loads in flight per lane and column in the ranges kernel

struct GkCols { // the integer key columns of the packed path
    const uint64_t *words[gk::MAX_KEYS];
    const uint8_t *valid[gk::MAX_KEYS]; // null: no NULLs
    uint64_t flip[gk::MAX_KEYS];        // order flip (ranges kernel)
    int32_t k;
    int32_t any_valid; // some key column has a validity bitmap
    int64_t n;
};

// 64 validity bits from bit 64 j of a bitmap of `nbytes` bytes that may be borrowed: nothing beyond its last byte is read
__device__ __forceinline__ uint64_t gk_valid_word(const uint8_t *v, int64_t j, int64_t nbytes) {
    const int64_t b = j * 8;
    if (b + 8 <= nbytes) return load_u64_unaligned(v + b);
    return b < nbytes ? tail_word(v + b, int32_t(nbytes - b)) : 0;
}

// validity of the code column, whole words: the AND of the keys' validity words, zero beyond row n
template <typename ValidOf>
__device__ __forceinline__ void gk_and_validity(ValidOf valid_of, int k, int64_t n, uint64_t *out) {
    const int64_t nwords = (n + 63) >> 6, nbytes = (n + 7) >> 3, stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < nwords; j += stride) {
        uint64_t w = ~0ull;
        for (int c = 0; c < k; ++c) {
            const uint8_t *v = valid_of(c);
            if (v) w &= gk_valid_word(v, j, nbytes);
        }
        const int64_t rest = n - j * 64;
        if (rest < 64) w &= (1ull << rest) - 1ull;
        out[j] = w;
    }
}

__device__ __forceinline__ void gk_minmax(uint64_t x, bool ok, uint64_t &lo, uint64_t &hi) {
    if (ok) {
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
    }
}

// out[2c] = min, out[2c + 1] = max of the order words of key c over its valid rows (initialised to ~0 / 0 by the host: a column without
// a valid row leaves min > max).  One pass over the k columns; per column a block reduction, then one 64-bit atomic min / max per block.
template <bool VEC> __global__ void __launch_bounds__(GK_THREADS) group_keys_ranges_kernel(GkCols a, unsigned long long *out) {
    __shared__ uint64_t s_lo[GK_THREADS / WAVE], s_hi[GK_THREADS / WAVE];
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int c = 0; c < a.k; ++c) {
        const uint64_t *w = a.words[c];
        const uint8_t *v = a.valid[c];
        const uint64_t flip = a.flip[c];
        uint64_t lo = ~0ull, hi = 0;
        if (VEC) {
            const ulonglong2 *w2 = reinterpret_cast<const ulonglong2 *>(w);
            const int64_t npairs = a.n >> 1;
            for (int64_t p = tid; p < npairs; p += stride * GK_UNROLL) {
                ulonglong2 x[GK_UNROLL];
                uint32_t bits[GK_UNROLL];
#pragma unroll
                for (int u = 0; u < GK_UNROLL; ++u) {
                    const int64_t q = p + u * stride;
                    const bool in = q < npairs;
                    x[u] = in ? w2[q] : make_ulonglong2(0, 0);
                    bits[u] = !in ? 0u : v ? (uint32_t(v[q >> 2]) >> ((q & 3) * 2)) & 3u : 3u; // rows 2q, 2q + 1 share a byte
                }
#pragma unroll
                for (int u = 0; u < GK_UNROLL; ++u) {
                    gk_minmax(x[u].x ^ flip, bits[u] & 1u, lo, hi);
                    gk_minmax(x[u].y ^ flip, bits[u] & 2u, lo, hi);
                }
            }
            if ((a.n & 1) && tid == 0) gk_minmax(w[a.n - 1] ^ flip, !v || get_bit(v, a.n - 1), lo, hi);
        } else {
            for (int64_t r = tid; r < a.n; r += stride * GK_UNROLL) {
                uint64_t x[GK_UNROLL];
                bool ok[GK_UNROLL];
#pragma unroll
                for (int u = 0; u < GK_UNROLL; ++u) {
                    const int64_t q = r + u * stride;
                    const bool in = q < a.n;
                    x[u] = in ? w[q] : 0;
                    ok[u] = in && (!v || get_bit(v, q));
                }
#pragma unroll
                for (int u = 0; u < GK_UNROLL; ++u) gk_minmax(x[u] ^ flip, ok[u], lo, hi);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t l2 = __shfl_xor((unsigned long long)lo, o, 64), h2 = __shfl_xor((unsigned long long)hi, o, 64);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if (lane_id() == 0) {
            s_lo[threadIdx.x / WAVE] = lo;
            s_hi[threadIdx.x / WAVE] = hi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < GK_THREADS / WAVE; ++i) {
                lo = s_lo[i] < lo ? s_lo[i] : lo;
                hi = s_hi[i] > hi ? s_hi[i] : hi;
            }
            if (lo <= hi) {
                atomicMin(&out[2 * c], (unsigned long long)lo);
                atomicMax(&out[2 * c + 1], (unsigned long long)hi);
            }
        }
        __syncthreads();
    }
}

struct GkPack {
    GkCols c;
    uint64_t min[gk::MAX_KEYS], stride[gk::MAX_KEYS];
    uint64_t *codes;     // [n]
    uint64_t *valid_out; // [(n + 63) / 64] words; null when no key column has a validity bitmap
};

// the validity bits of rows 2q, 2q + 1 over every key
template <int K> __device__ __forceinline__ uint32_t gk_pair_bits(const GkCols &c, int64_t q) {
    uint32_t bits = 3u;
#pragma unroll
    for (int i = 0; i < K; ++i)
        if (c.valid[i]) bits &= uint32_t(c.valid[i][q >> 2]) >> ((q & 3) * 2);
    return bits;
}

// One read of the K columns, one write of the codes.  A row with a NULL key gets code 0 (inside the code range: whatever sits in a NULL
// slot never reaches the aggregate's tables).  K is a template parameter so that the K loads of a row are issued together.
template <int K, bool VEC> __global__ void __launch_bounds__(GK_THREADS) group_keys_pack_kernel(GkPack a) {
    const GkCols &c = a.c;
    if (a.valid_out) gk_and_validity([&](int i) { return c.valid[i]; }, K, c.n, a.valid_out);
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (VEC) {
        const int64_t npairs = c.n >> 1;
        ulonglong2 *out2 = reinterpret_cast<ulonglong2 *>(a.codes);
        for (int64_t p = tid; p < npairs; p += stride * 2) {
            const int64_t q1 = p + stride;
            const bool in1 = q1 < npairs;
            ulonglong2 x0[K], x1[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const ulonglong2 *w2 = reinterpret_cast<const ulonglong2 *>(c.words[i]);
                x0[i] = w2[p];
                x1[i] = in1 ? w2[q1] : make_ulonglong2(0, 0);
            }
            ulonglong2 r0 = make_ulonglong2(0, 0), r1 = make_ulonglong2(0, 0);
#pragma unroll
            for (int i = 0; i < K; ++i) {
                r0.x += gk::pack_digit(x0[i].x, a.min[i], a.stride[i]);
                r0.y += gk::pack_digit(x0[i].y, a.min[i], a.stride[i]);
                r1.x += gk::pack_digit(x1[i].x, a.min[i], a.stride[i]);
                r1.y += gk::pack_digit(x1[i].y, a.min[i], a.stride[i]);
            }
            if (c.any_valid) {
                const uint32_t b0 = gk_pair_bits<K>(c, p), b1 = in1 ? gk_pair_bits<K>(c, q1) : 0u;
                r0.x = (b0 & 1u) ? r0.x : 0;
                r0.y = (b0 & 2u) ? r0.y : 0;
                r1.x = (b1 & 1u) ? r1.x : 0;
                r1.y = (b1 & 2u) ? r1.y : 0;
            }
            out2[p] = r0;
            if (in1) out2[q1] = r1;
        }
    }
    // every row without the pairs; with them the last row of an odd count
    for (int64_t r = VEC ? ((c.n & ~int64_t(1)) + tid) : tid; r < c.n; r += stride) {
        uint64_t code = 0;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            code += gk::pack_digit(c.words[i][r], a.min[i], a.stride[i]);
            if (c.valid[i]) ok = ok && get_bit(c.valid[i], r);
        }
        a.codes[r] = ok ? code : 0;
    }
}

struct GkDecode {
    const uint64_t *codes; // [g]
    int64_t g;
    int32_t k;
    uint64_t min[gk::MAX_KEYS], span[gk::MAX_KEYS], stride[gk::MAX_KEYS];
    uint64_t *out[gk::MAX_KEYS]; // [g] each
};

__global__ void __launch_bounds__(GK_THREADS) group_keys_decode_kernel(GkDecode a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.g; i += stride) {
        const uint64_t code = a.codes[i];
        for (int c = 0; c < a.k; ++c) a.out[c][i] = gk::decode_digit(code, a.min[c], a.span[c], a.stride[c]);
    }
}

struct GkDictKey {
    const uint64_t *words; // Int64 / UInt64
    const int32_t *offs;   // Utf8 (non-null selects the string form)
    const uint8_t *data;
    const uint8_t *valid;  // null: no NULLs
};
struct GkDict {
    GkDictKey key[gk::MAX_KEYS];
    int32_t k;
    int32_t any_valid;
    int64_t n;
    long long *slots; // [cap] representative row, -1 = empty
    uint32_t cap;     // power of two >= 2 n
    int32_t shift;
    int64_t *codes;      // [n]
    uint64_t *valid_out; // as GkPack
};

constexpr uint64_t GK_GOLD = 0x9E3779B97F4A7C15ull;
constexpr long long GK_EMPTY = -1;

// code[i] = the representative row of row i's key tuple: the first row to claim the tuple's slot.  Modelled on utf8_encode_kernel<true>
// (strings.hip): a slot holds a row number, a hit on an occupied slot compares every key with the representative's — 64-bit words, and
// the bytes of a Utf8 key — so the encoding is exact; the probe loop ends after `cap` steps at the latest (cap >= 2 n: it never gets
// there).  A row with a NULL key takes no slot; its code is 0 under a cleared validity bit.
__global__ void __launch_bounds__(GK_THREADS) group_keys_dict_kernel(GkDict a) {
    if (a.valid_out) gk_and_validity([&](int i) { return a.key[i].valid; }, a.k, a.n, a.valid_out);
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        bool ok = true;
        if (a.any_valid)
            for (int c = 0; c < a.k; ++c)
                if (a.key[c].valid) ok = ok && get_bit(a.key[c].valid, i);
        if (!ok) {
            a.codes[i] = 0;
            continue;
        }
        uint64_t h = GK_GOLD;
        for (int c = 0; c < a.k; ++c) {
            const GkDictKey &kc = a.key[c];
            uint64_t w;
            if (kc.offs) {
                const int32_t o = kc.offs[i];
                w = fnv1a64(kc.data + o, kc.offs[i + 1] - o);
            } else
                w = kc.words[i];
            h = mix64(h ^ w); // (mixed per key: (1, 2) and (2, 1) part ways)
        }
        uint32_t slot = uint32_t((h * GK_GOLD) >> a.shift);
        int64_t code = i;
        for (uint32_t probe = 0; probe < a.cap; ++probe) {
            long long cur = __hip_atomic_load(&a.slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == GK_EMPTY) {
                const long long old = (long long)atomicCAS((unsigned long long *)&a.slots[slot], (unsigned long long)GK_EMPTY, (unsigned long long)i);
                if (old == GK_EMPTY) break; // this row is the representative
                cur = old;
            }
            bool same = true;
            for (int c = 0; c < a.k && same; ++c) {
                const GkDictKey &kc = a.key[c];
                if (kc.offs) {
                    const int32_t o = kc.offs[i], len = kc.offs[i + 1] - o, co = kc.offs[cur], clen = kc.offs[cur + 1] - co;
                    same = clen == len && bytes_equal(kc.data + co, kc.data + o, len);
                } else
                    same = kc.words[cur] == kc.words[i];
            }
            if (same) {
                code = cur;
                break;
            }
            slot = (slot + 1) & (a.cap - 1);
        }
        a.codes[i] = code;
    }
}

__global__ void __launch_bounds__(GK_THREADS) group_keys_fill_kernel(long long *p, long long v, int64_t n) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

} // namespace

} // namespace nqe
