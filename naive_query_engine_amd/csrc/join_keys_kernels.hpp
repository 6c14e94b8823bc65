// join_keys_kernels.hpp — the probe side of the join on several keys (quirk Q21; the host side and the design are in join_keys.hip).  The
// build side's codes come from group_keys_pack / group_keys_dict over the build key columns; these kernels put a PROBE row's tuple into
// the same code space:
//
//   join_keys_pack_probe   code = sum (key_i - min_i) * stride_i under the build side's plan, or JOIN_KEYS_NO_MATCH when a key lies
//                          outside its build range
//   join_keys_lookup       find-only walk of the build side's tuple dictionary: the representative build row, or JOIN_KEYS_NO_MATCH
//
// Neither reads a validity buffer: the hash join compares raw slots (quirk Q11).
#pragma once

#include "group_keys_kernels.hpp" // GK_THREADS, GkDictKey, GK_GOLD, GK_EMPTY: the dictionary the lookup walks is group_keys_dict's
#include "join_keys_plan.hpp"

namespace nqe {

namespace {

struct JkPackProbe {
    const uint64_t *words[jk::MAX_KEYS]; // the probe key columns
    uint64_t min[jk::MAX_KEYS], span[jk::MAX_KEYS], stride[jk::MAX_KEYS]; // the BUILD side's plan
    int64_t n;
    uint64_t *codes; // [n]
};

// One read of the K probe key columns (8 K bytes per row), one write of the codes (8 bytes per row).  Shaped as group_keys_pack_kernel:
// K is a template parameter so that the K loads of a row are issued together; with VEC a lane takes two rows per 16-byte load and has
// two such pairs in flight; the last row of an odd count (all rows without VEC) goes through the scalar loop.
template <int K, bool VEC> __global__ void __launch_bounds__(GK_THREADS) join_keys_pack_probe_kernel(JkPackProbe a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    constexpr uint64_t NONE = uint64_t(jk::JOIN_KEYS_NO_MATCH);
    if (VEC) {
        const int64_t npairs = a.n >> 1;
        ulonglong2 *out2 = reinterpret_cast<ulonglong2 *>(a.codes);
        for (int64_t p = tid; p < npairs; p += stride * 2) {
            const int64_t q1 = p + stride;
            const bool in1 = q1 < npairs;
            ulonglong2 x0[K], x1[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const ulonglong2 *w2 = reinterpret_cast<const ulonglong2 *>(a.words[i]);
                x0[i] = w2[p];
                x1[i] = in1 ? w2[q1] : make_ulonglong2(0, 0);
            }
            ulonglong2 r0 = make_ulonglong2(0, 0), r1 = make_ulonglong2(0, 0);
            bool ok0x = true, ok0y = true, ok1x = true, ok1y = true;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                uint64_t d;
                ok0x = jk::probe_digit_in_range(x0[i].x, a.min[i], a.span[i], &d) && ok0x;
                r0.x += d * a.stride[i];
                ok0y = jk::probe_digit_in_range(x0[i].y, a.min[i], a.span[i], &d) && ok0y;
                r0.y += d * a.stride[i];
                ok1x = jk::probe_digit_in_range(x1[i].x, a.min[i], a.span[i], &d) && ok1x;
                r1.x += d * a.stride[i];
                ok1y = jk::probe_digit_in_range(x1[i].y, a.min[i], a.span[i], &d) && ok1y;
                r1.y += d * a.stride[i];
            }
            out2[p] = make_ulonglong2(ok0x ? r0.x : NONE, ok0y ? r0.y : NONE);
            if (in1) out2[q1] = make_ulonglong2(ok1x ? r1.x : NONE, ok1y ? r1.y : NONE);
        }
    }
    // every row without the pairs; with them the last row of an odd count
    for (int64_t r = VEC ? ((a.n & ~int64_t(1)) + tid) : tid; r < a.n; r += stride) {
        uint64_t code = 0;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            uint64_t d;
            ok = jk::probe_digit_in_range(a.words[i][r], a.min[i], a.span[i], &d) && ok;
            code += d * a.stride[i];
        }
        a.codes[r] = ok ? code : NONE;
    }
}

struct JkLookup {
    GkDictKey probe[jk::MAX_KEYS]; // the probe key columns (`valid` unused)
    GkDictKey build[jk::MAX_KEYS]; // the build key columns the dictionary's representatives are rows of
    int32_t k;
    int32_t shift;
    int64_t n;              // probe rows
    const long long *slots; // [cap] representative build row, GK_EMPTY = empty: group_keys_dict's finished table
    uint32_t cap;
    int64_t *codes; // [n]
};

// code[i] = the representative build row of probe row i's tuple, or JOIN_KEYS_NO_MATCH.  The hash and the probe sequence are
// group_keys_dict_kernel's, so the walk passes the slot the build side gave the tuple before it meets an empty one; an occupied slot is
// compared key by key with the BUILD representative — words, and length plus bytes for Utf8 —, so the answer is exact.  The table is
// finished: no atomics, and the walk ends after `cap` steps at the latest (cap >= 2 x build rows: it meets an empty slot long before).
__global__ void __launch_bounds__(GK_THREADS) join_keys_lookup_kernel(JkLookup a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        uint64_t h = GK_GOLD;
        for (int c = 0; c < a.k; ++c) {
            const GkDictKey &kc = a.probe[c];
            uint64_t w;
            if (kc.offs) {
                const int32_t o = kc.offs[i];
                w = fnv1a64(kc.data + o, kc.offs[i + 1] - o);
            } else
                w = kc.words[i];
            h = mix64(h ^ w);
        }
        uint32_t slot = uint32_t((h * GK_GOLD) >> a.shift);
        int64_t code = jk::JOIN_KEYS_NO_MATCH;
        for (uint32_t probe = 0; probe < a.cap; ++probe) {
            const long long cur = __hip_atomic_load(&a.slots[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == GK_EMPTY) break;
            bool same = true;
            for (int c = 0; c < a.k && same; ++c) {
                const GkDictKey &pc = a.probe[c], &bc = a.build[c];
                if (pc.offs) {
                    const int32_t o = pc.offs[i], len = pc.offs[i + 1] - o, bo = bc.offs[cur], blen = bc.offs[cur + 1] - bo;
                    same = blen == len && bytes_equal(bc.data + bo, pc.data + o, len);
                } else
                    same = bc.words[cur] == pc.words[i];
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

} // namespace

} // namespace nqe
