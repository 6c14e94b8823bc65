// utf8_bytes.hpp — hash and equality of short byte strings on the device, shared by the Utf8 dictionary of strings.hip and the tuple
// dictionary of group_keys.hip.
//
// Eight bytes per step (unaligned 8-byte loads: supported for global memory on gfx9 and later; the tail of fewer than eight bytes is
// read byte by byte, so nothing beyond the string is touched).  The hash is unobservable in results (as the reference's XxHash64 is,
// hash_join.rs:68-70): only its spread matters.  Byte-at-a-time FNV-1a made the dictionary encode of 10^7 sixteen-byte keys 1.3 ms.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nqe {

__device__ __forceinline__ uint64_t load_u64_unaligned(const uint8_t *p) {
    typedef uint64_t __attribute__((aligned(1))) u64_unaligned;
    return *reinterpret_cast<const u64_unaligned *>(p);
}
__device__ __forceinline__ uint64_t tail_word(const uint8_t *p, int32_t n) { // n < 8 bytes, little-endian
    uint64_t w = 0;
    for (int32_t i = 0; i < n; ++i) w |= uint64_t(p[i]) << (8 * i);
    return w;
}
__device__ __forceinline__ uint64_t fnv1a64(const uint8_t *p, int32_t len) {
    uint64_t h = 0xcbf29ce484222325ull ^ uint64_t(uint32_t(len));
    int32_t i = 0;
    for (; i + 8 <= len; i += 8) {
        h ^= load_u64_unaligned(p + i);
        h *= 0x9FB21C651E98DF25ull;
        h ^= h >> 29;
    }
    if (i < len) {
        h ^= tail_word(p + i, len - i);
        h *= 0x9FB21C651E98DF25ull;
        h ^= h >> 29;
    }
    return h * 0x100000001b3ull;
}

__device__ __forceinline__ bool bytes_equal(const uint8_t *a, const uint8_t *b, int32_t len) {
    int32_t i = 0;
    for (; i + 8 <= len; i += 8)
        if (load_u64_unaligned(a + i) != load_u64_unaligned(b + i)) return false;
    return i == len || tail_word(a + i, len - i) == tail_word(b + i, len - i);
}

} // namespace nqe
