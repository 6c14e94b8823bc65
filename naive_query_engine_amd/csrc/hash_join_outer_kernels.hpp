// hash_join_outer_kernels.hpp — the device side of the outer hash joins (quirk Q19; included once, by hash_join.hip, after
// hash_join_probe_kernels.hpp): the outer entries of the expand path's two passes — the count pass that keeps unmatched probe rows and
// marks matched build rows, and the output-driven write pass with NULL-extended rows.  Both are instances of the bodies the inner probe
// runs (expand_count / expand_write: the additions are described there); one general path over every build form (lookup_of is
// complete for all of them).  The pass over the build rows that never matched is marked_build_kernel<true> (hash_join_semi_kernels.hpp).
#pragma once
#include "hash_join_probe_kernels.hpp"

namespace nqe {

namespace {

// pass 1 of the outer probe: <false, false> is probe_count_kernel's code
template <bool KEEP_PROBE, bool MARKS>
__global__ void __launch_bounds__(JT_BLOCK) outer_count_kernel(const uint64_t *rkeys, int64_t n, Lookup L, uint64_t *pmeta, uint32_t *tile_counts,
                                                               uint32_t *marks, unsigned long long *misses, int *flags) {
    expand_count<KEEP_PROBE, MARKS>(rkeys, n, L, pmeta, tile_counts, marks, misses, flags);
}

// pass 2 of the outer probe: the load-balanced expansion with NULL-extended rows
template <bool PLAIN>
__global__ void __launch_bounds__(JT_BLOCK) outer_write_kernel(const uint64_t *pmeta, int64_t n, const uint64_t *tile_offsets, const uint32_t *perm, int direct,
                                                               ExpandCols ec) {
    expand_write<PLAIN, true>(pmeta, n, tile_offsets, perm, direct, ec);
}

// set bits among the first n_rows bits of a bitmap of whole 64-bit words, added to *out (one atomic per wave): the exact null count
// of an output column is n_rows minus this
__global__ void __launch_bounds__(256) count_set_bits_kernel(const uint64_t *words, int64_t n_rows, unsigned long long *out) {
    const int64_t nwords = (n_rows + 63) / 64;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long local = 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nwords; i += stride) {
        uint64_t w = words[i];
        if (i == nwords - 1 && (n_rows & 63)) w &= (1ull << (n_rows & 63)) - 1ull;
        local += (unsigned long long)__popcll(w);
    }
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if (lane_id() == 0 && local) atomicAdd(out, local);
}

} // namespace

} // namespace nqe
