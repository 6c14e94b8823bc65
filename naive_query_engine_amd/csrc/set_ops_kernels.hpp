// set_ops_kernels.hpp — the device side of DISTINCT and the set operators (quirk Q24; included once, by set_ops.hip; the hash, the
// canonical words and the capacity rule are in set_ops_plan.hpp):
//
//   set_table_init   every slot {representative, first} = {EMPTY, EMPTY}; the marks (INTERSECT / EXCEPT) zero
//   set_insert       every row of the inserted table finds or claims the slot of its tuple, lowers the slot's `first` to its own row
//                    index, and writes the slot index to slot_of[row]
//   set_find         every row of the probed table looks its tuple up and marks the slot on a hit; takes no slot, writes nothing per row
//   set_keep         one bit per inserted row into the selection's keep mask — first[slot_of[i]] == i, AND / AND NOT the slot's mark —
//                    and the per-tile counts
//
// The table is open addressing with linear probing over `cap` slots of 8 bytes: {representative row, first row}, both u32.  The
// representative is whichever row of the tuple wins the compare-and-swap: it is only the row other rows compare their keys with and
// never reaches the result.  `first` is the smallest row index of the tuple, kept with atomicMin: the result does not depend on who
// won, so it is the same on every run.
#pragma once

#include "device_utils.hpp"
#include "set_ops_plan.hpp"

namespace nqe {

namespace {

constexpr int SET_THREADS = 256;

// one key column of one table
struct SetKeyCol {
    const void *values;   // 8-byte words, packed bits (Boolean) or int32 offsets (Utf8)
    const uint8_t *data;  // Utf8 bytes
    const uint8_t *valid; // null: no NULLs.  May be the caller's own memory, ceil(n / 8) bytes: only the byte of a row is read
    int32_t dtype;
    int32_t pad_;
};
struct SetKeys {
    SetKeyCol key[NQE_MAX_SET_KEYS];
};
// the key columns of the WORDS instantiation
struct SetWords {
    const uint64_t *w[setop::MAX_WORD_KEYS];
};
struct SetTable {
    uint32_t *slots; // [2 cap]: slots[2 s] the representative row, slots[2 s + 1] the first row
    uint8_t *marks;  // [cap] (INTERSECT / EXCEPT), else null
    uint32_t mask;   // cap - 1
    int32_t shift;
};

__global__ void __launch_bounds__(SET_THREADS) set_table_init_kernel(unsigned long long *slots, uint64_t cap, unsigned long long *mark_words, uint64_t num_mark_words) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x, tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t s = tid; s < cap; s += stride) slots[s] = ~0ull;
    for (uint64_t s = tid; s < num_mark_words; s += stride) mark_words[s] = 0ull;
}

__device__ __forceinline__ bool set_is_null(const SetKeyCol &kc, int64_t row) { return kc.valid && !get_bit(kc.valid, row); }

// the canonical word of key `kc` at a valid row: what the hash reads
__device__ __forceinline__ uint64_t set_canonical(const SetKeyCol &kc, int64_t row) {
    if (kc.dtype == NQE_UTF8) {
        const int32_t *off = static_cast<const int32_t *>(kc.values);
        const int32_t o = off[row];
        return setop::fnv1a64_bytes(kc.data + o, off[row + 1] - o);
    }
    if (kc.dtype == NQE_BOOLEAN) return get_bit(static_cast<const uint8_t *>(kc.values), row) ? 1ull : 0ull;
    const uint64_t w = static_cast<const uint64_t *>(kc.values)[row];
    return kc.dtype == NQE_FLOAT64 ? setop::canonical_f64(w) : w;
}

__device__ __forceinline__ uint64_t set_hash_row(const SetKeys &a, int num_keys, int64_t row) {
    uint64_t h = setop::hash_start();
    for (int c = 0; c < num_keys; ++c) {
        const SetKeyCol &kc = a.key[c];
        h = setop::hash_step(h, set_is_null(kc, row) ? setop::NULL_TAG : set_canonical(kc, row));
    }
    return h;
}

// Q24's tuple equality of row `i` of table `a` and row `j` of table `b` (the same dtypes at every position).  The validity bits are
// compared first; what lies under a NULL is never read.
__device__ __forceinline__ bool set_rows_equal(const SetKeys &a, int64_t i, const SetKeys &b, int64_t j, int num_keys) {
    for (int c = 0; c < num_keys; ++c) {
        const SetKeyCol &ka = a.key[c], &kb = b.key[c];
        const bool na = set_is_null(ka, i), nb = set_is_null(kb, j);
        if (na != nb) return false;
        if (na) continue;
        if (ka.dtype == NQE_UTF8) {
            const int32_t *oa = static_cast<const int32_t *>(ka.values), *ob = static_cast<const int32_t *>(kb.values);
            const int32_t sa = oa[i], la = oa[i + 1] - sa, sb = ob[j], lb = ob[j + 1] - sb;
            if (la != lb || !setop::bytes_same(ka.data + sa, kb.data + sb, la)) return false;
        } else if (set_canonical(ka, i) != set_canonical(kb, j))
            return false;
    }
    return true;
}

// lowers first[slot] to `row`.  The plain read first: rows are visited in ascending order by every thread, so under heavy duplication
// almost every later row finds a smaller index already there and issues no atomic (a stale read is only ever too large: the atomic
// then runs and changes nothing)
// (-DNQE_SET_NO_FIRST_SKIP, a variant build of tools/build_variant.sh for profiles/set_ops: the atomicMin for every row)
__device__ __forceinline__ void set_lower_first(uint32_t *first, uint32_t row) {
#ifdef NQE_SET_NO_FIRST_SKIP
    atomicMin(first, row);
#else
    if (__hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row) atomicMin(first, row);
#endif
}

// the probe both forms share: true with *slot_out = the slot of the row's tuple — INSERT claims it if nobody had it, so an insert
// always returns true — false when a find-only probe meets an empty slot.  Found and the slot are reported apart: with more than 2^30
// rows cap is 2^32 and EVERY u32, 0xFFFFFFFF included, is a slot index (EMPTY is a sentinel of the ROW values a slot holds, rows being
// fewer than 2^31; it is never a sentinel of slot indices).  `same(rep)`: is the row's tuple the representative's.  Ends after cap
// steps at the latest (cap >= 2 n: an insert never gets there).
template <bool INSERT, typename Same> __device__ __forceinline__ bool set_probe(const SetTable &t, uint64_t h, uint32_t row, Same same, uint32_t *slot_out) {
    uint32_t slot = setop::home_slot(h, t.shift);
    for (uint64_t probe = 0; probe <= uint64_t(t.mask); ++probe) {
        uint32_t cur = __hip_atomic_load(&t.slots[2 * size_t(slot)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == setop::EMPTY) {
            if (!INSERT) return false;
            cur = atomicCAS(&t.slots[2 * size_t(slot)], setop::EMPTY, row);
            if (cur == setop::EMPTY) { // this row is the representative
                *slot_out = slot;
                return true;
            }
        }
        if (same(cur)) {
            *slot_out = slot;
            return true;
        }
        slot = (slot + 1) & t.mask;
    }
    return false;
}

// ---- GENERAL: any key dtypes, NULLs
// `own`: the keys of the rows that probe; `rep`: the keys of the inserted table (INSERT: the same table)
template <bool INSERT>
__global__ void __launch_bounds__(SET_THREADS) set_probe_general_kernel(SetKeys own, SetKeys rep, int32_t num_keys, int64_t n, SetTable t, uint32_t *slot_of) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t h = set_hash_row(own, num_keys, i);
        uint32_t slot = 0;
        const bool found = set_probe<INSERT>(t, h, uint32_t(i), [&](uint32_t r) { return set_rows_equal(own, i, rep, int64_t(r), num_keys); }, &slot);
        if (INSERT) { // (an insert always finds or claims a slot; were it not so, slot_of names slot 0, whose `first` is not this row: dropped)
            if (found) set_lower_first(&t.slots[2 * size_t(slot) + 1], uint32_t(i));
            slot_of[i] = slot;
        } else if (found) {
            t.marks[slot] = 1; // (racing stores of the same byte value)
        }
    }
}

// ---- WORDS: K non-nullable Int64 / UInt64 keys.  K is a template parameter so that the K loads of a row are issued together
// (group_keys_pack_kernel's reason)
template <int K, bool INSERT>
__global__ void __launch_bounds__(SET_THREADS) set_probe_words_kernel(SetWords own, SetWords rep, int64_t n, SetTable t, uint32_t *slot_of) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t w[K];
#pragma unroll
        for (int c = 0; c < K; ++c) w[c] = own.w[c][i];
        uint64_t h = setop::hash_start();
#pragma unroll
        for (int c = 0; c < K; ++c) h = setop::hash_step(h, w[c]);
        uint32_t slot = 0;
        const bool found = set_probe<INSERT>(t, h, uint32_t(i), [&](uint32_t r) {
            bool eq = true;
#pragma unroll
            for (int c = 0; c < K; ++c) eq = eq && rep.w[c][r] == w[c];
            return eq;
        }, &slot);
        if (INSERT) {
            if (found) set_lower_first(&t.slots[2 * size_t(slot) + 1], uint32_t(i));
            slot_of[i] = slot;
        } else if (found) {
            t.marks[slot] = 1;
        }
    }
}

// MODE 0: DISTINCT (and UNION over the concatenation); 1: INTERSECT; 2: EXCEPT.  One wave per 4096-row tile, per 64 rows one ballot
// word of the keep mask, per tile one count (marked_build_kernel's walk).
template <int MODE>
__global__ void __launch_bounds__(SET_THREADS) set_keep_kernel(const uint32_t *slot_of, int64_t n, int64_t ntiles, SetTable t, uint64_t *keep, uint32_t *tile_counts) {
    const int waves_per_block = blockDim.x / 64;
    for (int64_t tile = int64_t(blockIdx.x) * waves_per_block + threadIdx.x / 64; tile < ntiles; tile += int64_t(gridDim.x) * waves_per_block) {
        const int64_t row0 = tile * TILE_ROWS;
        uint32_t total = 0;
        for (int k = 0; k < TILE_WORDS; ++k) {
            const int64_t row = row0 + int64_t(k) * 64 + lane_id();
            bool kept = false;
            if (row < n) {
                const uint32_t s = slot_of[row];
                kept = t.slots[2 * size_t(s) + 1] == uint32_t(row); // (every u32 up to the mask is a slot: no sentinel among slot indices)
                if (MODE == 1) kept = kept && t.marks[s] != 0;
                if (MODE == 2) kept = kept && t.marks[s] == 0;
            }
            const uint64_t kw = __ballot(kept);
            if (row0 + int64_t(k) * 64 < n && lane_id() == 0) keep[tile * TILE_WORDS + k] = kw;
            total += __popcll(kw);
        }
        if (lane_id() == 0) tile_counts[tile] = total;
    }
}

} // namespace

} // namespace nqe
