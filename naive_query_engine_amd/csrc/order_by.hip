// order_by.hip — ORDER BY as an operator (quirk Q18; the reference parses the clause and drops it, sql/planner.rs:159-162): what arrow-rs'
// lexsort_to_indices followed by take would give.  A stable multi-key sort of one table, least significant key first over a u32
// permutation:
//
//   ob_encode   for one pass of one key: reads the key column THROUGH the current permutation (not for the first pass, where the
//               permutation is the identity) and writes an order-preserving u64 per row
//                 Int64    sign flip                          UInt64   the word
//                 Float64  −0.0 → +0.0, every NaN → one quiet NaN above +inf, then the sign / magnitude transform (the order of
//                          OrderedFloat, which min / max use)
//                 Boolean  the bit
//                 Utf8     option (a) of the issue: the string's big-endian 8-byte chunks, zero padded, last chunk first, with the byte
//                          length as the least significant pass — memcmp order, "" < "a" < "a\0" < "ab" < "b"
//                 descending: the complement.  A NULL row's word is 0 in every value pass (NULLs tie among themselves).
//               A nullable key column gets one more pass on the null flag alone, 0 / 1 by nulls_first, whatever `descending` says.
//   sort        radix_sort_pairs_u64 (sort.hip) on (u64, permutation): stable, and a digit pass whose histogram is one bucket is
//               skipped, so the flag pass is one digit pass, a Boolean key one, keys below 2^24 three
//   ob_positions the first `fetch` entries of the permutation widened to the int64 row list of take_column; every column is taken by
//               it, so a `fetch` touches `fetch` rows per column
//
// Up to 4096 rows sort.hip sorts by the composite (key, payload) in one workgroup, which is the stable order only when the payloads
// ascend with the input position: there the payload is the position in the current permutation and ob_compose applies the result.
#include <algorithm>
#include <cstring>
#include <string>

#include "device_utils.hpp"
#include "nqe_internal.hpp"

namespace nqe {

namespace {

constexpr int OB_THREADS = 256;
constexpr int64_t OB_SMALL = 4096; // sort.hip's single-workgroup form

enum ObKind : int { OB_I64 = 0, OB_U64 = 1, OB_F64 = 2, OB_BOOL = 3, OB_UTF8_CHUNK = 4, OB_UTF8_LEN = 5, OB_NULL_FLAG = 6 };

struct ObArgs {
    const uint64_t *words; // Int64 / UInt64 / Float64
    const uint8_t *bits;   // Boolean
    const int32_t *off;    // Utf8
    const uint8_t *data;
    const uint8_t *valid;  // null: no NULLs
    const uint32_t *perm;  // null: the identity
    int64_t n;
    int64_t chunk;         // OB_UTF8_CHUNK: bytes [8 chunk, 8 chunk + 8)
    uint64_t complement;   // ~0 for descending
    uint64_t null_word;    // OB_NULL_FLAG: the word of a NULL row (a valid row gets the other one of 0 / 1)
    uint64_t *keys;        // [n]
    uint32_t *iota;        // the identity pass also leaves 0 … n-1 here (null: not wanted)
};

__device__ __forceinline__ uint64_t ob_f64(uint64_t w) {
    if ((w & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) w = 0x7ff8000000000000ull; // every NaN: one value above +inf
    else if (w == 0x8000000000000000ull) w = 0;                                              // −0.0 ties with +0.0
    return (w >> 63) ? ~w : w | 0x8000000000000000ull;
}

template <int KIND> __global__ void __launch_bounds__(OB_THREADS) ob_encode_kernel(ObArgs a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < a.n; j += stride) {
        const int64_t r = a.perm ? int64_t(a.perm[j]) : j;
        const bool ok = !a.valid || get_bit(a.valid, r);
        uint64_t k = 0;
        if (KIND == OB_NULL_FLAG) {
            k = ok ? (a.null_word ^ 1) : a.null_word;
        } else if (ok) {
            if (KIND == OB_I64) k = a.words[r] ^ 0x8000000000000000ull;
            else if (KIND == OB_U64) k = a.words[r];
            else if (KIND == OB_F64) k = ob_f64(a.words[r]);
            else if (KIND == OB_BOOL) k = get_bit(a.bits, r) ? 1 : 0;
            else {
                const int64_t b = a.off[r], len = int64_t(a.off[r + 1]) - b;
                if (KIND == OB_UTF8_LEN) {
                    k = uint64_t(len);
                } else {
                    const int64_t lo = a.chunk * 8, cnt = min(int64_t(8), len - lo);
                    for (int64_t i = 0; i < cnt; ++i) k |= uint64_t(a.data[b + lo + i]) << (56 - 8 * i);
                }
            }
            k ^= a.complement;
        }
        a.keys[j] = k;
        if (a.iota) a.iota[j] = uint32_t(j);
    }
}

// the longest valid string of a Utf8 key column, in bytes
__global__ void __launch_bounds__(OB_THREADS) ob_max_len_kernel(const int32_t *off, const uint8_t *valid, int64_t n, uint32_t *out) {
    uint32_t m = 0;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
        if (!valid || get_bit(valid, i)) m = max(m, uint32_t(off[i + 1] - off[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, uint32_t(__shfl_xor(int(m), o, 64)));
    if (lane_id() == 0 && m) atomicMax(out, m);
}

// out[i] = perm[order[i]]: the small sort ordered positions of the current permutation
__global__ void __launch_bounds__(OB_THREADS) ob_compose_kernel(const uint32_t *perm, const uint32_t *order, int64_t n, uint32_t *out) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = perm[order[i]];
}

// pos[i] = perm[i] (null: i) for the first m rows of the result
__global__ void __launch_bounds__(OB_THREADS) ob_positions_kernel(const uint32_t *perm, int64_t m, int64_t *pos) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride) pos[i] = perm ? int64_t(perm[i]) : i;
}

void ob_launch_encode(nqe_ctx *ctx, int kind, const ObArgs &a) {
    const dim3 grid(unsigned(stream_grid(ctx, a.n, OB_THREADS))), block(OB_THREADS);
    const char *name = a.perm ? "ob_encode_gather" : "ob_encode";
    switch (kind) {
    case OB_I64: launch(ctx, name, ob_encode_kernel<OB_I64>, grid, block, 0, a); break;
    case OB_U64: launch(ctx, name, ob_encode_kernel<OB_U64>, grid, block, 0, a); break;
    case OB_F64: launch(ctx, name, ob_encode_kernel<OB_F64>, grid, block, 0, a); break;
    case OB_BOOL: launch(ctx, name, ob_encode_kernel<OB_BOOL>, grid, block, 0, a); break;
    case OB_UTF8_CHUNK: launch(ctx, name, ob_encode_kernel<OB_UTF8_CHUNK>, grid, block, 0, a); break;
    case OB_UTF8_LEN: launch(ctx, name, ob_encode_kernel<OB_UTF8_LEN>, grid, block, 0, a); break;
    default: launch(ctx, name, ob_encode_kernel<OB_NULL_FLAG>, grid, block, 0, a); break;
    }
}

// the permutation being built (SortPermutation: `cur` is null while it is still the identity)
struct ObState {
    nqe_ctx *ctx;
    int64_t n;
    SortPermutation &p;
    int next = 0;

    // one stable pass: rows that tie on the encoded word keep the order they have in `cur`
    void pass(int kind, ObArgs a) {
        a.n = n;
        a.perm = p.cur;
        a.keys = static_cast<uint64_t *>(p.keys_in->ptr);
        a.iota = p.cur ? nullptr : static_cast<uint32_t *>(p.iota->ptr);
        ob_launch_encode(ctx, kind, a);
        uint32_t *dst = static_cast<uint32_t *>(p.perm[next]->ptr);
        uint64_t *ko = static_cast<uint64_t *>(p.keys_out->ptr);
        const uint32_t *io = static_cast<const uint32_t *>(p.iota->ptr);
        if (!p.cur) {
            radix_sort_pairs_u64(ctx, a.keys, io, ko, dst, n, false);
        } else if (n > OB_SMALL) {
            radix_sort_pairs_u64(ctx, a.keys, p.cur, ko, dst, n, false);
        } else {
            uint32_t *ord = static_cast<uint32_t *>(p.order->ptr);
            radix_sort_pairs_u64(ctx, a.keys, io, ko, ord, n, false);
            launch(ctx, "ob_compose", ob_compose_kernel, dim3(unsigned(stream_grid(ctx, n, OB_THREADS))), dim3(OB_THREADS), 0, p.cur, (const uint32_t *)ord, n, dst);
        }
        p.cur = dst;
        next ^= 1;
    }
};

} // namespace

// the stable permutation of `in`'s rows by `keys` (checked by the caller; in->rows in (1, 2^32)), least significant key first
const uint32_t *build_sort_permutation(nqe_ctx *ctx, const nqe_table *in, const nqe_sort_key *keys, int32_t num_keys, SortPermutation *hold) {
    const int64_t n = in->rows;
    ObState st{ctx, n, *hold};
    SortPermutation &p = *hold;
    p.keys_in = dev_alloc(ctx, size_t(n) * 8);
    p.keys_out = dev_alloc(ctx, size_t(n) * 8);
    p.iota = dev_alloc(ctx, size_t(n) * 4);
    p.perm[0] = dev_alloc(ctx, size_t(n) * 4);
    if (n <= OB_SMALL) p.order = dev_alloc(ctx, size_t(n) * 4);
    for (int32_t k = num_keys - 1; k >= 0; --k) {
        const DevColumn &c = in->cols[size_t(keys[k].column)];
        ObArgs a;
        std::memset(&a, 0, sizeof(a));
        a.valid = c.null_count == 0 ? nullptr : c.valid();
        a.complement = keys[k].descending ? ~uint64_t(0) : 0;
        auto pass = [&](int kind) {
            if (!p.perm[1] && p.cur) p.perm[1] = dev_alloc(ctx, size_t(n) * 4); // (a single pass needs one buffer)
            st.pass(kind, a);
        };
        if (c.dtype == NQE_UTF8) {
            a.off = static_cast<const int32_t *>(c.values->ptr);
            a.data = c.data ? static_cast<const uint8_t *>(c.data->ptr) : nullptr;
            BufRef d = dev_alloc_zero(ctx, 8);
            launch(ctx, "ob_max_len", ob_max_len_kernel, dim3(unsigned(stream_grid(ctx, n, OB_THREADS, 4))), dim3(OB_THREADS), 0, a.off, a.valid, n, static_cast<uint32_t *>(d->ptr));
            const int64_t max_len = int64_t(read_scalar(ctx, static_cast<const uint32_t *>(d->ptr)));
            pass(OB_UTF8_LEN);
            for (int64_t ch = (max_len + 7) / 8 - 1; ch >= 0; --ch) {
                a.chunk = ch;
                pass(OB_UTF8_CHUNK);
            }
        } else if (c.dtype == NQE_BOOLEAN) {
            a.bits = c.bits();
            pass(OB_BOOL);
        } else {
            a.words = c.words();
            pass(c.dtype == NQE_INT64 ? OB_I64 : c.dtype == NQE_UINT64 ? OB_U64 : OB_F64);
        }
        if (a.valid) { // the flag alone: a full-range Int64 leaves no spare bit for it
            a.null_word = keys[k].nulls_first ? 0 : 1;
            a.complement = 0;
            pass(OB_NULL_FLAG);
        }
    }
    return p.cur;
}

} // namespace nqe

using namespace nqe;

nqe_status nqe_sort_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_sort_key *keys, int32_t num_keys, int64_t fetch, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !in || !out || (num_keys > 0 && !keys)) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (num_keys <= 0) fail(NQE_ERR_PLAN, "order by: the list of sort keys is empty");
    for (int32_t k = 0; k < num_keys; ++k) {
        if (keys[k].column < 0 || size_t(keys[k].column) >= in->cols.size()) fail(NQE_ERR_NOT_SUPPORTED, "order by: key column index out of range");
        const int dt = in->cols[size_t(keys[k].column)].dtype;
        if (!(is_word_type(dt) || dt == NQE_BOOLEAN || dt == NQE_UTF8)) fail(NQE_ERR_NOT_SUPPORTED, "order by: keys of this type are not implemented");
    }
    const int64_t n = in->rows;
    // the permutation is u32: refused before anything is allocated
    if (n >= (int64_t(1) << 32)) fail(NQE_ERR_NOT_SUPPORTED, "order by: " + std::to_string(n) + " rows, the sort handles fewer than 2^32");
    const int64_t m = fetch < 0 ? n : std::min(fetch, n);

    SortPermutation st;
    if (n > 1 && m > 0) build_sort_permutation(ctx, in, keys, num_keys, &st);

    // the first m positions as take's int64 row list; the launch's label carries m (what a test of `fetch` asks nqe_ctx_timing_query for)
    BufRef pos = dev_alloc(ctx, size_t(m) * 8 + 8);
    if (m > 0) {
        const std::string label = "ob_positions:" + std::to_string(m);
        launch(ctx, label.c_str(), ob_positions_kernel, dim3(unsigned(stream_grid(ctx, m, OB_THREADS))), dim3(OB_THREADS), 0, st.cur, m, static_cast<int64_t *>(pos->ptr));
    }
    st.keys_in.reset();
    st.keys_out.reset();
    auto t = std::make_unique<nqe_table>();
    t->ctx = ctx;
    t->rows = m;
    for (const DevColumn &c : in->cols) t->cols.push_back(take_column(ctx, c, static_cast<const int64_t *>(pos->ptr), m));
    *out = t.release();
    NQE_API_END()
}

// No NQE_MODULE_PROBE here: like nested_loop_join.hip, this unit's code object is loaded by the first ORDER BY of a process, not by
// nqe_ctx_create (an eagerly loaded unit cost the headline aggregate 1.3 %: profiles/nested_loop_join/README.md).
