// group_keys_host.hpp — the host steps that turn a tuple of key columns into one Int64 code column: measure the ranges, pack, or build
// the tuple dictionary (kernels: group_keys_kernels.hpp; the plan: group_keys_plan.hpp).  Shared by GROUP BY on several keys
// (group_keys.hip) and the join on several keys (join_keys.hip); `use_validity` = false reads no validity buffer: every slot counts.
#pragma once
#include <cstring>
#include <vector>

#include "device_utils.hpp"
#include "group_keys_kernels.hpp"
#include "group_keys_plan.hpp"
#include "nqe_internal.hpp"

namespace nqe {

namespace {

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

GkCols cols_of(const std::vector<DevColumn> &keys, int64_t n, bool use_validity = true) {
    GkCols c;
    std::memset(&c, 0, sizeof(c));
    c.k = int32_t(keys.size());
    c.n = n;
    for (size_t i = 0; i < keys.size(); ++i) {
        c.words[i] = keys[i].words();
        c.valid[i] = !use_validity || keys[i].null_count == 0 ? nullptr : keys[i].valid();
        c.flip[i] = gk::order_flip(keys[i].dtype == NQE_INT64);
        if (c.valid[i]) c.any_valid = 1;
    }
    return c;
}

// the code column's validity: whole words the kernels write, or none when no key column has a bitmap
DevColumn make_code_column(nqe_ctx *ctx, int64_t n, bool with_validity) {
    DevColumn codes = make_word_column(ctx, NQE_INT64, n, with_validity);
    codes.null_count = with_validity ? -1 : 0;
    return codes;
}

// the value range of every key over its valid rows: one launch, one read-back
gk::PackPlan measure_and_plan(nqe_ctx *ctx, const std::vector<DevColumn> &keys, const GkCols &c, bool vec) {
    const int k = int(keys.size());
    unsigned long long init[2 * gk::MAX_KEYS], got[2 * gk::MAX_KEYS];
    for (int i = 0; i < k; ++i) {
        init[2 * i] = ~0ull;
        init[2 * i + 1] = 0;
    }
    BufRef d = dev_alloc(ctx, sizeof(init));
    NQE_HIP_CHECK(hipMemcpyAsync(d->ptr, init, size_t(2 * k) * 8, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid(unsigned(stream_grid(ctx, vec ? c.n / 2 : c.n, GK_THREADS * GK_UNROLL))), block(GK_THREADS);
    if (vec) launch(ctx, "group_keys_ranges", group_keys_ranges_kernel<true>, grid, block, 0, c, static_cast<unsigned long long *>(d->ptr));
    else launch(ctx, "group_keys_ranges", group_keys_ranges_kernel<false>, grid, block, 0, c, static_cast<unsigned long long *>(d->ptr));
    NQE_HIP_CHECK(hipMemcpyAsync(got, d->ptr, size_t(2 * k) * 8, hipMemcpyDeviceToHost, ctx->stream));
    sync(ctx); // (`init` has been consumed as well)
    gk::KeyRange r[gk::MAX_KEYS];
    for (int i = 0; i < k; ++i) r[i] = gk::KeyRange{got[2 * i], got[2 * i + 1], keys[size_t(i)].dtype == NQE_INT64};
    return gk::plan_pack(r, k);
}

template <bool VEC> void launch_pack(nqe_ctx *ctx, int k, dim3 grid, const GkPack &a) {
    const dim3 block(GK_THREADS);
    switch (k) {
    case 2: launch(ctx, "group_keys_pack", group_keys_pack_kernel<2, VEC>, grid, block, 0, a); break;
    case 3: launch(ctx, "group_keys_pack", group_keys_pack_kernel<3, VEC>, grid, block, 0, a); break;
    case 4: launch(ctx, "group_keys_pack", group_keys_pack_kernel<4, VEC>, grid, block, 0, a); break;
    case 5: launch(ctx, "group_keys_pack", group_keys_pack_kernel<5, VEC>, grid, block, 0, a); break;
    case 6: launch(ctx, "group_keys_pack", group_keys_pack_kernel<6, VEC>, grid, block, 0, a); break;
    case 7: launch(ctx, "group_keys_pack", group_keys_pack_kernel<7, VEC>, grid, block, 0, a); break;
    default: launch(ctx, "group_keys_pack", group_keys_pack_kernel<8, VEC>, grid, block, 0, a); break;
    }
}

DevColumn pack_codes(nqe_ctx *ctx, const GkCols &c, const gk::PackPlan &p, bool vec) {
    DevColumn codes = make_code_column(ctx, c.n, c.any_valid != 0);
    GkPack a;
    a.c = c;
    for (int i = 0; i < p.k; ++i) {
        a.min[i] = p.min[i];
        a.stride[i] = p.stride[i];
    }
    a.codes = static_cast<uint64_t *>(codes.values->ptr);
    a.valid_out = codes.validity ? static_cast<uint64_t *>(codes.validity->ptr) : nullptr;
    vec = vec && aligned16(a.codes);
    const dim3 grid(unsigned(stream_grid(ctx, vec ? c.n / 2 : c.n, GK_THREADS * 2)));
    if (vec) launch_pack<true>(ctx, p.k, grid, a);
    else launch_pack<false>(ctx, p.k, grid, a);
    return codes;
}

// slots of the tuple dictionary over n rows (a power of two >= max(64, 2 n)); *shift: of its hash
uint32_t dict_capacity(int64_t n, int32_t *shift) {
    uint32_t cap = 64;
    while (uint64_t(cap) < 2ull * uint64_t(n)) cap <<= 1;
    int lg = 0;
    while ((1u << lg) < cap) ++lg;
    *shift = 64 - lg;
    return cap;
}

DevColumn dict_codes(nqe_ctx *ctx, const std::vector<DevColumn> &keys, int64_t n, BufRef *slots_keep, bool use_validity = true, const char *who = "group by", uint32_t *cap_out = nullptr,
                     int32_t *shift_out = nullptr) {
    // (the slot count is 32-bit, as the Utf8 dictionary's)
    if (n >= (int64_t(1) << 30)) fail(NQE_ERR_NOT_SUPPORTED, std::string(who) + ": the tuple dictionary handles fewer than 2^30 rows");
    GkDict a;
    std::memset(&a, 0, sizeof(a));
    a.k = int32_t(keys.size());
    a.n = n;
    for (size_t i = 0; i < keys.size(); ++i) {
        const DevColumn &kc = keys[i];
        a.key[i].valid = !use_validity || kc.null_count == 0 ? nullptr : kc.valid();
        if (a.key[i].valid) a.any_valid = 1;
        if (kc.dtype == NQE_UTF8) {
            a.key[i].offs = static_cast<const int32_t *>(kc.values->ptr);
            a.key[i].data = kc.data ? static_cast<const uint8_t *>(kc.data->ptr) : nullptr;
        } else
            a.key[i].words = kc.words();
    }
    const uint32_t cap = dict_capacity(n, &a.shift);
    a.cap = cap;
    if (cap_out) *cap_out = cap; // (the table's shape, for whoever walks it later: join_keys_lookup)
    if (shift_out) *shift_out = a.shift;
    *slots_keep = dev_alloc(ctx, size_t(cap) * 8);
    a.slots = static_cast<long long *>((*slots_keep)->ptr);
    launch(ctx, "group_keys_dict_init", group_keys_fill_kernel, dim3(unsigned(stream_grid(ctx, cap, GK_THREADS))), dim3(GK_THREADS), 0, a.slots, GK_EMPTY, int64_t(cap));
    DevColumn codes = make_code_column(ctx, n, a.any_valid != 0);
    a.codes = static_cast<int64_t *>(codes.values->ptr);
    a.valid_out = codes.validity ? static_cast<uint64_t *>(codes.validity->ptr) : nullptr;
    launch(ctx, "group_keys_dict", group_keys_dict_kernel, dim3(unsigned(stream_grid(ctx, n, GK_THREADS))), dim3(GK_THREADS), 0, a);
    return codes;
}

} // namespace

} // namespace nqe
