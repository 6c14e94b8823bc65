// cast.hip — an NQE_EXPR_CAST node (quirk Q29): PhysicalCastExpr, whose body the reference leaves todo!()
// (physical_plan/expression/cast.rs).  What a row becomes is cast_parts.hpp's, how the lanes share the work cast_kernels.hpp's.  This file
// picks the kernel family by the two types, decides whether the result carries a validity buffer of its own (from the static form alone:
// include/nqe.h) and launches.
//
// An infallible cast carries the operand's validity buffer (shared or copied: carry_validity) and its null_count; a fallible one builds
// its own by ballot, null_count -1.  Fixed-width casts and parses are ONE launch and nothing is read back.  A cast to Utf8 sizes its
// output first, as conditional.hip does: lengths, the 64-bit total read back BEFORE the scan and the data buffer (more than 2^31-1 bytes:
// NQE_ERR_ARROW with nothing but the offsets allocated), then the write.  Launching nothing: zero rows, and a cast to the operand's type.
#include "cast_kernels.hpp"
#include "device_utils.hpp"
#include "nqe_internal.hpp"

namespace nqe {

namespace {

static_assert(cast::BOOLEAN == NQE_BOOLEAN && cast::INT64 == NQE_INT64 && cast::UINT64 == NQE_UINT64 && cast::FLOAT64 == NQE_FLOAT64 && cast::UTF8 == NQE_UTF8,
              "cast_parts.hpp numbers the types as nqe_dtype does");

using FixedKernel = decltype(&cast_fixed_kernel<cast::INT64, cast::FLOAT64>);
using ParseKernel = decltype(&cast_parse_kernel<cast::INT64>);
using LengthsKernel = decltype(&cast_text_lengths_kernel<cast::INT64>);
using WriteKernel = decltype(&cast_text_write_kernel<cast::INT64>);

template <int FROM> FixedKernel fixed_to(int to) {
    // (the instance FROM -> FROM does not exist: a cast to the operand's type launches nothing)
    switch (to) {
    case NQE_BOOLEAN: if constexpr (FROM != cast::BOOLEAN) return cast_fixed_kernel<FROM, cast::BOOLEAN>; break;
    case NQE_INT64: if constexpr (FROM != cast::INT64) return cast_fixed_kernel<FROM, cast::INT64>; break;
    case NQE_UINT64: if constexpr (FROM != cast::UINT64) return cast_fixed_kernel<FROM, cast::UINT64>; break;
    case NQE_FLOAT64: if constexpr (FROM != cast::FLOAT64) return cast_fixed_kernel<FROM, cast::FLOAT64>; break;
    }
    return nullptr;
}
FixedKernel pick_fixed(int from, int to) {
    return from == NQE_BOOLEAN ? fixed_to<cast::BOOLEAN>(to) : from == NQE_INT64 ? fixed_to<cast::INT64>(to) : from == NQE_UINT64 ? fixed_to<cast::UINT64>(to) : fixed_to<cast::FLOAT64>(to);
}
ParseKernel pick_parse(int to) {
    return to == NQE_BOOLEAN ? cast_parse_kernel<cast::BOOLEAN> : to == NQE_INT64 ? cast_parse_kernel<cast::INT64> : to == NQE_UINT64 ? cast_parse_kernel<cast::UINT64> : cast_parse_kernel<cast::FLOAT64>;
}
LengthsKernel pick_lengths(int from) {
    return from == NQE_BOOLEAN ? cast_text_lengths_kernel<cast::BOOLEAN> : from == NQE_INT64 ? cast_text_lengths_kernel<cast::INT64> : cast_text_lengths_kernel<cast::UINT64>;
}
WriteKernel pick_write(int from) {
    return from == NQE_BOOLEAN ? cast_text_write_kernel<cast::BOOLEAN> : from == NQE_INT64 ? cast_text_write_kernel<cast::INT64> : cast_text_write_kernel<cast::UINT64>;
}

// Boolean / Int64 / UInt64 -> Utf8: infallible, the operand's validity
DevColumn cast_to_utf8(nqe_ctx *ctx, const DevColumn &src) {
    const int64_t n = src.length;
    DevColumn out;
    if (n == 0) {
        out = empty_utf8(ctx);
        carry_validity(ctx, src, &out);
        return out;
    }
    out.dtype = NQE_UTF8;
    out.length = n;
    carry_validity(ctx, src, &out);
    out.values = dev_alloc(ctx, size_t(n + 1) * 4 + 8); // lengths, then (after the scan) int32 offsets
    BufRef total64 = dev_alloc_zero(ctx, 8);
    launch(ctx, "cast_text_lengths", pick_lengths(src.dtype), dim3(stream_grid(ctx, n, CAST_LANE_ROWS)), dim3(256), 0, (const void *)src.values->ptr, src.valid(), n,
           (uint32_t *)out.values->ptr, (unsigned long long *)total64->ptr);
    const uint32_t total = utf8_size_output(ctx, total64, n, &out);
    if (total)
        launch(ctx, "cast_text_write", pick_write(src.dtype), dim3(stream_grid(ctx, n, CAST_LANE_ROWS)), dim3(256), 0, (const void *)src.values->ptr, (const uint32_t *)out.values->ptr,
               (uint8_t *)out.data->ptr, n);
    return out;
}

} // namespace

DevColumn cast_column(nqe_ctx *ctx, const DevColumn &src, int to) {
    const int from = src.dtype;
    if (from == to) return src; // the operand itself, as a bare column evaluates (an output copies what it may not alias)
    if (to == NQE_UTF8) {
        if (from != NQE_BOOLEAN && from != NQE_INT64 && from != NQE_UINT64) fail(NQE_ERR_NOT_SUPPORTED, "a cast of this type to Utf8");
        return cast_to_utf8(ctx, src);
    }
    const int64_t n = src.length;
    const bool own_validity = cast::fallible(from, to);
    DevColumn out = to == NQE_BOOLEAN ? make_bool_column(ctx, n, own_validity) : make_word_column(ctx, to, n, own_validity);
    if (!own_validity) carry_validity(ctx, src, &out);
    if (n == 0) return out;
    uint64_t *ov = own_validity ? (uint64_t *)out.validity->ptr : nullptr;
    if (from == NQE_UTF8) {
        launch(ctx, "cast_parse", pick_parse(to), dim3(stream_grid(ctx, n, CAST_LANE_ROWS)), dim3(256), 0, (const int32_t *)src.values->ptr,
               src.data ? (const uint8_t *)src.data->ptr : nullptr, src.valid(), n, (uint64_t *)out.values->ptr, ov);
        return out;
    }
    FixedKernel k = pick_fixed(from, to);
    if (!k) fail(NQE_ERR_NOT_SUPPORTED, "a cast between these types");
    launch(ctx, "cast_fixed", k, dim3(stream_grid(ctx, (n + CAST_ROWS - 1) / CAST_ROWS, 256)), dim3(256), 0, (const void *)src.values->ptr, src.valid(), n, (uint64_t *)out.values->ptr, ov);
    return out;
}

} // namespace nqe

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::cast_text_lengths_kernel<nqe::cast::INT64>);
