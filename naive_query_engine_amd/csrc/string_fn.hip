// string_fn.hip — the string functions of an NQE_EXPR_STRING node (quirk Q25) over one Utf8 column: TRIM / LTRIM / RTRIM, LOWER / UPPER,
// CHARACTER_LENGTH, REVERSE.  The reference names them in `enum UnaryOperator` and leaves them todo!() (unary.rs:97-106); what each
// computes is string_fn_parts.hpp's, how the lanes share the work string_fn_kernels.hpp's.  This file sizes the outputs and launches.
//
// The length-preserving functions (LOWER, UPPER, REVERSE) give a column with the operand's OFFSETS — the same buffer when an output may
// alias it, a copy otherwise — and new bytes; CHARACTER_LENGTH an Int64 column; none of them waits for the device.  The trims size their
// output like take_utf8: kept lengths, an exclusive scan, one read-back of the total, the copy.
#include "device_utils.hpp"
#include "nqe_internal.hpp"
#include "string_fn_kernels.hpp"
#include "string_lanes.hpp"

namespace nqe {

// the operand's validity as the result's: shared (reference-counted) when an output may alias it, else copied — what the unary node does
void carry_validity(nqe_ctx *ctx, const DevColumn &src, DevColumn *out) {
    const int64_t n = src.length;
    if (src.validity && !buf_shareable(src.validity)) {
        out->validity = dev_alloc_zero(ctx, bitmap_alloc_bytes(n));
        if (n) bitmap_place(ctx, src.valid(), (uint64_t *)out->validity->ptr, 0, n);
    } else
        out->validity = src.validity;
    out->null_count = src.null_count;
}

// the operand's offsets as the result's (the length-preserving functions)
BufRef carry_offsets(nqe_ctx *ctx, const DevColumn &src) {
    if (buf_shareable(src.values)) return src.values;
    const size_t bytes = size_t(src.length + 1) * 4;
    BufRef b = dev_alloc(ctx, bytes + 8);
    NQE_HIP_CHECK(hipMemcpyAsync(b->ptr, src.values->ptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return b;
}

DevColumn empty_utf8(nqe_ctx *ctx) {
    DevColumn c;
    c.dtype = NQE_UTF8;
    c.values = dev_alloc_zero(ctx, 4 + 8);
    c.data = dev_alloc(ctx, 8);
    return c;
}

DevColumn string_fn(nqe_ctx *ctx, int op, const DevColumn &src) {
    const int64_t n = src.length, bytes = src.data_length;
    const int32_t *off = n ? (const int32_t *)src.values->ptr : nullptr;
    const uint8_t *data = src.data ? (const uint8_t *)src.data->ptr : nullptr;
    const bool work = n > 0 && bytes > 0 && data; // zero rows or zero bytes: nothing is launched
    DevColumn out;
    if (op == NQE_UNARY_CHARACTER_LENGTH) {
        out = make_word_column(ctx, NQE_INT64, n, false);
        if (work) {
            const int lg = lanes_log2(bytes, n);
            launch(ctx, "str_length", NQE_STR_PICK(str_length_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, n, (int64_t *)out.values->ptr);
        } else if (n)
            NQE_HIP_CHECK(hipMemsetAsync(out.values->ptr, 0, size_t(n) * 8, ctx->stream));
        carry_validity(ctx, src, &out);
        return out;
    }
    if (n == 0) {
        out = empty_utf8(ctx);
        carry_validity(ctx, src, &out);
        return out;
    }
    out.dtype = NQE_UTF8;
    out.length = n;
    if (op == NQE_UNARY_LOWER || op == NQE_UNARY_UPPER || op == NQE_UNARY_REVERSE) {
        out.values = carry_offsets(ctx, src);
        // the new bytes lie at the operand's misalignment within 16 bytes, so one head serves the loads and the stores of str_case
        const size_t shift = work ? size_t(reinterpret_cast<uintptr_t>(data) & 15) : 0;
        BufRef block = dev_alloc(ctx, size_t(bytes) + 16 + 8);
        const size_t base = (shift + 16 - size_t(reinterpret_cast<uintptr_t>(block->ptr) & 15)) & 15;
        out.data = dev_view(block, base, size_t(bytes) + 8);
        out.data_length = bytes;
        uint8_t *dst = (uint8_t *)out.data->ptr;
        if (work && op == NQE_UNARY_REVERSE) {
            const int lg = lanes_log2(bytes, n);
            launch(ctx, "str_reverse", NQE_STR_PICK(str_reverse_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, dst, n);
        } else if (work) {
            const int64_t to_boundary = int64_t((16 - shift) & 15), head = to_boundary < bytes ? to_boundary : bytes;
            const dim3 grid(stream_grid(ctx, (bytes + 15) / 16, 256, 4));
            if (op == NQE_UNARY_UPPER) launch(ctx, "str_case", str_case_kernel<true>, grid, dim3(256), 0, data, dst, bytes, head);
            else launch(ctx, "str_case", str_case_kernel<false>, grid, dim3(256), 0, data, dst, bytes, head);
        }
        carry_validity(ctx, src, &out);
        return out;
    }
    // TRIM / LTRIM / RTRIM (parse admits no other operator)
    const int mode = op == NQE_UNARY_TRIM ? strfn::TRIM_BOTH : op == NQE_UNARY_LTRIM ? strfn::TRIM_FRONT : strfn::TRIM_BACK;
    if (!work) { // every string is empty already
        out.values = carry_offsets(ctx, src);
        out.data = dev_alloc(ctx, 8);
        carry_validity(ctx, src, &out);
        return out;
    }
    out.values = dev_alloc(ctx, size_t(n + 1) * 4 + 8); // kept lengths, then (after the scan) int32 offsets
    BufRef starts = dev_alloc(ctx, size_t(n) * 4 + 8);
    int lg = lanes_log2(bytes, n);
    launch(ctx, "str_trim_bounds", NQE_STR_PICK(str_trim_bounds_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, n, mode, (uint32_t *)out.values->ptr,
           (uint32_t *)starts->ptr);
    exclusive_scan_u32_inplace(ctx, (uint32_t *)out.values->ptr, n + 1);
    const uint32_t total = read_scalar(ctx, (const uint32_t *)out.values->ptr + n); // (never more than the operand's bytes: no int32 overflow)
    out.data_length = total;
    out.data = dev_alloc(ctx, size_t(total) + 8);
    if (total) {
        lg = lanes_log2(total, n);
        launch(ctx, "str_trim_copy", NQE_STR_PICK(str_trim_copy_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, (const uint32_t *)starts->ptr,
               (const uint32_t *)out.values->ptr, (uint8_t *)out.data->ptr, n);
    }
    carry_validity(ctx, src, &out);
    return out;
}

} // namespace nqe

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::str_case_kernel<false>);
