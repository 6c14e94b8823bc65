// string_args.hip — the string functions of an NQE_EXPR_STRING_ARGS node (quirk Q26) over one Utf8 column: SUBSTR(s, start, len),
// REPEAT(s, n), REPLACE(s, from, to).  The reference names them in `enum UnaryOperator` and leaves them todo!() (unary.rs:97-106); what
// each computes is string_args_parts.hpp's, how the lanes share the work string_args_kernels.hpp's.  This file sizes the outputs and
// launches.
//
// Every form sizes its output first — SUBSTR like a trim (kept lengths and starts, an exclusive scan, one read-back of the total,
// str_trim_copy), REPEAT and REPLACE with 64-bit lengths whose total is read back BEFORE the scan and the data buffer: a result of more
// than 2^31-1 bytes is NQE_ERR_ARROW with nothing but the offsets allocated.  REPLACE with |to| == |from| keeps the operand's offsets and
// never waits for a kernel; with an empty `from`, or one longer than the operand's data, it returns the operand.
#include "device_utils.hpp"
#include "nqe_internal.hpp"
#include "string_args_kernels.hpp"
#include "string_lanes.hpp"

namespace nqe {

namespace {

StrArgView view_of(const StrIntArg &a) { return {a.col ? (const int64_t *)a.col->values->ptr : nullptr, a.col ? a.col->valid() : nullptr, a.lit}; }

// The result's validity: the operand's, carried as Q25 carries it, when no argument column can be NULL; else the AND of the bitmaps
// with its exact null_count (one more wait).
void result_validity(nqe_ctx *ctx, const DevColumn &src, const DevColumn *a1, const DevColumn *a2, DevColumn *out) {
    const uint8_t *v1 = a1 ? a1->valid() : nullptr, *v2 = a2 ? a2->valid() : nullptr;
    if (!v1 && !v2) return carry_validity(ctx, src, out);
    const int64_t n = src.length;
    out->validity = dev_alloc(ctx, bitmap_alloc_bytes(n));
    BufRef valid_rows = dev_alloc_zero(ctx, 8);
    launch(ctx, "str_args_validity", str_args_validity_kernel, dim3(stream_grid(ctx, (n + 63) / 64, 256)), dim3(256), 0, src.valid(), v1, v2, n, (uint64_t *)out->validity->ptr,
           (unsigned long long *)valid_rows->ptr);
    out->null_count = n - int64_t(read_scalar(ctx, (const unsigned long long *)valid_rows->ptr));
}

// a NULL literal argument: every row NULL and empty
DevColumn all_null(nqe_ctx *ctx, int64_t n) { return utf8_literal_column(ctx, std::string(), true, n); }

} // namespace

// every result row is empty: offsets of zeros, no bytes, nothing launched
void utf8_empty_rows(nqe_ctx *ctx, int64_t n, DevColumn *out) {
    out->values = dev_alloc_zero(ctx, size_t(n + 1) * 4 + 8);
    out->data = dev_alloc(ctx, 8);
    out->data_length = 0;
}

// `lens` (n + 1 counts in out->values) become the offsets and the data buffer is allocated — after the 64-bit total has been read back and
// found to fit.  Returns the total; 0: nothing to copy.
uint32_t utf8_size_output(nqe_ctx *ctx, const BufRef &total64, int64_t n, DevColumn *out) {
    const unsigned long long total = read_scalar(ctx, (const unsigned long long *)total64->ptr);
    if (total > strargs::MAX_TOTAL) fail(NQE_ERR_ARROW, "offset overflow: the result holds " + std::to_string(total) + " bytes, int32 offsets address 2^31-1");
    if (total == 0) {
        utf8_empty_rows(ctx, n, out);
        return 0;
    }
    exclusive_scan_u32_inplace(ctx, (uint32_t *)out->values->ptr, n + 1);
    out->data_length = int64_t(total);
    out->data = dev_alloc(ctx, size_t(total) + 8);
    return uint32_t(total);
}

DevColumn string_substr(nqe_ctx *ctx, const DevColumn &src, const StrIntArg &start, const StrIntArg &len) {
    const int64_t n = src.length, bytes = src.data_length;
    if (start.lit_null || len.lit_null) return all_null(ctx, n);
    DevColumn out;
    if (n == 0) {
        out = empty_utf8(ctx);
        carry_validity(ctx, src, &out);
        return out;
    }
    out.dtype = NQE_UTF8;
    out.length = n;
    result_validity(ctx, src, start.col, len.col, &out);
    uint64_t lo, hi;
    const bool empty_window = !start.col && !len.col && !strargs::substr_window(start.lit, len.lit, &lo, &hi);
    if (bytes == 0 || !src.data || empty_window) { // every string is empty already, or the literal window holds no character
        utf8_empty_rows(ctx, n, &out);
        return out;
    }
    const int32_t *off = (const int32_t *)src.values->ptr;
    const uint8_t *data = (const uint8_t *)src.data->ptr;
    out.values = dev_alloc(ctx, size_t(n + 1) * 4 + 8); // kept lengths, then (after the scan) int32 offsets
    BufRef starts = dev_alloc(ctx, size_t(n) * 4 + 8);
    int lg = lanes_log2(bytes, n);
    launch(ctx, "str_substr_bounds", NQE_STR_PICK(str_substr_bounds_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, src.valid(), view_of(start), view_of(len),
           n, (uint32_t *)out.values->ptr, (uint32_t *)starts->ptr);
    exclusive_scan_u32_inplace(ctx, (uint32_t *)out.values->ptr, n + 1);
    const uint32_t total = read_scalar(ctx, (const uint32_t *)out.values->ptr + n); // (never more than the operand's bytes: no int32 overflow)
    out.data_length = total;
    out.data = dev_alloc(ctx, size_t(total) + 8);
    if (total) {
        lg = lanes_log2(total, n);
        launch(ctx, "str_trim_copy", NQE_STR_PICK(str_trim_copy_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, (const uint32_t *)starts->ptr,
               (const uint32_t *)out.values->ptr, (uint8_t *)out.data->ptr, n);
    }
    return out;
}

DevColumn string_repeat(nqe_ctx *ctx, const DevColumn &src, const StrIntArg &times) {
    const int64_t n = src.length, bytes = src.data_length;
    if (times.lit_null) return all_null(ctx, n);
    DevColumn out;
    if (n == 0) {
        out = empty_utf8(ctx);
        carry_validity(ctx, src, &out);
        return out;
    }
    out.dtype = NQE_UTF8;
    out.length = n;
    result_validity(ctx, src, times.col, nullptr, &out);
    if (bytes == 0 || !src.data || (!times.col && times.lit <= 0)) {
        utf8_empty_rows(ctx, n, &out);
        return out;
    }
    const int32_t *off = (const int32_t *)src.values->ptr;
    out.values = dev_alloc(ctx, size_t(n + 1) * 4 + 8);
    BufRef total64 = dev_alloc_zero(ctx, 8);
    launch(ctx, "str_repeat_lengths", str_repeat_lengths_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, off, src.valid(), view_of(times), n, (uint32_t *)out.values->ptr,
           (unsigned long long *)total64->ptr);
    const uint32_t total = utf8_size_output(ctx, total64, n, &out);
    if (total) {
        const int lg = lanes_log2(total, n); // from the OUTPUT's mean: one short string repeated a million times is a whole group's work
        launch(ctx, "str_repeat_copy", NQE_STR_PICK(str_repeat_copy_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, (const uint8_t *)src.data->ptr,
               (const uint32_t *)out.values->ptr, (uint8_t *)out.data->ptr, n);
    }
    return out;
}

DevColumn string_replace(nqe_ctx *ctx, const DevColumn &src, const std::string &from, bool from_null, const std::string &to, bool to_null) {
    const int64_t n = src.length, bytes = src.data_length;
    if (from_null || to_null) return all_null(ctx, n);
    DevColumn out;
    if (n == 0) {
        out = empty_utf8(ctx);
        carry_validity(ctx, src, &out);
        return out;
    }
    // nothing can match: the operand itself (as a bare column evaluates to the input column; an output copies what it may not alias)
    if (from.empty() || int64_t(from.size()) > bytes || !src.data) return src;
    const uint32_t m = uint32_t(from.size()), t = uint32_t(to.size());
    const int bordered = strargs::has_border((const uint8_t *)from.data(), m) ? 1 : 0;
    BufRef pattern = dev_alloc(ctx, size_t(m) + size_t(t) + 8); // `from`, then `to`: one upload
    {
        const std::string both = from + to;
        NQE_HIP_CHECK(hipMemcpyAsync(pattern->ptr, both.data(), both.size(), hipMemcpyHostToDevice, ctx->stream));
        sync(ctx); // `both` ends with this scope (the one wait of the equal-length form: for these bytes, never for a kernel)
    }
    const uint8_t *d_from = (const uint8_t *)pattern->ptr, *d_to = d_from + m;
    const int32_t *off = (const int32_t *)src.values->ptr;
    const uint8_t *data = (const uint8_t *)src.data->ptr;
    out.dtype = NQE_UTF8;
    out.length = n;
    carry_validity(ctx, src, &out);
    int lg = lanes_log2(bytes, n);
    if (t == m) { // the operand's offsets, new bytes, no scan and no read-back
        out.values = carry_offsets(ctx, src);
        out.data = dev_alloc(ctx, size_t(bytes) + 8);
        out.data_length = bytes;
        launch(ctx, "str_replace_same", NQE_STR_PICK(str_replace_same_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, d_from, d_to, m, bordered,
               (uint8_t *)out.data->ptr, n);
        return out;
    }
    out.values = dev_alloc(ctx, size_t(n + 1) * 4 + 8);
    BufRef total64 = dev_alloc_zero(ctx, 8);
    launch(ctx, "str_replace_count", NQE_STR_PICK(str_replace_count_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, src.valid(), d_from, m, t, bordered, n,
           (uint32_t *)out.values->ptr, (unsigned long long *)total64->ptr);
    const uint32_t total = utf8_size_output(ctx, total64, n, &out);
    if (total)
        launch(ctx, "str_replace_emit", NQE_STR_PICK(str_replace_emit_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, off, data, src.valid(), d_from, d_to, m, t, bordered,
               (const uint32_t *)out.values->ptr, (uint8_t *)out.data->ptr, n);
    return out;
}

} // namespace nqe

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::str_repeat_lengths_kernel);
