// string_match.hip — an NQE_EXPR_STRING_MATCH node (quirk Q27) over one Utf8 column: LIKE / NOT_LIKE / ILIKE / NOT_ILIKE, STARTS_WITH,
// ENDS_WITH, CONTAINS (Boolean) and STRPOS (Int64).  The reference has no pattern match (sql/planner.rs:478 is unimplemented!()); what
// a pattern means is string_match_plan.hpp's (the literal compiled into elements, segments and a form), what a string does with it
// string_match_parts.hpp's, how the lanes share the work string_match_kernels.hpp's.  This file picks the kernel by the form and launches.
//
// The result's size is known beforehand: nothing is read back, and a node is ONE launch behind ONE upload of the compiled pattern.  Zero
// rows, a NULL literal and the form ALWAYS launch no matching kernel (ALWAYS is the operand's validity as the value bits, or their
// complement under NOT: zeros).  The result carries the operand's validity; the kernels only read it.
#include <cstring>

#include "device_utils.hpp"
#include "nqe_internal.hpp"
#include "string_lanes.hpp"
#include "string_match_kernels.hpp"
#include "string_match_plan.hpp"

namespace nqe {

namespace {

// the first min(m, 8) bytes as a little-endian word
uint64_t low_word(const char *p, size_t m) {
    uint64_t w = 0;
    for (size_t k = 0; k < m && k < 8; ++k) w |= uint64_t(uint8_t(p[k])) << (8 * k);
    return w;
}

using ScanKernel = decltype(&str_match_scan_kernel<2, false, false>);
template <bool FOLD, bool POS> ScanKernel pick_scan(int lg) {
    return lg == 2 ? str_match_scan_kernel<2, FOLD, POS> : lg == 3 ? str_match_scan_kernel<3, FOLD, POS> : lg == 4 ? str_match_scan_kernel<4, FOLD, POS>
         : lg == 5 ? str_match_scan_kernel<5, FOLD, POS> : str_match_scan_kernel<6, FOLD, POS>;
}
static_assert(sizeof(strmatch::Segment) == sizeof(strmatch::SegView), "the segments are uploaded as the host compiled them");

} // namespace

DevColumn string_match(nqe_ctx *ctx, int op, const DevColumn &src, const std::string &pattern, bool pattern_null) {
    const int64_t n = src.length, bytes = src.data_length;
    const bool pos = op == NQE_MATCH_STRPOS;
    DevColumn out;
    if (pattern_null) { // every row NULL, every value 0
        out = pos ? make_word_column(ctx, NQE_INT64, n, true) : make_bool_column(ctx, n, true);
        if (n) {
            NQE_HIP_CHECK(hipMemsetAsync(out.values->ptr, 0, pos ? size_t(n) * 8 : bitmap_alloc_bytes(n), ctx->stream));
            NQE_HIP_CHECK(hipMemsetAsync(out.validity->ptr, 0, bitmap_alloc_bytes(n), ctx->stream));
        }
        out.null_count = n;
        return out;
    }
    out = pos ? make_word_column(ctx, NQE_INT64, n, false) : make_bool_column(ctx, n, false);
    carry_validity(ctx, src, &out);
    if (n == 0) return out;
    const strmatch::Compiled c = strmatch::compile(op, pattern);
    const int32_t *off = (const int32_t *)src.values->ptr;
    const uint8_t *data = src.data ? (const uint8_t *)src.data->ptr : nullptr;
    if (c.form == strmatch::FORM_ALWAYS && !pos) {
        if (c.negate)
            NQE_HIP_CHECK(hipMemsetAsync(out.values->ptr, 0, bitmap_alloc_bytes(n), ctx->stream));
        else { // true wherever the row is valid: the validity's bits (none: ones) with a zero tail
            BufRef counted = dev_alloc_zero(ctx, 8);
            launch(ctx, "str_match_always", str_args_validity_kernel, dim3(stream_grid(ctx, (n + 63) / 64, 256)), dim3(256), 0, src.valid(), (const uint8_t *)nullptr,
                   (const uint8_t *)nullptr, n, (uint64_t *)out.values->ptr, (unsigned long long *)counted->ptr);
        }
        return out;
    }
    // the compiled pattern in one upload: the elements, the ONE flags, the segments (8-aligned), 16 bytes of padding
    const size_t ne = c.elems.size(), seg_at = (2 * ne + 7) & ~size_t(7), total = seg_at + c.segs.size() * sizeof(strmatch::Segment);
    std::string image(total + 16, '\0');
    std::memcpy(&image[0], c.elems.data(), ne);
    std::memcpy(&image[ne], c.ones.data(), ne);
    if (!c.segs.empty()) std::memcpy(&image[seg_at], c.segs.data(), c.segs.size() * sizeof(strmatch::Segment));
    BufRef dev = dev_alloc(ctx, image.size());
    NQE_HIP_CHECK(hipMemcpyAsync(dev->ptr, image.data(), image.size(), hipMemcpyHostToDevice, ctx->stream));
    const uint8_t *d_el = (const uint8_t *)dev->ptr;

    if (c.form >= strmatch::FORM_EQUAL && c.form <= strmatch::FORM_PREFIX_SUFFIX) {
        StrAnchors a{};
        a.lit = d_el;
        a.exact = c.form == strmatch::FORM_EQUAL;
        a.negate = c.negate;
        const bool front = c.form != strmatch::FORM_SUFFIX; // the first segment is the prefix
        if (!c.segs.empty()) {
            a.pre = front ? c.segs[0].len : 0;
            a.suf = c.form == strmatch::FORM_SUFFIX ? c.segs[0].len : c.form == strmatch::FORM_PREFIX_SUFFIX ? c.segs[1].len : 0;
        }
        a.pre_word = low_word(c.elems.data(), a.pre);
        a.suf_word = low_word(c.elems.data() + a.pre, a.suf);
        auto kernel = c.fold ? str_match_anchor_kernel<true> : str_match_anchor_kernel<false>;
        launch(ctx, "str_match_anchor", kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, off, data, src.valid(), a, n, (uint64_t *)out.values->ptr);
    } else {
        strmatch::Pattern P{};
        P.el = d_el;
        P.one = d_el + ne;
        P.segs = (const strmatch::SegView *)(d_el + seg_at);
        P.nseg = uint32_t(c.segs.size());
        P.min_bytes = c.min_bytes;
        P.anchored_front = c.anchored_front;
        P.anchored_back = c.anchored_back;
        P.has_any = c.has_any;
        P.negate = c.negate;
        for (const strmatch::Segment &sg : c.segs) P.has_one |= sg.ones != 0;
        const int lg = lanes_log2(bytes, n);
        ScanKernel kernel = pos ? pick_scan<false, true>(lg) : c.fold ? pick_scan<true, false>(lg) : pick_scan<false, false>(lg);
        launch(ctx, "str_match_scan", kernel, dim3(stream_grid(ctx, (n + 63) / 64, 4)), dim3(256), 0, off, data, src.valid(), P, n, pos ? nullptr : (uint64_t *)out.values->ptr,
               pos ? (int64_t *)out.values->ptr : nullptr);
    }
    sync(ctx); // `image` ends with this scope (the one wait: for the pattern's bytes)
    return out;
}

} // namespace nqe

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::str_match_anchor_kernel<false>);
