// conditional.hip — an NQE_EXPR_CONDITIONAL node (quirk Q28): NOT, IS_NULL, IS_NOT_NULL, COALESCE, NULLIF and IF over operands of any form.
// The reference names none of them (sql/planner.rs leaves IsNull, Not and Case unimplemented!()); what a row becomes is
// conditional_parts.hpp's, how the lanes share the work conditional_kernels.hpp's.  This file decides whether the result carries a
// validity buffer (from the static form alone: include/nqe.h), picks the kernel family by the value type and launches.
//
// Words and bitmaps are ONE launch and nothing is read back.  Utf8 sizes its output first, as string_args.hip does: sources and lengths,
// the 64-bit total read back BEFORE the scan and the data buffer (more than 2^31-1 bytes: NQE_ERR_ARROW with nothing but the offsets
// allocated), then the copy.  Launching nothing: zero rows, and a COALESCE whose first operand is a column without validity (that column).
#include "conditional_kernels.hpp"
#include "device_utils.hpp"
#include "nqe_internal.hpp"
#include "string_lanes.hpp"

namespace nqe {

namespace {

static_assert(cond::NOT == NQE_COND_NOT && cond::IS_NULL == NQE_COND_IS_NULL && cond::IS_NOT_NULL == NQE_COND_IS_NOT_NULL && cond::COALESCE == NQE_COND_COALESCE &&
                  cond::NULLIF == NQE_COND_NULLIF && cond::IF == NQE_COND_IF,
              "conditional_parts.hpp numbers the functions as nqe_cond_operator does");

bool can_be_null(const CondArg &k) { return k.col ? k.col->validity != nullptr : k.lit_null; }

Operand operand_of(const CondArg &k) {
    Operand o;
    o.values = k.col && k.col->values ? k.col->values->ptr : nullptr;
    o.valid = k.col ? k.col->valid() : nullptr;
    o.lit = k.lit;
    o.is_lit = k.col ? 0 : 1;
    o.lit_null = k.lit_null ? 1 : 0;
    return o;
}

// does the static form carry a validity buffer?  (a, b: the value operands — IF's t and e)
bool result_has_validity(int op, const CondArg &a, const CondArg &b) {
    switch (op) {
    case NQE_COND_NOT: return can_be_null(a);
    case NQE_COND_COALESCE: return can_be_null(a) && can_be_null(b);
    case NQE_COND_IF: return can_be_null(a) || can_be_null(b);
    case NQE_COND_NULLIF: return true;
    default: return false; // IS_NULL, IS_NOT_NULL
    }
}

using WordsKernel = decltype(&cond_words_kernel<cond::IF, true>);
using BitsKernel = decltype(&cond_bits_kernel<cond::IF, true>);
template <int F> WordsKernel words_kernel(bool hv) { return hv ? cond_words_kernel<F, true> : cond_words_kernel<F, false>; }
template <int F> BitsKernel bits_kernel(bool hv) { return hv ? cond_bits_kernel<F, true> : cond_bits_kernel<F, false>; }
WordsKernel pick_words(int op, bool hv) {
    return op == NQE_COND_COALESCE ? words_kernel<cond::COALESCE>(hv) : op == NQE_COND_IF ? words_kernel<cond::IF>(hv) : cond_words_kernel<cond::NULLIF, true>;
}
BitsKernel pick_bits(int op, bool hv) {
    switch (op) {
    case NQE_COND_NOT: return bits_kernel<cond::NOT>(hv);
    case NQE_COND_IS_NULL: return cond_bits_kernel<cond::IS_NULL, false>;
    case NQE_COND_IS_NOT_NULL: return cond_bits_kernel<cond::IS_NOT_NULL, false>;
    case NQE_COND_COALESCE: return bits_kernel<cond::COALESCE>(hv);
    case NQE_COND_IF: return bits_kernel<cond::IF>(hv);
    default: return cond_bits_kernel<cond::NULLIF, true>;
    }
}

CondStr str_of(const DevColumn &c) { return {(const int32_t *)c.values->ptr, c.data ? (const uint8_t *)c.data->ptr : nullptr, c.valid()}; }

// COALESCE / NULLIF / IF over Utf8 columns (the caller has expanded literals): every form is "a where the condition holds, else b"
DevColumn conditional_utf8(nqe_ctx *ctx, int op, const CondArg &a, const CondArg &b, const CondArg &c, int64_t n) {
    const bool hv = result_has_validity(op, a, b);
    DevColumn out;
    if (n == 0) {
        out = empty_utf8(ctx);
        if (hv) {
            out.validity = dev_alloc_zero(ctx, 8);
            out.null_count = -1;
        }
        return out;
    }
    out.dtype = NQE_UTF8;
    out.length = n;
    BufRef zeros; // a bitmap of no set bit: a condition that never holds, an operand that is never valid
    auto never = [&]() {
        if (!zeros) zeros = dev_alloc_zero(ctx, bitmap_alloc_bytes(n));
        return (const uint8_t *)zeros->ptr;
    };
    const uint8_t *c_bits = nullptr, *c_valid = nullptr;
    CondStr A = str_of(*a.col), B = str_of(*b.col);
    DevColumn equal;
    if (op == NQE_COND_COALESCE)
        c_valid = a.col->valid();
    else if (op == NQE_COND_IF) {
        if (c.col) {
            c_bits = c.col->bits();
            c_valid = c.col->valid();
        } else if (c.lit_null || !c.lit)
            c_bits = never();
    } else { // NULLIF(a, b) = IF(a = b, NULL, a): the compare is strings.hip's, byte-wise
        equal = utf8_compare(ctx, NQE_OP_EQ, a.col, std::string(), false, b.col, std::string(), false, n);
        c_bits = equal.bits();
        c_valid = equal.valid();
        B = A;
        A.valid = never();
    }
    if (hv) {
        out.validity = dev_alloc(ctx, bitmap_alloc_bytes(n));
        out.null_count = -1;
    }
    out.values = dev_alloc(ctx, size_t(n + 1) * 4 + 8); // lengths, then (after the scan) int32 offsets
    BufRef pick = dev_alloc(ctx, size_t(n) + 8), total64 = dev_alloc_zero(ctx, 8);
    launch(ctx, "cond_str_lengths", cond_str_lengths_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, c_bits, c_valid, A, B, n, (uint8_t *)pick->ptr, (uint32_t *)out.values->ptr,
           hv ? (uint64_t *)out.validity->ptr : nullptr, (unsigned long long *)total64->ptr);
    const uint32_t total = utf8_size_output(ctx, total64, n, &out);
    if (total) {
        const int lg = lanes_log2(total, n); // from the RESULT's mean length
        launch(ctx, "cond_str_copy", NQE_STR_PICK(cond_str_copy_kernel, lg), dim3(group_grid(ctx, n, lg)), dim3(256), 0, A, B, (const uint8_t *)pick->ptr,
               (const uint32_t *)out.values->ptr, (uint8_t *)out.data->ptr, n);
    }
    return out;
}

} // namespace

DevColumn conditional(nqe_ctx *ctx, int op, int dtype, const CondArg &a, const CondArg &b, const CondArg &c, int64_t n) {
    // a first operand that cannot be NULL is the answer (as a bare column evaluates to the input column; an output copies what it may not alias)
    if (op == NQE_COND_COALESCE && a.col && !a.col->validity) return *a.col;
    const bool one_operand = op <= NQE_COND_IS_NOT_NULL;
    if (dtype == NQE_UTF8 && !one_operand) return conditional_utf8(ctx, op, a, b, c, n);
    const bool hv = result_has_validity(op, a, b);
    if (one_operand || dtype == NQE_BOOLEAN) {
        DevColumn out = make_bool_column(ctx, n, hv);
        if (n)
            launch(ctx, "cond_bits", pick_bits(op, hv), dim3(stream_grid(ctx, (n + 63) / 64, 256)), dim3(256), 0, operand_of(c), operand_of(a), operand_of(b), n,
                   (uint64_t *)out.values->ptr, hv ? (uint64_t *)out.validity->ptr : nullptr);
        return out;
    }
    if (!is_word_type(dtype)) fail(NQE_ERR_NOT_SUPPORTED, "a conditional function over this type");
    DevColumn out = make_word_column(ctx, dtype, n, hv);
    if (n)
        launch(ctx, "cond_words", pick_words(op, hv), dim3(stream_grid(ctx, (n + COND_ROWS - 1) / COND_ROWS, 256)), dim3(256), 0, operand_of(c), operand_of(a), operand_of(b), dtype == NQE_FLOAT64 ? 1 : 0, n,
               (uint64_t *)out.values->ptr, hv ? (uint64_t *)out.validity->ptr : nullptr);
    return out;
}

} // namespace nqe

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::cond_str_lengths_kernel);
