// expr.hip — PhysicalExpr::evaluate on the device (reference: src/physical_plan/expression/
// binary.rs:108-155, unary.rs:85-108, column.rs:39-57, literal.rs:32-34; arrow-rs 13 compare /
// kleene / arithmetic / arity::unary kernels at the call sites binary.rs:127-153, unary.rs:28-29).
//
// Two evaluation forms:
//   * general: one streaming kernel per binary or unary node (what arrow does), except that
//     literals stay scalars in registers instead of being materialised as n-row columns
//     (logical_plan/expression.rs:210-222, the TODO at binary.rs:121);
//   * fused:   `col [op lit]{0,2}` shapes (SimpleExpr) are evaluated inside the consumer
//     kernel (compaction, aggregation) from the streamed word — no temporary at all.
//
// The unit is split by concern: expr_plan.hpp (plain C++: the tree parser and type checker, the shape recognisers, the program builder),
// expr_kernels.hpp (every kernel), expr_jit.hpp (the run-time specialised kernels).  This file holds the node-at-a-time evaluator, the
// entry points that pick a form and launch it, and the C ABI.
#include <cmath>
#include <cstring>

#include "device_utils.hpp"
#include "expr_jit.hpp"
#include "expr_kernels.hpp"
#include "expr_plan.hpp"
#include "nqe_internal.hpp"

namespace nqe {

void jit_wait(nqe_ctx *ctx) { jit_wait_all(ctx); }

namespace {

// the one place a table becomes what expr_plan.hpp sees of it
ExprView view_of(const nqe_table *in) {
    ExprView v;
    v.cols.reserve(in->cols.size());
    for (const DevColumn &c : in->cols) v.cols.push_back({c.dtype, c.values != nullptr, c.values ? c.values->ptr : nullptr, c.valid(), c.length});
    return v;
}

struct Value {
    bool is_lit = false;
    bool lit_null = false;
    uint64_t lit = 0;
    std::string lit_str;
    int dtype = NQE_NULLTYPE;
    DevColumn col;
};

DevColumn materialise_literal(nqe_ctx *ctx, int dtype, uint64_t lit, bool lit_null, int64_t n) {
    // ScalarValue::into_array (logical_plan/expression.rs:210-222)
    if (dtype == NQE_NULLTYPE) fail(NQE_ERR_NOT_SUPPORTED, "Null-typed arrays are not supported on the device path");
    DevColumn c;
    if (dtype == NQE_BOOLEAN) {
        c = make_bool_column(ctx, n, lit_null);
        NQE_HIP_CHECK(hipMemsetAsync(c.values->ptr, (!lit_null && lit) ? 0xFF : 0x00, bitmap_alloc_bytes(n), ctx->stream));
    } else {
        c = make_word_column(ctx, dtype, n, lit_null);
        if (n)
            launch(ctx, "fill_words", fill_words_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0,
                   (uint64_t *)c.values->ptr, lit_null ? 0ull : lit, n);
    }
    if (lit_null) {
        NQE_HIP_CHECK(hipMemsetAsync(c.validity->ptr, 0, bitmap_alloc_bytes(n), ctx->stream));
        c.null_count = n;
    }
    return c;
}

Operand operand_of(const Value &v) {
    Operand o;
    o.values = v.is_lit ? nullptr : v.col.values->ptr;
    o.valid = v.is_lit ? nullptr : v.col.valid();
    o.lit = v.lit;
    o.is_lit = v.is_lit;
    o.lit_null = v.lit_null;
    return o;
}

Value eval_node(nqe_ctx *ctx, const nqe_table *in, const std::vector<Node> &t, int i) {
    const Node &x = t[size_t(i)];
    Value v;
    v.dtype = x.out_dtype;
    if (x.kind == NQE_EXPR_COLUMN) {
        v.col = in->cols[size_t(x.column)]; // Arc clone (column.rs:41-43)
        return v;
    }
    if (x.kind == NQE_EXPR_LITERAL) {
        v.is_lit = true;
        v.lit = x.lit;
        v.lit_str = x.lit_str;
        v.lit_null = x.lit_null;
        return v;
    }
    if (x.kind == NQE_EXPR_UNARY) {
        Value c = eval_node(ctx, in, t, x.left);
        const int64_t n = in->rows;
        if (c.is_lit) c.col = materialise_literal(ctx, c.dtype, c.lit, c.lit_null, n); // value.into_array() (unary.rs:90)
        v.col = make_word_column(ctx, NQE_FLOAT64, n, false);
        // arity::unary keeps the operand's null buffer: shared with the operand (reference-counted), unless it is memory borrowed
        // from the caller, which an output may not alias
        if (c.col.validity && !buf_shareable(c.col.validity)) {
            v.col.validity = dev_alloc_zero(ctx, bitmap_alloc_bytes(n));
            if (n) bitmap_place(ctx, c.col.valid(), (uint64_t *)v.col.validity->ptr, 0, n);
        } else
            v.col.validity = c.col.validity;
        v.col.null_count = c.col.null_count;
        if (n) {
            const uint64_t *src = (const uint64_t *)c.col.values->ptr;
            uint64_t *dst = (uint64_t *)v.col.values->ptr;
            const int64_t pairs = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) ? 0 : n / 2;
            // four workgroups per CU, not the eight of the other streaming kernels: with 16 bytes per lane and access the same map over 10^8
            // rows took 0.297 ms at 8 per CU, 0.311 at 16, 0.266 at 4 (abs, sin and `* 2.0` alike; two or four loads in flight per lane:
            // 0.33 / 0.355; the stack machine's 4 x 8-byte pattern: 0.276) — tools/unary_kernel_bench.hip, profiles/unary/kernel_variants.txt
            const dim3 grid(stream_grid(ctx, (n + 1) / 2, 256, 4));
            if (x.op == NQE_UNARY_ABS) launch(ctx, "expr_unary", unary_f64_kernel<NQE_UNARY_ABS>, grid, dim3(256), 0, src, dst, pairs, n);
            else if (x.op == NQE_UNARY_SIN) launch(ctx, "expr_unary", unary_f64_kernel<NQE_UNARY_SIN>, grid, dim3(256), 0, src, dst, pairs, n);
            else launch(ctx, "expr_unary", unary_f64_kernel<NQE_UNARY_COS>, grid, dim3(256), 0, src, dst, pairs, n); // Cos, and Tan (quirk Q16, unary.rs:96)
        }
        return v;
    }
    if (x.kind == NQE_EXPR_STRING) { // quirk Q25 (string_fn.hip): Utf8, or Int64 for CHARACTER_LENGTH, with the operand's validity
        Value c = eval_node(ctx, in, t, x.left);
        if (c.is_lit) c.col = utf8_literal_column(ctx, c.lit_str, c.lit_null, in->rows);
        v.col = string_fn(ctx, x.op, c.col);
        return v;
    }
    if (x.kind == NQE_EXPR_STRING_ARGS) { // quirk Q26 (string_args.hip): Utf8; NULL where any operand is
        Value s = eval_node(ctx, in, t, x.left);
        if (s.is_lit) s.col = utf8_literal_column(ctx, s.lit_str, s.lit_null, in->rows);
        Value a = eval_node(ctx, in, t, x.right), b;
        if (x.third >= 0) b = eval_node(ctx, in, t, x.third);
        if (x.op == NQE_UNARY_REPLACE) { // parse: both are Utf8 literals
            v.col = string_replace(ctx, s.col, a.lit_str, a.lit_null, b.lit_str, b.lit_null);
            return v;
        }
        auto int_arg = [](const Value &k) { return k.is_lit ? StrIntArg{nullptr, int64_t(k.lit), k.lit_null} : StrIntArg{&k.col, 0, false}; };
        v.col = x.op == NQE_UNARY_SUBSTR ? string_substr(ctx, s.col, int_arg(a), int_arg(b)) : string_repeat(ctx, s.col, int_arg(a));
        return v;
    }
    if (x.kind == NQE_EXPR_STRING_MATCH) { // quirk Q27 (string_match.hip): Boolean, Int64 for STRPOS; NULL where `s` or the literal is
        Value s = eval_node(ctx, in, t, x.left);
        if (s.is_lit) s.col = utf8_literal_column(ctx, s.lit_str, s.lit_null, in->rows);
        const Node &pat = t[size_t(x.right)]; // parse: a Utf8 literal
        v.col = string_match(ctx, x.op, s.col, pat.lit_str, pat.lit_null);
        return v;
    }
    if (x.kind == NQE_EXPR_CONDITIONAL) { // quirk Q28 (conditional.hip): operands of any form; IF: left = c, right = t, third = e
        Value k[3];
        const int ops[3] = {x.left, x.right, x.third};
        for (int q = 0; q < 3; ++q) {
            if (ops[q] < 0) continue;
            k[q] = eval_node(ctx, in, t, ops[q]);
            const bool value_operand = x.op >= NQE_COND_COALESCE && !(x.op == NQE_COND_IF && q == 0);
            if (value_operand && k[q].is_lit && k[q].dtype == NQE_UTF8) { // a Utf8 value: a column, as the string nodes expand it
                k[q].col = utf8_literal_column(ctx, k[q].lit_str, k[q].lit_null, in->rows);
                k[q].is_lit = false;
            }
        }
        auto arg = [](const Value &o) { return o.is_lit ? CondArg{nullptr, o.lit, o.lit_null} : CondArg{&o.col, 0, false}; };
        if (x.op == NQE_COND_IF) v.col = conditional(ctx, x.op, x.out_dtype, arg(k[1]), arg(k[2]), arg(k[0]), in->rows);
        else v.col = conditional(ctx, x.op, k[0].dtype, arg(k[0]), x.right >= 0 ? arg(k[1]) : CondArg{}, CondArg{}, in->rows);
        return v;
    }
    if (x.kind == NQE_EXPR_CAST) { // quirk Q29 (cast.hip): a literal is expanded and then cast like a column — there is no folding path
        Value c = eval_node(ctx, in, t, x.left);
        if (c.is_lit) c.col = c.dtype == NQE_UTF8 ? utf8_literal_column(ctx, c.lit_str, c.lit_null, in->rows) : materialise_literal(ctx, c.dtype, c.lit, c.lit_null, in->rows);
        v.col = cast_column(ctx, c.col, x.out_dtype);
        return v;
    }
    Value l = eval_node(ctx, in, t, x.left);
    Value r = eval_node(ctx, in, t, x.right);
    const int64_t n = in->rows;
    if (l.dtype == NQE_UTF8) { // only compares reach here (parse)
        v.col = utf8_compare(ctx, x.op, l.is_lit ? nullptr : &l.col, l.lit_str, l.lit_null, r.is_lit ? nullptr : &r.col, r.lit_str, r.lit_null, n);
        return v;
    }
    if (l.is_lit && r.is_lit) { // lit op lit: materialise one side, as into_array would
        l.col = materialise_literal(ctx, l.dtype, l.lit, l.lit_null, n);
        l.is_lit = false;
    }
    const int dt = l.dtype;
    bool need_valid = (l.is_lit ? l.lit_null : l.col.validity != nullptr) || (r.is_lit ? r.lit_null : r.col.validity != nullptr);
    bool bool_out = x.out_dtype == NQE_BOOLEAN;
    v.col = bool_out ? make_bool_column(ctx, n, need_valid) : make_word_column(ctx, x.out_dtype, n, need_valid);
    OpAux aux = r.is_lit && !r.lit_null ? plan::make_aux(x.op, dt, r.lit) : plan::make_aux(0, 0, 0);
    if (n)
        launch(ctx, "expr_binary", binary_kernel, dim3(stream_grid(ctx, n, 256)), dim3(256), 0, operand_of(l), operand_of(r),
               x.op, dt, aux, n, bool_out ? nullptr : (uint64_t *)v.col.values->ptr,
               bool_out ? (uint64_t *)v.col.values->ptr : nullptr, need_valid ? (uint64_t *)v.col.validity->ptr : nullptr,
               ctx->d_flags);
    return v;
}

// The interpreting kernels are instantiated per (nullable, <= 2 / <= 4 columns, trig): the column registers of a lane are the largest
// block of VGPRs, and an instance without a sin / cos step carries no transcendental code.
// (8 rows per lane measured 176 VGPRs = 2 waves per SIMD — an 8-operator chain 1.19 -> 1.13 ms per 2x10^8 rows, but
// `(id % 1000) * 3 + id / 7` 1.11 -> 1.36 and `v > 50 and id % 3 = 0` 0.98 -> 1.19: four rows per lane it is)
using TreeKernel = decltype(&expr_tree_kernel<false, 2, EX_ROWS, false>);
using TreeCompactKernel = decltype(&expr_tree_compact_kernel<false, 2, false>);
template <bool NU, int NC> TreeKernel pick_expr_tree_trig(bool trig) { return trig ? expr_tree_kernel<NU, NC, EX_ROWS, true> : expr_tree_kernel<NU, NC, EX_ROWS, false>; }
TreeKernel pick_expr_tree_kernel(bool nulls, int ncols, bool trig) {
    if (nulls) return ncols <= 2 ? pick_expr_tree_trig<true, 2>(trig) : pick_expr_tree_trig<true, 4>(trig);
    return ncols <= 2 ? pick_expr_tree_trig<false, 2>(trig) : pick_expr_tree_trig<false, 4>(trig);
}
template <bool NU, int NC> TreeCompactKernel pick_expr_tree_compact_trig(bool trig) { return trig ? expr_tree_compact_kernel<NU, NC, true> : expr_tree_compact_kernel<NU, NC, false>; }
TreeCompactKernel pick_expr_tree_compact_kernel(bool nulls, int ncols, bool trig) {
    if (nulls) return ncols <= 2 ? pick_expr_tree_compact_trig<true, 2>(trig) : pick_expr_tree_compact_trig<true, 4>(trig);
    return ncols <= 2 ? pick_expr_tree_compact_trig<false, 2>(trig) : pick_expr_tree_compact_trig<false, 4>(trig);
}

// A Boolean or validity result behind a selection: the compacting kernels write one byte per kept row (the rows of one bitmap word come
// from several waves), and the bytes are packed into the column's bitmap afterwards.
struct StagedBits {
    BufRef bytes;
    uint64_t *bitmap = nullptr;
    int64_t rows = 0;
    uint8_t *stage(nqe_ctx *ctx, int64_t m, void *bitmap_words) {
        rows = m;
        bitmap = static_cast<uint64_t *>(bitmap_words);
        bytes = dev_alloc(ctx, size_t(m) + 8);
        return static_cast<uint8_t *>(bytes->ptr);
    }
    void pack(nqe_ctx *ctx) const {
        if (bytes) pack_bytes_to_bits(ctx, static_cast<const uint8_t *>(bytes->ptr), rows, bitmap);
    }
};

// the tree's program in one pass of the stack machine — or of its run-time specialised form, once that has been compiled
DevColumn run_program(nqe_ctx *ctx, const plan::ExprProgram &e, int64_t rows) {
    const ExProgram &P = e.P;
    const int odt = e.top().out_dtype;
    const bool bool_out = odt == NQE_BOOLEAN, needs_valid = e.needs_valid;
    DevColumn out = bool_out ? make_bool_column(ctx, rows, needs_valid) : make_word_column(ctx, odt, rows, needs_valid);
    if (!rows) return out;
    dim3 grid(stream_grid(ctx, (rows + EX_ROWS - 1) / EX_ROWS, 256));
    uint64_t *ow = bool_out ? nullptr : (uint64_t *)out.values->ptr, *ob = bool_out ? (uint64_t *)out.values->ptr : nullptr;
    uint64_t *ov = needs_valid ? (uint64_t *)out.validity->ptr : nullptr;
    // three or more steps over a large input: the run-time specialised form of this very program, once it has been compiled
    if (!jit_expr_tree(ctx, P, needs_valid, rows, ow, ob, ov))
        launch(ctx, "expr_tree", pick_expr_tree_kernel(needs_valid, P.ncols, plan::program_has_trig(P)), grid, dim3(256), 0, P, rows, ow, ob, ov, ctx->d_flags);
    return out;
}

// the distinct columns of a projection list, as the generated kernels number them
void store_slots(const SlotTable &slots, JitProj *J) {
    static_assert(SLOT_MAX == JP_MAX_COLS, "the slot table holds what the widest consumer takes");
    J->ncols = slots.n;
    std::memcpy(J->col_values, slots.values, sizeof(J->col_values));
    std::memcpy(J->col_valid, slots.valid, sizeof(J->col_valid));
    std::memcpy(J->col_dtype, slots.dtype, sizeof(J->col_dtype));
}

} // namespace

// ------------------------------------------------------------------ the analysis, over a table (expr_plan.hpp)
bool make_fast_pred(const SimpleExpr &pe, FastPred *fp) { return plan::make_fast_pred(pe, fp); }
FastPred bitmap_fast_pred() { return plan::bitmap_fast_pred(); }
bool match_conj(const nqe_table *in, const nqe_expr_node *nodes, int n, ConjPred *out, int *cols) { return plan::match_conj(view_of(in), nodes, n, out, cols); }
bool match_tree_pred(const nqe_table *in, const nqe_expr_node *nodes, int n, TreePred *out) { return plan::match_tree_pred(view_of(in), nodes, n, out); }
ExprInfo analyze_expr(const nqe_table *in, const nqe_expr_node *nodes, int n) { return plan::analyze_expr(view_of(in), nodes, n); }

DevColumn evaluate_expr(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, int n) {
    plan::ExprProgram e;
    const bool fits = plan::program_of(view_of(in), nodes, n, 0, &e);
    // f(column) / f(literal) alone is one pass in its node kernel as well, and there the result shares the column's validity buffer
    const Node &rt = e.top();
    const bool bare_unary = rt.kind == NQE_EXPR_UNARY && !is_op_node(e.tree[size_t(rt.left)].kind);
    if (fits && !bare_unary) return run_program(ctx, e, in->rows);
    Value v = eval_node(ctx, in, e.tree, e.root);
    if (v.is_lit && v.dtype == NQE_UTF8) return utf8_literal_column(ctx, v.lit_str, v.lit_null, in->rows);
    if (v.is_lit) return materialise_literal(ctx, v.dtype, v.lit, v.lit_null, in->rows);
    return v.col;
}

// `e` over the rows a selection emits, written compacted (one pass over the referenced columns).  Returns false when the
// tree does not fit the stack machine (caller: compact the inputs, then evaluate_expr).
bool evaluate_expr_compacted(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, int n, const KeepMask &km, DevColumn *result) {
    plan::ExprProgram e;
    if (!plan::program_of(view_of(in), nodes, n, 0, &e)) return false;
    const ExProgram &P = e.P;
    const bool needs_valid = e.needs_valid || km.pvalid != nullptr;
    const int64_t m = km.total;
    const int odt = e.top().out_dtype;
    const bool bool_out = odt == NQE_BOOLEAN;
    DevColumn out = bool_out ? make_bool_column(ctx, m, needs_valid) : make_word_column(ctx, odt, m, needs_valid);
    StagedBits bool_bits, valid_bits;
    uint8_t *ob = bool_out ? bool_bits.stage(ctx, m, out.values->ptr) : nullptr, *ov = needs_valid ? valid_bits.stage(ctx, m, out.validity->ptr) : nullptr;
    if (km.ntiles && m > 0) {
        dim3 grid(stream_grid(ctx, km.ntiles, 4));
        const uint64_t *kp = (const uint64_t *)km.keep->ptr, *pv = km.pvalid ? (const uint64_t *)km.pvalid->ptr : nullptr;
        const uint64_t *to = (const uint64_t *)km.tile_offsets->ptr;
        uint64_t *ow = bool_out ? nullptr : (uint64_t *)out.values->ptr;
        launch(ctx, "expr_tree_compact", pick_expr_tree_compact_kernel(needs_valid, P.ncols, plan::program_has_trig(P)), grid, dim3(256), 0, P, kp, pv, to, km.n, km.ntiles, ow,
               ob, ov, ctx->d_flags);
    }
    bool_bits.pack(ctx);
    valid_bits.pack(ctx);
    *result = out;
    return true;
}

bool project_specialised(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, const int32_t *expr_offsets, int num_exprs, const KeepMask &km,
                         std::vector<DevColumn> *result) {
    if (jit_disabled() || num_exprs < 1 || num_exprs > JP_MAX_OUTS || km.n < jit_min_rows() || km.total <= 0) return false;
    const ExprView view = view_of(in);
    JitProj J;
    J.nulls = km.pvalid != nullptr;
    SlotTable slots;
    int steps = 0;
    for (int e = 0; e < num_exprs; ++e) {
        plan::ExprProgram p;
        const bool fits = plan::program_of(view, nodes + expr_offsets[e], expr_offsets[e + 1] - expr_offsets[e], 0, &p);
        const Node &rt = p.top();
        JitProjOut o;
        o.out_dtype = rt.out_dtype;
        if (rt.kind == NQE_EXPR_COLUMN) {
            const DevColumn &c = in->cols[size_t(rt.column)];
            if (!is_word_type(c.dtype) || c.length < km.n) return false; // (Boolean / Utf8 columns: their own compaction kernels)
            o.is_column = true;
            o.col = slots.slot_of(c.values->ptr, c.valid(), c.dtype, JP_MAX_COLS);
            if (o.col < 0) return false;
            o.needs_valid = c.validity != nullptr || km.pvalid != nullptr;
            J.nulls = J.nulls || c.validity != nullptr;
        } else if (fits && slots.renumber(p.P, JP_MAX_COLS, false)) {
            o.P = p.P;
            o.bool_out = rt.out_dtype == NQE_BOOLEAN;
            o.needs_valid = p.needs_valid || km.pvalid != nullptr;
            J.nulls = J.nulls || p.needs_valid;
            steps += o.P.n;
        } else
            return false; // a bare literal, or a tree that does not fit
        J.outs.push_back(o);
    }
    store_slots(slots, &J);
    // bare columns and one- or two-step chains are at the memory system's rate in their own kernels (measured: two bare columns
    // 0.51 ms in two compact_column passes, 0.55 ms fused): the fused pass pays when it removes interpretation
    if (steps < 3) return false;
    // outputs
    const int64_t m = km.total;
    std::vector<DevColumn> cols;
    std::vector<StagedBits> bool_bits(static_cast<size_t>(num_exprs)), valid_bits(static_cast<size_t>(num_exprs));
    uint64_t *ow[JP_MAX_OUTS] = {};
    uint8_t *ob[JP_MAX_OUTS] = {}, *ov[JP_MAX_OUTS] = {};
    for (int e = 0; e < num_exprs; ++e) {
        const JitProjOut &o = J.outs[size_t(e)];
        cols.push_back(o.bool_out ? make_bool_column(ctx, m, o.needs_valid) : make_word_column(ctx, o.out_dtype, m, o.needs_valid));
        if (o.bool_out) ob[e] = bool_bits[size_t(e)].stage(ctx, m, cols.back().values->ptr);
        else ow[e] = (uint64_t *)cols.back().values->ptr;
        if (o.needs_valid) ov[e] = valid_bits[size_t(e)].stage(ctx, m, cols.back().validity->ptr);
    }
    if (!jit_project(ctx, J, km, ow, ob, ov)) return false;
    for (int e = 0; e < num_exprs; ++e) {
        bool_bits[size_t(e)].pack(ctx);
        valid_bits[size_t(e)].pack(ctx);
    }
    *result = std::move(cols);
    return true;
}

namespace {

// The shape select_project_fused takes: a predicate TREE of three or more operators and a projection list of word-typed outputs, all
// over 8-byte columns without validity; fills S (the columns' union, the renumbered programs).
bool plan_select_project(const nqe_table *in, const nqe_expr_node *pred, int pred_nodes, const nqe_expr_node *nodes, const int32_t *expr_offsets, int num_exprs,
                         JitSelProj *S) {
    const ExprView view = view_of(in);
    SlotTable slots;
    {
        plan::ExprProgram p;
        if (!plan::program_of(view, pred, pred_nodes, plan::REQ_BINARY_ROOT | plan::REQ_BOOLEAN | plan::REQ_NO_NULLS, &p)) return false;
        S->pred = p.P;
        // (A/B, NQE_FUSED_SELECT_MIN_STEPS=1: plain `id < K` / `age + 100` through this kernel is SLOWER than the two static kernels —
        // C2 0.36 -> 0.42 ms, random ids 0.46 -> 0.49: their mask and compaction passes already read each column once)
        static const int min_steps = getenv("NQE_FUSED_SELECT_MIN_STEPS") ? atoi(getenv("NQE_FUSED_SELECT_MIN_STEPS")) : 3;
        // (nullable or bit-packed inputs, NULL literals: the two-kernel form handles them)
        if (S->pred.n < min_steps || !slots.renumber(S->pred, JP_MAX_COLS, true, &S->pred_cols, true)) return false;
    }
    for (int e = 0; e < num_exprs; ++e) {
        plan::ExprProgram p;
        const bool fits = plan::program_of(view, nodes + expr_offsets[e], expr_offsets[e + 1] - expr_offsets[e], plan::REQ_NOT_BOOLEAN | plan::REQ_NO_NULLS, &p);
        const Node &rt = p.top();
        JitProjOut o;
        o.out_dtype = rt.out_dtype;
        if (rt.kind == NQE_EXPR_COLUMN) {
            const DevColumn &c = in->cols[size_t(rt.column)];
            if (!is_word_type(c.dtype) || c.validity || c.length < in->rows) return false;
            o.is_column = true;
            o.col = slots.slot_of(c.values->ptr, nullptr, c.dtype, JP_MAX_COLS, true);
            if (o.col < 0) return false;
            S->proj_cols |= 1u << o.col;
        } else if (fits && slots.renumber(p.P, JP_MAX_COLS, true, &S->proj_cols, true)) {
            o.P = p.P;
        } else
            return false; // a bare literal, a Boolean output, NULLs, or a tree that does not fit
        S->proj.outs.push_back(o);
    }
    store_slots(slots, &S->proj);
    return true;
}

// The key of the specialised aggregate: `… % m`, m a literal other than 0, -1, +-1; integer all the way (the static path has vetted it
// as fault-free); a direct-mapped table of m or 2m - 1 slots, 512 <= slots <= 4096
bool plan_aggregate_key(const ExprView &view, const nqe_expr_node *group, int group_nodes, SlotTable *slots, JitAgg *G) {
    plan::ExprProgram p;
    if (!plan::program_of(view, group, group_nodes, plan::REQ_BINARY_ROOT | plan::REQ_NO_NULLS, &p) || p.P.n < 1) return false;
    G->key = p.P;
    const ExInstr &last = G->key.ins[G->key.n - 1];
    if (last.op != NQE_OP_MODULOS || last.b_src != EX_LIT || !(last.dt == NQE_INT64 || last.dt == NQE_UINT64)) return false;
    for (int i = 0; i < G->key.n; ++i) {
        const ExInstr &I = G->key.ins[i];
        if (!(I.dt == NQE_INT64 || I.dt == NQE_UINT64) || I.op < NQE_OP_PLUS || I.op > NQE_OP_MODULOS) return false;
        if ((I.op == NQE_OP_DIVIDE || I.op == NQE_OP_MODULOS) && (I.b_src != EX_LIT || I.lit_b == 0 || I.lit_b == ~0ull)) return false; // could fault
    }
    G->key_signed = last.dt == NQE_INT64;
    G->modulus = G->key_signed ? uint64_t(int64_t(last.lit_b) < 0 ? 0ull - last.lit_b : last.lit_b) : last.lit_b;
    if (G->modulus < 2) return false;
    const uint64_t span64 = G->key_signed ? 2 * G->modulus - 1 : G->modulus;
    if (span64 < 512 || span64 > 4096) return false; // (fewer slots: every lane of a wave updates the same few words — the static kernel replicates such tables)
    G->span = uint32_t(span64);
    return slots->renumber(G->key, JA_MAX_COLS, true, nullptr, true);
}

} // namespace

// Fused ProjectionPlan(SelectionPlan(input)) in ONE pass (expr_jit.hpp: jit_select_project): a predicate TREE (three or more
// operators: the shapes whose mask the specialised kernel computes anyway) over columns without validity, a projection list of
// word-typed outputs over columns without validity, a large input.  Returns false when the shape does not qualify or the kernel is
// still being compiled — the caller then takes the mask + compaction path, whose results are identical.
bool select_project_fused(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int pred_nodes, const nqe_expr_node *nodes, const int32_t *expr_offsets,
                          int num_exprs, std::vector<DevColumn> *result, int64_t *total_out) {
    const int64_t n = in->rows;
    if (jit_disabled() || getenv("NQE_NO_FUSED_SELECT") || num_exprs < 1 || num_exprs > JP_MAX_OUTS || n < jit_min_rows() || !pred || pred_nodes < 1) return false;
    JitSelProj S;
    if (!plan_select_project(in, pred, pred_nodes, nodes, expr_offsets, num_exprs, &S)) return false;
    // the outputs are allocated for the worst case (every row kept): beyond 16 GB of them (NQE_FUSED_SELECT_MAX_GB) the two-kernel
    // form, which sizes its outputs exactly, is the better citizen
    static const double max_gb = getenv("NQE_FUSED_SELECT_MAX_GB") ? atof(getenv("NQE_FUSED_SELECT_MAX_GB")) : 16.0;
    if (double(n) * 8.0 * num_exprs > max_gb * double(1ull << 30)) return false;
    JitEntry *kernel = jit_select_project_entry(ctx, S);
    if (!kernel) return false; // being compiled (or no hipRTC): nothing allocated yet
    // worst-case outputs (every row kept), the chunk status words, ticket and total
    const int64_t n_chunks = (n + SP_BLOCK * SP_R - 1) / (SP_BLOCK * SP_R); // steps: one status word per workgroup step
    std::vector<DevColumn> cols;
    uint64_t *ow[JP_MAX_OUTS] = {};
    BufRef status;
    try {
        for (int e = 0; e < num_exprs; ++e) {
            cols.push_back(make_word_column(ctx, S.proj.outs[size_t(e)].out_dtype, n, false));
            ow[e] = (uint64_t *)cols.back().values->ptr;
        }
        status = dev_alloc(ctx, size_t(n_chunks) * 8 + 16);
    } catch (const Error &e) {
        // the worst-case outputs do not fit: the two-kernel form sizes its outputs exactly and may still run
        if (e.code != NQE_ERR_OUT_OF_MEMORY) throw;
        return false;
    }
    NQE_HIP_CHECK(hipMemsetAsync(status->ptr, 0, size_t(n_chunks) * 8 + 16, ctx->stream));
    unsigned long long *st = (unsigned long long *)status->ptr;
    jit_select_project(ctx, kernel, S, n, ow, st, reinterpret_cast<uint32_t *>(st + n_chunks), st + n_chunks + 1);
    const int64_t total = int64_t(read_scalar(ctx, (const unsigned long long *)(st + n_chunks + 1)));
    for (auto &c : cols) {
        c.length = total;
        // fewer than half the rows the buffer holds and more than 64 MB of it unused: give the large block back (the copy moves
        // `total` rows — less than the pass wrote — and the result no longer pins several times the memory it needs)
        if (total * 2 < n && (n - total) * 8 > (int64_t(64) << 20)) c = slice_column(ctx, c, 0, total);
    }
    *total_out = total;
    *result = std::move(cols);
    return true;
}

// The streaming aggregate under a predicate tree through the lean specialised kernel (expr_jit.hpp: nqe_jit_agg).  On success the
// workgroups' tables are in *partials ([grid][span] sums | mins | maxs as doubles, then counts as uint32 with the NaN mark in the
// top bit) for aggregate.hip's merge kernel; false: the shape does not qualify or the kernel is still being compiled.
bool aggregate_tree_specialised(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int pred_nodes, const nqe_expr_node *group, int group_nodes,
                                int val_col, int grid, BufRef *partials, uint32_t *span_out, int64_t *bias_out, bool dry_run) {
    const int64_t n = in->rows;
    if (jit_disabled() || getenv("NQE_NO_AGG_JIT") || n < jit_min_rows() || !group || group_nodes < 1 || val_col < 0) return false;
    const DevColumn &vc = in->cols[size_t(val_col)];
    if (vc.validity || !is_word_type(vc.dtype) || vc.length < n) return false;
    const ExprView view = view_of(in);
    JitAgg G;
    std::memset(&G.pred, 0, sizeof(G.pred));
    SlotTable slots; // (8-byte columns without validity only, no NULL literal)
    if (!plan_aggregate_key(view, group, group_nodes, &slots, &G)) return false;
    G.val_slot = slots.slot_of(vc.values->ptr, nullptr, vc.dtype, JA_MAX_COLS, true);
    if (G.val_slot < 0) return false;
    G.val_dtype = vc.dtype;
    if (pred && pred_nodes > 0) {
        plan::ExprProgram p;
        if (!plan::program_of(view, pred, pred_nodes, plan::REQ_BINARY_ROOT | plan::REQ_BOOLEAN | plan::REQ_NO_NULLS, &p)) return false;
        G.pred = p.P;
        // a sin / cos step: under this kernel's 128-register cap (1024-thread workgroups) the library's argument reduction spills (70 VGPRs,
        // 188 bytes of scratch offline), and nobody has measured that against the bitmap + static kernel path — which such predicates keep
        if (plan::program_has_trig(G.pred)) return false;
        if (!slots.renumber(G.pred, JA_MAX_COLS, true, nullptr, true)) return false;
    }
    G.ncols = slots.n;
    std::memcpy(G.col, slots.values, sizeof(G.col));
    JitEntry *kernel = jit_aggregate_entry(ctx, G);
    if (!kernel) return false;
    if (dry_run) return true; // the caller only asks whether this query can take the kernel NOW (its compilation has been started otherwise)
    const size_t cells = size_t(grid) * G.span;
    *partials = dev_alloc(ctx, cells * 28 + 64);
    double *ps = (double *)(*partials)->ptr;
    jit_aggregate_launch(ctx, kernel, G, n, unsigned(grid), ps, ps + cells, ps + 2 * cells, reinterpret_cast<uint32_t *>(ps + 3 * cells));
    *span_out = G.span;
    *bias_out = G.key_signed ? int64_t(G.modulus) - 1 : 0;
    return true;
}

} // namespace nqe

using namespace nqe;

// A bare column evaluates to the input column itself (the reference's Arc clone, column.rs:41-43).  As an operator's OUTPUT it
// may stay an alias only of memory that an alias keeps alive; a column borrowed from the caller is copied.
static nqe::DevColumn own_output(nqe_ctx *ctx, nqe::DevColumn c) {
    if (c.shareable()) return c;
    nqe::DevColumn o = nqe::slice_column(ctx, c, 0, c.length);
    o.null_count = c.null_count;
    return o;
}

// ProjectionPlan::execute: every expression of the list over `in` (nqe_expr_evaluate: a list of one)
static void run_projection(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, const int32_t *expr_offsets, int32_t num_exprs, nqe_table **out) {
    // the error flags are reset and read back (a stream synchronisation) only when some expression can raise one
    bool fault = false;
    for (int e = 0; e < num_exprs; ++e) fault = fault || analyze_expr(in, nodes + expr_offsets[e], expr_offsets[e + 1] - expr_offsets[e]).may_fault;
    if (fault) flags_reset(ctx);
    auto t = std::make_unique<nqe_table>();
    t->ctx = ctx;
    t->rows = in->rows;
    for (int e = 0; e < num_exprs; ++e)
        t->cols.push_back(own_output(ctx, evaluate_expr(ctx, in, nodes + expr_offsets[e], expr_offsets[e + 1] - expr_offsets[e])));
    if (fault) throw_on_flags(ctx);
    *out = t.release();
}

extern "C" {

nqe_status nqe_expr_evaluate(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes, int32_t num_nodes,
                             nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !in || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    const int32_t offsets[2] = {0, num_nodes};
    run_projection(ctx, in, nodes, offsets, 1, out);
    NQE_API_END()
}

nqe_status nqe_projection_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *nodes,
                                  const int32_t *expr_offsets, int32_t num_exprs, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !in || !out || num_exprs < 0 || (num_exprs > 0 && (!nodes || !expr_offsets)))
        fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    run_projection(ctx, in, nodes, expr_offsets, num_exprs, out);
    NQE_API_END()
}

} // extern "C"

// this translation unit's code object is loaded when a context is created, not by the first query that needs it (context.hip: load_modules)
NQE_MODULE_PROBE(nqe::fill_words_kernel);
