// group_keys.hip — GROUP BY on several keys (quirk Q20; the reference's planner builds `group by a, b` plans and
// PhysicalAggregatePlan::execute reads group_expr[0] alone, aggregate/mod.rs:146).  Composition, not a new aggregate: new kernels turn
// a row's key tuple into ONE Int64 code, the existing tier ladder of aggregate.hip aggregates by that code — over `in` with the code
// column appended, so the indices in the predicate and the aggregates keep their meaning —, and small kernels turn the groups' codes
// back into key columns.  `group by <Utf8 column>` has always worked this way (utf8_encode_build, strings.hip); this is the same route
// for a tuple.
//
//   one integer key  forwards to the existing call with the key expression untouched (so `id % 1024` keeps its tier), then assembles
//                    [key, aggregates].  (One Utf8 key takes the dictionary path below: the existing call's keys_out reads each string
//                    from its representative row, and utf8_encode_build lets a NULL slot represent the valid rows that hold the same
//                    bytes — the string then comes back as a NULL.  The tuple dictionary never gives a NULL row a slot.)
//   packed path      every key Int64 / UInt64 and the product of the value spans at most 2^62 (group_keys_plan.hpp):
//                    group_keys_ranges (min / max per key; ONE read-back of 2k words, the path's only extra host wait) →
//                    group_keys_pack (mixed-radix code, key 0 most significant) → aggregate → group_keys_decode.  Ascending code is
//                    ascending tuple order: no sort.
//   dictionary path  a Utf8 key anywhere, or spans whose product overflows: group_keys_dict (code = representative row of the tuple)
//                    → aggregate → take of every key column by the groups' codes → the ORDER BY unit's sort by the key columns.
//
// A key that is not a bare column is evaluated into a temporary column first (evaluate_expr); when such a key can fault (a divisor
// that is not a literal) and there is a predicate, the selection runs first, as in the existing aggregate: the key must only see
// rows that survive the filter.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_utils.hpp"
#include "group_keys_host.hpp" // (and through it group_keys_kernels.hpp, group_keys_plan.hpp)
#include "nqe_internal.hpp"

static_assert(NQE_MAX_GROUP_KEYS == nqe::gk::MAX_KEYS, "the header and the plan agree on the key count");

namespace nqe {

namespace {

struct TableGuard { // a table handle of ours released on every way out
    nqe_table *t = nullptr;
    ~TableGuard() {
        if (t) nqe_table_release(t);
    }
};

// a key column of the result: no validity buffer (no group has a NULL key)
DevColumn without_validity(DevColumn c) {
    c.validity.reset();
    c.null_count = 0;
    return c;
}

std::vector<DevColumn> decode_codes(nqe_ctx *ctx, const std::vector<DevColumn> &keys, const gk::PackPlan &p, const DevColumn &codes) {
    const int64_t G = codes.length;
    std::vector<DevColumn> out;
    GkDecode a;
    std::memset(&a, 0, sizeof(a));
    a.codes = codes.words();
    a.g = G;
    a.k = p.k;
    for (int i = 0; i < p.k; ++i) {
        out.push_back(make_word_column(ctx, keys[size_t(i)].dtype, G, false));
        a.min[i] = p.min[i];
        a.span[i] = p.span[i];
        a.stride[i] = p.stride[i];
        a.out[i] = static_cast<uint64_t *>(out.back().values->ptr);
    }
    if (G) launch(ctx, "group_keys_decode", group_keys_decode_kernel, dim3(unsigned(stream_grid(ctx, G, GK_THREADS))), dim3(GK_THREADS), 0, a);
    return out;
}

// [keys, aggregates] sorted ascending by the key columns: nqe_sort_execute's order with default options
std::unique_ptr<nqe_table> sorted_by_keys(nqe_ctx *ctx, const nqe_table &t, int k) {
    nqe_sort_key sk[gk::MAX_KEYS];
    for (int i = 0; i < k; ++i) sk[i] = nqe_sort_key{i, 0, 1};
    nqe_table *sorted = nullptr;
    const nqe_status st = nqe_sort_execute(ctx, &t, sk, k, -1, &sorted);
    if (st != NQE_OK) fail(st, ctx->last_error);
    return std::unique_ptr<nqe_table>(sorted);
}

void run_group_aggregate(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int32_t pred_nodes, const nqe_expr_node *group_nodes,
                         const int32_t *group_offsets, int32_t num_keys, const nqe_aggregate *aggs, int32_t num_aggs, nqe_table **out) {
    // ---- everything that can be refused is refused here, before any launch
    check_aggregates(in, aggs, num_aggs);
    const bool has_pred = pred && pred_nodes > 0;
    std::vector<ExprInfo> kinfo;
    std::vector<bool> bare;
    bool keys_may_fault = false, all_integer = true;
    for (int32_t i = 0; i < num_keys; ++i) {
        const nqe_expr_node *kn = group_nodes + group_offsets[i];
        const int len = group_offsets[i + 1] - group_offsets[i];
        kinfo.push_back(analyze_expr(in, kn, len));
        bare.push_back(len == 1 && kn[0].kind == NQE_EXPR_COLUMN);
        const int dt = kinfo.back().out_dtype;
        if (dt != NQE_INT64 && dt != NQE_UINT64 && dt != NQE_UTF8) // aggregate/mod.rs:217
            fail(NQE_ERR_NOT_SUPPORTED, "group by only support by `Int64`, `UInt64`, `String`");
        if (dt == NQE_UTF8 && !bare.back()) fail(NQE_ERR_NOT_SUPPORTED, "group by: a Utf8 key must be a bare column");
        all_integer = all_integer && dt != NQE_UTF8;
        keys_may_fault = keys_may_fault || (!bare.back() && kinfo.back().may_fault);
    }
    if (has_pred && analyze_expr(in, pred, pred_nodes).out_dtype != NQE_BOOLEAN)
        fail(NQE_ERR_NOT_SUPPORTED, "predicate is not a BooleanArray (selection.rs:61 unwrap panics)");

    auto result = std::make_unique<nqe_table>();
    result->ctx = ctx;

    // ---- one integer key: the existing call, its tier included
    if (num_keys == 1 && all_integer) {
        TableGuard aggr, keys;
        const nqe_status st = nqe_aggregate_execute(ctx, in, pred, pred_nodes, group_nodes + group_offsets[0], group_offsets[1] - group_offsets[0], aggs, num_aggs, &aggr.t, &keys.t);
        if (st != NQE_OK) fail(st, ctx->last_error);
        if (!keys.t || keys.t->cols.size() != 1) fail(NQE_ERR_OTHERS, "group by: the aggregate returned no key column");
        result->rows = aggr.t->rows;
        result->cols.push_back(without_validity(keys.t->cols[0]));
        for (const DevColumn &c : aggr.t->cols) result->cols.push_back(c);
        *out = result.release(); // (the aggregate leaves integer keys sorted)
        return;
    }

    // ---- a key that can fault sees only the rows the filter keeps
    if (has_pred && keys_may_fault) {
        TableGuard sel;
        nqe_status st = nqe_selection_execute(ctx, in, pred, pred_nodes, &sel.t);
        if (st != NQE_OK) fail(st, ctx->last_error);
        run_group_aggregate(ctx, sel.t, nullptr, 0, group_nodes, group_offsets, num_keys, aggs, num_aggs, out);
        return;
    }

    // ---- the key columns
    const int64_t n = in->rows;
    std::vector<DevColumn> keys;
    if (keys_may_fault) flags_reset(ctx);
    for (int32_t i = 0; i < num_keys; ++i) {
        const nqe_expr_node *kn = group_nodes + group_offsets[i];
        if (bare[size_t(i)]) keys.push_back(in->cols[size_t(kn[0].column)]);
        else keys.push_back(evaluate_expr(ctx, in, kn, group_offsets[i + 1] - group_offsets[i]));
    }
    if (keys_may_fault) throw_on_flags(ctx); // what nqe_expr_evaluate reports

    // ---- tuple → code
    gk::PackPlan plan;
    DevColumn codes;
    BufRef dict_slots;
    if (n == 0) {
        codes = make_code_column(ctx, 0, false);
        if (all_integer) { // (an empty packed plan: the decode below writes nothing)
            plan.k = num_keys;
            plan.packed = true;
        }
    } else {
        if (all_integer) {
            const GkCols c = cols_of(keys, n);
            bool vec = true;
            for (int i = 0; i < num_keys; ++i) vec = vec && aligned16(c.words[i]);
            plan = measure_and_plan(ctx, keys, c, vec);
            if (plan.packed) codes = pack_codes(ctx, c, plan, vec);
        }
        if (!plan.packed) codes = dict_codes(ctx, keys, n, &dict_slots);
    }

    // ---- the existing aggregate over `in` + the code column, grouped by the bare code column
    nqe_table with_code;
    with_code.ctx = ctx;
    with_code.rows = n;
    with_code.cols = in->cols;
    with_code.cols.push_back(codes);
    // what the context remembers of a query shape is keyed by the table's identity: `in`'s, so that repeated executions over one table
    // find the tier they ended in (only ever a starting point, aggregate_memo.hpp) instead of filling the memo with one-off shapes
    with_code.uid = in->uid;
    nqe_expr_node gnode;
    std::memset(&gnode, 0, sizeof(gnode));
    gnode.kind = NQE_EXPR_COLUMN;
    gnode.column = int32_t(in->cols.size());
    TableGuard aggr, gcodes;
    const nqe_status st = nqe_aggregate_execute(ctx, &with_code, pred, pred_nodes, &gnode, 1, aggs, num_aggs, &aggr.t, &gcodes.t);
    if (st != NQE_OK) fail(st, ctx->last_error);
    if (!gcodes.t || gcodes.t->cols.size() != 1) fail(NQE_ERR_OTHERS, "group by: the aggregate returned no key column");
    const DevColumn &gc = gcodes.t->cols[0];
    const int64_t G = gc.length;

    // ---- codes of the groups → key columns
    result->rows = G;
    if (plan.packed) {
        for (DevColumn &c : decode_codes(ctx, keys, plan, gc)) result->cols.push_back(c);
    } else {
        for (const DevColumn &kc : keys) result->cols.push_back(without_validity(take_column(ctx, kc, reinterpret_cast<const int64_t *>(gc.words()), G)));
    }
    for (const DevColumn &c : aggr.t->cols) result->cols.push_back(c);
    if (!plan.packed && G > 1) result = sorted_by_keys(ctx, *result, num_keys);
    *out = result.release();
}

} // namespace

} // namespace nqe

using namespace nqe;

extern "C" nqe_status nqe_group_aggregate_execute(nqe_ctx *ctx, const nqe_table *in, const nqe_expr_node *pred, int32_t pred_nodes, const nqe_expr_node *group_nodes,
                                                  const int32_t *group_offsets, int32_t num_keys, const nqe_aggregate *aggs, int32_t num_aggs, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !in || !out || (num_aggs > 0 && !aggs)) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (num_keys <= 0) fail(NQE_ERR_PLAN, "group by: the list of keys is empty (the un-grouped form is nqe_aggregate_execute's)");
    if (num_keys > NQE_MAX_GROUP_KEYS) fail(NQE_ERR_NOT_SUPPORTED, "group by: at most " + std::to_string(NQE_MAX_GROUP_KEYS) + " keys");
    if (!group_nodes || !group_offsets || group_offsets[0] < 0) fail(NQE_ERR_INVALID_ARGUMENT, "group by: bad key expressions");
    for (int32_t i = 0; i < num_keys; ++i)
        if (group_offsets[i + 1] <= group_offsets[i]) fail(NQE_ERR_INVALID_ARGUMENT, "group by: the key offsets do not ascend");
    run_group_aggregate(ctx, in, pred, pred_nodes, group_nodes, group_offsets, num_keys, aggs, num_aggs, out);
    NQE_API_END()
}

// No NQE_MODULE_PROBE here: like order_by.hip, this unit's code object is loaded by the first grouped aggregate of a process, not by
// nqe_ctx_create (an eagerly loaded unit cost the headline aggregate 1.3 %: profiles/nested_loop_join/README.md).
