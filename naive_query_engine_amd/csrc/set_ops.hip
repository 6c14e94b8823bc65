// set_ops.hip — SELECT DISTINCT, UNION, INTERSECT and EXCEPT as operators (quirk Q24; the reference has none of them: its JoinType is
// {Inner, Left, Right, Cross} and its SQL planner knows no DISTINCT and no set operator).  The definition — tuple equality with
// NULL = NULL, -0.0 = +0.0 and one NaN, the first occurrence, the output order — is in include/nqe.h.
//
// One open-addressing SET TABLE serves all four (kernels: set_ops_kernels.hpp; checks, hash and capacity rule, plain C++ checked on the
// CPU: set_ops_plan.hpp):
//
//   set_table_init   cap = the power of two >= 2 n slots of {representative row, first row}; the marks for INTERSECT / EXCEPT
//   set_insert       every row of `in` / `left` / concat(left, right): find or claim the tuple's slot, lower its `first`, remember the slot
//   set_find         INTERSECT / EXCEPT: every row of `right` looks its tuple up and marks the slot
//   set_keep         bit i of the selection's keep mask = first[slot_of[i]] == i (and / and not the mark), plus the per-tile counts
//   finish_mask, compact_column (selection.hip) over the caller's own columns, as the semi join does: every payload dtype works
//
// Two instantiations of insert and find: WORDS<K> for 1..4 non-nullable Int64 / UInt64 keys (a row's K loads issue together, equality
// is K word compares), GENERAL for everything else (per-dtype canonical word, validity compared first, bytes under a NULL never read).
// UNION is nqe_table_concat, then the distinct path over every column.
//
// Out of scope: INTERSECT ALL and EXCEPT ALL (multiplicities); count(distinct x); DISTINCT over expressions at the C ABI (the mirrors
// make temporary columns, as the window plan does); SQL parsing (run_sql stays as it is); sharded forms.
#include <memory>
#include <vector>

#include "device_utils.hpp"
#include "nqe_internal.hpp"
#include "set_ops_kernels.hpp"
#include "set_ops_plan.hpp"

namespace nqe {

namespace {

struct TableView { // what the plan header sees of a table
    std::vector<int> dtypes;
    std::unique_ptr<bool[]> nullable;
    explicit TableView(const nqe_table *t) {
        const size_t nc = t ? t->cols.size() : 0;
        nullable.reset(new bool[nc + 1]);
        for (size_t c = 0; c < nc; ++c) {
            dtypes.push_back(t->cols[c].dtype);
            nullable[c] = t->cols[c].validity && t->cols[c].null_count != 0;
        }
    }
};

void fill_keys(const nqe_table *t, const std::vector<int32_t> &keys, SetKeys *general, SetWords *words) {
    std::memset(general, 0, sizeof(*general));
    std::memset(words, 0, sizeof(*words));
    for (size_t k = 0; k < keys.size(); ++k) {
        const DevColumn &c = t->cols[size_t(keys[k])];
        SetKeyCol &kc = general->key[k];
        kc.dtype = c.dtype;
        kc.values = c.values ? c.values->ptr : nullptr;
        kc.data = c.data ? static_cast<const uint8_t *>(c.data->ptr) : nullptr;
        kc.valid = c.null_count == 0 ? nullptr : c.valid();
        if (k < size_t(setop::MAX_WORD_KEYS)) words->w[k] = c.words();
    }
}

template <bool INSERT>
void launch_probe(nqe_ctx *ctx, const setop::Instance &inst, int32_t num_keys, const SetKeys &own_g, const SetWords &own_w, const SetKeys &rep_g, const SetWords &rep_w, int64_t n,
                  const SetTable &t, uint32_t *slot_of) {
    const char *label = INSERT ? "set_insert" : "set_find";
    const dim3 grid(unsigned(stream_grid(ctx, n, SET_THREADS))), block(SET_THREADS);
    if (inst.form == setop::FORM_WORDS) {
        switch (inst.k) {
#define NQE_SET_CASE(K) case K: launch(ctx, label, set_probe_words_kernel<K, INSERT>, grid, block, 0, own_w, rep_w, n, t, slot_of); return;
            NQE_SET_CASE(1) NQE_SET_CASE(2) NQE_SET_CASE(3) NQE_SET_CASE(4)
#undef NQE_SET_CASE
        default: fail(NQE_ERR_OTHERS, "set table: no WORDS instance for this key count");
        }
    }
    launch(ctx, label, set_probe_general_kernel<INSERT>, grid, block, 0, own_g, rep_g, num_keys, n, t, slot_of);
}

// The rows of `in` that are the first of their tuple over `keys`; with `probe` (INTERSECT: mode 1, EXCEPT: mode 2) those whose tuple
// occurs / does not occur among the rows of `probe` (the same key positions).  Every column of `in`, compacted.
std::unique_ptr<nqe_table> run_set_table(nqe_ctx *ctx, const nqe_table *in, const std::vector<int32_t> &keys, const nqe_table *probe, int mode) {
    const int64_t n = in->rows;
    const int32_t num_keys = int32_t(keys.size());
    KeepMask km;
    km.n = n;
    km.ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    km.keep = dev_alloc(ctx, size_t((n + 63) / 64) * 8 + 8);
    BufRef counts = dev_alloc(ctx, size_t(km.ntiles + 1) * 4);
    BufRef slots, marks, slot_of; // (released after the sync below)
    if (n > 0) {
        TableView view(in);
        const setop::Instance inst = setop::choose_instance(view.dtypes.data(), view.nullable.get(), keys.data(), num_keys);
        const uint64_t cap = setop::table_capacity(n);
        SetTable t;
        std::memset(&t, 0, sizeof(t));
        slots = dev_alloc(ctx, size_t(cap) * 8);
        const uint64_t mark_words = mode ? (cap + 7) / 8 : 0;
        if (mode) marks = dev_alloc(ctx, size_t(mark_words) * 8);
        slot_of = dev_alloc(ctx, size_t(n) * 4);
        t.slots = static_cast<uint32_t *>(slots->ptr);
        t.marks = marks ? static_cast<uint8_t *>(marks->ptr) : nullptr;
        t.mask = uint32_t(cap - 1);
        t.shift = setop::table_shift(cap);
        launch(ctx, "set_table_init", set_table_init_kernel, dim3(unsigned(stream_grid(ctx, int64_t(cap), SET_THREADS))), dim3(SET_THREADS), 0,
               static_cast<unsigned long long *>(slots->ptr), cap, marks ? static_cast<unsigned long long *>(marks->ptr) : nullptr, mark_words);
        SetKeys in_g;
        SetWords in_w;
        fill_keys(in, keys, &in_g, &in_w);
        launch_probe<true>(ctx, inst, num_keys, in_g, in_w, in_g, in_w, n, t, static_cast<uint32_t *>(slot_of->ptr));
        if (mode && probe->rows > 0) {
            // the probed side takes the WORDS form only when it qualifies too (a nullable Int64 column on the right against a
            // non-nullable one on the left): otherwise both sides are read through the general form, same hash, same table
            TableView pview(probe);
            setop::Instance pinst = setop::choose_instance(pview.dtypes.data(), pview.nullable.get(), keys.data(), num_keys);
            if (inst.form != setop::FORM_WORDS) pinst = setop::Instance{};
            SetKeys p_g;
            SetWords p_w;
            fill_keys(probe, keys, &p_g, &p_w);
            launch_probe<false>(ctx, pinst, num_keys, p_g, p_w, in_g, in_w, probe->rows, t, nullptr);
        }
        const dim3 grid(unsigned(stream_grid(ctx, km.ntiles, SET_THREADS / 64))), block(SET_THREADS);
        uint64_t *kp = static_cast<uint64_t *>(km.keep->ptr);
        uint32_t *cp = static_cast<uint32_t *>(counts->ptr);
        const uint32_t *so = static_cast<const uint32_t *>(slot_of->ptr);
        if (mode == 1) launch(ctx, "set_keep", set_keep_kernel<1>, grid, block, 0, so, n, km.ntiles, t, kp, cp);
        else if (mode == 2) launch(ctx, "set_keep", set_keep_kernel<2>, grid, block, 0, so, n, km.ntiles, t, kp, cp);
        else launch(ctx, "set_keep", set_keep_kernel<0>, grid, block, 0, so, n, km.ntiles, t, kp, cp);
    }
    km = finish_mask(ctx, km, counts);
    auto out = std::make_unique<nqe_table>();
    out->ctx = ctx;
    out->rows = km.total;
    for (const DevColumn &c : in->cols) out->cols.push_back(compact_column(ctx, c, km));
    if (!count_nulls_exact(ctx, out.get(), "set_null_count")) sync(ctx); // (either way the stream is drained: the table, the slot list and the mask are released on return)
    return out;
}

} // namespace

} // namespace nqe

using namespace nqe;

extern "C" {

nqe_status nqe_distinct_execute(nqe_ctx *ctx, const nqe_table *in, const int32_t *cols, int32_t num_cols, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    TableView view(in);
    const std::vector<int32_t> keys = setop::plan_distinct(ctx != nullptr, in != nullptr, out != nullptr, view.dtypes.data(), int32_t(view.dtypes.size()), in ? in->rows : 0, cols, num_cols);
    *out = run_set_table(ctx, in, keys, nullptr, 0).release();
    NQE_API_END()
}

nqe_status nqe_set_op_execute(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, int32_t op, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    TableView lv(left), rv(right);
    const std::vector<int32_t> keys = setop::plan_set_op(ctx != nullptr, left != nullptr, right != nullptr, out != nullptr, op, lv.dtypes.data(), int32_t(lv.dtypes.size()),
                                                         left ? left->rows : 0, rv.dtypes.data(), int32_t(rv.dtypes.size()), right ? right->rows : 0);
    if (op == NQE_SET_UNION) {
        const nqe_table *parts[2] = {left, right};
        nqe_table *both = nullptr;
        const nqe_status s = nqe_table_concat(ctx, parts, 2, &both); // (its own error text is already in the context)
        if (s != NQE_OK) return s;
        std::unique_ptr<nqe_table> guard(both);
        *out = run_set_table(ctx, both, keys, nullptr, 0).release();
    } else {
        *out = run_set_table(ctx, left, keys, right, op == NQE_SET_INTERSECT ? 1 : 2).release();
    }
    NQE_API_END()
}

} // extern "C"

// No NQE_MODULE_PROBE here: like order_by.hip, window.hip and nested_loop_join.hip, this unit's code object is loaded by the first
// DISTINCT or set operation of a process, not by nqe_ctx_create (an eagerly loaded unit cost the headline aggregate 1.3 %:
// profiles/nested_loop_join/README.md).
