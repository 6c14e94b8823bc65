// join_keys.hip — the hash join on several keys (quirk Q21; the reference's DataFrame::join zips every key pair into `on`,
// logical_plan/dataframe.rs:109, and HashJoin::execute reads on[0] alone, hash_join.rs:134, :171).  Composition, not a new join: the
// key tuple of a row becomes ONE Int64 code, the existing join of hash_join.hip — build tiers, inner probe tiers, the outer path,
// marks — runs over each table with its code column appended as the last column and the key, and the two code columns are dropped from
// the result (the output shares every other buffer).  GROUP BY on several keys (group_keys.hip) makes its codes the same way; what a
// join adds is that two tables must agree on one code space, and that a probe tuple may be one the build side has never seen.
//
//   one pair         forwards to nqe_hash_join_build / _probe / _probe_outer: a single key keeps its build and probe tiers.
//   packed path      every pair Int64 / UInt64 and the product of the BUILD key columns' spans at most 2^62 (group_keys_plan.hpp):
//                    build: group_keys_ranges (one read-back) → group_keys_pack;  probe: join_keys_pack_probe under the build's plan —
//                    a tuple with a key outside its build range gets JOIN_KEYS_NO_MATCH (join_keys_plan.hpp).
//   dictionary path  a Utf8 pair anywhere, or spans whose product overflows (NQE_JOIN_KEYS_FORCE_DICT=1, read per build call, sends
//                    an all-integer tuple here too: same result): build: group_keys_dict, code = representative build row, the slot
//                    table stays alive in the join table;  probe: join_keys_lookup, find-only over that table.
//
// The semi / anti probe (quirk Q22, nqe_hash_join_probe_semi: one door for tables built on one key and on several) composes the same way:
// the probe codes — or the one key column again — ride as the last column into hash_join.hip's probe_semi, which compacts the caller's
// columns alone.
//
// No validity buffer is read anywhere (the semi probe's NQE_SEMI_NULL_KEY_UNMATCHED apart): the hash join compares raw slots (quirk
// Q11), at every key position.  An EMPTY build side takes the packed path with spans of 0 (integer pairs) or an empty dictionary (a
// Utf8 pair): every probe row gets JOIN_KEYS_NO_MATCH.
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "group_keys_host.hpp"
#include "join_keys_kernels.hpp"
#include "join_keys_state.hpp"

static_assert(NQE_MAX_JOIN_KEYS == nqe::gk::MAX_KEYS, "the header and the plan agree on the key count");

namespace nqe {

namespace {

// ---- everything that can be refused without looking at the data; nothing here launches or allocates
void check_key_count(int32_t num_keys) {
    if (num_keys <= 0) fail(NQE_ERR_PLAN, "Inner Join on Conditions can't not be empty"); // hash_join.rs:125-129
    if (num_keys > NQE_MAX_JOIN_KEYS) fail(NQE_ERR_NOT_SUPPORTED, "join: at most " + std::to_string(NQE_MAX_JOIN_KEYS) + " key pairs");
}
const DevColumn &key_column(const nqe_table *t, int32_t idx) {
    if (idx < 0 || size_t(idx) >= t->cols.size()) fail(NQE_ERR_LOGICAL, "ColumnExpr must has name or idx");
    return t->cols[size_t(idx)];
}
void check_build_keys(const nqe_table *left, const int32_t *left_keys, int32_t k) {
    for (int32_t i = 0; i < k; ++i) join_check_key_types(key_column(left, left_keys[i]).dtype, -1);
    if (k > 1 && left->cols.size() + 1 > size_t(JOIN_MAX_COLS)) fail(NQE_ERR_NOT_SUPPORTED, "join output wider than 32 columns");
}
// `build_dtypes`: the build key columns' types, in pair order; `build_cols`: the build side's columns without the hidden one
void check_probe_keys(const int *build_dtypes, size_t build_cols, const nqe_table *right, const int32_t *right_keys, int32_t k) {
    for (int32_t i = 0; i < k; ++i) join_check_key_types(build_dtypes[i], key_column(right, right_keys[i]).dtype);
    if (k > 1 && build_cols + right->cols.size() + 2 > size_t(JOIN_MAX_COLS)) fail(NQE_ERR_NOT_SUPPORTED, "join output wider than 32 columns (a join on several keys adds two hidden ones)");
}

bool all_aligned16(const std::vector<DevColumn> &keys) {
    bool a = true;
    for (const DevColumn &c : keys) a = a && aligned16(c.words());
    return a;
}

// ---- build side: left + the code column → the existing build
nqe_join_table *build_keys(nqe_ctx *ctx, const nqe_table *left, const int32_t *left_keys, int32_t k) {
    const int64_t n = left->rows;
    auto st = std::make_shared<JoinKeysState>();
    st->k = k;
    bool all_integer = true;
    for (int32_t i = 0; i < k; ++i) {
        st->build_keys.push_back(left->cols[size_t(left_keys[i])]);
        all_integer = all_integer && st->build_keys.back().dtype != NQE_UTF8;
    }
    const bool force_dict = getenv("NQE_JOIN_KEYS_FORCE_DICT") != nullptr;
    DevColumn codes;
    if (n == 0) {
        codes = make_code_column(ctx, 0, false);
        st->packed = all_integer && !force_dict;
        if (st->packed) st->plan = jk::empty_build_plan(k);
        else { // an empty dictionary
            st->dict_cap = dict_capacity(0, &st->dict_shift);
            st->dict_slots = dev_alloc(ctx, size_t(st->dict_cap) * 8);
            launch(ctx, "group_keys_dict_init", group_keys_fill_kernel, dim3(1), dim3(GK_THREADS), 0, static_cast<long long *>(st->dict_slots->ptr), GK_EMPTY, int64_t(st->dict_cap));
        }
    } else {
        if (all_integer && !force_dict) {
            const GkCols c = cols_of(st->build_keys, n, false);
            const bool vec = all_aligned16(st->build_keys);
            st->plan = measure_and_plan(ctx, st->build_keys, c, vec);
            st->packed = st->plan.packed;
            if (st->packed) codes = pack_codes(ctx, c, st->plan, vec);
        }
        if (!st->packed) {
            codes = dict_codes(ctx, st->build_keys, n, &st->dict_slots, false, "join", &st->dict_cap, &st->dict_shift);
        }
    }
    nqe_table with_code;
    with_code.ctx = ctx;
    with_code.rows = n;
    with_code.cols = left->cols;
    with_code.cols.push_back(codes);
    return join_build_coded(ctx, &with_code, st);
}

template <bool VEC> void launch_pack_probe(nqe_ctx *ctx, int k, dim3 grid, const JkPackProbe &a) {
    const dim3 block(GK_THREADS);
    switch (k) {
    case 2: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<2, VEC>, grid, block, 0, a); break;
    case 3: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<3, VEC>, grid, block, 0, a); break;
    case 4: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<4, VEC>, grid, block, 0, a); break;
    case 5: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<5, VEC>, grid, block, 0, a); break;
    case 6: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<6, VEC>, grid, block, 0, a); break;
    case 7: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<7, VEC>, grid, block, 0, a); break;
    default: launch(ctx, "join_keys_pack_probe", join_keys_pack_probe_kernel<8, VEC>, grid, block, 0, a); break;
    }
}

void fill_dict_key(GkDictKey *dk, const DevColumn &c) {
    if (c.dtype == NQE_UTF8) {
        dk->offs = static_cast<const int32_t *>(c.values->ptr);
        dk->data = c.data ? static_cast<const uint8_t *>(c.data->ptr) : nullptr;
    } else
        dk->words = c.words();
}

// ---- probe side: the probe rows' codes in the build side's code space
DevColumn probe_codes(nqe_ctx *ctx, const JoinKeysState &st, const std::vector<DevColumn> &keys, int64_t n) {
    DevColumn codes = make_code_column(ctx, n, false);
    if (n == 0) return codes;
    if (st.packed) {
        JkPackProbe a;
        std::memset(&a, 0, sizeof(a));
        for (int i = 0; i < st.k; ++i) {
            a.words[i] = keys[size_t(i)].words();
            a.min[i] = st.plan.min[i];
            a.span[i] = st.plan.span[i];
            a.stride[i] = st.plan.stride[i];
        }
        a.n = n;
        a.codes = static_cast<uint64_t *>(codes.values->ptr);
        const bool vec = all_aligned16(keys) && aligned16(a.codes);
        const dim3 grid(unsigned(stream_grid(ctx, vec ? n / 2 : n, GK_THREADS * 2)));
        if (vec) launch_pack_probe<true>(ctx, st.k, grid, a);
        else launch_pack_probe<false>(ctx, st.k, grid, a);
    } else {
        JkLookup a;
        std::memset(&a, 0, sizeof(a));
        a.k = st.k;
        a.n = n;
        for (int i = 0; i < st.k; ++i) {
            fill_dict_key(&a.probe[i], keys[size_t(i)]);
            fill_dict_key(&a.build[i], st.build_keys[size_t(i)]);
        }
        a.slots = static_cast<const long long *>(st.dict_slots->ptr);
        a.cap = st.dict_cap;
        a.shift = st.dict_shift;
        a.codes = static_cast<int64_t *>(codes.values->ptr);
        launch(ctx, "join_keys_lookup", join_keys_lookup_kernel, dim3(unsigned(stream_grid(ctx, n, GK_THREADS))), dim3(GK_THREADS), 0, a);
    }
    return codes;
}

// the existing probe over right + the code column; then the two code columns leave the result (every other buffer is shared)
nqe_table *probe_keys(nqe_ctx *ctx, const nqe_join_table *jt, const JoinKeysState &st, const nqe_table *right, const int32_t *right_keys, uint32_t flags,
                      nqe_join_marks *marks) {
    std::vector<DevColumn> keys;
    for (int i = 0; i < st.k; ++i) keys.push_back(right->cols[size_t(right_keys[i])]);
    nqe_table with_code;
    with_code.ctx = ctx;
    with_code.rows = right->rows;
    with_code.cols = right->cols;
    with_code.cols.push_back(probe_codes(ctx, st, keys, right->rows));
    std::unique_ptr<nqe_table> out(join_probe_coded(ctx, jt, &with_code, flags, marks));
    const size_t left_cols = join_table_columns(jt); // the hidden one included: it is the last of them
    out->cols.pop_back();
    out->cols.erase(out->cols.begin() + std::ptrdiff_t(left_cols) - 1);
    return out.release();
}

// the semi / anti probe (quirk Q22): the caller's columns + the key to look up as the last column — the probe codes of a tuple, or the
// one key column again (an alias, not a copy).  The compaction loops over the caller's columns only: the code column never exists in
// the output.  `st` null: a table built on one key
nqe_table *probe_semi_keys(nqe_ctx *ctx, const nqe_join_table *jt, const JoinKeysState *st, const nqe_table *right, const int32_t *right_keys, int32_t k, uint32_t flags,
                           nqe_join_marks *marks, bool want_out) {
    std::vector<DevColumn> keys;
    const uint8_t *valid[NQE_MAX_JOIN_KEYS] = {};
    for (int i = 0; i < k; ++i) {
        keys.push_back(right->cols[size_t(right_keys[i])]);
        valid[i] = keys.back().valid();
    }
    nqe_table with_key;
    with_key.ctx = ctx;
    with_key.rows = right->rows;
    with_key.cols = right->cols;
    with_key.cols.push_back(st ? probe_codes(ctx, *st, keys, right->rows) : keys[0]);
    return join_semi_coded(ctx, jt, &with_key, right->cols.size(), flags, (flags & NQE_SEMI_NULL_KEY_UNMATCHED) ? valid : nullptr, marks, want_out);
}

void check_status(nqe_ctx *ctx, nqe_status st) {
    if (st != NQE_OK) fail(st, ctx->last_error);
}

} // namespace

} // namespace nqe

using namespace nqe;

extern "C" {

nqe_status nqe_hash_join_build_keys(nqe_ctx *ctx, const nqe_table *left, const int32_t *left_keys, int32_t num_keys, nqe_join_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !left || !left_keys || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    check_key_count(num_keys);
    check_build_keys(left, left_keys, num_keys);
    if (num_keys == 1) check_status(ctx, nqe_hash_join_build(ctx, left, left_keys[0], out));
    else *out = build_keys(ctx, left, left_keys, num_keys);
    NQE_API_END()
}

nqe_status nqe_hash_join_probe_keys(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, const int32_t *right_keys, int32_t num_keys, uint32_t flags,
                                    nqe_join_marks *marks, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !right || !right_keys || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    check_key_count(num_keys);
    const JoinKeysState *st = join_table_keys(build);
    if (num_keys != (st ? st->k : 1)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_keys: the join table was built on " + std::to_string(st ? st->k : 1) + " key(s)");
    if (!st) { // one pair: the single-key operators, their tiers included
        if (flags == 0 && !marks) check_status(ctx, nqe_hash_join_probe(ctx, build, right, right_keys[0], out));
        else check_status(ctx, nqe_hash_join_probe_outer(ctx, build, right, right_keys[0], flags, marks, out));
    } else {
        join_check_outer_args(ctx, build, flags, marks);
        int dtypes[NQE_MAX_JOIN_KEYS];
        for (int i = 0; i < st->k; ++i) dtypes[i] = st->build_keys[size_t(i)].dtype;
        check_probe_keys(dtypes, join_table_columns(build) - 1, right, right_keys, num_keys);
        *out = probe_keys(ctx, build, *st, right, right_keys, flags, marks);
    }
    NQE_API_END()
}

nqe_status nqe_hash_join_probe_semi(nqe_ctx *ctx, const nqe_join_table *build, const nqe_table *right, const int32_t *right_keys, int32_t num_keys, uint32_t flags,
                                    nqe_join_marks *marks, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !build || !right || !right_keys) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    if (!out && !marks) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_semi: neither an output nor marks");
    check_key_count(num_keys);
    const JoinKeysState *st = join_table_keys(build);
    if (num_keys != (st ? st->k : 1)) fail(NQE_ERR_INVALID_ARGUMENT, "nqe_hash_join_probe_semi: the join table was built on " + std::to_string(st ? st->k : 1) + " key(s)");
    join_check_semi_args(ctx, build, flags, marks);
    // (no column limit: the columns are compacted one at a time and no build column is written)
    const DevColumn *build_keys[NQE_MAX_JOIN_KEYS];
    for (int i = 0; i < num_keys; ++i) build_keys[i] = st ? &st->build_keys[size_t(i)] : &join_table_key_column(build);
    for (int i = 0; i < num_keys; ++i) key_column(right, right_keys[i]);
    for (int i = 0; i < num_keys; ++i) join_check_key_types(build_keys[i]->dtype, right->cols[size_t(right_keys[i])].dtype);
    if (flags & NQE_SEMI_NULL_KEY_UNMATCHED)
        for (int i = 0; i < num_keys; ++i)
            if (build_keys[i]->validity && build_keys[i]->null_count != 0)
                fail(NQE_ERR_NOT_SUPPORTED, "nqe_hash_join_probe_semi: NQE_SEMI_NULL_KEY_UNMATCHED over a build key column with NULLs (the table would have to be rebuilt without them)");
    nqe_table *t = probe_semi_keys(ctx, build, st, right, right_keys, num_keys, flags, marks, out != nullptr);
    if (out) *out = t;
    NQE_API_END()
}

nqe_status nqe_hash_join_execute_keys(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, const int32_t *left_keys, const int32_t *right_keys, int32_t num_keys,
                                      nqe_table **out) {
    NQE_API_BEGIN(ctx)
    if (!ctx || !left || !right || !left_keys || !right_keys || !out) fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    check_key_count(num_keys);
    check_build_keys(left, left_keys, num_keys);
    int dtypes[NQE_MAX_JOIN_KEYS];
    for (int i = 0; i < num_keys; ++i) dtypes[i] = left->cols[size_t(left_keys[i])].dtype;
    check_probe_keys(dtypes, left->cols.size(), right, right_keys, num_keys);
    if (num_keys == 1) check_status(ctx, nqe_hash_join_execute(ctx, left, right, left_keys[0], right_keys[0], out));
    else {
        struct Guard {
            nqe_join_table *jt = nullptr;
            ~Guard() {
                if (jt) nqe_join_table_release(jt);
            }
        } g;
        g.jt = build_keys(ctx, left, left_keys, num_keys);
        *out = probe_keys(ctx, g.jt, *join_table_keys(g.jt), right, right_keys, 0, nullptr);
    }
    NQE_API_END()
}

} // extern "C"

// No NQE_MODULE_PROBE here: like group_keys.hip, this unit's code object is loaded by the first join on several keys of a process, not by
// nqe_ctx_create.
