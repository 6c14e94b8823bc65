// join_keys_state.hpp — what a join table built on several keys (quirk Q21, join_keys.hip) remembers of its key tuple, and the doors
// hash_join.hip opens for that unit.  Such a table is an ordinary join table over `left` + one hidden Int64 code column (its LAST
// column, and its key); nqe_join_table::keys is null for a table built on one key.
#pragma once
#include <memory>
#include <vector>

#include "group_keys_plan.hpp"
#include "nqe_internal.hpp"

namespace nqe {

constexpr int JOIN_MAX_COLS = 32; // columns of a join's output (the argument blocks of its kernels); the hidden code columns count

struct JoinKeysState {
    int k = 0;                         // key pairs (>= 2)
    bool packed = false;               // plan (true) or the tuple dictionary (false) gives the codes
    gk::PackPlan plan;                 // over the build key columns
    BufRef dict_slots;                 // group_keys_dict's finished slot table
    uint32_t dict_cap = 0;
    int32_t dict_shift = 0;
    std::vector<DevColumn> build_keys; // the build key columns, in pair order (the dictionary's representatives are rows of these)
};

// ---- hash_join.hip, for join_keys.hip
// check_key_types of the single-key join (rdt < 0: the build side alone)
void join_check_key_types(int ldt, int rdt);
// build_table over `left_with_code`, keyed by its last column; the table keeps `keys`
nqe_join_table *join_build_coded(nqe_ctx *ctx, const nqe_table *left_with_code, std::shared_ptr<const JoinKeysState> keys);
const JoinKeysState *join_table_keys(const nqe_join_table *jt);
// the table's columns, the hidden one included
size_t join_table_columns(const nqe_join_table *jt);
// the flag and marks checks of nqe_hash_join_probe_outer; launches nothing
void join_check_outer_args(nqe_ctx *ctx, const nqe_join_table *jt, uint32_t flags, const nqe_join_marks *marks);
// probe_table (flags == 0 and no marks) or probe_outer over `right_with_code`, keyed by its last column
nqe_table *join_probe_coded(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right_with_code, uint32_t flags, nqe_join_marks *marks);
// ---- semi and anti joins (quirk Q22)
// the flag and marks checks of nqe_hash_join_probe_semi; launches nothing
void join_check_semi_args(nqe_ctx *ctx, const nqe_join_table *jt, uint32_t flags, const nqe_join_marks *marks);
// the column the table is keyed by (the hidden code column of a table built on several keys)
const DevColumn &join_table_key_column(const nqe_join_table *jt);
// probe_semi over `right_with_key`: its last column is the key to look up (the key column again, or the code column), its first
// `out_cols` columns are compacted into the result.  `key_valid`: NQE_MAX_JOIN_KEYS validity bitmaps of the probe key columns (null
// entries: all valid) when NULL keys match nothing, else null.  `want_out` false: the mark-only pass, returns null
nqe_table *join_semi_coded(nqe_ctx *ctx, const nqe_join_table *jt, const nqe_table *right_with_key, size_t out_cols, uint32_t flags, const uint8_t *const *key_valid,
                           nqe_join_marks *marks, bool want_out);

} // namespace nqe
