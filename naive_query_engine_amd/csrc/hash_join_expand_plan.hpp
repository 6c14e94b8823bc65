// hash_join_expand_plan.hpp — the column list of the join's count → scan → expand-and-write path (hash_join.hip: probe_expand), for
// both of its entries: the inner probe of a duplicate-key table and the outer probe (quirk Q19, `null_extend`).  Which kernel column
// reads what, where it lands in the output, and whether the write pass may take its PLAIN instance.
// Plain C++17, no HIP and no nqe_table: a side is seen as its column dtypes, which of them have a validity buffer, and (build side)
// which have a copy in sorted-row order, so tests/cpp/test_hash_join_expand_plan.cpp compiles this header alone.
//
// The two entries differ in three places, each marked below:
//   * a plain integer build key is taken from the probe key column.  The inner entry appends it BEHIND the left group — to the
//     kernel it is a probe-side column; the outer entry keeps it in the left column's own place with `from_probe`, because a
//     NULL-extended row must still get the left group's NULL;
//   * the two key columns of the output are one buffer when equal keys are identical bits; the outer entry also needs a batch
//     without NULL-extended rows for that;
//   * a left column of the outer entry gets a validity buffer when the batch holds a NULL-extended row, and the PLAIN rules differ.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/nqe.h"
#include "expr_shapes.hpp" // is_word_type

namespace nqe {

namespace jx {

struct SideCol {
    int dtype = NQE_INT64;
    bool validity = false;    // the column has a validity buffer
    bool sorted_copy = false; // build side: nqe_join_table::sorted_cols holds the column in sorted-row order
};
struct ExpandSides {
    std::vector<SideCol> left, right; // build side, probe side
    int left_key = 0, right_key = 0;
    int64_t left_rows = 0, right_rows = 0;
    bool direct = false;         // unique build keys: `start` is the build row itself, no sorted copies are read
    bool keys_shareable = false; // share_key_column's verdict on the two key columns
    bool null_extend = false;    // the outer entry
    bool has_null = false;       // outer entry: the batch holds a NULL-extended row
};

enum Source {
    SRC_LEFT = 0,        // build column `index`
    SRC_RIGHT = 1,       // probe column `index`
    SRC_LEFT_ROWID = 2,  // the build row numbers (the reference's outer_pos): feeds the Utf8 `take` of the build side
    SRC_RIGHT_ROWID = 3, // the probe row numbers (inner_pos)
    SRC_PROBE_KEY = 4,   // the probe key column standing in for the build key
};
constexpr int SLOT_OUTER_POS = -1, SLOT_INNER_POS = -2; // out_slot of the two row-number columns

struct ExpandCol {
    Source source = SRC_LEFT;
    int index = -1;         // column of its side (SRC_LEFT / SRC_RIGHT)
    int dtype = NQE_INT64;  // of the source as the kernel reads it
    int out_slot = 0;       // output column, or SLOT_OUTER_POS / SLOT_INNER_POS
    bool src_validity = false;
    bool by_pos = false;     // left column read from its sorted copy at start + match number
    bool from_probe = false; // left column read at the probe row (outer entry's key)
    uint64_t null_word = 0;  // what a NULL-extended row holds: 0, -1 for a take index
    bool validity = false;   // the output column gets a validity buffer
};
struct ExpandPlan {
    std::vector<ExpandCol> cols;
    int n_left = 0;          // cols[0, n_left) are addressed through the build side
    bool need_perm = false;  // some left column is addressed by build row
    bool key_shared = false; // output column left_key is output column left.size() + right_key, one buffer
    bool plain = false;      // the write pass takes its PLAIN instance
};

inline ExpandPlan plan_expand(const ExpandSides &s) {
    ExpandPlan p;
    const SideCol &lk = s.left[size_t(s.left_key)];
    bool utf8_left = false, utf8_right = false;
    for (auto &c : s.left) utf8_left |= c.dtype == NQE_UTF8;
    for (auto &c : s.right) utf8_right |= c.dtype == NQE_UTF8;
    const bool key_shortcut = lk.dtype != NQE_UTF8 && !lk.validity;
    p.key_shared = key_shortcut && s.keys_shareable && !(s.null_extend && s.has_null);
    auto side_col = [](Source src, int i, const SideCol &c, int slot) {
        ExpandCol e;
        e.source = src;
        e.index = i;
        e.dtype = c.dtype;
        e.out_slot = slot;
        e.src_validity = c.validity;
        return e;
    };
    auto rowid = [](Source src, int slot) {
        ExpandCol e;
        e.source = src;
        e.out_slot = slot;
        return e;
    };
    ExpandCol probe_key;
    probe_key.source = SRC_PROBE_KEY;
    probe_key.dtype = lk.dtype;
    probe_key.out_slot = s.left_key;
    for (size_t c = 0; c < s.left.size(); ++c) {
        if (s.left[c].dtype == NQE_UTF8) continue; // through outer_pos
        if (key_shortcut && int(c) == s.left_key) {
            if (s.null_extend && !p.key_shared) { // (the outer entry: in the left column's own place)
                probe_key.from_probe = true;
                p.cols.push_back(probe_key);
            }
            continue;
        }
        p.cols.push_back(side_col(SRC_LEFT, int(c), s.left[c], int(c)));
    }
    if (utf8_left) p.cols.push_back(rowid(SRC_LEFT_ROWID, SLOT_OUTER_POS));
    p.n_left = int(p.cols.size());
    if (key_shortcut && !p.key_shared && !s.null_extend) p.cols.push_back(probe_key); // (the inner entry: behind the left group)
    for (size_t c = 0; c < s.right.size(); ++c)
        if (s.right[c].dtype != NQE_UTF8) p.cols.push_back(side_col(SRC_RIGHT, int(c), s.right[c], int(s.left.size() + c)));
    if (utf8_right) p.cols.push_back(rowid(SRC_RIGHT_ROWID, SLOT_INNER_POS));
    // left columns with a copy in sorted-row order are read at start + match number: the matches of a probe row are adjacent words
    for (int k = 0; k < p.n_left; ++k) {
        ExpandCol &e = p.cols[size_t(k)];
        if (e.from_probe) continue;
        if (!s.direct && e.source == SRC_LEFT && s.left[size_t(e.index)].sorted_copy) e.by_pos = true;
        else p.need_perm = true;
    }
    p.plain = true;
    for (size_t k = 0; k < p.cols.size(); ++k) {
        ExpandCol &e = p.cols[k];
        const bool left = int(k) < p.n_left, take_index = e.out_slot < 0;
        // the NULL of a take index is -1, not a validity bit
        e.validity = e.src_validity || (s.null_extend && left && s.has_null && !take_index);
        e.null_word = s.null_extend && take_index ? ~0ull : 0ull;
        p.plain = p.plain && is_word_type(e.dtype) && !e.src_validity;
        // the inner entry's PLAIN instance loads source row 0 for its dead lanes without a branch: no source may be empty.  (The
        // outer entry's reads nothing without a match, and its left columns may have a validity byte array on PLAIN.)
        if (!s.null_extend) p.plain = p.plain && (left ? s.left_rows : s.right_rows) > 0;
    }
    return p;
}

} // namespace jx

} // namespace nqe
