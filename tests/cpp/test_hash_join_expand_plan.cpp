// The column list of the join's expand path (csrc/hash_join_expand_plan.hpp) on the CPU: this file includes that header alone.  The
// expected lists are written out by hand, per entry (inner probe of a duplicate-key table / outer probe), in the notation of show():
//   <source><column>@<output slot> + p (by_pos) f (from_probe) v (validity buffer) n (null_word = -1)
//   sources: L build column, R probe column, K the probe key standing in for the build key, LR / RR the row-number columns
#include <cstdio>
#include <string>

#include "hash_join_expand_plan.hpp"

using namespace nqe;
using namespace nqe::jx;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::string show(const ExpandPlan &p) {
    std::string s;
    for (size_t k = 0; k < p.cols.size(); ++k) {
        const ExpandCol &e = p.cols[k];
        if (int(k) == p.n_left) s += "| ";
        const char *src[] = {"L", "R", "LR", "RR", "K"};
        s += src[e.source];
        if (e.source == SRC_LEFT || e.source == SRC_RIGHT) s += std::to_string(e.index);
        s += "@" + std::to_string(e.out_slot);
        if (e.by_pos) s += "p";
        if (e.from_probe) s += "f";
        if (e.validity) s += "v";
        if (e.null_word == ~0ull) s += "n";
        else if (e.null_word != 0) s += "?";
        s += " ";
    }
    if (int(p.cols.size()) == p.n_left) s += "| ";
    s += std::string(p.need_perm ? "perm " : "") + (p.key_shared ? "shared " : "") + (p.plain ? "plain" : "general");
    return s;
}
#define EXPECT(sides, text)                                                                        \
    do {                                                                                           \
        const std::string got = show(plan_expand(sides));                                          \
        if (got != (text)) {                                                                       \
            std::printf("FAILED %s:%d:\n  got      %s\n  expected %s\n", __FILE__, __LINE__, got.c_str(), text); \
            ++failures;                                                                            \
        }                                                                                          \
    } while (0)

static SideCol col(int dtype, bool validity = false, bool sorted_copy = false) {
    SideCol c;
    c.dtype = dtype;
    c.validity = validity;
    c.sorted_copy = sorted_copy;
    return c;
}
static ExpandSides sides(std::vector<SideCol> left, int left_key, std::vector<SideCol> right, int right_key, bool shareable) {
    ExpandSides s;
    s.left = std::move(left);
    s.right = std::move(right);
    s.left_key = left_key;
    s.right_key = right_key;
    s.left_rows = 100;
    s.right_rows = 50;
    s.keys_shareable = shareable;
    return s;
}
static ExpandSides outer(ExpandSides s, bool has_null) {
    s.null_extend = true;
    s.has_null = has_null;
    return s;
}

int main() {
    const int I = NQE_INT64, U = NQE_UINT64, F = NQE_FLOAT64, B = NQE_BOOLEAN, S = NQE_UTF8;

    { // ---- plain integer key, every column plain, the payload has its sorted copy: the shape of the benchmark's duplicate-key join
        ExpandSides s = sides({col(I), col(I, false, true)}, 0, {col(I), col(F)}, 0, true);
        EXPECT(s, "L1@1p | R0@2 R1@3 shared plain");
        EXPECT(outer(s, false), "L1@1p | R0@2 R1@3 shared plain");
        // a NULL-extended row in the batch: the key columns differ (NULL against the probe key), every left column gets validity
        EXPECT(outer(s, true), "K@0fv L1@1pv | R0@2 R1@3 plain");
        // has_null means nothing to the inner entry
        s.has_null = true;
        EXPECT(s, "L1@1p | R0@2 R1@3 shared plain");
    }
    { // ---- the keys cannot share a buffer: the inner entry appends the probe key BEHIND the left group, the outer entry keeps its place
        ExpandSides s = sides({col(U), col(I, false, true)}, 0, {col(U), col(I)}, 0, false);
        EXPECT(s, "L1@1p | K@0 R0@2 R1@3 plain");
        EXPECT(outer(s, false), "K@0f L1@1p | R0@2 R1@3 plain");
        EXPECT(outer(s, true), "K@0fv L1@1pv | R0@2 R1@3 plain");
        CHECK(plan_expand(s).cols[1].dtype == U && plan_expand(outer(s, true)).cols[0].dtype == U); // (the build key's dtype)
        // … as it is when the probe key has a validity buffer (share_key_column refuses): that column is not plain
        s.right[0].validity = true;
        EXPECT(s, "L1@1p | K@0 R0@2v R1@3 general");
        EXPECT(outer(s, false), "K@0f L1@1p | R0@2v R1@3 general");
    }
    { // ---- the key is not column 0
        ExpandSides s = sides({col(I, false, true), col(I)}, 1, {col(I), col(I)}, 1, false);
        EXPECT(s, "L0@0p | K@1 R0@2 R1@3 plain");
        EXPECT(outer(s, true), "L0@0pv K@1fv | R0@2 R1@3 plain");
        s.keys_shareable = true;
        EXPECT(s, "L0@0p | R0@2 R1@3 shared plain");
        EXPECT(outer(s, true), "L0@0pv K@1fv | R0@2 R1@3 plain");
    }
    { // ---- an integer build key WITH validity: no shortcut, the key is gathered by build row like any column without a sorted copy
        ExpandSides s = sides({col(I, true), col(I, false, true)}, 0, {col(I), col(I)}, 0, false);
        EXPECT(s, "L0@0v L1@1p | R0@2 R1@3 perm general");
        EXPECT(outer(s, false), "L0@0v L1@1p | R0@2 R1@3 perm general");
        EXPECT(outer(s, true), "L0@0v L1@1pv | R0@2 R1@3 perm general");
        s.keys_shareable = true; // (share_key_column never says so for such a key; the shortcut rule holds on its own)
        EXPECT(s, "L0@0v L1@1p | R0@2 R1@3 perm general");
    }
    { // ---- Utf8 keys: both key columns go through the row-number columns and the Utf8 take; the take index of a NULL-extended row is -1
        ExpandSides s = sides({col(S), col(I, false, true)}, 0, {col(I), col(S)}, 1, false);
        EXPECT(s, "L1@1p LR@-1 | R0@2 RR@-2 perm plain");
        EXPECT(outer(s, false), "L1@1p LR@-1n | R0@2 RR@-2n perm plain");
        EXPECT(outer(s, true), "L1@1pv LR@-1n | R0@2 RR@-2n perm plain");
    }
    { // ---- Utf8 / Boolean / nullable payloads on either side
        ExpandSides s = sides({col(I), col(B), col(S), col(F, true)}, 0, {col(S), col(B, true), col(I)}, 2, true);
        EXPECT(s, "L1@1 L3@3v LR@-1 | R1@5v R2@6 RR@-2 perm shared general");
        EXPECT(outer(s, false), "L1@1 L3@3v LR@-1n | R1@5v R2@6 RR@-2n perm shared general");
        EXPECT(outer(s, true), "K@0fv L1@1v L3@3v LR@-1n | R1@5v R2@6 RR@-2n perm general");
        // one column kind at a time keeps PLAIN off, for both entries
        for (int kind = 0; kind < 4; ++kind)
            for (int side = 0; side < 2; ++side) {
                ExpandSides t = sides({col(I), col(I, false, true)}, 0, {col(I), col(I)}, 0, true);
                SideCol &c = side ? t.right[1] : t.left[1];
                c = kind == 0 ? col(B) : (kind == 1 ? col(I, true) : (kind == 2 ? col(B, true) : col(F, true)));
                CHECK(!plan_expand(t).plain && !plan_expand(outer(t, false)).plain && !plan_expand(outer(t, true)).plain);
            }
        // … a Utf8 column does not: the kernel sees its row numbers
        ExpandSides t = sides({col(I), col(S)}, 0, {col(I), col(S)}, 0, true);
        EXPECT(t, "LR@-1 | R0@2 RR@-2 perm shared plain");
        EXPECT(outer(t, true), "K@0fv LR@-1n | R0@2 RR@-2n perm plain");
    }
    { // ---- sorted copies: absent (the copy did not fit), or not read because the table is direct
        ExpandSides s = sides({col(I), col(I, false, true), col(F, false, false)}, 0, {col(I)}, 0, true);
        EXPECT(s, "L1@1p L2@2 | R0@3 perm shared plain");
        EXPECT(outer(s, true), "K@0fv L1@1pv L2@2v | R0@3 perm plain");
        s.left[2].sorted_copy = true;
        EXPECT(s, "L1@1p L2@2p | R0@3 shared plain");
        s.direct = true;
        EXPECT(s, "L1@1 L2@2 | R0@3 perm shared plain");
        EXPECT(outer(s, false), "L1@1 L2@2 | R0@3 perm shared plain");
        EXPECT(outer(s, true), "K@0fv L1@1v L2@2v | R0@3 perm plain");
        // a left group of the probe-taken key alone reads nothing through the build side
        ExpandSides k = sides({col(I)}, 0, {col(I), col(I)}, 0, true);
        k.direct = true;
        EXPECT(outer(k, true), "K@0fv | R0@1 R1@2 plain");
        EXPECT(outer(k, false), "| R0@1 R1@2 shared plain");
        EXPECT(k, "| R0@1 R1@2 shared plain");
    }
    { // ---- the 32-column boundary: the kernel's list is never longer than the output
        std::vector<SideCol> l(16, col(I, false, true)), r(16, col(I));
        l[0].sorted_copy = false;
        ExpandSides s = sides(l, 0, r, 0, false);
        CHECK(plan_expand(s).cols.size() == 32 && plan_expand(s).n_left == 15 && plan_expand(s).plain && !plan_expand(s).need_perm);
        CHECK(plan_expand(outer(s, true)).cols.size() == 32 && plan_expand(outer(s, true)).n_left == 16);
        CHECK(plan_expand(s).cols[15].source == SRC_PROBE_KEY && plan_expand(s).cols[15].out_slot == 0 && plan_expand(s).cols[31].out_slot == 31);
        CHECK(plan_expand(outer(s, true)).cols[0].source == SRC_PROBE_KEY && plan_expand(outer(s, true)).cols[0].from_probe);
        s.keys_shareable = true;
        CHECK(plan_expand(s).cols.size() == 31 && plan_expand(outer(s, false)).cols.size() == 31 && plan_expand(outer(s, true)).cols.size() == 32);
        // Utf8 columns on both sides: each side's strings collapse into one row-number column
        l[5] = l[6] = col(S);
        r[7] = r[8] = r[9] = col(S);
        s = sides(l, 0, r, 0, false);
        CHECK(plan_expand(s).cols.size() == 32 - 1 - 2 && plan_expand(s).n_left == 14);
        l[5] = col(I, false, true), r[8] = r[9] = col(I);
        s = sides(l, 0, r, 0, false);
        CHECK(plan_expand(s).cols.size() == 32 && plan_expand(s).n_left == 15 && plan_expand(s).cols[14].out_slot == SLOT_OUTER_POS &&
              plan_expand(s).cols[31].out_slot == SLOT_INNER_POS);
    }
    { // ---- the PLAIN verdict and empty sources: the inner entry's PLAIN instance loads source row 0 for dead lanes, so no source of
      // its list may be empty; the outer entry's reads nothing without a match and keeps PLAIN
        ExpandSides s = sides({col(I), col(I, false, true)}, 0, {col(I), col(I)}, 0, true);
        s.left_rows = 0;
        EXPECT(s, "L1@1p | R0@2 R1@3 shared general");
        EXPECT(outer(s, true), "K@0fv L1@1pv | R0@2 R1@3 plain");
        s.left_rows = 100, s.right_rows = 0;
        EXPECT(s, "L1@1p | R0@2 R1@3 shared general");
        EXPECT(outer(s, false), "L1@1p | R0@2 R1@3 shared plain");
        // an empty build side whose columns the list does not read (the shared key, and nothing else on the left)
        ExpandSides k = sides({col(I)}, 0, {col(I)}, 0, true);
        k.left_rows = 0;
        EXPECT(k, "| R0@1 shared plain");
        k.keys_shareable = false; // (the probe key stands behind the left group: a probe-side source)
        EXPECT(k, "| K@0 R0@1 plain");
        // the row-number column of an empty side is an empty source too
        ExpandSides u = sides({col(I), col(S)}, 0, {col(I)}, 0, true);
        u.left_rows = 0;
        EXPECT(u, "LR@-1 | R0@2 perm shared general");
    }
    if (failures) return 1;
    std::printf("hash join expand plan ok\n");
    return 0;
}
