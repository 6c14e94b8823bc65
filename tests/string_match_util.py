"""The model of string matching (quirk Q27: NQE_EXPR_STRING_MATCH — like, not_like, ilike, not_ilike, starts_with, ends_with, contains,
strpos) in plain Python over `bytes`, written from the rules in include/nqe.h and not from the kernels: LIKE is decided by the set of
byte positions reachable after every pattern element, not by the greedy walk the device takes.  Also the shared case lists.  The helpers
that move byte strings into Utf8 columns are tests/string_fn_util.py's."""
import functools
import itertools

from tests.string_args_util import character_numbers
from tests.string_fn_util import CONTENTS, FOUR, INVALID, THREE, TWO, model_lower, sized, utf8_column  # noqa: F401 (shared with the tests)

LIKE, NOT_LIKE, ILIKE, NOT_ILIKE, STARTS_WITH, ENDS_WITH, CONTAINS, STRPOS = range(8)
OPERATORS = (LIKE, NOT_LIKE, ILIKE, NOT_ILIKE, STARTS_WITH, ENDS_WITH, CONTAINS, STRPOS)
ANY, ONE = "any", "one"


# ----------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def elements(pattern: bytes) -> list:
    """`\\` + b is the literal b; a `\\` that ends the pattern is a literal; `%` is ANY (a run of them one); `_` is ONE; else a literal"""
    out, i = [], 0
    while i < len(pattern):
        b = pattern[i]
        if b == 0x5C and i + 1 < len(pattern):
            out.append(pattern[i + 1])
            i += 2
            continue
        if b == 0x25:
            if not out or out[-1] != ANY:
                out.append(ANY)
        elif b == 0x5F:
            out.append(ONE)
        else:
            out.append(b)
        i += 1
    return out


@functools.lru_cache(maxsize=None)
def character_ends(s: bytes) -> dict:
    """first byte of every character {j : c(j) = k} -> one past its last byte"""
    c = character_numbers(s)
    starts = [j for j in range(len(s)) if j == 0 or c[j] != c[j - 1]]
    return dict(zip(starts, starts[1:] + [len(s)]))


def model_like(s: bytes, pattern: bytes, fold: bool = False) -> bool:
    """true iff the bytes of s can be cut into consecutive pieces, one per element: the positions reachable behind every element"""
    els = elements(pattern)  # (cached: never changed in place)
    if fold:
        s = model_lower(s)
        els = [model_lower(bytes([e]))[0] if isinstance(e, int) else e for e in els]
    ends = character_ends(s)
    reach = {0}
    for e in els:
        if e == ANY:
            reach = set(range(min(reach), len(s) + 1)) if reach else set()
        elif e == ONE:
            reach = {ends[i] for i in reach if i in ends}
        else:
            reach = {i + 1 for i in reach if i < len(s) and s[i] == e}
    return len(s) in reach


def model_strpos(s: bytes, sub: bytes) -> int:
    if not sub:
        return 1
    j = s.find(sub)
    return 0 if j < 0 else character_numbers(s)[j]


def model(op: int, s: bytes, pattern: bytes):
    if op in (LIKE, NOT_LIKE, ILIKE, NOT_ILIKE):
        return model_like(s, pattern, fold=op in (ILIKE, NOT_ILIKE)) != (op in (NOT_LIKE, NOT_ILIKE))
    if op == STARTS_WITH:
        return s.startswith(pattern)
    if op == ENDS_WITH:
        return s.endswith(pattern)
    if op == CONTAINS:
        return pattern in s
    return model_strpos(s, pattern)


def model_rows(op: int, items, pattern, mask=None):
    """(values, validity): a NULL row — the string's, or every row under a NULL pattern — holds False / 0"""
    n = len(items)
    valid = [pattern is not None and (mask is None or bool(mask[i])) for i in range(n)]
    zero = 0 if op == STRPOS else False
    return [model(op, s, pattern) if ok else zero for s, ok in zip(items, valid)], valid


def greedy_like(s: bytes, pattern: bytes) -> bool:
    """the device's strategy restated: the first segment at 0, every inner segment at its leftmost match at or behind the cursor, the
    last segment ending at the string's end — model_like must agree with it on every input"""
    els = elements(pattern)
    segs, cur = [[]], None
    for e in els:
        if e == ANY:
            segs.append([])
        else:
            segs[-1].append(e)
    has_any = len(segs) > 1
    ends = character_ends(s)

    def match_at(seg, i):
        for e in seg:
            if i >= len(s):
                return -1
            if e == ONE:
                if i not in ends:
                    return -1
                i = ends[i]
            else:
                if s[i] != e:
                    return -1
                i += 1
        return i

    if not has_any:
        return match_at(segs[0], 0) == len(s)
    cur = match_at(segs[0], 0)
    if cur < 0:
        return False
    for seg in segs[1:-1]:
        for i in range(cur, len(s) + 1):
            e = match_at(seg, i)
            if e >= 0:
                cur = e
                break
        else:
            return False
    return any(match_at(segs[-1], i) == len(s) for i in range(cur, len(s) + 1))


# ----------------------------------------------------------------------------- the shared cases
ALPHABET = (b"a", b"b", b"\xa9", b"\xc3", b"%", b"_")  # two letters, a continuation byte, a two-byte lead, and the two wildcards as data


def all_strings(max_symbols: int) -> list:
    """every string of up to max_symbols symbols of the alphabet (9331 for 5)"""
    out = []
    for k in range(max_symbols + 1):
        out += [b"".join(t) for t in itertools.product(ALPHABET, repeat=k)]
    return out


# LIKE patterns covering every form: ALWAYS, EQUAL, PREFIX, SUFFIX, PREFIX_SUFFIX, CONTAINS, GENERAL (ONE, several segments, anchors)
LIKE_PATTERNS = [b"%", b"%%", b"", b"a", b"ab", b"a%", b"ab%", b"%a", b"%ab", b"a%b", b"ab%ba", b"a%a", b"%a%", b"%ab%", b"%\xc3\xa9%", b"_", b"__", b"%_", b"_%", b"_%_", b"%_%",
                 b"a_", b"_a", b"a_b", b"%a_", b"_a%", b"%a%b%", b"%a%b", b"a%b%", b"a%b%a", b"%ab%ba%", b"%a_b%", b"%_a_%", b"\\%", b"\\_", b"%\\%%", b"\\_%", b"%\\_",
                 b"%\xa9", b"\xc3%", b"%\xc3_", b"_\xc3%", b"%b_%a", b"%aa%aa%"]
VERBATIM = [b"", b"a", b"ab", b"%", b"_", b"a%", b"\xa9", b"\xc3\xa9", b"ba", b"aab"]

# (operator, pattern) pairs that are constant over a column by their meaning: the guard of test_string_match_model.py names them
CONSTANT_BY_MEANING = {(LIKE, b"%"), (LIKE, b"%%"), (NOT_LIKE, b"%"), (NOT_LIKE, b"%%"), (ILIKE, b"%"), (ILIKE, b"%%"), (NOT_ILIKE, b"%"), (NOT_ILIKE, b"%%"),
                       (STARTS_WITH, b""), (ENDS_WITH, b""), (CONTAINS, b""), (STRPOS, b"")}


def exhaustive_cases() -> list:
    """(operator, pattern) of the exhaustive slice"""
    out = [(op, p) for op in (LIKE, NOT_LIKE) for p in LIKE_PATTERNS]
    out += [(ILIKE, p) for p in (b"A%", b"%aB%", b"_A%", b"%B", b"a%B%A")]
    out += [(op, p) for op in (STARTS_WITH, ENDS_WITH, CONTAINS, STRPOS) for p in VERBATIM]
    return out


ROW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 257)
ROW_POOL = [b"ab", b"", b"abc", b"xab", b"b", b"a", "é".encode(), b"ba-ab", b"abab", b"zzzzzzzzzzab", b"a\xa9b", b"xa-b"]
ROW_CASES = [(LIKE, b"ab%"), (LIKE, b"%ab"), (LIKE, b"a%b"), (LIKE, b"ab"), (NOT_LIKE, b"ab%"), (LIKE, b"%ab%"), (LIKE, b"a_%"), (NOT_LIKE, b"%a_b%"), (ILIKE, b"%AB"), (STARTS_WITH, b"ab"),
             (ENDS_WITH, b"ab"), (CONTAINS, b"ab"), (STRPOS, b"ab"), (STRPOS, b"b")]

GROUPS = (4, 8, 16, 32, 64)


def group_strings(group: int) -> list:
    """lengths 0, 1, G-1, G, G+1, 2G, 2G+1 with the match `xy` (and `x…y…z` for the two-inner-segment LIKE) wholly in chunk 0, across the
    first chunk edge, in the last partial chunk, or absent"""
    out = []
    for n in (0, 1, group - 1, group, group + 1, 2 * group, 2 * group + 1):
        out.append(b"q" * n)  # absent
        for at in (0, group - 2, group - 1, group, n - 2, n - 3):
            if 0 <= at and at + 2 <= n:
                s = bytearray(b"q" * n)
                s[at:at + 2] = b"xy"
                out.append(bytes(s))
                if at + 3 <= n:
                    s[at + 2:at + 3] = b"z"
                    out.append(bytes(s))
        if n >= 3:
            s = bytearray(b"q" * n)
            s[0], s[n // 2], s[n - 1] = ord("x"), ord("y"), ord("z")
            out.append(bytes(s))
            out.append(("é" * (n // 2)).encode() + b"xy")  # multi-byte characters in front: strpos counts characters
    return out


def wide_group_strings(group: int) -> list:
    """A segment of at most 8 literal bytes is searched 8 positions per lane: a chunk is 8G positions.  Strings of 8G-1, 8G, 8G+1, 16G and
    16G+1 bytes with `xy` / `xyz` wholly in chunk 0, at 8G-2, 8G-1 (across the chunk edge), 8G, and at the end of the last partial
    chunk; `x…y…z` spread over the chunks; two-byte characters in front, so that strpos counts characters in a later chunk; and absent"""
    out, edge = [], 8 * group
    for n in (edge - 1, edge, edge + 1, 2 * edge, 2 * edge + 1):
        out.append(b"q" * n)  # absent
        for at in (3, edge - 3, edge - 2, edge - 1, edge, edge + 1, 2 * edge - 2, 2 * edge - 1, n - 3, n - 2):
            if at + 2 <= n:
                s = bytearray(b"q" * n)
                s[at:at + 2] = b"xy"
                out.append(bytes(s))
                s[0:6] = "ééé".encode()  # (at >= 3 + 3: never over the match, but for at = 3)
                if at >= 6:
                    out.append(bytes(s))
                if at + 3 <= n:
                    s[at + 2:at + 3] = b"z"
                    out.append(bytes(s))
        for ax, ay, az in ((1, edge - 1, edge), (edge - 1, edge, n - 1), (0, edge + 2, n - 1), (edge, edge + 1, edge + 2)):
            if ax < ay < az < n:
                s = bytearray(b"q" * n)
                s[ax], s[ay], s[az] = ord("x"), ord("y"), ord("z")
                out.append(bytes(s))
                s[ay + 1:ay + 2] = b"z" if ay + 1 < n else b""
                out.append(bytes(s))
    return out


def long_group_strings(group: int) -> list:
    """a literal of 3G bytes (the one-position-per-lane walk) at 0, 1, G-1, G+1, followed by nothing or two bytes; too short by one; absent"""
    return [b"q" * k + b"x" * (3 * group) + b"q" * j for k in (0, 1, group - 1, group + 1) for j in (0, 2)] + [b"x" * (3 * group - 1), b"q" * (4 * group)]


def long_group_cases(group: int) -> list:
    return [(CONTAINS, b"x" * (3 * group)), (STRPOS, b"x" * (3 * group)), (LIKE, b"%" + b"_" * (3 * group) + b"qq"), (LIKE, b"%x" + b"_" * (3 * group - 2) + b"x%")]


GROUP_CASES = [(CONTAINS, b"xy"), (STRPOS, b"xy"), (LIKE, b"%x%y%z%"), (LIKE, b"q%x%yz%"), (LIKE, b"%x_z%"), (NOT_LIKE, b"%xy%")]

ONE_PATTERNS = [b"_", b"__", b"%_", b"_%_", b"a_c", "%é_".encode(), b"_%", "é_%".encode(), b"%_\xc3", b"\xa9%_", b"a_____c", b"a_%_c", b"%__"]
ONE_STRINGS = [b"", b"a", b"ab", b"abc", b"a" + TWO + b"c", b"a" + THREE + b"c", b"a" + FOUR + b"c", TWO, THREE, FOUR, TWO + TWO, TWO + b"x", TWO + THREE, b"x" + TWO + FOUR,
               b"\xa9", b"\xa9\xa9a", b"\xa9a", b"\xa9ab", b"\xa9a\xa9c", b"a\xc3", b"\xc3", b"ab\xc3", b"\xa9" * 5, b"a" + b"\xa9" * 5, b"a" + b"\xa9" * 5 + b"c", b"a\xa9c", b"a\xa9\xa9c",
               TWO + b"\xc3", b"ac", b"abcc", b"aXc", b"a" + TWO + b"2" + THREE + b"4" + FOUR + b"c"]

ILIKE_PATTERNS = [b"AB%", b"%ab", b"%B%", b"a_C", "É%".encode(), "%é".encode(), b"[%", b"@%", b"`%", b"{%", b"%Z"]
ILIKE_STRINGS = [b"ab", b"AB", b"Ab", b"aB", b"xAB", b"abc", b"ABC", b"aXc", b"AxC", "É".encode(), "é".encode(), "Éa".encode(), "éa".encode(), b"[", b"{", b"@", b"`", b"@a", b"`a", b"[z",
                 b"{z", b"Z", b"z", b"", b"Q"]

ESCAPE_PATTERNS = [b"\\%", b"\\_", b"\\\\", b"\\a", b"a\\", b"\\", b"%\\%", b"\\%%", b"a\\%b", b"a\\_b", b"%\\\\%", b"\\%\\_"]
ESCAPE_STRINGS = [b"%", b"_", b"\\", b"a", b"a\\", b"a%b", b"a_b", b"axb", b"x%", b"%x", b"a\\b", b"\\%", b"%_", b"", b"\\\\", b"\\a", b"xa%", b"xa_"]

# the verbatim operators take these bytes as they are: no wildcard, no escape
VERBATIM_ESCAPES = [b"%", b"_", b"a%", b"a_", b"\\", b"\\%", b"a\\"]

# prefixes and suffixes on both sides of the 8-byte word compare of str_match_anchor
WORD_BASE = b"abcdefghijklmnopqrstuvwxyz0123456789"
WORD_STRINGS = ([WORD_BASE[:k] for k in range(0, 30)] + [WORD_BASE[k:] for k in range(0, 30)]
                + [WORD_BASE, WORD_BASE + WORD_BASE, b"abcdefgX" + WORD_BASE[8:], WORD_BASE[:-9] + b"Y" + WORD_BASE[-8:], WORD_BASE.upper()])
WORD_SIZES = (1, 7, 8, 9, 15, 16, 17, 24)


def word_cases(k: int) -> list:
    b = WORD_BASE
    return [(LIKE, b[:k] + b"%"), (LIKE, b"%" + b[-k:]), (LIKE, b[:k] + b"%" + b[-k:]), (LIKE, b[:k]), (NOT_LIKE, b[:k] + b"%"), (ILIKE, b[:k].upper() + b"%" + b[-k:]), (STARTS_WITH, b[:k]),
            (ENDS_WITH, b[-k:])]


# the largest pattern, and its segments: 4096 bytes
BIG_STRINGS = [b"a" * 4096, b"a" * 4095, b"a" * 4097, b"a" * 4095 + b"b"]
BIG_CASES = [(LIKE, b"a" * 4096), (LIKE, b"_" * 4096), (LIKE, b"%a" * 2048), (CONTAINS, b"a" * 4095 + b"b"), (STRPOS, b"a" * 4095 + b"b")]
