"""The model of the string functions with arguments (quirk Q26: NQE_EXPR_STRING_ARGS — substr, repeat, replace) in plain Python over
`bytes`, written from the rules in include/nqe.h and not from the kernels, and the shared case lists.  The helpers that move byte
strings into and out of Utf8 columns are tests/string_fn_util.py's."""
from tests.string_fn_util import CONTENTS, FOUR, INVALID, LENGTHS, ROW_COUNTS, THREE, TWO, byte_strings, relative_offsets, sized, straddlers, utf8_column  # noqa: F401 (shared with the tests)

INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


# ----------------------------------------------------------------------------- the model
def character_numbers(s: bytes) -> list:
    """c(j) = max(1, number of bytes k <= j with (s[k] & 0xC0) != 0x80)"""
    out, seen = [], 0
    for b in s:
        seen += (b & 0xC0) != 0x80
        out.append(max(1, seen))
    return out


def model_substr(s: bytes, start: int, length: int) -> bytes:
    """the bytes with max(start, 1) <= c(j) < start + length, the sum saturating at INT64_MAX"""
    lo, hi = max(start, 1), min(start + length, INT64_MAX)
    return bytes(b for b, c in zip(s, character_numbers(s)) if lo <= c < hi)


def model_repeat(s: bytes, n: int) -> bytes:
    return s * max(n, 0)


def model_replace(s: bytes, frm: bytes, to: bytes) -> bytes:
    """leftmost non-overlapping occurrences, left to right; an empty `from` leaves the string as it is (bytes.replace would insert)"""
    return s if not frm else s.replace(frm, to)


def model_rows(func, items, *args, mask=None):
    """func over rows: every argument is a scalar or a per-row list; a None (scalar or in a list) or a False in `mask` makes the row
    NULL, and a NULL row is the empty string.  Returns (byte strings, validity)."""
    n = len(items)
    cols = [a if isinstance(a, list) else [a] * n for a in args]
    out, valid = [], []
    for i, s in enumerate(items):
        row = [c[i] for c in cols]
        ok = (mask is None or bool(mask[i])) and all(a is not None for a in row)
        valid.append(ok)
        out.append(func(s, *row) if ok else b"")
    return out, valid


# ----------------------------------------------------------------------------- the shared cases
# (start, len) pairs: the ends of the window on every side of 1, of the string's end and of the 8- and 16-byte marks, negative and huge values
WINDOWS = [(1, 2), (3, INT64_MAX), (1, INT64_MAX), (0, 3), (-2, 5), (-2, 3), (-5, 2), (2, 0), (2, -1), (7, 3), (8, 2), (9, 9), (15, 3), (17, 1), (1, 16), (30, 100),
           (1000, 5), (INT64_MAX, INT64_MAX), (INT64_MAX, 1), (INT64_MIN, INT64_MAX), (INT64_MIN, 5), (5, INT64_MIN), (2, INT64_MAX - 1), (INT64_MAX - 1, 2)]
REPEATS = (-1, 0, 1, 2, 9)
# (from, to): border-free and bordered patterns, the three length relations, empty and multi-byte
PATTERNS = [(b"a", b"b"), (b"a", b""), (b"a", b"xyz"), (b"ab", b"ba"), (b"ab", b"X"), (b"ab", b"abab"), (b"aa", b"b"), (b"aa", b"bb"), (b"aa", b"ccc"), (b"aba", b"_"),
            (b"aba", b"xyz"), (b"aba", b"[aba]"), (b" ", b""), (b" ", b"  "), (b"  ", b" "), (TWO, b"e"), (THREE, FOUR), (FOUR, THREE), (b"\xa9", b"?"), (b"\xa9\xa9", b"\xa9"),
            (b"", b"x"), (b"", b""), (b"Zz", b"zZ"), (b"abcdefgh", b"12345678"), (b"abcdefghi", b"")]


def bordered_runs(group: int) -> list:
    """"aa" over "a" * (2G + 1) and "aba" over "ababab…": the greedy carry across chunks of G positions, plus neighbours of those lengths"""
    out = []
    for n in (2 * group - 1, 2 * group, 2 * group + 1, 3 * group + 2):
        out += [b"a" * n, (b"ab" * n)[:n], (b"ab" * n)[:n] + b"a", b"x" + b"a" * n]
    return out
