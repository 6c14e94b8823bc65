"""CPU: the model of tests/string_args_util.py (what the GPU tests compare against) against independent statements of the same
functions, for valid UTF-8: Python's own slicing of the decoded string, `bytes * n`, `bytes.replace`."""
import pytest

from tests.string_args_util import CONTENTS, INT64_MAX, INT64_MIN, INVALID, PATTERNS, WINDOWS, character_numbers, model_repeat, model_replace, model_rows, model_substr


def valid_utf8(s: bytes) -> bool:
    try:
        s.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


VALID = [s for s in CONTENTS if valid_utf8(s)]


def test_the_case_lists_hold_what_they_should():
    assert len(VALID) > 40 and any(len(s.decode()) != len(s) for s in VALID) and not any(valid_utf8(s) for s in INVALID if s != b"")
    assert any(start < 1 for start, _ in WINDOWS) and any(n == INT64_MAX for _, n in WINDOWS) and any(n <= 0 for _, n in WINDOWS)


def test_substr_is_python_slicing_of_the_code_points():
    for s in VALID:
        text = s.decode()
        for start in list(range(1, 12)) + [40, 1000, INT64_MAX]:
            for length in (0, 1, 2, 3, 8, 100, INT64_MAX):
                assert model_substr(s, start, length) == text[start - 1: start - 1 + length].encode(), (s, start, length)


def test_substr_with_a_start_before_one_counts_the_missing_characters():
    for s in VALID:
        text = s.decode()
        for start in (0, -1, -2, -7, INT64_MIN):
            for length in (-1, 0, 1, 2, 3, 9, 12):
                assert model_substr(s, start, length) == text[: max(start + length - 1, 0)].encode(), (s, start, length)
            assert model_substr(s, start, INT64_MAX) == (s if start > INT64_MIN + 1 else b"")


def test_substr_on_invalid_utf8_is_a_contiguous_range_by_character_number():
    assert character_numbers(b"\xa9\xa9ab") == [1, 1, 1, 2] and character_numbers(b"a\xa9\xa9b") == [1, 1, 1, 2] and character_numbers(b"") == []
    assert model_substr(b"\xa9\xa9ab", 1, 1) == b"\xa9\xa9a" and model_substr(b"\xa9\xa9ab", 2, 1) == b"b"   # leading continuation bytes belong to character 1
    assert model_substr(b"\xa9" * 6, 1, 1) == b"\xa9" * 6 and model_substr(b"\xa9" * 6, 2, 5) == b""
    for s in INVALID:
        for start, length in WINDOWS:
            got = model_substr(s, start, length)
            assert got in s and (not got or s.index(got) >= 0)


def test_repeat_and_replace():
    for s in CONTENTS + INVALID:
        for n in (-3, -1, 0, 1, 2, 9):
            assert model_repeat(s, n) == (s * n if n > 0 else b"")
        for frm, to in PATTERNS:
            got = model_replace(s, frm, to)
            assert got == (s.replace(frm, to) if frm else s)
            if frm and to and frm not in to:
                assert len(got) == len(s) + s.count(frm) * (len(to) - len(frm))
    assert model_replace(b"aaaaa", b"aa", b"b") == b"bba" and model_replace(b"ababab", b"aba", b"_") == b"_bab" and model_replace(b"abc", b"", b"x") == b"abc"


def test_null_rows_are_empty():
    out, valid = model_rows(model_substr, [b"abc", b"def", b"ghi", b"jkl"], [1, None, 2, 1], 2, mask=[True, True, False, True])
    assert out == [b"ab", b"", b"", b"jk"] and valid == [True, False, False, True]
    out, valid = model_rows(model_replace, [b"abc"] * 2, b"a", None)
    assert out == [b"", b""] and valid == [False, False]
