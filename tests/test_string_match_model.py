"""The plain-Python model of string matching (tests/string_match_util.py, quirk Q27) against pyarrow.compute on valid UTF-8, against a
restatement of the device's greedy strategy on arbitrary bytes, and a guard over the GPU case lists: every (operator, pattern, column)
there has a true and a false valid row under the model, so that no GPU case can pass by answering a constant."""
import numpy as np
import pytest

from tests.string_match_util import (BIG_CASES, BIG_STRINGS, VERBATIM_ESCAPES, WORD_SIZES, WORD_STRINGS, long_group_cases, long_group_strings, wide_group_strings, word_cases, ALPHABET, CONSTANT_BY_MEANING, CONTAINS, ENDS_WITH, ESCAPE_PATTERNS, ESCAPE_STRINGS, GROUP_CASES, GROUPS, ILIKE, ILIKE_PATTERNS, ILIKE_STRINGS, LIKE,
                                     LIKE_PATTERNS, ONE_PATTERNS, ONE_STRINGS, ROW_CASES, ROW_POOL, STARTS_WITH, STRPOS, character_ends, elements, exhaustive_cases, all_strings,
                                     greedy_like, group_strings, model, model_like, model_strpos)

PIECES = ["a", "b", "A", "B", "é", "É", "日", "😀", "%", "_", "\\", "-", " "]


def random_text(rng, pieces, max_len):
    return "".join(pieces[int(i)] for i in rng.integers(0, len(pieces), int(rng.integers(0, max_len + 1))))


def test_the_rules_spelled_out():
    assert elements(b"a\\%%%_\\") == [ord("a"), ord("%"), "any", "one", 0x5C]
    assert elements(b"\\\\\\_") == [0x5C, ord("_")]
    assert character_ends(b"\xa9\xa9a\xa9b") == {0: 4, 4: 5}  # continuation bytes at the very front belong to character 1
    assert character_ends(b"\xa9\xa9") == {0: 2} and character_ends(b"") == {}
    assert model_like(b"\xa9\xa9a", b"_") and not model_like(b"\xa9\xa9ab", b"_") and model_like(b"\xa9\xa9ab", b"__")
    assert model_like("é".encode(), b"_") and not model_like("é".encode(), b"__") and model_like("é".encode(), b"%\xa9") and not model_like("é".encode(), b"%_%\xa9")
    assert model_like(b"", b"") and model_like(b"", b"%") and not model_like(b"", b"_") and not model_like(b"a", b"")
    assert model_like(b"ABC", b"a_c", fold=True) and not model_like("É".encode(), "é".encode(), fold=True)
    assert [model_strpos(s, b"b") for s in (b"ab", "éb".encode(), b"\xa9\xa9b", b"a", b"")] == [2, 2, 1, 0, 0]
    assert model_strpos(b"", b"") == 1 and model_strpos(b"xyz", b"") == 1 and model_strpos(b"aXbXc", b"Xc") == 4


def test_model_against_pyarrow_on_valid_utf8():
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    rng = np.random.default_rng(27)
    strings = [random_text(rng, PIECES, 8) for _ in range(400)]
    arr = pa.array(strings, type=pa.string())
    raw = [s.encode() for s in strings]
    patterns = [random_text(rng, ["a", "b", "é", "%", "_", "%", "_", "\\", "A", "-"], 5) for _ in range(150)]
    compared = 0
    for p in patterns:
        pb = p.encode()
        if (len(p) - len(p.rstrip("\\"))) % 2:
            # a `\` that ends the pattern: the rule makes it a literal `\`; pyarrow drops it (`-\` matches "-" there).  Not comparable.
            assert elements(pb)[-1] == 0x5C, p
            continue
        compared += 1
        assert pc.match_like(arr, p).to_pylist() == [model_like(s, pb) for s in raw], p
    assert compared > 100
    for sub in [random_text(rng, ["a", "b", "é", "%", "_", "日"], 3) for _ in range(60)]:
        sb = sub.encode()
        assert pc.starts_with(arr, sub).to_pylist() == [model(STARTS_WITH, s, sb) for s in raw], sub
        assert pc.ends_with(arr, sub).to_pylist() == [model(ENDS_WITH, s, sb) for s in raw], sub
        assert pc.match_substring(arr, sub).to_pylist() == [model(CONTAINS, s, sb) for s in raw], sub
        at = pc.find_substring(arr, sub).to_pylist()  # a BYTE index, -1 when absent: as a character number
        assert [0 if j < 0 else len(s[:j].decode()) + 1 for j, s in zip(at, raw)] == [model(STRPOS, s, sb) for s in raw], sub


def test_ilike_against_pyarrow_on_ascii():
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    rng = np.random.default_rng(5)
    ascii_pieces = ["a", "b", "A", "B", "z", "Z", "[", "@", "`", "{", "-"]
    strings = [random_text(rng, ascii_pieces, 7) for _ in range(300)]
    arr = pa.array(strings, type=pa.string())
    for p in [random_text(rng, ascii_pieces + ["%", "_", "%"], 5) for _ in range(120)]:
        assert pc.match_like(arr, p, ignore_case=True).to_pylist() == [model_like(s.encode(), p.encode(), fold=True) for s in strings], p


def test_model_against_the_greedy_restatement_on_arbitrary_bytes():
    """the reachable-set model and the greedy walk share no algorithm; they must agree on broken UTF-8 too"""
    rng = np.random.default_rng(11)
    symbols = [b"a", b"b", b"\xa9", b"\xc3", b"\xe6", b"\xf0", b"%", b"_", b"\\"]
    draw = lambda pool, most: b"".join(pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(0, most + 1))))
    for _ in range(20000):
        s, p = draw(symbols[:6], 9), draw(symbols, 6)
        assert model_like(s, p) == greedy_like(s, p), (s, p)
    for p in LIKE_PATTERNS:
        for s in all_strings(4):
            assert model_like(s, p) == greedy_like(s, p), (s, p)


def columns_of_the_gpu_cases():
    """(what, operator, pattern, strings) for every case list the GPU tests run"""
    strings = all_strings(5)
    for op, p in exhaustive_cases():
        yield "exhaustive", op, p, strings
    for op, p in ROW_CASES:
        yield "rows", op, p, ROW_POOL
    for g in GROUPS:
        for op, p in GROUP_CASES:
            yield f"group {g}", op, p, group_strings(g)
    for g in GROUPS:
        for op, p in GROUP_CASES:
            yield f"group {g}, wide", op, p, wide_group_strings(g)
        for op, p in long_group_cases(g):
            yield f"group {g}, long", op, p, long_group_strings(g)
    for p in ONE_PATTERNS:
        yield "one", LIKE, p, ONE_STRINGS
    for p in VERBATIM_ESCAPES:
        for op in (STARTS_WITH, ENDS_WITH, CONTAINS, STRPOS):
            yield "verbatim", op, p, ESCAPE_STRINGS
    for k in WORD_SIZES:
        for op, p in word_cases(k):
            yield f"word {k}", op, p, WORD_STRINGS
    for op, p in BIG_CASES:
        yield "big", op, p, BIG_STRINGS
    for p in ILIKE_PATTERNS:
        yield "ilike", ILIKE, p, ILIKE_STRINGS
    for p in ESCAPE_PATTERNS:
        yield "escapes", LIKE, p, ESCAPE_STRINGS


def test_no_gpu_case_is_constant_under_the_model():
    seen_exceptions = set()
    for what, op, p, strings in columns_of_the_gpu_cases():
        values = {bool(model(op, s, p)) for s in strings}
        if (op, p) in CONSTANT_BY_MEANING:
            assert len(values) == 1, (what, op, p)
            seen_exceptions.add((op, p))
        else:
            assert values == {True, False}, (what, op, p)
    assert seen_exceptions  # the list is not dead
    assert len(ALPHABET) == 6 and len(all_strings(5)) == 9331


def test_the_wide_group_strings_reach_past_the_word_walks_first_chunk():
    """a chunk of the 8-positions-per-lane walk is 8G positions: for every lane group there are matching rows whose leftmost `xy` lies
    in chunk 0, across the edge, in chunk 1 and in chunk 2, with characters of two bytes in front of some of them"""
    for g in GROUPS:
        rows = wide_group_strings(g)
        at = [s.find(b"xy") for s in rows]
        assert {-1, 3, 8 * g - 2, 8 * g - 1, 8 * g, 8 * g + 1, 16 * g - 2, 16 * g - 1} <= set(at), (g, sorted(set(at)))
        assert any(a >= 8 * g and model(STRPOS, s, b"xy") < a + 1 for a, s in zip(at, rows))  # fewer characters than bytes in front
        assert any(model(LIKE, s, b"%x%y%z%") and s.find(b"x") < 8 * g <= s.find(b"y", s.find(b"x")) for s in rows)
        assert max(len(s) for s in rows) == 16 * g + 1
