"""CPU: the model the GPU tests of the string functions compare against (tests/string_fn_util.py, quirk Q25) is what everybody else
means by these functions wherever they are comparable: Python's str methods on valid UTF-8 / ASCII, and pyarrow's utf8_* / ascii_*
kernels where pyarrow imports.  These tests pass without the feature by construction: they are about the yardstick."""
import itertools

import numpy as np
import pytest

from tests.string_fn_util import (CONTENTS, INVALID, LENGTH, LENGTHS, LOWER, LTRIM, REVERSE, RTRIM, TRIM, UPPER, model, model_length, model_lower, model_reverse,
                                  model_trim, model_upper, sized, unit_starts)


def valid_strings():
    out = []
    for b in CONTENTS:
        try:
            out.append(b.decode("utf-8"))
        except UnicodeDecodeError:
            pass
    out += ["", " ", "  a  ", "\t x\n", " x ", "　x　", "ß", "À", "\U0001F600", "aé日\U0001F600z", " é "]
    return out


def test_model_equals_python_on_valid_utf8():
    strings = valid_strings()
    assert len(strings) > 40
    for s in strings:
        b = s.encode()
        assert model(TRIM, b) == s.strip(" ").encode(), s
        assert model(LTRIM, b) == s.lstrip(" ").encode(), s
        assert model(RTRIM, b) == s.rstrip(" ").encode(), s
        assert model(LENGTH, b) == len(s), s
        assert model(REVERSE, b) == s[::-1].encode(), s


def test_model_equals_python_on_ascii():
    rng = np.random.default_rng(1)
    strings = [bytes(range(0, 0x80))] + [bytes(rng.integers(0, 0x80, int(n)).astype(np.uint8)) for n in rng.integers(0, 40, 200)]
    for b in strings:
        s = b.decode("ascii")
        assert model(LOWER, b) == s.lower().encode("ascii")
        assert model(UPPER, b) == s.upper().encode("ascii")
    # and every byte >= 0x80 is left alone, so the length never changes
    high = bytes(range(0x80, 0x100))
    assert model_lower(high) == high and model_upper(high) == high
    for s in ("Straße", "İ", "ǅ", "ÀÉ"):
        b = s.encode()
        assert len(model_lower(b)) == len(b) == len(model_upper(b))
        assert bytes(x for x in model_lower(b) if x >= 0x80) == bytes(x for x in b if x >= 0x80)


def test_model_equals_pyarrow():
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    strings = valid_strings()
    arr = pa.array(strings, type=pa.string())
    enc = [s.encode() for s in strings]
    assert pc.utf8_trim(arr, characters=" ").to_pylist() == [model(TRIM, b).decode() for b in enc]
    assert pc.utf8_ltrim(arr, characters=" ").to_pylist() == [model(LTRIM, b).decode() for b in enc]
    assert pc.utf8_rtrim(arr, characters=" ").to_pylist() == [model(RTRIM, b).decode() for b in enc]
    assert pc.ascii_lower(arr).to_pylist() == [model(LOWER, b).decode() for b in enc]
    assert pc.ascii_upper(arr).to_pylist() == [model(UPPER, b).decode() for b in enc]
    assert pc.utf8_length(arr).to_pylist() == [model(LENGTH, b) for b in enc]
    assert pc.utf8_reverse(arr).to_pylist() == [model(REVERSE, b).decode() for b in enc]


def test_reverse_is_a_permutation_of_arbitrary_bytes_and_an_involution_on_valid_utf8():
    rng = np.random.default_rng(2)
    alphabet = [0x20, 0x41, 0x7A, 0xC3, 0xA9, 0xF0, 0x9F, 0xE6, 0x80, 0xBF, 0xFF]
    arbitrary = list(INVALID) + [bytes(rng.choice(alphabet, int(n)).astype(np.uint8)) for n in rng.integers(0, 30, 500)]
    arbitrary += [bytes(t) for k in range(5) for t in itertools.product([0x41, 0xC3, 0xA9], repeat=k)]
    for b in arbitrary:
        r = model_reverse(b)
        assert sorted(r) == sorted(b), b
        starts = unit_starts(b)
        run = 0
        for st in starts:
            run = 1 if st else run + 1
            assert run <= 4, b
    assert model_reverse(b"\xa9" * 6) == b"\xa9" * 6
    assert model_reverse(b"\xc3" + b"\xa9" * 5) == b"\xa9\xa9\xc3\xa9\xa9\xa9"
    for s in valid_strings():
        b = s.encode()
        assert model_reverse(model_reverse(b)) == b, s


def test_sized_strings_have_their_length_and_the_trims_compose():
    for L in LENGTHS:
        for seed in range(3):
            b = sized(L, seed)
            assert len(b) == L
            assert model_trim(b, True, True) == model_trim(model_trim(b, True, False), False, True)
            assert model_length(b) <= L
