"""CPU: the record-splitter model and the case lists of tests/csv_util.py, before tests/test_gpu_csv_edges.py takes the same files
to the device.

  * the model's two splitters (one sequential walk; the tiled composition of transition vectors, at the device's sizes and at
    chunk / block / carry = 4 / 4 / 4) cut out exactly the fields the oracle's reader returns, for every file;
  * coverage, asserted: every automaton state enters every edge; every feature sits at every offset of every edge; a carry tile
    is entered inside quotes and right after a quote; every file length ends in every way;
  * every modelled kernel mistake (csv_util.MUTANTS) mis-splits at least one of the files the device test runs."""
import functools
import os
import re

import pytest

from naive_query_engine_amd import ErrorCode
from oracle import oracle as orc
from tests import csv_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "naive_query_engine_amd", "csrc")
MINI = dict(chunk=4, block=4, carry=4)
MINI_LIMIT = 64 << 10


@functools.lru_cache(maxsize=None)
def scan_chunk() -> int:
    return int(re.search(r"constexpr int SCAN_CHUNK = (\d+);", open(os.path.join(CSRC, "sort.hip")).read()).group(1))


@functools.lru_cache(maxsize=None)
def groups():
    return cu.all_cases(scan_chunk())


@functools.lru_cache(maxsize=None)
def oracle_of(group: str, i: int):
    """(what oracle.csv_read returned or raised, its columns as lists), computed once per file"""
    _, data, kw = groups()[group][i]
    try:
        res = orc.csv_read(data, **kw)
    except ErrorCode as e:
        return e, None
    return res, cu.oracle_rows(res)


@functools.lru_cache(maxsize=None)
def walk_of(group: str, i: int):
    """the sequential walk of one file, with the state at byte CHUNK and at every workgroup's first byte"""
    data = groups()[group][i][1]
    return cu.sequential(data, probes=[cu.CHUNK] + list(range(0, len(data) + 1, cu.WG_BYTES)))


@functools.lru_cache(maxsize=None)
def tiled_of(group: str, i: int):
    return cu.split_chunked(groups()[group][i][1])


def every_case():
    for g in cu.GROUPS:
        for i, (label, data, kw) in enumerate(groups()[g]):
            yield g, i, label, data, kw


def test_constants_are_the_ones_of_the_kernels():
    src = open(os.path.join(CSRC, "csv.hip")).read()
    assert int(re.search(r"constexpr int CSV_CHUNK = (\d+);", src).group(1)) == cu.CHUNK == 64
    assert int(re.search(r"constexpr int CSV_BLOCK = (\d+);", src).group(1)) == cu.BLOCK == 256
    assert int(re.search(r"constexpr int CSV_MAX_COLS = (\d+);", src).group(1)) == cu.MAX_COLS
    assert cu.WG_BYTES == cu.CHUNK * cu.BLOCK == 16384
    # csv_block_scan_kernel: one workgroup of CSV_BLOCK lanes walks the totals in tiles of CSV_BLOCK
    assert re.search(r"for \(int64_t base = 0; base < nblocks; base \+= CSV_BLOCK\)", src)
    assert cu.CARRY_BYTES == cu.WG_BYTES * cu.BLOCK == 4194304
    assert int(re.search(r"__launch_bounds__\((\d+)\) csv_fields_kernel", src).group(1)) == cu.FIELD_BLOCK == 256
    assert src.count(f"(rows + {cu.FIELD_BLOCK - 1}) / {cu.FIELD_BLOCK}") == 2 and src.count(f"grid, dim3({cu.FIELD_BLOCK})") == 2
    assert scan_chunk() == 4096
    # the automaton's numbering is the header's
    hdr = open(os.path.join(CSRC, "csv_split.hpp")).read()
    assert re.search(r"ST_R = 0 .*ST_F = 1 .*ST_U = 2 .*ST_Q = 3 .*ST_E = 4 ", hdr)
    assert (cu.R, cu.F, cu.U, cu.Q, cu.E) == (0, 1, 2, 3, 4)


def test_case_counts_and_the_limit_on_big_files():
    g = groups()
    big = [c for grp in g.values() for c in grp if len(c[1]) >= cu.CARRY_BYTES]
    assert len(big) == sum(len(g[k]) for k in g if k.startswith("carry")) <= cu.MAX_BIG_FILES
    labels = [c[0] for grp in g.values() for c in grp]
    assert len(set(labels)) == len(labels)
    for edge in cu.SLIDE_EDGES[:-1]:
        assert len(g[f"slide_{edge}"]) == 2 * (3 * len(cu.FEATURES) + 1)   # feature x offset x padding form (+ the second split of 日)


@pytest.mark.parametrize("group", cu.GROUPS)
def test_both_splitters_cut_out_what_the_oracle_reads(group):
    for i, (label, data, kw) in enumerate(groups()[group]):
        res, lists = oracle_of(group, i)
        starts, ends, at_wg = walk_of(group, i)
        assert cu.disagreement(data, starts, ends, kw, res, lists) is None, label
        sizes = [{}] + ([MINI] if len(data) < MINI_LIMIT else [])
        for size in sizes:
            m = cu.split_chunked(data, **size) if size else tiled_of(group, i)
            assert m["starts"] == starts and m["ends"] == ends, f"{label} {size}"
            chunk, block, carry = size.get("chunk", cu.CHUNK), size.get("block", cu.BLOCK), size.get("carry", cu.BLOCK)
            nwg, ntile = len(m["wg_in"]), len(m["tile_in"])
            probes = [w * chunk * block for w in range(nwg)] + ([c * chunk for c in range(len(m["chunk_in"]))] if len(data) < MINI_LIMIT else [])
            seen = cu.sequential(data, probes=probes)[2] if size or len(data) < MINI_LIMIT else at_wg
            n = len(data)
            # the incoming state of every workgroup and carry tile (and of every chunk of the smaller files) is the walk's
            assert [seen[w * chunk * block] for w in range(nwg) if w * chunk * block <= n] == [s for w, s in enumerate(m["wg_in"]) if w * chunk * block <= n], f"{label} {size}"
            assert [seen[t * chunk * block * carry] for t in range(ntile)] == m["tile_in"], f"{label} {size}"
            if len(data) < MINI_LIMIT:
                assert [seen[c * chunk] for c in range(len(m["chunk_in"]))] == m["chunk_in"], f"{label} {size}"


def test_every_state_enters_every_edge():
    entered = {edge: set() for edge in cu.COVERAGE_EDGES}
    for g, i, label, data, kw in every_case():
        seen = walk_of(g, i)[2]
        for edge in cu.COVERAGE_EDGES:
            if edge < len(data):
                entered[edge].add(seen[edge])
    for edge in cu.COVERAGE_EDGES:
        assert entered[edge] == {cu.R, cu.F, cu.U, cu.Q, cu.E}, f"byte {edge} is entered only in {sorted(cu.STATE_NAMES[s] for s in entered[edge])}"


def test_every_feature_sits_at_every_offset_of_every_edge():
    for edge in cu.SLIDE_EDGES:
        have = set()
        for label, data, kw, tags in cu.slide_cases(edge):
            for feature, off in tags:
                first = data[edge + off: edge + off + 1]
                assert first in cu.FIRST_BYTE[feature], f"{label}: {feature} does not begin at byte {edge + off}"
                have.add((feature, off))
        missing = {(f, o) for f in cu.FEATURES for o in cu.OFFSETS} - have
        assert not missing, f"edge {edge}: {sorted(missing)}"
    # both padding forms, each entering the chunk before the feature in its own state (below the carry: every feature in both)
    for edge in (cu.CHUNK * 2, cu.WG_BYTES):
        for label, data, kw, tags in cu.slide_cases(edge):
            st = cu.sequential(data, probes=[edge - cu.CHUNK])[2][edge - cu.CHUNK]
            assert st == (cu.Q if "padding=quoted" in label else cu.U), label


def test_a_carry_tile_is_entered_inside_quotes_and_right_after_a_quote():
    states = set()
    for g in cu.GROUPS:
        if g.startswith("carry"):
            for i in range(len(groups()[g])):
                states.update(tiled_of(g, i)["tile_in"][1:])
    assert {cu.Q, cu.E} <= states, sorted(cu.STATE_NAMES[s] for s in states)


def test_every_length_ends_in_every_way():
    have = {key for _, _, _, key in cu.eof_cases()}
    for n in cu.EOF_LENGTHS:
        for ending, tail in cu.EOF_ENDINGS.items():
            if n == 1 and ending in ("crlf", "after_closing_quote"):
                continue                                # these endings are two bytes
            assert (n, ending) in have
    for label, data, kw, (n, ending) in cu.eof_cases():
        assert len(data) == n
        final = cu.sequential(data, probes=[n])[2][n]
        if ending in ("lf", "crlf", "cr"):
            assert final == cu.R and data[-1:] in (b"\n", b"\r"), label
        else:
            assert final == {"none": cu.U, "delimiter": cu.F, "inside_quotes": cu.Q, "after_closing_quote": cu.E}[ending], label
    # the branch `hi == n && st != ST_R` taken by the last thread of a full chunk
    assert any(n % cu.CHUNK == 0 and ending == "none" for _, _, _, (n, ending) in cu.eof_cases())


def killed_by(mutant: str, group: str, i: int) -> bool:
    label, data, kw = groups()[group][i]
    res, lists = oracle_of(group, i)
    m = cu.split_chunked(data, mutant=mutant)
    if len(m["starts"]) != len(m["ends"]):
        return True
    if not isinstance(res, Exception) and len(m["starts"]) != res[2][0].length + (1 if kw.get("has_header", True) else 0):
        return True                                     # (cheaper than cutting fields: the record count alone is wrong)
    return cu.disagreement(data, m["starts"], m["ends"], kw, res, lists) is not None


@pytest.mark.parametrize("mutant", cu.MUTANTS)
def test_every_mutant_is_killed(mutant):
    """each switch makes the model disagree with the oracle on at least one file of the set the device test runs"""
    order = ["flip", "eof", "slide_64", "slide_16384", "dense", "slide_128", "slide_16448", "rows", "carry_flip", "carry_slide", "carry_eof", "carry_dense"]
    assert sorted(order) == sorted(cu.GROUPS)
    for group in order:
        for i in range(len(groups()[group])):
            if killed_by(mutant, group, i):
                return
    pytest.fail(f"mutant {mutant} survives every case")
