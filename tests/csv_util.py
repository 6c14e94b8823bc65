"""The model and the cases of the CSV ingest edge tests (csrc/csv.hip, csrc/csv_split.hpp).

Plain numpy and Python, no device and no library.  Two record splitters written from the csv crate's rules as the oracle's
comment states them (oracle/nqe_oracle.cpp, CsvReaderState): a quote is special only at the start of a field, "" inside quotes
is one quote, text after a closing quote is appended, \\r / \\n / \\r\\n end a record, empty lines are skipped, a last record
without a terminator is kept.

  * `sequential(data)`: one walk of the five-state automaton over the file; also answers "which state is byte p entered in".
  * `split_chunked(data, chunk, block, carry)`: the tiling of the device pipeline: one transition vector per chunk, composed per
    workgroup of `block` chunks, then across workgroups in tiles of `carry` workgroups with a carried vector, then the incoming
    state of every chunk is read at entry R and the chunks are walked again to mark record starts and ends.  `mutant=` switches
    on one plausible kernel mistake (MUTANTS); mutants exist only in this model and are never run on a device.

The case lists live here so that the CPU test of the model (tests/test_csv_split_model.py) and the device test
(tests/test_gpu_csv_edges.py) walk the same files.  Every generator returns (label, bytes, kwargs of oracle.csv_read)."""
import functools

import numpy as np

# the tiling of csv.hip (asserted against its source text by tests/test_csv_split_model.py)
CHUNK = 64                              # CSV_CHUNK: bytes per thread
BLOCK = 256                             # CSV_BLOCK: threads per workgroup, and workgroup totals per tile of csv_block_scan_kernel
WG_BYTES = CHUNK * BLOCK                # 16384
CARRY_BYTES = WG_BYTES * BLOCK          # 4194304: one tile of the totals loop, after which the carry is used
FIELD_BLOCK = 256                       # rows per workgroup of csv_fields_kernel
MAX_COLS = 64                           # CSV_MAX_COLS
SLIDE_EDGES = (CHUNK, 2 * CHUNK, WG_BYTES, WG_BYTES + CHUNK, CARRY_BYTES)
COVERAGE_EDGES = (CHUNK, WG_BYTES, CARRY_BYTES)
EOF_LENGTHS = (1, 63, 64, 65, 127, 128, 16383, 16384, 16385, 4194304, 4194305)
MAX_BIG_FILES = 40                      # files of CARRY_BYTES or more, over all groups

# ----------------------------------------------------------------------------- the automaton
R, F, U, Q, E = range(5)                # record start, field start, unquoted, quoted, quote seen inside quotes
STATE_NAMES = "RFUQE"
NL, QUOTE, DELIM, OTHER, PAD = range(5)  # byte classes; PAD: past the end of the file (no byte)


def step(st, cls):
    """one byte of class `cls` in state `st` → (next state, this byte opens a record, this byte closes one)"""
    if st == Q:                                        # inside quotes only a quote matters
        return (E if cls == QUOTE else Q), False, False
    if cls == NL:                                      # R: an empty line; else the terminator of the record
        return R, False, st != R
    opens = st == R
    if cls == DELIM:
        return F, opens, False
    if cls == QUOTE:
        if st == E:                                    # "" inside quotes: one quote of content
            return Q, False, False
        return (Q if st in (R, F) else U), opens, False  # special only at the start of a field
    return U, opens, False                             # other bytes; after a closing quote (E) the field goes on unquoted


def parity_step(st, cls):
    """the mistake `step` is there to avoid: every quote toggles "inside quotes\""""
    if st in (Q, E):
        return (U if cls == QUOTE else Q), False, False
    if cls == QUOTE:
        return Q, st == R, False
    return step(st, cls)


def _table(fn):
    t = np.zeros((5, 5), dtype=np.int64)
    for st in range(5):
        for cls in range(4):
            t[st, cls] = fn(st, cls)[0]
        t[st, PAD] = st
    return t


TABLE = _table(step)
PARITY_TABLE = _table(parity_step)
IDENT = (R, F, U, Q, E)


def classify(data: bytes, delim: int = 44) -> np.ndarray:
    b = np.frombuffer(data, dtype=np.uint8)
    cls = np.full(b.size, OTHER, dtype=np.uint8)
    cls[(b == 10) | (b == 13)] = NL
    cls[b == 34] = QUOTE
    cls[b == delim] = DELIM
    return cls


def sequential(data: bytes, delim: int = 44, probes=()):
    """→ (record starts, record ends, {p: state byte p is entered in} for p in probes; p == len(data): the final state).
    Runs of ordinary bytes are stepped over at once (R, F, E → U; U and Q stay), so a file that is mostly padding is cheap."""
    n = len(data)
    cls = classify(data, delim)
    idx = np.flatnonzero(cls != OTHER).tolist()
    kinds = cls[idx].tolist() if idx else []
    want = sorted(p for p in set(probes) if 0 <= p <= n)
    seen, wi = {}, 0
    starts, ends = [], []
    st, pos = R, 0
    for i, c in zip(idx + [n], kinds + [None]):
        while wi < len(want) and want[wi] <= i:
            p = want[wi]
            seen[p] = st if p == pos else step(st, OTHER)[0]
            wi += 1
        if i > pos:                                    # ordinary bytes pos .. i-1
            if st == R:
                starts.append(pos)
            st = step(st, OTHER)[0]
        if c is None:
            break
        st, a, b = step(st, c)
        if a:
            starts.append(i)
        if b:
            ends.append(i)
        pos = i + 1
    if st != R:
        ends.append(n)                                 # the last record has no terminator
    return starts, ends, seen


# ----------------------------------------------------------------------------- the chunked splitter
MUTANTS = (
    "swap_workgroup",       # compose(b, a) in the scan over the chunks of a workgroup
    "swap_totals",          # ... in the scan over the workgroup totals of one tile
    "swap_carry",           # ... where the carry meets a tile's prefixes and its total
    "swap_mark",            # ... where the block prefix meets the chunk's prefix
    "carry_not_advanced",   # the carry stays the identity
    "carry_exclusive",      # the carry takes the exclusive prefix of the tile's last lane, not the tile's total
    "start_field",          # the stream starts at F, not at R
    "entry_E_identity",     # a chunk's vector keeps E → E
    "entry_Q_identity",     # a chunk's vector keeps Q → Q
    "quote_parity",         # any quote toggles
    "eof_wrong_chunk",      # "last record without terminator" tested on chunk n / chunk: no chunk when n % chunk == 0
)


def _comp(a, b, swap=False):
    """vectors as arrays [..., 5]: a then b"""
    if swap:
        a, b = b, a
    return np.take_along_axis(b, a, axis=-1)


def _comp1(a, b, swap=False):
    if swap:
        a, b = b, a
    return tuple(b[a[s]] for s in range(5))


def split_chunked(data: bytes, delim: int = 44, chunk: int = CHUNK, block: int = BLOCK, carry: int = BLOCK, mutant=None):
    """→ dict(starts, ends, chunk_in, wg_in, tile_in): record positions and the state every chunk, every workgroup (block chunks)
    and every carry tile (carry workgroups) is entered in, all computed the tiled way"""
    assert mutant is None or mutant in MUTANTS
    n = len(data)
    table = PARITY_TABLE if mutant == "quote_parity" else TABLE
    nchunks = (n + chunk - 1) // chunk
    nwg = max(1, (nchunks + block - 1) // block)
    tpad = nwg * block
    cls = np.full(tpad * chunk, PAD, dtype=np.uint8)
    cls[:n] = classify(data, delim)
    cls = cls.reshape(tpad, chunk)
    # one vector per chunk: the end state for each of the five start states
    vec = np.tile(np.arange(5, dtype=np.int64), (tpad, 1))
    for j in range(chunk):
        vec = table[vec, cls[:, j:j + 1]]
    if mutant == "entry_E_identity":
        vec[:, E] = E
    if mutant == "entry_Q_identity":
        vec[:, Q] = Q
    # level 1: exclusive prefixes inside each workgroup, and its total
    vec = vec.reshape(nwg, block, 5)
    excl = np.empty_like(vec)
    acc = np.tile(np.arange(5, dtype=np.int64), (nwg, 1))
    for t in range(block):
        excl[:, t] = acc
        acc = _comp(acc, vec[:, t], mutant == "swap_workgroup")
    totals = [tuple(int(x) for x in row) for row in acc]
    # level 2: exclusive prefixes of the totals, in tiles with a carry
    bpre, tile_in, carried = [], [], IDENT
    for base in range(0, nwg, carry):
        tile_in.append(carried)
        run, before_last = IDENT, IDENT
        for i in range(base, base + carry):             # lanes past the last workgroup hold the identity
            before_last = run
            if i < nwg:
                bpre.append(_comp1(carried, run, mutant == "swap_carry"))
                run = _comp1(run, totals[i], mutant == "swap_totals")
        if mutant == "carry_not_advanced":
            pass
        elif mutant == "carry_exclusive":
            carried = _comp1(carried, before_last)
        else:
            carried = _comp1(carried, run, mutant == "swap_carry")
    # level 3: block prefix then chunk prefix, read at the state the stream starts in
    pre = _comp(np.broadcast_to(np.array(bpre, dtype=np.int64)[:, None, :], excl.shape), excl, mutant == "swap_mark")
    entry = F if mutant == "start_field" else R
    st_in = pre[..., entry].reshape(tpad)
    # second walk: marks
    st = st_in.copy()
    opens = np.zeros((tpad, chunk), dtype=bool)
    closes = np.zeros((tpad, chunk), dtype=bool)
    for j in range(chunk):
        c = cls[:, j]
        nl = c == NL
        opens[:, j] = (st == R) & ~nl & (c != PAD)
        closes[:, j] = nl & ((st == F) | (st == U) | (st == E))
        st = table[st, c]
    starts = np.flatnonzero(opens.ravel()).tolist()
    ends = np.flatnonzero(closes.ravel()).tolist()
    if n:
        last = n // chunk if mutant == "eof_wrong_chunk" else (n - 1) // chunk
        if last * chunk < n and st[last] != R:          # (a chunk that starts at or past n does nothing)
            ends.append(n)
    return dict(starts=starts, ends=ends, chunk_in=st_in[:nchunks].tolist(), wg_in=st_in[::block][:nwg].tolist(),
                tile_in=[v[entry] for v in tile_in])


# ----------------------------------------------------------------------------- fields of one record, and the oracle's view of them
def cut_fields(rec: bytes, delim: int = 44):
    """the fields the csv crate hands out for one record (terminator not included)"""
    return _cut_fields_cached(rec, delim) if len(rec) <= 64 else _cut_fields(rec, delim)


def _cut_fields(rec: bytes, delim: int):
    out, i, n = [], 0, len(rec)
    while True:
        cur = bytearray()
        if i < n and rec[i] == 34:
            i += 1
            while i < n:
                if rec[i] == 34:
                    if i + 1 < n and rec[i + 1] == 34:
                        cur.append(34)
                        i += 2
                        continue
                    i += 1                              # the closing quote
                    break
                cur.append(rec[i])
                i += 1
        j = rec.find(bytes([delim]), i)                 # unquoted text, or text after the closing quote
        j = n if j < 0 else j
        cur += rec[i:j]
        out.append(bytes(cur))
        if j >= n:
            return tuple(out)
        i = j + 1


_cut_fields_cached = functools.lru_cache(maxsize=4096)(_cut_fields)


def model_table(data: bytes, starts, ends, has_header=True, delimiter=",", batch_size=1_000_000, **_):
    """record positions → (header fields or None, rows of fields of the first batch); None when the positions are no table"""
    if len(starts) != len(ends) or not starts:
        return None
    d = ord(delimiter)
    recs = [cut_fields(data[s:e], d) for s, e in zip(starts, ends)]
    header = recs[0] if has_header else None
    rows = recs[1:] if has_header else recs
    if batch_size >= 0:
        rows = rows[:batch_size]
    return header, rows


def oracle_rows(result):
    """oracle.csv_read's columns → one list of Python values per column"""
    return [c.to_list() for c in result[2]]


def disagreement(data: bytes, starts, ends, kwargs, oracle_result, oracle_lists=None):
    """None when the oracle's table is exactly what the record positions cut out, else a short description.
    oracle_result: what oracle.csv_read returned, or the ErrorCode it raised"""
    from naive_query_engine_amd import DType

    if isinstance(oracle_result, Exception):
        tab = model_table(data, starts, ends, **kwargs)
        if tab is None or len({len(r) for r in tab[1]} | {len(tab[0] if tab[0] is not None else tab[1][0])}) != 1:
            return None                                 # no records, or ragged: the oracle's error is the model's
        return f"the oracle fails ({oracle_result}) where the model finds {len(tab[1])} well-formed rows"
    names, _, cols = oracle_result
    tab = model_table(data, starts, ends, **kwargs)
    if tab is None:
        return f"model: {len(starts)} starts, {len(ends)} ends; oracle: {cols[0].length} rows"
    header, rows = tab
    if len(rows) != cols[0].length:
        return f"model: {len(rows)} rows, oracle: {cols[0].length}"
    if header is not None and [h.decode("utf-8", "replace") for h in header] != names:
        return f"model header {header}, oracle {names}"
    if any(len(r) != len(cols) for r in rows):
        return "model: a row with a different number of fields"
    lists = oracle_lists if oracle_lists is not None else oracle_rows(oracle_result)
    for c, col in enumerate(cols):
        exp = lists[c]
        for r, row in enumerate(rows):
            f = row[c]
            try:
                if col.dtype == DType.UTF8:
                    got = f.decode("utf-8")
                elif not f:
                    got = None
                elif col.dtype == DType.INT64:
                    got = int(f)
                elif col.dtype == DType.FLOAT64:
                    got = float(f)
                else:
                    got = {b"true": True, b"false": False}[f.lower()]
            except (ValueError, KeyError):
                return f"row {r} column {c}: the model's field {f[:40]!r} is no {col.dtype.name}"
            if got != exp[r] and not (got != got and exp[r] != exp[r]):
                return f"row {r} column {c}: model {got!r}, oracle {exp[r]!r}"
    return None


# ----------------------------------------------------------------------------- cases
KW = {"max_read_records": -1}

# ---- slide cases.  Columns k Int64, p Utf8 (the padding field), t Utf8, f Float64, b Boolean, s Utf8; the first data record is
# `7,<padding><continuation>`.  Unquoted form: the padding is P...P, every chunk before the feature is entered in U; quoted form:
# "P...P, entered in Q.  A continuation is (bytes, index of the feature's first byte) for each form.
SLIDE_HEADER = b"k,p,t,f,b,s\n"
ORDINARY = (b'-3,"q,""uo""\nted",plain,-0.125,false,"a\r\nb"\n'
            b'9223372036854775807,x,,1.5,TRUE,\n'
            b',last,"",,,"e""nd"\n')
REST = b",tt,2.5,true,zz\n"
EMPTY_LINE_RUNS = (b"\r", b"\n\r", b"\r\r\n", b"\n\r\n\r", b"\r\n\n\r\n")
UTF8_CHAR = "日".encode("utf-8")


def _both(cont: bytes, idx: int):
    """a continuation that does not use the padding's own quote: the quoted form closes the padding first"""
    return (cont, idx), (b'"' + cont, idx + 1)


FEATURES = {
    "open_quote":        _both(b',"tt",2.5,true,zz\n', 1),
    "close_then_delim":  ((b',"tt",2.5,true,zz\n', 4), (b'"' + REST, 0)),
    "close_then_term":   _both(b',tt,2.5,true,"zz"\n', 16),
    "escaped_pair":      ((b',"t""t",2.5,true,zz\n', 3), (b'""P2"' + REST, 0)),
    "escaped_then_close": ((b',"t""",2.5,true,zz\n', 3), (b'"""' + REST, 0)),
    "text_after_close":  ((b',"ab"cd,2.5,true,zz\n', 4), (b'"cd' + REST, 0)),
    "literal_quote":     ((b'"y' + REST, 0), (b'",t"t,2.5,true,zz\n', 3)),
    "crlf":              _both(b",tt,2.5,true,zz\r\n", 15),
    "bare_cr":           _both(b",tt,2.5,true,zz\r", 15),
    "empty_lines":       None,                          # built per case: the run length varies
    "delim_at_edge":     _both(REST, 0),
    "empty_last_field":  _both(b",tt,2.5,true,\n", 12),
    "empty_quoted":      _both(b',"",2.5,true,zz\n', 1),
    "utf8_split":        ((UTF8_CHAR + REST, 0), (UTF8_CHAR + b'"' + REST, 0)),
}
FIRST_BYTE = {"open_quote": b'"', "close_then_delim": b'"', "close_then_term": b'"', "escaped_pair": b'"', "escaped_then_close": b'"',
              "text_after_close": b'"', "literal_quote": b'"', "crlf": b"\r", "bare_cr": b"\r", "empty_lines": b"\r\n", "delim_at_edge": b",",
              "empty_last_field": b",", "empty_quoted": b'"', "utf8_split": UTF8_CHAR[:1]}
OFFSETS = (-1, 0, 1)


def _place(head: bytes, opener: bytes, cont: bytes, idx: int, target: int) -> bytes:
    """head + opener + padding + cont with cont[idx] at byte `target`"""
    pad = target - len(head) - len(opener) - idx
    assert pad >= 1, (target, idx)
    return head + opener + b"P" * pad + cont


def slide_cases(edge: int):
    """→ [(label, bytes, kwargs, tags)]; tags: the (feature, offset) pairs the file puts at `edge`.  Below CARRY_BYTES one file
    per feature, offset and padding form.  At CARRY_BYTES the limit of MAX_BIG_FILES leaves 23 files, so three dense strings of
    features slide over the edge a byte at a time and every file carries up to three features (see _big_slide_cases)."""
    if edge >= CARRY_BYTES:
        return _big_slide_cases(edge)
    out = []
    for name, forms in FEATURES.items():
        offsets = OFFSETS + ((-2,) if name == "utf8_split" else ())   # -1 and -2 split the character after its 1st and 2nd byte
        for oi, off in enumerate(offsets):
            for fi, form in enumerate(("unquoted", "quoted")):
                if name == "empty_lines":
                    run = EMPTY_LINE_RUNS[(2 * oi + fi) % len(EMPTY_LINE_RUNS)]
                    cont, idx = _both(REST + run, len(REST))[fi]
                else:
                    cont, idx = forms[fi]
                data = _place(SLIDE_HEADER + b"7,", b'"' if fi else b"", cont, idx, edge + off) + ORDINARY
                out.append((f"slide edge={edge} offset={off:+d} feature={name} padding={form}", data, KW, [(name, off)]))
    return out


# three strings in which almost every byte begins a feature: (header, record up to the padding, padding form, string, {index: features})
_SOUPS = (
    # inside the quoted padding: ""  """  close,  delimiter  ""(empty quoted, opening quote)  close,  delimiter
    ("A", b"k,p,t,u,f,b,s\n", b"7,", "quoted", b'""","",tt,2.5,true,zz\n',
     {0: ("escaped_pair", "escaped_then_close"), 2: ("close_then_delim",), 3: ("delim_at_edge",), 4: ("empty_quoted", "open_quote")}),
    # after the unquoted padding (last but one column): literal quote, delimiter + empty last field, CR LF, LF CR LF as empty lines, 日
    ("B", b"u,k,f,b,p,s\n", b"aa,7,2.5,true,", "unquoted", b'",\r\n\r\n' + UTF8_CHAR + b"x,8,1.5,false,pp,zz\n",
     {0: ("literal_quote",), 1: ("empty_last_field", "delim_at_edge"), 2: ("crlf",), 3: ("empty_lines",), 6: ("utf8_split",)}),
    # the quoted padding closes into text, then "z" ends the record with a bare CR and the next record follows at once
    ("C", b"u,k,f,b,p,s\n", b"aa,7,2.5,true,", "quoted", b'"c,"z"\rbb,8,1.5,false,pp,zz\n',
     {0: ("text_after_close",), 5: ("close_then_term",), 6: ("bare_cr",)}),
)
# One device thread walks a whole record, so a file of CARRY_BYTES is not one long field: whole records of about 1000 bytes (no
# divisor of the chunk size, so that chunks are entered in every phase of a record) fill it up to the last few hundred bytes
_SOUP_FILLER = {b"k,p,t,u,f,b,s\n": b"5," + b"F" * 983 + b',"f,l",x,0.5,true,zz\n', b"u,k,f,b,p,s\n": b"ff,5,0.5,true," + b"F" * 981 + b',"f,l"\n'}
_SOUP_ORDINARY = {b"k,p,t,u,f,b,s\n": b'-3,"q,""uo""\nted",plain,,-0.125,false,"a\r\nb"\n,last,"",x,,,"e""nd"\n',
                  b"u,k,f,b,p,s\n": b'"q,""uo""\nted",-3,-0.125,false,plain,"a\r\nb"\nlast,,,,"","e""nd"\n'}


def _big_slide_cases(edge: int):
    out = []
    for name, header, head, form, soup, feats in _SOUPS:
        at_edge = sorted({i - off for i in feats for off in OFFSETS})     # soup[k] at the edge puts feature i at offset i - k
        for k in at_edge:
            fill = _SOUP_FILLER[header]
            start = header + fill * ((edge - 300 - len(header)) // len(fill)) + head
            data = _place(start, b'"' if form == "quoted" else b"", soup, 0, edge - k) + _SOUP_ORDINARY[header]
            tags = [(f, i - k) for i, fs in feats.items() if i - k in OFFSETS for f in fs]
            label = f"slide edge={edge} soup={name}[{k:+d}] padding={form} " + " ".join(f"{f}@{o:+d}" for f, o in tags)
            out.append((label, data, KW, tags))
    return out


# ---- end of file
EOF_ENDINGS = {"lf": b"12,xy\n", "crlf": b"12,xy\r\n", "cr": b"12,xy\r", "none": b"12,xy", "delimiter": b"12,", "inside_quotes": b'12,"xy',
               "after_closing_quote": b'12,"xy"'}
# one byte is no header and a record: the same endings as far as one or two bytes can spell them, without a header
EOF_TINY = {1: {"lf": b"\n", "cr": b"\r", "none": b"a", "delimiter": b",", "inside_quotes": b'"'}}


def eof_cases():
    """→ [(label, bytes, kwargs, (n, ending))]: files of exactly n bytes, every ending"""
    out = []
    for n in EOF_LENGTHS:
        for ending, tail in EOF_ENDINGS.items():
            if n in EOF_TINY:
                if ending not in EOF_TINY[n]:
                    continue                            # \r\n and "" need two bytes
                data, kw = EOF_TINY[n][ending], dict(KW, has_header=False)
            else:
                head = b"a,b\n"
                if n >= CARRY_BYTES:                    # records of 1000 bytes, not one long field: a device thread walks a whole record
                    head += (b"1," + b"P" * 997 + b"\n") * (n // 1000 - 1)
                fill = n - len(head) - len(tail)        # one record `1,PPP..\n`
                data, kw = head + b"1," + b"P" * (fill - 3) + b"\n" + tail, KW
            assert len(data) == n
            out.append((f"eof n={n} ending={ending}", data, kw, (n, ending)))
    return out


# ---- flip pairs: one early byte decides how everything after it parses
def flip_pairs():
    """→ [(label, bytes, kwargs)], members of a pair next to each other"""
    out = []
    # past three workgroup tiles, and once three workgroups past the carry (the carried vector then meets prefixes that are no identity)
    for tag, span in (("3wg", 3 * WG_BYTES), ("carry", CARRY_BYTES + 3 * WG_BYTES)):
        u = b'"x\n"\n'
        n_units = span // len(u) + 101
        out.append((f"flip one-column {tag} plain", b"h\n" + u * n_units, KW))
        out.append((f"flip one-column {tag} flipped", b'h\n"' + u * n_units + b'"\n', KW))
        if tag == "3wg":                                # (the limit on big files leaves room for one pair past the carry)
            u = b'"x,\n",1\n'
            n_units = span // len(u) + 101
            out.append((f"flip two-column {tag} plain", b"h,i\n" + u * n_units, KW))
            out.append((f"flip two-column {tag} flipped", b'h,i\n"' + u * n_units + b'",1\n', KW))
    return out


# ---- dense
def dense_cases():
    out = []
    head = b"a,b\n"
    lead = b"1," + b"P" * (CHUNK - len(head) - 2 - 2) + b"\n"      # one record, so that the next one starts at byte CHUNK - 1
    for run in (63, 64, 65, 127, 128):
        q = b'"' * run
        # at a field start: the run begins at byte CHUNK; the first quote opens, pairs escape, an odd rest closes
        field = q + (b'"' if run % 2 else b"")
        out.append((f"dense quotes run={run} at field start", head + lead[:-1] + b"P\n" + field + b",1\n" + b"tail,2\n", KW))
        # inside a quoted field: `"` at byte CHUNK - 1 opens, the run begins at byte CHUNK
        field = b'"' + q + (b"" if run % 2 else b'"')
        out.append((f"dense quotes run={run} inside quotes", head + lead + field + b",1\n" + b"tail,2\n", KW))
    for size, tag in ((3 * WG_BYTES + 100, "3 workgroups"), (CARRY_BYTES + 4 * WG_BYTES + 100, "past the carry")):
        body = (b"line one\nline,two\r\n" * (size // 19 + 1))[:size]
        out.append((f"dense quoted field of {size} bytes ({tag})", head + b'"' + body + b'",1\nx,2\n"y\n",3\n', KW))
    out.append(("dense one-byte records", b"n\n" + b"1\n" * 30000, KW))
    return out


# ---- row counts against the per-record stages
def _row_table(rows: int):
    nulls = {0, rows - 1, 63, 64}
    lines = [b"i,f,b,u,nb,e,w"]
    for r in range(rows):
        null = r in nulls
        i = b"" if null else str((r * 2654435761) % (1 << 40) - (1 << 39)).encode()
        f = b"" if null else (b"%d.%03d" % (r - 100, r % 1000))
        b = b"" if null else (b"true", b"FALSE", b"True")[r % 3]
        u = (b"", b"a", b'"q,""%d"' % r, UTF8_CHAR * (r % 4), b"plain%d" % r)[r % 5]
        nb = (b"false", b"true")[(r // 3) % 2]
        w = b"" if r == 63 else str(r).encode()          # row 63: the last bit of the first validity word is the only NULL
        lines.append(b",".join((i, f, b, u, nb, b"", w)))
    return b"\n".join(lines) + b"\n"


def row_edge_cases(scan_chunk: int):
    """scan_chunk: SCAN_CHUNK of sort.hip (the Utf8 offsets scan covers rows + 1 entries)"""
    out = [("rows=0 header only", b"i,f,b,u\n", KW), ("rows=0 terminators after the header", b"i,f,b,u\n\r\n\n\r", KW)]
    for rows in (1, 63, 64, 65, FIELD_BLOCK - 1, FIELD_BLOCK, FIELD_BLOCK + 1, scan_chunk - 1, scan_chunk, scan_chunk + 1):
        out.append((f"rows={rows} one column of each type", _row_table(rows), KW))
    wide = b",".join(b"c%d" % c for c in range(MAX_COLS)) + b"\n" + b"".join(b",".join(b"%d" % (r * 100 + c) for c in range(MAX_COLS)) + b"\n" for r in range(3))
    out.append((f"rows=3 columns={MAX_COLS}", wide, KW))
    return out


def too_many_columns_case():
    """MAX_COLS + 1 columns: nqe_csv_read must refuse it (InvalidArgument)"""
    n = MAX_COLS + 1
    return b",".join(b"c%d" % c for c in range(n)) + b"\n" + b",".join(b"%d" % c for c in range(n)) + b"\n"


GROUPS = tuple(f"slide_{e}" for e in SLIDE_EDGES[:-1]) + ("eof", "flip", "dense", "rows", "carry_slide", "carry_eof", "carry_flip", "carry_dense")


def all_cases(scan_chunk: int):
    """→ {group: [(label, bytes, kwargs)]}: the files the device test runs, grouped as it parametrises them (GROUPS); every file
    of CARRY_BYTES or more is in one of the carry_* groups"""
    groups = {f"slide_{edge}": [c[:3] for c in slide_cases(edge)] for edge in SLIDE_EDGES[:-1]}
    by_kind = {"slide": [c[:3] for c in slide_cases(CARRY_BYTES)], "eof": [c[:3] for c in eof_cases()], "flip": flip_pairs(), "dense": dense_cases()}
    for kind, cases in by_kind.items():
        groups[f"carry_{kind}"] = [c for c in cases if len(c[1]) >= CARRY_BYTES]
        if kind != "slide":
            groups[kind] = [c for c in cases if len(c[1]) < CARRY_BYTES]
    groups["rows"] = row_edge_cases(scan_chunk)
    assert tuple(sorted(groups)) == tuple(sorted(GROUPS))
    return groups
