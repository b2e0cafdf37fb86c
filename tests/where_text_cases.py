"""Selection of lines by the text of their fields (gzpx_where_text_device, gzpx_where_text_table_device), written once
and run twice: through the emulated library on CPU (tests/test_emu_where_text.py) and through the real HIP library on the
MI355X (tests/test_gpu_where_text.py).

The yardstick is never the library.  It is range_cases.Plain (zlib's inflate of every member, joined), the lines that
line_cases.Lines cuts, Python's bytes.split for the fields, Python's comparison of bytes and bytes.startswith for the
truth of a TEXT term, where_cases.term_truth on the cells of column_cases.Want for the numeric terms, and the edge
detection of where_cases.model on the selected rows of every range by itself.  Every comparison is exact.  The run table
is pre-filled with 0xEE and has GUARD entries behind runs_cap; entries behind n_runs and behind runs_cap must still be
0xEE."""
import ctypes

import numpy as np

import where_cases
from column_cases import FLT, INT, NL, OK, TAB, number_text
from field_cases import put_ranges
from gzp_amd import _native
from line_cases import Lines, Opened, cut
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem
from where_cases import EQ, FILL, FORMATS, GE, GT, GUARD, IS_OK, LE, LT, NE, NOT_OK, UNTOUCHED

TEXT = _native.COL_TEXT
PREFIX, NOT_PREFIX = _native.WHERE_PREFIX, _native.WHERE_NOT_PREFIX
TEXT_OPS = (LT, LE, EQ, NE, GE, GT, IS_OK, NOT_OK, PREFIX, NOT_PREFIX)
PIECE = 16384
K64 = bytes(range(0x30, 0x70))  # 64 distinct bytes, neither delimiter among them
K63 = K64[:63]
assert len(K64) == _native.WHERE_TEXT_MAX == 64 and (TEXT, PREFIX, NOT_PREFIX) == (2, 8, 9)


# ------------------------------------------------------------------------------------------------ the model
def text_truth(op, const, cell):
    """The truth of one TEXT term on one cell: the field's bytes, None when the line has no such field."""
    if op == IS_OK:
        return cell is not None
    if op == NOT_OK:
        return cell is None
    if cell is None:
        return False  # (NE and NOT_PREFIX too)
    return {LT: cell < const, LE: cell <= const, EQ: cell == const, NE: cell != const, GE: cell >= const, GT: cell > const,
            PREFIX: cell.startswith(const), NOT_PREFIX: not cell.startswith(const)}[op]


_parts = {}


def parts_of(ln, delim, fd):
    """The fields of every line, by bytes.split."""
    key = (id(ln), delim, fd)
    if key not in _parts:
        plain, st, d = ln.pl.plain, ln.start, bytes([delim])
        out = []
        for k in range(ln.L):
            line = plain[int(st[k]):int(st[k + 1])]
            out.append((line[:-1] if line.endswith(d) else line).split(bytes([fd])))
        _parts[key] = (ln, out)
    return _parts[key][1]


def passes(ln, delim, fd, terms, any_):
    """(bool[L]: the lines that pass, int[L]: the cells of the distinct fields that are not OK)."""
    parts = parts_of(ln, delim, fd)
    numeric = [t for t in terms if t[1] != TEXT]
    want = where_cases.want_of(ln, delim, fd, where_cases.columns_of(numeric)) if numeric else None
    at = {f: c for c, (f, _) in enumerate(where_cases.columns_of(numeric))}
    truths = []
    for field, kind, op, value in terms:
        if kind == TEXT:
            truths.append(np.array([text_truth(op, value, p[field] if field < len(p) else None) for p in parts], dtype=bool))
        else:
            truths.append(where_cases.term_truth(kind, op, value, want.st[at[field]], np.ascontiguousarray(want.val[at[field]])))
    bad = np.zeros(ln.L, dtype=np.int64)
    if want is not None:
        bad += (want.st != OK).sum(axis=0)
    for field in sorted({t[0] for t in terms if t[1] == TEXT}):
        bad += np.array([field >= len(p) for p in parts], dtype=np.int64)  # MISSING is a TEXT cell's only other status
    return (np.any(truths, axis=0) if any_ else np.all(truths, axis=0)), bad


def model(ln, delim, fd, ranges, terms, any_=False, invert=False):
    """(runs as line ranges in row order, selected rows, rows, cells that are not OK): where_cases.model with the truth
    of TEXT terms beside the numeric ones."""
    ok, bad = passes(ln, delim, fd, terms, any_)
    runs, selected, rows, not_ok = [], 0, 0, 0
    for a, b in ranges:
        if a >= b:
            continue
        sel = ok[a:b] != invert
        edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
        runs += [(a + int(i0), a + int(i1)) for i0, i1 in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1))]
        selected += int(sel.sum())
        rows += b - a
        not_ok += int(bad[a:b].sum())
    assert len(runs) <= (rows + len(ranges)) // 2
    return runs, selected, rows, not_ok


# ------------------------------------------------------------------------------------------------ the calls
def where(mem, o, ranges, fd, terms, any_=False, invert=False, cap=None, table=False, old=False):
    """where_cases.where through where_text_device / where_text_table_device (`old`: through the calls without text)."""
    n = len(ranges)
    keep, p, room = None, None, 0
    if cap is not None:
        room = (cap + GUARD) * 16
        keep, p = mem.put(bytes([FILL]) * room)
    host, dev = (o.d.where_lines_device, o.d.where_lines_table_device) if old else (o.d.where_text_device, o.d.where_text_table_device)
    try:
        if table:
            kr, rp = put_ranges(mem, ranges)
            got = dev(o.ix, o.lt, o.ptr, o.n, rp, n, fd, terms, any_, invert, p, cap or 0)
            if n:
                assert mem.get(kr, 16 * n) == np.array(ranges, dtype=np.uint64).tobytes(), "the range table was written"
        else:
            got = host(o.ix, o.lt, o.ptr, o.n, ranges, fd, terms, any_, invert, p, cap or 0)
    except _native.GzpxError as e:
        got = e
    return got, (np.frombuffer(mem.get(keep, room), dtype=np.uint64).reshape(-1, 2).tolist() if cap is not None else None)


def check(mem, o, ln, ranges, fd, terms, any_, invert, what, table=False, count=False, delim=NL):
    """The runs into a table of exactly n_runs entries (count: the count-only call in front of it)."""
    runs, selected, rows, not_ok = model(ln, delim, fd, ranges, terms, any_, invert)
    if count:
        got, _ = where(mem, o, ranges, fd, terms, any_, invert, None, table)
        assert got == (len(runs), selected, rows, not_ok), (what, "count only", got, (len(runs), selected, rows, not_ok))
    got, tb = where(mem, o, ranges, fd, terms, any_, invert, len(runs), table)
    assert got == (len(runs), selected, rows, not_ok), (what, "counts", got, (len(runs), selected, rows, not_ok))
    wrong = [i for i, r in enumerate(runs) if tb[i] != list(r)]
    assert not wrong, (what, "runs", wrong[:5], tb[wrong[0]], runs[wrong[0]])
    assert tb[len(runs):] == [[UNTOUCHED, UNTOUCHED]] * GUARD, (what, "written behind runs_cap")
    ms = o.d.last_where_ms()
    assert all(t >= 0.0 for t in ms), (what, ms)
    return runs


def raw_text(lib, o, ranges, fd, raw_terms, n_terms, flags, text, text_len, cap=0, mem=None, d_runs=None, table=False, runs=False):
    """The C call itself: (rc, (n_runs, n_selected, n_rows, n_not_ok), the table's entries or None), the counts preset to
    77.  `text` is bytes or None; text_len is passed as given.  runs: into a table of its own, cap + GUARD entries."""
    r = np.ascontiguousarray(np.array(ranges, dtype=np.uint64).reshape(-1, 2))
    tm = np.zeros(max(len(raw_terms), 1), dtype=_native.WHERE_TERM_DTYPE)
    for i, t in enumerate(raw_terms):
        tm[i] = t
    keep = None
    if runs:
        keep, d_runs = mem.put(bytes([FILL]) * 16 * (cap + GUARD))
    c = [ctypes.c_uint64(77) for _ in range(4)]
    bad, info = ctypes.c_size_t(77), _native.GzpxCheckInfo()
    fn, rp = lib.L.gzpx_where_text_device, r.ctypes.data
    if table:
        kr, rp = put_ranges(mem, ranges)
        fn = lib.L.gzpx_where_text_table_device
    rc = fn(o.d.h, o.ix.h, o.lt.h, o.ptr, o.n, rp, r.shape[0], fd, tm.ctypes.data, n_terms, text, text_len, flags, d_runs, cap,
            ctypes.byref(c[0]), ctypes.byref(c[1]), ctypes.byref(c[2]), ctypes.byref(c[3]), ctypes.byref(bad), ctypes.byref(info), None)
    tb = np.frombuffer(mem.get(keep, 16 * (cap + GUARD)), dtype=np.uint64).reshape(-1, 2).tolist() if keep is not None else None
    return rc, tuple(x.value for x in c), tb


def at(offset, length):
    """A TEXT term's value."""
    return offset | length << 32


# ------------------------------------------------------------------------------------------------ 1. operators
OP_CELLS = [K64, K63, K64[:62], K64 + b"x", K64 + b"xy", K64 + b"z" * (5000 - 64),          # equal, proper prefixes, 65, 66, 5,000 bytes
            K63 + b"~", K63 + b"!", b"1" + K64[1:], b"/" + K64[1:], K63[:40] + b"~" + K63[41:],  # differences at the last byte and at byte 0
            K63 + b"\x80", K63 + b"\xff", K64[:62] + b"\x80", K64[:62] + b"\x80" + b"o",         # bytes >= 0x80 against bytes < 0x80
            b"\x80", b"\x7f", b"\xff\xff\xff", b"\x81", b"A", b"B", b"@", b"AB", b"A\x00", b"\x00", b"\x00\x00", b"A\rB", b"\r",
            b"", b"0", b"00", b"a", K64 * 3]
OP_CONSTANTS = (b"", b"A", b"\x80", K63, K64, K63[:62] + b"\x80", K63 + b"\x80", b"A\x00", b"\r")
assert sorted({len(c) for c in OP_CONSTANTS}) == [0, 1, 2, 63, 64]


def operators(lib):
    """Column 1 holds hand-written cells; every third line has one field more in front of them, and some lines have no
    field 1 at all.  All ten ops against constants of 0, 1, 63 and 64 bytes, one term a call; then MISSING by itself."""
    mem = Mem(lib)
    lines = []
    for i, f in enumerate(OP_CELLS):
        lines += [b"%d\t%s\t%d\n" % (i, f, i % 7), b"%d\t%s\n" % (i, f)]  # (the cell in the middle of its line and at its end)
        if i % 5 == 0:
            lines.append(b"%d\n" % i)  # MISSING
    text = b"".join(lines)
    for fmt in FORMATS:
        s = cut(fmt, text, [len(text) // 2])
        ln = Lines(Plain(fmt, s), NL)
        whole = [(0, ln.L)]
        cells = [p[1] if len(p) > 1 else None for p in parts_of(ln, NL, TAB)]
        assert set(OP_CELLS) <= set(cells) and None in cells
        # the model itself on the pairs a wrong compare gets wrong: signed bytes, length before content, the 65th byte
        assert text_truth(GT, b"A", b"\x80") and text_truth(LT, K63 + b"\x80", K64) and text_truth(GT, K64, K64 + b"x")
        assert text_truth(LT, K64, K63) and text_truth(EQ, b"", b"") and text_truth(PREFIX, b"", b"\x00") and not text_truth(NE, K64, None)
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for j, const in enumerate(OP_CONSTANTS):
                for op in TEXT_OPS:
                    if op in (IS_OK, NOT_OK) and j:
                        continue
                    runs = check(mem, o, ln, whole, TAB, [(1, TEXT, op, b"" if op in (IS_OK, NOT_OK) else const)], False, False,
                                 ("one term", fmt, op, const), table=(j + op) % 2 == 1)
                    if op == EQ and const == K64:
                        assert sum(b - a for a, b in runs) == 2, "only the field that is the constant equals it"
            # MISSING: from the lane that closes the line; false for NE and NOT_PREFIX, seen by the status ops
            assert check(mem, o, ln, whole, TAB, [(3, TEXT, NOT_OK, b"")], False, False, ("missing", fmt)) == [(0, ln.L)]
            for op in (NE, NOT_PREFIX, GE, PREFIX):
                assert check(mem, o, ln, whole, TAB, [(3, TEXT, op, b"")], False, False, ("missing", fmt, op)) == []
            got, _ = where(mem, o, whole, TAB, [(1, TEXT, IS_OK, None)], cap=None)
            assert got[3] == cells.count(None), "n_not_ok counts the MISSING cells of a TEXT field"


# ------------------------------------------------------------------------------------------------ 2. the edges of the walk
def filler(n):
    """n >= 16 bytes of whole lines of three fields."""
    out = [b"00\tabcdefgh\t1.5\n"] * (n // 16 - 1)
    r = n - 16 * (n // 16 - 1)  # 16 <= r < 32
    return b"".join(out) + b"00\t" + b"q" * (r - 8) + b"\t1.5\n"


EDGE_VARIANTS = (K64, K64 + b"p", K64[:63] + b"~", K64[:30])  # equal, longer, greater at the last byte, a proper prefix


def boundary_text(ds):
    """Lines of three fields.  For the j-th d of `ds`, field 1 of one line starts d bytes in front of byte 16384 (j + 1)
    of the text: with d = 0 its opener is the last byte in front of that boundary, otherwise d of its bytes lie in front of
    it.  The field agrees with K64 in its first min(d + 1, its length) bytes at least: what decides it lies behind the
    boundary.  Returns (text, where those fields start)."""
    out, size, starts = [], 0, []
    for j, d in enumerate(ds):
        head = b"%02d\t" % (j % 100)
        gap = PIECE * (j + 1) - d - len(head) - size
        assert gap >= 16
        field = EDGE_VARIANTS[(j + d) % 4]
        if d >= len(field):
            field = K64  # (the field has to reach the boundary)
        line = head + field + b"\t%d.5\n" % (j % 10)
        out += [filler(gap), line]
        starts.append(size + gap + len(head))
        size += gap + len(line)
    out.append(filler(40))
    return b"".join(out), starts


EDGE_TERMS = (([(1, TEXT, EQ, K64)], False), ([(1, TEXT, GT, K64), (1, TEXT, PREFIX, K64[:31])], False),
              ([(0, TEXT, GE, b"05"), (1, TEXT, NE, K64), (1, TEXT, NOT_PREFIX, b"q")], False),
              ([(1, TEXT, LT, K64[:30] + b"0"), (1, TEXT, EQ, K63 + b"~"), (2, FLT, GE, 8.0)], True),
              ([(0, TEXT, EQ, b"07"), (2, TEXT, PREFIX, b"3.")], True))


def edges(lib):
    """Against the 16 KiB piece: a TEXT field whose opener is a piece's last byte, fields with 1 to 64 of their bytes in
    front of the boundary (a quarter of the distances in each pair of format and route), members that end inside such a
    field, ranges whose first line's first field has a term, ranges that end at the stream's end, terminated or not."""
    mem = Mem(lib)
    for i in range(6):
        fmt, route = FORMATS[i % 2], ROUTES[(i // 2) % 2]
        # every distance once, a quarter of them a stream and the three term sets that tell the variants apart; then two
        # short streams with every set of terms on sets of ranges
        ds = list(range(i, 65, 4)) if i < 4 else [0, 7, 64]
        text, starts = boundary_text(ds)
        if i % 2:
            text = text[:-1]  # the last line is unterminated
        for d, at_ in zip(ds, starts):
            assert (at_ + d) % PIECE == 0 and text[at_ - 1] == TAB
        s = cut(fmt, text, [at_ + 3 for at_ in starts[::3]])  # members end inside every third of those fields
        pl = Plain(fmt, s)
        assert pl.plain == text
        ln = Lines(pl, NL)
        if i < 4:
            sets, term_sets = [[(0, ln.L)]], EDGE_TERMS[:3]
        else:
            sets = [[(0, ln.L)], [(k, ln.L) for k in (1, 2, 5)] + [(ln.L - 1, ln.L)], [(3, ln.L - 7), (ln.L - 3, ln.L)]]
            term_sets = EDGE_TERMS
        with Opened(lib, mem, fmt, s, NL, route) as o:
            for j, rs in enumerate(sets):
                for k, (terms, any_) in enumerate(term_sets):
                    invert = bool((i + j + k) % 2) and k > 0
                    runs = check(mem, o, ln, rs, TAB, terms, any_, invert, ("edges", fmt, route, rs[:2], terms), table=(j + k) % 2 == 1)
                    if i < 4 and k == 0:
                        assert len(runs) >= 3, "fields that equal the constant across a boundary"
    past_the_end(lib, mem)


def past_the_end(lib, mem):
    """The range's last line is unterminated and its last field is a proper prefix of the constant, while the bytes behind
    the range's end continue the constant: the call in front of it, in the same context, inflated a stream whose text goes
    on with them.  A compare that reads behind `end` selects the last row."""
    head = b"".join(b"%03d\tfill\t%s\n" % (k, K64) for k in range(50))
    long, short = head + b"xx\tyy\t" + K64 + b"\n", head + b"xx\tyy\t" + K64[:40]
    for fmt in FORMATS:
        for route in ROUTES:
            with Opened(lib, mem, fmt, cut(fmt, long, [100])) as o:
                keep, ptr = mem.put(cut(fmt, short, [100]))
                n = len(cut(fmt, short, [100]))
                pl = Plain(fmt, cut(fmt, short, [100]))
                ln = Lines(pl, NL)
                assert ln.L == 51 and pl.plain == short
                o.d.set_route(route)
                with o.d.build_index_device(ptr, n) as ix, o.d.build_lines_device(ix, ptr, n, NL) as lt:
                    second = type("O", (), dict(d=o.d, ix=ix, lt=lt, ptr=ptr, n=n))
                    for terms, want_last in (([(2, TEXT, EQ, K64)], False), ([(2, TEXT, PREFIX, K64[:41])], False),
                                             ([(2, TEXT, GE, K64[:41])], False), ([(2, TEXT, LT, K64)], True),
                                             ([(2, TEXT, EQ, K64[:40])], True)):
                        for table in (False, True):
                            got, _ = where(mem, o, [(0, 51)], TAB, terms, cap=60, table=table)  # the longer text into staging
                            assert not isinstance(got, Exception)
                            for rs in ([(0, 51)], [(50, 51)], [(10, 51), (50, 51)]):
                                runs = check(mem, second, ln, rs, TAB, terms, False, False, ("past the end", fmt, route, terms, rs), table=table)
                                assert (runs[-1][1] == 51 if runs else False) == want_last, (fmt, route, terms, rs)


# ------------------------------------------------------------------------------------------------ 3. mixed and most
WORDS = (b"chr1", b"chr7", b"chr10", b"chrX", b"", b"PASS", b"PASS;q10", b"q10", b"\xc3\xa9t\xc3\xa9")


def mixed_text(n_rows, seed):
    """Rows of 8 fields: a word, an integer, a word, a %.6g float, an integer, a word, and sometimes two more."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_rows):
        w = [WORDS[int(k)] for k in rng.integers(0, len(WORDS), 4)]
        p = [w[0], b"%d" % int(rng.integers(-50, 50)), w[1], b"%.6g" % float(rng.normal() * 30.0), b"%d" % int(rng.integers(0, 9)), w[2]]
        k = int(rng.integers(0, 4))
        out.append(b"\t".join(p + [b"x", w[3]][:max(k - 1, 0)] if k else p[:3]) + b"\n")
    return b"".join(out)


MIXED_SETS = ([(0, TEXT, EQ, b"chr7"), (3, FLT, GE, 0.0), (5, TEXT, PREFIX, b"PASS")],
              [(0, TEXT, PREFIX, b"chr1"), (1, INT, LT, 0), (2, TEXT, NE, b""), (3, FLT, NOT_OK, 0)],
              [(0, TEXT, GE, b"chr10"), (0, TEXT, LT, b"chrX"), (1, INT, GE, -25), (4, INT, IS_OK, 0), (7, TEXT, IS_OK, None)],
              [(1, INT, EQ, 7), (5, TEXT, EQ, b"\xc3\xa9t\xc3\xa9"), (7, TEXT, NOT_PREFIX, b"chr"), (7, TEXT, NOT_OK, None)])


def mixed(lib):
    """TEXT, INT64 and FLOAT64 terms in one call under ALL, ANY and INVERT, host form and table form."""
    mem = Mem(lib)
    text = mixed_text(700, 31)
    for fmt in FORMATS:
        s = cut(fmt, text, [len(text) // 3])
        ln = Lines(Plain(fmt, s), NL)
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == BGZF]) as o:
            for k, terms in enumerate(MIXED_SETS):
                for any_ in (False, True):
                    for invert in (False, True):
                        rs = [(0, ln.L), (100, 300), (40, 40)]
                        runs = check(mem, o, ln, rs, TAB, terms, any_, invert, ("mixed", fmt, k, any_, invert), table=(k + invert) % 2 == 1,
                                     count=k == 0)
                        assert k or any_ or invert or 0 < sum(b - a for a, b in runs) < ln.L // 4  # (some rows pass and most do not)


def most(lib):
    """32 TEXT terms with 32 distinct constants of 64 bytes -- the pool full -- on 16 distinct fields; then constants that
    overlap in the pool, through the C call."""
    mem = Mem(lib)
    rng = np.random.default_rng(9)
    consts = [[bytes(rng.integers(0x21, 0x7F, 64).astype(np.uint8)) for _ in range(3)] for _ in range(16)]
    for f in range(16):
        consts[f][1] = consts[f][0][:63] + bytes([consts[f][0][63] ^ 1])  # (two of a field's three agree in 63 bytes)
    rows = rng.choice(3, (300, 16), p=(0.04, 0.04, 0.92))
    text = b"".join(b"7\tx\t" + b"\t".join(consts[f][v] + (b"+" if (k + f) % 11 == 0 else b"") for f, v in enumerate(r)) + b"\n"
                    for k, r in enumerate(rows))
    terms = []
    for f in range(16):
        terms += [(f + 2, TEXT, NE, consts[f][0]), (f + 2, TEXT, NOT_PREFIX, consts[f][1])]
    tm, pool = _native.DContext.where_text_terms(terms)
    assert len(terms) == _native.WHERE_MAX_TERMS and len(pool) == _native.WHERE_TEXT_POOL_MAX == 2048 and len(set(t[3] for t in terms)) == 32
    s = cut(BGZF, text, [30000, 60000, 90000, 150000, 210000])
    ln = Lines(Plain(BGZF, s), NL)
    with Opened(lib, mem, BGZF, s) as o:
        for any_ in (False, True):
            for invert in (False, True):
                runs = check(mem, o, ln, [(0, ln.L), (100, 200)], TAB, terms, any_, invert, ("32 terms", any_, invert), table=invert)
                assert any_ or invert or 20 < sum(b - a for a, b in runs) < 380
        rare = [(f, k, EQ if op == NE else PREFIX, v) for f, k, op, v in terms]
        check(mem, o, ln, [(0, ln.L)], TAB, rare, True, False, "32 equalities and prefixes")
    overlapping(lib, mem)


def overlapping(lib, mem):
    """Constants that share the pool's bytes: "chr1", "chr12", "chr" and "12" out of the five bytes "chr12", and the empty
    constant at the pool's end."""
    text = b"".join(b"%s\t%s\n" % (a, b) for a in (b"chr1", b"chr12", b"chr", b"12", b"chr2", b"") for b in (b"12", b"chr12", b"1", b""))
    pool = b"chr12"
    raw = [(0, TEXT, GE, at(0, 4)), (0, TEXT, LE, at(0, 5)), (0, TEXT, PREFIX, at(0, 3)), (1, TEXT, NE, at(3, 2)), (1, TEXT, PREFIX, at(5, 0))]
    same = [(0, TEXT, GE, b"chr1"), (0, TEXT, LE, b"chr12"), (0, TEXT, PREFIX, b"chr"), (1, TEXT, NE, b"12"), (1, TEXT, PREFIX, b"")]
    for fmt in FORMATS:
        s = cut(fmt, text, [33])
        ln = Lines(Plain(fmt, s), NL)
        with Opened(lib, mem, fmt, s) as o:
            for flags, any_, invert in ((0, False, False), (_native.WHERE_ANY | _native.WHERE_INVERT, True, True)):
                runs, selected, rows, not_ok = model(ln, NL, TAB, [(0, ln.L)], same, any_, invert)
                assert any_ or runs == [(1, 4), (5, 8)]  # chr1 and chr12 with anything but 12 behind them
                for table in (False, True):
                    rc, counts, tb = raw_text(lib, o, [(0, ln.L)], TAB, raw, len(raw), flags, pool, len(pool), cap=len(runs), mem=mem, table=table, runs=True)
                    assert (rc, counts) == (_native.OK, (len(runs), selected, rows, not_ok)), (fmt, flags, table, counts)
                    assert tb == [list(r) for r in runs] + [[UNTOUCHED, UNTOUCHED]] * GUARD, (fmt, flags, table)


# ------------------------------------------------------------------------------------------------ 4. equivalence
def equivalence(lib):
    """Terms on numbers alone through the new calls: the runs and the counts of the old calls, compared directly."""
    mem = Mem(lib)
    text = number_text(30000, 5)
    sets = ([(0, INT, GE, 0), (1, FLT, LT, 1.0)], [(1, FLT, NOT_OK, 0)], [(0, INT, LT, -10 ** 8), (0, INT, NE, 7), (4, INT, IS_OK, 0), (6, FLT, GT, 0.5)])
    for fmt in FORMATS:
        s = cut(fmt, text, [17000])
        ln = Lines(Plain(fmt, s), NL)
        rs = [(0, ln.L), (ln.L // 2, ln.L), (3, 3), (7, 90)]
        cap = (ln.L * 2 + 4) // 2
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for terms in sets:
                for k, (any_, invert) in enumerate(((False, False), (False, True), (True, False), (True, True))):
                    table = (k + (fmt == MGZIP)) % 2 == 1  # (both forms under every pair of flags, one a format)
                    new = where(mem, o, rs, TAB, terms, any_, invert, cap, table)
                    old = where(mem, o, rs, TAB, terms, any_, invert, cap, table, old=True)
                    assert new == old and not isinstance(new[0], Exception) and new[0][2] > 0, (fmt, terms, any_, invert, table)
                    if k == 0:
                        assert where(mem, o, rs, TAB, terms, any_, invert, None, table)[0] == old[0]
            runs = check(mem, o, ln, rs, TAB, sets[0], True, False, ("equivalence", fmt))  # and the model agrees
            assert len(runs) > 50


# ------------------------------------------------------------------------------------------------ 5. closing the loop
def vcf_text(n_rows, seed):
    """Rows like a VCF's: CHROM POS ID REF ALT QUAL FILTER INFO, the INFO holding what FILTER and CHROM may hold."""
    rng = np.random.default_rng(seed)
    chroms, filters = (b"chr1", b"chr7", b"chr17", b"chr10", b"chrX", b"7"), (b"PASS", b"q10", b"LowQual;PASS", b"PASS;x", b".")
    out = []
    for k in range(n_rows):
        qual = b"." if rng.integers(0, 9) == 0 else b"%.1f" % float(rng.uniform(0, 80))
        info = b"DP=%d;F=%s;C=%s" % (int(rng.integers(1, 99)), filters[int(rng.integers(0, 5))], chroms[int(rng.integers(0, 6))])
        out.append(b"\t".join([chroms[int(rng.integers(0, 6))], b"%d" % (1000 + 37 * k), b"rs%d" % k if k % 4 else b".", b"ACGT"[k % 4:k % 4 + 1],
                               b"ACGT"[(k + 1) % 4:(k + 1) % 4 + 1], qual, filters[int(rng.integers(0, 5))], info]) + b"\n")
    return b"".join(out)


def close_the_loop(lib):
    """grep rs | awk '($1 == "chr7" || $1 == "chr17" || $1 == "chrX") && $7 == "PASS" && $6 >= 30' | cut -f 1,2,6 on the device:
    select_lines_device, its table into where_text_table_device under ANY (CHROM in a set), that table into
    where_text_table_device (the chained AND), that into read_fields_table_device; against the same pipeline in Python."""
    mem = Mem(lib)
    text = vcf_text(900, 3)
    in_set = [(0, TEXT, EQ, c) for c in (b"chr17", b"chr7", b"chrX")]
    rest = [(5, FLT, GE, 30.0), (6, TEXT, EQ, b"PASS")]
    for fmt in FORMATS:
        s = cut(fmt, text, [40, 21000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        all_lines = pl.plain.splitlines(keepends=True)
        assert len(all_lines) == ln.L
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            grep = [k for k, x in enumerate(all_lines) if b"rs" in x]
            cap_g = -(-ln.L // 2)
            kg, pg = mem.put(bytes([FILL]) * 16 * cap_g)
            n_g, n_rec, _ = o.d.select_lines_device(o.ix, o.lt, o.ptr, o.n, b"rs", 1, False, pg, cap_g)
            assert n_g >= 2 and n_rec == len(grep)
            g_runs = [tuple(r) for r in np.frombuffer(mem.get(kg, 16 * n_g), dtype=np.uint64).reshape(-1, 2).tolist()]
            runs_1, sel_1, rows_1, bad_1 = model(ln, NL, TAB, g_runs, in_set, any_=True)
            cap_1 = (rows_1 + n_g) // 2
            k1, p1 = mem.put(bytes([FILL]) * 16 * (cap_1 + GUARD))
            got = o.d.where_text_table_device(o.ix, o.lt, o.ptr, o.n, pg, n_g, TAB, in_set, True, False, p1, cap_1)
            assert got == (len(runs_1), sel_1, rows_1, bad_1) and rows_1 == len(grep), (fmt, got)
            tb = np.frombuffer(mem.get(k1, 16 * (cap_1 + GUARD)), dtype=np.uint64).reshape(-1, 2).tolist()
            assert tb[:len(runs_1)] == [list(r) for r in runs_1] and tb[len(runs_1):] == [[UNTOUCHED, UNTOUCHED]] * (cap_1 + GUARD - len(runs_1))
            runs_2, sel_2, rows_2, bad_2 = model(ln, NL, TAB, runs_1, rest)
            cap_2 = (rows_2 + len(runs_1)) // 2
            k2, p2 = mem.put(bytes([FILL]) * 16 * (cap_2 + GUARD))
            got = o.d.where_text_table_device(o.ix, o.lt, o.ptr, o.n, p1, len(runs_1), TAB, rest, False, False, p2, cap_2)
            assert got == (len(runs_2), sel_2, rows_2, bad_2) and rows_2 == sel_1, (fmt, got)
            first = mem.get(k2, 16 * (cap_2 + GUARD))
            tb = np.frombuffer(first, dtype=np.uint64).reshape(-1, 2).tolist()
            assert tb[:len(runs_2)] == [list(r) for r in runs_2] and tb[len(runs_2):] == [[UNTOUCHED, UNTOUCHED]] * (cap_2 + GUARD - len(runs_2))
            # a second call: the same bytes
            assert o.d.where_text_table_device(o.ix, o.lt, o.ptr, o.n, p1, len(runs_1), TAB, rest, False, False, p2, cap_2) == got
            assert mem.get(k2, 16 * (cap_2 + GUARD)) == first
            # the pipeline in Python, by the rows' own text
            keepers = []
            for k in grep:
                p = all_lines[k][:-1].split(b"\t")
                try:
                    q = float(p[5])
                except ValueError:
                    continue
                if p[0] in (b"chr7", b"chr17", b"chrX") and p[6] == b"PASS" and q >= 30.0:
                    keepers.append(k)
            assert keepers == [k for a, b in runs_2 for k in range(a, b)] and 10 < len(keepers) < len(grep) // 4
            expect = b"".join(b"\t".join(all_lines[k][:-1].split(b"\t")[i] for i in (0, 1, 5)) + b"\n" for k in keepers)
            ko, po = mem.put(bytes([FILL]) * (len(expect) + 64))
            assert o.d.read_fields_table_device(o.ix, o.lt, o.ptr, o.n, p2, got[0], TAB, [(0, 2), (5, 6)], po, len(expect)) == len(expect)
            assert mem.get(ko, len(expect) + 64) == expect + bytes([FILL]) * 64, fmt


# ------------------------------------------------------------------------------------------------ 6. capacity, errors, a damaged member
def capacity(lib):
    mem = Mem(lib)
    text = vcf_text(600, 8)
    terms = [(0, TEXT, PREFIX, b"chr1"), (5, FLT, GE, 40.0), (6, TEXT, EQ, b"PASS")]
    for fmt in FORMATS:
        s = cut(fmt, text, [17000])
        ln = Lines(Plain(fmt, s), NL)
        rs = [(0, ln.L), (ln.L // 2, ln.L), (3, 3)]
        want_runs, selected, rows, not_ok = model(ln, NL, TAB, rs, terms, True)
        n = len(want_runs)
        totals = (n, selected, rows, not_ok)
        assert n > 50
        with Opened(lib, mem, fmt, s) as o:
            for table in (False, True):
                assert where(mem, o, rs, TAB, terms, True, False, None, table)[0] == totals  # d_runs == NULL counts
                for cap in (0, n - 1):
                    e, tb = where(mem, o, rs, TAB, terms, True, False, cap, table)
                    assert isinstance(e, _native.GzpxError) and (e.code, e.needed) == (_native.ERR_INSUFFICIENT_SPACE, n), (fmt, table, cap)
                    assert tb[:cap] == [list(r) for r in want_runs[:cap]], (fmt, table, cap, "the first runs_cap runs")
                    assert tb[cap:] == [[UNTOUCHED, UNTOUCHED]] * GUARD, (fmt, table, cap, "written behind runs_cap")
                    tm, pool = _native.DContext.where_text_terms(terms)
                    rc, counts, _ = raw_text(lib, o, rs, TAB, [tuple(int(x) for x in t) for t in tm.tolist()], len(terms), _native.WHERE_ANY,
                                             pool, len(pool), cap=cap, mem=mem, table=table, runs=True)
                    assert (rc, counts) == (_native.ERR_INSUFFICIENT_SPACE, totals), (fmt, cap, "the totals always come back")
                got, tb = where(mem, o, rs, TAB, terms, True, False, n + 7, table)
                assert got == totals and tb == [list(r) for r in want_runs] + [[UNTOUCHED, UNTOUCHED]] * (7 + GUARD), "entries behind n_runs"


def errors(lib):
    """Every rule of a TEXT term and of the pool: GZPX_ERR_INVALID_ARG, all counts 0, nothing inflated, the table
    untouched.  What the rules allow at their edges is GZPX_OK."""
    mem = Mem(lib)
    text = vcf_text(200, 5)
    INV = _native.ERR_INVALID_ARG
    pool = K64 + b"chr7"
    for fmt in FORMATS:
        s = cut(fmt, text, [3000])
        pl = Plain(fmt, s)
        L = Lines(pl, NL).L
        with Opened(lib, mem, fmt, s) as o:
            whole = [(0, L)]
            kr, pr = mem.put(bytes([FILL]) * 16 * 64)
            big = bytes(2049)
            cases = (("len 65", [(0, TEXT, EQ, at(0, 65))], pool, len(pool)), ("offset + len > text_len", [(0, TEXT, EQ, at(65, 4))], pool, len(pool)),
                     ("offset > text_len", [(0, TEXT, EQ, at(69, 0))], pool, len(pool)), ("offset + len wraps 32 bits", [(0, TEXT, EQ, at(0xFFFFFFFF, 2))], pool, len(pool)),
                     ("a constant and no pool", [(0, TEXT, EQ, at(0, 1))], None, 0), ("text_len 2049", [(0, TEXT, EQ, at(0, 4))], big, 2049),
                     ("text_len 2049, numeric terms", [(1, INT, GE, 0)], big, 2049), ("text NULL, text_len 4", [(0, TEXT, EQ, at(0, 4))], None, 4),
                     ("text NULL, text_len 4, numeric terms", [(1, INT, GE, 0)], None, 4),
                     ("PREFIX on INT64", [(1, INT, PREFIX, 0)], pool, len(pool)), ("NOT_PREFIX on FLOAT64", [(5, FLT, NOT_PREFIX, 0)], pool, len(pool)),
                     ("IS_OK with a value", [(0, TEXT, IS_OK, at(0, 4))], pool, len(pool)), ("NOT_OK with a value", [(0, TEXT, NOT_OK, 1)], pool, len(pool)),
                     ("IS_OK with a value, INT64", [(1, INT, IS_OK, 1)], pool, len(pool)),
                     ("two types on one field", [(0, TEXT, EQ, at(64, 4)), (0, INT, GE, 0)], pool, len(pool)),
                     ("two types on one field, TEXT behind", [(5, FLT, GE, 0), (5, TEXT, NE, at(0, 0))], pool, len(pool)),
                     ("op 10", [(0, TEXT, 10, at(0, 4))], pool, len(pool)), ("type 3", [(0, 3, EQ, at(0, 4))], pool, len(pool)),
                     ("descending fields", [(6, TEXT, EQ, at(0, 4)), (0, TEXT, EQ, at(0, 4))], pool, len(pool)))
            for table in (False, True):
                for what, raw, tx, tl in cases:
                    rc, counts, _ = raw_text(lib, o, whole, TAB, raw, len(raw), 0, tx, tl, cap=16, mem=mem, d_runs=pr, table=table)
                    assert (rc, counts) == (INV, (0, 0, 0, 0)), (fmt, table, what, rc, counts)
                    assert o.d.last_lines_members() == 0, (fmt, table, what)
                    assert mem.get(kr, 16 * 64) == bytes([FILL]) * 16 * 64, (fmt, table, what)
                    assert raw_text(lib, o, [(0, 1)], TAB, [(0, TEXT, EQ, at(64, 4))], 1, 0, pool, len(pool))[0] == _native.OK  # (something is inflated in between)
                    assert o.d.last_lines_members() > 0
            # the edges of the rules
            full = bytes(range(256)) * 8
            ok_cases = (("len 64 at the pool's end", [(0, TEXT, NE, at(2048 - 64, 64))], full, 2048), ("len 0 at text_len", [(0, TEXT, PREFIX, at(68, 0))], pool, 68),
                        ("no pool, no constants", [(0, TEXT, IS_OK, 0), (1, INT, GE, 0)], None, 0), ("the empty constant of an empty pool", [(0, TEXT, NE, 0)], None, 0),
                        ("a pool that no term uses", [(1, INT, GE, 0)], pool, len(pool)))
            for what, raw, tx, tl in ok_cases:
                rc, counts, _ = raw_text(lib, o, whole, TAB, raw, len(raw), 0, tx, tl)
                assert rc == _native.OK and counts[1] == counts[2] == L, (fmt, what, rc, counts)
            # a bad line range, in both forms: the existing report
            for table in (False, True):
                e, tb = where(mem, o, [(0, 2), (L - 1, L + 1)], TAB, [(0, TEXT, EQ, b"chr7")], False, False, 16, table)
                assert isinstance(e, _native.GzpxError) and (e.code, e.range_index) == (INV, 1), (fmt, table)
                assert tb == [[UNTOUCHED, UNTOUCHED]] * (16 + GUARD) and o.d.last_lines_members() == 0
                assert where(mem, o, [], TAB, [(0, TEXT, EQ, b"chr7")], False, True, 4, table) == ((0, 0, 0, 0), [[UNTOUCHED, UNTOUCHED]] * (4 + GUARD))
            # the calls without text keep refusing what is new, and the columns refuse the type
            for raw in ([(0, TEXT, EQ, 0)], [(1, INT, PREFIX, 0)], [(1, INT, NOT_PREFIX, 0)]):
                assert where_cases.raw_where(lib, o, whole, TAB, raw, 1, 0) == (INV, (0, 0, 0, 0))
            try:
                o.d.read_columns_device(o.ix, o.lt, o.ptr, o.n, whole, TAB, [(0, TEXT)], None, None, 0)
                raise AssertionError("read_columns_device took GZPX_COL_TEXT")
            except _native.GzpxError as e:
                assert e.code == INV


def damaged(lib):
    """A member with a damaged CRC that the ranges touch: the inflate's error class and the member's index, all counts 0,
    the table untouched; the context serves on."""
    mem = Mem(lib)
    terms = [(0, TEXT, PREFIX, b"chr1"), (5, FLT, NOT_OK, 0), (6, TEXT, EQ, b"PASS")]
    tm, pool = _native.DContext.where_text_terms(terms)
    raw = [tuple(int(x) for x in t) for t in tm.tolist()]
    text = vcf_text(700, 12)
    for fmt in FORMATS:
        s = cut(fmt, text, [5000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        route = ROUTES[fmt == BGZF]
        with Opened(lib, mem, fmt, s, route=route) as o:  # (the table of the undamaged stream)
            for victim in (0, 3, 7):
                m = bytearray(s)
                m[pl.off[victim] + pl.size[victim] - 8] ^= 0xFF
                keep, ptr = mem.put(m)
                with o.d.build_index_device(ptr, len(m)) as ix:  # (the members' extents are the same: the table serves)
                    bad = type("O", (), dict(d=o.d, ix=ix, lt=o.lt, ptr=ptr, n=len(m)))
                    for table in (False, True):
                        e, tb = where(mem, bad, [(0, ln.L)], TAB, terms, True, False, 8, table)
                        assert isinstance(e, _native.GzpxError), (fmt, victim, e)
                        assert (e.code, e.block, e.needed) == (_native.ERR_INVALID_CHECK, victim, None), (fmt, route, victim, table)
                        assert tb == [[UNTOUCHED, UNTOUCHED]] * (8 + GUARD)
                    rc, counts, _ = raw_text(lib, bad, [(0, ln.L)], TAB, raw, len(raw), 0, pool, len(pool))
                    assert (rc, counts) == (_native.ERR_INVALID_CHECK, (0, 0, 0, 0)), (fmt, victim, "the counts of a failing member")
            check(mem, o, ln, [(0, ln.L)], TAB, terms, True, False, (fmt, route, "after the damage"), count=True)
