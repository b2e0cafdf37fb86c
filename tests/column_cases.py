"""Numeric columns of lines (gzpx_read_columns_device, gzpx_read_columns_table_device), written once and run twice:
through the emulated library on CPU (tests/test_emu_columns.py) and through the real HIP library on the MI355X
(tests/test_gpu_columns.py).

The yardstick is never the library.  It is range_cases.Plain (zlib's inflate of every member, joined), the lines that
line_cases.Lines cuts, body.split(fd), and a Python model of include/gzpx.h's rules: the two regular expressions,
int(), and the w / q rule with Python integers.  For every OK float cell the model itself is checked against
struct.pack('<d', float(s)).  Every comparison is exact.  The outputs are pre-filled with 0xEE, the value array
misaligned by 8 bytes x an odd count and the status array by 3 bytes; the cells behind R in every column and 64 bytes
behind the arrays must still be 0xEE."""
import ctypes
import re
import struct

import numpy as np
import pytest

from gzp_amd import _native
from field_cases import put_ranges, range_set
from line_cases import Lines, Opened, cut
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem

NL, TAB = 0x0A, 0x09
FILL = 0xEE
GUARD = 64
PIECE = 16384
FORMATS = (BGZF, MGZIP)
INT, FLT = _native.COL_INT64, _native.COL_FLOAT64
OK, MISSING, EMPTY, INVALID, RANGE = (_native.CELL_OK, _native.CELL_MISSING, _native.CELL_EMPTY, _native.CELL_INVALID,
                                      _native.CELL_RANGE)
NAN = 0x7FF8000000000000
MASK = (1 << 64) - 1
UNTOUCHED = int.from_bytes(bytes([FILL]) * 8, "little")


# ------------------------------------------------------------------------------------------------ the model
INT_RE = re.compile(rb"[+-]?[0-9]+")
FLT_RE = re.compile(rb"[+-]?(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")
SPC_RE = re.compile(rb"[+-]?(nan|inf|infinity)", re.I)
_cells = {}


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def model(field, kind):
    """(status, the cell as a 64-bit pattern) of a field's bytes; None: the line has no such field."""
    bad = 0 if kind == INT else NAN
    if field is None:
        return MISSING, bad
    if len(field) == 0:
        return EMPTY, bad
    if len(field) > _native.CELL_MAX_BYTES:
        return INVALID, bad
    if kind == INT:
        if not INT_RE.fullmatch(field):
            return INVALID, bad
        v = int(field)
        return (OK, v & MASK) if -2 ** 63 <= v < 2 ** 63 else (RANGE, bad)
    m = SPC_RE.fullmatch(field)
    if m:
        return OK, NAN if m.group(1).lower() == b"nan" else bits_of(float(field))
    m = FLT_RE.fullmatch(field)
    if not m:
        return INVALID, bad
    ip, fp = (m.group(1), m.group(2) or b"") if m.group(1) is not None else (b"", m.group(3))
    digits = (ip + fp).lstrip(b"0")
    kept = digits.rstrip(b"0")
    w = int(kept) if kept else 0
    q = int(m.group(4) or 0) - len(fp) + (len(digits) - len(kept))
    neg = field[:1] == b"-"
    if w == 0:
        got = bits_of(-0.0 if neg else 0.0)
    elif w <= 2 ** 53 and -22 <= q <= 22:
        v = float(w) * float(10 ** q) if q >= 0 else float(w) / float(10 ** -q)
        got = bits_of(-v if neg else v)
    else:
        return RANGE, bad
    assert got == bits_of(float(field)), (field, "the rule of exact conversion disagrees with float()")
    return OK, got


def cell(field, kind):
    key = (field, kind)
    if key not in _cells:
        _cells[key] = model(field, kind)
    return _cells[key]


class Want:
    """The cells of every line of a stream for one field delimiter and column list; made once, read by every range set."""

    def __init__(self, ln, delim, fd, cols):
        plain, st = ln.pl.plain, ln.start
        d, f = bytes([delim]), bytes([fd])
        self.cols = cols
        self.st = np.zeros((len(cols), ln.L), dtype=np.uint8)
        self.val = np.zeros((len(cols), ln.L), dtype=np.uint64)
        for k in range(ln.L):
            line = plain[int(st[k]):int(st[k + 1])]
            parts = (line[:-1] if line.endswith(d) else line).split(f)
            for c, (num, kind) in enumerate(cols):
                self.st[c, k], self.val[c, k] = cell(parts[num] if num < len(parts) else None, kind)

    def rows(self, ranges):
        idx = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in ranges] + [np.zeros(0, dtype=np.int64)])
        offs = [0] + np.cumsum([max(b - a, 0) for a, b in ranges]).tolist()
        return self.val[:, idx], self.st[:, idx], offs


# ------------------------------------------------------------------------------------------------ the calls
def read_cols(mem, o, ranges, fd, cols, cap, table=False, values=True, status=True, counts=True):
    """One call into guarded arrays: (n_rows, n_not_ok, row_offsets, values[n_cols, cap] or None, status or None,
    per-column counts or None).  Raises what the call raises, after checking that nothing was written."""
    n_cols, n = len(cols), len(ranges)
    kv, pv = mem.put(bytes([FILL]) * (8 * n_cols * cap + GUARD), shift=24) if values else (None, None)
    ks, ps = mem.put(bytes([FILL]) * (n_cols * cap + GUARD), shift=3) if status else (None, None)
    kc, pc = mem.put(bytes([FILL]) * 8 * (n_cols + 4)) if counts else (None, None)

    def arrays():
        v = np.frombuffer(mem.get(kv, 8 * n_cols * cap + GUARD + 24)[24:], dtype=np.uint8) if values else None
        s = np.frombuffer(mem.get(ks, n_cols * cap + GUARD + 3)[3:], dtype=np.uint8) if status else None
        return v, s

    try:
        if table:
            kr, rp = put_ranges(mem, ranges)
            ko, op = mem.put(bytes([FILL]) * 8 * (n + 1 + 4))
            n_rows, n_bad, _ = o.d.read_columns_table_device(o.ix, o.lt, o.ptr, o.n, rp, n, fd, cols, pv, ps, cap, pc, op)
            offs = np.frombuffer(mem.get(ko, 8 * (n + 1 + 4)), dtype=np.uint64).tolist()
            assert offs[n + 1:] == [UNTOUCHED] * 4, "entries written behind d_row_offsets"
            offs = offs[:n + 1]
        else:
            n_rows, n_bad, offs = o.d.read_columns_device(o.ix, o.lt, o.ptr, o.n, ranges, fd, cols, pv, ps, cap, pc)
            offs = offs.tolist()
    except _native.GzpxError:
        for a in arrays():
            assert a is None or bool(np.all(a == FILL)), "an output array was written by a call that failed"
        raise
    v, s = arrays()
    if values:
        assert bool(np.all(v[8 * n_cols * cap:] == FILL)), "bytes written behind d_values"
        v = v[:8 * n_cols * cap].view(np.uint64).reshape(n_cols, cap)
        assert bool(np.all(v[:, n_rows:] == UNTOUCHED)), "cells written behind the rows"
    if status:
        assert bool(np.all(s[n_cols * cap:] == FILL)), "bytes written behind d_status"
        s = s[:n_cols * cap].reshape(n_cols, cap)
        assert bool(np.all(s[:, n_rows:] == FILL)), "status bytes written behind the rows"
    col_bad = None
    if counts:
        col_bad = np.frombuffer(mem.get(kc, 8 * (n_cols + 4)), dtype=np.uint64).tolist()
        assert col_bad[n_cols:] == [UNTOUCHED] * 4, "entries written behind d_col_not_ok"
        col_bad = col_bad[:n_cols]
    return n_rows, n_bad, offs, v, s, col_bad


def check(mem, o, want, ranges, fd, what, table=False, extra=5):
    val, st, offs = want.rows(ranges)
    R = val.shape[1]
    n_rows, n_bad, got_offs, v, s, col_bad = read_cols(mem, o, ranges, fd, want.cols, R + extra, table=table)
    assert n_rows == R and got_offs == offs, (what, "rows", n_rows, R)
    wrong = np.argwhere(s[:, :R] != st)
    assert wrong.size == 0, (what, "status", wrong[:5].tolist(), s[:, :R][tuple(wrong[0])], st[tuple(wrong[0])])
    wrong = np.argwhere(v[:, :R] != val)
    assert wrong.size == 0, (what, "values", wrong[:5].tolist(), hex(int(v[:, :R][tuple(wrong[0])])), hex(int(val[tuple(wrong[0])])))
    assert col_bad == (st != OK).sum(axis=1).tolist() and n_bad == int((st != OK).sum()), (what, "counts")
    ms = o.d.last_columns_ms()
    assert all(t >= 0.0 for t in ms), (what, ms)
    return v, s


# ------------------------------------------------------------------------------------------------ 1. the grammar
HAND = [
    b"0", b"1", b"-1", b"+1", b"007", b"-007", b"+0", b"-0", b"00", b"9", b"10", b"42", b"123456789", b"-123456789",
    b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"+9223372036854775807",
    b"+9223372036854775808", b"18446744073709551615", b"18446744073709551616", b"99999999999999999999", b"9999999999999999999",
    b"1000000000000000000", b"10000000000000000000", b"0" * 30 + b"9223372036854775807", b"0" * 30 + b"9223372036854775808",
    b"-" + b"0" * 30 + b"9223372036854775808", b"0" * 30, b"0" * 64, b"0" * 65, b"1" * 64, b"1" * 65, b"-" + b"0" * 63, b"+" + b"0" * 64,
    b"9007199254740992", b"9007199254740993", b"9007199254740991", b"-9007199254740992", b"-9007199254740993", b"90071992547409920",
    b"9007199254740992e22", b"9007199254740992e23", b"9007199254740992e-22", b"9007199254740992e-23", b"9007199254740993e0",
    b"1e22", b"1e23", b"1e-22", b"1e-23", b"1E22", b"1E+22", b"1e+23", b"-1e22", b"-1e-23", b"10e21", b"10e22", b"100e21",
    b"0.1e23", b"0.1e24", b"1.0e22", b"1.0e23", b"0.01e-20", b"0.01e-21", b"1" + b"0" * 22, b"1" + b"0" * 23, b"123" + b"0" * 20,
    b"0." + b"0" * 21 + b"1", b"0." + b"0" * 22 + b"1", b"1.", b".5", b".", b"e5", b"1e", b"1e+", b"1e-", b"+-1", b"-+1", b"1 ",
    b" 1", b"0x10", b"1x", b"x", b"+", b"-", b"+.", b"-.", b".e1", b"1.e1", b".1e1", b"1..2", b"1.2.3", b"1e1e1", b"1e1.5", b"1e 5",
    b"-0.0", b"+0.0", b"0.0", b"0e0", b"0e-99999", b"-0e99999", b"0.000e+0000000000000000000000000000000000000000000000000000009",
    b"1e0000000000000000000000000000000000000000000000000000000000005", b"1e99999", b"1e-99999", b"1e400", b"1e-400",
    b"NaN", b"nan", b"NAN", b"+nan", b"-nan", b"-NaN", b"nan1", b"na", b"nanx", b"inf", b"-inf", b"+inf", b"INF", b"Inf",
    b"Infinity", b"-infinity", b"+INFINITY", b"infinit", b"infinityy", b"in", b"infi", b"-in", b"i", b"1inf",
    b"3.14159", b"-2.5", b"2.5e3", b"2.5E-3", b"1.5", b"0.5", b"0.25", b"0.1", b"0.2", b"0.3", b"1e1", b"1.0", b"100", b"100.00",
    b"000100.00100", b"123456789012345", b"1234567890123456", b"12345678901234567", b"0.1234567890123456", b"0.123456789012345",
    b"1.7976931348623157e308", b"5e-324", b"2.2250738585072014e-308", b"4.9406564584124654e-324", b"1234.5678e-4", b"1e5",
    b"12345678901234567890", b"123456789012345678901234567890", b"0.000000000000000000000000000001", b"1" + b"0" * 63,
    b"1." + b"0" * 62, b"1." + b"0" * 63, b"." + b"0" * 62 + b"1", b"." + b"0" * 63 + b"1", b"1\r", b"\r", b"1,5", b"1_000", b"1e5\r",
    b"4503599627370496.5", b"4503599627370497.5", b"0.30000000000000004", b"8.5e-10", b"99.99", b"-99.99e+2", b"+99.99E-2",
]
assert len(HAND) >= 150 and len(set(HAND)) == len(HAND)


def random_fields(n, seed):
    """n strings: most from the float grammar (the integer grammar is inside it), digit counts and exponents drawn so that
    every status occurs; some damaged by one byte."""
    rng = np.random.default_rng(seed)
    out = []

    def digits(k):
        return bytes(rng.integers(48, 58, k, dtype=np.uint8)) if k else b""

    for _ in range(n):
        kind = int(rng.integers(0, 10))
        sign = (b"", b"", b"-", b"+")[int(rng.integers(0, 4))]
        if kind < 3:
            s = sign + digits(int(rng.integers(1, 22)))
        elif kind < 8:
            ni, nf = int(rng.integers(0, 12)), int(rng.integers(0, 12))
            body = digits(ni) + (b"." + digits(nf) if nf or rng.integers(0, 2) else b"") if ni else b"." + digits(max(nf, 1))
            if rng.integers(0, 3) == 0:
                body = body.replace(b"5", b"0").replace(b"7", b"0")
            e = b""
            if rng.integers(0, 2):
                e = (b"e", b"E")[int(rng.integers(0, 2))] + (b"", b"-", b"+")[int(rng.integers(0, 3))] + b"%d" % int(rng.integers(0, 30))
            s = sign + body + e
        elif kind == 8:
            s = sign + (b"nan", b"inf", b"Infinity", b"NaN", b"INF")[int(rng.integers(0, 5))]
        else:
            s = digits(int(rng.integers(0, 6)))
        if rng.integers(0, 12) == 0 and s:
            at = int(rng.integers(0, len(s)))
            s = s[:at] + bytes([b"x e.-+,"[int(rng.integers(0, 7))]]) + s[at + 1:]
        out.append(s)
    return out


def grammar(lib):
    """The hand-written table and 20,000 drawn fields as column 1 of one TSV, read as INT64 and as FLOAT64."""
    mem = Mem(lib)
    fields = HAND + random_fields(20000, 20260301)
    text = b"".join(b"%d\t%s\tz\n" % (i, f) for i, f in enumerate(fields))
    s = cut(BGZF, text, list(range(40000, len(text), 40000)))
    pl = Plain(BGZF, s)
    ln = Lines(pl, NL)
    assert ln.L == len(fields)
    with Opened(lib, mem, BGZF, s) as o:
        for kind in (INT, FLT):
            want = Want(ln, NL, TAB, [(0, INT), (1, kind), (3, kind)])
            seen = set(want.st[1].tolist())
            assert seen == {OK, EMPTY, INVALID, RANGE}, (kind, seen)
            assert set(want.st[2].tolist()) == {MISSING} and not want.st[0].any()
            check(mem, o, want, [(0, ln.L)], TAB, ("grammar", kind))


# ------------------------------------------------------------------------------------------------ 2. the edges of the walk
def edge_text(prefix, fd=TAB, delim=NL, terminated=True, long_line=True):
    """A first line of `prefix` bytes, then lines of exactly 16 bytes "dd<fd>dddd<fd>d.ddddd<delim>": with the prefix
    0..31 every field delimiter and every line delimiter stands once at byte 15 of a word and as the last byte of a
    piece, fields straddle the pieces' edges and start on a piece's first byte.  In the middle: empty lines, a line that
    ends in a field delimiter, fields of 64 and 65 bytes, and a line of 3,000 fields (about 20 KiB: pieces without a line
    delimiter in front of its field 2,500).  Unterminated: the text ends in a field delimiter."""
    f, d = bytes([fd]), bytes([delim])
    out = [b"8" * (prefix - 1) + d] if prefix else []
    for i in range(2300):
        out.append(b"%02d" % (i % 100) + f + b"%04d" % (i * 7 % 10000) + f + b"%d.%05d" % (i % 10, i * 31 % 100000) + d)
        if i == 1100:
            out += [d, d, b"5" + f + d, f + f + b"6" + d, b"1" * 64 + f + b"2" * 65 + f + b"0." + b"3" * 62 + d,
                    b"2" * 65 + f + b"1" * 64 + f + b"0." + b"3" * 63 + d]
            if long_line:
                out.append(f.join(b"%d" % (k * 3) for k in range(3000)) + d)
    out.append(b"77" + f + b"88" + f if not terminated else b"77" + f + b"88" + f + b"9.5" + d)
    return b"".join(out)


EDGE_COLS = [(0, INT), (1, FLT), (2, FLT), (2500, INT)]


def edges(lib):
    mem = Mem(lib)
    long_seen = set()
    for prefix in range(32):
        fmt, route = FORMATS[prefix % 2], ROUTES[(prefix // 2) % 2]
        long_line = prefix % 5 == 0  # (0, 5, 10, 15, ...: every pair of format and route gets the line of 3,000 fields)
        text = edge_text(prefix, terminated=prefix % 3 != 1, long_line=long_line)
        assert len(text) > 2 * PIECE
        s = cut(fmt, text, [] if fmt == MGZIP else [20000, 40000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        with Opened(lib, mem, fmt, s, NL, route, shift=prefix % 16) as o:
            want = Want(ln, NL, TAB, EDGE_COLS)
            if long_line:
                assert OK in want.st[3].tolist()
                long_seen.add((fmt, route))
            first = 1 if prefix else 0
            sets = [[(0, ln.L)], [(first, ln.L)]] + ([[(k, ln.L) for k in range(1, 18)], [(ln.L - 1, ln.L)]] if prefix < 2 else [])
            for rs in sets:
                check(mem, o, want, rs, TAB, ("edges", prefix, fmt, route, rs[:2]))
    assert long_seen == {(fmt, route) for fmt in FORMATS for route in ROUTES}
    k = 0
    for fd, delim in ((0x00, 0xFF), (0xFF, 0x00)):  # both delimiters as bytes that text does not hold
        for terminated in (True, False):
            fmt, route = FORMATS[k % 2], ROUTES[k // 2]
            k += 1
            text = edge_text(13, fd, delim, terminated)
            s = cut(fmt, text, [30000])
            ln = Lines(Plain(fmt, s), delim)
            with Opened(lib, mem, fmt, s, delim, route) as o:
                want = Want(ln, delim, fd, EDGE_COLS)
                assert OK in want.st[3].tolist()
                check(mem, o, want, [(0, ln.L), (3, 9)], fd, ("edges", fd, delim, terminated, fmt, route))


# ------------------------------------------------------------------------------------------------ 3. range sets
def number_text(n, seed):
    """About n bytes of lines of 1..8 tab-separated fields: integers, %.6g floats, empty fields and words."""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        parts = []
        for _ in range(int(rng.integers(1, 9))):
            k = int(rng.integers(0, 8))
            parts.append(b"" if k == 0 else b"qu" if k == 1 else b"%d" % int(rng.integers(-10 ** 9, 10 ** 9)) if k < 5
                         else b"%.6g" % float(rng.normal() * 10.0 ** int(rng.integers(-5, 6))))
        line = b"\t".join(parts) + b"\n"
        out.append(line)
        size += len(line)
    return b"".join(out)


RANGE_COLS = [(0, INT), (1, FLT), (4, INT), (6, FLT)]


def ranges(lib):
    """64 KiB of short lines, about 200 ranges (overlapping, repeated, empty, descending, [L, L)): rows and row_offsets;
    the host form and the table form give identical arrays; twice, the same arrays; both routes; the members read."""
    mem = Mem(lib)
    text = number_text(65536, 3)
    for i, fmt in enumerate(FORMATS):
        s = cut(fmt, text, [9000, 30000, 30000, 50001], eof=fmt == BGZF)
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        rs = range_set(ln, 40 + i)
        want = Want(ln, NL, TAB, RANGE_COLS)
        for route in ROUTES:
            with Opened(lib, mem, fmt, s, NL, route, shift=7 * i) as o:
                v0, s0 = check(mem, o, want, rs, TAB, ("ranges", fmt, route))
                assert o.d.last_lines_members() == len(pl.union([ln.cover(a, b) for a, b in rs]))
                v1, s1 = check(mem, o, want, rs, TAB, ("ranges", fmt, route, "table form"), table=True)
                assert o.d.last_lines_members() == len(pl.union([ln.cover(a, b) for a, b in rs]))
                v2, s2 = check(mem, o, want, rs, TAB, ("ranges", fmt, route, "again"))
                assert np.array_equal(v0, v1) and np.array_equal(s0, s1) and np.array_equal(v0, v2) and np.array_equal(s0, s2)
                for table in (False, True):
                    assert read_cols(mem, o, [], TAB, RANGE_COLS, 4, table=table)[:3] == (0, 0, [0])
                    assert o.d.last_lines_members() == 0
                    got = read_cols(mem, o, [(5, 5), (ln.L, ln.L)], TAB, RANGE_COLS, 4, table=table)
                    assert got[:3] == (0, 0, [0, 0, 0]) and got[5] == [0] * 4


# ------------------------------------------------------------------------------------------------ 4. capacity
def capacity(lib):
    mem = Mem(lib)
    text = number_text(40000, 5)
    for fmt in FORMATS:
        s = cut(fmt, text, [17000])
        ln = Lines(Plain(fmt, s), NL)
        rs = [(0, ln.L), (ln.L // 2, ln.L), (3, 3)]
        want = Want(ln, NL, TAB, RANGE_COLS)
        val, st, offs = want.rows(rs)
        R = val.shape[1]
        n_bad, col_bad = int((st != OK).sum()), (st != OK).sum(axis=1).tolist()
        with Opened(lib, mem, fmt, s) as o:
            for table in (False, True):
                for cap in (R - 1, 0):
                    with pytest.raises(_native.GzpxError) as e:  # (read_cols checks that both arrays are untouched)
                        read_cols(mem, o, rs, TAB, RANGE_COLS, cap, table=table)
                    assert (e.value.code, e.value.needed) == (_native.ERR_INSUFFICIENT_SPACE, R), (fmt, table, cap)
                check(mem, o, want, rs, TAB, (fmt, table, "R + 5"), table=table, extra=5)
                check(mem, o, want, rs, TAB, (fmt, table, "R"), table=table, extra=0)
                got = read_cols(mem, o, rs, TAB, RANGE_COLS, R, table=table, status=False)
                assert got[:3] == (R, n_bad, offs) and np.array_equal(got[3], val) and got[5] == col_bad
                got = read_cols(mem, o, rs, TAB, RANGE_COLS, R, table=table, values=False)
                assert got[:3] == (R, n_bad, offs) and np.array_equal(got[4], st) and got[5] == col_bad
                got = read_cols(mem, o, rs, TAB, RANGE_COLS, 0, table=table, values=False, status=False)
                assert got[:3] == (R, n_bad, offs) and got[5] == col_bad
                got = read_cols(mem, o, rs, TAB, RANGE_COLS, 0, table=table, values=False, status=False, counts=False)
                assert got[:3] == (R, n_bad, offs)


# ------------------------------------------------------------------------------------------------ 5. errors
def raw_columns(lib, o, ranges, fd, cols, n_cols, d_values=None, d_status=None, cap=0):
    r = np.ascontiguousarray(np.array(ranges, dtype=np.uint64).reshape(-1, 2))
    cl = np.zeros(max(len(cols), 1), dtype=_native.COLUMN_DTYPE)
    for i, c in enumerate(cols):
        cl[i] = c
    n_rows, n_bad, bad, info = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_size_t(77), _native.GzpxCheckInfo()
    rc = lib.L.gzpx_read_columns_device(o.d.h, o.ix.h, o.lt.h, o.ptr, o.n, r.ctypes.data, r.shape[0], fd, cl.ctypes.data, n_cols, d_values,
                                        d_status, cap, ctypes.byref(n_rows), ctypes.byref(n_bad), None, None, ctypes.byref(bad),
                                        ctypes.byref(info), None)
    return rc, n_rows.value, n_bad.value


def errors(lib):
    mem = Mem(lib)
    text = number_text(20000, 6)
    INV = _native.ERR_INVALID_ARG
    for fmt in FORMATS:
        s = cut(fmt, text, [7000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        L = ln.L
        with Opened(lib, mem, fmt, s) as o:
            kv, pv = mem.put(bytes([FILL]) * 8 * 4096)
            ks, ps = mem.put(bytes([FILL]) * 4096)
            whole = [(0, L)]
            many = [(2 * k, k % 2, 0) for k in range(17)]
            assert raw_columns(lib, o, whole, TAB, many[:16], 16)[:2] == (_native.OK, L) and o.d.last_lines_members() == pl.n
            for what, call in (("0 columns", lambda: raw_columns(lib, o, whole, TAB, [(0, 0, 0)], 0, pv, ps, 16)),
                              ("17 columns", lambda: raw_columns(lib, o, whole, TAB, many, 17, pv, ps, 16)),
                              ("equal field numbers", lambda: raw_columns(lib, o, whole, TAB, [(2, 0, 0), (2, 1, 0)], 2, pv, ps, 16)),
                              ("descending field numbers", lambda: raw_columns(lib, o, whole, TAB, [(3, 0, 0), (1, 0, 0)], 2, pv, ps, 16)),
                              ("an unknown type", lambda: raw_columns(lib, o, whole, TAB, [(0, 2, 0)], 1, pv, ps, 16)),
                              ("reserved != 0", lambda: raw_columns(lib, o, whole, TAB, [(0, 0, 1)], 1, pv, ps, 16)),
                              ("field_delim == the table's delimiter", lambda: raw_columns(lib, o, whole, NL, [(0, 0, 0)], 1, pv, ps, 16)),
                              ("field_delim > 255", lambda: raw_columns(lib, o, whole, 256, [(0, 0, 0)], 1, pv, ps, 16)),
                              ("d_values not 8-byte aligned", lambda: raw_columns(lib, o, whole, TAB, [(0, 0, 0)], 1, pv + -pv % 8 + 4, ps, 16)),
                              ("d_values one byte off", lambda: raw_columns(lib, o, whole, TAB, [(0, 1, 0)], 1, pv + -pv % 8 + 1, None, 16)),
                              ("a bad list and no ranges", lambda: raw_columns(lib, o, [], TAB, [(0, 7, 0)], 1, pv, ps, 16))):
                got = call()
                assert got == (INV, 0, 0), (fmt, what, got)
                assert o.d.last_lines_members() == 0, (fmt, what)
                assert mem.get(kv, 8 * 4096) == bytes([FILL]) * 8 * 4096 and mem.get(ks, 4096) == bytes([FILL]) * 4096, (fmt, what)
                raw_columns(lib, o, [(0, 1)], TAB, [(0, 0, 0)], 1)  # (something is inflated in between)
            good = [(0, 2), (L - 2, L), (5, 5)]
            for what, r, at in (("b = L + 1", [(L - 1, L + 1)], 3), ("a > b", [(11, 10)], 3), ("first", None, 0)):
                rs = good + r + good if r else [(L + 5, L + 6)] + good
                for table in (False, True):
                    with pytest.raises(_native.GzpxError) as e:
                        read_cols(mem, o, rs, TAB, [(0, INT)], 64, table=table)
                    assert (e.value.code, e.value.range_index) == (INV, at), (fmt, what, table)
                    assert o.d.last_lines_members() == 0
            # the table with the index of another stream, and with another context
            other = cut(fmt, number_text(12000, 7), [5000])
            keep2, ptr2 = mem.put(other)
            raw_columns(lib, o, [(0, 1)], TAB, [(0, 0, 0)], 1)
            with o.d.build_index_device(ptr2, len(other)) as ix2:
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_columns_device(ix2, o.lt, ptr2, len(other), [(0, 1)], TAB, [(0, INT)], pv, ps, 16)
                assert e.value.code == INV and e.value.range_index is None and o.d.last_lines_members() == 0
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.read_columns_device(o.ix, o.lt, o.ptr, o.n, [(0, 1)], TAB, [(0, INT)], pv, ps, 16)
                assert e.value.code == INV
            assert o.d.last_columns_ms() == (0.0, 0.0)
            assert mem.get(kv, 8 * 4096) == bytes([FILL]) * 8 * 4096 and mem.get(ks, 4096) == bytes([FILL]) * 4096


# ------------------------------------------------------------------------------------------------ 6. a damaged member
def damaged(lib):
    """A damaged member that the ranges touch: the inflate's error class and the member's index in the stream; the context
    serves on.  One that they do not touch is never seen."""
    mem = Mem(lib)
    for fmt in FORMATS:
        text = number_text(8 * 5000, 11)[:8 * 5000 - 1] + b"\n"
        s = cut(fmt, text, [5000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        want = Want(ln, NL, TAB, RANGE_COLS)
        mid = int(np.searchsorted(ln.start, 3 * 5000 + 2500))
        for route in ROUTES:
            with Opened(lib, mem, fmt, s, route=route) as o:  # (the table of the undamaged stream)
                for victim in (0, 3, 7):
                    for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                           ("block type", pl.off[victim] + HDR[fmt], _native.ERR_BAD_DATA)):
                        m = bytearray(s)
                        if what == "crc":
                            m[at] ^= 0xFF
                        else:
                            m[at] |= 0x06  # BTYPE = 3, reserved
                        keep, ptr = mem.put(m)
                        with o.d.build_index_device(ptr, len(m)) as ix:  # (the members' extents are the same: the table serves)
                            bad = type("O", (), dict(d=o.d, ix=ix, lt=o.lt, ptr=ptr, n=len(m)))
                            with pytest.raises(_native.GzpxError) as e:
                                read_cols(mem, bad, [(0, ln.L)], TAB, RANGE_COLS, ln.L)
                            assert (e.value.code, e.value.block, e.value.needed) == (code, victim, None), (fmt, route, victim, what)
                            if victim != 3 and what == "crc":  # a range that does not touch the member
                                check(mem, bad, want, [(mid, mid + 3)], TAB, (fmt, route, victim, what))
                check(mem, o, want, [(0, ln.L)], TAB, (fmt, route, "after the damage"))


# ------------------------------------------------------------------------------------------------ 7. closing the loop
def close_the_loop(lib):
    """select_lines_device (group = 1), then read_columns_table_device on the run table where it lies."""
    mem = Mem(lib)
    text = number_text(30000, 8)
    pattern = b"qu"
    for fmt in FORMATS:
        s = cut(fmt, text, [40, 11000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        all_lines = pl.plain.splitlines(keepends=True)
        assert len(all_lines) == ln.L
        want = Want(ln, NL, TAB, RANGE_COLS)
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for invert in (False, True):
                keepers = [k for k, x in enumerate(all_lines) if (pattern in x) != invert]
                cap_runs = -(-ln.L // 2)
                kr, rp = mem.put(bytes([FILL]) * 16 * cap_runs)
                n_runs, n_records, _ = o.d.select_lines_device(o.ix, o.lt, o.ptr, o.n, pattern, 1, invert, rp, cap_runs)
                assert n_runs >= 2 and n_records == len(keepers)
                R = len(keepers)
                kv, pv = mem.put(bytes([FILL]) * (8 * 4 * R + GUARD), shift=8)
                ks, ps = mem.put(bytes([FILL]) * (4 * R + GUARD), shift=3)
                n_rows, n_bad, _ = o.d.read_columns_table_device(o.ix, o.lt, o.ptr, o.n, rp, n_runs, TAB, RANGE_COLS, pv, ps, R)
                assert n_rows == R and n_bad == int((want.st[:, keepers] != OK).sum()), (fmt, invert)
                v = np.frombuffer(mem.get(kv, 8 * 4 * R + GUARD + 8)[8:], dtype=np.uint8)
                st = np.frombuffer(mem.get(ks, 4 * R + GUARD + 3)[3:], dtype=np.uint8)
                assert np.array_equal(v[:8 * 4 * R].view(np.uint64).reshape(4, R), want.val[:, keepers]), (fmt, invert)
                assert np.array_equal(st[:4 * R].reshape(4, R), want.st[:, keepers]), (fmt, invert)
                assert bool(np.all(v[8 * 4 * R:] == FILL)) and bool(np.all(st[4 * R:] == FILL)), (fmt, invert)
