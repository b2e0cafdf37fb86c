"""Fields of lines (gzpx_read_fields_device, gzpx_read_fields_table_device), written once and run twice: through the
emulated library on CPU (tests/test_emu_fields.py) and through the real HIP library on the MI355X
(tests/test_gpu_fields.py).

The yardstick is never the library's own inflate or walk.  It is range_cases.Plain (zlib's inflate of every member,
joined), the lines that line_cases.Lines cuts, and for every line the expression of include/gzpx.h:
fd.join(f for k, f in enumerate(body.split(fd)) if k in S) + (delim if the line has one).  Every comparison is exact;
d_out is pre-filled with 0xEE and 64 guard bytes behind the expected length must still be 0xEE afterwards."""
import ctypes

import numpy as np
import pytest

from gzp_amd import _native
from line_cases import Lines, Opened, cut
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem

NL, TAB = 0x0A, 0x09
FILL = 0xEE
GUARD = 64      # bytes behind the output that must stay as they were
GUARD_OFF = 4   # entries behind d_out_offsets likewise
UNTOUCHED = int.from_bytes(bytes([FILL]) * 8, "little")
END = _native.FIELDS_TO_END
PIECE = 16384   # kFlPiece: the passes cut staging on this grid
FORMATS = (BGZF, MGZIP)


# ------------------------------------------------------------------------------------------------ the yardstick
def in_set(fields, complement):
    return lambda k: any(b <= k < e for b, e in fields) != complement


def cut_line(line, delim, fd, sel):
    d, f = bytes([delim]), bytes([fd])
    has = line.endswith(d)
    body = line[:-1] if has else line
    return f.join(x for k, x in enumerate(body.split(f)) if sel(k)) + (d if has else b"")


class Want:
    """What every line of a stream becomes for one field delimiter and field list; made once, read by every range set."""

    def __init__(self, ln, delim, fd, fields, complement):
        sel = in_set(fields, complement)
        plain, st = ln.pl.plain, ln.start
        self.lines = [cut_line(plain[int(st[k]):int(st[k + 1])], delim, fd, sel) for k in range(ln.L)]
        self.cum = np.concatenate([[0], np.cumsum([len(x) for x in self.lines])]).astype(np.int64)

    def data(self, ranges):
        return b"".join(b"".join(self.lines[a:b]) for a, b in ranges)

    def offsets(self, ranges):
        return [0] + np.cumsum([int(self.cum[b] - self.cum[a]) if a < b else 0 for a, b in ranges]).tolist()


# ------------------------------------------------------------------------------------------------ the calls
def read_fields(mem, o, ranges, fd, fields, complement, cap, shift=3):
    """One gzpx_read_fields_device into an output misaligned by `shift`, 0xEE in it and in GUARD bytes behind `cap`:
    (bytes returned, out_offsets)."""
    room = cap + GUARD
    keep, p = mem.put(bytes([FILL]) * room, shift=shift)
    out_len, offs = o.d.read_fields_device(o.ix, o.lt, o.ptr, o.n, np.array(ranges, dtype=np.uint64).reshape(-1, 2), fd, fields, p, cap,
                                           complement)
    whole = mem.get(keep, room + shift)[shift:]
    assert whole[out_len:] == bytes([FILL]) * (room - out_len), "bytes written behind the output"
    return whole[:out_len], offs.tolist()


def check(mem, o, ln, want, ranges, fd, fields, complement, what, query=True, shift=3):
    data, offs = want.data(ranges), want.offsets(ranges)
    if query:  # d_out = None: the length and the offsets
        assert o.d.read_fields_device(o.ix, o.lt, o.ptr, o.n, ranges, fd, fields, None, 0, complement)[0] == len(data), (what, "query")
    got, got_offs = read_fields(mem, o, ranges, fd, fields, complement, len(data), shift)
    assert got_offs == offs, (what, "out_offsets")
    assert got == data, (what, "bytes")
    assert o.d.last_lines_members() == len(ln.pl.union([ln.cover(a, b) for a, b in ranges])), (what, "members read")
    ms = o.d.last_fields_ms()
    assert all(t >= 0.0 for t in ms), (what, ms)
    assert o.d.last_lines_ms()[3] == 0.0, (what, "no gather runs")


def put_ranges(mem, ranges):
    a = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
    return mem.put(a.tobytes() if a.size else b"\0" * 16)


def read_table(mem, o, ranges, fd, fields, complement, cap, offsets=True, shift=5):
    """One gzpx_read_fields_table_device: the line ranges and d_out_offsets are device arrays.
    (bytes returned, d_out_offsets with its guard entries or None)."""
    n = len(ranges)
    room = cap + GUARD
    keep, p = mem.put(bytes([FILL]) * room, shift=shift)
    kr, rp = put_ranges(mem, ranges)
    ko, op = mem.put(bytes([FILL]) * 8 * (n + 1 + GUARD_OFF)) if offsets else (None, None)
    out_len = o.d.read_fields_table_device(o.ix, o.lt, o.ptr, o.n, rp, n, fd, fields, p, cap, complement, op)
    whole = mem.get(keep, room + shift)[shift:]
    assert whole[out_len:] == bytes([FILL]) * (room - out_len), "bytes written behind the output"
    if n:
        assert mem.get(kr, 16 * n) == np.array(ranges, dtype=np.uint64).tobytes(), "the range table was written"
    offs = np.frombuffer(mem.get(ko, 8 * (n + 1 + GUARD_OFF)), dtype=np.uint64).tolist() if offsets else None
    return whole[:out_len], offs


# ------------------------------------------------------------------------------------------------ 1. the rule
RULE_LISTS = ([(0, 1)], [(1, 2)], [(2, 3), (5, 6)], [(3, END)], [(0, END)])
RULE_PAIRS = ((TAB, NL, False), (ord(","), NL, False), (0x00, 0xFF, True), (0xFF, 0x00, True))  # (field delimiter, delimiter, binary)


def rule_text(fd, delim, terminated, binary):
    """About 3 KiB: lines of 1, 2, 3, 6 and 40 fields, empty lines, lines of delimiters only, empty fields at the start, in
    the middle and at the end; the last line of several fields.  Binary: every byte value but the two delimiters occurs in
    the fields, and the two delimiters occur as themselves."""
    alphabet = [b for b in (range(256) if binary else range(ord("a"), ord("z") + 1)) if b not in (fd, delim)]
    state = [0]

    def field(n):
        out = bytes(alphabet[(state[0] + i) % len(alphabet)] for i in range(n))
        state[0] += n
        return out

    f, d = bytes([fd]), bytes([delim])
    lines = []
    for rep in range(8):
        for F in (1, 2, 3, 6, 40):
            lines.append(f.join(field(1 + (3 * k + rep) % 9) for k in range(F)))
        lines += [b"", b"", f, f * 2, f * 5, f * 7]
        lines += [f + field(4) + f + field(2), field(3) + f + f + field(5), field(2) + f + field(2) + f, f + f + field(1) + f + f + f + field(6)]
    lines.append(f.join(field(5) for _ in range(7)))
    text = d.join(lines) + (d if terminated else b"")
    assert 2500 <= len(text) <= 4200
    return text


def rule(lib):
    """Every field list of RULE_LISTS, plain and complemented, for every delimiter pair, terminated and not, both formats and
    both routes; [0, END) against read_lines_device's bytes too, its complement gives the line delimiters only."""
    mem = Mem(lib)
    for fd, delim, binary in RULE_PAIRS:
        for terminated in (True, False):
            text = rule_text(fd, delim, terminated, binary)
            if binary:
                assert set(text) == set(range(256))
            for fmt in FORMATS:
                s = cut(fmt, text, [1000, 1000, 2100], eof=fmt == BGZF and terminated)
                pl = Plain(fmt, s)
                ln = Lines(pl, delim)
                assert (ln.D == ln.L) == terminated
                F = [pl.plain[int(ln.start[k]):int(ln.start[k + 1])].count(bytes([fd])) + 1 for k in range(ln.L)]
                assert {1, 2, 3, 6, 40} <= set(F)
                wants = {(i, c): Want(ln, delim, fd, fields, c) for i, fields in enumerate(RULE_LISTS) for c in (False, True)}
                # the s0 rule of [2, 3) + [5, 6): F <= 2 a bare delimiter, F in 3..5 one field and no separator
                w = wants[(2, False)]
                for k in range(ln.L):
                    if F[k] <= 2:
                        assert w.lines[k] in (b"", bytes([delim]))
                    elif F[k] <= 5:
                        assert bytes([fd]) not in w.lines[k]
                assert wants[(4, False)].data([(0, ln.L)]) == pl.plain
                assert wants[(4, True)].data([(0, ln.L)]) == bytes([delim]) * ln.D
                for route in ROUTES:
                    with Opened(lib, mem, fmt, s, delim, route, shift=fd % 16) as o:
                        for (i, c), want in wants.items():
                            what = (fd, delim, terminated, fmt, route, RULE_LISTS[i], c)
                            check(mem, o, ln, want, [(0, ln.L)], fd, RULE_LISTS[i], c, what, query=route == ROUTES[0])
                        some = [(3, 9), (0, 1), (ln.L - 1, ln.L), (7, 7), (5, ln.L)]
                        check(mem, o, ln, wants[(2, False)], some, fd, RULE_LISTS[2], False, (fd, delim, fmt, route, "some ranges"))
                        # everything: what the read by line returns
                        keep, p = mem.put(bytes(len(text) + 16))
                        n, _, _ = o.d.read_lines_device(o.ix, o.lt, o.ptr, o.n, [(0, ln.L)], p, len(text))
                        got, _ = read_fields(mem, o, [(0, ln.L)], fd, [(0, END)], False, len(text))
                        assert got == mem.get(keep, n) == text


# ------------------------------------------------------------------------------------------------ 2. the edges of the walk
def edge_text(prefix):
    """`prefix` bytes (a line of their own), a short line, a line of 40 KiB with a field delimiter every 7 bytes -- one
    field is 5 bytes longer, so that with no prefix one delimiter is the last byte of a piece and a later one the first
    byte of a piece -- and a short line.  Returns (text, the field in front of which the first of the two delimiters
    stands, the field in front of which the second does)."""
    head = (b"p" * (prefix - 1) + b"\n" if prefix else b"") + b"ab\tcd\n"
    s0 = 6  # where the long line starts when there is no prefix
    parts, pos, k, k_last, k_first = [], s0, 0, None, None
    while pos - s0 < 40 * 1024:
        width = 6
        if k_last is not None and k_first is None and (2 * PIECE - (pos + width)) % 7 == 5 and pos > PIECE + 1000:
            width = 11
        if k == 0:
            width = 6 + (PIECE - 1 - (s0 + 6)) % 7  # the first field's width puts a delimiter at PIECE - 1
        parts.append(bytes(ord("a") + (k + i) % 26 for i in range(width)))
        pos += width
        if pos == PIECE - 1:
            k_last = k + 1
        if pos == 2 * PIECE:
            k_first = k + 1
        pos += 1
        k += 1
    long_line = b"\t".join(parts) + b"\n"
    text = head + long_line + b"x\ty\tz\n"
    assert k_last and k_first and 40 * 1024 <= len(long_line) <= 41 * 1024
    if not prefix:
        assert text[PIECE - 1] == TAB and text[2 * PIECE] == TAB and text[PIECE] != TAB and text[2 * PIECE - 1] != TAB
    return text, k_last, k_first


def edges(lib):
    """The long line of edge_text as one range (three pieces, two of them without a line delimiter) and inside the whole
    text; single fields around the two delimiters that lie on piece edges, which thereby straddle the edge or touch it;
    then the same behind prefixes of 1..16 bytes, so that the range's first byte has every alignment in staging."""
    mem = Mem(lib)
    for prefix in range(17):
        text, k_last, k_first = edge_text(prefix)
        ks = [k_last - 1, k_last, k_last + 1, k_first - 1, k_first, k_first + 1]
        combos = [(fmt, route) for fmt in FORMATS for route in ROUTES] if prefix == 0 else [(FORMATS[prefix % 2], ROUTES[(prefix // 2) % 2])]
        for fmt, route in combos:
            s = cut(fmt, text, [] if fmt == MGZIP else [20000, 40000])
            pl = Plain(fmt, s)
            ln = Lines(pl, NL)
            first = 1 if prefix else 0  # the short line in front of the long one
            assert ln.L == first + 3 and int(ln.start[first + 1]) == prefix + 6
            # (the long line alone: its first piece starts where the line does; with no prefix, the whole text too)
            sets = [[(first + 1, first + 2)]] + ([[(0, ln.L)]] if prefix == 0 else [])
            with Opened(lib, mem, fmt, s, NL, route) as o:
                lists = [[(k, k + 1)] for k in (ks if prefix == 0 else (k_last, k_first - 1))] + [[(0, 1), (k_last, k_last + 1), (k_first, END)]]
                for fields in lists:
                    for comp in ((False, True) if fields is lists[0] or fields is lists[-1] else (False,)):
                        want = Want(ln, NL, TAB, fields, comp)
                        for rs in sets:
                            check(mem, o, ln, want, rs, TAB, fields, comp, (prefix, fmt, route, fields, comp, rs), query=False,
                                  shift=prefix % 16)


# ------------------------------------------------------------------------------------------------ 3. range sets
def table_text(n, seed):
    """About n bytes of lines of 1..12 tab-separated fields of 0..9 letters."""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n:
        line = b"\t".join(bytes(rng.integers(97, 123, int(rng.integers(0, 10)), dtype=np.uint8)) for _ in range(int(rng.integers(1, 13)))) + b"\n"
        out.append(line)
        size += len(line)
    return b"".join(out)


def range_set(ln, seed):
    """About 200 line ranges: the whole, empty ones ([L, L) among them), repeated and overlapping ones, single lines, and
    log-uniform lengths at random places -- most of them start in the middle of a piece -- in a shuffled order."""
    L = ln.L
    rng = np.random.default_rng(seed)
    a, b = L // 3, L // 3 + 40
    r = [(0, L), (0, 0), (L // 2, L // 2), (L, L), (a, b), (a, b), (a, b), (a - 5, a + 5), (a + 20, b + 9), (L - 1, L), (0, 1)]
    r += [(k, k + 1) for k in rng.integers(0, L, 60).tolist()]
    for _ in range(130):
        n = min(int(np.exp(rng.uniform(0, np.log(L + 1)))), L)
        at = int(rng.integers(0, L - n + 1))
        r.append((at, at + n))
    return [r[j] for j in rng.permutation(len(r))]


def ranges(lib):
    """64 KiB of short lines, about 200 ranges: out_offsets and the bytes through the host form; through the table form the
    line ranges and d_out_offsets are device arrays (with and without the offsets)."""
    mem = Mem(lib)
    text = table_text(65536, 3)
    for i, fmt in enumerate(FORMATS):
        s = cut(fmt, text, [9000, 30000, 30000, 50001], eof=fmt == BGZF)
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        rs = range_set(ln, 40 + i)
        assert 190 <= len(rs) <= 210
        for j, route in enumerate(ROUTES):
            with Opened(lib, mem, fmt, s, NL, route, shift=7 * i) as o:
                for fields, comp in ((([(1, 3), (6, 7)], False), ([(0, 2)], True))[(i + j) % 2],):
                    want = Want(ln, NL, TAB, fields, comp)
                    what = (fmt, route, fields, comp)
                    check(mem, o, ln, want, rs, TAB, fields, comp, what)
                    data, offs = want.data(rs), want.offsets(rs)
                    got, got_offs = read_table(mem, o, rs, TAB, fields, comp, len(data))
                    assert got == data and got_offs == offs + [UNTOUCHED] * GUARD_OFF, (what, "table form")
                    assert o.d.last_lines_members() == len(pl.union([ln.cover(a, b) for a, b in rs]))
                    assert read_table(mem, o, rs[:9], TAB, fields, comp, len(want.data(rs[:9])), offsets=False)[0] == want.data(rs[:9])
                assert read_table(mem, o, [], TAB, [(0, 1)], False, 0) == (b"", [0] + [UNTOUCHED] * GUARD_OFF)
                assert read_fields(mem, o, [], TAB, [(0, 1)], False, 0) == (b"", [0]) and o.d.last_lines_members() == 0
                assert read_fields(mem, o, [(5, 5), (ln.L, ln.L)], TAB, [(0, 1)], False, 0) == (b"", [0, 0, 0])


# ------------------------------------------------------------------------------------------------ 4. closing the loop
def close_the_loop(lib):
    """select_lines_device (group = 1), then read_fields_table_device on the run table where it lies: grep | cut."""
    mem = Mem(lib)
    text = table_text(30000, 8)
    pattern = b"qu"
    for fmt in FORMATS:
        s = cut(fmt, text, [40, 11000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        all_lines = pl.plain.splitlines(keepends=True)
        assert len(all_lines) == ln.L
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for invert in (False, True):
                for fields, comp in (([(0, 2), (4, 5)], False), ([(1, 2)], True)):
                    sel = in_set(fields, comp)
                    want = b"".join(cut_line(x, NL, TAB, sel) for x in all_lines if (pattern in x) != invert)
                    cap_runs = -(-ln.L // 2)
                    kr, rp = mem.put(bytes([FILL]) * 16 * cap_runs)
                    n_runs, n_records, _ = o.d.select_lines_device(o.ix, o.lt, o.ptr, o.n, pattern, 1, invert, rp, cap_runs)
                    assert n_runs >= 2 and n_records == sum(1 for x in all_lines if (pattern in x) != invert)
                    keep, p = mem.put(bytes([FILL]) * (len(want) + GUARD), shift=5)
                    out_len = o.d.read_fields_table_device(o.ix, o.lt, o.ptr, o.n, rp, n_runs, TAB, fields, p, len(want), comp)
                    assert out_len == len(want), (fmt, invert, fields, comp)
                    assert mem.get(keep, len(want) + GUARD + 5)[5:] == want + bytes([FILL]) * GUARD, (fmt, invert, fields, comp)


# ------------------------------------------------------------------------------------------------ 5. size query and capacity
def capacity(lib):
    mem = Mem(lib)
    text = table_text(40000, 5)
    for fmt in FORMATS:
        s = cut(fmt, text, [17000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        rs = [(0, ln.L), (ln.L // 2, ln.L), (3, 3)]
        fields = [(1, 4)]
        want = Want(ln, NL, TAB, fields, False)
        data, offs = want.data(rs), want.offsets(rs)
        need = len(data)
        with Opened(lib, mem, fmt, s) as o:
            # d_out = None: the length and the offsets, in both forms; the writing pass does not run
            out_len, got_offs = o.d.read_fields_device(o.ix, o.lt, o.ptr, o.n, rs, TAB, fields, None, 0)
            assert (out_len, got_offs.tolist()) == (need, offs) and o.d.last_fields_ms()[2] == 0.0
            kr, rp = put_ranges(mem, rs)
            ko, op = mem.put(bytes([FILL]) * 8 * (len(rs) + 1 + GUARD_OFF))
            assert o.d.read_fields_table_device(o.ix, o.lt, o.ptr, o.n, rp, len(rs), TAB, fields, None, 0, False, op) == need
            assert np.frombuffer(mem.get(ko, 8 * (len(rs) + 1 + GUARD_OFF)), dtype=np.uint64).tolist() == offs + [UNTOUCHED] * GUARD_OFF
            # one byte short: the size needed, d_out untouched
            for cap in (need - 1, 0):
                keep, p = mem.put(bytes([FILL]) * (need + GUARD), shift=1)
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_fields_device(o.ix, o.lt, o.ptr, o.n, rs, TAB, fields, p, cap)
                assert (e.value.code, e.value.needed) == (_native.ERR_INSUFFICIENT_SPACE, need), (fmt, cap)
                assert mem.get(keep, need + GUARD + 1)[1:] == bytes([FILL]) * (need + GUARD), (fmt, cap, "output written")
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_fields_table_device(o.ix, o.lt, o.ptr, o.n, rp, len(rs), TAB, fields, p, cap)
                assert (e.value.code, e.value.needed) == (_native.ERR_INSUFFICIENT_SPACE, need), (fmt, cap)
                assert mem.get(keep, need + GUARD + 1)[1:] == bytes([FILL]) * (need + GUARD), (fmt, cap, "output written")
            assert read_fields(mem, o, rs, TAB, fields, False, need) == (data, offs)
            assert read_fields(mem, o, rs, TAB, fields, False, need + 7)[0] == data


# ------------------------------------------------------------------------------------------------ 6. errors
def raw_fields(lib, o, ranges, fd, fields, n_fields, flags, d_out=None, cap=0):
    r = np.ascontiguousarray(np.array(ranges, dtype=np.uint64).reshape(-1, 2))
    f = np.ascontiguousarray(np.array(fields, dtype=np.uint64).reshape(-1, 2))
    out_len, bad, info = ctypes.c_size_t(77), ctypes.c_size_t(77), _native.GzpxCheckInfo()
    rc = lib.L.gzpx_read_fields_device(o.d.h, o.ix.h, o.lt.h, o.ptr, o.n, r.ctypes.data, r.shape[0], fd, f.ctypes.data, n_fields, flags,
                                       d_out, cap, ctypes.byref(out_len), None, ctypes.byref(bad), ctypes.byref(info), None)
    return rc, out_len.value


def errors(lib):
    mem = Mem(lib)
    text = table_text(20000, 6)
    INV = _native.ERR_INVALID_ARG
    for fmt in FORMATS:
        s = cut(fmt, text, [7000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        L = ln.L
        with Opened(lib, mem, fmt, s) as o:
            keep, p = mem.put(bytes([FILL]) * 4096)
            whole = [(0, L)]
            many = [(2 * k, 2 * k + 1) for k in range(65)]
            assert raw_fields(lib, o, whole, TAB, many[:64], 64, 0)[0] == _native.OK and o.d.last_lines_members() == pl.n
            for what, call in (("field_delim == the table's delimiter", lambda: raw_fields(lib, o, whole, NL, [(0, 1)], 1, 0, p, 4096)),
                              ("field_delim > 255", lambda: raw_fields(lib, o, whole, 256, [(0, 1)], 1, 0, p, 4096)),
                              ("n_fields == 0", lambda: raw_fields(lib, o, whole, TAB, [(0, 1)], 0, 0, p, 4096)),
                              ("n_fields == 65", lambda: raw_fields(lib, o, whole, TAB, many, 65, 0, p, 4096)),
                              ("begin == end", lambda: raw_fields(lib, o, whole, TAB, [(3, 3)], 1, 0, p, 4096)),
                              ("begin > end", lambda: raw_fields(lib, o, whole, TAB, [(0, 1), (4, 3)], 2, 0, p, 4096)),
                              ("overlapping", lambda: raw_fields(lib, o, whole, TAB, [(0, 3), (2, 5)], 2, 0, p, 4096)),
                              ("descending", lambda: raw_fields(lib, o, whole, TAB, [(4, 5), (0, 1)], 2, 0, p, 4096)),
                              ("TO_END not in the last", lambda: raw_fields(lib, o, whole, TAB, [(0, END), (5, 6)], 2, 0, p, 4096)),
                              ("a flag that is not defined", lambda: raw_fields(lib, o, whole, TAB, [(0, 1)], 1, 2, p, 4096)),
                              ("a flag that is not defined, with COMPLEMENT", lambda: raw_fields(lib, o, whole, TAB, [(0, 1)], 1, 0x80000001, p, 4096)),
                              ("a bad list and no ranges", lambda: raw_fields(lib, o, [], TAB, [(3, 3)], 1, 0, p, 4096))):
                got = call()
                assert got == (INV, 0), (fmt, what, got)
                assert o.d.last_lines_members() == 0, (fmt, what)
                assert mem.get(keep, 4096) == bytes([FILL]) * 4096, (fmt, what)
                raw_fields(lib, o, [(0, 1)], TAB, [(0, 1)], 1, 0)  # (something is inflated in between)
            assert raw_fields(lib, o, whole, TAB, [(0, 1), (1, 2), (2, END)], 3, 1) == (_native.OK, ln.D)  # touching ranges, S empty
            # a bad line range
            good = [(0, 2), (L - 2, L), (5, 5)]
            for what, r, at in (("b = L + 1", [(L - 1, L + 1)], 3), ("a > b", [(11, 10)], 3), ("first", None, 0)):
                rs = good + r + good if r else [(L + 5, L + 6)] + good
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_fields_device(o.ix, o.lt, o.ptr, o.n, rs, TAB, [(0, 1)], p, 4096)
                assert (e.value.code, e.value.range_index) == (INV, at), (fmt, what)
                assert o.d.last_lines_members() == 0
                kr, rp = put_ranges(mem, rs)
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_fields_table_device(o.ix, o.lt, o.ptr, o.n, rp, len(rs), TAB, [(0, 1)], p, 4096)
                assert (e.value.code, e.value.range_index) == (INV, at), (fmt, what, "table form")
                assert mem.get(keep, 4096) == bytes([FILL]) * 4096, (fmt, what)
            # the table with the index of another stream, and with another context
            other = cut(fmt, table_text(12000, 7), [5000])
            keep2, ptr2 = mem.put(other)
            raw_fields(lib, o, [(0, 1)], TAB, [(0, 1)], 1, 0)
            with o.d.build_index_device(ptr2, len(other)) as ix2:
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_fields_device(ix2, o.lt, ptr2, len(other), [(0, 1)], TAB, [(0, 1)], p, 4096)
                assert e.value.code == INV and e.value.range_index is None and o.d.last_lines_members() == 0
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.read_fields_device(o.ix, o.lt, o.ptr, o.n, [(0, 1)], TAB, [(0, 1)], p, 4096)
                assert e.value.code == INV
            assert o.d.last_fields_ms() == (0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ 7. a damaged member
def damaged(lib):
    """A damaged member that the ranges touch: the inflate's error class and the member's index in the stream; the context
    serves on.  One that they do not touch is never seen."""
    mem = Mem(lib)
    for fmt in FORMATS:
        text = table_text(8 * 5000, 11)[:8 * 5000 - 1] + b"\n"
        s = cut(fmt, text, [5000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        fields = [(0, 2)]
        want = Want(ln, NL, TAB, fields, False)
        mid = int(np.searchsorted(ln.start, 3 * 5000 + 2500))  # its tile is the stream's second: members 3..6  # a line in the middle of member 3
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
                        kp, p = mem.put(bytes(len(text) + 16))
                        with o.d.build_index_device(ptr, len(m)) as ix:  # (the members' extents are the same: the table serves)
                            with pytest.raises(_native.GzpxError) as e:
                                o.d.read_fields_device(ix, o.lt, ptr, len(m), [(0, ln.L)], TAB, fields, p, len(text))
                            assert (e.value.code, e.value.block, e.value.needed) == (code, victim, None), (fmt, route, victim, what)
                            if victim != 3 and what == "crc":  # a range that does not touch the member
                                bad = type("O", (), dict(d=o.d, ix=ix, lt=o.lt, ptr=ptr, n=len(m)))
                                check(mem, bad, ln, want, [(mid, mid + 3)], TAB, fields, False, (fmt, route, victim, what), query=False)
                check(mem, o, ln, want, [(0, ln.L)], TAB, fields, False, (fmt, route, "after the damage"))
