"""Selection of lines by content (gzpx_select_lines_device) and the read by line that takes its table where it lies
(gzpx_read_lines_table_device), written once and run twice: through the emulated library on CPU
(tests/test_emu_select.py) and through the real HIP library on the MI355X (tests/test_gpu_select.py).

The yardstick is never the library's own inflate or search.  It is range_cases.Plain (zlib's inflate of every member,
joined), find_cases.host_hits / host_lines on it, integer division by the group, numpy's edge detection on the selected
records, and the join of the lines that line_cases.Lines cuts.

Not covered: GZPX_ERR_INVALID_ARG for R > 0xFFFFFFF0, which takes a stream of more than 2^32 lines."""
import ctypes
import os
import re

import numpy as np
import pytest

import find_cases
import line_cases
from find_cases import BATCHES, NL, TAB, host_hits, host_lines, letters, pattern_of
from gzp_amd import _native
from line_cases import Lines, cut, short_lines
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem

GUARD = 4    # entries behind runs_cap that must stay as they were
FILL = 0xEE
UNTOUCHED = int.from_bytes(bytes([FILL]) * 8, "little")

_dev = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gzp_amd", "csrc", "gzpx_device.h")).read()
RUN_RECORDS = int(re.search(r"kSlRunRecords = (\d+);", _dev).group(1))  # records per workgroup of the runs kernels
SCAN_STEP = int(re.search(r"kSlScanStep = (\d+);", _dev).group(1))      # workgroups per step of the runs scan


# ------------------------------------------------------------------------------------------------ the yardstick
def host_select(pl, ln, delim, pattern, g, invert):
    """(runs as line ranges, selected records, hits) by the definitions of include/gzpx.h."""
    hits = host_hits(pl.plain, bytes(pattern))
    lines = host_lines(pl.plain, delim, hits)
    L = ln.L
    R = -(-L // g)
    sel = np.zeros(R, dtype=bool)
    sel[np.unique(lines // g)] = True
    if invert:
        sel = ~sel
    edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
    r0, r1 = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    runs = [(int(g * a), int(min(g * b, L))) for a, b in zip(r0, r1)]
    assert len(runs) <= -(-R // 2)
    return runs, int(sel.sum()), int(hits.size)


# ------------------------------------------------------------------------------------------------ the calls
class Opened(line_cases.Opened):
    """A stream in device memory with its context, index and line table."""

    def __init__(self, lib, mem, fmt, s, delim=NL, route=ROUTES[0], batch=0, shift=0):
        super().__init__(lib, mem, fmt, s, delim, route, batch, shift)
        self.mem = mem

    def count(self, pattern, g=1, invert=False):
        return self.d.select_lines_device(self.ix, self.lt, self.ptr, self.n, pattern, g, invert)

    def select(self, pattern, g, invert, cap):
        """One writing call with `cap` entries and GUARD more behind them:
        ((n_runs, n_records, n_hits) or the GzpxError raised, the table's cap + GUARD entries as [begin, end] rows)."""
        room = (cap + GUARD) * 16
        keep, p = self.mem.put(bytes([FILL]) * room)
        try:
            got = self.d.select_lines_device(self.ix, self.lt, self.ptr, self.n, pattern, g, invert, p, cap)
        except _native.GzpxError as e:
            got = e
        return got, np.frombuffer(self.mem.get(keep, room), dtype=np.uint64).reshape(-1, 2).tolist()


def check(o, pl, ln, delim, pattern, g, invert, what, count=True):
    """Count only, then the runs into a table of exactly n_runs entries."""
    runs, records, hits = host_select(pl, ln, delim, pattern, g, invert)
    if count:
        assert o.count(pattern, g, invert) == (len(runs), records, hits), (what, "count only")
    got, table = o.select(pattern, g, invert, len(runs))
    assert got == (len(runs), records, hits), (what, "counts", got)
    assert table[:len(runs)] == [list(r) for r in runs], (what, "runs")
    assert table[len(runs):] == [[UNTOUCHED, UNTOUCHED]] * GUARD, (what, "written behind runs_cap")
    assert all(t >= 0.0 for t in o.d.last_select_ms())
    return runs


def check_batches(lib, mem, name, fmt, s, pl, delim, cases, route=ROUTES[0], batches=BATCHES, shift=0):
    """cases: (pattern, group, invert) triples; every one at every batch size (the count-only call at the first)."""
    ln = Lines(pl, delim)
    with Opened(lib, mem, fmt, s, delim, route, shift=shift) as o:
        for batch in batches:
            o.d.set_lines_batch(batch)
            for pattern, g, invert in cases:
                check(o, pl, ln, delim, pattern, g, invert, (name, fmt, route, batch, bytes(pattern[:20]), g, invert),
                      count=batch == batches[0])


# ------------------------------------------------------------------------------------------------ 1. bitmap and run edges
def record_sets(R):
    return [[0], [R - 1], [31], [32], [31, 32], [32, 33], [63, 64], list(range(30, 70)), list(range(0, R, 2)), list(range(R)), []]


def edge_sets(lib):
    """One line a record; the lines that hold "H" are exactly each of record_sets(R), R % 32 in {0, 1, 31}; plain and
    inverted, where the bits behind R must neither start a run nor count."""
    mem = Mem(lib)
    i = 0
    for R in (96, 97, 127):
        for chosen in record_sets(R):
            text = b"".join(b"H\n" if k in set(chosen) else b"x\n" for k in range(R))
            fmt, route = (BGZF, MGZIP)[i % 2], ROUTES[(i // 2) % 2]
            s = cut(fmt, text, [70, 131], eof=fmt == BGZF and i % 3 == 0)
            pl = Plain(fmt, s)
            ln = Lines(pl, NL)
            assert ln.L == R
            runs, records, _ = host_select(pl, ln, NL, b"H", 1, False)
            assert records == len(chosen) and (chosen != list(range(0, R, 2)) or len(runs) == -(-R // 2))
            check_batches(lib, mem, "R=%d set=%s" % (R, chosen[:4]), fmt, s, pl, NL, [(b"H", 1, False), (b"H", 1, True)], route,
                          batches=(0, 1) if i % 4 else BATCHES, shift=i % 16)
            i += 1


def scan_step(lib):
    """About 140,000 lines, mostly empty: the bitmap crosses one step of the runs scan (kSlScanStep workgroups of
    kSlRunRecords records).  Three patterns, each with runs of its own: across the step, ending at it, starting at it;
    the same at workgroups' edges; the first and the last record; both sides of a byte of the bitmap."""
    mem = Mem(lib)
    W, S = RUN_RECORDS, RUN_RECORDS * SCAN_STEP
    L = S + 4 * W + 37
    assert 130000 <= L <= 290000
    ranges = {b"A": [(0, 1), (3 * W - 1, 3 * W + 1), (S - 2, S + 3), (L - 1, L)],
              b"B": [(7, 8), (5 * W, 5 * W + 2), (S - 3, S), (S + W - 1, S + W), (S + 2 * W, S + 2 * W + 1)],
              b"C": [(8, 9), (5 * W - 2, 5 * W), (S, S + 2), (S + 3 * W - 64, S + 3 * W + 64)]}
    marks = {}
    for letter, rs in ranges.items():
        for a, b in rs:
            for k in range(a, b):
                marks[k] = marks.get(k, b"") + letter
    parts, at = [], 0
    for k in sorted(marks):
        parts += [b"\n" * (k - at), marks[k] + b"\n"]
        at = k + 1
    text = b"".join(parts) + b"\n" * (L - at)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [50000, 100000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        assert ln.L == L and len(s) <= 300000
        for letter, rs in ranges.items():
            assert host_select(pl, ln, NL, letter, 1, False)[0] == rs
        check_batches(lib, mem, "scan step", fmt, s, pl, NL, [(p, 1, inv) for p in ranges for inv in (False, True)],
                      route=ROUTES[fmt == MGZIP], batches=(0, 70000))


# ------------------------------------------------------------------------------------------------ 2. records
def record_text(L, terminated):
    """L lines; "HIT" twice in line 3, in lines 8 and 9, 12, 20, 28 and in the last line."""
    lines = [b"line %d of the text" % k for k in range(L)]
    for k in (8, 9, 12, 20, 28, L - 1):
        lines[k] = b"a HIT in line %d" % k
    lines[3] = b"HIT and HIT"
    return b"\n".join(lines) + (b"\n" if terminated else b"")


def records(lib):
    """g = 1, 2, 4, 5 and g > L; L a multiple of g and not; the last line terminated and not, a hit in it."""
    mem = Mem(lib)
    i = 0
    for L in (40, 43):
        for terminated in (True, False):
            text = record_text(L, terminated)
            for fmt in (BGZF, MGZIP):
                s = cut(fmt, text, [100, 333], eof=fmt == BGZF and terminated)
                pl = Plain(fmt, s)
                ln = Lines(pl, NL)
                assert ln.L == L and (ln.D == L) == terminated
                h = host_lines(pl.plain, NL, host_hits(pl.plain, b"HIT")).tolist()
                assert h == [3, 3, 8, 9, 12, 20, 28, L - 1]
                runs4 = host_select(pl, ln, NL, b"HIT", 4, False)[0]
                # (g = 4: lines 8 and 9 share record 2, record 3 is adjacent: one run; records 5 and 7 lie one apart: two)
                assert runs4[:4] == [(0, 4), (8, 16), (20, 24), (28, 32)] and runs4[-1][1] == L
                assert host_select(pl, ln, NL, b"HIT", 1000, False)[:2] == ([(0, L)], 1)
                cases = [(b"HIT", g, inv) for g in (1, 2, 4, 5, 1000, 1 << 40) for inv in (False, True)]
                # (three members of a few hundred bytes: every batch size but 1 is one batch)
                check_batches(lib, mem, "records L=%d t=%d" % (L, terminated), fmt, s, pl, NL, cases, ROUTES[i % 2],
                              batches=BATCHES if i == 0 else (0, 1), shift=i % 16)
                i += 1


# ------------------------------------------------------------------------------------------------ 3. line attribution
def attribution_every_split(lib):
    """find_cases.batches_every_split with delimiters: a hit for every split (k, 17 - k) of a 17-byte pattern across a batch
    boundary, a delimiter two bytes in front of every hit and one inside the pattern, so that the carry holds delimiters
    in front of and behind the hit's first byte.  With g = 4 two hits of one record lie in different batches."""
    mem = Mem(lib)
    pat = bytearray(pattern_of(17))
    pat[5] = NL
    pat = bytes(pat)
    text = bytearray(letters(18000, 13))
    starts = [1000 * k - k for k in range(1, 17)]
    for p in starts:
        text[p - 2] = NL
        text[p:p + 17] = pat
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, bytes(text), list(range(1000, 18000, 1000)))
        pl = Plain(fmt, s)
        hl = host_lines(pl.plain, NL, host_hits(pl.plain, pat))
        assert host_hits(pl.plain, pat).tolist() == starts and hl.tolist() == list(range(1, 32, 2))
        assert np.unique(hl // 4).size == 8  # two hits a record, 1,000 bytes apart
        cases = [(pat, 1, False), (pat, 4, True), (pat, 2, False), (pat[5:], 1, True)]
        # (members of 1,000 bytes: a batch of 1,000 and a batch of 1 both make every member a batch)
        check_batches(lib, mem, "every split", fmt, s, pl, NL, cases, route=ROUTES[1], batches=(0, 1000) if fmt == BGZF else (0, 1))


def attribution_tiny_members(lib):
    """About 300 members of one to three bytes, each a batch of its own (find_cases.batches_tiny_members)."""
    mem = Mem(lib)
    rng = np.random.default_rng(11)
    text = bytearray(b"abcdefg" * 90)
    for p in (20, 330, 600):
        text[p] = ord("X")
    cuts = np.cumsum(rng.integers(1, 4, 400))
    cuts = cuts[cuts < len(text)].tolist()
    long_pat, short_pat = bytes(text[23:279]), bytes(text[400:417])
    for fmt, case in ((BGZF, (short_pat, 4, True)), (MGZIP, (long_pat, 1, False))):
        s = cut(fmt, bytes(text), cuts, eof=fmt == BGZF)
        pl = Plain(fmt, s)
        assert 280 <= pl.n <= 350 and max(pl.isize) <= 3
        assert host_select(pl, Lines(pl, ord("a")), ord("a"), *case)[2] >= 7
        check_batches(lib, mem, "tiny members", fmt, s, pl, ord("a"), [case], route=ROUTES[fmt == BGZF], batches=(0, 1))


def attribution_delimiters(lib):
    """Patterns that start with, end with and consist of the delimiter; a hit across a cut with delimiters around its
    first byte; a delimiter of 0x09 (find_cases.line_text)."""
    mem = Mem(lib)
    for delim in (NL, TAB):
        d = bytes([delim])
        for terminated in (True, False):
            text, cross_at = find_cases.line_text(delim, terminated)
            patterns = [b"HIT", b"HIT" + d, d + b"HIT", b"a" + d + b"HIT" + d + b"b", d, d + d]
            cases = [(p, (1, 4)[j % 2], j % 3 == 1) for j, p in enumerate(patterns)] + [(b"HIT", 2, True), (d, 3, False)]
            fmt = BGZF if terminated == (delim == NL) else MGZIP
            s = cut(fmt, text, [40, cross_at + 6, 6000], eof=fmt == BGZF and terminated)
            pl = Plain(fmt, s)
            # (four members of a few thousand bytes: every batch size but 1 is one batch)
            check_batches(lib, mem, "delimiters", fmt, s, pl, delim, cases, route=ROUTES[delim == TAB], batches=(0, 1))


# ------------------------------------------------------------------------------------------------ 4. lost updates
def lost_updates(lib):
    """24,000 lines of two bytes that all hit: every bit of the bitmap is set, 32 of a word by four lanes, and the words
    at the pieces' edges by two workgroups.  One run {0, L} with n_records = R.  (The emulator's atomics are
    cooperative: only the run on the GPU decides whether the update is atomic.)"""
    mem = Mem(lib)
    L = 24000
    text = b"H\n" * L
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [9000, 30001])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        assert ln.L == L
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for batch in (0, 20000):
                o.d.set_lines_batch(batch)
                for g in (1, 4, 5):
                    R = -(-L // g)
                    got, table = o.select(b"H", g, False, 1)
                    assert got == (1, R, L) and table[0] == [0, L], (fmt, batch, g, got, table[0])
                    assert o.count(b"H", g, True) == (0, 0, L), (fmt, batch, g)
                    assert check(o, pl, ln, NL, b"H", g, False, (fmt, batch, g)) == [(0, L)]


# ------------------------------------------------------------------------------------------------ 5. capacity
def capacity(lib):
    mem = Mem(lib)
    text, _ = find_cases.line_text(NL, True)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        with Opened(lib, mem, fmt, s) as o:
            for pattern, g, invert in ((b"HIT", 1, False), (b"qu", 2, False), (b"e", 1, True)):
                runs, records, hits = host_select(pl, ln, NL, pattern, g, invert)
                n = len(runs)
                assert n >= 5
                for batch in (0, 5000):
                    o.d.set_lines_batch(batch)
                    # (count only: runs_cap is ignored)
                    assert o.d.select_lines_device(o.ix, o.lt, o.ptr, o.n, pattern, g, invert, None, 3) == (n, records, hits)
                    for cap in (n, n + 3, n - 1, 1, 0):
                        got, table = o.select(pattern, g, invert, cap)
                        what = (fmt, pattern, g, invert, batch, cap)
                        if cap >= n:
                            assert got == (n, records, hits), what
                        else:
                            assert isinstance(got, _native.GzpxError), what
                            assert (got.code, got.needed) == (_native.ERR_INSUFFICIENT_SPACE, n), what
                        k = min(cap, n)
                        assert table[:k] == [list(r) for r in runs[:k]], what
                        assert table[k:] == [[UNTOUCHED, UNTOUCHED]] * (cap + GUARD - k), (what, "written behind runs_cap")


# ------------------------------------------------------------------------------------------------ 6. errors
def raw_select(lib, o, pattern, m, g, flags, d_runs=None, cap=0, n=None):
    runs, records, hits, info = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint64(77), _native.GzpxCheckInfo()
    rc = lib.L.gzpx_select_lines_device(o.d.h, o.ix.h, o.lt.h, o.ptr, o.n if n is None else n, pattern, m, g, flags, d_runs, cap,
                                        ctypes.byref(runs), ctypes.byref(records), ctypes.byref(hits), ctypes.byref(info), None)
    return rc, runs.value, records.value, hits.value, info.block


def errors(lib):
    mem = Mem(lib)
    text, _ = find_cases.line_text(NL, True)
    INV = _native.ERR_INVALID_ARG
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        with Opened(lib, mem, fmt, s) as o:
            keep, p = mem.put(bytes([FILL]) * 64)
            for what, got in (("group == 0", raw_select(lib, o, b"HIT", 3, 0, 0, p, 4)),
                              ("a flag that is not defined", raw_select(lib, o, b"HIT", 3, 1, 2, p, 4)),
                              ("a flag that is not defined, with INVERT", raw_select(lib, o, b"HIT", 3, 1, 0x80000001, p, 4)),
                              ("pattern_len == 0", raw_select(lib, o, b"HIT", 0, 1, 0, p, 4)),
                              ("pattern_len == 257", raw_select(lib, o, b"x" * 257, 257, 1, 0, p, 4)),
                              ("fewer bytes than the index covers", raw_select(lib, o, b"HIT", 3, 1, 0, p, 4, n=o.n - 1))):
                assert got[:4] == (INV, 0, 0, 0), (fmt, what, got)
                assert mem.get(keep, 64) == bytes([FILL]) * 64, (fmt, what)
            assert raw_select(lib, o, b"x" * 256, 256, 1, 0)[:4] == (_native.OK, 0, 0, 0)
            assert o.count(b"HIT", 1 << 63)[:2] == (1, 1) and o.count(b"HIT", (1 << 64) - 1, True)[:2] == (0, 0)
            # the table with the index of another stream, and with another context
            other = cut(fmt, short_lines(12000, 5), [5000])
            keep2, ptr2 = mem.put(other)
            with o.d.build_index_device(ptr2, len(other)) as ix2:
                with pytest.raises(_native.GzpxError) as e:
                    o.d.select_lines_device(ix2, o.lt, ptr2, len(other), b"HIT")
                assert e.value.code == INV and e.value.needed is None
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.select_lines_device(o.ix, o.lt, o.ptr, o.n, b"HIT")
                assert e.value.code == INV
        # m > n: nothing is inflated; plain no run, inverted the one run {0, L}
        for text2, L in ((b"ab\ncd", 2), (b"ab\n", 1)):
            s2 = cut(fmt, text2, [1])
            with Opened(lib, mem, fmt, s2) as o:
                pat = b"x" * (len(text2) + 1)
                assert o.lt.n_lines == L
                assert o.count(pat) == (0, 0, 0) and o.select(pat, 1, False, 2) == ((0, 0, 0), [[UNTOUCHED] * 2] * (2 + GUARD))
                assert o.count(pat, 1, True) == (1, L, 0) and o.count(pat, 5, True) == (1, 1, 0)
                got, table = o.select(pat, 1, True, 1)
                assert got == (1, L, 0) and table == [[0, L]] + [[UNTOUCHED] * 2] * GUARD
                got, table = o.select(pat, 1, True, 0)
                assert isinstance(got, _native.GzpxError) and (got.code, got.needed) == (_native.ERR_INSUFFICIENT_SPACE, 1)
                assert table == [[UNTOUCHED] * 2] * GUARD
                assert o.d.last_select_ms() == (0.0, 0.0, 0.0)
                assert o.count(text2[:2]) == (1, 1, 1)  # m <= n: the stream is searched
        # L == 0: no member, and empty members only
        for s0 in (b"", cut(fmt, b"", [0, 0])):
            with Opened(lib, mem, fmt, s0) as o:
                assert o.lt.n_lines == 0
                for invert in (False, True):
                    assert o.count(b"x", 3, invert) == (0, 0, 0)
                    assert o.select(b"x", 1, invert, 1) == ((0, 0, 0), [[UNTOUCHED] * 2] * (1 + GUARD))


def damaged(lib):
    """A damaged member: the inflate's error class and the member's index in the stream (two members a batch), zeros in
    the counts; the context serves on."""
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        text = short_lines(8 * 5000, 11)
        s = cut(fmt, text, [5000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        for route in ROUTES:
            with Opened(lib, mem, fmt, s, route=route, batch=11000) as o:  # (the table of the undamaged stream)
                for victim in (0, 3, 7):
                    for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                           ("block type", pl.off[victim] + HDR[fmt], _native.ERR_BAD_DATA)):
                        m = bytearray(s)
                        if what == "crc":
                            m[at] ^= 0xFF
                        else:
                            m[at] |= 0x06  # BTYPE = 3, reserved
                        keep, ptr = mem.put(m)
                        kr, rp = mem.put(b"\0" * 16 * 64)
                        with o.d.build_index_device(ptr, len(m)) as ix:  # (the members' extents are the same: the table serves)
                            with pytest.raises(_native.GzpxError) as e:
                                o.d.select_lines_device(ix, o.lt, ptr, len(m), b"e\n", 2, False, rp, 64)
                            assert (e.value.code, e.value.block, e.value.needed) == (code, victim, None), (fmt, route, victim, what)
                            bad = type("O", (), dict(d=o.d, ix=ix, lt=o.lt, ptr=ptr, n=len(m)))
                            if what == "crc":  # the counts as the C call leaves them
                                assert raw_select(lib, bad, b"e", 1, 1, 1) == (code, 0, 0, 0, victim), (fmt, route, victim)
                runs, records, hits = host_select(pl, ln, NL, b"e\n", 2, False)
                assert o.count(b"e\n", 2) == (len(runs), records, hits)


# ------------------------------------------------------------------------------------------------ 7. the read by table
def put_ranges(mem, ranges):
    a = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
    return mem.put(a.tobytes() if a.size else b"\0" * 16)


def read_table(mem, o, ranges, cap=None, offsets=True, byte_ranges=True, fill=FILL):
    """One gzpx_read_lines_table_device into an output misaligned by 3 with guard bytes behind it, the two optional
    tables with GUARD entries behind theirs: (bytes returned, d_out_offsets or None, d_byte_ranges or None)."""
    n = len(ranges)
    room = (cap if cap is not None else 0) + 64
    keep, p = mem.put(bytes([fill]) * room, shift=3)
    kr, rp = put_ranges(mem, ranges)
    ko, op = mem.put(bytes([fill]) * 8 * (n + 1 + GUARD)) if offsets else (None, None)
    kb, bp = mem.put(bytes([fill]) * 16 * (n + GUARD)) if byte_ranges else (None, None)
    out_len = o.d.read_lines_table_device(o.ix, o.lt, o.ptr, o.n, rp, n, p, cap, op, bp)
    whole = mem.get(keep, room + 3)[3:]
    assert whole[out_len:] == bytes([fill]) * (room - out_len), "bytes written behind the output"
    if n:
        assert mem.get(kr, 16 * n) == np.array(ranges, dtype=np.uint64).tobytes(), "the range table was written"
    offs = np.frombuffer(mem.get(ko, 8 * (n + 1 + GUARD)), dtype=np.uint64).tolist() if offsets else None
    br = np.frombuffer(mem.get(kb, 16 * (n + GUARD)), dtype=np.uint64).reshape(-1, 2).tolist() if byte_ranges else None
    return whole[:out_len], offs, br


def check_read_table(mem, o, ln, ranges, what, twin=False, **tables):
    want = [ln.byte_range(a, b) for a, b in ranges]
    lens = [e - b for b, e in want]
    got, offs, br = read_table(mem, o, ranges, cap=sum(lens), **tables)
    assert got == ln.expected(ranges), (what, "bytes")
    if offs is not None:
        assert offs == [0] + np.cumsum(lens).tolist() + [UNTOUCHED] * GUARD, (what, "d_out_offsets")
    if br is not None:
        assert br == [list(x) for x in want] + [[UNTOUCHED] * 2] * GUARD, (what, "d_byte_ranges")
    members = o.d.last_lines_members()
    assert members == len(ln.pl.union([ln.cover(a, b) for a, b in ranges])), (what, "members read")
    if twin:  # the host's twin reads the same members
        keep, p = mem.put(b"\0" * (sum(lens) + 16))
        o.d.read_lines_device(o.ix, o.lt, o.ptr, o.n, np.array(ranges, dtype=np.uint64), p, sum(lens))
        assert o.d.last_lines_members() == members, (what, "members read by read_lines_device")
    assert all(t >= 0.0 for t in o.d.last_lines_ms())


def table_reads(lib, oracle):
    """Ranges that overlap, repeat, are empty ([L, L) among them) or lie in any order (line_cases.range_set, shuffled)
    against the joined lines; each of the two optional tables present and absent."""
    mem = Mem(lib)
    names = ("bgzf crafted", "mgzip crafted, unterminated", "mgzip members of 5,000 bytes", "bgzf no member", "mgzip 1 bytes")
    picked = [x for x in line_cases.streams(oracle) if x[0] in names]
    assert len(picked) == len(names)
    for i, (name, fmt, s, pl) in enumerate(picked):
        ln = Lines(pl, NL)
        rs = line_cases.range_set(ln, 2000 + i)
        shuffled = [rs[j] for j in np.random.default_rng(i).permutation(len(rs))]
        few = [r for r in rs[::11] if r[1] - r[0] < 30]
        with Opened(lib, mem, fmt, s, route=ROUTES[i % 2], shift=(5 * i) % 16) as o:
            check_read_table(mem, o, ln, shuffled, (name, "shuffled"))
            check_read_table(mem, o, ln, few, (name, "few, no d_out_offsets"), twin=bool(few), offsets=False)
            check_read_table(mem, o, ln, few[::-1], (name, "few, no d_byte_ranges"), byte_ranges=False)
            check_read_table(mem, o, ln, [(0, ln.L)], (name, "whole, no tables"), offsets=False, byte_ranges=False)
            check_read_table(mem, o, ln, [(ln.L, ln.L)], (name, "empty"), twin=True)
            assert read_table(mem, o, [], cap=0) == (b"", [0] + [UNTOUCHED] * GUARD, [[UNTOUCHED] * 2] * GUARD)
            assert o.d.last_lines_members() == 0


def table_errors(lib, oracle):
    mem = Mem(lib)
    all_streams = line_cases.streams(oracle)
    for name, fmt, s, pl in all_streams[:2]:
        ln = Lines(pl, NL)
        L = ln.L
        with Opened(lib, mem, fmt, s) as o:
            good = [(0, 2), (L - 2, L), (5, 5)]
            for what, r, at in (("b = L + 1", [(L - 1, L + 1)], 3), ("a > b", [(11, 10)], 3), ("both", [(L, L + 1), (7, 2)], 3),
                                ("first", None, 0), ("huge", [(0, 1 << 63)], 3)):
                rs = good + r + good if r else [(L + 5, L + 6)] + good
                with pytest.raises(_native.GzpxError) as e:
                    read_table(mem, o, rs, cap=4096)
                assert (e.value.code, e.value.range_index) == (_native.ERR_INVALID_ARG, at), (name, what)
                assert o.d.last_lines_members() == 0
            # an output that is one byte short: the size needed, nothing written to d_out
            rs = [(0, L), (L // 2, L)]
            need = ln.total + ln.total - int(ln.start[L // 2])
            for cap in (need - 1, 0):
                keep, p = mem.put(bytes([FILL]) * (need + 64))
                kr, rp = put_ranges(mem, rs)
                kb, bp = mem.put(bytes([FILL]) * 16 * (2 + GUARD))
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_lines_table_device(o.ix, o.lt, o.ptr, o.n, rp, 2, p, cap, None, bp)
                assert (e.value.code, e.value.needed) == (_native.ERR_INSUFFICIENT_SPACE, need), (name, cap)
                assert mem.get(keep, need + 64) == bytes([FILL]) * (need + 64), (name, cap, "output written")
                br = np.frombuffer(mem.get(kb, 16 * (2 + GUARD)), dtype=np.uint64).reshape(-1, 2).tolist()
                assert br == [[0, ln.total], [int(ln.start[L // 2]), ln.total]] + [[UNTOUCHED] * 2] * GUARD, (name, cap)
            assert read_table(mem, o, rs, cap=need)[0] == ln.expected(rs)
            # fewer bytes than the index covers; another context
            kr, rp = put_ranges(mem, [(0, 1)])
            with pytest.raises(_native.GzpxError) as e:
                o.d.read_lines_table_device(o.ix, o.lt, o.ptr, o.n - 1, rp, 1, o.ptr, 0)
            assert e.value.code == _native.ERR_INVALID_ARG and e.value.range_index is None
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.read_lines_table_device(o.ix, o.lt, o.ptr, o.n, rp, 1, o.ptr, 0)
                assert e.value.code == _native.ERR_INVALID_ARG and e.value.range_index is None


# ------------------------------------------------------------------------------------------------ 8. closing the loop
def close_the_loop(lib):
    """select, then read_lines_table_device on d_runs: the joined selected records, byte for byte.  The test reads the
    counts; the table stays where select wrote it."""
    mem = Mem(lib)
    text, cross_at = find_cases.line_text(NL, False)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, cross_at + 6, 6000])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        all_lines = pl.plain.splitlines(keepends=True)
        assert len(all_lines) == ln.L
        with Opened(lib, mem, fmt, s, route=ROUTES[fmt == MGZIP]) as o:
            for batch in (0, 1):
                o.d.set_lines_batch(batch)
                for g in (1, 4):
                    for invert in (False, True):
                        recs = [all_lines[k:k + g] for k in range(0, ln.L, g)]
                        want = b"".join(b"".join(r) for r in recs if any(b"HIT" in x for x in r) != invert)
                        cap_runs = -(-len(recs) // 2)
                        kr, rp = mem.put(bytes([FILL]) * 16 * cap_runs)
                        n_runs, n_records, n_hits = o.d.select_lines_device(o.ix, o.lt, o.ptr, o.n, b"HIT", g, invert, rp, cap_runs)
                        assert n_records == sum(1 for r in recs if any(b"HIT" in x for x in r) != invert) and n_runs >= 2
                        keep, p = mem.put(bytes([FILL]) * (len(want) + 64), shift=5)
                        out_len = o.d.read_lines_table_device(o.ix, o.lt, o.ptr, o.n, rp, n_runs, p, len(want))
                        assert out_len == len(want), (fmt, batch, g, invert)
                        assert mem.get(keep, len(want) + 64 + 5)[5:] == want + bytes([FILL]) * 64, (fmt, batch, g, invert)
