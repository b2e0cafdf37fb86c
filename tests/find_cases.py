"""The search (gzpx_find_device), written once and run twice: through the emulated library on CPU
(tests/test_emu_find.py) and through the real HIP library on the MI355X (tests/test_gpu_find.py).

The yardstick is never the library's own inflate.  It is range_cases.Plain: zlib's inflate of every member, joined.  The
hits come from a loop of bytes.find(pattern, p + 1), the lines from np.searchsorted over np.flatnonzero(plain == delim),
as include/gzpx.h defines them."""
import ctypes

import numpy as np
import pytest

import line_cases
from gzp_amd import _native
from line_cases import Lines, cut, short_lines
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem

T = 16384    # the piece of staging a workgroup searches
PAD = 256    # staging starts with a pad of this size: byte p of a batch lies at PAD + p
BATCHES = (0, 70000, 20000, 1)
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 255, 256)
NL, TAB = 0x0A, 0x09
GUARD = 4    # entries behind hits_cap that must stay as they were
FILL = 0xEE


# ------------------------------------------------------------------------------------------------ the yardstick
def host_hits(plain, pattern):
    hits, p = [], plain.find(pattern)
    while p >= 0:
        hits.append(p)
        p = plain.find(pattern, p + 1)
    return np.array(hits, dtype=np.int64)


def host_lines(plain, delim, hits):
    return np.searchsorted(np.flatnonzero(np.frombuffer(plain, dtype=np.uint8) == delim), hits, side="left").astype(np.int64)


_wanted = {}


def wanted(pl, pattern, delim):
    """(hits, lines) of the host's search; computed once per (stream, pattern, delimiter) and left unchanged."""
    key = (id(pl), bytes(pattern), delim)
    if key not in _wanted:
        hits = host_hits(pl.plain, bytes(pattern))
        lines = host_lines(pl.plain, delim, hits) if delim is not None else None
        _wanted[key] = (pl, hits, lines)  # (pl kept alive: its id stays its own)
    return _wanted[key][1:]


# ------------------------------------------------------------------------------------------------ the call
class Opened:
    """A stream in device memory with its context and index."""

    def __init__(self, lib, mem, fmt, s, route=ROUTES[0], shift=0):
        self.mem = mem
        self.keep, self.ptr = mem.put(s, shift=shift)
        self.n = len(s)
        self.d = _native.DContext(format=fmt, lib=lib)
        self.d.set_route(route)
        self.ix = self.d.build_index_device(self.ptr, self.n)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix.close()
        self.d.close()

    def count(self, pattern, delim=None):
        return self.d.find_device(self.ix, self.ptr, self.n, pattern, delim)

    def find(self, pattern, delim, cap, positions=True, lines=True):
        """One writing call with `cap` entries and GUARD more behind them in each array:
        (n_hits or the GzpxError raised, positions[:cap + GUARD] or None, lines[:cap + GUARD] or None)."""
        room = (cap + GUARD) * 8
        kp, pp = self.mem.put(bytes([FILL]) * room) if positions else (None, None)
        kl, lp = self.mem.put(bytes([FILL]) * room) if lines else (None, None)
        try:
            got = self.d.find_device(self.ix, self.ptr, self.n, pattern, delim, pp, lp, cap)
        except _native.GzpxError as e:
            got = e
        back = lambda k: np.frombuffer(self.mem.get(k, room), dtype=np.uint64) if k is not None else None
        return got, back(kp), back(kl)


UNTOUCHED = np.frombuffer(bytes([FILL]) * 8 * GUARD, dtype=np.uint64)


def check(o, pl, pattern, delim, what):
    """Count only, then positions and lines into arrays of exactly n_hits entries."""
    hits, lines = wanted(pl, pattern, delim)
    assert o.count(pattern) == hits.size, (what, "count only")
    n, pos, ln = o.find(pattern, delim, hits.size, lines=delim is not None)
    assert n == hits.size, (what, "n_hits", n)
    assert pos[:hits.size].tolist() == hits.tolist(), (what, "positions")
    assert np.array_equal(pos[hits.size:], UNTOUCHED), (what, "positions written behind hits_cap")
    if delim is not None:
        assert ln[:hits.size].tolist() == lines.tolist(), (what, "lines")
        assert np.array_equal(ln[hits.size:], UNTOUCHED), (what, "lines written behind hits_cap")
    assert all(t >= 0.0 for t in o.d.last_find_ms())


def check_batches(lib, mem, name, fmt, s, pl, cases, route=ROUTES[0], batches=BATCHES, shift=0):
    """cases: (pattern, delim) pairs; every one at every batch size."""
    with Opened(lib, mem, fmt, s, route, shift) as o:
        for batch in batches:
            o.d.set_lines_batch(batch)
            for pattern, delim in cases:
                check(o, pl, pattern, delim, (name, route, batch, bytes(pattern[:20]), len(pattern), delim))


# ------------------------------------------------------------------------------------------------ 1. planted hits
def letters(n, seed):
    return np.random.default_rng(seed).integers(ord("a"), ord("z") + 1, n, dtype=np.uint8).tobytes()


def pattern_of(m, seed=0):
    """m bytes: a lower-case first byte, which the text is full of, then capitals, which it does not hold."""
    rng = np.random.default_rng(1000 + m + seed)
    return b"a" + rng.integers(ord("A"), ord("Z") + 1, m - 1, dtype=np.uint8).tobytes()


N_PLANT = 2 * T + 5000
PLANT_CUTS = [12000, 20000, 20000, 26000]  # (20000 twice: an empty member; with batches of 20,000 a batch ends there too)


def planted(m, seed=0):
    """(text, pattern, the starts planted): at 0 and ending at n; starting at and ending at each of the 16 offsets of a
    word (every dword crossing among them); across the pieces' edges of staging (with the default batch byte p lies at
    PAD + p, with a batch that starts at 20,000 at PAD + p - 20000), across a member cut, and across a cut with an empty
    member in it, which batches of 20,000 make a batch boundary."""
    n, pat = N_PLANT, pattern_of(m, seed)
    starts, cursor = [0], 300
    for o in range(16):
        at = (cursor + 15) // 16 * 16 + 16 + o
        starts.append(at)
        cursor = at + m + 1
    for o in range(16):
        end = (cursor + m + 15) // 16 * 16 + 16 + o
        starts.append(end - m)
        cursor = end + 1
    assert cursor < 11000
    half = max(m // 2, 1)
    for edge in (12000, T - PAD, T, 20000, 20000 + T - PAD, 2 * T - PAD, 2 * T):
        starts.append(edge - half)
        if m == 1:
            starts.append(edge)
    starts.append(n - m)
    text = bytearray(letters(n, 7 + m))
    for p in starts:
        text[p:p + m] = pat
    return bytes(text), pat, sorted(starts)


def planted_streams():
    for m in LENGTHS:
        text, pat, starts = planted(m)
        for fmt in (BGZF, MGZIP):
            eof = fmt == BGZF and m % 2 == 1  # with and without the BGZF EOF member
            s = cut(fmt, text, PLANT_CUTS, eof=eof)
            yield "planted m=%d fmt=%d eof=%d" % (m, fmt, eof), fmt, s, Plain(fmt, s), pat, starts


def hits_planted(lib):
    mem = Mem(lib)
    for i, (name, fmt, s, pl, pat, starts) in enumerate(planted_streams()):
        hits, _ = wanted(pl, pat, None)
        assert set(starts) <= set(hits.tolist()) and (len(pat) == 1 or hits.size == len(starts)), name
        assert pl.isize.count(0) == (2 if "eof=1" in name else 1)
        check_batches(lib, mem, name, fmt, s, pl, [(pat, None)], ROUTES[i % 2], shift=i % 16)


def hits_small_members(lib):
    """A 10-byte pattern across four members of 3 bytes; a hit that crosses a cut with two empty members in it."""
    mem = Mem(lib)
    pat = pattern_of(10)
    text = bytearray(letters(2000, 3))
    for p in (0, 1001, 1500 - 4, 2000 - 10):
        text[p:p + 10] = pat
    cuts = list(range(1000, 1031, 3)) + [1500, 1500, 1500]
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, bytes(text), cuts, eof=fmt == BGZF)
        pl = Plain(fmt, s)
        assert len(pl.union([(1001, 1011)])) == 4 and wanted(pl, pat, None)[0].tolist() == [0, 1001, 1496, 1990]
        check_batches(lib, mem, "members of 3 bytes", fmt, s, pl, [(pat, None), (pat[:1], None), (pat[:3], NL)])


def hits_newline(lib, oracle):
    """The newline as a pattern of one byte: D of line_cases.Lines and the delimiters' positions."""
    mem = Mem(lib)
    all_streams = line_cases.streams(oracle)
    for name, fmt, s, pl in all_streams[:2] + [x for x in all_streams if x[0] in ("mgzip crafted", "bgzf crafted + EOF")]:
        ln = Lines(pl, NL)
        hits, lines = wanted(pl, b"\n", NL)
        assert hits.size == ln.D and hits.tolist() == (ln.start[1:ln.D + 1] - 1).tolist() and lines.tolist() == list(range(ln.D))
        check_batches(lib, mem, name, fmt, s, pl, [(b"\n", NL)])


SPECIAL = (0x00, 0x7F, 0x80, 0xFF)


def hits_special_bytes(lib):
    """0x00, 0x7F, 0x80 and 0xFF on random bytes, where the bytes that differ from them in one bit or by one stand beside
    them: alone, doubled, and in front of the byte that follows their first occurrence."""
    mem = Mem(lib)
    for name, fmt, s, pl in line_cases.binary_streams():
        cases = []
        for b in SPECIAL:
            first = pl.plain.find(bytes([b]))
            long_one = pl.plain[first:first + 5]
            cases += [(bytes([b]), None), (bytes([b, b]), b), (pl.plain[first:first + 2], None), (long_one, SPECIAL[(SPECIAL.index(b) + 1) % 4])]
            assert wanted(pl, bytes([b]), None)[0].size > 100 and wanted(pl, long_one, None)[0].size >= 1
        check_batches(lib, mem, name, fmt, s, pl, cases)


def hits_overlaps(lib):
    mem = Mem(lib)
    a40 = b"A" * 40000
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, a40, [9000, 25000])
        pl = Plain(fmt, s)
        assert wanted(pl, b"A" * 256, None)[0].size == 39745 and wanted(pl, b"AAAA", None)[0].size == 39997
        # (the last two: a first byte that is everywhere under a pattern that never matches)
        check_batches(lib, mem, "40,000 x A", fmt, s, pl, [(b"A", None), (b"AAAA", None), (b"A" * 256, None), (b"AB", None), (b"A" * 5 + b"B", None)])
        s = cut(fmt, b"ab" * 20000, [16000, 16001, 33333])
        pl = Plain(fmt, s)
        assert wanted(pl, b"abab", None)[0].size == 19999
        check_batches(lib, mem, "ab x 20,000", fmt, s, pl, [(b"abab", None), (b"ba", None)])


def hits_edges(lib):
    """A pattern absent; m = n; m = n + 1; no member; empty members only."""
    mem = Mem(lib)
    text = letters(300, 5)
    for fmt in (BGZF, MGZIP):
        for name, s, cases in (("absent", cut(fmt, letters(40000, 6), [17000]), [(b"aQ", None), (b"QQQQQQQQQQQQ", NL), (b"Q", None)]),
                               ("m = n, m = n + 1", cut(fmt, text[:256], [100]), [(text[:256], None), (text[:255], NL), (text[1:256], None)]),
                               ("m = n + 1", cut(fmt, text[:255], [255]), [(text[:256], None), (text[:255], None)]),
                               ("one byte", cut(fmt, b"x", []), [(b"x", NL), (b"xx", None), (b"y", None)]),
                               ("no member", b"", [(b"x", None), (b"x", NL)]),
                               ("empty members only", cut(fmt, b"", [0, 0]), [(b"x", None), (b"x" * 256, NL)])):
            pl = Plain(fmt, s)
            check_batches(lib, mem, name, fmt, s, pl, cases)


# ------------------------------------------------------------------------------------------------ 2. batches
def batches_tiny_members(lib):
    """About 300 members of one to three bytes, each a batch of its own: the carry is put together from many batches and
    every hit starts in it."""
    mem = Mem(lib)
    rng = np.random.default_rng(11)
    text = bytearray(b"abcdefg" * 90)
    for p in (20, 330, 600):
        text[p] = ord("X")  # (between 21 and 329 the period holds for 309 bytes)
    cuts = np.cumsum(rng.integers(1, 4, 400))
    cuts = cuts[cuts < len(text)].tolist()
    long_pat, short_pat = bytes(text[23:279]), bytes(text[400:417])
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, bytes(text), cuts, eof=fmt == BGZF)
        pl = Plain(fmt, s)
        assert 280 <= pl.n <= 350 and max(pl.isize) <= 3
        assert wanted(pl, long_pat, None)[0].size >= 7 and wanted(pl, short_pat, None)[0].size >= 70
        check_batches(lib, mem, "tiny members", fmt, s, pl, [(short_pat, ord("X")), (long_pat, ord("a"))], batches=(1, 0))


def batches_every_split(lib):
    """A hit for every split (k, 17 - k) of a 17-byte pattern across a batch boundary: members of 1,000 bytes, one a batch."""
    mem = Mem(lib)
    pat = pattern_of(17)
    text = bytearray(letters(18000, 13))
    starts = [1000 * k - k for k in range(1, 17)]
    for p in starts:
        text[p:p + 17] = pat
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, bytes(text), list(range(1000, 18000, 1000)))
        pl = Plain(fmt, s)
        assert wanted(pl, pat, None)[0].tolist() == starts
        check_batches(lib, mem, "every split", fmt, s, pl, [(pat, None), (pat, ord("e"))], batches=(1000, 1, 0), route=ROUTES[1])


# ------------------------------------------------------------------------------------------------ 3. lines
def line_text(delim, terminated):
    d = bytes([delim])
    head = (b"HIT in the first line" + d + d + d + b"one HIT and another HIT here" + d + d + b"ends with HIT" + d + b"HIT starts" + d
            + d + d + b"around HITHIT" + d + d)
    body = short_lines(3000, 21, delim)
    # a hit across a cut (with batch 1 a batch boundary) with delimiters in the carry in front of and behind its first byte
    cross_at = len(head) + len(body) + 3
    cross = b"q" + d + b"za" + d + b"HIT" + d + b"b" + d + d
    tail = short_lines(6000, 22, delim) + d + b"the last line has a HIT" + (d if terminated else b"")
    return head + body + b"ppp" + cross + tail, cross_at


def lines(lib):
    mem = Mem(lib)
    for delim in (NL, TAB):
        d = bytes([delim])
        for terminated in (True, False):
            text, cross_at = line_text(delim, terminated)
            cases = [(b"HIT", delim), (b"HIT" + d, delim), (d + b"HIT", delim), (b"a" + d + b"HIT" + d + b"b", delim), (d, delim),
                     (d + d, delim), (b"HIT", NL + TAB - delim)]
            for fmt in (BGZF, MGZIP):
                s = cut(fmt, text, [40, cross_at + 6, 6000], eof=fmt == BGZF and terminated)
                pl = Plain(fmt, s)
                assert text[cross_at + 6:cross_at + 8] == b"IT" and text[cross_at + 2:cross_at + 4] == b"za"
                for pattern, dl in cases[:4]:
                    assert wanted(pl, pattern, dl)[0].size >= 1
                ln = Lines(pl, delim)
                hits, hl = wanted(pl, b"HIT", delim)
                assert hl[0] == 0 and hl[-1] == ln.L - 1 and np.unique(hl).size < hl.size  # first line, last line, two in a line
                check_batches(lib, mem, "lines", fmt, s, pl, cases, route=ROUTES[delim == TAB])


def lines_close_the_loop(lib):
    """find -> line_offsets_device and read_lines_device: every hit lies in the line it was given, and reading the lines
    of the hits returns the lines that hold the pattern."""
    mem = Mem(lib)
    text, cross_at = line_text(NL, False)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, cross_at + 6, 6000])
        pl = Plain(fmt, s)
        with line_cases.Opened(lib, mem, fmt, s) as o:
            for batch in (0, 1):
                o.d.set_lines_batch(batch)
                n = o.d.find_device(o.ix, o.ptr, o.n, b"HIT")
                kp, pp = mem.put(b"\0" * 8 * n)
                kl, lp = mem.put(b"\0" * 8 * n)
                assert o.d.find_device(o.ix, o.ptr, o.n, b"HIT", NL, pp, lp, n) == n
                pos = np.frombuffer(mem.get(kp, 8 * n), dtype=np.uint64).astype(np.int64)
                ln = np.frombuffer(mem.get(kl, 8 * n), dtype=np.uint64).astype(np.int64)
                begin, end = o.offsets(ln).astype(np.int64), o.offsets(ln + 1).astype(np.int64)
                assert n > 5 and bool(np.all(begin <= pos)) and bool(np.all(pos < end))
                wanted_lines = [l for l in pl.plain.splitlines(keepends=True) if b"HIT" in l]
                uniq = np.unique(ln)
                got, offs, br = line_cases.read(mem, o, [(k, k + 1) for k in uniq.tolist()], cap=sum(len(l) for l in wanted_lines))
                assert got == b"".join(wanted_lines) and len(wanted_lines) == uniq.size


# ------------------------------------------------------------------------------------------------ 4. capacity
def capacity_text():
    """line_text three times over (27 KiB): with the default batch its hits lie in two pieces of staging, on both sides of
    the first row of the second."""
    return line_text(NL, True)[0] * 3


def piece_caps(starts):
    """Two values of hits_cap that end the writing inside the stream's second piece, from the host's ascending starts of
    the hits; they hold for one batch (the default), where byte p of the stream lies at PAD + p of staging.  The hits in
    front of staging offset T: piece 1's first rank equals the cap, and its workgroup leaves before the walk.  The hits in
    front of T + 4096: the cap is reached when piece 1's first row of 256 words is done, and the walk leaves its loop."""
    caps = [int(np.searchsorted(starts, at - PAD, side="left")) for at in (T, T + 4096)]
    assert 1 < caps[0] < caps[1] < len(starts) - 1, caps
    return caps


def capacity(lib):
    mem = Mem(lib)
    text = capacity_text()
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        pl = Plain(fmt, s)
        for pattern in (b"HIT", b"e"):
            hits, lns = wanted(pl, pattern, NL)
            n = hits.size
            assert n >= 8
            with Opened(lib, mem, fmt, s) as o:
                for batch in (0, 5000):
                    o.d.set_lines_batch(batch)
                    assert o.count(pattern) == n and o.count(pattern, NL) == n
                    assert o.d.find_device(o.ix, o.ptr, o.n, pattern, None, None, None, 3) == n  # (count only: hits_cap is ignored)
                    # (piece_caps: at batch 0 they end the writing inside the second piece -- the workgroup's early return, the walk's
                    # early out; at batch 5000 staging is laid out otherwise and they are two more values)
                    for cap in [n, n + 3, n - 1, 1, 0] + piece_caps(hits):
                        for positions, lines_ in ((True, True), (True, False), (False, True)):
                            got, pos, ln = o.find(pattern, NL, cap, positions, lines_)
                            what = (fmt, pattern, batch, cap, positions, lines_)
                            if cap >= n:
                                assert got == n, what
                            else:
                                assert isinstance(got, _native.GzpxError), what
                                assert (got.code, got.needed) == (_native.ERR_INSUFFICIENT_SPACE, n), what
                            k = min(cap, n)
                            if positions:
                                assert pos[:k].tolist() == hits[:k].tolist(), what
                                assert bool(np.all(pos[k:] == UNTOUCHED[0])), (what, "written behind hits_cap")
                            if lines_:
                                assert ln[:k].tolist() == lns[:k].tolist(), what
                                assert bool(np.all(ln[k:] == UNTOUCHED[0])), (what, "written behind hits_cap")


# ------------------------------------------------------------------------------------------------ 5. errors
def errors(lib):
    mem = Mem(lib)
    text, _ = line_text(NL, True)
    for fmt in (BGZF, MGZIP):
        s = cut(fmt, text, [40, 5000])
        with Opened(lib, mem, fmt, s) as o:
            keep, p = mem.put(bytes([FILL]) * 64)

            def invalid(call):
                with pytest.raises(_native.GzpxError) as e:
                    call()
                assert e.value.code == _native.ERR_INVALID_ARG and e.value.needed is None and e.value.block in (None, 0)
                assert mem.get(keep, 64) == bytes([FILL]) * 64

            invalid(lambda: o.count(b""))
            invalid(lambda: o.count(b"x" * 257))
            invalid(lambda: o.count(b"HIT", 256))
            invalid(lambda: o.count(b"HIT", -2))
            invalid(lambda: o.d.find_device(o.ix, o.ptr, o.n, b"HIT", None, None, p, 8))  # d_lines without a delimiter
            invalid(lambda: o.d.find_device(o.ix, o.ptr, o.n - 1, b"HIT"))                # fewer bytes than the index covers
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:             # another context's index
                invalid(lambda: d2.find_device(o.ix, o.ptr, o.n, b"HIT"))
            assert o.count(b"x" * 256) == 0 and o.count(b"HIT", 255) > 0 and o.count(b"HIT", 0) > 0


def damaged(lib):
    """A damaged member: the inflate's error class and the member's index in the stream (two members a batch), n_hits = 0."""
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        text = short_lines(8 * 10000, 11)
        s = cut(fmt, text, [10000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        keep0, ptr0 = mem.put(s)
        for route in ROUTES:
            with _native.DContext(format=fmt, lib=lib) as d:
                d.set_route(route)
                d.set_lines_batch(22000)
                for victim in (0, 3, 7):
                    for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                           ("block type", pl.off[victim] + HDR[fmt], _native.ERR_BAD_DATA)):
                        m = bytearray(s)
                        if what == "crc":
                            m[at] ^= 0xFF
                        else:
                            m[at] |= 0x06  # BTYPE = 3, reserved
                        keep, ptr = mem.put(m)
                        kp, pp = mem.put(b"\0" * 8 * 64)
                        with d.build_index_device(ptr, len(m)) as ix:
                            with pytest.raises(_native.GzpxError) as e:
                                d.find_device(ix, ptr, len(m), b"e\n", NL, pp, None, 64)
                            assert (e.value.code, e.value.block, e.value.needed) == (code, victim, None), (fmt, route, victim, what)
                            n, info = ctypes.c_uint64(77), _native.GzpxCheckInfo()
                            rc = lib.L.gzpx_find_device(d.h, ix.h, ptr, len(m), b"e", 1, -1, None, None, 0, ctypes.byref(n),
                                                        ctypes.byref(info), None)
                            assert (rc, n.value, info.block) == (code, 0, victim), (fmt, route, victim, what)
                with d.build_index_device(ptr0, len(s)) as ix0:  # the context serves on
                    assert d.find_device(ix0, ptr0, len(s), b"e\n") == wanted(pl, b"e\n", None)[0].size
