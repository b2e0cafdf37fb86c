"""Reads by line (gzpx_dlines_*, gzpx_line_offsets_device, gzpx_read_lines_device), written once and run twice: through
the emulated library on CPU (tests/test_emu_lines.py) and through the real HIP library on the MI355X
(tests/test_gpu_lines.py).

The yardstick is never the library's own inflate.  It is range_cases.Plain: zlib's inflate of every member, joined.  The
delimiter positions come from np.flatnonzero(plain == delim); start(k), P, the tiles, the covers and the members a call
must read (Plain.union of the covers) are computed here from the definitions of include/gzpx.h."""
import numpy as np
import pytest

from gzp_amd import _native, synth
from range_cases import Plain, ROUTES
from scan_cases import BGZF, MGZIP, HDR, Mem, member, our_streams

T = _native.LINES_TILE
DELIMS = (0x0A, 0x00, 0x7F, 0x80, 0xFF, 0x09)
NL = 0x0A


# ------------------------------------------------------------------------------------------------ the yardstick
class Lines:
    """The host's view of a stream's lines for one delimiter byte."""

    def __init__(self, pl, delim):
        a = np.frombuffer(pl.plain, dtype=np.uint8)
        self.pl, self.total = pl, pl.total
        pos = np.flatnonzero(a == delim).astype(np.int64)
        self.D = int(pos.size)
        self.L = self.D if self.total == 0 or a[-1] == delim else self.D + 1
        tail = [self.total] if self.L == self.D + 1 else []
        self.start = np.concatenate([[0], pos + 1, tail]).astype(np.int64)  # start(k), 0 <= k <= L
        self.tiles = -(-self.total // T)
        self.P = np.concatenate([[0], np.cumsum(np.bincount(pos // T, minlength=self.tiles))]).astype(np.int64)
        assert self.P.size == self.tiles + 1 and self.P[-1] == self.D

    def tile(self, k):
        """The t with P[t] < k <= P[t + 1], for 1 <= k <= D."""
        assert 1 <= k <= self.D
        t = int(np.searchsorted(self.P[1:], k, side="left"))
        assert self.P[t] < k <= self.P[t + 1]
        return t

    def tile_cover(self, k):
        """What line_offsets_device has to inflate for boundary k: its own tile, or nothing."""
        if k == 0 or k > self.D:
            return (0, 0)
        t = self.tile(k)
        return (T * t, min(T * (t + 1), self.total))

    def cover(self, a, b):
        """What read_lines_device has to inflate for the line range [a, b)."""
        if a >= b:
            return (0, 0)
        return (0 if a == 0 else T * self.tile(a), self.total if b > self.D else min(T * (self.tile(b) + 1), self.total))

    def byte_range(self, a, b):
        return (int(self.start[a]), int(self.start[b])) if a < b else (0, 0)  # (an empty range is reported as (0, 0))

    def expected(self, ranges):
        return b"".join(self.pl.plain[int(self.start[a]):int(self.start[b])] for a, b in ranges)


# ------------------------------------------------------------------------------------------------ streams
def cut(fmt, data, cuts, level=1, eof=False):
    """`data` as members that end at the bytes of `cuts` (a repeated cut: an empty member), then at its end."""
    edges = [0] + sorted(cuts) + [len(data)]
    s = b"".join(member(fmt, data[b:e], level) for b, e in zip(edges[:-1], edges[1:]))
    return s + (member(BGZF, b"", level) if eof else b"")


def short_lines(n, seed, delim=NL):
    """n bytes of lines of 0..120 letters."""
    rng = np.random.default_rng(seed)
    a = rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8)
    at = np.cumsum(rng.integers(1, 122, n // 40 + 2))
    a[at[at < n]] = delim
    return a.tobytes()


def crafted_text(end_with_delim=True):
    """Empty lines as runs of delimiters, a line longer than a tile, a line that spans four members of crafted_cuts(), a
    delimiter as the first and as the last byte of the stream's first two tiles (crafted_cuts() makes them the last and
    the first byte of members too)."""
    body = bytearray(b"\n" + short_lines(2 * T + 99, 1))
    for p in (T - 1, T, 2 * T - 1, 2 * T):
        body[p] = NL
    body += b"\n" * 50
    body += b"A" * 20000 + b"\n"
    body += short_lines(8000, 2) + b"\n\n\n"
    long_at = len(body)
    body += b"B" * 30000 + b"\n"
    body += short_lines(5000, 3)
    body[-1] = NL if end_with_delim else ord("z")
    return bytes(body), long_at


def crafted_cuts(long_at):
    # (T twice: an empty member between a member that ends with a delimiter and one that starts with one)
    return [5000, T, T, 2 * T, 2 * T + 60, 2 * T + 60, 2 * T + 60, long_at - 10, long_at + 9000, long_at + 18000, long_at + 27000]


_cache = {}


def streams(oracle):
    """[(name, format, stream, Plain)] of every newline-delimited stream of the issue's list; made once a session."""
    if "text" in _cache:
        return _cache["text"]
    out = []
    text, long_at = crafted_text()
    bare, _ = crafted_text(end_with_delim=False)
    assert text[:-1] == bare[:-1] and text[-1] == NL != bare[-1]
    for fmt in (BGZF, MGZIP):
        f = "bgzf" if fmt == BGZF else "mgzip"
        out.append((f + " crafted", fmt, cut(fmt, text, crafted_cuts(long_at))))
        out.append((f + " crafted, unterminated", fmt, cut(fmt, bare, crafted_cuts(long_at), level=3)))
        out.append((f + " no delimiter", fmt, cut(fmt, b"x" * 40000, [3, 20000])))
        out.append((f + " delimiters only", fmt, cut(fmt, b"\n" * 40000, [1, T, 30000])))
        out.append((f + " no member", fmt, b""))
        out.append((f + " empty members only", fmt, cut(fmt, b"", [0])))
        for n in (1, T - 1, T, T + 1):
            out.append((f + " %d bytes" % n, fmt, cut(fmt, text[:n], [n // 2] if n > 1 else [])))
        three = short_lines(3 * T + 123, 4)
        out.append((f + " members of 5,000 bytes", fmt, cut(fmt, three, list(range(5000, len(three), 5000)))))
    out.append(("bgzf crafted + EOF", BGZF, cut(BGZF, text, crafted_cuts(long_at), eof=True)))
    big = synth.make("text", 250000, 5).tobytes()
    out.append(("mgzip members of 100 KB", MGZIP, cut(MGZIP, big, [100000, 200000])))
    out.append(("mgzip one member of 150 KB", MGZIP, cut(MGZIP, synth.make("fastq", 150000, 6).tobytes(), [])))
    for name, fmt, s, a in our_streams(oracle, classes=("fastq", "text"), levels=(1,)):
        if "bs=1048576" not in name and " n=0 " not in name and " n=1 " not in name and not (" n=65280 " in name and "no-eof" in name):
            out.append((name, fmt, s))
    out = [(name, fmt, s, Plain(fmt, s)) for name, fmt, s in out]
    for name, fmt, s, pl in out:
        assert pl.consumed == len(s) and pl.total <= 300000, name
    crafted = out[0][3]
    assert crafted.plain == text and crafted.isize.count(0) == 3
    assert len(crafted.union([(long_at, long_at + 30001)])) >= 3 and 20000 > T  # the two long lines
    _cache["text"] = out
    return out


def binary_streams():
    """Random bytes for the delimiters that text does not hold: every byte value about once in 256 bytes."""
    if "binary" not in _cache:
        a = synth.make("random", 3 * T + 5, 9).tobytes()
        _cache["binary"] = [(name, fmt, s, Plain(fmt, s)) for name, fmt, s in
                            (("bgzf random", BGZF, cut(BGZF, a, [7000, T - 1, T - 1, 2 * T + 1])),
                             ("mgzip random", MGZIP, cut(MGZIP, a, [T, 40000])))]
    return _cache["binary"]


class Opened:
    """A stream in device memory with its context, index and line table."""

    def __init__(self, lib, mem, fmt, s, delim=NL, route=ROUTES[0], batch=0, shift=0):
        self.keep, self.ptr = mem.put(s, shift=shift)
        self.n = len(s)
        self.d = _native.DContext(format=fmt, lib=lib)
        self.d.set_route(route)
        self.d.set_lines_batch(batch)
        self.ix = self.d.build_index_device(self.ptr, self.n)
        self.lt = self.d.build_lines_device(self.ix, self.ptr, self.n, delim)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lt.close()
        self.ix.close()
        self.d.close()

    def offsets(self, ks):
        return self.d.line_offsets_device(self.ix, self.lt, self.ptr, self.n, ks)


def check_table(o, ln, what):
    assert (o.lt.n_delims, o.lt.n_lines) == (ln.D, ln.L), what
    assert o.lt.prefix().tolist() == ln.P.tolist(), what


# ------------------------------------------------------------------------------------------------ 1. the table
def table(lib, oracle):
    """P, D and L against the host's: every stream on both routes and with batches that split tiles; the delimiters that
    the zero-byte test could get wrong on random bytes."""
    mem = Mem(lib)
    for i, (name, fmt, s, pl) in enumerate(streams(oracle)):
        ln = Lines(pl, NL)
        for route, batch in ((ROUTES[0], 0), (ROUTES[1], 0), (ROUTES[0], 1), (ROUTES[1], 20000), (ROUTES[0], 70000)):
            with Opened(lib, mem, fmt, s, NL, route, batch, shift=i % 16) as o:
                check_table(o, ln, (name, route, batch))
                inflate_ms, count_ms = o.d.last_lines_build_ms()
                assert inflate_ms >= 0.0 and count_ms >= 0.0
    for name, fmt, s, pl in binary_streams() + streams(oracle)[:2]:
        for delim in DELIMS:
            ln = Lines(pl, delim)
            assert ln.D > 100 or "crafted" in name
            for route, batch in ((ROUTES[0], 0), (ROUTES[1], 1), (ROUTES[0], 20000), (ROUTES[1], 70000)):
                with Opened(lib, mem, fmt, s, delim, route, batch) as o:
                    check_table(o, ln, (name, delim, route, batch))


# ------------------------------------------------------------------------------------------------ 2. offsets
def pick_lines(ln, seed):
    if ln.L <= 3000:
        return list(range(ln.L + 1))
    rng = np.random.default_rng(seed)
    return [0, ln.L, ln.D, 1] + rng.integers(0, ln.L + 1, 300).tolist()


def offsets(lib, oracle):
    mem = Mem(lib)
    for i, (name, fmt, s, pl) in enumerate(streams(oracle)):
        ln = Lines(pl, NL)
        ks = pick_lines(ln, 100 + i)
        with Opened(lib, mem, fmt, s, shift=(3 * i) % 16) as o:
            assert o.offsets(ks).tolist() == ln.start[ks].tolist(), name
            assert o.d.last_lines_members() == len(pl.union([ln.tile_cover(k) for k in ks])), name
            assert all(t >= 0.0 for t in o.d.last_lines_ms())
            assert o.offsets([]).size == 0 and o.d.last_lines_members() == 0
            few = ks[::97]  # a few boundaries: most members stay untouched
            assert o.offsets(few).tolist() == ln.start[few].tolist(), name
            assert o.d.last_lines_members() == len(pl.union([ln.tile_cover(k) for k in few])), name
            for bad in ([ln.L + 1], [0, ln.L, ln.L + 7, 1, ln.L + 1], [1 << 63]):
                with pytest.raises(_native.GzpxError) as e:
                    o.offsets(bad)
                assert (e.value.code, e.value.range_index) == (_native.ERR_INVALID_ARG, 2 if len(bad) > 1 else 0), name
                assert o.d.last_lines_members() == 0
    for name, fmt, s, pl in binary_streams():  # another delimiter through the search
        ln = Lines(pl, 0x80)
        with Opened(lib, mem, fmt, s, 0x80, ROUTES[1]) as o:
            assert o.offsets(range(ln.L + 1)).tolist() == ln.start.tolist(), name


# ------------------------------------------------------------------------------------------------ 3. reads
def range_set(ln, seed):
    """The line ranges of the issue's list."""
    L = ln.L
    rng = np.random.default_rng(seed)
    r = [(k, k + 1) for k in range(L)] if L <= 3000 else []
    r += [(0, L)]
    r += [(0, 0), (L // 2, L // 2), (L, L)]  # empty: at 0, in the middle, at L
    if L:
        a, b = L // 3, min(L // 3 + 40, L)
        r += [(a, b), (a, b), (a, b), (max(a - 5, 0), min(a + 5, L)), (a + (b - a) // 2, min(b + 9, L))]  # duplicates, overlaps
        r += [(4 * i, min(4 * i + 4, L)) for i in range(0, -(-L // 4), max(L // 800, 1))]  # FASTQ records
        for _ in range(300):  # log-uniform line counts
            n = min(int(np.exp(rng.uniform(0, np.log(L + 1)))), L)
            a = int(rng.integers(0, L - n + 1))
            r.append((a, a + n))
    return r


def read(mem, o, ranges, cap=None, fill=0xEE):
    """One gzpx_read_lines_device into an output misaligned by 3 with guard bytes behind it:
    (bytes returned, out_offsets, byte_ranges)."""
    room = (cap if cap is not None else 0) + 64
    keep, p = mem.put(bytes([fill]) * room, shift=3)
    out_len, offs, br = o.d.read_lines_device(o.ix, o.lt, o.ptr, o.n, np.array(ranges, dtype=np.uint64).reshape(-1, 2), p, cap)
    whole = mem.get(keep, room + 3)[3:]
    assert whole[out_len:] == bytes([fill]) * (room - out_len), "bytes written behind the output"
    return whole[:out_len], offs.tolist(), br.tolist()


def check_read(mem, o, ln, ranges, what):
    want = [ln.byte_range(a, b) for a, b in ranges]
    lens = [e - b for b, e in want]
    got, offs, br = read(mem, o, ranges, cap=sum(lens))
    assert br == [list(x) for x in want], (what, "byte_ranges")
    assert offs == [0] + np.cumsum(lens).tolist(), (what, "out_offsets")
    assert got == ln.expected(ranges), (what, "bytes")
    assert o.d.last_lines_members() == len(ln.pl.union([ln.cover(a, b) for a, b in ranges])), (what, "members read")


def reads(lib, oracle):
    mem = Mem(lib)
    for i, (name, fmt, s, pl) in enumerate(streams(oracle)):
        ln = Lines(pl, NL)
        rs = range_set(ln, 1000 + i)
        shuffled = [rs[j] for j in np.random.default_rng(i).permutation(len(rs))]
        few = [r for r in rs[::11] if r[1] - r[0] < 30]  # short ranges only: most members stay untouched
        with Opened(lib, mem, fmt, s, shift=(5 * i) % 16) as o:
            check_read(mem, o, ln, rs, (name, "all"))
            assert all(t >= 0.0 for t in o.d.last_lines_ms())
            check_read(mem, o, ln, few, (name, "few"))
            if i % 3 == 0:  # the output follows the order given
                check_read(mem, o, ln, shuffled, (name, "shuffled"))
            check_read(mem, o, ln, [(0, ln.L)], (name, "whole"))
            check_read(mem, o, ln, [(ln.L, ln.L)], (name, "empty"))
            assert read(mem, o, [], cap=0) == (b"", [0], [])
        with Opened(lib, mem, fmt, s, route=ROUTES[1], shift=(7 * i) % 16) as o:  # the other inflate route
            check_read(mem, o, ln, rs if "crafted" in name else [(0, ln.L)], (name, ROUTES[1], "all"))
            check_read(mem, o, ln, few, (name, ROUTES[1], "few"))
    for name, fmt, s, pl in binary_streams():
        ln = Lines(pl, 0xFF)
        with Opened(lib, mem, fmt, s, 0xFF) as o:
            check_read(mem, o, ln, range_set(ln, 7), (name, "0xFF"))


# ------------------------------------------------------------------------------------------------ 4. errors
def errors(lib, oracle):
    mem = Mem(lib)
    all_streams = streams(oracle)
    for name, fmt, s, pl in all_streams[:2] + [x for x in all_streams if x[0] == "mgzip crafted"]:
        ln = Lines(pl, NL)
        L = ln.L
        with Opened(lib, mem, fmt, s) as o:
            good = [(0, 2), (L - 2, L), (5, 5)]
            for what, r, at in (("b = L + 1", [(L - 1, L + 1)], 3), ("a > b", [(11, 10)], 3), ("both", [(L, L + 1), (7, 2)], 3),
                                ("first", None, 0), ("beyond", [(L + 1, L + 1)], 3), ("huge", [(0, 1 << 63)], 3)):
                rs = good + r + good if r else [(L + 5, L + 6)] + good
                cap = 4096
                keep, p = mem.put(b"\xEE" * cap)
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_lines_device(o.ix, o.lt, o.ptr, o.n, np.array(rs, dtype=np.uint64), p, cap)
                assert (e.value.code, e.value.range_index) == (_native.ERR_INVALID_ARG, at), (name, what)
                assert mem.get(keep, cap) == b"\xEE" * cap, (name, what, "output written")
                assert o.d.last_lines_members() == 0
            # an output that is too small: the size needed, nothing written
            rs = [(0, L), (L // 2, L)]
            need = ln.total + ln.total - int(ln.start[L // 2])
            for cap in (0, 1, need - 1):
                keep, p = mem.put(b"\xEE" * (need + 64))
                with pytest.raises(_native.GzpxError) as e:
                    o.d.read_lines_device(o.ix, o.lt, o.ptr, o.n, np.array(rs, dtype=np.uint64), p, cap)
                assert (e.value.code, e.value.needed) == (_native.ERR_INSUFFICIENT_SPACE, need), (name, cap)
                assert mem.get(keep, need + 64) == b"\xEE" * (need + 64), (name, cap, "output written")
            assert read(mem, o, rs, cap=need)[0] == ln.expected(rs)
            # fewer bytes than the index covers
            with pytest.raises(_native.GzpxError) as e:
                o.d.line_offsets_device(o.ix, o.lt, o.ptr, o.n - 1, [1])
            assert e.value.code == _native.ERR_INVALID_ARG and e.value.range_index is None
            # delim = 256
            with pytest.raises(_native.GzpxError) as e:
                o.d.build_lines_device(o.ix, o.ptr, o.n, 256)
            assert e.value.code == _native.ERR_INVALID_ARG
            # the table with the index of another stream, and with another context
            other = next(x for x in all_streams if x[1] == fmt and x[0].endswith("members of 5,000 bytes"))
            keep2, ptr2 = mem.put(other[2])
            with o.d.build_index_device(ptr2, len(other[2])) as ix2:
                for call in (lambda: o.d.line_offsets_device(ix2, o.lt, ptr2, len(other[2]), [1]),
                             lambda: o.d.read_lines_device(ix2, o.lt, ptr2, len(other[2]), [(0, 1)], o.ptr, 0)):
                    with pytest.raises(_native.GzpxError) as e:
                        call()
                    assert e.value.code == _native.ERR_INVALID_ARG and e.value.range_index is None, name
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    d2.line_offsets_device(o.ix, o.lt, o.ptr, o.n, [1])
                assert e.value.code == _native.ERR_INVALID_ARG
                with pytest.raises(_native.GzpxError) as e:
                    d2.build_lines_device(o.ix, o.ptr, o.n)
                assert e.value.code == _native.ERR_INVALID_ARG


def touched(lib):
    """Damage in a member no cover needs is never seen by a search; in one that is needed it is reported with the member's
    index in the stream; a build sees every member and returns no table."""
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        text = short_lines(8 * 20000, 11)
        s = cut(fmt, text, [20000 * i for i in range(1, 8)])
        pl = Plain(fmt, s)
        ln = Lines(pl, NL)
        hdr = HDR[fmt]
        k3 = int(np.searchsorted(ln.start, 3 * 20000 + 9000))  # a line that starts in the middle of member 3
        rs = [(k3, k3 + 5), (ln.L - 3, ln.L)]
        needed = sorted(pl.union([ln.cover(a, b) for a, b in rs]))
        assert needed in ([3, 7], [2, 3, 7], [3, 4, 7]) and 0 not in needed and 5 not in needed
        keep0, ptr0 = mem.put(s)
        for route in ROUTES:
            with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr0, len(s)) as ix0, \
                    d.build_lines_device(ix0, ptr0, len(s)) as lt:  # the table of the undamaged stream
                d.set_route(route)
                d.set_lines_batch(45000)  # (two members a batch: the index in the stream is not the one in the batch)
                for victim in range(pl.n):
                    for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                           ("block type", pl.off[victim] + hdr, _native.ERR_BAD_DATA)):
                        m = bytearray(s)
                        if what == "crc":
                            m[at] ^= 0xFF
                        else:
                            m[at] |= 0x06  # BTYPE = 3, reserved
                        keep, ptr = mem.put(m)
                        with d.build_index_device(ptr, len(m)) as ix:  # (the members' extents are the same: the table serves)
                            if victim in (0, 3, 6):  # a build over a damaged stream: the error, no table
                                with pytest.raises(_native.GzpxError) as e:
                                    d.build_lines_device(ix, ptr, len(m))
                                assert (e.value.code, e.value.block) == (code, victim), (fmt, route, victim, what, "build")
                            o = type("O", (), dict(d=d, ix=ix, lt=lt, ptr=ptr, n=len(m)))
                            if victim in needed:
                                with pytest.raises(_native.GzpxError) as e:
                                    read(mem, o, rs, cap=4096)
                                assert (e.value.code, e.value.block) == (code, victim), (fmt, route, victim, what)
                                assert e.value.range_index is None
                            else:
                                check_read(mem, o, ln, rs, (fmt, route, victim, what))
                                ks = [k3, ln.L - 1]
                                got = d.line_offsets_device(ix, lt, ptr, len(m), ks)
                                assert got.tolist() == ln.start[ks].tolist()
