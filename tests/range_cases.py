"""Random-access reads by range (gzpx_dindex_*, gzpx_read_ranges_device), written once and run twice: through the
emulated library on CPU (tests/test_emu_ranges.py) and through the real HIP library on the MI355X
(tests/test_gpu_ranges.py).

The yardstick is the same everywhere: every member of the stream is inflated on the CPU with zlib and the results are
joined; a read must return the concatenation of plain[begin:end] over its ranges, in the order given.  Virtual offsets
are resolved with a host table of member starts.  The library's own full inflate is never the yardstick."""
import bisect
import ctypes
import struct
import zlib

import numpy as np
import pytest

from gzp_amd import _native, synth
from inflate_cases import SEG_BIG_BYTES
from scan_cases import BGZF, MGZIP, HDR, EOF, Mem, member, our_streams

ROUTES = (_native.INFLATE_SEG, _native.INFLATE_WAVE)


# ------------------------------------------------------------------------------------------------ the yardstick
class Plain:
    """The host's view of a stream: member starts and sizes from the headers, every member inflated with zlib."""

    def __init__(self, fmt, s):
        s = bytes(s)
        self.off, self.size, parts = [], [], []
        pos = 0
        while len(s) - pos >= HDR[fmt]:
            size = (struct.unpack_from("<H", s, pos + 16)[0] + 1 if fmt == BGZF else struct.unpack_from("<I", s, pos + 16)[0])
            if len(s) - pos < size:
                break
            parts.append(zlib.decompress(s[pos + HDR[fmt]:pos + size - 8], -15))
            assert len(parts[-1]) == struct.unpack_from("<I", s, pos + size - 4)[0]
            self.off.append(pos)
            self.size.append(size)
            pos += size
        self.consumed = pos
        self.n = len(self.off)
        self.isize = [len(p) for p in parts]
        self.ustart = [0]
        for p in parts:
            self.ustart.append(self.ustart[-1] + len(p))
        self.total = self.ustart[-1]
        self.plain = b"".join(parts)

    def expected(self, ranges):
        return b"".join(self.plain[b:e] for b, e in ranges)

    def union(self, ranges):
        """The members a read must touch: [first, last] of every non-empty range, first = the last member whose
        uncompressed start is <= begin, last = the last member whose uncompressed start is < end."""
        hit = set()
        starts = self.ustart[:self.n]
        for b, e in ranges:
            if e > b:
                hit.update(range(bisect.bisect_right(starts, b) - 1, bisect.bisect_left(starts, e)))
        return hit

    def virtual_forms(self, p):
        """Every BGZF virtual offset that names position p of the inflated stream (two at a member boundary, more
        around empty members), in stream order."""
        return [(self.off[m] << 16) | (p - self.ustart[m]) for m in range(self.n)
                if 0 <= p - self.ustart[m] <= self.isize[m]]


def range_set(pl, seed):
    """The ranges of the issue's list over a stream of pl.total bytes."""
    t = pl.total
    rng = np.random.default_rng(seed)
    r = []
    for u in pl.ustart:  # every single-byte range around every member boundary
        r += [(p, p + 1) for p in range(u - 2, u + 2) if 0 <= p < t]
    for i, u in enumerate(pl.ustart):  # ranges that start or end exactly on boundaries
        r += [(max(u - 5, 0), u), (u, min(u + 7, t)), (u, pl.ustart[min(i + 2, pl.n)]), (pl.ustart[max(i - 1, 0)], u)]
    r += [(0, t)]                            # the whole stream
    r += [(0, 0), (t // 2, t // 2), (t, t)]  # empty: at 0, in the middle, at inflated_len
    if t:
        a, b = t // 3, min(t // 3 + 1000, t)
        r += [(a, b), (a, b), (a, b), (max(a - 100, 0), min(a + 100, t)), (a + (b - a) // 2, min(b + 50, t))]  # duplicates, overlaps
        for _ in range(300):  # log-uniform lengths
            n = min(int(np.exp(rng.uniform(0, np.log(t + 1)))), t)
            b = int(rng.integers(0, t - n + 1))
            r.append((b, b + n))
    return r


def read(mem, d, ix, ptr, in_len, ranges, coords="uncompressed", cap=None, fill=0xEE):
    """One gzpx_read_ranges_device: (bytes returned, out_offsets, the whole output buffer afterwards)."""
    want = sum(max(int(e) - int(b), 0) for b, e in ranges) if coords == "uncompressed" else cap
    cap = want if cap is None else cap
    room = cap + 64
    keep, p = mem.put(bytes([fill]) * room, shift=3)  # (an output that does not start on a 16-byte boundary)
    out_len, offs = d.read_ranges_device(ix, ptr, in_len, np.array(ranges, dtype=np.uint64).reshape(-1, 2), p, cap, coords)
    whole = mem.get(keep, room + 3)[3:]
    assert whole[out_len:] == bytes([fill]) * (room - out_len), "bytes written behind the output"
    return whole[:out_len], offs.tolist()


def check_read(mem, d, ix, pl, ptr, in_len, ranges, what):
    got, offs = read(mem, d, ix, ptr, in_len, ranges)
    lens = [e - b for b, e in ranges]
    assert offs == [0] + np.cumsum(lens).tolist(), (what, "out_offsets")
    assert got == pl.expected(ranges), (what, "bytes")
    assert d.last_ranges_members() == len(pl.union(ranges)), (what, "members read")


# ------------------------------------------------------------------------------------------------ streams
def zlib_streams():
    """(name, format, stream) of zlib-made streams of uneven members, with empty members in the middle."""
    for fmt in (BGZF, MGZIP):
        for level in (1, 3):
            sizes = (3000, 0, 17, 40000, 0, 0, 1, 65000 if fmt == BGZF else 150000, 2500)
            chunks = [synth.make(("text", "dna", "random", "fastq")[i % 4], n, i + level).tobytes() for i, n in enumerate(sizes)]
            yield "zlib %d l%d" % (fmt, level), fmt, b"".join(member(fmt, c, level) for c in chunks)


def oracle_streams(oracle):
    for name, fmt, s, a in our_streams(oracle, classes=("mixed",), levels=(1, 3)):
        if "bs=1048576" in name or " n=0 " in name or " n=1 " in name:
            continue
        yield name, fmt, s


# ------------------------------------------------------------------------------------------------ 1. the index
def index(lib, oracle):
    mem = Mem(lib)
    seen = 0
    for name, fmt, s in list(oracle_streams(oracle)) + list(zlib_streams()):
        pl = Plain(fmt, s)
        keep, ptr = mem.put(s, shift=seen % 16)
        with _native.DContext(format=fmt, lib=lib) as d:
            want, wused, wtotal = d.index_device(ptr, len(s))
            with d.build_index_device(ptr, len(s)) as ix:
                assert (ix.n_members, ix.consumed, ix.inflated_len) == (want.shape[0], wused, wtotal), name
                assert ix.entries().tolist() == want.tolist(), name
                assert ix.entries().tolist() == [[o, u] for o, u in zip(pl.off, pl.ustart)], name
                assert (ix.consumed, ix.inflated_len) == (pl.consumed, pl.total), name
                few = np.zeros((2, 2), dtype=np.uint64)  # a capped entries array: the count is still the whole stream's
                cnt = ctypes.c_size_t(0)
                lib.check(lib.L.gzpx_dindex_entries(ix.h, few.ctypes.data, 2, ctypes.byref(cnt)))
                assert cnt.value == want.shape[0] and few[:cnt.value].tolist() == want[:2].tolist()
            # a truncated last member is left out, as by gzpx_index_device
            cut = pl.off[-2] + pl.size[-2] // 2 if pl.n >= 2 else 5
            want, wused, wtotal = d.index_device(ptr, cut)
            with d.build_index_device(ptr, cut) as ix:
                assert (ix.n_members, ix.consumed, ix.inflated_len) == (want.shape[0], wused, wtotal), name
                assert ix.entries().tolist() == want.tolist() and ix.n_members == max(pl.n - 2, 0), name
            # an invalid header: the same error
            if pl.n >= 2:
                bad = bytearray(s)
                bad[pl.off[1] + 12] ^= 1
                keep2, ptr2 = mem.put(bad)
                for call in (d.index_device, d.build_index_device):
                    with pytest.raises(_native.GzpxError) as e:
                        call(ptr2, len(bad))
                    assert e.value.code == _native.ERR_INVALID_HEADER, name
        seen += 1
    assert seen >= 10


def empty_stream(lib):
    """An index of nothing is valid: 0 members, every non-empty range is out of bounds."""
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        keep, ptr = mem.put(b"\0" * 64)
        for n in (0, 5):
            with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, n) as ix:
                assert (ix.n_members, ix.consumed, ix.inflated_len) == (0, 0, 0) and ix.entries().shape[0] == 0
                assert read(mem, d, ix, ptr, n, [(0, 0), (0, 0)]) == (b"", [0, 0, 0])
                assert read(mem, d, ix, ptr, n, []) == (b"", [0])
                with pytest.raises(_native.GzpxError) as e:
                    read(mem, d, ix, ptr, n, [(0, 0), (0, 1)])
                assert (e.value.code, e.value.range_index) == (_native.ERR_INVALID_ARG, 1)
                assert d.last_ranges_members() == 0


# ------------------------------------------------------------------------------------------------ 2. ranges
def ranges(lib, oracle, streams=None):
    mem = Mem(lib)
    seen = 0
    for name, fmt, s in (streams or list(oracle_streams(oracle)) + list(zlib_streams())):
        pl = Plain(fmt, s)
        assert pl.consumed == len(s)
        keep, ptr = mem.put(s, shift=(5 * seen) % 16)
        rs = range_set(pl, seed=1000 + seen)
        shuffled = [rs[i] for i in np.random.default_rng(seen).permutation(len(rs))]
        few = [r for r in rs[::7] if r[1] - r[0] < 3000]  # short ranges only: most members stay untouched
        for route in ROUTES:
            with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(s)) as ix:
                d.set_route(route)
                check_read(mem, d, ix, pl, ptr, len(s), rs, (name, route, "all"))
                assert all(t >= 0.0 for t in d.last_ranges_ms())
                check_read(mem, d, ix, pl, ptr, len(s), few, (name, route, "few"))
                if route == ROUTES[0]:  # the output follows the order given
                    check_read(mem, d, ix, pl, ptr, len(s), shuffled, (name, route, "shuffled"))
                    check_read(mem, d, ix, pl, ptr, len(s), [(0, pl.total)], (name, route, "whole"))
                    check_read(mem, d, ix, pl, ptr, len(s), [(pl.total, pl.total)], (name, route, "empty"))
        seen += 1
    assert seen >= 10 or streams


# ------------------------------------------------------------------------------------------------ 3. virtual offsets
def virtual(lib, oracle):
    mem = Mem(lib)
    seen = 0
    for name, fmt, s in list(oracle_streams(oracle)) + list(zlib_streams()):
        pl = Plain(fmt, s)
        keep, ptr = mem.put(s, shift=seen % 16)
        if fmt == MGZIP:  # BGZF only
            with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(s)) as ix:
                with pytest.raises(_native.GzpxError) as e:
                    read(mem, d, ix, ptr, len(s), [(0, 0)], coords="virtual", cap=64)
                assert e.value.code == _native.ERR_INVALID_ARG and e.value.range_index is None, name
            continue
        rng = np.random.default_rng(77 + seen)
        rs = range_set(pl, seed=2000 + seen)
        vr = []
        for b, e in rs:  # the same slices as virtual offsets, every form of a boundary position in turn
            ve = pl.virtual_forms(e)
            v_end = ve[int(rng.integers(0, len(ve)))]
            vb = [v for v in pl.virtual_forms(b) if v <= v_end]
            vr.append((vb[int(rng.integers(0, len(vb)))], v_end))
        last = pl.n - 1
        forms = [((pl.off[m] << 16) | pl.isize[m], (pl.off[m + 1] << 16) | min(9, pl.isize[m + 1])) for m in range(last)]
        forms += [((pl.off[m] << 16) | max(pl.isize[m] - 9, 0), (pl.off[m] << 16) | pl.isize[m]) for m in range(pl.n)]
        want_forms = b"".join(pl.plain[pl.ustart[m + 1]:pl.ustart[m + 1] + min(9, pl.isize[m + 1])] for m in range(last))
        want_forms += b"".join(pl.plain[pl.ustart[m] + max(pl.isize[m] - 9, 0):pl.ustart[m + 1]] for m in range(pl.n))
        total = sum(e - b for b, e in rs)
        with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(s)) as ix:
            got, offs = read(mem, d, ix, ptr, len(s), vr, coords="virtual", cap=total)
            assert got == pl.expected(rs), name
            assert offs == [0] + np.cumsum([e - b for b, e in rs]).tolist(), name
            assert d.last_ranges_members() == len(pl.union(rs)), name
            got, offs = read(mem, d, ix, ptr, len(s), forms, coords="virtual", cap=len(want_forms))
            assert got == want_forms, (name, "offset == ISIZE forms")
            seen += 1
            if last == 0:  # (a single member: the rejections below need a neighbour)
                continue
            # rejected, with the first offender's index; nothing is written
            m = next(i for i in range(last) if pl.isize[i])
            ok = ((pl.off[m] << 16) | 0, (pl.off[m] << 16) | 1)
            bad = {"not a member start": (((pl.off[m] + 1) << 16), ((pl.off[m] + 1) << 16)),
                   "end not a member start": (ok[0], ((pl.off[m + 1] - 1) << 16)),
                   "behind the last member": ((len(s) << 16), (len(s) << 16)),
                   "lower part above ISIZE": (ok[0], (pl.off[m] << 16) | (pl.isize[m] + 1)),
                   "begin above ISIZE": ((pl.off[m] << 16) | (pl.isize[m] + 1), (pl.off[m + 1] << 16)),
                   "begin behind end": ((pl.off[m] << 16) | 1, (pl.off[m] << 16) | 0),
                   "begin behind end, same position": ((pl.off[m + 1] << 16), (pl.off[m] << 16) | pl.isize[m])}
            for what, r in bad.items():
                with pytest.raises(_native.GzpxError) as e:
                    read(mem, d, ix, ptr, len(s), [ok, ok, r, ok, r], coords="virtual", cap=64)
                assert (e.value.code, e.value.range_index) == (_native.ERR_INVALID_ARG, 2), (name, what)
    assert seen >= 10


# ------------------------------------------------------------------------------------------------ 4. errors
def errors(lib):
    mem = Mem(lib)
    for name, fmt, s in zlib_streams():
        pl = Plain(fmt, s)
        keep, ptr = mem.put(s)
        t = pl.total
        with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(s)) as ix:
            good = [(0, 10), (t - 10, t), (5, 5)]
            for what, r, at in (("end > inflated_len", [(t - 1, t + 1)], 3), ("begin > end", [(11, 10)], 3),
                                ("both", [(t, t + 1), (7, 2)], 3), ("first", None, 0), ("beyond", [(t + 1, t + 1)], 3),
                                ("huge", [(0, 1 << 63)], 3)):
                rs = good + r + good if r else [(t + 5, t + 6)] + good
                cap = 4096
                keep2, p = mem.put(b"\xEE" * cap)
                with pytest.raises(_native.GzpxError) as e:
                    d.read_ranges_device(ix, ptr, len(s), np.array(rs, dtype=np.uint64), p, cap)
                assert (e.value.code, e.value.range_index) == (_native.ERR_INVALID_ARG, at), (name, what)
                assert mem.get(keep2, cap) == b"\xEE" * cap, (name, what, "output written")
                assert d.last_ranges_members() == 0
            # an output that is too small: the size needed, nothing written
            rs = [(0, t), (t // 2, t)]
            need = t + t - t // 2
            for cap in (0, 1, need - 1):
                keep2, p = mem.put(b"\xEE" * (need + 64))
                with pytest.raises(_native.GzpxError) as e:
                    d.read_ranges_device(ix, ptr, len(s), np.array(rs, dtype=np.uint64), p, cap)
                assert (e.value.code, e.value.needed) == (_native.ERR_INSUFFICIENT_SPACE, need), (name, cap)
                assert mem.get(keep2, need + 64) == b"\xEE" * (need + 64), (name, cap, "output written")
            assert read(mem, d, ix, ptr, len(s), rs, cap=need)[0] == pl.expected(rs)
            # fewer bytes than the index covers; another context's index
            with pytest.raises(_native.GzpxError) as e:
                read(mem, d, ix, ptr, len(s) - 1, [(0, 1)])
            assert e.value.code == _native.ERR_INVALID_ARG and e.value.range_index is None
            with _native.DContext(format=BGZF + MGZIP - fmt, lib=lib) as d2:
                with pytest.raises(_native.GzpxError) as e:
                    read(mem, d2, ix, ptr, len(s), [(0, 1)])
                assert e.value.code == _native.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ 5. only what is needed
def touched(lib):
    """Damage in a member no range needs is never seen; in one that is needed it is reported with the member's index in
    the stream."""
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        chunks = [synth.make(("text", "dna", "fastq")[i % 3], 9000 + 1000 * i, i).tobytes() for i in range(8)]
        s = b"".join(member(fmt, c, 1 + 2 * (i % 2)) for i, c in enumerate(chunks))
        pl = Plain(fmt, s)
        u = pl.ustart
        rs = [(u[1] + 10, u[3] - 10), (u[5] + 1, u[5] + 2), (u[2], u[2] + 5), (u[5] + 100, u[6])]
        assert pl.union(rs) == {1, 2, 5}
        hdr = HDR[fmt]
        for route in ROUTES:
            for victim in (0, 3, 4, 6, 7):  # not needed: payload, CRC and a reserved block type
                for at, flip in ((pl.off[victim] + hdr + 40, 0x5A), (pl.off[victim] + pl.size[victim] - 8, 0xFF),
                                 (pl.off[victim] + hdr, 0x06)):
                    m = bytearray(s)
                    m[at] = m[at] | 0x06 if flip == 0x06 else m[at] ^ flip
                    keep, ptr = mem.put(m)
                    with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(m)) as ix:
                        d.set_route(route)
                        check_read(mem, d, ix, pl, ptr, len(m), rs, (fmt, route, victim, at))
            for victim in (1, 2, 5):  # needed
                for what, at, code in (("crc", pl.off[victim] + pl.size[victim] - 8, _native.ERR_INVALID_CHECK),
                                       ("block type", pl.off[victim] + hdr, _native.ERR_BAD_DATA)):
                    m = bytearray(s)
                    if what == "crc":
                        m[at] ^= 0xFF
                    else:
                        m[at] |= 0x06  # BTYPE = 3, reserved: zlib and libdeflate both call it bad data
                        with pytest.raises(zlib.error):
                            zlib.decompress(bytes(m[pl.off[victim] + hdr:pl.off[victim] + pl.size[victim] - 8]), -15)
                    keep, ptr = mem.put(m)
                    with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(m)) as ix:
                        d.set_route(route)
                        with pytest.raises(_native.GzpxError) as e:
                            read(mem, d, ix, ptr, len(m), rs)
                        assert (e.value.code, e.value.block) == (code, victim), (fmt, route, victim, what)
                        assert e.value.range_index is None
                        if what == "crc":
                            crc = zlib.crc32(chunks[victim])
                            assert "found: %d, expected: %d" % (crc, crc ^ 0xFF) in str(e.value)
            # two damaged members among the needed: the first in stream order
            m = bytearray(s)
            m[pl.off[5] + pl.size[5] - 8] ^= 0xFF
            m[pl.off[2] + pl.size[2] - 8] ^= 0xFF
            keep, ptr = mem.put(m)
            with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(m)) as ix:
                d.set_route(route)
                with pytest.raises(_native.GzpxError) as e:
                    read(mem, d, ix, ptr, len(m), rs)
                assert (e.value.code, e.value.block) == (_native.ERR_INVALID_CHECK, 2)
                # a lying ISIZE changes the index itself; the member then fails its length check
            m = bytearray(s)
            struct.pack_into("<I", m, pl.off[2] + pl.size[2] - 4, pl.isize[2] - 1)
            keep, ptr = mem.put(m)
            with _native.DContext(format=fmt, lib=lib) as d, d.build_index_device(ptr, len(m)) as ix:
                d.set_route(route)
                assert ix.inflated_len == pl.total - 1
                with pytest.raises(_native.GzpxError) as e:
                    read(mem, d, ix, ptr, len(m), [(u[2], u[2] + 5)])
                assert (e.value.code, e.value.block) == (_native.ERR_INSUFFICIENT_SPACE, 2)


# ------------------------------------------------------------------------------------------------ 6. large members
def big_members(lib):
    """The launch form of k_inflate_seg with several waves a member, through a read: Mgzip streams of zlib-made members
    whose compressed average -- the index's consumed // n, which the read hands to the launch -- lies on either side
    of SEG_BIG_BYTES, one of them with a member far below it.  A chunk is three quarters random bytes and then the tail of
    a text buffer of its size, so that real Huffman blocks stand beside the stored ones."""
    mem = Mem(lib)
    for sizes, big in (((146000, 147000), False), ((156000, 158000, 165000), True), ((60000, 260000), True)):
        chunks = [synth.make("random", 3 * n // 4, n).tobytes() + synth.make("text", n, n).tobytes()[3 * n // 4:] for n in sizes]
        s = b"".join(member(MGZIP, c, 1) for c in chunks)
        pl = Plain(MGZIP, s)
        assert pl.plain == b"".join(chunks) and pl.consumed == len(s)
        assert (pl.consumed // pl.n >= SEG_BIG_BYTES) == big, (sizes, pl.size)
        keep, ptr = mem.put(s, shift=len(sizes))
        u, t = pl.ustart, pl.total
        reads = (("whole", [(0, t)]), ("across the first boundary", [(u[1] - 3, u[1] + 70000)]), ("last byte", [(t - 1, t)]),
                 ("empty", [(u[1], u[1])]))
        for route in ROUTES:
            with _native.DContext(format=MGZIP, lib=lib) as d, d.build_index_device(ptr, len(s)) as ix:
                assert (ix.consumed // ix.n_members >= SEG_BIG_BYTES) == big, (sizes, ix.consumed)
                d.set_route(route)
                for what, rs in reads:
                    check_read(mem, d, ix, pl, ptr, len(s), rs, (sizes, route, what))
