"""Member discovery on the device (gzpx_scan_blocks_device, gzpx_decompress_stream_device, gzpx_index_device),
written once and run twice: through the emulated library on CPU (tests/test_emu_scan_device.py, where a device
pointer is a host pointer) and through the real HIP library on the MI355X (tests/test_gpu_scan_device.py).

The yardstick of every comparison is gzpx_scan_blocks on the same bytes in host memory: return code, member count,
`consumed` and both tables must be equal, for every input and every max_blocks."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

from gzp_amd import _native, par, synth

BGZF, MGZIP = _native.FORMAT_BGZF, _native.FORMAT_MGZIP
HDR = {BGZF: 18, MGZIP: 20}
EOF = 28  # the BGZF end-of-file marker: an empty member


class Mem:
    """Device memory as the library under test sees it: numpy arrays under the emulator, torch tensors on the GPU."""

    def __init__(self, lib):
        self.on_gpu = "emu" not in os.path.basename(lib.path)
        if self.on_gpu:
            import torch
            self.torch = torch

    def put(self, data, shift=0):
        """(handle, pointer) of a copy of `data` that starts `shift` bytes into its allocation."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        host = np.zeros(a.size + shift + 1, dtype=np.uint8)
        host[shift:shift + a.size] = a
        if self.on_gpu:
            t = self.torch.from_numpy(host).cuda()
            return t, t.data_ptr() + shift
        return host, host.ctypes.data + shift

    def empty(self, n):
        if self.on_gpu:
            t = self.torch.zeros(max(n, 1), dtype=self.torch.uint8, device="cuda")
            return t, t.data_ptr()
        host = np.zeros(max(n, 1), dtype=np.uint8)
        return host, host.ctypes.data

    def get(self, handle, n):
        if self.on_gpu:
            return handle[:n].cpu().numpy().tobytes()
        return handle[:n].tobytes()


def member(fmt, chunk, level=6):
    """One member as zlib makes it (tests/test_emu_decompress.py: bgzf_member), in either format."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    payload = co.compress(bytes(chunk)) + co.flush()
    if fmt == BGZF:
        hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, ord("B"), ord("C"), 2, len(payload) + 25)
    else:
        hdr = struct.pack("<BBBBIBBHBBHI", 31, 139, 8, 4, 0, 0, 255, 8, ord("I"), ord("G"), 4, len(payload) + 28)
    return hdr + payload + struct.pack("<II", zlib.crc32(bytes(chunk)), len(chunk))


def host_scan(lib, fmt, data, max_blocks=None, tables=True):
    """gzpx_scan_blocks, raw: (rc, n_blocks, consumed, offsets, sizes)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    nb, used = ctypes.c_size_t(77), ctypes.c_size_t(77)
    ptr = a.ctypes.data if a.size else None
    if not tables:
        rc = lib.L.gzpx_scan_blocks(fmt, ptr, a.size, None, None, max_blocks or 0, ctypes.byref(nb), ctypes.byref(used))
        return rc, nb.value, used.value, [], []
    if max_blocks is None:
        lib.L.gzpx_scan_blocks(fmt, ptr, a.size, None, None, 0, ctypes.byref(nb), ctypes.byref(used))
        max_blocks = nb.value + 1
    offs = np.zeros(max_blocks + 1, dtype=np.uint64)
    sizes = np.zeros(max_blocks + 1, dtype=np.uint32)
    rc = lib.L.gzpx_scan_blocks(fmt, ptr, a.size, offs.ctypes.data, sizes.ctypes.data, max_blocks, ctypes.byref(nb),
                                ctypes.byref(used))
    return rc, nb.value, used.value, offs[:nb.value].tolist(), sizes[:nb.value].tolist()


def dev_scan(d, ptr, n, max_blocks, tables=True):
    """gzpx_scan_blocks_device, raw, same shape.  The arrays have one spare entry that must stay untouched."""
    nb, used = ctypes.c_size_t(77), ctypes.c_size_t(77)
    if not tables:
        rc = d.lib.L.gzpx_scan_blocks_device(d.h, ptr, n, None, None, max_blocks or 0, ctypes.byref(nb), ctypes.byref(used), None)
        return rc, nb.value, used.value, [], []
    offs = np.full(max_blocks + 1, 0xABCD, dtype=np.uint64)
    sizes = np.full(max_blocks + 1, 0xABCD, dtype=np.uint32)
    rc = d.lib.L.gzpx_scan_blocks_device(d.h, ptr, n, offs.ctypes.data, sizes.ctypes.data, max_blocks, ctypes.byref(nb),
                                         ctypes.byref(used), None)
    assert offs[max_blocks] == 0xABCD and sizes[max_blocks] == 0xABCD  # nothing written behind the cap
    return rc, nb.value, used.value, offs[:nb.value].tolist(), sizes[:nb.value].tolist()


def agree(lib, mem, d, fmt, data, caps=None, shift=0, what=""):
    """The device's walk of `data` against the host's: without tables, with room for every member, and with every
    cap in `caps`.  Returns the host's (rc, n, consumed) of the uncapped walk."""
    data = bytes(data) if not isinstance(data, np.ndarray) else data
    keep, ptr = mem.put(data, shift)
    n = len(data)
    want = host_scan(lib, fmt, data, tables=False)
    got = dev_scan(d, ptr, n, 0, tables=False)
    assert got == want, (what, "no tables", got[:3], want[:3])
    full = host_scan(lib, fmt, data)
    for cap in [full[1] + 1] + list(caps or []):
        w = host_scan(lib, fmt, data, max_blocks=cap)
        g = dev_scan(d, ptr, n, cap)
        assert g[:3] == w[:3], (what, "cap", cap, g[:3], w[:3])
        assert g[3] == w[3] and g[4] == w[4], (what, "cap", cap, "tables differ")
    del keep
    return want[:3]


# ------------------------------------------------------------------------------------------------ 1. well-formed streams
def our_streams(oracle, classes=None, levels=(1, 3)):
    """(name, format, stream bytes, input bytes) of oracle-made streams: every class, sizes 0, 1, one block, several
    blocks + a ragged tail; BGZF with and without its EOF marker."""
    for fmt, bs in ((BGZF, 65280), (MGZIP, 50000), (MGZIP, 1 << 20)):
        for cls in (classes or sorted(synth.CLASSES)):
            for n in (0, 1, bs, 3 * bs + 4321 if bs < (1 << 20) else 2 * bs + 4321):
                a = synth.make(cls, n, 7)
                for level in levels:
                    s = oracle.compress_stream(a, fmt, level, oracle.COMPAT_1_24, bs)
                    name = "%s bs=%d %s n=%d l%d" % ("bgzf" if fmt == BGZF else "mgzip", bs, cls, n, level)
                    yield name, fmt, s, a
                    if fmt == BGZF:
                        assert struct.unpack("<H", s[-EOF + 16:-EOF + 18])[0] + 1 == EOF  # (the marker: an empty member)
                        yield name + " no-eof", fmt, s[:-EOF], a


def well_formed(lib, oracle, classes=None):
    mem = Mem(lib)
    ds = {f: _native.DContext(format=f, lib=lib) for f in (BGZF, MGZIP)}
    seen = 0
    for name, fmt, s, a in our_streams(oracle, classes):
        rc, n, used = agree(lib, mem, ds[fmt], fmt, s, what=name)
        assert rc == _native.OK and used == len(s), name
        seen += 1
    assert seen >= 3 * len(classes or synth.CLASSES) * 4 * 2
    for d in ds.values():
        d.close()


def foreign_members(lib):
    """zlib-made members of uneven sizes; one with a wrong gzip magic and XLEN != 6 bytes, which the host walk accepts
    (it checks the FEXTRA flag, the SID and the size, nothing else) -- so must the device."""
    mem = Mem(lib)
    rng = np.random.default_rng(11)
    for fmt in (BGZF, MGZIP):
        with _native.DContext(format=fmt, lib=lib) as d:
            chunks = [synth.make(("text", "dna", "random", "zeros", "fastq")[i % 5], int(rng.integers(0, 40000)), i).tobytes()
                      for i in range(9)]
            ms = [member(fmt, c, level=(1, 6, 9)[i % 3]) for i, c in enumerate(chunks)]
            s = b"".join(ms)
            rc, n, used = agree(lib, mem, d, fmt, s, caps=range(0, 11), what="foreign")
            assert (rc, n, used) == (_native.OK, 9, len(s))
            for shift in (1, 5, 15):  # the stream need not start on a 16-byte boundary of device memory
                agree(lib, mem, d, fmt, s, shift=shift, what="foreign shift %d" % shift)
            odd = bytearray(ms[4])
            odd[0], odd[1], odd[2] = 0x50, 0x4B, 0  # no gzip magic, CM = 0
            odd[10], odd[11] = 77, 1                # XLEN says something else
            odd[14], odd[15] = 9, 9                 # so does SLEN
            s2 = b"".join(ms[:4]) + bytes(odd) + b"".join(ms[5:])
            rc, n, used = agree(lib, mem, d, fmt, s2, what="odd header")
            assert (rc, n, used) == (_native.OK, 9, len(s2))


# ------------------------------------------------------------------------------------------------ 2. truncation
def truncation(lib):
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        ms = [member(fmt, synth.make(c, n, 3).tobytes()) for c, n in (("text", 900), ("random", 333), ("dna", 1500))]
        s = b"".join(ms)
        bounds = np.cumsum([len(m) for m in ms]).tolist()
        lens = set(range(0, 45))
        for b in bounds:
            lens.update(range(b - 30, min(b + 30, len(s)) + 1))
        with _native.DContext(format=fmt, lib=lib) as d:
            for n in sorted(lens):
                rc, nb, used = agree(lib, mem, d, fmt, s[:n], caps=(0, 1, 2, 3), what="prefix %d" % n)
                assert rc == _native.OK
                assert used == max([0] + [b for b in bounds if b <= n]) and nb == sum(b <= n for b in bounds)


# ------------------------------------------------------------------------------------------------ 3. max_blocks
def max_blocks(lib, oracle):
    mem = Mem(lib)
    a = synth.make("mixed", 6 * 65280 + 99, 2)
    for fmt, bs in ((BGZF, 65280), (MGZIP, 50000)):
        s = oracle.compress_stream(a, fmt, 1, oracle.COMPAT_1_24, bs)
        n = host_scan(lib, fmt, s, tables=False)[1]
        assert n >= 7
        with _native.DContext(format=fmt, lib=lib) as d:
            agree(lib, mem, d, fmt, s, caps=(0, 1, n - 1, n, n + 1), what="caps")
            # without tables the cap is ignored, as on the host
            keep, ptr = mem.put(s)
            for cap in (0, 1, n - 1, n, n + 1):
                assert dev_scan(d, ptr, len(s), cap, tables=False) == host_scan(lib, fmt, s, cap, tables=False)
                assert dev_scan(d, ptr, len(s), cap, tables=False)[1] == n
            # the Python face
            offs, sizes, used = d.scan_blocks_device(ptr, len(s))
            ho, hs, hu = d.scan_blocks(s)
            assert offs.tolist() == ho.tolist() and sizes.tolist() == hs.tolist() and used == hu
            offs, sizes, used = d.scan_blocks_device(ptr, len(s), max_blocks=2)
            assert offs.tolist() == ho[:2].tolist() and used == int(ho[2])
            assert d.scan_blocks_device(ptr, len(s), want_tables=False) == (n, hu)
            assert d.last_scan_ms() >= 0.0


# ------------------------------------------------------------------------------------------------ 4. invalid headers
def invalid_headers(lib):
    mem = Mem(lib)
    for fmt in (BGZF, MGZIP):
        hdr = HDR[fmt]
        ms = [member(fmt, synth.make(("text", "random", "dna", "fastq", "runs")[i], 200 + 211 * i, i).tobytes())
              for i in range(5)]
        starts = [0] + np.cumsum([len(m) for m in ms]).tolist()

        def put_size(buf, at, size):
            if fmt == BGZF:
                buf[at + 16:at + 18] = struct.pack("<H", (size - 1) & 0xFFFF)
            else:
                buf[at + 16:at + 20] = struct.pack("<I", size & 0xFFFFFFFF)

        def mutations(buf, at, size):
            m = bytearray(buf); m[at + 3] &= ~4 & 0xFF; yield "flag", m
            m = bytearray(buf); m[at + 12] ^= 1; yield "sid0", m
            m = bytearray(buf); m[at + 13] ^= 0x20; yield "sid1", m
            m = bytearray(buf); put_size(m, at, hdr + 7); yield "size hdr+7", m
            m = bytearray(buf); put_size(m, at, hdr + 8); yield "size hdr+8", m  # valid: lands inside the member
            if fmt == MGZIP:
                m = bytearray(buf); put_size(m, at, 0); yield "size 0", m
            else:
                m = bytearray(buf); put_size(m, at, 1); yield "bsize 0", m
            m = bytearray(buf); put_size(m, at, size - 1); yield "one short", m
            m = bytearray(buf); put_size(m, at, size + 1); yield "one long", m

        s = b"".join(ms)
        with _native.DContext(format=fmt, lib=lib) as d:
            saw_err = 0
            for k in (0, 2, 4):
                for name, m in mutations(s, starts[k], len(ms[k])):
                    # the cap edge: k valid members, then the bad header: ERR for max_blocks >= k, OK below
                    rc, nb, used = agree(lib, mem, d, fmt, m, caps=range(0, 7), what="%s at member %d" % (name, k))
                    if name in ("flag", "sid0", "sid1", "size hdr+7", "size 0", "bsize 0"):
                        assert (rc, nb, used) == (_native.ERR_INVALID_HEADER, 0, 0), (name, k)
                        saw_err += 1
                        for cap in range(0, 7):
                            w = host_scan(lib, fmt, m, max_blocks=cap)
                            assert w[0] == (_native.ERR_INVALID_HEADER if cap >= k else _native.OK), (name, k, cap)
                        keep, ptr = mem.put(m)
                        o, p = mem.empty(1 << 16)
                        with pytest.raises(_native.GzpxError) as e:
                            d.decompress_stream_device(ptr, len(m), p, 1 << 16)
                        assert e.value.code == _native.ERR_INVALID_HEADER
                        assert not any(mem.get(o, 1 << 16))  # nothing inflated
            assert saw_err == 15
            # garbage from the first byte, and a stream of zeros
            agree(lib, mem, d, fmt, synth.uniform_random(5000, 1), what="noise")
            agree(lib, mem, d, fmt, bytes(100), what="zeros")


# ------------------------------------------------------------------------------------------------ 5. impostors
def wrap_stored(inner, per_member=60000):
    """`inner` cut into stored (level 0) BGZF members: the payloads carry its bytes verbatim."""
    return b"".join(member(BGZF, inner[i:i + per_member], level=0) for i in range(0, len(inner), per_member))


def impostors(lib, oracle, shifts=range(0, 18)):
    """A valid BGZF stream wrapped again in stored members: every payload holds whole, byte-exact fake members and
    fake chains at unaligned offsets.  They are candidates, they resolve each other -- and none is on the walk."""
    mem = Mem(lib)
    a = synth.make("text", 3 * 65280 + 500, 21)
    inner = oracle.compress_stream(a, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, 65280)
    small = b"".join(member(BGZF, synth.make("dna", 40 + 13 * i, i).tobytes()) for i in range(40))  # a fake chain of 40
    with _native.DContext(format=BGZF, lib=lib) as d:
        for shift in shifts:
            payload = bytes(range(1, shift + 1)) + inner + small + inner[:-EOF]
            outer = wrap_stored(payload)
            assert inner[:200] in outer  # (stored: byte-exact)
            rc, nb, used = agree(lib, mem, d, BGZF, outer, caps=(0, 1, 2), what="wrapped shift %d" % shift)
            assert (rc, nb, used) == (_native.OK, -(-len(payload) // 60000), len(outer))
            keep, ptr = mem.put(outer)
            o, p = mem.empty(len(payload) + 64)
            out_len, n, used = d.decompress_stream_device(ptr, len(outer), p, len(payload) + 64)
            assert (out_len, n, used) == (len(payload), nb, len(outer))
            assert mem.get(o, out_len) == payload, shift
        # the SID bytes wherever one looks, and the densest candidates there can be: a header every four bytes (flag
        # bit, SID and a size that is large enough all repeat) -- far more candidates than the first guess has room for
        for name, unit in (("BC pairs", b"BC"), ("dense", b"BC\x00\xff")):
            payload = unit * (150000 // len(unit))
            outer = wrap_stored(payload) + inner
            rc, nb, used = agree(lib, mem, d, BGZF, outer, caps=(0, 2, 3, 4), what=name)
            assert (rc, used) == (_native.OK, len(outer)) and nb == 3 + 5
            agree(lib, mem, d, BGZF, payload, what=name + " bare")  # no stream at all: as the host says
            agree(lib, mem, d, BGZF, outer[:-3], shift=7, what=name + " cut")


# ------------------------------------------------------------------------------------------------ 6. scan + inflate
def _dev_tables_decompress(d, ptr, n, offs, sizes, p, cap):
    """gzpx_decompress_blocks_device with the host's tables: (code, block, out_len)."""
    try:
        return (_native.OK, None, d.decompress_device(ptr, n, offs, sizes, p, cap))
    except _native.GzpxError as e:
        return (e.code, e.block, None)


def _dev_stream_decompress(d, ptr, n, p, cap):
    try:
        return (_native.OK, None, d.decompress_stream_device(ptr, n, p, cap)[0])
    except _native.GzpxError as e:
        return (e.code, e.block, None)


def stream_decompress(lib, oracle, scale=1):
    """Output bytes, `consumed`, error classes and hand-back counts of the scan + inflate call against the calls that
    take the host's tables.  (Text: k_inflate_seg keeps a first-block hint that any member of a launch writes and any
    reads, so on data whose members differ in kind the number of hand-backs depends on the order the hardware took
    them in; on members of one kind it does not.)"""
    mem = Mem(lib)
    for fmt, bs, level in ((BGZF, 65280, 1), (MGZIP, 50000, 3), (MGZIP, 1 << 20, 1)):
        big = bs >= (1 << 20)
        lite = big and not mem.on_gpu  # (the emulator takes seconds per MiB: there, the round trip of three members only)
        a = synth.make("text", (2 * bs + 777) if lite else (5 * bs + 777) * (1 if big else scale), 31)
        s = oracle.compress_stream(a, fmt, level, oracle.COMPAT_1_24, bs)
        for route in (_native.INFLATE_SEG, _native.INFLATE_WAVE):
            with _native.DContext(format=fmt, lib=lib) as d:
                d.set_route(route)
                if not lite:
                    assert d.decompress(s) == a.tobytes()
                offs, sizes, used = d.scan_blocks(s)
                keep, ptr = mem.put(s)
                o, p = mem.empty(a.size + 64)
                out_len, nb, consumed = d.decompress_stream_device(ptr, len(s), p, a.size + 64)
                assert (out_len, nb, consumed) == (a.size, offs.size, len(s))
                assert mem.get(o, out_len) == a.tobytes()
                assert d.last_inflate_ms() >= 0.0 and d.last_scan_ms() >= 0.0
                if lite:
                    continue
                # a trailing partial member is the caller's
                cut = int(offs[3]) + int(sizes[3]) // 2
                o3, p3 = mem.empty(a.size + 64)
                out_len, nb, consumed = d.decompress_stream_device(ptr, cut, p3, a.size + 64)
                assert (nb, consumed) == (3, int(offs[3])) and mem.get(o3, out_len) == a.tobytes()[:out_len]
                assert out_len == 3 * bs
                # nothing there at all
                assert d.decompress_stream_device(ptr, 5, p3, 64) == (0, 0, 0)
                # errors: the same code and the same block as with the host's tables
                hdr = HDR[fmt]
                cases = (("crc", int(offs[2]) + int(sizes[2]) - 8, a.size + 64),
                         ("isize", int(offs[1]) + int(sizes[1]) - 4, a.size + 64),
                         ("data", int(offs[4]) + hdr + 40, a.size + 64),
                         ("data0", int(offs[0]) + hdr, a.size + 64),
                         ("cap", None, 2 * bs + 100), ("cap0", None, 0))
                for what, at, cap in cases:
                    m = bytearray(s)
                    if at is not None:
                        m[at] ^= 0x5A
                    keep2, ptr2 = mem.put(m)
                    # (two fresh contexts: k_inflate_seg keeps a first-block hint from launch to launch, so how many
                    # members it hands back depends on what a context inflated before -- the same nothing for both)
                    with _native.DContext(format=fmt, lib=lib) as d1, _native.DContext(format=fmt, lib=lib) as d2:
                        d1.set_route(route)
                        d2.set_route(route)
                        o4, p4 = mem.empty(a.size + 64)
                        want = _dev_tables_decompress(d1, ptr2, len(m), offs, sizes, p4, cap)
                        o5, p5 = mem.empty(a.size + 64)
                        got = _dev_stream_decompress(d2, ptr2, len(m), p5, cap)
                        assert got == want, (fmt, bs, route, what, got, want)
                        assert d2.last_redo_count() == d1.last_redo_count(), what
                        assert mem.get(o5, cap) == mem.get(o4, cap), what
                    if what in ("crc", "cap", "cap0"):
                        assert want[0] != _native.OK, what
                # ... and the hand-backs of the stream as it is, on contexts with the same (empty) past
                with _native.DContext(format=fmt, lib=lib) as d1, _native.DContext(format=fmt, lib=lib) as d2:
                    d1.set_route(route)
                    d2.set_route(route)
                    o6, p6 = mem.empty(a.size + 64)
                    assert d1.decompress_device(ptr, len(s), offs, sizes, p6, a.size + 64) == a.size
                    assert d2.decompress_stream_device(ptr, len(s), p6, a.size + 64) == (a.size, offs.size, len(s))
                    assert d2.last_redo_count() == d1.last_redo_count()


# ------------------------------------------------------------------------------------------------ 7. the index
def index(lib, oracle, scale=1):
    """On the streams of twin_cases.block_index (write, flush, write, finish): a reader's index of what the twin wrote
    against the writer's own."""
    from twin_cases import _builder, BS
    mem = Mem(lib)
    a = synth.make("mixed", (9 * BS + 100) * scale, 5)
    for fmt, ofmt, bs in ((par.Bgzf, BGZF, BS), (par.Mgzip, MGZIP, 50000)):
        sink = io.BytesIO()
        w = _builder(lib, fmt, batch=2, bs=bs).from_writer(sink)
        w.write(a[:3 * bs + 10])
        w.flush()
        w.write(a[3 * bs + 10:])
        w.finish()
        par_idx = w.index()
        gzi = w.gzi()
        w.close()
        out = sink.getvalue()
        keep, ptr = mem.put(out)
        with _native.DContext(format=ofmt, lib=lib) as d:
            idx, consumed, total = d.index_device(ptr, len(out))
            assert consumed == len(out) and total == a.size
            n = par_idx.shape[0]
            assert idx[:n].tolist() == par_idx.tolist()
            if ofmt == BGZF:  # the EOF marker is a member to a reader
                assert idx.shape[0] == n + 1 and idx[n].tolist() == [len(out) - EOF, a.size]
            else:
                assert idx.shape[0] == n
            # gzpx_gzi_write takes it as it is
            part = np.ascontiguousarray(idx[:n])
            buf = np.zeros(lib.L.gzpx_gzi_size(n), dtype=np.uint8)
            got = ctypes.c_size_t(0)
            lib.check(lib.L.gzpx_gzi_write(part.ctypes.data, n, buf.ctypes.data, buf.size, ctypes.byref(got)))
            assert buf[:got.value].tobytes() == gzi
            # a capped entries array: the count is still the whole stream's
            few = np.zeros((2, 2), dtype=np.uint64)
            cnt, used, tot = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
            lib.check(lib.L.gzpx_index_device(d.h, ptr, len(out), few.ctypes.data, 2, ctypes.byref(cnt), ctypes.byref(used),
                                              ctypes.byref(tot), None))
            assert cnt.value == idx.shape[0] and few.tolist() == idx[:2].tolist() and tot.value == a.size
            # an invalid header: the scan's answer
            bad = bytearray(out)
            bad[int(idx[2, 0]) + 12] ^= 1
            keep2, ptr2 = mem.put(bad)
            with pytest.raises(_native.GzpxError) as e:
                d.index_device(ptr2, len(bad))
            assert e.value.code == _native.ERR_INVALID_HEADER
