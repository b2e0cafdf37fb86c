"""Who frees what in the C ABI layer (gzp_amd/csrc/gzpx_own.h): every device / pinned allocation, event and stream a
context takes is given back when it is destroyed, an allocation that fails anywhere leaves nothing behind and
reports GZPX_ERR_DEVICE, and a context whose growth failed is as usable afterwards as before.  The CPU emulator's
HIP stubs count what is live and inject the failures (tests/emu/emu_runtime.cpp: emu_live_*, emu_fail_nth_alloc);
on a GPU the same owners run, the failures cannot be provoked there.

Every byte result is checked as the other emulator tests check it: compressed streams against the oracle (Snap:
decoded back to the input), inflated bytes against the input."""
import ctypes
import functools
import gc
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import snap_cases
from gzp_amd import _native, synth
from scan_cases import Mem

BS = 65280            # compress side: Bgzf's default buffer
SLAB3 = 3 * BS + 100  # the "larger" slab: four blocks, the last one short
DBS = 32768           # inflate side: the members' buffer size
CAP = 300             # an armed sequence must have succeeded by this n


def _hooks(emu_lib):
    L = emu_lib.L
    for f in (L.emu_live_allocs, L.emu_live_events, L.emu_live_streams):
        f.restype = ctypes.c_long
    L.emu_fail_nth_alloc.argtypes = [ctypes.c_long]
    L.emu_fail_nth_alloc.restype = ctypes.c_long  # what was left of the previous arming
    return L


@pytest.fixture
def live(emu_lib):
    """A function that reads (allocations, events, streams) live now; the two process-lifetime states (gzpx_crc32's
    and gzpx_adler32's stream and buffers) exist before its first reading, and no context of an earlier test is left."""
    L = _hooks(emu_lib)
    _native.crc32(b"abc", lib=emu_lib)
    _native.adler32(b"abc", lib=emu_lib)
    gc.collect()
    return lambda: (L.emu_live_allocs(), L.emu_live_events(), L.emu_live_streams())


@functools.lru_cache(maxsize=None)
def _text(n, seed):
    return synth.make("text", n, seed)


@functools.lru_cache(maxsize=None)
def _slab_want(oracle, level, n):
    return oracle.compress_stream(_text(n, 7), oracle.FMT_BGZF, level, oracle.COMPAT_1_24, BS)


@functools.lru_cache(maxsize=None)
def _members(oracle, n_members):
    """(input bytes, a BGZF stream of exactly n_members members of it: the EOF marker is cut off)."""
    a = _text((n_members - 1) * DBS + 20000, 3 + n_members)
    s = oracle.compress_stream(a, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, DBS)
    return a.tobytes(), bytes(s[:-28])


def _bgzf(level, lib):
    return _native.Context(format=_native.FORMAT_BGZF, level=level, buffer_size=BS, lib=lib, max_slab_bytes=SLAB3)


def _snap(lib):
    return _native.Context(format=_native.FORMAT_SNAP, buffer_size=BS, lib=lib, max_slab_bytes=SLAB3)


def _check_slab(oracle, c, level, n):
    assert c.compress_slab(_text(n, 7), True) == _slab_want(oracle, level, n), "level %d, %d bytes" % (level, n)


def _check_snap(c, n):
    got = c.compress_slab(_text(n, 7), True)
    assert snap_cases.decode_frames(got)[0] == _text(n, 7).tobytes(), "snap, %d bytes" % n
    return got


def _check_inflate(oracle, d, n_members):
    plain, s = _members(oracle, n_members)
    assert len(d.scan_blocks(s)[0]) == n_members
    assert d.decompress(s) == plain, "%d members" % n_members


# ------------------------------------------------------------------------------------------------ 1. balance
@pytest.mark.parametrize("level", [1, 3, 6])
def test_compress_context_gives_everything_back(emu_lib, oracle, live, level):
    before = live()
    with _bgzf(level, emu_lib) as c:
        for n in (100, SLAB3, 100):  # staging and size tables grow once and are reused
            _check_slab(oracle, c, level, n)
        assert live() != before
    assert live() == before
    if level != 1:
        return
    with _snap(emu_lib) as c:
        _check_snap(c, SLAB3)
        c.debug_snap(True)
        mid = live()
        _check_snap(c, 100)
        c.debug_snap(False)
        assert live() == (mid[0] - 1, mid[1], mid[2])
        c.debug_snap(True)  # ... and left enabled for the destructor
    assert live() == before


def _zlib_batch(emu_lib, d, mem):
    parts = [_text(5000, 21).tobytes(), b"", _text(40000, 22).tobytes()]
    zs = [zlib.compress(p, 6) for p in parts]
    keep = [mem.put(b"".join(zs)), mem.put(np.cumsum([0] + [len(z) for z in zs[:-1]]).astype(np.uint64).view(np.uint8)),
            mem.put(np.array([len(z) for z in zs], dtype=np.uint32).view(np.uint8)),
            mem.put(np.array([len(p) for p in parts], dtype=np.uint32).view(np.uint8)), mem.empty(45000 + 64)]
    got = d.inflate_batch_device(_native.WRAP_ZLIB, keep[0][1], sum(len(z) for z in zs), keep[1][1], keep[2][1], keep[3][1],
                                 3, keep[4][1], 45000)
    assert got == (45000, 0) and mem.get(keep[4][0], 45000) == b"".join(parts)


def _line_reads_and_find(d, mem, ix, ptr, s, plain, batch):
    """A line table built in batches of `batch` inflated bytes, one line_offsets, one read_lines and one find with
    positions and line numbers, each against the host's answer."""
    starts = [0] + [i + 1 for i, ch in enumerate(plain) if ch == 10]
    d.set_lines_batch(batch)
    with d.build_lines_device(ix, ptr, len(s)) as lt:
        assert (lt.n_delims, lt.n_lines) == (len(starts) - 1, len(starts) - (plain[-1:] == b"\n"))
        ks = [0, 1, len(starts) // 2, len(starts) - 1]
        assert d.line_offsets_device(ix, lt, ptr, len(s), ks).tolist() == [starts[k] for k in ks]
        ranges = [(0, 2), (len(starts) // 2, len(starts) // 2 + 3), (5, 5)]
        want = b"".join(plain[starts[a]:starts[b]] for a, b in ranges)
        out, p_out = mem.empty(len(want) + 64)
        m, o, br = d.read_lines_device(ix, lt, ptr, len(s), ranges, p_out, len(want))
        assert m == len(want) and mem.get(out, m) == want
        assert o.tolist() == np.cumsum([0] + [starts[b] - starts[a] for a, b in ranges]).tolist()
    pattern = plain[starts[1]:starts[1] + 3]
    hits = [i for i in range(len(plain) - 2) if plain[i:i + 3] == pattern]
    pos, p_pos = mem.empty(len(hits) * 8)
    lns, p_lns = mem.empty(len(hits) * 8)
    assert d.find_device(ix, ptr, len(s), pattern, 10, p_pos, p_lns, len(hits)) == len(hits) > 0
    assert np.frombuffer(mem.get(pos, len(hits) * 8), dtype=np.uint64).tolist() == hits
    assert np.frombuffer(mem.get(lns, len(hits) * 8), dtype=np.uint64).tolist() == \
        (np.searchsorted(starts, hits, side="right") - 1).tolist()


def _checksum_batch(d, mem):
    parts = [_text(5000, 21).tobytes(), b"", _text(40000, 22).tobytes()]
    keep = [mem.put(b"".join(parts)), mem.put(np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64).view(np.uint8)),
            mem.empty(3 * 4)]
    assert d.checksum_batch_device(_native.CHECK_ADLER32, keep[0][1], 45000, keep[1][1], None, 3, keep[2][1]) == (0, None)
    assert np.frombuffer(mem.get(keep[2][0], 12), dtype=np.uint32).tolist() == [zlib.adler32(p) for p in parts]


def test_dcontext_gives_everything_back(emu_lib, oracle, live):
    before = live()
    mem = Mem(emu_lib)
    with _native.DContext(format=_native.FORMAT_BGZF, lib=emu_lib) as d:
        for n_members in (1, 40, 1):
            _check_inflate(oracle, d, n_members)
        for n_members in (40, 1):
            plain, s = _members(oracle, n_members)
            keep, ptr = mem.put(s, shift=5)
            offs, sizes, used = d.scan_blocks(s)
            ustart = np.arange(n_members, dtype=np.uint64) * DBS
            out, p_out = mem.empty(len(plain) + 64)
            assert d.decompress_stream_device(ptr, len(s), p_out, len(plain) + 64) == (len(plain), n_members, len(s))
            assert mem.get(out, len(plain)) == plain
            got = d.scan_blocks_device(ptr, len(s))
            assert (got[0].tolist(), got[1].tolist(), got[2]) == (offs.tolist(), sizes.tolist(), used)
            idx, iused, total = d.index_device(ptr, len(s))
            assert (idx[:, 0].tolist(), idx[:, 1].tolist(), iused, total) == (offs.tolist(), ustart.tolist(), used, len(plain))
            with d.build_index_device(ptr, len(s)) as ix:
                assert ix.entries().tolist() == idx.tolist()
                one = [(len(plain) // 2, len(plain) // 2 + 777)]
                many = [((i * 7919) % (len(plain) - 100), (i * 7919) % (len(plain) - 100) + 100) for i in range(200)]
                for ranges in (one, many, one):
                    want = b"".join(plain[b:e] for b, e in ranges)
                    m, o = d.read_ranges_device(ix, ptr, len(s), ranges, p_out, len(want))
                    assert m == len(want) and mem.get(out, m) == want
                    assert o.tolist() == np.cumsum([0] + [e - b for b, e in ranges]).tolist()
                _line_reads_and_find(d, mem, ix, ptr, s, plain, 20 * DBS)  # (40 members: two batches)
                assert live() != before
            _zlib_batch(emu_lib, d, mem)
            _checksum_batch(d, mem)
    assert live() == before


# ------------------------------------------------------------------------------------------------ 2. allocation failure
def _compress_steps(oracle, kind):
    if kind == "snap":
        return lambda lib: _snap(lib), [lambda c: _check_snap(c, 100), lambda c: _check_snap(c, SLAB3)]
    level = {"bgzf1": 1, "bgzf6": 6}[kind]
    return (lambda lib: _bgzf(level, lib),
            [lambda c: _check_slab(oracle, c, level, 100), lambda c: _check_slab(oracle, c, level, SLAB3)])


def _indexed_reads(emu_lib, oracle, d):
    """index build -> read ranges -> lines build -> read lines -> find -> checksum batch, on a stream of three members."""
    mem = Mem(emu_lib)
    plain, s = _members(oracle, 3)
    keep, ptr = mem.put(s)
    with d.build_index_device(ptr, len(s)) as ix:
        ranges = [(100, 877), (DBS - 5, DBS + 5), (len(plain) - 9, len(plain))]
        want = b"".join(plain[b:e] for b, e in ranges)
        out, p_out = mem.empty(len(want) + 64)
        m, o = d.read_ranges_device(ix, ptr, len(s), ranges, p_out, len(want))
        assert m == len(want) and mem.get(out, m) == want
        _line_reads_and_find(d, mem, ix, ptr, s, plain, 2 * DBS)  # (two batches)
    _checksum_batch(d, mem)


def _sequence(oracle, kind):
    if kind == "dreads":
        return (lambda lib: _native.DContext(format=_native.FORMAT_BGZF, lib=lib),
                [lambda d: _indexed_reads(d.lib, oracle, d)])
    if kind == "dctx":
        return (lambda lib: _native.DContext(format=_native.FORMAT_BGZF, lib=lib),
                [lambda d: _check_inflate(oracle, d, 1), lambda d: _check_inflate(oracle, d, 40)])
    return _compress_steps(oracle, kind)


def _run(emu_lib, make, steps):
    """create -> every step (each checks its own bytes) -> destroy; a GzpxError of the first failing call ends it."""
    with make(emu_lib) as c:
        for step in steps:
            step(c)


@pytest.mark.parametrize("kind", ["bgzf1", "bgzf6", "snap", "dctx", "dreads"])
def test_any_failing_allocation_leaves_nothing_behind(emu_lib, oracle, live, kind):
    L = _hooks(emu_lib)
    make, steps = _sequence(oracle, kind)
    before = live()
    # the allocations of the whole sequence, counted once: the cap below is a condition, not a measurement
    L.emu_fail_nth_alloc(10 ** 6)
    try:
        _run(emu_lib, make, steps)
    finally:
        n_allocs = 10 ** 6 - L.emu_fail_nth_alloc(0)
    assert 0 < n_allocs < CAP - 1, n_allocs
    assert live() == before
    for n in range(1, CAP + 1):
        L.emu_fail_nth_alloc(n)
        try:
            _run(emu_lib, make, steps)
            failed = None
        except _native.GzpxError as e:
            failed = e
        finally:
            L.emu_fail_nth_alloc(0)
        assert live() == before, "allocation %d failing: (allocations, events, streams) left live" % n
        if failed is None:
            break
        assert failed.code == _native.ERR_DEVICE, (n, failed)
        _run(emu_lib, make, steps)  # a fresh context is none the worse for it: the reference bytes
        assert live() == before
    else:
        pytest.fail("the sequence never succeeded with an allocation failure armed up to n = %d" % CAP)
    assert n == n_allocs + 1, "every one of the %d allocations must have been made to fail once" % n_allocs


# ------------------------------------------------------------------------------------------------ 3. growth failure
def _fails_once_then_works(emu_lib, grow, again):
    L = _hooks(emu_lib)
    L.emu_fail_nth_alloc(1)  # the first allocation of the call that has to grow
    try:
        with pytest.raises(_native.GzpxError) as e:
            grow()
    finally:
        assert L.emu_fail_nth_alloc(0) == 0, "the call did not allocate"
    assert e.value.code == _native.ERR_DEVICE
    grow()
    again()


def test_failed_growth_keeps_the_dcontext_usable(emu_lib, oracle, live):
    before = live()
    with _native.DContext(format=_native.FORMAT_BGZF, lib=emu_lib) as d:
        _check_inflate(oracle, d, 1)
        _fails_once_then_works(emu_lib, lambda: _check_inflate(oracle, d, 40), lambda: _check_inflate(oracle, d, 1))
    assert live() == before


def test_failed_growth_keeps_the_compress_context_usable(emu_lib, oracle, live):
    before = live()
    with _bgzf(1, emu_lib) as c:
        _check_slab(oracle, c, 1, 100)
        _fails_once_then_works(emu_lib, lambda: _check_slab(oracle, c, 1, SLAB3), lambda: _check_slab(oracle, c, 1, 100))
    assert live() == before


# ------------------------------------------------------------------------------------------------ 4. gzpx_adler32's state
_ADLER_CHILD = r"""
import ctypes, sys, zlib
L = ctypes.CDLL(sys.argv[1])
for f in (L.emu_live_allocs, L.emu_live_events, L.emu_live_streams):
    f.restype = ctypes.c_long
L.emu_fail_nth_alloc.argtypes = [ctypes.c_long]
L.gzpx_adler32_checked.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
live = lambda: (L.emu_live_allocs(), L.emu_live_events(), L.emu_live_streams())
data = bytes((i * 131 + 7) & 255 for i in range(1000))
out = ctypes.c_uint32(0)
before = live()
L.emu_fail_nth_alloc(2)  # the stream and the first buffer exist by then
rc = L.gzpx_adler32_checked(1, data, len(data), ctypes.byref(out))
L.emu_fail_nth_alloc(0)
print(rc, live() == before)
rc = L.gzpx_adler32_checked(1, data, len(data), ctypes.byref(out))
print(rc, out.value == zlib.adler32(data))
"""


def test_adler32_state_is_made_whole_or_not_at_all(emu_lib):
    """The state is static, so a fresh process: its first call fails in the middle of making the state, the second
    must find nothing half-made (a stream without buffers used to send it through a null pointer)."""
    r = subprocess.run([sys.executable, "-c", _ADLER_CHILD, os.path.abspath(emu_lib.path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(_native.ERR_DEVICE), "True", str(_native.OK), "True"], (r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------------ 5. gzpx_crc32's state
_CRC_CHILD = r"""
import ctypes, sys, zlib
L = ctypes.CDLL(sys.argv[1])
for f in (L.emu_live_allocs, L.emu_live_events, L.emu_live_streams):
    f.restype = ctypes.c_long
L.emu_fail_nth_alloc.argtypes = [ctypes.c_long]
L.gzpx_crc32_checked.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
live = lambda: (L.emu_live_allocs(), L.emu_live_events(), L.emu_live_streams())
data = bytes((i * 131 + 7) & 255 for i in range(1000))
out = ctypes.c_uint32(0)
before = live()
L.emu_fail_nth_alloc(2)  # the stream and the tiles' table exist by then
rc = L.gzpx_crc32_checked(0, data, len(data), ctypes.byref(out))
L.emu_fail_nth_alloc(0)
print(rc, live() == before)
rc = L.gzpx_crc32_checked(0, data, len(data), ctypes.byref(out))
print(rc, out.value == zlib.crc32(data))
# a running CRC over more than one 64 KiB tile with an odd tail (the staging grows for it)
big = bytes((i * i * 31 + i) & 255 for i in range(200001))
rc = L.gzpx_crc32_checked(zlib.crc32(big[:1000]), big[1000:], len(big) - 1000, ctypes.byref(out))
print(rc, out.value == zlib.crc32(big))
"""


def test_crc32_state_is_made_whole_or_not_at_all(emu_lib):
    """The sibling of the Adler-32 test, in a fresh process for the same reason: the first call ever fails while the
    state is being made and must leave nothing live; the second finds nothing half-made and computes zlib's value."""
    r = subprocess.run([sys.executable, "-c", _CRC_CHILD, os.path.abspath(emu_lib.path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(_native.ERR_DEVICE), "True", str(_native.OK), "True", str(_native.OK), "True"], \
        (r.stdout, r.stderr)
