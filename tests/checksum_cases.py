"""Checksums of a table of device-resident buffers (gzpx_checksum_batch_device), written once and run twice: through
the emulated library on CPU (tests/test_emu_checksums.py, where a device pointer is a host pointer) and through the
real HIP library on the MI355X (tests/test_gpu_checksums.py).

Every comparison is exact equality.  The yardsticks are zlib.crc32 and zlib.adler32, and for CRC-32C the table-driven
routine below, pinned on published answers (known_answers) before anything is compared with it.  Sums of buffers too
long to hash on the host come from gzpx_crc32_combine (host arithmetic that tests/test_checks.py pins on zlib), from
the closed form of Adler-32, and from crc32c_combine below, which known_answers pins on direct hashing."""
import ctypes
import functools
import os
import subprocess
import sys
import zlib

import numpy as np

import batch_cases
import scan_cases
from gzp_amd import _native, synth

CRC32, ADLER32, CRC32C = _native.CHECK_CRC32, _native.CHECK_ADLER32, _native.CHECK_CRC32C
KINDS = {"crc32": CRC32, "adler32": ADLER32, "crc32c": CRC32C}
OK, E_ARG, E_CHECK = _native.OK, _native.ERR_INVALID_ARG, _native.ERR_INVALID_CHECK
TILE = 65536
LENGTHS = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 131071, 131072,
           131073, 3 * 65536 + 17)  # around the lane's segment, the 16-byte load and the tile
MISALIGNMENTS = (0, 1, 3, 8, 13, 15)
ADLER_BASE = 65521


# ------------------------------------------------------------------------------------------------ references
def _crc32c_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        t.append(c)
    return t


_T = _crc32c_table()


def crc32c(buf, seed=0):
    """CRC-32C (Castagnoli, reflected, init and xor-out all ones) with zlib.crc32's signature."""
    c = seed ^ 0xFFFFFFFF
    t = _T
    for b in bytes(buf):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _crc32c_cached(buf, seed):
    return crc32c(buf, seed)


def reference(kind, buf, seed=None):
    buf = bytes(buf)
    if kind == CRC32:
        return zlib.crc32(buf, 0 if seed is None else seed)
    if kind == ADLER32:
        return zlib.adler32(buf, 1 if seed is None else seed)
    return _crc32c_cached(buf, 0 if seed is None else seed)


def _gf2_times(mat, vec):
    s, i = 0, 0
    while vec:
        if vec & 1:
            s ^= mat[i]
        vec >>= 1
        i += 1
    return s


def _gf2_square(mat):
    return [_gf2_times(mat, mat[i]) for i in range(32)]


def crc32c_combine(crc1, crc2, len2):
    """CRC-32C of A || B from the two sums and len(B): zlib's crc32_combine (matrix form) with the other polynomial."""
    if len2 == 0:
        return crc1
    odd = [0x82F63B78] + [1 << i for i in range(31)]  # the operator for one zero bit
    even = _gf2_square(odd)   # two bits
    odd = _gf2_square(even)   # four
    while True:
        even = _gf2_square(odd)
        if len2 & 1:
            crc1 = _gf2_times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = _gf2_square(even)
        if len2 & 1:
            crc1 = _gf2_times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def adler32_zeros(adler, n):
    """Adler-32 behind n more zero bytes: a stays, b grows by n a."""
    a, b = adler & 0xFFFF, adler >> 16
    return a | (((b + (n % ADLER_BASE) * a) % ADLER_BASE) << 16)


def known_answers():
    """The references themselves, on published vectors."""
    s = b"123456789"
    assert crc32c(s) == 0xE3069283 and zlib.crc32(s) == 0xCBF43926 and zlib.adler32(s) == 0x091E01DE
    # RFC 3720 B.4
    assert crc32c(bytes(32)) == 0x8A9136AA and crc32c(b"\xff" * 32) == 0x62A8AB43
    assert crc32c(bytes(range(32))) == 0x46DD794E and crc32c(bytes(range(31, -1, -1))) == 0x113FDB5C
    assert crc32c(s[4:], crc32c(s[:4])) == 0xE3069283  # the running form
    rng = np.random.RandomState(5)
    for la, lb in ((0, 7), (7, 0), (1, 1), (300, 5000), (4097, 33), (13, 70001)):
        a, b = rng.randint(0, 256, la, dtype=np.uint8).tobytes(), rng.randint(0, 256, lb, dtype=np.uint8).tobytes()
        assert crc32c_combine(crc32c(a), crc32c(b), lb) == crc32c(a + b), (la, lb)
        assert adler32_zeros(zlib.adler32(a), lb) == zlib.adler32(a + bytes(lb))
    for n in (1, 2, 5, 1000, 70001):
        assert zeros_sum(n, crc32c(bytes(1)), crc32c_combine) == crc32c(bytes(n)), n


# ------------------------------------------------------------------------------------------------ one call
class Result:
    pass


def put_aligned(mem, blob, lead=0):
    """(handle, pointer): a copy of `blob` in device memory whose first byte lies `lead` bytes behind a 16-byte boundary."""
    shift = lead
    for _ in range(8):
        h, p = mem.put(blob, shift)
        if p % 16 == lead:
            return h, p
        shift = (shift + lead - p) % 16 + 16
    raise AssertionError("no allocation with the alignment asked for")


def table(mem, keep, a):
    keep.append(mem.put(np.ascontiguousarray(a).view(np.uint8)))
    return keep[-1]


def call(lib, d, kind, d_in, in_len, offs, sizes, n, seeds=None, expected=None, sums=True, results=True, stream=None):
    """One gzpx_checksum_batch_device call on host tables (sizes None: the span form, offs has n + 1 entries); every
    written table has a spare entry that must stay as it was."""
    mem = scan_cases.Mem(lib)
    keep = []
    p_off = table(mem, keep, np.array(list(offs) + [0], dtype=np.uint64))[1]
    p_size = table(mem, keep, np.array(list(sizes) + [0], dtype=np.uint32))[1] if sizes is not None else None
    p_seed = table(mem, keep, np.array(list(seeds) + [0], dtype=np.uint32))[1] if seeds is not None else None
    p_exp = table(mem, keep, np.array(list(expected) + [0], dtype=np.uint32))[1] if expected is not None else None
    h_sums = table(mem, keep, np.full(n + 1, 0xABCD, dtype=np.uint32)) if sums else (None, None)
    h_res = table(mem, keep, np.full(4 * (n + 1), 0xABCD, dtype=np.uint32)) if results else (None, None)
    r = Result()
    n_failed = ctypes.c_size_t(77)
    info = _native.GzpxCheckInfo()
    r.rc = lib.L.gzpx_checksum_batch_device(d.h, kind, d_in, in_len, p_off, p_size, n, p_seed, p_exp, h_sums[1], h_res[1],
                                            ctypes.byref(n_failed), ctypes.byref(info), stream)
    r.n_failed, r.block, r.found, r.expected = n_failed.value, info.block, info.found, info.expected
    if sums:
        a = np.frombuffer(mem.get(h_sums[0], 4 * (n + 1)), dtype=np.uint32)
        assert a[n] == 0xABCD, "d_sums written behind [n)"
        r.sums = a[:n].tolist()
    if results:
        a = np.frombuffer(mem.get(h_res[0], 16 * (n + 1)), dtype=np.uint32).reshape(n + 1, 4)
        assert (a[n] == 0xABCD).all(), "d_results written behind [n)"
        r.results = [tuple(int(v) for v in x) for x in a[:n]]
    del keep
    return r


def context(lib):
    return _native.DContext(format=_native.FORMAT_BGZF, lib=lib)


def check_good(r, kind, blob, offs, sizes, seeds=None, what=None):
    """Every entry of a call without d_expected against the reference."""
    want = [reference(kind, blob[o:o + s], None if seeds is None else seeds[i]) for i, (o, s) in enumerate(zip(offs, sizes))]
    assert r.rc == OK and r.n_failed == 0, (what, r.rc, r.n_failed, r.block)
    bad = [(i, offs[i], sizes[i], hex(r.sums[i]), hex(want[i])) for i in range(len(want)) if r.sums[i] != want[i]]
    assert not bad, (what, len(bad), bad[:8])
    if hasattr(r, "results"):
        assert r.results == [(OK, min(s, 0xFFFFFFFF), w, 0) for s, w in zip(sizes, want)], what


# ------------------------------------------------------------------------------------------------ 1. values
def content(name, n, seed=3):
    if name == "random":
        return np.random.RandomState(seed).randint(0, 256, n, dtype=np.uint8).tobytes()
    return (b"\xff" if name == "ff" else b"\x00") * n


def values(lib, kind, what, misalignments=MISALIGNMENTS, lengths=LENGTHS):
    """Every length at every misalignment of its first byte, in one table."""
    offs, sizes = [], []
    pos = 5
    for length in lengths:
        for mis in misalignments:
            pos += (mis - pos) % 16
            offs.append(pos)
            sizes.append(length)
            pos += length + 1
    blob = content(what, pos + 3)
    mem = scan_cases.Mem(lib)
    h, d_in = put_aligned(mem, blob)
    with context(lib) as d:
        r = call(lib, d, kind, d_in, len(blob), offs, sizes, len(offs))
        check_good(r, kind, blob, offs, sizes, what=(kind, what))
    del h


# ------------------------------------------------------------------------------------------------ 2. seeds
def seeds(lib, kind):
    rng = np.random.RandomState(17)
    blob = content("random", 200000, 9)
    mem = scan_cases.Mem(lib)
    h, d_in = put_aligned(mem, blob, 3)
    if kind == ADLER32:  # halves below the modulus
        fixed = [0, 1, 0xFFF0FFF0]
        rnd = [int(rng.randint(0, ADLER_BASE)) | (int(rng.randint(0, ADLER_BASE)) << 16) for _ in range(9)]
    else:
        fixed = [0, 1, 0xFFFFFFFF]
        rnd = [int(x) for x in rng.randint(0, 1 << 32, 9, dtype=np.uint64)]
    entries = [(0, 0), (7, 1), (100, 70000), (65536, 65536), (11, 131073), (199999, 1), (200000, 0)]
    offs, sizes, sd = [], [], []
    for s in fixed + rnd:
        for o, z in entries:
            offs.append(o)
            sizes.append(z)
            sd.append(s)
    with context(lib) as d:
        r = call(lib, d, kind, d_in, len(blob), offs, sizes, len(offs), seeds=sd)
        check_good(r, kind, blob, offs, sizes, seeds=sd, what=(kind, "seeds"))
        for i, z in enumerate(sizes):
            if z == 0:
                assert r.sums[i] == sd[i], "an empty entry yields its seed"
        # one buffer in k pieces, k calls, each seeded with the sum before it
        cuts = [0, 1, 70001, 70001, 131072, 196609, 200000]
        run = None
        for a, b in zip(cuts, cuts[1:]):
            r = call(lib, d, kind, d_in, len(blob), [a], [b - a], 1, seeds=None if run is None else [run])
            assert r.rc == OK
            run = r.sums[0]
        assert run == reference(kind, blob), (kind, "pieces")
    del h


# ------------------------------------------------------------------------------------------------ 3. both table shapes, the ZIP case
def zip_case(lib, n=24, small=False):
    """A RAW batch inflated on the device, then verified where it lies against the CRC-32 a ZIP directory would hold:
    d_out_offsets as the span form, (d_out_offsets[:n], d_out_sizes) as the sizes form."""
    sizes = [(40000, 0, 70000, 1, 17, 3000, 16385, 65536)[i % 8] + 13 * i for i in range(n)]
    if small:
        sizes = [s if s < 30000 else s // 4 for s in sizes]
    plains = [synth.make(batch_cases.CLASSES[i % 5], s, 40 + i).tobytes() for i, s in enumerate(sizes)]
    members = [batch_cases.deflate(p, batch_cases.RAW) for p in plains]
    crcs = [zlib.crc32(p) for p in plains]
    blob = b"".join(members)
    m_off = batch_cases.prefix([len(m) for m in members])[:-1]
    total = sum(sizes)
    mem = scan_cases.Mem(lib)
    for route, d in batch_cases.contexts(lib):
        keep = [mem.put(blob), mem.empty(total + 16)]
        t_off = table(mem, keep, np.array(m_off, dtype=np.uint64))
        t_size = table(mem, keep, np.array([len(m) for m in members], dtype=np.uint32))
        t_osize = table(mem, keep, np.array(sizes, dtype=np.uint32))
        t_ooff = table(mem, keep, np.zeros(n + 1, dtype=np.uint64))
        assert d.inflate_batch_device(batch_cases.RAW, keep[0][1], len(blob), t_off[1], t_size[1], t_osize[1], n, keep[1][1],
                                      total, d_out_offsets_ptr=t_ooff[1]) == (total, 0)
        d_out = keep[1][1]
        t_exp = table(mem, keep, np.array(crcs, dtype=np.uint32))
        t_sums = table(mem, keep, np.zeros(n, dtype=np.uint32))
        # the span form, verify only (no d_sums), through the Python call
        assert d.checksum_batch_device(CRC32, d_out, total, t_ooff[1], None, n, d_expected_ptr=t_exp[1]) == (0, None)
        assert d.last_check_ms() >= 0.0
        # the sizes form over the same offsets
        assert d.checksum_batch_device(CRC32, d_out, total, t_ooff[1], t_osize[1], n, d_sums_ptr=t_sums[1]) == (0, None)
        assert np.frombuffer(mem.get(t_sums[0], 4 * n), dtype=np.uint32).tolist() == crcs, route
        # two directory entries are wrong
        wrong = list(crcs)
        wrong[5] ^= 0x00010000
        wrong[17] ^= 1
        ooff = batch_cases.prefix(sizes)
        for form_sizes in (None, sizes):
            r = call(lib, d, CRC32, d_out, total, ooff if form_sizes is None else ooff[:-1], form_sizes, n, expected=wrong)
            assert r.rc == E_CHECK and r.block == 5 and r.n_failed == 2, (route, r.rc, r.block, r.n_failed)
            assert (r.found, r.expected) == (crcs[5], wrong[5])
            assert r.sums == crcs, route
            assert r.results == [(E_CHECK if i in (5, 17) else OK, sizes[i], crcs[i], wrong[i]) for i in range(n)], route
        n_failed, info = d.checksum_batch_device(CRC32, d_out, total, t_ooff[1], None, n, d_sums_ptr=t_sums[1],
                                                 d_expected_ptr=table(mem, keep, np.array(wrong, dtype=np.uint32))[1],
                                                 raise_on_entry_error=False)
        assert (n_failed, info.block, info.found, info.expected) == (2, 5, crcs[5], wrong[5])
        try:
            d.checksum_batch_device(CRC32, d_out, total, t_ooff[1], None, n, d_expected_ptr=keep[-1][1])
            raise AssertionError("no error for a failing entry")
        except _native.GzpxError as e:
            assert (e.code, e.block) == (E_CHECK, 5)
        del keep


# ------------------------------------------------------------------------------------------------ 4. overlap and order
def overlap_and_order(lib, kind):
    blob = content("random", 300000, 21)
    mem = scan_cases.Mem(lib)
    h, d_in = put_aligned(mem, blob, 13)
    with context(lib) as d:
        # one entry three times, nested entries, descending offsets
        offs = [1000, 1000, 1000, 0, 10, 100, 1000, 70000, 250000, 200000, 150000, 100000, 50000, 0]
        sizes = [140000, 140000, 140000, 300000, 299980, 299800, 100, 5, 50000, 50001, 65536, 65537, 3, 131072]
        r = call(lib, d, kind, d_in, len(blob), offs, sizes, len(offs))
        check_good(r, kind, blob, offs, sizes, what=(kind, "overlap"))
        # a table shuffled with a fixed seed
        rng = np.random.RandomState(4)
        cuts = sorted(set([0, len(blob)] + [int(x) for x in rng.randint(0, len(blob), 60)]))
        pairs = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
        order = rng.permutation(len(pairs))
        offs, sizes = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
        r = call(lib, d, kind, d_in, len(blob), offs, sizes, len(offs))
        check_good(r, kind, blob, offs, sizes, what=(kind, "shuffled"))
    del h


# ------------------------------------------------------------------------------------------------ 5. invalid entries and arguments
def invalid(lib):
    blob = content("random", 100000, 8)
    in_len = len(blob)
    mem = scan_cases.Mem(lib)
    h, d_in = put_aligned(mem, blob, 1)
    good = [(0, 100), (99000, 1000), (500, 70000), (in_len, 0)]
    with context(lib) as d:
        for kind in (CRC32, ADLER32, CRC32C):
            # the sizes form: an offset above in_len; offset + size one byte over in_len
            for bad in ((in_len + 1, 0), (in_len - 10, 11)):
                pairs = good[:2] + [bad] + good[2:]
                offs, sizes = [p[0] for p in pairs], [p[1] for p in pairs]
                want = [reference(kind, blob[o:o + s]) if (o, s) != bad else 0 for o, s in pairs]
                r = call(lib, d, kind, d_in, in_len, offs, sizes, len(pairs), expected=want)
                assert (r.rc, r.block, r.n_failed) == (E_ARG, 2, 1), (kind, bad, r.rc, r.block, r.n_failed)
                assert r.sums == want and (r.found, r.expected) == (0, 0)
                assert r.results == [(E_ARG if i == 2 else OK, 0 if i == 2 else sizes[i], want[i], want[i]) for i in range(5)]
            # the span form: one decreasing pair; the last offset above in_len
            for span, bad in (([0, 100, 50000, 40000, 90000, in_len], (2,)), ([0, 100, 50000, 50000, in_len + 1], (3,))):
                n = len(span) - 1
                want = [0 if i in bad else reference(kind, blob[span[i]:span[i + 1]]) for i in range(n)]
                r = call(lib, d, kind, d_in, in_len, span, None, n)
                assert (r.rc, r.block, r.n_failed) == (E_ARG, bad[0], len(bad)), (kind, span, r.rc, r.block, r.n_failed)
                assert r.sums == want
                assert [x[0] for x in r.results] == [E_ARG if i in bad else OK for i in range(n)]
        # a failed check in front of an invalid entry: the first in table order is reported
        r = call(lib, d, CRC32, d_in, in_len, [0, in_len + 5, 10], [10, 1, 10], 3,
                 expected=[zlib.crc32(blob[:10]) ^ 2, 0, zlib.crc32(blob[10:20])])
        assert (r.rc, r.block, r.n_failed, r.found, r.expected) == (E_CHECK, 0, 2, zlib.crc32(blob[:10]), zlib.crc32(blob[:10]) ^ 2)
        # n == 0
        r = call(lib, d, CRC32, d_in, in_len, [], [], 0)
        assert (r.rc, r.n_failed) == (OK, 0)
        r = call(lib, d, ADLER32, None, 0, [0], None, 0)
        assert (r.rc, r.n_failed) == (OK, 0)
        # the argument errors: nothing is launched, nothing written
        f = lib.L.gzpx_checksum_batch_device
        keep = []
        p_off = table(mem, keep, np.array([0, 10], dtype=np.uint64))[1]
        p_size = table(mem, keep, np.array([10, 10], dtype=np.uint32))[1]
        h_sums = table(mem, keep, np.full(2, 0xABCD, dtype=np.uint32))
        nf, info = ctypes.c_size_t(0), _native.GzpxCheckInfo()
        pnf, pinfo = ctypes.byref(nf), ctypes.byref(info)
        args = dict(ctx=d.h, kind=CRC32, d_in=d_in, in_len=in_len, off=p_off, size=p_size, n=1, seeds=None, exp=None,
                    sums=h_sums[1], res=None, nf=pnf, info=pinfo)
        order = ("ctx", "kind", "d_in", "in_len", "off", "size", "n", "seeds", "exp", "sums", "res", "nf", "info")
        assert f(*[args[k] for k in order], None) == OK
        assert np.frombuffer(mem.get(h_sums[0], 8), dtype=np.uint32).tolist() == [zlib.crc32(blob[:10]), 0xABCD]
        for change in (dict(ctx=None), dict(d_in=None), dict(off=None), dict(off=None, n=0), dict(nf=None), dict(info=None),
                       dict(kind=3), dict(kind=-1), dict(sums=None), dict(n=0xFFFFFFF1)):
            a = dict(args, **change)
            assert f(*[a[k] for k in order], None) == E_ARG, change
        assert np.frombuffer(mem.get(h_sums[0], 8), dtype=np.uint32).tolist() == [zlib.crc32(blob[:10]), 0xABCD]
        del keep
    del h


# ------------------------------------------------------------------------------------------------ 6. ragged
def ragged(lib, kind, n_small=20000, big=0, widths=(0,)):
    """Thousands of entries of 0 to 300 bytes, entries of 9 tiles + 5 bytes between them, runs of empty entries, and
    (big) one long entry: workgroups that start inside an entry, entries that reach across several workgroups,
    workgroups that hold hundreds of entries, empty entries at a workgroup's first and last tile."""
    rng = np.random.RandomState(12)
    long_len = 9 * TILE + 5
    n_long = 6
    blob_len = max(2 * long_len, big + 4096)
    blob = content("random", blob_len, 30)
    small = rng.randint(0, 301, n_small)
    pairs = []
    every = n_small // n_long
    for i, s in enumerate(small):
        if i % every == every // 2:
            pairs.append((int(rng.randint(0, blob_len - long_len)), long_len))
            pairs += [(int(rng.randint(0, blob_len)), 0)] * 70  # a run of empty entries behind a long one
        if i % 997 == 0:
            pairs += [(0, 0)] * 130
        pairs.append((int(rng.randint(0, blob_len - 300)), int(s)))
    if big:
        pairs.insert(len(pairs) // 3, (3, big))
    pairs = [(0, 0)] * 65 + pairs + [(blob_len, 0)] * 65
    offs, sizes = [p[0] for p in pairs], [p[1] for p in pairs]
    mem = scan_cases.Mem(lib)
    h, d_in = put_aligned(mem, blob, 5)
    with context(lib) as d:
        for width in widths:
            d.set_checksum_width(width)
            r = call(lib, d, kind, d_in, blob_len, offs, sizes, len(pairs), results=False)
            check_good(r, kind, blob, offs, sizes, what=(kind, "ragged", width))
    del h


# ------------------------------------------------------------------------------------------------ 7. 64-bit (GPU)
def beyond_4gib(lib):
    import pytest
    import torch
    head_n = tail_n = 100 * 1024
    total = (1 << 32) + 200 * 1024
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip("less than 6 GiB of device memory free")
    rng = np.random.RandomState(77)
    head, tail = rng.randint(0, 256, head_n, dtype=np.uint8), rng.randint(0, 256, tail_n, dtype=np.uint8)
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    buf[:head_n] = torch.from_numpy(head).cuda()
    buf[total - tail_n:] = torch.from_numpy(tail).cuda()
    head, tail = head.tobytes(), tail.tobytes()
    zeros = total - head_n - tail_n

    def at(pos, n):  # bytes of the buffer without having it on the host
        out = bytearray(n)
        for i in range(n):
            p = pos + i
            out[i] = head[p] if p < head_n else tail[p - (total - tail_n)] if p >= total - tail_n else 0
        return bytes(out)
    known_answers()

    def combine32(x, y, n):
        return _native.crc32_combine(x, y, n, lib=lib)
    whole = {
        # head || zeros || tail, the run of zeros by doubling
        CRC32: combine32(combine32(zlib.crc32(head), zeros_sum(zeros, zlib.crc32(bytes(1)), combine32), zeros), zlib.crc32(tail), tail_n),
        CRC32C: crc32c_combine(crc32c_combine(crc32c(head), zeros_sum(zeros, crc32c(bytes(1)), crc32c_combine), zeros),
                               crc32c(tail), tail_n),
        ADLER32: zlib.adler32(tail, adler32_zeros(zlib.adler32(head), zeros)),
    }
    e1 = at((1 << 32) + 5, 70001)
    e2 = at((1 << 32) - 65537, 131073)
    with context(lib) as d:
        for kind in (CRC32, ADLER32, CRC32C):
            r = call(lib, d, kind, buf.data_ptr(), total, [0, total], None, 1)  # the span form: an entry above 4 GiB
            assert r.rc == OK and r.sums == [whole[kind]], (kind, hex(r.sums[0]), hex(whole[kind]))
            assert r.results == [(OK, 0xFFFFFFFF, whole[kind], 0)]
            r = call(lib, d, kind, buf.data_ptr(), total, [(1 << 32) + 5, (1 << 32) - 65537], [70001, 131073], 2)
            assert r.rc == OK and r.sums == [reference(kind, e1), reference(kind, e2)], kind
    del buf


def zeros_sum(n, one, combine):
    """The CRC of n zero bytes from the CRC of one (`one`), by doubling through `combine`."""
    run, run_len, z, z_len = one, 1, 0, 0
    while n:
        if n & 1:
            z = combine(z, run, run_len) if z_len else run
            z_len += run_len
        run = combine(run, run, run_len)
        run_len *= 2
        n >>= 1
    return z


# ------------------------------------------------------------------------------------------------ 8. no read outside the input
def guard_child(lib_path):
    """(Emulator only: a device pointer is a host pointer.)  The input lies between two pages without access, flush
    against both at every misalignment: a load that leaves the aligned 16-byte words of the input ends the process."""
    lib = _native.GzpxLib(lib_path)
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mmap.restype = ctypes.c_void_p
    libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = os.sysconf("SC_PAGE_SIZE")
    npages = 40  # 160 KiB between the guards: entries of more than two tiles
    base = libc.mmap(None, (npages + 2) * page, 3, 0x22, -1, 0)  # PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS
    assert base not in (None, ctypes.c_void_p(-1).value)
    assert libc.mprotect(base, page, 0) == 0 and libc.mprotect(base + (npages + 1) * page, page, 0) == 0
    lo, room = base + page, npages * page
    fill = content("random", room, 2)
    ctypes.memmove(lo, fill, room)
    with context(lib) as d:
        for front in range(16):
            for back in range(16):
                if (front + back) % 5 and front != back:  # (every misalignment at both ends; a thinned cross product)
                    continue
                d_in, in_len = lo + front, room - front - back
                data = fill[front:front + in_len]
                # flush against the front, flush against the back, and the whole input
                pairs = [(0, 1), (0, 17), (0, 300), (0, 70000), (in_len - 1, 1), (in_len - 17, 17), (in_len - 300, 300),
                         (in_len - 70000, 70000), (in_len - 65536, 65536), (0, in_len), (in_len, 0), (0, 0)]
                offs = np.array([p[0] for p in pairs], dtype=np.uint64)
                sizes = np.array([p[1] for p in pairs], dtype=np.uint32)
                for kind in (CRC32, ADLER32, CRC32C):
                    sums = np.zeros(len(pairs), dtype=np.uint32)
                    assert d.checksum_batch_device(kind, d_in, in_len, offs.ctypes.data, sizes.ctypes.data, len(pairs),
                                                   d_sums_ptr=sums.ctypes.data) == (0, None)
                    assert sums.tolist() == [reference(kind, data[o:o + s]) for o, s in pairs], (kind, front, back)
    print("guard ok")


def no_read_outside_input(lib):
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import checksum_cases; checksum_cases.guard_child(%r)" % (
        here, os.path.dirname(here), lib.path)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "guard ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------ 9. stream order (GPU)
def stream_order(lib):
    """The bytes arrive by a copy on the caller's stream immediately in front of the call, which is handed that stream."""
    import torch
    n = 48 << 20
    src = torch.from_numpy(np.random.RandomState(6).randint(0, 256, n, dtype=np.uint8)).cuda()
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cuts = [0, 1 << 20, (1 << 20) + 3, 20 << 20, n]
    host = src.cpu().numpy().tobytes()
    want = [zlib.crc32(host[a:b]) for a, b in zip(cuts, cuts[1:])]
    offs = torch.tensor(cuts, dtype=torch.int64, device="cuda")
    sums = torch.zeros(len(want), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with context(lib) as d:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dst.copy_(src, non_blocking=True)
            assert d.checksum_batch_device(CRC32, dst.data_ptr(), n, offs.data_ptr(), None, len(want), d_sums_ptr=sums.data_ptr(),
                                           stream=s.cuda_stream) == (0, None)
        got = [int(v) & 0xFFFFFFFF for v in sums.cpu().tolist()]
        assert got == want
