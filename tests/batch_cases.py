"""Batches of raw / zlib / gzip members in device memory (gzpx_inflate_batch_device), written once and run twice:
through the emulated library on CPU (tests/test_emu_batch.py, where a device pointer is a host pointer) and through
the real HIP library on the MI355X (tests/test_gpu_batch.py).

Two yardsticks, never the library's own other entry points: Python's zlib for bytes and for making members, and the
verdict of libdeflate's gzip / zlib / deflate decompress calls as tests/golden/make_wrap_verdicts.py recorded it in
tests/golden/wrap_verdicts.json (0 OK, 1 BAD_DATA, 2 SHORT_OUTPUT, 3 INSUFFICIENT_SPACE).  INVALID_HEADER,
INVALID_CHECK and BAD_DATA all answer libdeflate's 1, a short output without SHORT_OK is BAD_DATA here and 2 there,
INSUFFICIENT_SPACE is 3; INVALID_ARG has no counterpart.  Members are cut exactly, so the rule "the trailer is the
member's last bytes" and libdeflate's "the trailer follows the final block" agree."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np

import inflate_cases
import scan_cases
from gzp_amd import _native, synth

RAW, ZLIB, GZIP = _native.WRAP_RAW, _native.WRAP_ZLIB, _native.WRAP_GZIP
WRAPS = {"raw": RAW, "zlib": ZLIB, "gzip": GZIP}
ROUTES = {"seg": _native.INFLATE_SEG, "wave": _native.INFLATE_WAVE}
OK, E_ARG, E_SPACE = _native.OK, _native.ERR_INVALID_ARG, _native.ERR_INSUFFICIENT_SPACE
E_HEADER, E_CHECK, E_BAD = _native.ERR_INVALID_HEADER, _native.ERR_INVALID_CHECK, _native.ERR_BAD_DATA
LD_ANSWERS = {0: (OK,), 1: (E_HEADER, E_CHECK, E_BAD), 2: (E_BAD,), 3: (E_SPACE,)}  # libdeflate's verdict -> ours
VERDICTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrap_verdicts.json")
GUARD = 64  # bytes behind the output that must stay as they were
SHIFT = 3   # d_in and d_out start this far into their allocations


# ------------------------------------------------------------------------------------------------ making members
def deflate(data, wrap, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_every=None):
    """One member as zlib makes it, in the wrapper's own framing."""
    wb = {RAW: -wbits, ZLIB: wbits, GZIP: 16 + wbits}[wrap]
    co = zlib.compressobj(level, zlib.DEFLATED, wb, 9, strategy)
    data = bytes(data)
    if flush_every is None:
        return co.compress(data) + co.flush()
    out = b""
    for i in range(0, len(data), flush_every):
        out += co.compress(data[i:i + flush_every]) + co.flush(zlib.Z_SYNC_FLUSH)
    return out + co.flush()


def rewrap(raw, data, wrap):
    """A raw DEFLATE stream that inflates to `data`, in the wrapper."""
    if wrap == RAW:
        return bytes(raw)
    if wrap == ZLIB:
        return b"\x78\x9c" + bytes(raw) + struct.pack(">I", zlib.adler32(data))
    return gzip_member(raw, data)


def gzip_member(raw, data, extra=None, name=None, comment=None, hcrc=None, text=False, flags_or=0, cm=8, magic=b"\x1f\x8b",
                crc=None, isize=None):
    """A gzip member around a raw stream with the header fields asked for; hcrc: None, "right" or "wrong"."""
    flg = (1 if text else 0) | (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | \
          (16 if comment is not None else 0) | flags_or
    h = magic + bytes([cm, flg]) + struct.pack("<IBB", 0, 0, 255)
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name
    if comment is not None:
        h += comment
    if hcrc:
        v = zlib.crc32(h) & 0xFFFF
        h += struct.pack("<H", v if hcrc == "right" else v ^ 0x0101)
    return h + bytes(raw) + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def reference_inflate(member, wrap):
    return zlib.decompress(member, {RAW: -15, ZLIB: 15, GZIP: 31}[wrap])


# ------------------------------------------------------------------------------------------------ one call
class Result:
    pass


def run(lib, d, wrap, members, out_sizes, order=None, out_cap=None, short_ok=False, offsets=True, results=True, table=None,
        tail=0, in_shift=SHIFT, seed=1):
    """One gzpx_inflate_batch_device call.  The members lie in memory in `order` (a permutation; default: reversed in
    pairs) with gaps of junk between them and `tail` junk bytes behind the last, and are listed in table order; d_in
    and d_out start SHIFT bytes into their allocations and GUARD bytes behind the output are watched.  `table`
    overrides table entries: {index: (offset, size)}.  out_sizes None: no size table (gzip)."""
    mem = scan_cases.Mem(lib)
    n = len(members)
    rng = np.random.RandomState(seed)
    if order is None:
        order = [i ^ 1 if (i ^ 1) < n else i for i in range(n)]
    offs = [0] * n
    blob = bytearray()
    for k, i in enumerate(order):
        blob += rng.randint(0, 256, 1 + (k * 7) % 38, dtype=np.uint8).tobytes()  # junk in front of every member
        offs[i] = len(blob)
        blob += members[i]
    blob += rng.randint(0, 256, tail, dtype=np.uint8).tobytes() if tail else b""
    sizes = [len(m) for m in members]
    for i, (o, s) in (table or {}).items():
        offs[i], sizes[i] = o, s
    in_len = len(blob)
    total = sum(out_sizes) if out_sizes is not None else None
    if out_cap is None:
        assert total is not None
        out_cap = total
    keep = [mem.put(bytes(blob), in_shift)]
    d_in = keep[0][1]
    h_out = np.full(out_cap + GUARD, 0xA5, dtype=np.uint8)
    keep.append(mem.put(h_out, SHIFT))
    out_handle, d_out = keep[-1]

    def table_ptr(a):
        keep.append(mem.put(np.ascontiguousarray(a).view(np.uint8)))
        return keep[-1]
    p_off = table_ptr(np.array(offs + [0], dtype=np.uint64))[1]
    p_size = table_ptr(np.array(sizes + [0], dtype=np.uint32))[1]
    p_osize = table_ptr(np.array(list(out_sizes) + [0], dtype=np.uint32))[1] if out_sizes is not None else None
    h_offs = table_ptr(np.full(n + 2, 0xABCD, dtype=np.uint64)) if offsets else (None, None)
    h_res = table_ptr(np.full(4 * (n + 1), 0xABCD, dtype=np.uint32)) if results else (None, None)
    r = Result()
    out_len, n_failed = ctypes.c_size_t(77), ctypes.c_size_t(77)
    info = _native.GzpxCheckInfo()
    r.rc = lib.L.gzpx_inflate_batch_device(d.h, wrap, 1 if short_ok else 0, d_in, in_len, p_off, p_size, p_osize, n, d_out,
                                           out_cap, h_offs[1], h_res[1], ctypes.byref(out_len), ctypes.byref(n_failed),
                                           ctypes.byref(info), None)
    r.out_len, r.n_failed, r.block, r.found, r.expected = out_len.value, n_failed.value, info.block, info.found, info.expected
    whole = np.frombuffer(mem.get(out_handle, SHIFT + out_cap + GUARD), dtype=np.uint8)
    assert (whole[:SHIFT] == 0).all(), "bytes in front of d_out were written"
    r.out = whole[SHIFT:SHIFT + out_cap].tobytes()
    r.guard_ok = bool((whole[SHIFT + out_cap:] == 0xA5).all())
    if offsets:
        a = np.frombuffer(mem.get(h_offs[0], 8 * (n + 2)), dtype=np.uint64)
        assert a[n + 1] == 0xABCD, "d_out_offsets written behind [n]"
        r.offsets = a[:n + 1].tolist()
    if results:
        a = np.frombuffer(mem.get(h_res[0], 16 * (n + 1)), dtype=np.uint32).reshape(n + 1, 4)
        assert (a[n] == 0xABCD).all(), "d_results written behind [n)"
        r.status, r.produced = a[:n, 0].tolist(), a[:n, 1].tolist()
        r.values = [(int(x[2]), int(x[3])) for x in a[:n]]
    del keep
    return r


def prefix(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def contexts(lib, routes=("seg", "wave")):
    for route in routes:
        # (any context serves, whatever format it was made for)
        with _native.DContext(format=_native.FORMAT_MGZIP if route == "wave" else _native.FORMAT_BGZF, lib=lib) as d:
            d.set_route(ROUTES[route])
            yield route, d


def check_all_good(r, plains, what):
    sizes = [len(p) for p in plains]
    assert r.rc == OK and r.n_failed == 0, (what, r.rc, r.n_failed, r.block, getattr(r, "status", None))
    assert r.out_len == sum(sizes), what
    assert r.offsets == prefix(sizes), what
    assert r.status == [OK] * len(plains) and r.produced == sizes, (what, r.status)
    assert r.out[:sum(sizes)] == b"".join(plains), (what, "bytes differ")
    assert r.guard_ok, (what, "bytes behind the output were written")


# ------------------------------------------------------------------------------------------------ 1. bytes
CLASSES = ("text", "dna", "random", "fastq", "mixed")
VARIANTS = (dict(level=6), dict(level=0), dict(level=1), dict(level=9), dict(level=6, strategy=zlib.Z_FIXED),
            dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY), dict(level=6, flush_every=37), dict(level=6, wbits=9))
SIZES = (40000, 0, 16385, 1, 150000, 17, 70000, 3000, 16384, 32769)  # 16384 / 16385: one and two k_lzcopy tiles


def _plain_members(sizes, wrap, seed=11):
    plains, members = [], []
    for k, n in enumerate(sizes):
        p = synth.make(CLASSES[k % len(CLASSES)], n, seed + k).tobytes()
        var = dict(VARIANTS[k % len(VARIANTS)])
        if var.get("flush_every") and n > 5000:  # (a sync flush every 37 bytes: on a small member)
            var = dict(level=6)
        plains.append(p)
        members.append(deflate(p, wrap, **var))
    return plains, members


def bytes_right(lib, wrap, sizes=SIZES, small=False):
    sizes = [s for s in sizes if not small or s <= 40000]
    plains, members = _plain_members(sizes, wrap)
    # every way of making a member is there at a size where it matters
    extra = synth.make("text", 3000, 5).tobytes()
    for var in VARIANTS:
        plains.append(extra)
        members.append(deflate(extra, wrap, **var))
    for p, m in zip(plains, members):
        assert reference_inflate(m, wrap) == p
    for route, d in contexts(lib):
        r = run(lib, d, wrap, members, [len(p) for p in plains])
        check_all_good(r, plains, (wrap, route))


def big_launch(lib, wrap, n=300000):
    """in_len / n >= 131072: the launch form with several waves per member (kSegBigW)."""
    plains = [synth.make(c, n, 3).tobytes() for c in ("random", "text", "mixed")]
    members = [deflate(p, wrap, level=lv) for p, lv in zip(plains, (6, 1, 6))]
    tail = max(0, 3 * inflate_cases.SEG_BIG_BYTES + 4096 - sum(len(m) for m in members))
    for route, d in contexts(lib):
        r = run(lib, d, wrap, members, [len(p) for p in plains], tail=tail)
        check_all_good(r, plains, (wrap, route, "big"))


# ------------------------------------------------------------------------------------------------ 2. one stream, two doors
def two_doors(lib, oracle, n=300000):
    for level in (1, 3):
        a = synth.make("mixed", n, 21)
        s = oracle.compress_stream(a, scan_cases.BGZF, level, oracle.COMPAT_1_24, 65280)
        s = bytes(s[0] if isinstance(s, tuple) else s)
        rc, nb, used, offs, sizes = scan_cases.host_scan(lib, scan_cases.BGZF, s)
        assert rc == OK and used == len(s) and sizes[-1] == scan_cases.EOF  # (the EOF marker: a legal empty member)
        members = [s[o:o + z] for o, z in zip(offs, sizes)]
        plains = [zlib.decompress(m, 31) for m in members]
        assert b"".join(plains) == a.tobytes()
        isz = [struct.unpack("<I", m[-4:])[0] for m in members]
        assert isz == [len(p) for p in plains]
        for route, d in contexts(lib):
            r = run(lib, d, GZIP, members, None, out_cap=len(a))  # the member table itself, sizes from the footers
            check_all_good(r, plains, ("gzip door", level, route))
            r = run(lib, d, RAW, [m[18:-8] for m in members], isz)
            check_all_good(r, plains, ("raw door", level, route))


# ------------------------------------------------------------------------------------------------ 3. + 4. headers
def _payload():
    data = synth.make("text", 2500, 9).tobytes()
    return data, deflate(data, RAW)


def gzip_header_cases():
    """(name, member, the status expected) -- every legal combination of header fields, then each malformed form."""
    data, raw = _payload()
    out = []
    for ei, extra in enumerate((None, b"", b"\x07", bytes(range(256)) + bytes(44))):
        for name in (None, b"file name.txt\x00"):
            for comment in (None, b"a comment, \xe9\x00"):
                for hcrc in (None, "right", "wrong"):
                    for text in (False, True):
                        tag = "ok x%d n%d c%d h%s t%d" % (ei, name is not None, comment is not None, hcrc or "no", text)
                        out.append((tag, gzip_member(raw, data, extra, name, comment, hcrc, text), OK))
    for bit in (32, 64, 128):
        out.append(("reserved %d" % bit, gzip_member(raw, data, flags_or=bit), E_HEADER))
    out.append(("cm 7", gzip_member(raw, data, cm=7), E_HEADER))
    out.append(("magic", gzip_member(raw, data, magic=b"\x1f\x8c"), E_HEADER))
    out.append(("wrong crc", gzip_member(raw, data, crc=zlib.crc32(data) ^ 0x400), E_CHECK))
    out.append(("wrong isize", gzip_member(raw, data, isize=len(data) + 1), E_CHECK))
    m = gzip_member(raw, data, name=b"never ends")
    out.append(("unterminated name", m[:13] + bytes(b or 1 for b in m[13:]), E_HEADER))
    out.append(("unterminated comment", gzip_member(b"\x01" * 40, data, comment=b"x" * 9).replace(b"\x00", b"\x01"), E_HEADER))
    out.append(("xlen past the end", gzip_member(raw, data, extra=b"ab")[:10] + struct.pack("<H", 60000) +
                gzip_member(raw, data, extra=b"ab")[12:], E_HEADER))
    out.append(("name ends in the trailer", gzip_member(b"", b"", name=b"nnnnnnnn")[:18] + b"\x01\x01\x01\x01\x00\x01\x01\x01", E_HEADER))
    out.append(("hcrc in the trailer", (gzip_member(b"", b"", hcrc="right")[:10] + bytes(8)), E_HEADER))
    return data, out


def zlib_header_cases():
    data, raw = _payload()
    good = rewrap(raw, data, ZLIB)
    adler = struct.pack(">I", zlib.adler32(data))

    def hdr(cmf, flg=None, fdict=0):
        if flg is None:
            flg = fdict | (31 - ((cmf << 8) | fdict) % 31) % 31
        return bytes([cmf, flg]) + raw + adler
    out = [("ok", good, OK), ("ok wbits 9", deflate(data, ZLIB, wbits=9), OK), ("ok level bits", hdr(0x78, 0xDA), OK),
           ("ok cinfo 0", hdr(0x08), OK),
           ("wrong fcheck", hdr(0x78, 0x9D), E_HEADER), ("fdict", hdr(0x78, fdict=0x20), E_HEADER),
           ("cinfo 8", hdr(0x88), E_HEADER), ("cm 7", hdr(0x77), E_HEADER),
           ("wrong adler", good[:-1] + bytes([good[-1] ^ 1]), E_CHECK)]
    assert out[1][1][:2] == b"\x18\x95"
    return data, out


def adler_buffers(big):
    """The buffers on which a sum of too few bits or a late reduction goes wrong: NMAX = 5552 and the modulus, in 0xFF."""
    out = [("ff %d" % n, b"\xff" * n) for n in (5551, 5552, 5553, 65520, 65521, 65522, big)]
    out.append(("zeros", bytes(70000)))
    out.append(("ramp", bytes(i & 255 for i in range(70001))))
    return out


def load_verdicts():
    with open(VERDICTS) as f:
        return {v["case"]: v for v in json.load(f)["verdicts"]}


def recorded_cases():
    """(case name, wrap, member, room) of everything whose libdeflate verdict the golden file holds."""
    data, g = gzip_header_cases()
    for name, m, _ in g:
        yield "gzip " + name, GZIP, m, len(data)
    data, z = zlib_header_cases()
    for name, m, _ in z:
        yield "zlib " + name, ZLIB, m, len(data)
    for w in ("raw", "zlib", "gzip"):
        plains, members, _ = local_members(WRAPS[w])
        for i in LOCAL_DAMAGED:
            yield "local %s %d" % (w, i), WRAPS[w], members[i], len(plains[i])
    data, raw = _payload()
    for w in ("raw", "zlib", "gzip"):
        m = rewrap(raw, data, WRAPS[w])
        yield "room %s +1" % w, WRAPS[w], m, len(data) + 1
        yield "room %s -1" % w, WRAPS[w], m, len(data) - 1


def _verdict(verdicts, case, member):
    v = verdicts[case]
    assert v["sha256"] == hashlib.sha256(member).hexdigest(), (case, "the member is not the one the verdict was recorded for")
    return v["rc"]


def headers(lib, wrap):
    verdicts = load_verdicts()
    data, cases = gzip_header_cases() if wrap == GZIP else zlib_header_cases()
    tag = "gzip " if wrap == GZIP else "zlib "
    for name, m, want in cases:
        assert want in LD_ANSWERS[_verdict(verdicts, tag + name, m)], (name, "the expectation contradicts libdeflate")
    members = [m for _, m, _ in cases]
    for route, d in contexts(lib):
        r = run(lib, d, wrap, members, [len(data)] * len(members))
        bad = [i for i, (_, _, want) in enumerate(cases) if want != OK]
        assert r.status == [want for _, _, want in cases], (route, [(cases[i][0], r.status[i]) for i in range(len(cases)) if r.status[i] != cases[i][2]])
        assert r.n_failed == len(bad) and r.rc == cases[bad[0]][2] and r.block == bad[0], (route, r.rc, r.block)
        assert r.offsets == prefix([len(data)] * len(members)) and r.guard_ok
        for i, (name, _, want) in enumerate(cases):  # the good members of the same batch are still right
            if want == OK:
                assert r.out[i * len(data):(i + 1) * len(data)] == data, (route, name)
        i = [c[0] for c in cases].index("wrong isize") if wrap == GZIP else None
        if i is not None:
            assert r.values[i] == (len(data) + 1, len(data))


def adler_edges(lib, big):
    for route, d in contexts(lib):
        plains, members, flipped = [], [], []
        for name, buf in adler_buffers(big):
            for level in (0, 6):
                m = deflate(buf, ZLIB, level=level)
                plains += [buf, buf]
                members += [m, m[:-2] + bytes([m[-2] ^ 0x10]) + m[-1:]]
                flipped += [False, True]
        r = run(lib, d, ZLIB, members, [len(p) for p in plains])
        assert r.status == [E_CHECK if f else OK for f in flipped], (route, r.status)
        for i, f in enumerate(flipped):
            if f:
                assert r.values[i] == (zlib.adler32(plains[i]), struct.unpack(">I", members[i][-4:])[0]), (route, i)
        assert r.rc == E_CHECK and r.block == 1 and (r.found, r.expected) == r.values[1]
        assert r.out[:sum(len(p) for p in plains)] == b"".join(plains) and r.guard_ok


def adler_host_call(lib, big):
    for name, buf in adler_buffers(big):
        for running in (1, 0x12345678 % 65521 | (77 << 16)):
            assert _native.adler32(buf, running, lib=lib) == zlib.adler32(buf, running), (name, running)


# ------------------------------------------------------------------------------------------------ 5. failures stay local
LOCAL_DAMAGED = (7, 8, 31)


def local_members(wrap):
    """40 members; 7: the first block's type made the reserved one (one bit of a dynamic block's header), 8: one
    trailer byte changed (raw has no trailer: its member 8 stays good), 31: cut short by 5 bytes."""
    plains = [synth.make(CLASSES[(i + 3) % 5], 1500 + 211 * i, 60 + i).tobytes() for i in range(40)]
    members = [deflate(p, wrap) for p in plains]
    hdr = {RAW: 0, ZLIB: 2, GZIP: 10}[wrap]
    m = bytearray(members[7])
    assert m[hdr] & 7 == 5  # BFINAL, BTYPE = 2: dynamic
    m[hdr] ^= 2
    members[7] = bytes(m)
    if wrap != RAW:
        m = bytearray(members[8])
        m[-3] ^= 0x80
        members[8] = bytes(m)
    members[31] = members[31][:-5]
    return plains, members, hdr


def failures_stay_local(lib, wrap):
    verdicts = load_verdicts()
    plains, members, _ = local_members(wrap)
    w = {RAW: "raw", ZLIB: "zlib", GZIP: "gzip"}[wrap]
    sizes = [len(p) for p in plains]
    want = {}
    for i in LOCAL_DAMAGED:
        want[i] = LD_ANSWERS[_verdict(verdicts, "local %s %d" % (w, i), members[i])]
    if wrap != RAW:
        want[8] = (E_CHECK,)
    want[7] = (E_BAD,)
    want[12] = (E_ARG,)
    want[39] = (E_SPACE,)
    for route, d in contexts(lib):
        in_len = len(b"".join(members)) + sum(1 + (k * 7) % 38 for k in range(40))  # (run()'s layout)
        r = run(lib, d, wrap, members, sizes, out_cap=sum(sizes) - 1, table={12: (in_len - 3, 100)})
        for i in range(40):
            assert r.status[i] in want.get(i, (OK,)), (w, route, i, r.status[i])
        failed = [i for i in range(40) if r.status[i] != OK]
        assert r.n_failed == len(failed) and r.block == failed[0] and r.rc == r.status[failed[0]], (w, route, r.rc, r.block)
        assert failed[0] == 7 and set(failed) >= {7, 12, 31, 39}
        assert r.offsets == prefix(sizes) and r.out_len == sum(sizes), (w, route)  # the plain prefix sum, whoever failed
        assert r.guard_ok, (w, route)
        off = prefix(sizes)
        for i in range(40):
            if r.status[i] == OK:
                assert r.out[off[i]:off[i + 1]] == plains[i], (w, route, i)
                assert r.produced[i] == sizes[i]
        if wrap != RAW:
            assert r.values[8][0] != r.values[8][1]


# ------------------------------------------------------------------------------------------------ 6. sizes
def sizes_and_flags(lib):
    verdicts = load_verdicts()
    data, raw = _payload()
    n = len(data)
    for route, d in contexts(lib):
        for w, wrap in WRAPS.items():
            m = rewrap(raw, data, wrap)
            assert LD_ANSWERS[_verdict(verdicts, "room %s +1" % w, m)] == (E_BAD,)
            assert LD_ANSWERS[_verdict(verdicts, "room %s -1" % w, m)] == (E_SPACE,)
            if wrap == GZIP:  # the size is the trailer's: explicit sizes equal and unequal to it
                r = run(lib, d, wrap, [m, m, m], [n, n + 1, n - 1])
                assert r.status == [OK, E_CHECK, E_CHECK] and r.values[1] == (n, n + 1) and r.values[2] == (n, n - 1)
                assert r.produced[1:] == [0, 0] and r.offsets == [0, n, 2 * n + 1, 3 * n] and r.out[:n] == data
                lie_more = gzip_member(raw, data, isize=n + 1)
                lie_less = gzip_member(raw, data, isize=n - 1)
                r = run(lib, d, wrap, [lie_more, m, lie_less], None, out_cap=3 * n)
                assert r.status == [E_BAD, OK, E_SPACE] and r.offsets == [0, n + 1, 2 * n + 1, 3 * n], (route, r.status)
                assert r.out[n + 1:2 * n + 1] == data and r.guard_ok
            else:
                r = run(lib, d, wrap, [m, m, m], [n + 1, n, n - 1])
                assert r.status == [E_BAD, OK, E_SPACE] and r.out[n + 1:2 * n + 1] == data, (w, route, r.status)
                assert r.rc == E_BAD and r.block == 0 and r.n_failed == 2 and r.guard_ok
                # capacities: +1, +1000 and exact
                r = run(lib, d, wrap, [m, m, m, m], [n + 1, n + 1000, n, n - 1], short_ok=True)
                assert r.status == [OK, OK, OK, E_SPACE] and r.produced[:3] == [n, n, n], (w, route, r.status, r.produced)
                off = prefix([n + 1, n + 1000, n, n - 1])
                assert r.offsets == off and all(r.out[off[i]:off[i] + n] == data for i in range(3)) and r.guard_ok
                if wrap == ZLIB:  # the Adler-32 is taken over the bytes produced, not over the capacity
                    bad = m[:-1] + bytes([m[-1] ^ 4])
                    r = run(lib, d, wrap, [bad, m], [n + 9, n + 9], short_ok=True)
                    assert r.status == [E_CHECK, OK] and r.values[0] == (zlib.adler32(data), zlib.adler32(data) ^ 4)
        # the refusals of the flag, and of a missing size table where no trailer states one
        m = rewrap(raw, data, GZIP)
        for wrap, osz, short in ((GZIP, [n], True), (GZIP, None, True), (RAW, None, False), (ZLIB, None, False), (ZLIB, None, True)):
            r = run(lib, d, wrap, [m], osz, out_cap=n, short_ok=short)
            assert r.rc == E_ARG and r.n_failed == 0 and r.out_len == 0 and r.out == b"\xa5" * n, (wrap, osz, short)
        r = run(lib, d, 3, [m], [n])
        assert r.rc == E_ARG
        # n == 0; no offsets, no results
        r = run(lib, d, ZLIB, [], [], out_cap=16)
        assert r.rc == OK and r.out_len == 0 and r.n_failed == 0 and r.offsets == [0] and r.out == b"\xa5" * 16
        z = rewrap(raw, data, ZLIB)
        bad = z[:-1] + bytes([z[-1] ^ 1])
        r = run(lib, d, ZLIB, [z, bad], [n, n], offsets=False, results=False)
        assert r.rc == E_CHECK and r.block == 1 and r.n_failed == 1 and r.out_len == 2 * n and r.out[:n] == data
        assert (r.found, r.expected) == (zlib.adler32(data), zlib.adler32(data) ^ 1)
        # the Python call
        mem = scan_cases.Mem(lib)
        keep = [mem.put(z + bad), mem.put(np.array([0, len(z)], dtype=np.uint64).view(np.uint8)),
                mem.put(np.array([len(z), len(bad)], dtype=np.uint32).view(np.uint8)),
                mem.put(np.array([n, n], dtype=np.uint32).view(np.uint8)), mem.empty(2 * n)]
        args = (keep[0][1], len(z) + len(bad), keep[1][1], keep[2][1], keep[3][1])
        assert d.inflate_batch_device(ZLIB, *args, 1, keep[4][1], 2 * n) == (n, 0)
        assert d.inflate_batch_device(ZLIB, *args, 2, keep[4][1], 2 * n, raise_on_member_error=False) == (2 * n, 1, 1)
        try:
            d.inflate_batch_device(ZLIB, *args, 2, keep[4][1], 2 * n)
            raise AssertionError("no error for a failing member")
        except _native.GzpxError as e:
            assert (e.code, e.block) == (E_CHECK, 1)
        assert mem.get(keep[4][0], n) == data


# ------------------------------------------------------------------------------------------------ 7. crafted streams
def crafted(lib, wrap, sample=None):
    """The accepted and the rejected streams of tests/inflate_cases.py as members of one batch: verdict and bytes as
    tests/golden/inflate_verdicts.json records libdeflate's."""
    verdicts = inflate_cases.load_verdicts()
    cases = inflate_cases.cases()
    if sample:
        cases = cases[::sample]
    want, outs, members = [], [], []
    for x in cases:
        code, out = inflate_cases._expect(verdicts[x.name], x)
        want.append(OK if code is None else code)
        outs.append(out if code is None else None)
        members.append(rewrap(x.raw, out or b"", wrap))
    sizes = [x.isize for x in cases]
    off = prefix(sizes)
    for route, d in contexts(lib):
        r = run(lib, d, wrap, members, sizes)
        diff = [(x.name, r.status[i], want[i]) for i, x in enumerate(cases) if r.status[i] != want[i]]
        assert not diff, (wrap, route, diff)
        for i, x in enumerate(cases):
            if want[i] == OK:
                assert r.out[off[i]:off[i + 1]] == outs[i], (wrap, route, x.name)
        assert r.n_failed == sum(1 for c in want if c != OK) and r.guard_ok and r.offsets == off


# ------------------------------------------------------------------------------------------------ 8. no read past the input
def guard_child(lib_path):
    """(Emulator only: a device pointer is a host pointer.)  The input lies so that its last byte is the last byte in
    front of a page without access; any load of compressed bytes that leaves the aligned 16-byte words of the input
    ends the process."""
    lib = _native.GzpxLib(lib_path)
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mmap.restype = ctypes.c_void_p
    libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = os.sysconf("SC_PAGE_SIZE")
    npages = 4
    base = libc.mmap(None, (npages + 1) * page, 3, 0x22, -1, 0)  # PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS
    assert base not in (None, ctypes.c_void_p(-1).value)
    assert libc.mprotect(base + npages * page, page, 0) == 0
    plains = [synth.make(c, n, 31).tobytes() for c, n in (("text", 5000), ("random", 300), ("dna", 2000), ("mixed", 3000))]
    for wrap in (RAW, ZLIB):
        for last_level in (6, 0):  # the last member ends in a Huffman block / in a stored block
            members = [deflate(p, wrap, level=last_level if i == 3 else 6) for i, p in enumerate(plains)]
            blob = b"".join(members)
            assert len(blob) < npages * page
            d_in = base + npages * page - len(blob)
            ctypes.memmove(d_in, blob, len(blob))
            offs = np.array(prefix([len(m) for m in members])[:-1], dtype=np.uint64)
            sizes = np.array([len(m) for m in members], dtype=np.uint32)
            osz = np.array([len(p) for p in plains], dtype=np.uint32)
            total = int(osz.sum())
            for route, d in contexts(lib):
                out = np.zeros(total + 16, dtype=np.uint8)
                res = d.inflate_batch_device(wrap, d_in, len(blob), offs.ctypes.data, sizes.ctypes.data, osz.ctypes.data, 4,
                                             out.ctypes.data, total)
                assert res == (total, 0) and out[:total].tobytes() == b"".join(plains), (wrap, route)
    print("guard ok")


def no_read_past_input(lib):
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import batch_cases; batch_cases.guard_child(%r)" % (
        here, os.path.dirname(here), lib.path)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "guard ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
