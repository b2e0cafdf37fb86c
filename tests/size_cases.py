"""The size query of a batch of raw / zlib / gzip members (gzpx_inflate_batch_sizes_device), written once and run
twice: through the emulated library on CPU (tests/test_emu_sizes.py) and through the real HIP library on the MI355X
(tests/test_gpu_sizes.py).

Two yardsticks, never the library's own other entry points: Python's zlib (the bytes a member inflates to, and
len(member) - len(unused_data) for its length) and what libdeflate's *_decompress_ex calls answered with both
actual_*_ret pointers, as tests/golden/make_size_verdicts.py recorded it in tests/golden/size_verdicts.json.  The one
exception is the round trip, where gzpx_inflate_batch_device behind the size query is part of what is tested."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np

import batch_cases
import inflate_cases
import scan_cases
from batch_cases import E_ARG, E_BAD, E_HEADER, E_SPACE, GZIP, LD_ANSWERS, OK, RAW, SHIFT, WRAPS, ZLIB, contexts, deflate, prefix, rewrap
from gzp_amd import _native, synth

VERDICTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "size_verdicts.json")
ROOM = 1 << 20  # the room libdeflate was given for every recorded member, and the cap the tests pass for them
HDR = {RAW: 0, ZLIB: 2, GZIP: 10}
TRAILER = {RAW: 0, ZLIB: 4, GZIP: 8}
WNAME = {RAW: "raw", ZLIB: "zlib", GZIP: "gzip"}
MARK = 0xABCD


# ------------------------------------------------------------------------------------------------ one call
class Result:
    pass


def layout(members, order=None, tail=0, seed=1):
    """The members in memory in `order` (default: reversed in pairs) with junk in front of each and `tail` junk bytes
    behind the last: (blob, offsets in table order)."""
    n = len(members)
    rng = np.random.RandomState(seed)
    if order is None:
        order = [i ^ 1 if (i ^ 1) < n else i for i in range(n)]
    offs = [0] * n
    blob = bytearray()
    for k, i in enumerate(order):
        blob += rng.randint(0, 256, 1 + (k * 7) % 38, dtype=np.uint8).tobytes()
        offs[i] = len(blob)
        blob += members[i]
    blob += rng.randint(0, 256, tail, dtype=np.uint8).tobytes() if tail else b""
    return bytes(blob), offs


def loose_sizes(blob, offs, members, plus_one=None):
    """Every entry runs to the start of the member that follows it in memory, or to in_len; `plus_one`: that entry
    runs one byte past its member's last."""
    starts = sorted(offs) + [len(blob)]
    nxt = {o: starts[k + 1] for k, o in enumerate(starts[:-1])}
    sizes = [nxt[o] - o for o in offs]
    if plus_one is not None:
        sizes[plus_one] = len(members[plus_one]) + 1
    return sizes


def call(lib, d, wrap, blob, offs, sizes, max_out=0, used=True, results=True, in_shift=SHIFT, out_sizes=True):
    """One gzpx_inflate_batch_sizes_device call on a table; every written table has a spare entry that must stay."""
    mem = scan_cases.Mem(lib)
    n = len(offs)
    keep = [mem.put(blob, in_shift)]
    d_in = keep[0][1]

    def table(a):
        keep.append(mem.put(np.ascontiguousarray(a).view(np.uint8)))
        return keep[-1]
    p_off = table(np.array(list(offs) + [0], dtype=np.uint64))[1]
    p_size = table(np.array(list(sizes) + [0], dtype=np.uint32))[1]
    h_osz = table(np.full(n + 1, MARK, dtype=np.uint32)) if out_sizes else (None, None)
    h_used = table(np.full(n + 1, MARK, dtype=np.uint32)) if used else (None, None)
    h_res = table(np.full(4 * (n + 1), MARK, dtype=np.uint32)) if results else (None, None)
    r = Result()
    total, n_failed = ctypes.c_uint64(77), ctypes.c_size_t(77)
    info = _native.GzpxCheckInfo()
    r.rc = lib.L.gzpx_inflate_batch_sizes_device(d.h, wrap, d_in, len(blob), p_off, p_size, n, max_out, h_osz[1], h_used[1],
                                                 h_res[1], ctypes.byref(total), ctypes.byref(n_failed), ctypes.byref(info), None)
    r.total, r.n_failed, r.block = total.value, n_failed.value, info.block
    r.guard_ok = True
    if out_sizes:
        a = np.frombuffer(mem.get(h_osz[0], 4 * (n + 1)), dtype=np.uint32)
        r.guard_ok = r.guard_ok and a[n] == MARK
        r.out_sizes = a[:n].tolist()
    if used:
        a = np.frombuffer(mem.get(h_used[0], 4 * (n + 1)), dtype=np.uint32)
        r.guard_ok = r.guard_ok and a[n] == MARK
        r.in_used = a[:n].tolist()
    if results:
        a = np.frombuffer(mem.get(h_res[0], 16 * (n + 1)), dtype=np.uint32).reshape(n + 1, 4)
        r.guard_ok = r.guard_ok and bool((a[n] == MARK).all())
        r.status = a[:n, 0].tolist()
        r.rows = [tuple(int(v) for v in x) for x in a[:n]]
    r.d_in, r.p_off, r.p_size, r.p_osz, r.p_used, r.keep, r.mem = d_in, p_off, p_size, h_osz[1], h_used[1], keep, mem
    return r


def check_all_good(r, plains, members, what):
    sizes = [len(p) for p in plains]
    assert r.rc == OK and r.n_failed == 0, (what, r.rc, r.n_failed, r.block, getattr(r, "status", None))
    assert r.out_sizes == sizes, (what, [(i, a, b) for i, (a, b) in enumerate(zip(r.out_sizes, sizes)) if a != b])
    assert r.in_used == [len(m) for m in members], (what, [(i, a, len(m)) for i, (a, m) in enumerate(zip(r.in_used, members)) if a != len(m)])
    assert r.rows == [(OK, len(p), len(m), 0) for p, m in zip(plains, members)], what
    assert r.total == sum(sizes), what
    assert r.guard_ok, (what, "a table was written behind [n)")


# ------------------------------------------------------------------------------------------------ members
SIZES = (0, 1, 258, 259, 4095, 4096, 4097, 16383, 16384, 16385, 32769, 65280, 70000)


def plain_members(wrap, sizes=SIZES, seed=11):
    """Members of every plain size, the ways of making one cycling over them; every way once more on 3,000 bytes of
    text; and a member that is one stored block."""
    plains, members = [], []
    for k, n in enumerate(sizes):
        p = synth.make(batch_cases.CLASSES[k % len(batch_cases.CLASSES)], n, seed + k).tobytes()
        var = dict(batch_cases.VARIANTS[k % len(batch_cases.VARIANTS)])
        if var.get("flush_every") and n > 5000:
            var = dict(level=6)
        plains.append(p)
        members.append(deflate(p, wrap, **var))
    extra = synth.make("text", 3000, 5).tobytes()
    for var in batch_cases.VARIANTS:
        plains.append(extra)
        members.append(deflate(extra, wrap, **var))
    stored = synth.make("random", 700, 8).tobytes()
    plains.append(stored)
    members.append(deflate(stored, wrap, level=0))
    return plains, members


def zlib_says(member, wrap):
    """(bytes out, bytes of the member used) by Python's zlib."""
    do = zlib.decompressobj({RAW: -15, ZLIB: 15, GZIP: 31}[wrap])
    out = do.decompress(member)
    assert do.eof
    return len(out), len(member) - len(do.unused_data)


def load_verdicts():
    with open(VERDICTS) as f:
        return {v["case"]: v for v in json.load(f)["verdicts"]}


def _verdict(verdicts, case, member):
    v = verdicts[case]
    assert v["sha256"] == hashlib.sha256(member).hexdigest(), (case, "the member is not the one the verdict was recorded for")
    return v


def crafted_members(wrap):
    """(case name, member): inflate_cases.cases() in the wrapper.  The trailer of a zlib member is the Adler-32 of no
    bytes: the size query verifies none."""
    return [("crafted %s %s" % (WNAME[wrap], x.name), rewrap(x.raw, b"", wrap)) for x in inflate_cases.cases()]


LOCAL = {5: "arg", 9: "header", 17: "truncated", 23: "code", 31: "trailer"}


def local_members(wrap):
    """40 members; 9: the wrapper's header damaged (RAW has none: the reserved block type), 17: cut in the middle,
    23: the first block's type made the reserved one, 31: the last byte cut off (ZLIB / GZIP: of the trailer)."""
    plains = [synth.make(batch_cases.CLASSES[(i + 3) % 5], 1500 + 211 * i, 60 + i).tobytes() for i in range(40)]
    members = [deflate(p, wrap) for p in plains]
    hdr = HDR[wrap]
    m = bytearray(members[9])
    if wrap == RAW:
        m[0] |= 6  # BTYPE = 3
    elif wrap == ZLIB:
        m[0] = 0x77  # CM = 7
    else:
        m[1] = 0x8C
    members[9] = bytes(m)
    members[17] = members[17][:len(members[17]) // 2]
    m = bytearray(members[23])
    m[hdr] |= 6  # BTYPE = 3
    members[23] = bytes(m)
    members[31] = members[31][:-1]
    return plains, members


def recorded_cases():
    """(case name, wrap, member) of everything whose libdeflate answer the golden file holds."""
    for w in (RAW, ZLIB, GZIP):
        _, members = plain_members(w)
        for i, m in enumerate(members):
            yield "plain %s %d" % (WNAME[w], i), w, m
        _, members = local_members(w)
        for i in LOCAL:
            if LOCAL[i] != "arg":
                yield "local %s %d" % (WNAME[w], i), w, members[i]
    for w in (RAW, ZLIB):
        for name, m in crafted_members(w):
            yield name, w, m


# ------------------------------------------------------------------------------------------------ 1. sizes right
def sizes_right(lib, wrap, small=False):
    plains, members = plain_members(wrap, [s for s in SIZES if not small or s <= 33000])
    for p, m in zip(plains, members):
        assert zlib_says(m, wrap) == (len(p), len(m))
    blob, offs = layout(members)
    for route, d in contexts(lib):
        r = call(lib, d, wrap, blob, offs, [len(m) for m in members])
        check_all_good(r, plains, members, (wrap, route))


# ------------------------------------------------------------------------------------------------ 2. loose extents
def loose_extents(lib, wrap, small=False):
    plains, members = plain_members(wrap, [s for s in SIZES if not small or s <= 17000])
    n = len(members)
    blob, offs = layout(members, tail=23)
    sizes = loose_sizes(blob, offs, members, plus_one=3)
    assert all(s > len(m) for s, m in zip(sizes, members)) and max(o + s for o, s in zip(offs, sizes)) == len(blob)
    for route, d in contexts(lib):
        r = call(lib, d, wrap, blob, offs, sizes)
        check_all_good(r, plains, members, (wrap, route, "loose"))
        # the inflate call on the same table: strict about extents, as documented, so the loose entries fail their
        # checks where the wrapper carries one; with the lengths the size query found they pass
        total = sum(len(p) for p in plains)
        out = r.mem.empty(total + 1)
        got = d.inflate_batch_device(wrap, r.d_in, len(blob), r.p_off, r.p_size, r.p_osz, n, out[1], total,
                                     raise_on_member_error=False)
        if wrap == RAW:
            assert got == (total, 0, None), (route, got)
        else:
            assert got[1] == n and got[2] == 0, (wrap, route, got)
        got = d.inflate_batch_device(wrap, r.d_in, len(blob), r.p_off, r.p_used, r.p_osz, n, out[1], total)
        assert got == (total, 0) and r.mem.get(out[0], total) == b"".join(plains), (wrap, route)


# ------------------------------------------------------------------------------------------------ 3. round trip
def round_trip(lib, wrap, small=False):
    """Nothing known but where the members start: sizes, the prefix (here: just the total), then the inflate call."""
    plains, members = plain_members(wrap, [s for s in SIZES if not small or s <= 17000], seed=40)
    n = len(members)
    blob, offs = layout(members, order=list(range(n))[::-1], tail=5)
    sizes = loose_sizes(blob, offs, members)
    for route, d in contexts(lib):
        r = call(lib, d, wrap, blob, offs, sizes, results=False)
        assert r.rc == OK and r.n_failed == 0 and r.total == sum(len(p) for p in plains), (wrap, route, r.rc, r.block)
        out = r.mem.empty(r.total + 64)
        res = r.mem.put(np.zeros(16 * n, dtype=np.uint8))
        got = d.inflate_batch_device(wrap, r.d_in, len(blob), r.p_off, r.p_used, r.p_osz, n, out[1], r.total, None, res[1])
        assert got == (r.total, 0), (wrap, route, got)
        assert r.mem.get(out[0], r.total) == b"".join(plains), (wrap, route)
        rows = np.frombuffer(r.mem.get(res[0], 16 * n), dtype=np.uint32).reshape(n, 4)
        assert rows[:, 0].tolist() == [OK] * n and rows[:, 1].tolist() == [len(p) for p in plains]


# ------------------------------------------------------------------------------------------------ 4. several waves per member
def big_launch(lib, wrap, n=300000):
    plains = [synth.make(c, n, 3).tobytes() for c in ("random", "text", "mixed")]
    members = [deflate(p, wrap, level=lv) for p, lv in zip(plains, (6, 1, 6))]
    tail = max(0, 3 * inflate_cases.SEG_BIG_BYTES + 4096 - sum(len(m) for m in members))
    blob, offs = layout(members, tail=tail)
    assert len(blob) // 3 >= inflate_cases.SEG_BIG_BYTES
    for sizes in ([len(m) for m in members], loose_sizes(blob, offs, members)):
        for route, d in contexts(lib):
            r = call(lib, d, wrap, blob, offs, sizes)
            check_all_good(r, plains, members, (wrap, route, "big"))


# ------------------------------------------------------------------------------------------------ 5. crafted streams
def crafted(lib, wrap, sample=None):
    verdicts = load_verdicts()
    cases = crafted_members(wrap)
    if sample:  # (the matches that reach the member's first byte and one in front of it are in every sample)
        cases = cases[::sample] + [c for i, c in enumerate(cases) if i % sample and " distance_" in c[0]]
    members = [m for _, m in cases]
    vs = [_verdict(verdicts, name, m) for name, m in cases]
    names = [name.split()[-1] for name, _ in cases]
    assert vs[names.index("distance_one_before_start")]["rc"] == 1 and vs[names.index("distance_to_start")]["rc"] == 0
    blob, offs = layout(members)
    for route, d in contexts(lib):
        r = call(lib, d, wrap, blob, offs, [len(m) for m in members], max_out=ROOM)
        diff = [(name, r.status[i], v["rc"]) for i, ((name, _), v) in enumerate(zip(cases, vs)) if r.status[i] not in LD_ANSWERS[v["rc"]]]
        assert not diff, (wrap, route, diff)
        for i, ((name, _), v) in enumerate(zip(cases, vs)):
            if v["rc"] == 0:
                assert (r.out_sizes[i], r.in_used[i]) == (v["actual_out"], v["actual_in"]), (wrap, route, name, r.rows[i], v)
            else:
                assert r.rows[i][1:] == (0, 0, 0) and r.out_sizes[i] == 0 and r.in_used[i] == 0, (wrap, route, name)
        assert r.status[names.index("distance_one_before_start")] == E_BAD, (wrap, route)  # BAD_DATA, not a size
        good = [v["actual_out"] for v in vs if v["rc"] == 0]
        assert r.n_failed == len(vs) - len(good) and r.total == sum(good) and r.guard_ok


# ------------------------------------------------------------------------------------------------ 6. failures stay local
def failures_stay_local(lib, wrap):
    verdicts = load_verdicts()
    plains, members = local_members(wrap)
    blob, offs = layout(members)
    sizes = [len(m) for m in members]
    offs[5], sizes[5] = len(blob) - 3, 100
    want = {5: E_ARG, 9: E_BAD if wrap == RAW else E_HEADER, 17: E_BAD, 23: E_BAD, 31: E_BAD}
    for i, why in LOCAL.items():
        if why != "arg":
            v = _verdict(verdicts, "local %s %d" % (WNAME[wrap], i), members[i])
            assert want[i] in LD_ANSWERS[v["own_rc" if why == "header" else "rc"]], (i, why)  # (a header is the wrapper's own call's to judge)
    good = [i for i in range(40) if i not in want]
    for i in good:
        assert zlib_says(members[i], wrap) == (len(plains[i]), len(members[i]))
    for route, d in contexts(lib):
        r = call(lib, d, wrap, blob, offs, sizes)
        assert [r.status[i] for i in sorted(want)] == [want[i] for i in sorted(want)], (wrap, route, r.status)
        for i in want:
            assert r.out_sizes[i] == 0 and r.in_used[i] == 0 and r.rows[i][1:] == (0, 0, 0), (wrap, route, i)
        for i in good:
            assert r.rows[i] == (OK, len(plains[i]), len(members[i]), 0), (wrap, route, i, r.rows[i])
        assert r.n_failed == 5 and r.block == 5 and r.rc == E_ARG, (wrap, route, r.n_failed, r.block, r.rc)
        assert r.total == sum(len(plains[i]) for i in good) and r.guard_ok


# ------------------------------------------------------------------------------------------------ 7. max_out_size
def max_out_size(lib, count_steps=False):
    plains = [synth.make("text", 999, 2).tobytes(), bytes(1000), synth.make("dna", 400, 3).tobytes(), b""]
    bomb = bytes(65536)
    for w, wrap in sorted(WRAPS.items()):
        members = [deflate(p, wrap) for p in plains]
        blob, offs = layout(members)
        sizes = [len(m) for m in members]
        zbomb = deflate(bomb, wrap, level=9)
        assert len(zbomb) < 120
        for route, d in contexts(lib):
            r = call(lib, d, wrap, blob, offs, sizes, max_out=999)
            assert r.status == [OK, E_SPACE, OK, OK] and r.rc == E_SPACE and r.block == 1 and r.n_failed == 1, (w, route, r.status)
            assert r.out_sizes == [999, 0, 400, 0] and r.in_used == [sizes[0], 0, sizes[2], sizes[3]] and r.total == 1399
            r = call(lib, d, wrap, blob, offs, sizes, max_out=1000)
            check_all_good(r, plains, members, (w, route, "cap 1000"))
            r = call(lib, d, wrap, zbomb, [0], [len(zbomb)], max_out=4096)
            assert r.status == [E_SPACE] and r.rows[0][1:] == (0, 0, 0) and r.total == 0, (w, route, r.rows)
            r = call(lib, d, wrap, zbomb, [0], [len(zbomb)], max_out=65536)
            assert r.rows == [(OK, 65536, len(zbomb), 0)], (w, route, r.rows)
    if count_steps:
        # the one-wave-per-member kernel's debug record: [4] its rounds of 128 bit positions.  Stopped at 4,096 of
        # 65,536 bytes it has not walked the stream to its end.
        zbomb = deflate(bomb, RAW, level=9)
        with _native.DContext(lib=lib) as d:
            d.set_route(_native.INFLATE_WAVE)
            d.debug_inflate(1)
            r = call(lib, d, RAW, zbomb, [0], [len(zbomb)], max_out=4096)
            capped = d.debug_inflate(1)
            r2 = call(lib, d, RAW, zbomb, [0], [len(zbomb)])
            whole = d.debug_inflate(0)
            assert r.status == [E_SPACE] and r2.rows == [(OK, 65536, len(zbomb), 0)]
            assert 0 < capped[4] < whole[4] and capped[5] < whole[5], (capped, whole)


# ------------------------------------------------------------------------------------------------ 7b. debug 2
def debug_two_counts_alike(lib):
    """debug_inflate(2) asks for k_lzcopy's clocks, and a sizes call launches no k_lzcopy: on both routes it answers what
    it answers under debug_inflate(0) -- sizes, in_used, verdicts and the call's own out-values, with and without a cap
    that one member exceeds."""
    plains = [synth.make("text", 999, 2).tobytes(), bytes(1000), synth.make("dna", 400, 3).tobytes(), b""]
    for w, wrap in sorted(WRAPS.items()):
        members = [deflate(p, wrap) for p in plains]
        blob, offs = layout(members)
        sizes = [len(m) for m in members]
        for route, d in contexts(lib):
            got = {}
            for debug in (0, 2):
                d.debug_inflate(debug)
                got[debug] = [call(lib, d, wrap, blob, offs, sizes, max_out=cap) for cap in (0, 999)]
            d.debug_inflate(0)
            check_all_good(got[0][0], plains, members, (w, route, "debug 0"))
            assert got[0][1].status == [OK, E_SPACE, OK, OK] and got[0][1].out_sizes == [999, 0, 400, 0], (w, route)
            for a, b in zip(got[0], got[2]):
                assert (b.out_sizes, b.in_used, b.rows) == (a.out_sizes, a.in_used, a.rows), (w, route, b.rows, a.rows)
                assert (b.rc, b.n_failed, b.block, b.total) == (a.rc, a.n_failed, a.block, a.total) and b.guard_ok, (w, route)


# ------------------------------------------------------------------------------------------------ 8. arguments
def arguments(lib):
    data = synth.make("text", 2500, 9).tobytes()
    for fmt in (_native.FORMAT_BGZF, _native.FORMAT_MGZIP):  # a context made for either format serves
        with _native.DContext(format=fmt, lib=lib) as d:
            for w, wrap in sorted(WRAPS.items()):
                m = deflate(data, wrap)
                r = call(lib, d, wrap, m, [0], [len(m)])
                assert r.rows == [(OK, len(data), len(m), 0)] and r.total == len(data), (fmt, w, r.rows)
            z = deflate(data, ZLIB)
            r = call(lib, d, ZLIB, z, [], [])  # n == 0
            assert r.rc == OK and r.total == 0 and r.n_failed == 0 and r.guard_ok
            r = call(lib, d, ZLIB, z, [0], [len(z)], out_sizes=False)  # NULL d_out_sizes
            assert r.rc == E_ARG and r.total == 0 and r.n_failed == 0 and r.guard_ok and r.in_used == [MARK]
            r = call(lib, d, 3, z, [0], [len(z)])  # unknown wrap
            assert r.rc == E_ARG and r.out_sizes == [MARK]
            r = call(lib, d, ZLIB, z + z[:-1], [0, len(z)], [len(z), len(z) - 1], used=False, results=False)  # NULL optional tables
            assert r.rc == E_BAD and r.block == 1 and r.n_failed == 1 and r.total == len(data) and r.out_sizes == [len(data), 0]
            # the Python face
            mem = scan_cases.Mem(lib)
            keep = [mem.put(z + z[:-1]), mem.put(np.array([0, len(z)], dtype=np.uint64).view(np.uint8)),
                    mem.put(np.array([len(z), len(z) - 1], dtype=np.uint32).view(np.uint8)), mem.empty(8), mem.empty(8)]
            args = (keep[0][1], 2 * len(z) - 1, keep[1][1], keep[2][1])
            assert d.inflate_batch_sizes_device(ZLIB, *args, 1, keep[3][1], keep[4][1]) == (len(data), 0)
            assert np.frombuffer(mem.get(keep[4][0], 4), dtype=np.uint32)[0] == len(z)
            assert d.inflate_batch_sizes_device(ZLIB, *args, 2, keep[3][1], raise_on_member_error=False) == (len(data), 1, 1)
            assert d.inflate_batch_sizes_device(ZLIB, *args, 1, keep[3][1], max_out_size=len(data) - 1,
                                                raise_on_member_error=False) == (0, 1, 0)
            try:
                d.inflate_batch_sizes_device(ZLIB, *args, 2, keep[3][1])
                raise AssertionError("no error for a failing member")
            except _native.GzpxError as e:
                assert (e.code, e.block) == (E_BAD, 1)


# ------------------------------------------------------------------------------------------------ 9. no read past the input
def guard_child(lib_path):
    """(Emulator only: a device pointer is a host pointer.)  The batch lies so that its last byte is the last byte in
    front of a page without access: any load that leaves the aligned words of the input ends the process.  Entries
    exact, then loose -- the last one ends exactly at in_len either way."""
    lib = _native.GzpxLib(lib_path)
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mmap.restype = ctypes.c_void_p
    libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    page = os.sysconf("SC_PAGE_SIZE")
    npages = 4
    base = libc.mmap(None, (npages + 1) * page, 3, 0x22, -1, 0)
    assert base not in (None, ctypes.c_void_p(-1).value)
    assert libc.mprotect(base + npages * page, page, 0) == 0
    plains = [synth.make(c, n, 31).tobytes() for c, n in (("text", 5000), ("random", 300), ("dna", 2000), ("mixed", 3000))]
    for wrap in (RAW, ZLIB, GZIP):
        for last_level in (6, 0):  # the last member ends in a Huffman block / in a stored block
            members = [deflate(p, wrap, level=last_level if i == 3 else 6) for i, p in enumerate(plains)]
            for cut in (0, 1):  # whole; the last member short of its last byte: its stream or trailer runs into the end
                blob = b"".join(members)[:-cut] if cut else b"".join(members)
                assert len(blob) < npages * page
                d_in = base + npages * page - len(blob)
                ctypes.memmove(d_in, blob, len(blob))
                starts = prefix([len(m) for m in members])[:-1]
                offs = np.array(starts, dtype=np.uint64)
                exact = [len(m) for m in members[:3]] + [len(members[3]) - cut]
                for sz in (exact, [len(blob) - o for o in starts]):
                    sizes = np.array(sz, dtype=np.uint32)
                    for route, d in contexts(lib):
                        osz, used = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
                        res = d.inflate_batch_sizes_device(wrap, d_in, len(blob), offs.ctypes.data, sizes.ctypes.data, 4,
                                                           osz.ctypes.data, used.ctypes.data, raise_on_member_error=False)
                        if cut:
                            assert res == (sum(len(p) for p in plains[:3]), 1, 3), (wrap, route, res)
                            assert osz.tolist() == [len(p) for p in plains[:3]] + [0]
                        else:
                            assert res == (sum(len(p) for p in plains), 0, None), (wrap, route, res)
                            assert osz.tolist() == [len(p) for p in plains] and used.tolist() == [len(m) for m in members]
    print("guard ok")


def no_read_past_input(lib):
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import size_cases; size_cases.guard_child(%r)" % (
        here, os.path.dirname(here), lib.path)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "guard ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
