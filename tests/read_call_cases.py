"""The host-side work of the decode half's calls on device-resident data (gzpx_api.cpp: index, ranges, lines, find,
batch, sizes, checksums), as the CPU emulator counts it: hipEventRecord calls, stream synchronisations and allocations
of every call of one fixed script, next to its return code and everything it hands back.  The kernels decide the bytes;
this table pins what the host puts around them, so that a reorganisation of the host code that moves, adds or drops an
event, a round trip or a buffer shows as a changed row whatever the bytes say.

One BGZF stream of six members (five of 20,000 bytes and one of 100), batches of 45,000 inflated bytes: two members a
batch, three batches.  The calls go through the C ABI itself (not the Python wrappers, which raise): the out-values of
the failing paths are part of the row.  Emulator only: the pointers are host arrays."""
import ctypes
import functools
import os
import sys
import zlib

import numpy as np

if __name__ == "__main__":  # (run as a script: the package lies one directory up)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from gzp_amd import _native, synth

BS = 20000
N = 5 * BS + 100
BATCH = 45000
PATTERN = b"weees"
VICTIM = 3  # the damaged member: the second of the second batch
UNSET = (777, 0x11, 0x22)  # gzpx_check_info as the script hands it in: a row that shows it was not written


@functools.lru_cache(maxsize=None)
def stream(oracle):
    """(text, six members of it without the EOF marker, the same with member VICTIM's CRC damaged)."""
    text = synth.make("text", N, 7).tobytes()
    s = bytes(oracle.compress_stream(np.frombuffer(text, dtype=np.uint8), oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, BS))[:-28]
    bad = bytearray(s)
    pos = 0
    for _ in range(VICTIM + 1):
        pos += (bad[pos + 16] | (bad[pos + 17] << 8)) + 1
    bad[pos - 8] ^= 0x40
    return text, s, bytes(bad)


def _dev(a):
    a = np.ascontiguousarray(a)
    return a, a.ctypes.data


def _crc(a, n=None):
    return zlib.crc32(np.ascontiguousarray(a).view(np.uint8)[:n].tobytes())


def run(lib, oracle):
    """The script: [(call, row)], row = return code, out-values ..., (event records, stream syncs, allocations)."""
    L = lib.L
    for f in (L.emu_event_record_count, L.emu_stream_sync_count, L.emu_fail_nth_alloc):
        f.restype = ctypes.c_long
    L.emu_fail_nth_alloc.argtypes = [ctypes.c_long]
    text, s, s_bad = stream(oracle)
    rows = []
    sz, u64 = ctypes.c_size_t, ctypes.c_uint64
    none = sz(-1).value

    def counted(name, call):
        ev, sy = L.emu_event_record_count(), L.emu_stream_sync_count()
        L.emu_fail_nth_alloc(10 ** 6)
        try:
            out = call()
        finally:
            allocs = 10 ** 6 - L.emu_fail_nth_alloc(0)
        rows.append((name, tuple(out) + ((L.emu_event_record_count() - ev, L.emu_stream_sync_count() - sy, allocs),)))

    def info_of(info):
        return (info.block, info.found, info.expected)

    def fresh_info():
        return _native.GzpxCheckInfo(*UNSET)

    k_in, p_in = _dev(np.frombuffer(s, dtype=np.uint8))
    k_bad, p_bad = _dev(np.frombuffer(s_bad, dtype=np.uint8))
    with _native.DContext(format=_native.FORMAT_BGZF, lib=lib) as d:
        d.set_lines_batch(BATCH)
        h_ix = ctypes.c_void_p()

        def index():
            n, used, total = sz(0), sz(0), u64(0)
            rc = L.gzpx_dindex_build_device(d.h, p_in, len(s), ctypes.byref(h_ix), ctypes.byref(n), ctypes.byref(used),
                                            ctypes.byref(total), None)
            return rc, n.value, used.value, total.value
        counted("index build", index)
        try:
            def ranges(r, p_stream=p_in, short=0):
                r = np.asarray(r, dtype=np.uint64).reshape(-1, 2)
                want = sum(int(e) - int(b) for b, e in r if b <= e <= N)
                out, p_out = _dev(np.full(N + 64, 0xEE, dtype=np.uint8))
                offs = np.full(r.shape[0] + 1, 0xABABABAB, dtype=np.uint64)
                out_len, bad, info = sz(123), sz(123), fresh_info()
                rc = L.gzpx_read_ranges_device(d.h, h_ix, p_stream, len(s), r.ctypes.data, r.shape[0], _native.RANGE_UNCOMPRESSED,
                                               p_out, want - short, ctypes.byref(out_len), offs.ctypes.data, ctypes.byref(bad),
                                               ctypes.byref(info), None)
                if rc == _native.OK:
                    assert out[:out_len.value].tobytes() == b"".join(text[int(b):int(e)] for b, e in r)
                return (rc, out_len.value, bad.value == none or bad.value, _crc(offs), _crc(out), info_of(info),
                        d.last_ranges_members())
            one = [(N // 2, N // 2 + 777)]
            many = [((i * 7919) % (N - 100), (i * 7919) % (N - 100) + 100) for i in range(200)]
            counted("ranges: one", lambda: ranges(one))
            counted("ranges: 200", lambda: ranges(many))
            counted("ranges: empty only", lambda: ranges([(5, 5), (N, N), (70000, 70000)]))
            counted("ranges: bad range", lambda: ranges([(5, 9), (N - 1, N + 1), (9, 5)]))
            counted("ranges: one byte short", lambda: ranges(many, short=1))
            counted("ranges: damaged member", lambda: ranges([(10, 20), (VICTIM * BS + 5, VICTIM * BS + 50), (N - 10, N)], p_bad))

            h_lt = ctypes.c_void_p()

            def build(p_stream, h):
                nd, nl, info = u64(123), u64(123), fresh_info()
                rc = L.gzpx_dlines_build_device(d.h, h_ix, p_stream, len(s), 10, ctypes.byref(h), ctypes.byref(nd), ctypes.byref(nl),
                                                ctypes.byref(info), None)
                return (rc, bool(h.value), nd.value, nl.value, info_of(info), d.last_lines_build_ms() >= (0.0, 0.0))
            counted("lines build", lambda: build(p_in, h_lt))
            try:
                assert rows[-1][1][2] == text.count(b"\n")
                counted("lines build: damaged member", lambda: build(p_bad, ctypes.c_void_p()))
                starts = [0] + [i + 1 for i, ch in enumerate(text) if ch == 10]

                def offsets(ks):
                    k = np.asarray(ks, dtype=np.uint64)
                    offs = np.full(k.size, 0xABABABAB, dtype=np.uint64)
                    bad, info = sz(123), fresh_info()
                    rc = L.gzpx_line_offsets_device(d.h, h_ix, h_lt, p_in, len(s), k.ctypes.data, k.size, offs.ctypes.data,
                                                    ctypes.byref(bad), ctypes.byref(info), None)
                    if rc == _native.OK:
                        assert offs.tolist() == [starts[i] for i in ks]
                    return rc, bad.value == none or bad.value, _crc(offs), info_of(info), d.last_lines_members()
                counted("line offsets", lambda: offsets([0, 3, 400, 401, 848]))

                def lines(r, p_stream=p_in, short=0):
                    r = np.asarray(r, dtype=np.uint64).reshape(-1, 2)
                    want = b"".join(text[starts[a]:starts[b]] for a, b in r.tolist())
                    out, p_out = _dev(np.full(N + 64, 0xEE, dtype=np.uint8))
                    offs = np.full(r.shape[0] + 1, 0xABABABAB, dtype=np.uint64)
                    br = np.full((r.shape[0], 2), 0xABABABAB, dtype=np.uint64)
                    out_len, bad, info = sz(123), sz(123), fresh_info()
                    rc = L.gzpx_read_lines_device(d.h, h_ix, h_lt, p_stream, len(s), r.ctypes.data, r.shape[0], p_out,
                                                  len(want) - short, ctypes.byref(out_len), offs.ctypes.data, br.ctypes.data,
                                                  ctypes.byref(bad), ctypes.byref(info), None)
                    if rc == _native.OK:
                        assert out[:out_len.value].tobytes() == want
                    return (rc, out_len.value, bad.value == none or bad.value, _crc(offs), _crc(br), _crc(out), info_of(info),
                            d.last_lines_members())
                some = [(0, 2), (400, 405), (7, 7), (840, 849)]
                counted("read lines", lambda: lines(some))
                counted("read lines: one byte short", lambda: lines(some, short=1))
                counted("read lines: damaged member", lambda: lines([(0, 2), (500, 600)], p_bad))
            finally:
                L.gzpx_dlines_destroy(h_lt)

            def find(positions, with_lines, cap, p_stream=p_in):
                pos, p_pos = _dev(np.full(max(cap, 1), 0xABABABAB, dtype=np.uint64))
                lns, p_lns = _dev(np.full(max(cap, 1), 0xABABABAB, dtype=np.uint64))
                n, info = u64(123), fresh_info()
                rc = L.gzpx_find_device(d.h, h_ix, p_stream, len(s), PATTERN, len(PATTERN), 10 if with_lines else _native.FIND_NO_LINES,
                                        p_pos if positions else None, p_lns if with_lines else None, cap, ctypes.byref(n),
                                        ctypes.byref(info), None)
                return rc, n.value, _crc(pos), _crc(lns), info_of(info), d.last_find_ms() >= (0.0, 0.0, 0.0)
            hits = text.count(PATTERN)
            counted("find: count only", lambda: find(False, False, 0))
            assert rows[-1][1][1] == hits
            counted("find: positions + lines", lambda: find(True, True, hits))
            counted("find: hits_cap too small", lambda: find(True, True, hits - 3))
            counted("find: damaged member", lambda: find(True, True, hits, p_bad))
        finally:
            L.gzpx_dindex_destroy(h_ix)

        parts = [text[:5000], b"", text[5000:45000]]
        zs = [zlib.compress(p, 6) for p in parts]
        k_z, p_z = _dev(np.frombuffer(b"".join(zs), dtype=np.uint8))
        k_off, p_off = _dev(np.cumsum([0] + [len(z) for z in zs[:-1]]).astype(np.uint64))
        k_sz, p_sz = _dev(np.array([len(z) for z in zs], dtype=np.uint32))
        k_osz, p_osz = _dev(np.array([len(p) for p in parts], dtype=np.uint32))
        n_z = sum(len(z) for z in zs)

        def batch():
            out, p_out = _dev(np.full(45000 + 64, 0xEE, dtype=np.uint8))
            out_len, n_failed, info = sz(123), sz(123), fresh_info()
            rc = L.gzpx_inflate_batch_device(d.h, _native.WRAP_ZLIB, 0, p_z, n_z, p_off, p_sz, p_osz, 3, p_out, 45000, None, None,
                                             ctypes.byref(out_len), ctypes.byref(n_failed), ctypes.byref(info), None)
            assert out[:45000].tobytes() == b"".join(parts)
            return rc, out_len.value, n_failed.value, info_of(info)
        counted("inflate batch", batch)

        def sizes():
            got, p_got = _dev(np.zeros(3, dtype=np.uint32))
            total, n_failed, info = u64(123), sz(123), fresh_info()
            rc = L.gzpx_inflate_batch_sizes_device(d.h, _native.WRAP_ZLIB, p_z, n_z, p_off, p_sz, 3, 0, p_got, None, None,
                                                   ctypes.byref(total), ctypes.byref(n_failed), ctypes.byref(info), None)
            return rc, total.value, n_failed.value, got.tolist(), info_of(info)
        counted("inflate batch sizes", sizes)

        def checksums(expected):
            sums, p_sums = _dev(np.zeros(3, dtype=np.uint32))
            k_exp, p_exp = _dev(np.array(expected, dtype=np.uint32))
            k_po, p_po = _dev(np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64))
            k_t, p_t = _dev(np.frombuffer(b"".join(parts), dtype=np.uint8))
            n_failed, info = sz(123), fresh_info()
            rc = L.gzpx_checksum_batch_device(d.h, _native.CHECK_ADLER32, p_t, 45000, p_po, None, 3, None, p_exp, p_sums, None,
                                              ctypes.byref(n_failed), ctypes.byref(info), None)
            return rc, n_failed.value, sums.tolist() == [zlib.adler32(p) for p in parts], info_of(info)
        adlers = [zlib.adler32(p) for p in parts]
        counted("checksum batch", lambda: checksums(adlers))
        counted("checksum batch: one wrong", lambda: checksums([adlers[0], adlers[1], adlers[2] ^ 1]))
    return rows


if __name__ == "__main__":  # python tests/read_call_cases.py prints the emulator's table
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    from oracle import oracle as o
    o.build()
    for name, row in run(_native.GzpxLib(build_emu.build()), o):
        print('    ("%s", %r),' % (name, row))
