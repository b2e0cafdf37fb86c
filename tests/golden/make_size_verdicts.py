"""Record what the system's libdeflate.so.0 says to the members of tests/size_cases.py when it is asked for sizes:

    python tests/golden/make_size_verdicts.py          (rewrites tests/golden/size_verdicts.json)

Per case: its name, the wrapper, the SHA-256 of the member, the return code (0 ok, 1 BAD_DATA, 3 INSUFFICIENT_SPACE;
own_rc: that of the wrapper's own call on the whole member, which also judges the header and the checksum) and, where
rc is 0, actual_in / actual_out as libdeflate_deflate_decompress_ex / libdeflate_zlib_decompress_ex /
libdeflate_gzip_decompress_ex reported them through both actual_*_ret pointers, with size_cases.ROOM bytes of room.

The size query verifies no checksum, so what is recorded for a wrapped member is the raw call on its payload -- the
bytes behind the wrapper's header -- with the header and the trailer added to actual_in, and BAD_DATA where the
trailer does not fit; wherever the wrapper's own call accepts the member, it has to agree.  For every member recorded
as good, Python's zlib has to agree too -- output length, and len(member) - len(unused_data) for the input -- so the
two yardsticks of the tests cannot differ silently; the crafted streams that zlib refuses outright where libdeflate
accepts (incomplete codes and the like: tests/inflate_cases.py) are marked "zlib": "refuses".  The tests assert against
the file, so they need no libdeflate."""
import ctypes
import hashlib
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def box_libdeflate():
    for path in ("libdeflate.so.0", "/lib/x86_64-linux-gnu/libdeflate.so.0", "/usr/lib/x86_64-linux-gnu/libdeflate.so.0",
                 "/usr/lib64/libdeflate.so.0"):
        try:
            L = ctypes.CDLL(path)
        except OSError:
            continue
        L.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
        calls = []
        for name in ("libdeflate_deflate_decompress_ex", "libdeflate_zlib_decompress_ex", "libdeflate_gzip_decompress_ex"):
            f = getattr(L, name)
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                          ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
            calls.append(f)
        d = L.libdeflate_alloc_decompressor()

        def ask(wrap, data, room):
            out = ctypes.create_string_buffer(max(room, 1))
            a_in, a_out = ctypes.c_size_t(0), ctypes.c_size_t(0)
            rc = calls[wrap](d, bytes(data), len(data), out, room, ctypes.byref(a_in), ctypes.byref(a_out))
            return rc, a_in.value, a_out.value
        return ask
    return None


def gzip_header_len(m):
    """The length of a gzip header whose fields are well formed (the recorded members have no others)."""
    flg, pos = m[3], 10
    if flg & 4:
        pos += 2 + m[pos] + (m[pos + 1] << 8)
    for bit in (8, 16):
        if flg & bit:
            pos = m.index(b"\x00", pos) + 1
    return pos + (2 if flg & 2 else 0)


def main():
    import size_cases
    from size_cases import GZIP, RAW, ROOM, TRAILER, ZLIB
    ask = box_libdeflate()
    if ask is None:
        sys.exit("no libdeflate.so.0 on this box")
    rows = []
    for name, wrap, m in size_cases.recorded_cases():
        hdr = 0 if wrap == RAW else 2 if wrap == ZLIB else gzip_header_len(m)
        own = ask(wrap, m, ROOM)
        rc, a_in, a_out = ask(RAW, m[hdr:], ROOM)
        if rc == 0:
            a_in += hdr + TRAILER[wrap]
            if a_in > len(m):
                rc = 1
        if own[0] == 0:
            assert (rc, a_in, a_out) == own, (name, own, (rc, a_in, a_out))
        elif wrap == RAW:
            assert own[0] == rc, (name, own, rc)
        row = {"case": name, "wrap": wrap, "sha256": hashlib.sha256(m).hexdigest(), "rc": rc, "own_rc": own[0]}
        if rc == 0:
            row["actual_in"], row["actual_out"] = a_in, a_out
            try:
                do = zlib.decompressobj(-15)
                out = do.decompress(m[hdr:])
                assert do.eof and len(out) == a_out and hdr + len(m[hdr:]) - len(do.unused_data) + TRAILER[wrap] == a_in, name
            except zlib.error:  # (only a crafted stream may be libdeflate's alone: the codes zlib refuses as a matter of policy)
                assert name.startswith("crafted "), name
                row["zlib"] = "refuses"
        rows.append(row)
    assert len({r["case"] for r in rows}) == len(rows)
    with open(size_cases.VERDICTS, "w") as f:
        f.write(json.dumps({"reference": "libdeflate_{deflate,zlib,gzip}_decompress_ex of libdeflate.so.0 (v1.10 behaviour), "
                                         "%d bytes of room" % ROOM, "verdicts": rows}, indent=1, sort_keys=True) + "\n")
    print("wrote %s (%d cases, %d good)" % (size_cases.VERDICTS, len(rows), sum(1 for r in rows if r["rc"] == 0)))


if __name__ == "__main__":
    main()
